#!/usr/bin/env python3
"""Generate zecale_amd/csrc/bw6_params.h: field constants for BW6-761 Fq / Fr in the
two limb forms the product uses:
  * device form: 29-bit limbs in u32 (NL = 27 for Fq, 14 for Fr), Montgomery radix 2^(29*NL)
  * host/ABI form: 64-bit limbs (12 / 6), Montgomery radix 2^768 / 2^384 (libff in-memory form)
Moduli and generators: reference client/test_commands/test_bw6_761_groth16_contract.py:26-35.
Run:  python tools/gen_params.py > zecale_amd/csrc/bw6_params.h
"""
Q = 0x0122e824fb83ce0ad187c94004faff3eb926186a81d14688528275ef8087be41707ba638e584e91903cebaff25b423048689c8ed12f9fd9071dcd3dc73ebff2e98a116c25667a8f8160cf8aeeaf0a437e6913e6870000082f49d00000000008b
R = 0x01ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001
G1 = (0x01075b020ea190c8b277ce98a477beaee6a0cfb7551b27f0ee05c54b85f56fc779017ffac15520ac11dbfcd294c2e746a17a54ce47729b905bd71fa0c9ea097103758f9a280ca27f6750dd0356133e82055928aca6af603f4088f3af66e5b43d,
      0x0058b84e0a6fc574e6fd637b45cc2a420f952589884c9ec61a7348d2a2e573a3265909f1af7e0dbac5b8fa1771b5b806cc685d31717a4c55be3fb90b6fc2cdd49f9df141b3053253b2b08119cad0fb93ad1cb2be0b20d2a1bafc8f2db4e95363)
G2 = (0x0110133241d9b816c852a82e69d660f9d61053aac5a7115f4c06201013890f6d26b41c5dab3da268734ec3f1f09feb58c5bbcae9ac70e7c7963317a300e1b6bace6948cb3cd208d700e96efbc2ad54b06410cf4fe1bf995ba830c194cd025f1c,
      0x0017c3357761369f8179eb10e4b6d2dc26b7cf9acec2181c81a78e2753ffe3160a1d86c80b95a59c94c97eb733293fef64f293dbd2c712b88906c170ffa823003ea96fcd504affc758aa2d3a3c5a02a591ec0594f9eac689eb70a16728c73b61)
FR_GEN = 15
B = 29
MASK = (1 << B) - 1


def limbs(x, n, bits):
    out = []
    for _ in range(n):
        out.append(x & ((1 << bits) - 1))
        x >>= bits
    assert x == 0
    return out


def arr(name, vals, ty="uint32_t", per=6, fmt="0x%08xu"):
    s = "  static constexpr %s %s[%d] = {\n" % (ty, name, len(vals))
    for i in range(0, len(vals), per):
        s += "      " + ", ".join(fmt % v for v in vals[i:i + per]) + ",\n"
    return s + "  };\n"


def sub_safe_multiple(p, k, nl):
    """k*p written with limbs d_i such that every limb except the top is in [2^29, 2^30)
    (so a_i + d_i - b_i >= 0 for normalised a_i, b_i < 2^29) and sum d_i 2^(29 i) = k*p."""
    v = limbs(k * p, nl, B)
    d = list(v)
    # borrow 1 from limb i+1 to give 2^29 to limb i
    for i in range(nl - 1):
        d[i] += 1 << B
        d[i + 1] -= 1
    assert all(x >= MASK for x in d[:-1]) and d[-1] >= 0, d
    assert sum(x << (B * i) for i, x in enumerate(d)) == k * p
    return d


def field(name, p, nl, n64, extra=""):
    Rdev = 1 << (B * nl)
    Rabi = 1 << (64 * n64)
    assert Rdev > (p << 10), "need >= 10 spare bits for lazy reduction"
    pinv = (-pow(p, -1, 1 << B)) % (1 << B)
    pinv64 = (-pow(p, -1, 1 << 64)) % (1 << 64)
    s = "struct %s {\n" % name
    s += "  static constexpr int NL = %d;      // 29-bit limbs (device form)\n" % nl
    s += "  static constexpr int N64 = %d;     // 64-bit limbs (ABI / host form)\n" % n64
    s += "  static constexpr int NBITS = %d;\n" % p.bit_length()
    s += "  static constexpr uint32_t PINV = 0x%08xu;   // -p^-1 mod 2^29\n" % pinv
    s += "  static constexpr uint64_t PINV64 = 0x%016xull;   // -p^-1 mod 2^64\n" % pinv64
    s += arr("P", limbs(p, nl, B))
    s += arr("ONE", limbs(Rdev % p, nl, B))               # 1 in device Montgomery form
    s += arr("R2", limbs(Rdev * Rdev % p, nl, B))         # canonical -> device form
    # ABI(x*Rabi) -> device(x*Rdev): montmul by Rdev^2/Rabi ; device -> ABI: montmul by Rabi
    s += arr("ABI2DEV", limbs(Rdev * Rdev * pow(Rabi, -1, p) % p, nl, B))
    s += arr("DEV2ABI", limbs(Rabi % p, nl, B))
    for k in (2, 4, 8, 16):
        s += arr("SUBK%d" % k, sub_safe_multiple(p, k, nl))
    n32 = (p.bit_length() + 31) // 32
    s += "  static constexpr int N32 = %d;     // packed 32-bit words of a canonical-size value\n" % n32
    s += arr("P64", limbs(p, n64, 64), "uint64_t", 3, "0x%016xull")
    s += arr("ONE64", limbs(Rabi % p, n64, 64), "uint64_t", 3, "0x%016xull")
    s += arr("R2_64", limbs(Rabi * Rabi % p, n64, 64), "uint64_t", 3, "0x%016xull")
    s += extra
    s += "};\n\n"
    return s


def edwards_params():
    """The twisted Edwards curve (a = -1) that G1's curve y^2 = x^3 - 1 is 2-isogenous to.
    With X = x - 1 the curve is y^2 = X (X^2 + 3X + 3); Velu's quotient by (0, 0) is E': Y^2 = X (X^2 - 6X - 3); -3 = s^2 is a square, so
    u = X'/s, v = Y'/s^2 is the Montgomery curve s v^2 = u^3 + A u^2 + u, A = -6/s; then a_E = (A + 2)/s, d_E = (A - 2)/s, and with
    t^2 = -a_E, x_e = t u / v, y_e = (u - 1)/(u + 1) lands on -x_e^2 + y_e^2 = 1 + d x_e^2 y_e^2, d = -d_E / a_E.
    chi: G1 -> Edwards, written out:  x_e = t s y / (3 - X^2),  y_e = (y^2 - s X^2) / (y^2 + s X^2).
    psi: Edwards -> G1 (the dual isogeny after the inverse maps), psi(chi(P)) = 2P:  x = 1 + c1 / x_e^2,  y = c2 y_e / (x_e (1 - y_e^2)),
    c1 = -3 t^2 / 4, c2 = 3 t / 2."""
    q = Q
    inv = lambda a: pow(a % q, q - 2, q)
    s = pow(-3 % q, (q + 1) // 4, q)          # q = 3 mod 4: the principal square root
    assert s * s % q == q - 3
    A = -6 * inv(s) % q
    aE = (A + 2) * inv(s) % q
    dE = (A - 2) * inv(s) % q
    t = pow(-aE % q, (q + 1) // 4, q)
    assert t * t % q == -aE % q
    d = -dE * inv(aE) % q
    assert pow(d, (q - 1) // 2, q) == 1       # d is a square: the formulas are complete only on the odd-order part
    return {"s": s, "A": A, "t": t, "d": d, "c1": -3 * t * t * inv(4) % q, "c2": 3 * t * inv(2) % q, "half_r": pow(2, -1, R)}


def main():
    out = "// GENERATED by tools/gen_params.py - do not edit.\n"
    out += "// BW6-761 field constants (moduli: reference client/test_commands/test_bw6_761_groth16_contract.py:26-27).\n"
    out += "#pragma once\n#include <stdint.h>\n\nnamespace zkhip {\n\n"
    Rabi_q = 1 << 768
    extra_q = arr("G1_GEN_X64", limbs(G1[0] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    extra_q += arr("G1_GEN_Y64", limbs(G1[1] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    extra_q += arr("G2_GEN_X64", limbs(G2[0] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    extra_q += arr("G2_GEN_Y64", limbs(G2[1] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    fe = (Q ** 6 - 1) // R            # Tate pairing final exponent (q^6 - 1) / r
    assert (Q ** 6 - 1) % R == 0
    nfe = (fe.bit_length() + 63) // 64
    extra_q += "  static constexpr int FINAL_EXP_LIMBS = %d;\n" % nfe
    extra_q += arr("FINAL_EXP", limbs(fe, nfe, 64), "uint64_t", 3, "0x%016xull")
    extra_q += arr("R_ORDER64", limbs(R, 6, 64), "uint64_t", 3, "0x%016xull")
    # G1's 2-isogenous twisted Edwards curve (edwards_params; ec_edw.cuh), device Montgomery form
    ep = edwards_params()
    mont = lambda v: limbs(v * (1 << (B * 27)) % Q, 27, B)
    extra_q += arr("EDW_D2", mont(2 * ep["d"]))                     # 2d
    extra_q += arr("EDW_S", mont(ep["s"]))                          # s = sqrt(-3)
    extra_q += arr("EDW_TS", mont(ep["t"] * ep["s"]))               # t s
    extra_q += arr("EDW_C1", mont(ep["c1"]))                        # -3 t^2 / 4
    extra_q += arr("EDW_C2", mont(ep["c2"]))                        # 3 t / 2
    extra_q += arr("EDW_THREE", mont(3))
    extra_q += arr("EDW_DINV", mont(pow(ep["d"], -1, Q)))           # 1 / d: a bucket opened from a table point, T = (2 d x y) / d
    # psi's constants once more in the host's form: the window result of an Edwards launch is mapped back on the host (msm.hip edw_abi_to_jac)
    extra_q += arr("EDW_C1_64", limbs(ep["c1"] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    extra_q += arr("EDW_C2_64", limbs(ep["c2"] * Rabi_q % Q, 12, 64), "uint64_t", 3, "0x%016xull")
    out += field("FqParams", Q, 27, 12, extra_q)
    Rabi_r = 1 << 384
    two_adic = pow(FR_GEN, (R - 1) >> 46, R)
    assert pow(two_adic, 1 << 45, R) == R - 1
    extra_r = "  static constexpr int TWO_ADICITY = 46;\n"
    extra_r += arr("GEN64", limbs(FR_GEN * Rabi_r % R, 6, 64), "uint64_t", 3, "0x%016xull")
    extra_r += arr("ROOT_2_46_64", limbs(two_adic * Rabi_r % R, 6, 64), "uint64_t", 3, "0x%016xull")
    # 1/2 mod r = (r + 1) / 2 as an integer in 29-bit limbs: the scalar that halves the bases of an Edwards table (msm.hip k_half_bases)
    extra_r += arr("HALF_RAW", limbs(pow(2, -1, R), 14, B))
    out += field("FrParams", R, 14, 6, extra_r)
    out += "}  // namespace zkhip\n"
    print(out, end="")


if __name__ == "__main__":
    main()
