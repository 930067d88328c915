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


def _ec_mul(k, P):
    """k P on y^2 = x^3 - 1 over Fq, affine (None: the point at infinity): only to tell the two endomorphism eigenvalues apart"""
    def add(A, Bp):
        if A is None:
            return Bp
        if Bp is None:
            return A
        if A[0] == Bp[0]:
            if (A[1] + Bp[1]) % Q == 0:
                return None
            l = 3 * A[0] * A[0] * pow(2 * A[1], -1, Q) % Q
        else:
            l = (Bp[1] - A[1]) * pow(Bp[0] - A[0], -1, Q) % Q
        x = (l * l - A[0] - Bp[0]) % Q
        return (x, (l * (A[0] - x) - A[1]) % Q)
    acc = None
    for bit in bin(k)[2:]:
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, P)
    return acc


def glv_params(t_bits=576):
    """G1 is y^2 = x^3 - 1 (j = 0) and q = r = 1 mod 3: phi(x, y) = (omega x, y), omega^3 = 1 in Fq, acts on G1 as a cube root of unity
    lambda in Fr.  Of the two omega and two lambda the pair with phi(G1_GEN) = lambda G1_GEN is taken.  The decomposition
    k = k1 + k2 lambda (mod r) with |k1|, |k2| < 2^bits: v1 = (a1, b1), v2 = (a2, b2) is a reduced basis of the lattice
    {(a, b): a + b lambda = 0 mod r} from the extended Euclidean algorithm on (r, lambda); (k1, k2) = (k, 0) - c1 v1 - c2 v2 with
    c1 = round(k b2 / det), c2 = round(-k b1 / det), the quotients as floor((k g_i + 2^(t-1)) / 2^t), g_i = round(2^t |.| / r)."""
    assert Q % 3 == 1 and R % 3 == 1
    g = 2
    while pow(g, (Q - 1) // 3, Q) == 1:
        g += 1
    omegas = [pow(g, (Q - 1) // 3, Q)]
    omegas.append(omegas[0] * omegas[0] % Q)
    g = 2
    while pow(g, (R - 1) // 3, R) == 1:
        g += 1
    lam = pow(g, (R - 1) // 3, R)
    lams = [lam, lam * lam % R]
    pair = [(w, l) for w in omegas for l in lams if _ec_mul(l, G1) == (w * G1[0] % Q, G1[1])]
    omega, lam = min(pair)                       # (both omegas have their lambda: the smaller omega, for a fixed choice)
    assert (lam * lam + lam + 1) % R == 0 and pow(omega, 3, Q) == 1 and omega != 1
    # extended Euclid on (r, lambda): remainders r_i = s_i r + t_i lambda, so (r_i, -t_i) is in the lattice
    rs, ts = [R, lam], [0, 1]
    while rs[-1] * rs[-1] >= R:
        qt = rs[-2] // rs[-1]
        rs.append(rs[-2] - qt * rs[-1]); ts.append(ts[-2] - qt * ts[-1])
    qt = rs[-2] // rs[-1]
    rs.append(rs[-2] - qt * rs[-1]); ts.append(ts[-2] - qt * ts[-1])
    v1 = (rs[-2], -ts[-2])
    cands = [(rs[-3], -ts[-3]), (rs[-1], -ts[-1])]
    v2 = min(cands, key=lambda v: v[0] * v[0] + v[1] * v[1])
    for a, b in (v1, v2):
        assert (a + b * lam) % R == 0
    det = v1[0] * v2[1] - v2[0] * v1[1]
    assert abs(det) == R
    sgn = 1 if det > 0 else -1
    n1, n2 = sgn * v2[1], -sgn * v1[1]           # c1 = round(k n1 / r), c2 = round(k n2 / r)
    rnd = lambda n: ((abs(n) << t_bits) + R // 2) // R
    # |k_i| <= (|a1| + |a2|) / 2 resp. (|b1| + |b2|) / 2 for exact rounding; the truncated quotients are off by at most one each
    bound = max(abs(v1[0]) + abs(v2[0]), abs(v1[1]) + abs(v2[1])) * 3 // 2 + 2
    bits = bound.bit_length()
    assert bits <= 192
    return dict(omega=omega, omega2=omega * omega % Q, lam=lam, v1=v1, v2=v2, n=(n1, n2), g=(rnd(n1), rnd(n2)), t=t_bits, bits=bits)


def glv_decompose(k, gp):
    """the host's decomposition (csrc/phase2.cuh phase2_glv_decompose), in Python: the generator checks it on a few thousand scalars"""
    c = [((k * g + (1 << (gp["t"] - 1))) >> gp["t"]) * (1 if n > 0 else -1) for g, n in zip(gp["g"], gp["n"])]
    k1 = k - c[0] * gp["v1"][0] - c[1] * gp["v2"][0]
    k2 = -c[0] * gp["v1"][1] - c[1] * gp["v2"][1]
    return k1, k2


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
    # the endomorphism phi(x, y) = (omega x, y) of G1 and the decomposition of a scalar along it (glv_params; phase2.cuh)
    gp = glv_params()
    import random
    rng = random.Random(1)
    for k in [0, 1, 2, R - 1, gp["lam"], R - gp["lam"], (R + 1) // 2] + [rng.randrange(R) for _ in range(2000)]:
        k1, k2 = glv_decompose(k, gp)
        assert (k1 + k2 * gp["lam"] - k) % R == 0 and abs(k1) < 1 << gp["bits"] and abs(k2) < 1 << gp["bits"], k
    extra_q += arr("GLV_OMEGA", mont(gp["omega"]))                  # phi(x, y) = (omega x, y) = lambda (x, y) on G1
    extra_q += arr("GLV_OMEGA2", mont(gp["omega2"]))                # omega^2 = 1 / omega: back from omega x to x
    out += field("FqParams", Q, 27, 12, extra_q)
    Rabi_r = 1 << 384
    two_adic = pow(FR_GEN, (R - 1) >> 46, R)
    assert pow(two_adic, 1 << 45, R) == R - 1
    extra_r = "  static constexpr int TWO_ADICITY = 46;\n"
    extra_r += arr("GEN64", limbs(FR_GEN * Rabi_r % R, 6, 64), "uint64_t", 3, "0x%016xull")
    extra_r += arr("ROOT_2_46_64", limbs(two_adic * Rabi_r % R, 6, 64), "uint64_t", 3, "0x%016xull")
    # 1/2 mod r = (r + 1) / 2 as an integer in 29-bit limbs: the scalar that halves the bases of an Edwards table (msm.hip k_half_bases)
    extra_r += arr("HALF_RAW", limbs(pow(2, -1, R), 14, B))
    u64 = lambda name, v, n: arr(name, limbs(v, n, 64), "uint64_t", 3, "0x%016xull")
    extra_r += u64("GLV_LAMBDA64", gp["lam"], 6)                    # canonical (not Montgomery)
    extra_r += "  static constexpr int GLV_BITS = %d;      // |k1|, |k2| < 2^GLV_BITS\n" % gp["bits"]
    extra_r += "  static constexpr int GLV_SHIFT = %d;     // c_i = (k GLV_G_i + 2^(GLV_SHIFT - 1)) >> GLV_SHIFT\n" % gp["t"]
    extra_r += u64("GLV_G1_64", gp["g"][0], 9) + u64("GLV_G2_64", gp["g"][1], 9)
    # magnitudes of the basis (a1, b1), (a2, b2); GLV_SIGNS bit j set: term j of (c1 a1, c2 a2, c1 b1, c2 b2) is NEGATIVE, the sign of
    # c_i included, so that k1 = k - (+-)c1 |a1| - (+-)c2 |a2| and k2 = -(+-)c1 |b1| - (+-)c2 |b2| with c_i >= 0
    (a1, b1), (a2, b2) = gp["v1"], gp["v2"]
    sg = lambda n: 1 if n > 0 else -1
    terms = (sg(gp["n"][0]) * a1, sg(gp["n"][1]) * a2, sg(gp["n"][0]) * b1, sg(gp["n"][1]) * b2)
    extra_r += u64("GLV_A1_64", abs(a1), 3) + u64("GLV_A2_64", abs(a2), 3) + u64("GLV_B1_64", abs(b1), 3) + u64("GLV_B2_64", abs(b2), 3)
    extra_r += "  static constexpr int GLV_SIGNS = %d;\n" % sum(1 << j for j, v in enumerate(terms) if v < 0)
    out += field("FrParams", R, 14, 6, extra_r)
    out += "}  // namespace zkhip\n"
    print(out, end="")


if __name__ == "__main__":
    main()
