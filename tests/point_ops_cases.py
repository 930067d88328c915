"""Cases and exact expectations for the point layer of zecale_amd/csrc/ec.cuh, ec_mem.cuh and ec_edw.cuh on RAW limbs (test-side
helpers, no GPU needed to build them).  One generator and one checker serve the g++ build of the five register forms
(tests/test_point_ops_host.py) and the device build (tests/test_point_ops_gpu.py, through zkhip_internal_point_ops_selftest);
tests/test_point_ops_cases.py checks the generator itself.

A case is a group-level SITUATION (which points A and B are: unrelated, equal, opposite, infinite, empty, the identity, the 2-torsion
point (1, 0) of G1, the point (0, 2) of G2's curve) and a REPRESENTATIVE for every coordinate: the residue is scaled by a non-zero
lambda^2 / lambda^3 (a common Z for the Edwards forms) and lifted to v + j p with j at both ends of the coordinate's lazy bound [k].
lambda is also CHOSEN so that one coordinate's residue lies within a few units of 0 or of p: with j = 0 or k - 1 the integer then sits
next to 0 or next to k p, where a too-small lend of an fp_sub<K> or a value past a packing's range shows.  A coordinate = 0 (mod p) is
given as zero limbs and as a non-zero multiple of p; ZZ = 0 of every infinite operand as 0 and as p.

Coordinates are in the device's Montgomery form (v = value * 2^783 mod p).  The formulas are homogeneous, so the checks work on the raw
numbers: X = x ZZ, Y = y ZZZ, ZZ^3 = ZZZ^2 R (XYZZ);  X = x_e Z, Y = y_e Z, T Z = X Y (Edwards).

Contracts, from the comments of the three headers: stored XYZZ points X [10], Y <= 4p (closed: xyzz_neg of Y = 0 gives exactly 4p), ZZ
[2], ZZZ [2]; register affine operands [2]; packed words canonical; an X that goes through lds_st_packed below 2^768; Edwards
coordinates [2].  precondition() ASSERTS them on every case: a case that breaks one is an error of this file, never skipped.

The cases of an op come in waves of 64 lanes (16 cases for the quad forms, four lanes each): fp_is_zero_2p_rare votes over the wave
and the rolled loops are left on the same-x flag, so there is a wave without a same-x lane, one where every lane is same-x, waves
with exactly one (first, middle, last lane), and a wave where only some take the same-x or the copy path (WAVES below)."""
import functools
import random
from types import SimpleNamespace

from oracle import pyref as R
from tests import field_ops_cases as FC
from tests import test_edwards_model as EM

F = FC.FQ
p = F.p
RM = F.Rdev % p                      # the Montgomery factor 2^783 mod p: fp_one()
ROW_IN, ROW_OUT = 224, 217
N_MIN = 300
T2 = (1, 0)                          # the 2-torsion point of G1 that generates chi's kernel
X0 = (0, 2)                          # x = 0 on G2's curve y^2 = x^3 + 4
OMEGA = next(w for w in (pow(g, (p - 1) // 3, p) for g in range(2, 50)) if w != 1)      # (OMEGA, 0), (OMEGA^2, 0): G1's other 2-torsion
KB = (10, 4, 2, 2)                   # [k] of X, Y, ZZ, ZZZ of a stored point (Y: closed)
SEED = 0x90171


def _op(code, kind, **kw):
    d = dict(code=code, kind=kind, quad=False, refs=False, lds=False, packed=False, a_inf=True, b_inf=True, y_mul2=False, flag=False)
    d.update(kw)
    return SimpleNamespace(**d)


# refs: takes an XyzzRef (runs with mem 0 and 1); lds: the accumulator's X comes back as 24 packed words; packed: B is an AffPacked /
# EdwPacked; a_inf / b_inf: the operand may be infinite (Edwards: empty); y_mul2: Y3 is an fp_mul2 output [2]; flag: returns a bool
OPS = {
    "xyzz_dbl_affine": _op(0, "dbl_affine"),
    "xyzz_dbl": _op(1, "dbl"),
    "xyzz_madd": _op(2, "madd", b_inf=False),
    "xyzz_add": _op(3, "add"),
    "xyzz_neg": _op(4, "neg"),
    "madd_mem": _op(5, "madd", refs=True, packed=True, a_inf=False, b_inf=False, flag=True),
    "madd_lds_regy": _op(6, "madd", refs=True, lds=True, packed=True, a_inf=False, b_inf=False, y_mul2=True, flag=True),
    "add_lds_regy": _op(7, "add", refs=True, lds=True, a_inf=False, b_inf=False, y_mul2=True, flag=True),
    "add_mem_s": _op(8, "add", refs=True, y_mul2=True),
    "dbl_mem": _op(9, "dbl", refs=True, y_mul2=True),
    "add_mem_quad": _op(10, "add", refs=True, quad=True),
    "dbl_mem_quad": _op(11, "dbl", refs=True, quad=True),
    "edw_madd_lds_regy": _op(12, "edw_madd", lds=True, packed=True, a_inf=False, b_inf=False),
    "edw_add_lds_regy": _op(13, "edw_add", refs=True, lds=True, a_inf=False, b_inf=False),
    "edw_add_mem": _op(14, "edw_add", refs=True),
    "edw_add_mem_quad": _op(15, "edw_add", refs=True, quad=True),
    "edw_dbl_mem_quad": _op(16, "edw_dbl", refs=True, quad=True),
    "edw_from_affine": _op(17, "from_affine", packed=True, flag=True),
    "edw_lock": _op(18, "lock", lds=True),
}
REGISTER_OPS = ("xyzz_dbl_affine", "xyzz_dbl", "xyzz_madd", "xyzz_add", "xyzz_neg")      # ZK_HD: g++ runs them too


def mems(name):
    return (0, 1) if OPS[name].refs else (0,)


def wave_cases(name):
    return 16 if OPS[name].quad else 64


def inv(a):
    return pow(a % p, -1, p)


# ---------------------------------------------------------------- points
@functools.lru_cache(maxsize=None)
def pool(curve):
    """k G for k = 1 .. 8, G the generator of G1 / G2"""
    g = R.G1_GEN if curve == "g1" else R.G2_GEN
    out, P = [], None
    for _ in range(8):
        P = R.ec_add(P, g)
        out.append(P)
    return tuple(out)


def on_some_curve(P):
    return P is None or R.on_curve(P, R.G1_B) or R.on_curve(P, R.G2_B)


def _root(c, e):
    """an e-th root of c (e = 2: p = 3 mod 4; e = 3: p = 4 mod 9), or None"""
    r = pow(c, (p + 1) // 4, p) if e == 2 else pow(c, (2 * p + 1) // 9, p)
    return r if pow(r, e, p) == c % p else None


assert p % 4 == 3 and p % 9 == 4


@functools.lru_cache(maxsize=None)
def near_lambda(P, coord, side):
    """lambda such that coordinate `coord` of P's XYZZ representative (x l^2, y l^3, l^2, l^3) has a Montgomery residue within a few
    units of 0 (side 0) or of p (side 1); None when that coordinate of P is 0"""
    base = (P[0] * RM, P[1] * RM, RM, RM)[coord] % p
    if base == 0:
        return None
    bi = inv(base)
    for d in range(1, 200):
        lam = _root((d if side == 0 else p - d) * bi % p, 2 if coord in (0, 2) else 3)
        if lam:
            return lam
    raise AssertionError("no residue near %d p has a root" % side)


STYLES = ("lo", "hi", "rand") + tuple("near%d%d" % (c, s) for c in range(4) for s in range(2))


def _zero_j(rng, c, closed):
    k = KB[c] if c < 4 else 2
    top = k if (closed and c == 1) else k - 1
    return rng.choice([0, top, top, rng.randrange(top + 1)])


def rep_xyzz(P, rng, style):
    """[X, Y, ZZ, ZZZ] of the finite point P as raw integers"""
    lam, js = None, None
    if style.startswith("near"):
        c, s = int(style[4]), int(style[5])
        lam = near_lambda(P, c, s)
        js = [rng.randrange(k) for k in KB]
        js[c] = 0 if s == 0 else KB[c] - 1
    if lam is None:
        lam = rng.randrange(1, p)
    if js is None or style in ("lo", "hi", "rand"):
        js = [0] * 4 if style == "lo" else [k - 1 for k in KB] if style == "hi" else [rng.randrange(k) for k in KB]
    l2 = lam * lam % p
    l3 = l2 * lam % p
    res = [P[0] * l2 * RM % p, P[1] * l3 * RM % p, l2 * RM % p, l3 * RM % p]
    return [v + (j if v else _zero_j(rng, c, True)) * p for c, (v, j) in enumerate(zip(res, js))]


def rep_inf(rng, variant):
    """an infinite XYZZ operand: ZZ and ZZZ as 0 or p (variant bits 0, 1), X and Y zero (bit 2 clear: what xyzz_infinity() leaves) or
    anything inside the contract (what doubling a 2-torsion point leaves)"""
    zz, zzz = (variant & 1) * p, ((variant >> 1) & 1) * p
    if variant & 4:
        return [rng.randrange(10 * p), rng.randrange(4 * p + 1), zz, zzz]
    return [0, 0, zz, zzz]


def rep_aff_reg(P, rng, style):
    """a register affine operand [2]"""
    js = (0, 0) if style == "lo" else (1, 1) if style == "hi" else (rng.randrange(2), rng.randrange(2))
    return [P[0] * RM % p + js[0] * p, P[1] * RM % p + js[1] * p]


def aff_packed(P):
    return [P[0] * RM % p, P[1] * RM % p]


@functools.lru_cache(maxsize=None)
def chi_e(P):
    """Edwards affine image of a G1 point; None (infinity of G1) is the identity (0, 1)"""
    return (0, 1) if P is None else EM.chi(P)


def rep_edw(P, rng, style):
    """[X, Y, Z, T] of chi(P) as raw integers, coordinates [2]"""
    xe, ye = chi_e(P)
    js = [0] * 4 if style == "lo" else [1] * 4 if style == "hi" else [rng.randrange(2) for _ in range(4)]
    Z = rng.randrange(1, p)
    if style.startswith("near"):
        c, s = int(style[4]), int(style[5])
        base = (xe, ye, 1, xe * ye)[c] * RM % p
        if base:
            Z = (1 + rng.randrange(3) if s == 0 else p - 1 - rng.randrange(3)) * inv(base) % p
            js[c] = s
    res = [xe * Z * RM % p, ye * Z * RM % p, Z * RM % p, xe * ye * Z * RM % p]
    return [v + (j if v else rng.randrange(2)) * p for v, j in zip(res, js)]


def rep_edw_empty(rng):
    return [rng.randrange(2 * p), rng.randrange(2 * p), 0, rng.randrange(2 * p)]


def edw_packed(P, neg=False):
    return [v * RM % p for v in EM.precomputed(chi_e(P), neg)]


# ---------------------------------------------------------------- situations and waves
WAVES = ("none", "all", "first", "middle", "last", "some")


def _situations(op):
    non = ["gen_g1", "gen_g2", "tors_a", "tors_b", "x0_a", "x0_b"]
    if op.a_inf:
        non.append("a_inf")
    if op.b_inf:
        non.append("b_inf")
    if op.a_inf and op.b_inf:
        non.append("both_inf")
    return non, ["eq_g1", "opp_g1", "eq_g2", "opp_g2", "tors_eq", "x0_eq", "x0_opp"]


@functools.lru_cache(maxsize=None)
def layout(name):
    """(situations in lane order, [(wave kind, first case, size)])"""
    op = OPS[name]
    W = wave_cases(name)
    sits, waves = [], []

    def wave(kind, w):
        waves.append((kind, len(sits), len(w)))
        sits.extend(w)

    if op.kind in ("madd", "add"):
        non, same = _situations(op)
        copyish = [s for s in non if s.endswith("inf")] or non
        wave("none", [non[i % len(non)] for i in range(W)])
        wave("all", [same[i % len(same)] for i in range(W)])
        for k, (kind, pos) in enumerate((("first", 0), ("middle", W // 2 - 1), ("last", W - 1))):
            w = [non[(i + k) % len(non)] for i in range(W)]
            w[pos] = same[k]
            wave(kind, w)
        wave("some", [(same, copyish, non)[i % 3][(i // 3) % len((same, copyish, non)[i % 3])] for i in range(W)])
        k = 0
        while len(sits) < N_MIN:
            both = non + same
            wave("mixed", [both[(5 * i + 3 * k) % len(both)] for i in range(W)])
            k += 1
        wave("mixed", [(non + same)[i % (len(non) + len(same))] for i in range(W // 2 + 1)])      # a last wave that is not full
    else:
        lst = {"dbl": ["gen_g1", "gen_g2", "inf", "tors", "x0"], "dbl_affine": ["gen_g1", "gen_g2", "tors", "x0"],
               "neg": ["gen_g1", "gen_g2", "inf", "tors", "x0"],
               "edw_madd": ["gen", "eq", "opp", "a_id0", "a_id"],
               "edw_add": ["gen", "eq", "opp", "a_id", "b_id", "both_id"] + (["a_empty"] if op.a_inf else []) + (["b_empty"] if op.b_inf else [])
               + (["both_empty"] if op.a_inf and op.b_inf else []),
               "edw_dbl": ["gen", "id", "empty"]}[op.kind]
        n = N_MIN + W // 2 + 1 + (-N_MIN) % W
        for s in range(0, n, W):
            wave("mixed", [lst[(i + s // W) % len(lst)] for i in range(s, min(n, s + W))])
    return tuple(sits), tuple(waves)


def _case(**kw):
    d = dict(A=None, B=None, neg=False, entries=(), pa=None, pb=None, want=None, same_x=False, path="computed", copy=None, sit="", style="")
    d.update(kw)
    return SimpleNamespace(**d)


def _pick(rng, curve, avoid=()):
    while True:
        P = rng.choice(pool(curve))
        if all(P[0] != a[0] for a in avoid if a):
            return P


@functools.lru_cache(maxsize=None)
def cases(name):
    """the cases of one op in lane order; deterministic"""
    op = OPS[name]
    if op.kind == "from_affine":
        out = _from_affine_cases()
    elif op.kind == "lock":
        out = _lock_cases()
    else:
        rng = random.Random(SEED + op.code)
        sits, _ = layout(name)
        build = _build_edw if op.kind.startswith("edw") else _build_xyzz
        out = tuple(build(name, op, s, i, rng) for i, s in enumerate(sits))
    for c in out:
        precondition(name, c)
    return out


def n_cases(name):
    return len(cases(name))


def _build_xyzz(name, op, sit, i, rng):
    sa, sb = STYLES[i % len(STYLES)], STYLES[(i // len(STYLES) + 3 * i) % len(STYLES)]
    s, curve = (sit[:-3], sit[-2:]) if sit[-3:] in ("_g1", "_g2") else (sit, "g1")
    neg = op.packed and op.kind == "madd" and rng.random() < 0.5
    if op.kind in ("dbl", "dbl_affine", "neg"):
        P = {"gen": _pick(rng, curve), "inf": None, "tors": T2, "x0": X0 if i % 2 else R.ec_neg(X0)}[s]
        if op.kind == "dbl_affine":
            return _finish(name, op, _case(B=rep_aff_reg(P, rng, ("lo", "hi", "rand")[i % 3]), pb=P, pa=P, sit=sit, style=sa))
        A = rep_inf(rng, i % 8) if P is None else rep_xyzz(P, rng, sa)
        if op.kind == "neg" and i % 4 == 0 and P is not None and P[1] == 0:
            A[1] = 0                                                     # Y = 0 as zero limbs: 4p - 0
        return _finish(name, op, _case(A=A, pa=P, pb=P, sit=sit, style=sa))
    # madd / add: pa and the EFFECTIVE pb (after neg)
    if s == "gen":
        pa = _pick(rng, curve)
        pb = _pick(rng, curve, (pa,))
    elif s in ("eq", "opp"):
        pa = _pick(rng, curve)
        pb = pa if s == "eq" else R.ec_neg(pa)
    elif s in ("tors_a", "tors_b"):
        other = _pick(rng, "g1") if rng.random() < 0.7 else R.ec_add(_pick(rng, "g1"), T2)
        pa, pb = (T2, other) if s == "tors_a" else (other, T2)
    elif s == "tors_eq":
        pa = pb = T2
    elif s in ("x0_a", "x0_b", "x0_eq", "x0_opp"):
        x0 = X0 if rng.random() < 0.5 else R.ec_neg(X0)
        other = {"x0_a": None, "x0_b": None, "x0_eq": x0, "x0_opp": R.ec_neg(x0)}[s] or _pick(rng, "g2")
        pa, pb = (other, x0) if s == "x0_b" else (x0, other)
    elif s == "a_inf":
        pa, pb = None, _pick(rng, curve)
    elif s == "b_inf":
        pa, pb = _pick(rng, curve), None
    else:
        assert s == "both_inf", sit
        pa = pb = None
    A = rep_inf(rng, i % 8) if pa is None else rep_xyzz(pa, rng, sa)
    if op.kind == "add":
        B = rep_inf(rng, (i // 8 + i) % 8) if pb is None else rep_xyzz(pb, rng, sb)
    else:
        given = R.ec_neg(pb) if neg else pb                              # what the table holds
        B = aff_packed(given) if op.packed else rep_aff_reg(given, rng, ("lo", "hi", "rand")[(i // 2) % 3])
    return _finish(name, op, _case(A=A, B=B, neg=neg, pa=pa, pb=pb, sit=sit, style=sa + "/" + sb))


def _finish(name, op, c):
    """the expectation of an XYZZ case: want (affine sum, None = infinity), same_x, path, copy"""
    pa, pb = c.pa, c.pb
    if op.kind == "neg":
        c.want, c.path = R.ec_neg(pa), "neg"
        c.copy = [c.A[0], 4 * p - c.A[1], c.A[2], c.A[3]]
    elif op.kind in ("dbl", "dbl_affine"):
        c.want = R.ec_add(pa, pa)
        c.path = "keep" if (pa is None and op.refs) else "dbl"
    elif pb is None:
        c.want, c.path = pa, "keep"
    elif pa is None:
        c.want, c.path = pb, "copy"
        c.copy = list(c.B) if op.kind == "add" else [c.B[0], c.B[1], RM, RM]
    elif pa[0] == pb[0]:
        c.same_x = True
        c.want = R.ec_add(pa, pb)
        c.path = "dbl" if pa == pb else "cancel"
    else:
        c.want = R.ec_add(pa, pb)
    if c.path == "keep":
        c.copy = list(c.A)
    return c


def _build_edw(name, op, sit, i, rng):
    sa, sb = STYLES[i % len(STYLES)], STYLES[(i // len(STYLES) + 3 * i) % len(STYLES)]
    neg = op.kind == "edw_madd" and rng.random() < 0.5
    pa = _pick(rng, "g1")
    pb = _pick(rng, "g1", (pa,))
    a_empty = sit in ("a_empty", "both_empty") or sit == "empty"
    b_empty = sit in ("b_empty", "both_empty")
    if sit == "eq":
        pb = pa
    elif sit == "opp":
        pb = R.ec_neg(pa)
    if sit in ("a_id", "a_id0", "both_id", "id"):
        pa = None
    if sit in ("b_id", "both_id"):
        pb = None
    if op.kind == "edw_dbl":
        pb = pa
    A = rep_edw_empty(rng) if a_empty else [0, RM, RM, 0] if sit == "a_id0" else rep_edw(pa, rng, sa)      # a_id0: edw_set_identity's limbs
    c = _case(A=A, neg=neg, pa=pa, pb=pb, sit=sit, style=sa + "/" + sb)
    if op.kind == "edw_madd":
        c.B = edw_packed(R.ec_neg(pb) if neg else pb)
    elif op.kind == "edw_add":
        c.B = rep_edw_empty(rng) if b_empty else rep_edw(pb, rng, sb)
    if op.kind != "edw_dbl" and b_empty:
        c.path, c.copy = "keep", list(A)
    elif a_empty:
        c.path, c.copy = ("keep", list(A)) if op.kind == "edw_dbl" else ("copy", list(c.B))
    else:
        c.want = chi_e(R.ec_add(pa, pb))
    return c


@functools.lru_cache(maxsize=None)
def g1_points(n):
    out, P = [], None
    for _ in range(n):
        P = R.ec_add(P, R.G1_GEN)
        out.append(P)
    return tuple(out)


def _from_affine_cases():
    """edw_from_affine: points of G1 (accepted, the packed words are precomputed(chi(P))); points of G2's curve, the three points of
    order 2 and P + (1, 0) for P in G1 (refused).  The case's same_x field holds the expected return value."""
    rng = random.Random(SEED + 17)
    g1 = g1_points(240)
    out = []
    g2, Q = [X0, R.ec_neg(X0)], None
    for _ in range(46):
        Q = R.ec_add(Q, R.G2_GEN)
        g2.append(Q)
    for i in range(N_MIN + 21):
        k = i % 8
        if k == 3:
            P, ok, sit = g2[(i // 8) % len(g2)], False, "g2"
        elif k == 6 and (i // 8) % 4 == 0:
            P, ok, sit = T2, False, "tors"
        elif k == 6 and (i // 8) % 4 in (1, 2):                          # y = 0, x != 1: no denominator vanishes, x_e = 0 does
            P, ok, sit = (pow(OMEGA, (i // 8) % 4, p), 0), False, "tors_w"
        elif k == 5:
            P, ok, sit = R.ec_add(g1[(i // 8) % len(g1)], T2), False, "g1_plus_tors"
        else:
            P = g1[(7 * i + 1) % len(g1)]
            P, ok, sit = (R.ec_neg(P) if rng.random() < 0.5 else P), True, "g1"
        out.append(_case(B=aff_packed(P), pb=P, sit=sit, same_x=ok, want=edw_packed(P) if ok else None))
    return tuple(out)


LOCK_TABLE_POINTS = 24


@functools.lru_cache(maxsize=None)
def lock_table():
    """the table of the lockstep run: precomputed(chi(k G)), k = 1 .. 24, canonical Montgomery words (72 per point)"""
    return tuple(tuple(w for v in edw_packed(P) for w in F.words(v)[:24]) for P in g1_points(LOCK_TABLE_POINTS))


def _lock_cases():
    """runs of 1, 2 or 3 entries (index | neg << 31), descending count inside every wave of 64 as in the kernel's bucket order"""
    rng = random.Random(SEED + 18)
    pts = g1_points(LOCK_TABLE_POINTS)
    out = []
    shapes = ([3] * 64, [3] * 22 + [2] * 21 + [1] * 21, [2] * 64, [1] * 64, [3] * 63 + [1], [3] + [2] * 62 + [1], [2] * 40)
    for w, shape in enumerate(shapes):
        for i, cnt in enumerate(shape):
            idx = [rng.randrange(len(pts)) for _ in range(cnt)]
            sg = [rng.randrange(2) for _ in range(cnt)]
            sit = "gen"
            if cnt >= 2 and i % 5 == 1:
                idx[1], sg[1], sit = idx[0], sg[0] ^ 1, "opp"             # P - P: the identity, an ordinary point, then one more entry
            elif cnt >= 2 and i % 5 == 2:
                idx[1], sg[1], sit = idx[0], sg[0], "eq"                  # P + P through the unified addition
            elif cnt == 3 and i % 5 == 3:
                idx[2], sg[2], sit = idx[1], sg[1] ^ 1, "opp_last"
            tot = None
            for k, s in zip(idx, sg):
                tot = R.ec_add(tot, R.ec_neg(pts[k]) if s else pts[k])
            out.append(_case(entries=tuple(k | (s << 31) for k, s in zip(idx, sg)), sit=sit, want=chi_e(tot), pa=tot))
    return tuple(out)


# ---------------------------------------------------------------- preconditions
def _fits(v):
    return 0 <= v < 1 << (F.sh + 32)


def _pre_xyzz(P, v, finite_only, lds):
    assert all(_fits(x) for x in v) and v[0] < 10 * p and v[1] <= 4 * p and v[2] < 2 * p and v[3] < 2 * p
    assert (v[2] ** 3 - v[3] ** 2 * RM) % p == 0                         # ZZ^3 = ZZZ^2
    if P is None:
        assert not finite_only and v[2] in (0, p) and v[3] in (0, p)
    else:
        assert v[2] % p and (v[0] - P[0] * v[2]) % p == 0 and (v[1] - P[1] * v[3]) % p == 0 and on_some_curve(P)
    assert not lds or v[0] < 1 << 768


def _pre_edw(P, v, empty, may_be_empty, lds):
    assert all(0 <= x < 2 * p for x in v)
    if empty:
        assert may_be_empty and v[2] == 0
        return
    xe, ye = chi_e(P)
    assert EM.e_on_curve((xe, ye)) and v[2] % p and (v[0] - xe * v[2]) % p == 0 and (v[1] - ye * v[2]) % p == 0
    assert (v[3] * v[2] - v[0] * v[1]) % p == 0
    assert not lds or v[0] < 1 << 768


def precondition(name, c):
    """the documented input contract of the op, on one case"""
    op = OPS[name]
    k = op.kind
    if k == "from_affine":
        assert all(0 <= v < p for v in c.B)
    elif k == "lock":
        assert 1 <= len(c.entries) <= 3 and all((e & 0x7FFFFFFF) < LOCK_TABLE_POINTS for e in c.entries)
    elif k == "dbl_affine":
        assert all(0 <= v < 2 * p for v in c.B) and c.pb is not None and on_some_curve(c.pb)
        assert [v % p for v in c.B] == aff_packed(c.pb)
    elif k in ("dbl", "neg"):
        _pre_xyzz(c.pa, c.A, False, False)
    elif k in ("madd", "add"):
        _pre_xyzz(c.pa, c.A, not op.a_inf, op.lds)
        if k == "add":
            _pre_xyzz(c.pb, c.B, not op.b_inf, False)
        else:
            given = R.ec_neg(c.pb) if c.neg else c.pb
            assert given is not None and on_some_curve(given) and [v % p for v in c.B] == aff_packed(given)
            assert all(0 <= v < (p if op.packed else 2 * p) for v in c.B)
    elif k == "edw_madd":
        _pre_edw(c.pa, c.A, False, False, True)
        assert c.pb is not None and c.B == edw_packed(R.ec_neg(c.pb) if c.neg else c.pb) and all(0 <= v < p for v in c.B)
    elif k == "edw_add":
        _pre_edw(c.pa, c.A, c.sit in ("a_empty", "both_empty"), op.a_inf, op.lds)
        _pre_edw(c.pb, c.B, c.sit in ("b_empty", "both_empty"), op.b_inf, False)
    else:
        assert k == "edw_dbl"
        _pre_edw(c.pa, c.A, c.sit == "empty", True, False)


def check_layout(name):
    """the wave composition the module's docstring promises (and, for the lockstep run, the descending counts)"""
    op = OPS[name]
    cs = cases(name)
    W = wave_cases(name)
    if op.kind == "lock":
        for s in range(0, len(cs), 64):
            cnt = [len(c.entries) for c in cs[s:s + 64]]
            assert cnt == sorted(cnt, reverse=True)
        return
    if op.kind not in ("madd", "add"):
        return
    _, waves = layout(name)
    kinds = {}
    for kind, start, size in waves:
        assert start % W == 0
        kinds.setdefault(kind, []).append([c.same_x for c in cs[start:start + size]])
    assert set(WAVES) <= set(kinds)
    assert not any(kinds["none"][0]) and all(kinds["all"][0])
    assert kinds["first"][0] == [True] + [False] * (W - 1) and kinds["last"][0] == [False] * (W - 1) + [True]
    assert sum(kinds["middle"][0]) == 1 and kinds["middle"][0][W // 2 - 1]
    some = cs[waves[5][1]:waves[5][1] + waves[5][2]]
    assert 0 < sum(c.same_x for c in some) < len(some)
    assert not op.a_inf or any(c.path in ("copy", "keep") for c in some)


# ---------------------------------------------------------------- rows
def _b_words(op, c):
    if c.B is None:
        return []
    if op.packed:
        return [w for v in c.B for w in F.words(v)[:24]]
    return [w for v in c.B for w in F.limbs(v)]


def operands(name, c):
    """the case as the ROW_IN words of the hook"""
    op = OPS[name]
    row = [0] * ROW_IN
    if c.A is not None:
        row[0:108] = [w for v in c.A for w in F.limbs(v)]
    b = _b_words(op, c)
    row[108:108 + len(b)] = b
    row[216] = int(c.neg)
    row[217:217 + len(c.entries)] = list(c.entries)
    row[220] = len(c.entries)
    return row


def _int29(l, what):
    assert all(x < 1 << 29 for x in l[:26]), what + ": limbs not normalised"
    return sum(x << (29 * i) for i, x in enumerate(l))


def decode(name, row):
    """the four coordinates of an output row as integers (X of an LDS form from its 24 packed words)"""
    op = OPS[name]
    out = []
    for c in range(4):
        l = row[27 * c:27 * c + 27]
        if c == 0 and op.lds:
            assert l[24:] == [0, 0, 0], name
            out.append(sum(w << (32 * j) for j, w in enumerate(l[:24])))
        else:
            out.append(_int29(l, "%s coordinate %d" % (name, c)))
    return out


# ---------------------------------------------------------------- the checker
def check(name, c, row):
    """one output row of the hook against the case's expectation; raises AssertionError"""
    op = OPS[name]
    row = [int(x) for x in row]
    assert len(row) == ROW_OUT
    what = "%s [%s %s]" % (name, c.sit, c.style)
    flag = row[108]
    # 5. B is returned as it was given
    b = _b_words(op, c)
    assert row[109:109 + len(b)] == b, what + ": B was written"
    if op.kind == "from_affine":
        assert flag == int(c.same_x), what + ": returned %d, want %d" % (flag, int(c.same_x))
        if c.same_x:
            assert row[:72] == [w for v in c.want for w in F.words(v)[:24]], what + ": packed words differ from precomputed(chi(P))"
        return
    v = decode(name, row)
    if op.kind.startswith("edw") or op.kind == "lock":
        empty = v[2] in (0, p)
        assert flag == int(empty), what + ": flag"
        if c.path in ("keep", "copy"):
            assert v == c.copy, what + ": the operand was not left / copied as it stood"
            return
        assert all(x < 2 * p for x in v), what + ": a coordinate is not below 2p: %s" % [x // p for x in v]        # 3. [2]
        xe, ye = c.want
        assert v[2] % p, what + ": Z = 0"
        assert (v[0] - xe * v[2]) % p == 0 and (v[1] - ye * v[2]) % p == 0, what + ": not the sum"                   # 1. value
        assert (v[3] * v[2] - v[0] * v[1]) % p == 0, what + ": T Z != X Y"                                          # 2. invariant
        return
    # XYZZ
    assert flag == int(c.same_x if op.flag else c.want is None), what + ": flag %d" % flag                           # 4. flag
    if c.path in ("keep", "copy", "neg"):
        assert v == c.copy, what + ": expected the exact limbs %s, got %s" % ([hex(x) for x in c.copy], [hex(x) for x in v])
    elif c.path == "cancel":
        assert v == [0, 0, 0, 0], what + ": P + (-P) does not leave the limbs of infinity"
    kx, ky, closed = out_bound(op, c)
    assert v[0] < kx * p, what + ": X = %.3f p, documented [%d]" % (v[0] / p, kx)                                    # 3. bounds
    assert v[1] < ky * p or (closed and v[1] == ky * p), what + ": Y = %.3f p, documented [%d]" % (v[1] / p, ky)
    assert v[2] < 2 * p and v[3] < 2 * p, what + ": ZZ / ZZZ not below 2p"
    assert (v[2] ** 3 - v[3] ** 2 * RM) % p == 0, what + ": ZZ^3 != ZZZ^2"                                          # 2. invariant
    if c.want is None:                                                                                              # 1. value
        assert v[2] % p == 0, what + ": the sum is infinity, ZZ is not 0"
    else:
        assert v[2] % p, what + ": ZZ = 0, the sum is finite"
        assert (v[0] - c.want[0] * v[2]) % p == 0 and (v[1] - c.want[1] * v[3]) % p == 0, what + ": not the sum"


def out_bound(op, c):
    """(k of X, k of Y, Y's bound closed) the comments promise for this case's path"""
    if c.path in ("keep", "copy", "neg", "cancel"):
        return 10, 4, True                           # a stored point as it stood (neg: 4p - Y <= 4p)
    if c.path == "dbl":
        if c.same_x and op.lds:
            return 1, 4, False                       # the same-x path hands X back canonical
        return 6, 2 if (op.y_mul2 and not c.same_x) else 4, False
    return 10, 2 if op.y_mul2 else 4, False
