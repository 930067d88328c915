"""tests/point_ops_cases.py checked on its own (CPU): counts and wave layout, every precondition, the expectations against an
independent affine computation, and the presence of every listed situation and of both ends of every bound for every op."""
import pytest

from oracle import pyref as R
from tests import point_ops_cases as C
from tests import test_edwards_model as EM

p = C.p
ALL = list(C.OPS)
XYZZ_STORED = [n for n, o in C.OPS.items() if o.kind in ("dbl", "neg", "madd", "add")]
EDW_STORED = [n for n, o in C.OPS.items() if o.kind in ("edw_madd", "edw_add", "edw_dbl")]


@pytest.mark.parametrize("name", ALL)
def test_counts_layout_and_preconditions(name):
    cs = C.cases(name)
    assert len(cs) == C.n_cases(name) >= 300
    assert cs is C.cases(name)                                           # deterministic and shared
    for c in cs:
        C.precondition(name, c)
        assert len(C.operands(name, c)) == C.ROW_IN
    C.check_layout(name)
    assert C.mems(name) == ((0, 1) if name in ("madd_mem", "madd_lds_regy", "add_lds_regy", "add_mem_s", "dbl_mem", "add_mem_quad", "dbl_mem_quad",
                                               "edw_add_lds_regy", "edw_add_mem", "edw_add_mem_quad", "edw_dbl_mem_quad") else (0,))


def _affine(name, v):
    """an XYZZ representative back to the affine point, by division"""
    if v[2] % p == 0:
        return None
    return v[0] * C.inv(v[2]) % p, v[1] * C.inv(v[3]) % p


@pytest.mark.parametrize("name", [n for n, o in C.OPS.items() if o.kind in ("madd", "add", "dbl", "dbl_affine", "neg")])
def test_xyzz_expectations_against_the_affine_law(name):
    """the sum recomputed from the operands' LIMB values alone, with the Edwards model's w_add (an implementation of the affine law
    that is not the generator's)"""
    op = C.OPS[name]
    for c in C.cases(name):
        a = _affine(name, c.A) if c.A is not None else None
        if op.kind in ("dbl", "dbl_affine", "neg"):
            b = a if c.A is not None else tuple(v * C.inv(C.RM) % p for v in c.B)
            a = b
        elif op.kind == "add":
            b = _affine(name, c.B)
        else:
            b = tuple(v * C.inv(C.RM) % p for v in c.B)
            if c.neg:
                b = EM.w_neg(b)
        want = EM.w_neg(a) if op.kind == "neg" else EM.w_add(a, b)
        assert want == c.want, (name, c.sit)
        assert c.same_x == (op.kind in ("madd", "add") and a is not None and b is not None and a[0] == b[0])


@pytest.mark.parametrize("name", EDW_STORED + ["edw_lock"])
def test_edwards_expectations_against_the_edwards_law(name):
    """chi(A + B) against the affine EDWARDS addition of the operands' own affine values (e_add_affine: neither chi nor G1's law)"""
    op = C.OPS[name]
    tab = C.g1_points(C.LOCK_TABLE_POINTS)
    for c in C.cases(name):
        if c.path != "computed":
            continue
        if op.kind == "lock":
            acc = (0, 1)
            for e in c.entries:
                x, y = EM.chi(tab[e & 0x7FFFFFFF])
                acc = EM.e_add_affine(acc, ((-x) % p if e >> 31 else x, y))
            assert acc == c.want
            continue
        a = EM.e_affine(c.A)
        if op.kind == "edw_dbl":
            b = a
        elif op.kind == "edw_add":
            b = EM.e_affine(c.B)
        else:
            ymx, ypx, t2d = (v * C.inv(C.RM) % p for v in c.B)
            b = ((ypx - ymx) * C.inv(2) % p, (ypx + ymx) * C.inv(2) % p)
            assert t2d == 2 * EM.D * b[0] * b[1] % p
            if c.neg:
                b = ((-b[0]) % p, b[1])
        assert EM.e_add_affine(a, b) == c.want, (name, c.sit)


@pytest.mark.parametrize("name", [n for n, o in C.OPS.items() if o.kind in ("madd", "add")])
def test_every_situation_of_the_additions(name):
    op = C.OPS[name]
    cs = C.cases(name)
    sits = {c.sit for c in cs}
    need = {"gen_g1", "gen_g2", "eq_g1", "eq_g2", "opp_g1", "opp_g2", "tors_a", "tors_b", "tors_eq", "x0_a", "x0_b", "x0_eq", "x0_opp"}
    need |= ({"a_inf"} if op.a_inf else set()) | ({"b_inf"} if op.b_inf else set()) | ({"both_inf"} if op.a_inf and op.b_inf else set())
    assert need <= sits
    # the same-x pairs are the same point under ANOTHER scaling and other representatives
    if op.kind == "add":
        assert all(c.A != c.B for c in cs if c.sit.startswith("eq"))
        assert any(c.A[2] % p != c.B[2] % p for c in cs if c.sit.startswith("eq"))
    if op.packed:                                                        # (1, 0) through neg: y = 0 negated is exactly 2p
        assert any(c.neg and c.pb == C.T2 for c in cs) and any(not c.neg and c.pb == C.T2 for c in cs)
        assert any(c.neg and c.same_x for c in cs) and any(not c.neg and c.same_x for c in cs)
    for who, flag in (("A", op.a_inf), ("B", op.b_inf and op.kind == "add")):
        if flag:                                                         # ZZ = 0 as zero limbs and as p for every infinity test
            zz = {getattr(c, who)[2] for c in cs if (c.pa if who == "A" else c.pb) is None}
            assert zz == {0, p}, (name, who)


@pytest.mark.parametrize("name", XYZZ_STORED)
def test_both_ends_of_every_bound_xyzz(name):
    """every coordinate of a stored operand at j = 0 and j = k - 1, its integer within 200 of 0 and of k p, and a coordinate = 0
    (mod p) as zero limbs and as a non-zero multiple of p"""
    op = C.OPS[name]
    for who in ("A", "B") if op.kind == "add" else ("A",):
        reps = [(getattr(c, who), c.pa if who == "A" else c.pb) for c in C.cases(name)]
        fin = [v for v, P in reps if P is not None]
        for k, kb in enumerate(C.KB):
            js = {v[k] // p for v in fin if v[k] % p}
            assert {0, kb - 1} <= js, (name, who, k, js)
            assert any(0 < v[k] < 200 for v in fin), (name, who, k, "next to 0")
            assert any(0 < kb * p - v[k] < 200 for v in fin), (name, who, k, "next to k p")
        for k in (0, 1):
            zero = {v[k] for v in fin if v[k] % p == 0}
            assert 0 in zero and any(zero - {0}), (name, who, k)
        if not (op.lds and who == "A"):
            assert any(v[1] == 4 * p for v in fin), (name, who, "Y = 4p")


@pytest.mark.parametrize("name", EDW_STORED)
def test_both_ends_of_every_bound_edwards(name):
    op = C.OPS[name]
    cs = C.cases(name)
    for who in ("A", "B") if op.kind == "edw_add" else ("A",):
        fin = [getattr(c, who) for c in cs if getattr(c, who)[2] % p]
        for k in range(4):
            assert {0, 1} <= {v[k] // p for v in fin if v[k] % p}
            assert any(0 < v[k] < 200 for v in fin) and any(0 < 2 * p - v[k] < 200 for v in fin), (name, who, k)
        assert {v[0] for v in fin if v[0] % p == 0} == {0, p}            # the identity's X = 0 both ways
    sits = {c.sit for c in cs}
    if op.kind == "edw_add":
        need = {"gen", "eq", "opp", "a_id", "b_id", "both_id"} | ({"a_empty", "b_empty", "both_empty"} if op.a_inf else set())
        assert need <= sits
        assert any(c.sit == "opp" and c.want == (0, 1) for c in cs)
    if op.quad:                                                          # a wave in which only some quads take the copy path
        w0 = cs[:16]
        assert 0 < sum(c.path != "computed" for c in w0) < 16


def test_the_other_ops_situations():
    for name in ("xyzz_dbl", "dbl_mem", "dbl_mem_quad", "xyzz_neg"):
        assert {"gen_g1", "gen_g2", "inf", "tors", "x0"} <= {c.sit for c in C.cases(name)}
        assert {c.A[2] for c in C.cases(name) if c.pa is None} == {0, p}
    assert {"gen_g1", "gen_g2", "tors", "x0"} <= {c.sit for c in C.cases("xyzz_dbl_affine")}
    assert {tuple(v // p for v in c.B) for c in C.cases("xyzz_dbl_affine")} >= {(0, 0), (1, 1)}
    # xyzz_neg at Y = 0 limbs: of the infinity xyzz_infinity() leaves and of (1, 0)
    assert any(c.A[1] == 0 and c.pa is None for c in C.cases("xyzz_neg")) and any(c.A[1] == 0 and c.pa == C.T2 for c in C.cases("xyzz_neg"))
    fa = C.cases("edw_from_affine")
    assert {"g1", "g2", "tors", "tors_w", "g1_plus_tors"} <= {c.sit for c in fa}
    assert {c.pb for c in fa if c.sit == "tors_w"} == {(C.OMEGA, 0), (C.OMEGA * C.OMEGA % p, 0)}
    for i, c in enumerate(fa):
        on_g1 = R.on_curve(c.pb, R.G1_B)
        assert on_g1 == (c.sit != "g2")
        assert c.same_x == (c.sit == "g1")
        if c.sit == "g1":
            assert c.want == [v * C.RM % p for v in EM.precomputed(EM.chi(c.pb))]
        if i % 16 < 6:                                                   # the order, on a sample (377-bit scalar multiplications)
            assert c.sit != "g1" or R.ec_mul(R.R_MOD, c.pb) is None
            assert c.sit != "g1_plus_tors" or R.ec_mul(R.R_MOD, c.pb) == C.T2       # even order
    lk = C.cases("edw_lock")
    assert {len(c.entries) for c in lk} == {1, 2, 3} and {"gen", "opp", "eq", "opp_last"} <= {c.sit for c in lk}
    assert any(c.want == (0, 1) for c in lk) and {e >> 31 for c in lk for e in c.entries[:1]} == {0, 1}


def test_the_checker_refuses_wrong_rows():
    """a correct row passes; one coordinate lifted past its bound, a wrong sum, a broken invariant, a wrong flag and a touched B fail"""
    name = "xyzz_add"
    c = next(c for c in C.cases(name) if c.sit == "gen_g1")
    want = C.rep_xyzz(c.want, __import__("random").Random(1), "lo")
    b = [w for v in c.B for w in C.F.limbs(v)]

    def row(v, flag=0, bw=b):
        return [w for x in v for w in C.F.limbs(x)] + [flag] + bw

    C.check(name, c, row(want))
    for bad in ([want[0] + 10 * p] + want[1:], [want[0], want[1] + 4 * p] + want[2:], [want[0] + 1] + want[1:], want[:2] + [want[2] + p * 2, want[3]],
                want[:3] + [(-want[3]) % p]):
        with pytest.raises(AssertionError):
            C.check(name, c, row(bad))
    with pytest.raises(AssertionError):
        C.check(name, c, row(want, 1))
    with pytest.raises(AssertionError):
        C.check(name, c, row(want, 0, [b[0] ^ 1] + b[1:]))
