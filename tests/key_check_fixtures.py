"""Synthetic proving keys for the key check, and the report a Python model gives them: the shared fixtures of
tests/test_key_check_host.py (CPU) and tests/test_key_check_gpu.py.

A check takes a descriptor, so the inputs are keys, not circuits: A, H, L and vk_abc entries are small multiples of g1, the B entries
are s_i g1 / s_i g2 for the same s_i, beta and delta are the same multiple in both groups.  Every point is a Pt: the limbs that go to
the library, the code pyref gives it (point_check_fixtures.pyref_code: on_curve, ec_mul(r, .); 2 for limbs that are not reduced, by
construction) and the multiple k of its group's generator (None where there is none: a refused point).  The model never multiplies a
point: a pair relation holds iff the multiples agree, the B relation iff sum rho_i s1_i = sum rho_i s2_i (mod r)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import pyref as R
from tests import point_check_fixtures as P
from tests import verify_fixtures as V
from tests.helpers import aff_limbs

Pt = namedtuple("Pt", "limbs code k")

ELEMENTS = ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2", "a_query", "b_g2_query", "b_g1_query", "h_query", "l_query", "vk_abc")
G2_ELEMENTS = ("beta_g2", "delta_g2", "b_g2_query")
SINGLE = ELEMENTS[:5]
A, B_G2, B_G1, H, L, VK_ABC = 5, 6, 7, 8, 9, 10          # ZKHIP_KEY_* of the vectors
INFINITY = Pt(np.zeros(24, dtype=np.uint64), 0, 0)


@functools.lru_cache(maxsize=None)
def multiple(k, g2):
    """k times the generator of G1 / G2, its code from pyref (0: these are the points a check must pass)"""
    pt = (V.g2mul if g2 else V.g1mul)(k)
    return Pt(aff_limbs(pt), P.pyref_code(pt, g2), k % R.R_MOD)


def refused(elem):
    """a Pt from an Elem of point_check_fixtures.bad_points"""
    assert elem.code >= P.ENCODING
    return Pt(elem.limbs, elem.code, None)


class Key:
    """n_vars, n_primary, domain_size and the eleven elements as lists of Pt"""

    def __init__(self, n_vars, n_primary, domain_size, el):
        self.n_vars, self.n_primary, self.domain_size, self.el = n_vars, n_primary, domain_size, el

    def replace(self, name, index, pt):
        el = {k: list(v) for k, v in self.el.items()}
        el[name][index] = pt
        return Key(self.n_vars, self.n_primary, self.domain_size, el)

    def arrays(self):
        """(pk dict as zkhip.Crs takes it, vk_abc)"""
        arr = lambda pts: np.array([p.limbs for p in pts], dtype=np.uint64).reshape(-1, 24)
        pk = {k: arr(self.el[k]).reshape(24) for k in SINGLE}
        pk.update(A=arr(self.el["a_query"]), B2=arr(self.el["b_g2_query"]), B1=arr(self.el["b_g1_query"]), H=arr(self.el["h_query"]),
                  L=arr(self.el["l_query"]))
        return pk, arr(self.el["vk_abc"])


def synthetic_key(n_vars=6, n_primary=1, domain_size=8, seed=3, infinity=()):
    """A key every check passes.  infinity: indices at which A, B-G1 and B-G2 are the point at infinity (as an unused variable's are)."""
    import random
    rng = random.Random(seed)
    small = lambda: rng.randrange(2, 1 << 12)
    g1 = lambda k: multiple(k, False)
    g2 = lambda k: multiple(k, True)
    b, d = small(), small()
    s = [small() for _ in range(n_vars)]
    el = dict(alpha_g1=[g1(small())], beta_g1=[g1(b)], beta_g2=[g2(b)], delta_g1=[g1(d)], delta_g2=[g2(d)],
              a_query=[INFINITY if i in infinity else g1(small()) for i in range(n_vars)],
              b_g2_query=[INFINITY if i in infinity else g2(s[i]) for i in range(n_vars)],
              b_g1_query=[INFINITY if i in infinity else g1(s[i]) for i in range(n_vars)],
              h_query=[g1(small()) for _ in range(domain_size - 1)],
              l_query=[g1(small()) for _ in range(n_vars - n_primary - 1)],
              vk_abc=[g1(small()) for _ in range(n_primary + 1)])
    return Key(n_vars, n_primary, domain_size, el)


def rho_for(n_vars, seed=11):
    """n_vars distinct non-zero 128-bit scalars"""
    import random
    rng = random.Random(seed)
    out = []
    while len(out) < n_vars:
        r = rng.randrange(1, 1 << 128)
        if r not in out:
            out.append(r)
    return out


def structure_model(key, cs):
    """(element, first index) the rule of include/zkhip.h gives, (0, None) when the key fits.  cs: dict(A, B, C: rows of (var, coeff),
    n_vars, n_primary)."""
    m, l, n = cs["n_vars"], cs["n_primary"], len(cs["A"])
    if key.n_vars != m:
        return A, None
    if key.n_primary != l:
        return L, None
    if key.domain_size < n + l + 1:
        return H, None
    occ = {name: {i for row in cs[name] for i, c in row if (int(c, 16) if isinstance(c, str) else c) % R.R_MOD} for name in "ABC"}
    inf = lambda name, i: not key.el[name][i].limbs.any()
    for i in range(m):
        if inf("a_query", i) != (i > l and i not in occ["A"]):
            return A, i
    for code, name in ((B_G2, "b_g2_query"), (B_G1, "b_g1_query")):
        for i in range(m):
            if inf(name, i) != (i not in occ["B"]):
                return code, i
    for i in range(key.domain_size - 1):
        if inf("h_query", i):
            return H, i
    for i in range(l + 1, m):
        if inf("l_query", i - l - 1) != (i not in occ["A"] | occ["B"] | occ["C"]):
            return L, i - l - 1
    for i in range(len(key.el["vk_abc"])):
        if inf("vk_abc", i):
            return VK_ABC, i
    return 0, None


def model_report(key, rho, cs=None, with_vk_abc=True):
    """What zkhip.KeyReport.fields() must be for this key, from the Pts' codes and multiples alone."""
    elements, clean = {}, {}
    for name in ELEMENTS:
        pts = key.el[name] if (with_vk_abc or name != "vk_abc") else []
        bad = [i for i, p in enumerate(pts) if p.code]
        elements[name] = (len(pts), sum(1 for p in pts if not p.code and not p.limbs.any()),
                          tuple(sum(1 for p in pts if p.code == c) for c in (P.ENCODING, P.OFF_CURVE, P.NOT_ORDER_R)),
                          bad[0] if bad else None, pts[bad[0]].code if bad else 0)
        clean[name] = not bad
    pairs = evaluated = 0
    for bit, (n1, n2) in enumerate((("beta_g1", "beta_g2"), ("delta_g1", "delta_g2"))):
        if clean[n1] and clean[n2]:
            evaluated |= 1 << bit
            if key.el[n1][0].k != key.el[n2][0].k:
                pairs |= 1 << bit
    if clean["b_g1_query"] and clean["b_g2_query"]:
        evaluated |= 4
        s1 = sum(r * p.k for r, p in zip(rho, key.el["b_g1_query"])) % R.R_MOD
        s2 = sum(r * p.k for r, p in zip(rho, key.el["b_g2_query"])) % R.R_MOD
        if s1 != s2:
            pairs |= 4
    mism = [i for i, (p1, p2) in enumerate(zip(key.el["b_g1_query"], key.el["b_g2_query"])) if p1.limbs.any() != p2.limbs.any()]
    structure, first = structure_model(key, cs) if cs is not None else (0, None)
    ok = all(clean.values()) and pairs == 0 and evaluated == 7 and not mism and structure == 0
    return dict(elements=elements, pairs=pairs, pairs_evaluated=evaluated, b_infinity_mismatch=mism[0] if mism else None,
                structure=structure, structure_first=first, ok=int(ok))


def check(zk, key, rho, host, cs_desc=None, with_vk_abc=True):
    """the library's report for a Key, as plain values"""
    pk, abc = key.arrays()
    rep = zk.check_key((pk, key.n_vars, key.n_primary, key.domain_size), vk_abc=abc if with_vk_abc else None, r1cs=cs_desc, rho=rho, host=host)
    return rep.fields()


def gpu_key(zk, n_vars, n_primary=1, seed=5):
    """A longer key every check passes, its points from the library's fixed-base kernel (multiples of the generators: code 0 and a
    known k by construction).  The H query is as long as the first power of two above n_vars allows."""
    import random
    rng = random.Random(seed)
    can = lambda xs: np.array([R.int_to_limbs(x % R.R_MOD, 6) for x in xs], dtype=np.uint64).reshape(-1, 6)
    g1l, g2l = aff_limbs(R.G1_GEN), aff_limbs(R.G2_GEN)

    def mul(g2, ks):
        if not ks:
            return []
        pts = zk.fixed_base_mul(g2l if g2 else g1l, can(ks), montgomery=False)
        return [Pt(np.array(p, dtype=np.uint64), 0, k % R.R_MOD) for p, k in zip(pts, ks)]

    rnd = lambda n: [rng.randrange(1, R.R_MOD) for _ in range(n)]
    b, d = rnd(2)
    s = rnd(n_vars)
    # a domain of 2^k points with an H query of 2^k - 1 entries: the first power of two above n_vars
    dom = 1
    while dom - 1 < n_vars:
        dom *= 2
    el = dict(alpha_g1=mul(False, rnd(1)), beta_g1=mul(False, [b]), beta_g2=mul(True, [b]), delta_g1=mul(False, [d]), delta_g2=mul(True, [d]),
              a_query=mul(False, rnd(n_vars)), b_g2_query=mul(True, s), b_g1_query=mul(False, s), h_query=mul(False, rnd(dom - 1)),
              l_query=mul(False, rnd(n_vars - n_primary - 1)), vk_abc=mul(False, rnd(n_primary + 1)))
    return Key(n_vars, n_primary, dom, el)


@functools.lru_cache(maxsize=None)
def report_cases():
    """[(label, Key, rho)]: the keys both routes are pinned on.  rho: distinct caller scalars, the same for both sums and both routes."""
    key = synthetic_key()
    rho = tuple(rho_for(key.n_vars))
    bad = {g2: [refused(e) for e in P.bad_points(g2)] for g2 in (False, True)}
    kind = lambda name, j: bad[name in G2_ELEMENTS][j % 8]
    out = [("clean", key, rho), ("clean, unused variables at infinity", synthetic_key(infinity=(2, 5)), rho)]
    # each kind of bad point in each of the ten elements: key j holds kind (j + e) % 8 in element e, at index j % its length
    for j in range(8):
        k = key
        for e, name in enumerate(ELEMENTS[:10]):
            k = k.replace(name, j % len(key.el[name]), kind(name, j + e))
        out.append(("kind %d + e in every element" % j, k, rho))
    # one refusal alone, per element: the other relations are still evaluated
    for e, name in enumerate(ELEMENTS):
        out.append(("%s alone: %d" % (name, e), key.replace(name, len(key.el[name]) - 1, kind(name, e)), rho))
    out.append(("a G1 point in b_g2_query", key.replace("b_g2_query", 3, refused(P.bad_points(True)[5])), rho))
    assert P.bad_points(True)[5].code == P.OFF_CURVE
    out.append(("refused at index 0", key.replace("a_query", 0, kind("a_query", 0)), rho))
    out.append(("refused at the last index", key.replace("a_query", key.n_vars - 1, kind("a_query", 4)), rho))
    out.append(("two refusals in one vector", key.replace("h_query", 5, kind("h_query", 6)).replace("h_query", 2, kind("h_query", 1)), rho))
    for i in (0, 3, key.n_vars - 1):
        out.append(("b_g2_query[%d] another multiple" % i, key.replace("b_g2_query", i, multiple(4099 + i, True)), rho))
    out.append(("beta_g2 another multiple", key.replace("beta_g2", 0, multiple(4111, True)), rho))
    out.append(("delta_g1 another multiple", key.replace("delta_g1", 0, multiple(4112, False)), rho))
    b1 = key.el["b_g1_query"]
    out.append(("b_g1_query 1 and 4 swapped", key.replace("b_g1_query", 1, b1[4]).replace("b_g1_query", 4, b1[1]), rho))
    out.append(("infinity mismatch", key.replace("b_g1_query", 2, INFINITY), rho))
    out.append(("refused B point", key.replace("b_g1_query", 1, kind("b_g1_query", 0)), rho))
    out.append(("empty l_query", synthetic_key(n_vars=3, n_primary=2, domain_size=4, seed=4), rho[:3]))
    k = key
    for i in range(key.n_vars):
        k = k.replace("a_query", i, INFINITY)
    out.append(("a_query all infinity", k, rho))
    for i in range(key.n_vars):
        k = k.replace("b_g1_query", i, INFINITY).replace("b_g2_query", i, INFINITY)
    out.append(("a and both b queries all infinity", k, rho))
    return out


def golden_small():
    """(Key, cs dict, CSR triples) of tests/golden/groth16_small.json: a real key with its own system"""
    from tests.helpers import csr_from_rows, golden, pt_from_json
    g = golden("groth16_small.json")
    pt = lambda p, g2: Pt(aff_limbs(pt_from_json(p)), 0, None)
    pk = g["pk"]
    el = {k: [pt(pk[k], k in G2_ELEMENTS)] for k in SINGLE}
    el.update(a_query=[pt(p, False) for p in pk["A"]], b_g2_query=[pt(p, True) for p in pk["B2"]], b_g1_query=[pt(p, False) for p in pk["B1"]],
              h_query=[pt(p, False) for p in pk["H"]], l_query=[pt(p, False) for p in pk["L"]], vk_abc=[pt(p, False) for p in g["vk"]["ABC"]])
    cs = dict(A=g["A"], B=g["B"], C=g["C"], n_vars=len(g["z"]), n_primary=g["n_primary"])
    return Key(len(g["z"]), g["n_primary"], 1 << g["log_d"], el), cs


def cs_desc(zk, cs):
    """the (desc, keep) of zkhip.make_r1cs_desc for a cs dict"""
    from tests.helpers import csr_from_rows
    return zk.make_r1cs_desc(*(csr_from_rows(cs[k]) for k in "ABC"), cs["n_vars"], cs["n_primary"])
