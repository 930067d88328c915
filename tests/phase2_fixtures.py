"""Phase-2 contributions on synthetic keys, and the report a Python model gives them: the shared fixtures of
tests/test_phase2_host.py (CPU) and tests/test_phase2_gpu.py.  Built on tests/key_check_fixtures.py: every point is a Pt (limbs, the code
pyref gives it, the multiple k of its group's generator), so the model never multiplies a point - the delta pair holds iff the multiples
agree, the ratio iff sum rho_i k'_i delta' = sum rho_i k_i delta (mod r), the proof of knowledge iff z delta = t + c delta' (mod r)
with c from hashlib."""
import functools
import hashlib
import struct

import numpy as np

from oracle import pyref as R
from tests import key_check_fixtures as K
from tests import point_check_fixtures as P
from tests.helpers import aff_limbs, fr_limbs

RM = R.R_MOD
ZERO_DIGEST = b"\0" * 32
ELEMENTS = ("delta_g1", "delta_g2", "h", "l", "pok_commit")
UNCHANGED = (("alpha_g1", 0), ("beta_g1", 1), ("beta_g2", 2), ("a_query", K.A), ("b_g2_query", K.B_G2), ("b_g1_query", K.B_G1))
S1, K1 = 0x1234567 * 3 ** 150 % RM, 0x7654321 * 5 ** 120 % RM      # a secret and a nonce, full size
S2, K2 = 7 ** 130 % RM, 11 ** 100 % RM
S3, K3 = 13 ** 99 % RM, 17 ** 90 % RM


def _fnv1a(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def key_file_bytes(key):
    """the keypair file of a Key (the container of zkhip_keypair_write: header, the eleven arrays, FNV-1a)"""
    pk, abc = key.arrays()
    parts = [pk[k].reshape(-1, 24) for k in K.SINGLE] + [pk[k] for k in ("A", "B2", "B1", "H", "L")] + [abc]
    body = b"ZKHIPKP1" + struct.pack("<7Q", key.n_vars, key.n_primary, key.domain_size, 0, 0, 0, 0) + b"".join(
        np.ascontiguousarray(p, dtype="<u8").tobytes() for p in parts)
    return body + struct.pack("<Q", _fnv1a(body))


def keypair_of(zk, key, tmp_path, name="key.bin"):
    """a zkhip.Keypair that holds exactly the Key's limbs (through the key file: host code)"""
    path = tmp_path / name
    path.write_bytes(key_file_bytes(key))
    return zk.Keypair.read(path)


def pt_bytes(pt):
    return np.ascontiguousarray(pt.limbs, dtype="<u8").tobytes()


class Record:
    """a contribution record in the model: three Pts and the response z as an integer (canonical)"""

    def __init__(self, delta_g1, delta_g2, commit, z):
        self.delta_g1, self.delta_g2, self.commit, self.z = delta_g1, delta_g2, commit, z

    def replace(self, **kw):
        d = dict(delta_g1=self.delta_g1, delta_g2=self.delta_g2, commit=self.commit, z=self.z)
        d.update(kw)
        return Record(**d)

    def to_bytes(self):
        assert 0 <= self.z < 1 << 384
        return pt_bytes(self.delta_g1) + pt_bytes(self.delta_g2) + pt_bytes(self.commit) + self.z.to_bytes(48, "little")

    def struct(self, zk):
        return zk.Contribution.from_bytes(self.to_bytes())


def challenge(prev, delta_g1, delta_g1_new, commit):
    h = hashlib.sha256(b"zkhip phase2 pok v1" + prev + pt_bytes(delta_g1) + pt_bytes(delta_g1_new) + pt_bytes(commit)).digest()
    return int.from_bytes(h[:16], "little")


def link(prev, record):
    return hashlib.sha256(b"zkhip phase2 link v1" + prev + record.to_bytes()).digest()


def with_infinite_l(key, indices=(1,)):
    """the key with L entries at infinity (a variable no constraint uses)"""
    for i in indices:
        key = key.replace("l_query", i, K.INFINITY)
    return key


def pyref_mul(ms, g2):
    """the multiples ms of a generator as Pts, by pyref (cached)"""
    return [K.multiple(m % RM, g2) for m in ms]


def library_mul(zk):
    """the same from the library's fixed-base kernel in one launch (tests/key_check_fixtures.py gpu_key makes its keys this way): a long
    key's few hundred full-size multiples would take pyref a quarter of a minute"""
    def mul(ms, g2):
        if not ms:
            return []
        can = np.array([R.int_to_limbs(m % RM, 6) for m in ms], dtype=np.uint64).reshape(-1, 6)
        pts = zk.fixed_base_mul(aff_limbs(R.G2_GEN if g2 else R.G1_GEN), can, montgomery=False)
        return [K.Pt(np.array(p, dtype=np.uint64), 0, m % RM) if m % RM else K.INFINITY for p, m in zip(pts, ms)]
    return mul


def contribute_model(key, s, k, prev, mul=pyref_mul):
    """(the Key after the contribution, its Record, the new digest) for a key whose delta, H and L points have known multiples"""
    sinv = pow(s, -1, RM)
    d = key.el["delta_g1"][0].k
    assert d == key.el["delta_g2"][0].k
    el = {name: list(v) for name, v in key.el.items()}
    el["delta_g1"], el["delta_g2"] = mul([d * s], False), mul([d * s], True)
    for name in ("h_query", "l_query"):
        finite = [i for i, p in enumerate(key.el[name]) if p.limbs.any()]
        for i, pt in zip(finite, mul([key.el[name][i].k * sinv for i in finite], False)):
            el[name][i] = pt
    after = K.Key(key.n_vars, key.n_primary, key.domain_size, el)
    commit = mul([k * d], False)[0]
    c = challenge(prev, key.el["delta_g1"][0], el["delta_g1"][0], commit)
    rec = Record(el["delta_g1"][0], el["delta_g2"][0], commit, (k + c * s) % RM)
    return after, rec, link(prev, rec)


def rho_for(key, seed=17):
    return K.rho_for((key.domain_size - 1) + (key.n_vars - key.n_primary - 1), seed)


def model_report(before, after, rec, prev, rho):
    """What zkhip.Phase2Report.fields() must be, and the digest (None unless ok), from the Pts' limbs, codes and multiples alone."""
    none_el = {name: (0, 0, (0, 0, 0), None, 0) for name in ELEMENTS}
    if (before.n_vars, before.n_primary, before.domain_size) != (after.n_vars, after.n_primary, after.domain_size):
        return dict(changed=1 << 31, elements=none_el, infinity_mismatch=0, infinity_mismatch_first=None, relations=0, relations_evaluated=0, ok=0), None
    same = lambda a, b: len(a) == len(b) and all((p.limbs == q.limbs).all() for p, q in zip(a, b))
    changed = sum(1 << bit for name, bit in UNCHANGED if not same(before.el[name], after.el[name]))
    changed |= (0 if same([rec.delta_g1], after.el["delta_g1"]) else 1 << 3) | (0 if same([rec.delta_g2], after.el["delta_g2"]) else 1 << 4)
    pts = dict(delta_g1=after.el["delta_g1"], delta_g2=after.el["delta_g2"], h=after.el["h_query"], l=after.el["l_query"], pok_commit=[rec.commit])
    elements, clean, finite = {}, {}, {}
    for name in ELEMENTS:
        bad = [i for i, p in enumerate(pts[name]) if p.code]
        n_inf = sum(1 for p in pts[name] if not p.code and not p.limbs.any())
        elements[name] = (len(pts[name]), n_inf, tuple(sum(1 for p in pts[name] if p.code == c) for c in (P.ENCODING, P.OFF_CURVE, P.NOT_ORDER_R)),
                          bad[0] if bad else None, pts[name][bad[0]].code if bad else 0)
        clean[name], finite[name] = not bad, n_inf == 0
    mism, first = 0, None
    for code, name in ((K.H, "h_query"), (K.L, "l_query")):
        bad = [i for i, (p, q) in enumerate(zip(before.el[name], after.el[name])) if p.limbs.any() != q.limbs.any()]
        if bad and not mism:
            mism, first = code, bad[0]
    points_ok = all(clean.values()) and not mism and finite["delta_g1"] and finite["delta_g2"] and finite["pok_commit"]
    d_old, d1, d2 = before.el["delta_g1"][0].k, after.el["delta_g1"][0].k, after.el["delta_g2"][0].k
    relations = evaluated = 0
    if clean["delta_g1"] and clean["delta_g2"] and finite["delta_g1"] and finite["delta_g2"]:
        evaluated |= 1
        relations |= 0 if d1 == d2 else 1
    if points_ok:
        evaluated |= 2
        s_old = sum(r * p.k for r, p in zip(rho, before.el["h_query"] + before.el["l_query"]))
        s_new = sum(r * p.k for r, p in zip(rho, after.el["h_query"] + after.el["l_query"]))
        relations |= 0 if (s_new * d2 - s_old * before.el["delta_g2"][0].k) % RM == 0 else 2
    if clean["delta_g1"] and clean["pok_commit"] and finite["delta_g1"] and finite["pok_commit"]:
        evaluated |= 4
        c = challenge(prev, before.el["delta_g1"][0], after.el["delta_g1"][0], rec.commit)      # (the new KEY's delta: the checked one)
        holds = rec.z < RM and (rec.z * d_old - rec.commit.k - c * d1) % RM == 0
        relations |= 0 if holds else 4
    ok = int(changed == 0 and points_ok and relations == 0 and evaluated == 7)
    return dict(changed=changed, elements=elements, infinity_mismatch=mism, infinity_mismatch_first=first, relations=relations,
                relations_evaluated=evaluated, ok=ok), (link(prev, rec) if ok else None)


def verify(zk, before, after, rec, prev, rho, host):
    """the library's report for Keys and a Record, as plain values, and its digest"""
    desc = lambda key: (key.arrays()[0], key.n_vars, key.n_primary, key.domain_size)
    rep, digest = zk.phase2_verify(desc(before), desc(after), rec.struct(zk), prev, rho=rho, host=host)
    return rep.fields(), digest


def tamperings(before, after, rec, prev, mul=pyref_mul):
    """[(label, before, after, Record, prev_digest)]: the honest contribution and every way of spoiling it that a verifier must catch.
    Every replaced point has a known multiple (or is a refused point of point_check_fixtures.bad_points)."""
    g1, g2 = (lambda m: mul([m], False)[0]), (lambda m: mul([m], True)[0])
    nh, nl = len(after.el["h_query"]), len(after.el["l_query"])
    out = [("honest", before, after, rec, prev)]
    def ends_and_middle(name):      # the first, a middle and the last index that holds a finite point
        f = [i for i, p in enumerate(after.el[name]) if p.limbs.any()]
        return sorted({f[0], f[len(f) // 2], f[-1]})
    for i in ends_and_middle("l_query"):
        out.append(("l'[%d] another multiple" % i, before, after.replace("l_query", i, g1(4099 + i)), rec, prev))
    for i in ends_and_middle("h_query"):
        out.append(("h'[%d] by another scalar" % i, before, after.replace("h_query", i, g1(before.el["h_query"][i].k * pow(S2, -1, RM))), rec, prev))
    d = after.el["delta_g1"][0].k
    out.append(("delta_g2' another multiple", before, after.replace("delta_g2", 0, g2(d + 1)), rec.replace(delta_g2=g2(d + 1)), prev))
    out.append(("delta' another common multiple", before, after.replace("delta_g1", 0, g1(d + 1)).replace("delta_g2", 0, g2(d + 1)),
                rec.replace(delta_g1=g1(d + 1), delta_g2=g2(d + 1)), prev))
    out.append(("the record's delta_g1 is not the key's", before, after, rec.replace(delta_g1=g1(d + 1)), prev))
    out.append(("a_query[0] changed", before, after.replace("a_query", 0, g1(5003)), rec, prev))
    out.append(("beta_g2 changed", before, after.replace("beta_g2", 0, g2(5004)), rec, prev))
    out.append(("n_primary changed", before, K.Key(after.n_vars, after.n_primary + 1, after.domain_size,
                                                   dict(after.el, l_query=after.el["l_query"][:-1])), rec, prev))
    finite_l = [i for i, p in enumerate(after.el["l_query"]) if p.limbs.any()]
    out.append(("an l' entry set to infinity", before, after.replace("l_query", finite_l[-1], K.INFINITY), rec, prev))
    inf_l = [i for i, p in enumerate(after.el["l_query"]) if not p.limbs.any()]
    if inf_l:
        out.append(("an infinite l' entry made finite", before, after.replace("l_query", inf_l[0], g1(5005)), rec, prev))
    finite_h = [i for i, p in enumerate(after.el["h_query"]) if p.limbs.any()]
    out.append(("an h' entry set to infinity", before, after.replace("h_query", finite_h[-1], K.INFINITY), rec, prev))
    out.append(("delta' at infinity", before, after.replace("delta_g1", 0, K.INFINITY).replace("delta_g2", 0, K.INFINITY),
                rec.replace(delta_g1=K.INFINITY, delta_g2=K.INFINITY), prev))
    out.append(("the commitment at infinity", before, after, rec.replace(commit=K.INFINITY), prev))
    for j, e in enumerate(P.bad_points(False)):
        bad = K.refused(e)
        out.append(("h'[%d]: %s" % (j % nh, e.name), before, after.replace("h_query", j % nh, bad), rec, prev))
        out.append(("l'[%d]: %s" % (j % nl, e.name), before, after.replace("l_query", j % nl, bad), rec, prev))
        out.append(("delta_g1': %s" % e.name, before, after.replace("delta_g1", 0, bad), rec.replace(delta_g1=bad), prev))
        out.append(("T: %s" % e.name, before, after, rec.replace(commit=bad), prev))
    out.append(("a G1 point as delta_g2'", before, after.replace("delta_g2", 0, K.refused(P.bad_points(True)[5])),
                rec.replace(delta_g2=K.refused(P.bad_points(True)[5])), prev))
    out.append(("pok_response + 1", before, after, rec.replace(z=(rec.z + 1) % RM), prev))
    out.append(("pok_response >= r", before, after, rec.replace(z=rec.z + RM), prev))
    out.append(("another prev_digest", before, after, rec, hashlib.sha256(b"another transcript").digest()))
    other, _, _ = contribute_model(before, S3, K3, prev, mul)      # a valid key of the same chain: only the proof of knowledge can tell
    out.append(("replayed on another before", other, after, rec, prev))
    return out


@functools.lru_cache(maxsize=None)
def host_cases():
    """[(label, before, after, Record, prev, rho)] on the synthetic key, without and with entries of L at infinity"""
    out = []
    for tag, key in (("", K.synthetic_key()), ("inf: ", with_infinite_l(K.synthetic_key(infinity=(2, 5))))):
        after, rec, _ = contribute_model(key, S1, K1, ZERO_DIGEST)
        rho = tuple(rho_for(key))
        out += [(tag + label, b, a, r, p, rho) for label, b, a, r, p in tamperings(key, after, rec, ZERO_DIGEST)]
    return out


def scalar_limbs(x):
    """a scalar as the six Montgomery limbs contribute takes"""
    return fr_limbs(x % RM)
