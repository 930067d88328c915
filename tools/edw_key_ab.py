#!/usr/bin/env python3
"""Which kind of proving key for which workload: a one-level XYZZ key, an every-bit-position (NAF) key and an Edwards key
(zkhip_key_opts.table_model = 1), taking turns in ONE process on one GPU, medians of at least five repeats.

Legs (--legs, comma list):
  wrap   the wrapping stream (batch 2, one input per nested proof) through the pipeline at the bench's settings
  nine   the nine-input stream, the same way
  one    one 2^20 proof alone (the plain entry point; its second call on)
  five   five 2^20 proofs in flight (five prover instances, one host thread each)

Per leg and kind the report holds proofs/s (median, min .. max: the spread of the repeats), the accumulation launches' own times of one
proof alone (the sum of both sequences for an Edwards key), the entry count of the proof and the entries of each of its five MSMs -
G1's share s of the additions, which bounds what the cheaper addition can give: (1 - 0.224 s) of XYZZ's accumulation time.  Written to --out (profiles/edw_key_ab.txt holds the run this repository's figures come from)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("xyzz", "naf", "edwards")


def opts_of(zk, kind):
    if kind == "xyzz":
        return zk.key_opts(table_naf=False, table_model=0)
    if kind == "naf":
        return zk.key_opts(table_naf=True, table_model=0)
    return zk.key_opts(table_naf=False, table_model=1)


def describe(crs):
    return "tables: %s, window %d, model %s" % ({0: "none", 1: "one level per window", 2: "every bit position"}[crs.table_kind], crs.table_window,
                                                 "Edwards" if crs.table_model else "XYZZ")


def free_bytes(zk):
    import ctypes
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    lib = zk.load()
    lib.zkhip_device_memory.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    lib.zkhip_device_memory(ctypes.byref(free), ctypes.byref(total))
    return free.value


def upload_keys(zk, kp, first=None):
    """{kind: key}, {kind: GB of device memory the key took}"""
    keys, gb = {}, {}
    for k in KINDS:
        before = free_bytes(zk)
        keys[k] = first if (k == "xyzz" and first is not None) else kp.upload_crs(opts_of(zk, k))
        gb[k] = (before - free_bytes(zk)) / 1e9
    return keys, gb


def spread(vals):
    return "median %.2f  min %.2f  max %.2f  (n = %d)" % (statistics.median(vals), min(vals), max(vals), len(vals))


def proof_alone(zk, crs, r1, z, r, s):
    """accumulation time and entries of one proof alone through the plain entry point (its work space is there from an earlier call)"""
    zk.groth16_prove(crs, r1, z, r, s)
    t0 = time.time()
    proof = zk.groth16_prove(crs, r1, z, r, s)
    return proof, (time.time() - t0) * 1e3, zk.last_accumulate_ms(), zk.last_accumulate_entries(), zk.last_prove_table_model()


def entries_per_job(zk, kp, r1, z, window):
    """the bucket entries (mixed additions) of each of a proof's five MSMs at this window: every query vector once as a base set of
    its own, one MSM over it, the count read back from its sort"""
    pk, m, l, d = kp.pk_arrays()
    h = r1.qap_h(z)
    out = {}
    for name, key, scal in (("A", "A", z), ("B-G2", "B2", z), ("B-G1", "B1", z), ("H", "H", h[:d - 1]), ("L", "L", z[l + 1:])):
        b = zk.Bases.upload(pk[key]).precompute(window, table_naf=False)
        b.msm(scal)
        out[name] = zk.last_accumulate_entries()
        b.free()
    return out


def entries_line(e):
    g1 = sum(v for k, v in e.items() if k != "B-G2")
    return "  entries per job at the one-level window: %s; G1's share s = %.3f: the arithmetic promises an accumulation time of %.3f of XYZZ's" % (
        e, g1 / max(1, sum(e.values())), 1 - 0.224 * g1 / max(1, sum(e.values())))


def stream_leg(zk, bench, args, inputs_per_proof, steps, warmup, repeats, out):
    nvk_l, npr, nin, trapdoor = bench.aggregator_inputs(inputs_per_proof)
    agg = zk.AggregatorCircuit(2, inputs_per_proof)
    desc = zk.r1cs_desc_from_aggregator(agg)
    kp = zk.Keypair(desc, *trapdoor)
    r1 = zk.r1cs_from_desc(desc)
    rr, ss = bench.random_fr_uniform(5, 1)[0], bench.random_fr_uniform(6, 1)[0]
    submit = lambda p_: p_.submit(nvk_l, npr, nin, rr, ss)
    vk = kp.vk()
    keys, gb = upload_keys(zk, kp)
    z = agg.witness(nvk_l, npr, nin)
    out.append("%d inputs per nested proof: %d constraints, domain %d, finite bases A / B-G2 / B-G1 / H / L = %s" %
               (inputs_per_proof, agg.num_constraints, kp.domain_size, keys["xyzz"].finite_terms()))
    out.append(entries_line(entries_per_job(zk, kp, r1, z, keys["xyzz"].table_window)))
    ref = None
    for k in KINDS:
        proof, wall, acc, entries, model = proof_alone(zk, keys[k], r1, z, rr, ss)
        ref = proof if ref is None else ref
        assert (proof == ref).all(), "the three keys must give the same proof"
        out.append("  %-8s %s, %.2f GB; one proof alone %.2f ms, accumulation launches %.3f ms, entries %d, Edwards route %d" % (k, describe(keys[k]), gb[k], wall, acc, entries, model))
    rates = {k: [] for k in KINDS}
    for rep in range(repeats):
        for k in KINDS:                                   # the kinds take turns
            res, proof = bench.stream_rates(zk, args, agg, keys[k], vk, submit, steps, warmup, nested_vk=nvk_l)
            assert res["last_proof_verifies"] and res["result_bits"] == 3
            rates[k].append(res["value"])
    for k in KINDS:
        out.append("  %-8s stream proofs/s: %s" % (k, spread(rates[k])))
    for c in keys.values():
        c.free()
    r1.free(); kp.free(); agg.free()
    return rates


def full_size_legs(zk, bench, legs, repeats, out):
    before = free_bytes(zk)
    fs = bench.FullSizeProver(zk, 20, opts=opts_of(zk, "xyzz"))
    first_gb = (before - free_bytes(zk)) / 1e9             # (with the constraint system's buffers)
    keys, gb = upload_keys(zk, fs.kp, first=fs.crs)
    gb["xyzz"] = first_gb
    out.append("2^20 constraints: finite bases A / B-G2 / B-G1 / H / L = %s" % fs.crs.finite_terms())
    for k in KINDS:
        out.append("  %-8s %s, %.2f GB%s" % (k, describe(keys[k]), gb[k], " (with the constraint system's device buffers)" if k == "xyzz" else ""))
    out.append(entries_line(entries_per_job(zk, fs.kp, fs.r1, fs.z, fs.crs.table_window)))
    ref = None
    alone = {k: [] for k in KINDS}
    acc = {k: [] for k in KINDS}
    info = {}
    if "one" in legs:
        for rep in range(repeats):
            for k in KINDS:
                proof, wall, a, entries, model = proof_alone(zk, keys[k], fs.r1, fs.z, fs.rr, fs.ss)
                ref = proof if ref is None else ref
                assert (proof == ref).all(), "the three keys must give the same proof"
                alone[k].append(1e3 / wall); acc[k].append(a); info[k] = (entries, model)
        for k in KINDS:
            out.append("  %-8s one proof alone, proofs/s: %s; accumulation launches ms: %s; entries %d, Edwards route %d" %
                       (k, spread(alone[k]), spread(acc[k]), info[k][0], info[k][1]))
    flight = {k: [] for k in KINDS}
    if "five" in legs:
        from concurrent.futures import ThreadPoolExecutor
        provers = {k: [zk.Prover(keys[k], fs.desc) for _ in range(5)] for k in KINDS}
        for k in KINDS:
            for which in (0, 1):
                for p_ in provers[k]:
                    p_.create_streams(which)
            for p_ in provers[k]:
                p_.prove(fs.z, fs.rr, fs.ss)
        with ThreadPoolExecutor(max_workers=5) as pool:
            for rep in range(repeats):
                for k in KINDS:
                    t0 = time.time()
                    futs = [pool.submit(provers[k][i % 5].prove, fs.z, fs.rr, fs.ss) for i in range(15)]
                    last = [f.result() for f in futs][-1]
                    flight[k].append(15 / (time.time() - t0))
                    assert ref is None or (last == ref).all()
        for k in KINDS:
            out.append("  %-8s five proofs in flight, proofs/s: %s; a launch inside the stream %.3f ms" % (k, spread(flight[k]), max(p_.last_accumulate_ms() for p_ in provers[k])))
            for p_ in provers[k]:
                p_.free()
    for k in KINDS[1:]:
        keys[k].free()
    fs.free()
    return alone, flight


def verdict(name, rates, out):
    """the Edwards key is recommended only where its median beats the other kind's by more than the larger of the two spreads"""
    med = {k: statistics.median(v) for k, v in rates.items() if v}
    if "edwards" not in med:
        return
    sp = {k: max(rates[k]) - min(rates[k]) for k in med}
    best_other = max((k for k in med if k != "edwards"), key=lambda k: med[k])
    gap, need = med["edwards"] - med[best_other], max(sp["edwards"], sp[best_other])
    word = "WINS" if gap > need else ("LOSES" if -gap > need else "is within the spread of")
    out.append("  => %s: the Edwards key %s the %s key (medians %.2f against %.2f, difference %+.2f, larger spread %.2f)" %
               (name, word, best_other, med["edwards"], med[best_other], gap, need))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--legs", default="wrap,nine,one,five")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps-wrap", type=int, default=960)
    ap.add_argument("--steps-nine", type=int, default=576)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edw_key_ab.txt"))
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("medians of at least five repeats")
    legs = set(a.legs.split(","))
    import bench
    from zecale_amd import zkhip as zk
    zk.init(0)
    args = bench.parse_args([])                           # the bench's own settings: gpu slots, witness workers
    out = ["Key kinds A/B (tools/edw_key_ab.py): one process, one GPU, the kinds take turns, %d repeats each" % a.repeats, ""]
    if "wrap" in legs:
        verdict("wrapping stream", stream_leg(zk, bench, args, 1, a.steps_wrap, 96, a.repeats, out), out)
        out.append("")
    if "nine" in legs:
        verdict("nine-input stream", stream_leg(zk, bench, args, 9, a.steps_nine, 96, a.repeats, out), out)
        out.append("")
    if legs & {"one", "five"}:
        alone, flight = full_size_legs(zk, bench, legs, a.repeats, out)
        verdict("one 2^20 proof alone", alone, out)
        verdict("five 2^20 proofs in flight", flight, out)
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
