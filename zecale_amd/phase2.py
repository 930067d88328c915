"""Phase-2 contributions from the command line: one participant's turn of a circuit-specific ceremony, and the coordinator's check.

  python -m zecale_amd.phase2 contribute IN.key OUT.key --transcript T.json [--host]
  python -m zecale_amd.phase2 verify BEFORE.key AFTER.key --transcript T.json [--index N] [--host]

contribute reads a keypair file (zkhip_keypair_write's container), multiplies delta by a secret drawn from the OS - which nobody ever
sees and which is gone when the command returns -, writes the new keypair and appends the contribution's record to the transcript.
verify checks the chain of digests through the whole transcript, and that AFTER is an honest contribution on top of BEFORE
(zkhip_phase2_verify) under record N of it (--index, counted from 1; default: the last record).  Record 1 must start from SHA-256 of
BEFORE.  A coordinator who keeps every turn's key file runs it once per record, N = 1, 2, ...: the proof of knowledge, the ratio and
the point checks of a link all need that link's two keys.  It prints the report and exits non-zero when the link fails.

The transcript is a JSON list of records {prev_digest, delta_g1, delta_g2, pok_commit, pok_response, digest}: limbs as hex, little
endian words.  The first prev_digest is SHA-256 of the first key file.

SCOPE.  Phase 2 re-randomises delta ONLY.  A key is sound only if tau, alpha and beta are unknown as well; that takes a powers-of-tau
ceremony and the linear-combination step that turns its output into a circuit's queries, which this library does not have.  A key
from the single-party setup with contributions on top still has a tau, alpha and beta that its first author knew.
BEFORE is taken as validated already (zkhip.check_key, or an earlier accepted contribution)."""
import argparse
import hashlib
import json
import os
import sys

FIELDS = (("delta_g1", 24), ("delta_g2", 24), ("pok_commit", 24), ("pok_response", 6))


def record_to_json(rec, prev, digest):
    out = {"prev_digest": prev.hex(), "digest": digest.hex()}
    for name, n in FIELDS:
        out[name] = ["%016x" % int(v) for v in getattr(rec, name)]
    return out


def record_from_json(zk, obj):
    rec = zk.Contribution()
    for name, n in FIELDS:
        words = [int(w, 16) for w in obj[name]]
        if len(words) != n or any(w >> 64 for w in words):
            raise ValueError("transcript record: %s is not %d 64-bit words" % (name, n))
        for i, w in enumerate(words):
            getattr(rec, name)[i] = w
    return rec, bytes.fromhex(obj["prev_digest"]), bytes.fromhex(obj["digest"])


def link_digest(rec, prev):
    return hashlib.sha256(b"zkhip phase2 link v1" + prev + rec.to_bytes()).digest()


def load_transcript(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        t = json.load(f)
    if not isinstance(t, list):
        raise ValueError("the transcript is a JSON list of records")
    return t


def file_digest(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).digest()


def contribute(zk, a):
    transcript = load_transcript(a.transcript)
    prev = bytes.fromhex(transcript[-1]["digest"]) if transcript else file_digest(a.before)
    kp = zk.Keypair.read(a.before)
    new, rec, digest = kp.contribute(prev_digest=prev, host=a.host)
    new.write(a.after)
    transcript.append(record_to_json(rec, prev, digest))
    with open(a.transcript, "w") as f:
        json.dump(transcript, f, indent=1)
    print("contribution %d written: %s, digest %s" % (len(transcript), a.after, digest.hex()))
    kp.free(); new.free()
    return 0


def verify(zk, a):
    transcript = load_transcript(a.transcript)
    if not transcript:
        print("phase 2: the transcript holds no record")
        return 1
    records = [record_from_json(zk, obj) for obj in transcript]
    # the chain: every record hashes to its digest and names its predecessor's
    for i, (rec, prev, digest) in enumerate(records):
        if link_digest(rec, prev) != digest:
            print("phase 2: record %d does not hash to its digest" % (i + 1))
            return 1
        if i and prev != records[i - 1][2]:
            print("phase 2: record %d does not follow record %d" % (i + 1, i))
            return 1
    index = a.index if a.index else len(records)
    if not 1 <= index <= len(records):
        print("phase 2: the transcript holds %d record(s), there is no record %d" % (len(records), index))
        return 1
    if index == 1 and records[0][1] != file_digest(a.before):
        print("phase 2: the transcript does not start from %s" % a.before)
        return 1
    # link `index` against the two key files
    rec, prev, digest = records[index - 1]
    before, after = zk.Keypair.read(a.before), zk.Keypair.read(a.after)
    report, got = zk.phase2_verify(before, after, rec, prev, host=a.host)
    before.free(); after.free()
    print(report.describe())
    if not report.ok or got != digest:
        return 1
    print("record %d of %d, digest %s" % (index, len(records), digest.hex()))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m zecale_amd.phase2", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    for name, first, second in (("contribute", "IN.key", "OUT.key"), ("verify", "BEFORE.key", "AFTER.key")):
        p = sub.add_parser(name)
        p.add_argument("before", metavar=first)
        p.add_argument("after", metavar=second)
        p.add_argument("--transcript", required=True, metavar="T.json")
        p.add_argument("--host", action="store_true", help="the host route: no GPU")
        p.add_argument("--device", type=int, default=0)
        if name == "verify":
            p.add_argument("--index", type=int, default=0, metavar="N", help="the record BEFORE -> AFTER is (from 1; default: the last)")
    a = ap.parse_args(argv)
    from zecale_amd import zkhip as zk
    if not a.host:
        zk.init(a.device)
    try:
        return (contribute if a.command == "contribute" else verify)(zk, a)
    except (zk.ZkhipError, ValueError, KeyError) as e:
        print("phase 2: %s" % e)
        return 1


if __name__ == "__main__":
    sys.exit(main())
