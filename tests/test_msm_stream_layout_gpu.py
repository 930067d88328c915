"""How a handle-owned MSM stream (zkhip_msm_stream_*) lays out the HIP streams of its contexts (api_msm.hip msm_stream_layout;
DESIGN.md section 10): a pair per context at its first submit (0), all primaries and then all secondaries when the stream is made
(1), primaries only with a context's whole launch sequence on it (2).  The layout decides where the runtime's hardware queues see
the launches - never what they compute: every result here is compared exactly with the closed form (sum s_i k_i) G.

One table-backed base set of known multiples of G (tests/msm_cases.py) serves four scalar vectors built digit by digit as in
tests/test_msm_lockstep_gpu.py, two that the lockstep route of the Edwards accumulation takes (with the threshold on the non-empty
buckets lowered to 1) and two that it does not.  Every slot of a stream sees them in turn, so a context's flag word, bucket slots
and stitching lists carry nothing into its next launch under any layout.  Which vectors are eligible is asserted on the host, from
their histograms against the cap (counts_of); the route a stream's context took cannot be read back (last_acc_path serves the
single-MSM entry points only), so the alternation of routes is that of the inputs, not one observed on the device."""
import pytest

from tests import msm_cases as M
from tests.test_msm_lockstep_gpu import CAP, CASES, counts_of

pytestmark = pytest.mark.gpu

LAYOUTS = (0, 1, 2)             # every variant the library ships
C = 8
SEQ = ("mixed_cap", "cap_plus_one", "uniform", "witness_like")       # eligible, not, eligible, not


@pytest.fixture(scope="module")
def vectors(zk, oracle_lib):
    """the base set (each case's multiples in a range of its own), one device vector per case (scalar 0 outside its range), the
    closed forms, computed once, and the length of SEQ[0]'s range, which starts the set: an MSM over that prefix alone"""
    made, start, all_ks = {}, {}, []
    for name in SEQ:
        c, ks, scal = CASES[name][0]()
        assert c == C and 256 <= len(ks) <= 4096
        cnt, _ = counts_of(ks, scal, c)
        assert (max(cnt) <= CAP) == bool(CASES[name][1])
        made[name] = (ks, scal)
        start[name] = len(all_ks)
        all_ks += ks
    zk.set_table_model(1)
    try:
        b = zk.Bases.upload(M.bases_of(oracle_lib, all_ks)).precompute(C)
    finally:
        zk.set_table_model(-1)
    assert b.table_model == 1
    dev, exp = {}, {}
    for name in SEQ:
        ks, scal = made[name]
        full = [0] * len(all_ks)
        full[start[name]:start[name] + len(scal)] = scal
        dev[name] = zk.DeviceBuffer(M.canonical_limbs(full))
        exp[name] = M.closed_form(oracle_lib, ks, scal)
    yield b, len(all_ks), dev, exp, len(made[SEQ[0]][0])
    for d in dev.values():
        d.free()
    b.free()


@pytest.fixture
def knobs(zk):
    zk.set_lockstep(1, 1)
    yield
    zk.set_lockstep(-1, -1)
    zk.set_msm_stream_layout(-1)


def _stream(zk, b, depth, layout):
    zk.set_msm_stream_layout(layout)
    try:
        return zk.MsmStream(b, depth=depth)
    finally:
        zk.set_msm_stream_layout(-1)


@pytest.mark.parametrize("depth", (1, 3, 16))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_slot_alternates_routes_under_every_layout(zk, vectors, knobs, layout, depth):
    b, n, dev, exp, _ = vectors
    stream = _stream(zk, b, depth, layout)
    try:
        # submit() takes the lowest free slot: a full round fills slots 0 .. depth - 1 in order; round r gives slot k the vector
        # SEQ[(k + r) % 4], so every slot alternates between an eligible and an ineligible launch
        for r in range(4):
            names = [SEQ[(k + r) % 4] for k in range(depth)]
            tickets = [stream.submit(dev[nm].ptr, n, montgomery=False) for nm in names]
            with pytest.raises(zk.ZkhipError):
                stream.submit(dev[SEQ[0]].ptr, n, montgomery=False)             # every slot is in flight
            if r % 2 == 0:                                                       # by ticket, newest first
                for t, nm in reversed(list(zip(tickets, names))):
                    assert (zk.jac_to_affine(stream.collect(t)) == exp[nm]).all(), (r, nm)
            else:                                                                # "the oldest", after one taken from the middle
                mid = depth // 2
                assert (zk.jac_to_affine(stream.collect(tickets[mid])) == exp[names[mid]]).all(), (r, names[mid])
                for k in range(depth):
                    if k != mid:
                        assert (zk.jac_to_affine(stream.collect(None)) == exp[names[k]]).all(), (r, k, names[k])
            with pytest.raises(zk.ZkhipError):
                stream.collect(None)                                             # nothing in flight
    finally:
        stream.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_stream_freed_with_launches_pending_and_slots_unused(zk, vectors, knobs, layout):
    b, n, dev, exp, _ = vectors
    stream = _stream(zk, b, 16, layout)
    for nm in SEQ[:3]:
        stream.submit(dev[nm].ptr, n, montgomery=False)          # three of sixteen slots planned, none collected
    stream.free()
    unused = _stream(zk, b, 16, layout)                          # and one that never saw a launch
    unused.free()
    again = _stream(zk, b, 2, layout)
    try:
        t0, t1 = (again.submit(dev[nm].ptr, n, montgomery=False) for nm in ("witness_like", "uniform"))
        assert (zk.jac_to_affine(again.collect(t1)) == exp["uniform"]).all()
        assert (zk.jac_to_affine(again.collect(t0)) == exp["witness_like"]).all()
    finally:
        again.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_slot_planned_again_for_a_longer_msm_keeps_its_streams(zk, vectors, knobs, layout):
    """A slot's plan is sized by its first launch; a longer one makes it again.  The plan owns memory only: the slot's HIP streams and
    events are its lane's, which the stream holds from zkhip_msm_stream_new (layouts 1 and 2) or the slot's first submit (layout 0)
    until free(), so the new plan runs where the old one did - here for slot 0 with nothing in flight, for slot 1 while slot 0's
    long MSM is pending -, and free() afterwards destroys every lane once: a stream made after it works."""
    b, n, dev, exp, short = vectors
    assert short < n
    first = SEQ[0]                                               # its range is the prefix [0, short) of the base set
    stream = _stream(zk, b, 2, layout)
    try:
        for rnd in range(2):                                     # short, long (planned again), short (the long plan serves it), long
            ts = [stream.submit(dev[first].ptr, short, montgomery=False) for _ in range(2)]
            for t in ts:
                assert (zk.jac_to_affine(stream.collect(t)) == exp[first]).all(), (rnd, "short")
            names = ("witness_like", "uniform")
            ts = [stream.submit(dev[nm].ptr, n, montgomery=False) for nm in names]
            for t, nm in reversed(list(zip(ts, names))):
                assert (zk.jac_to_affine(stream.collect(t)) == exp[nm]).all(), (rnd, nm)
    finally:
        stream.free()
    again = _stream(zk, b, 2, layout)
    try:
        t = again.submit(dev["mixed_cap"].ptr, n, montgomery=False)
        assert (zk.jac_to_affine(again.collect(t)) == exp["mixed_cap"]).all()
    finally:
        again.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_slot_planned_again_while_its_neighbour_is_in_flight(zk, vectors, knobs, layout):
    """Slot 0 is planned for a prefix longer than `short`, serves the short prefix with that plan, and - with slot 1's launch (a plan
    of the same length, made while slot 0's was pending) still in flight - is given the whole set: its plan is made again on its own
    lane while the neighbour's lane is busy.  Collected newest first."""
    b, n, dev, exp, short = vectors
    first = SEQ[0]                                               # zero outside [0, short): every prefix from `short` on has its sum
    mid = (short + n) // 2
    assert short < mid < n
    stream = _stream(zk, b, 2, layout)
    try:
        t = stream.submit(dev[first].ptr, mid, montgomery=False)                 # slot 0: planned for mid
        assert (zk.jac_to_affine(stream.collect(t)) == exp[first]).all(), "long"
        t_short = stream.submit(dev[first].ptr, short, montgomery=False)         # slot 0: the long plan serves it
        t_mid = stream.submit(dev[first].ptr, mid, montgomery=False)             # slot 1: planned for mid, slot 0 pending
        assert (zk.jac_to_affine(stream.collect(t_short)) == exp[first]).all(), "short"
        t_all = stream.submit(dev["uniform"].ptr, n, montgomery=False)           # slot 0: planned again, slot 1 pending
        with pytest.raises(zk.ZkhipError):
            stream.submit(dev[first].ptr, short, montgomery=False)               # (both slots in flight)
        assert (zk.jac_to_affine(stream.collect(t_all)) == exp["uniform"]).all(), "whole set"
        assert (zk.jac_to_affine(stream.collect(t_mid)) == exp[first]).all(), "neighbour"
    finally:
        stream.free()
