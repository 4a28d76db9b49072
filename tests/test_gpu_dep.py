"""The device dependency buffer (am_dep, materializer.DepBuffer) against tests/depsim.py served one
arrival at a time: the delivered tags per partition in order, every partition's clock and presence,
and every queue's tags.  No tolerances.  The sizes are the smallest at which the kernel can go wrong:
more partitions than a wave has lanes, queues around the 64-lane step, every group width."""
import random

import pytest

from antidote_amd import abi
from tests import depcases
from tests.depcases import Model, txn

pytestmark = pytest.mark.gpu

U64_MAX = depcases.U64_MAX
CASES = depcases.hand_cases()


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def check(mat, script, n_dc, own=0, n_part=1, order=None, cap=None):
    """The script on the device and on DepSim: deliveries of every call, then clocks and queues."""
    n = sum(len(c[1]) for c in script if c[0] == "deliver")
    dev, sim = mat.dep_buffer(n_dc, own, n_part, cap or max(n, 1), order), Model(n_dc, own, n_part, order)
    try:
        for i, cmd in enumerate(script):
            got, want = depcases.serve(dev, [cmd]), depcases.serve(sim, [cmd])
            assert got == want, (i, cmd[0], got, want)
        assert depcases.state_of(dev, n_dc, n_part) == sim.state()
        assert dev.size()[0] == sum(len(q) for q in sim.state()[1].values())
        return sim
    finally:
        dev.close()


def three_ways(mat, arrivals, n_dc, own=0, n_part=1, order=None, now=100):
    """One call per arrival, the whole history in one call, and two calls split at every position: with
    one `now` for the history all equal DepSim served one arrival at a time."""
    check(mat, [("deliver", [t], now) for t in arrivals], n_dc, own, n_part, order)
    want = Model(n_dc, own, n_part, order)
    per = [want.deliver([t], now) for t in arrivals]
    for cut in range(len(arrivals) + 1):
        dev = mat.dep_buffer(n_dc, own, n_part, max(len(arrivals), 1), order)
        try:
            got = [dev.deliver(arrivals[:cut], now), dev.deliver(arrivals[cut:], now)]
            for p in range(n_part):
                assert got[0][p] == sum((d[p] for d in per[:cut]), []), (cut, p)
                assert got[1][p] == sum((d[p] for d in per[cut:]), []), (cut, p)
            assert depcases.state_of(dev, n_dc, n_part) == want.state(), cut
        finally:
            dev.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_literal_outputs(mat, case):
    _, n_dc, own, order, steps = case
    dev = mat.dep_buffer(n_dc, own, 1, len(steps), order)
    try:
        for t, now, delivered, clock in steps:
            assert dev.deliver([t], now) == [delivered]
            assert dev.clock(0) == clock
    finally:
        dev.close()


# own-dc is left out here: its two steps have different `now` values, and a call takes one `now`, so
# its arrivals cannot share a call (test_hand_cases_literal_outputs serves it one call per arrival)
@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "own-dc"], ids=[c[0] for c in CASES if c[0] != "own-dc"])
def test_batching_invariance_of_the_hand_cases(mat, case):
    _, n_dc, own, order, steps = case
    three_ways(mat, [s[0] for s in steps], n_dc, own, 1, order)


@pytest.mark.parametrize("seed", range(6))
def test_batching_invariance_of_random_histories(mat, seed):
    rng = random.Random(40 + seed)
    n_dc, n_part = rng.choice([2, 3, 5]), rng.choice([1, 2])
    order = rng.sample(range(n_dc), n_dc) if seed % 2 else None
    arr = depcases.random_history(rng, n_dc, n_part, 12, p_ping=0.15, now=100, order=order, non_monotone=seed == 3)
    three_ways(mat, arr, n_dc, 0, n_part, order)


@pytest.mark.parametrize("n_part", [1, 2, 65])
@pytest.mark.parametrize("n_dc", [1, 2, 3, 8, 9, 32])
def test_random_histories(mat, n_dc, n_part):
    """Calls of 0, 1, 2, 63, 64, 65 and 200 arrivals, each size at least once as a full batch, now
    advancing.  The conditions on the inputs are DepSim's own figures (depcases.conditioned_history)."""
    sizes = [0, 1, 2, 63, 64, 65, 200]
    script, m = depcases.conditioned_history(n_dc, n_part, sum(sizes) + 25, sizes)
    assert set(sizes) <= {len(c[1]) for c in script}
    assert m.delivered * 10 >= m.nonping * 9
    assert m.first_try_failed() * 3 >= m.nonping if n_dc > 1 else m.first_try_failed() == 0
    sim = check(mat, script, n_dc, 0, n_part)
    assert sim.delivered == m.delivered


def tile_history(n, bad_at=None):
    """n transactions of DC 1 behind one blocker (it waits for DC 2 at 5); entry bad_at can never pass."""
    arr = [txn(1, 10, {2: 5}, 1)]
    for i in range(n):
        arr.append(txn(1, 11 + i, {2: 5, 3: 1 << 40} if i == bad_at else {2: 5 if i % 3 else 0}, 100 + i))
    return arr, txn(2, 5, ping=True)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_tile_edges_released_by_one_ping(mat, n):
    arr, ping = tile_history(n)
    sim = check(mat, [("deliver", arr, 7), ("deliver", [ping], 7)], 4)
    assert sim.clock(0) == {1: 10 + n, 2: 5} and sim.delivered == n + 1
    check(mat, [("deliver", arr + [ping], 7)], 4)
    for bad_at in (0, 63, 64, n - 1):
        if bad_at >= n:
            continue
        arr, ping = tile_history(n, bad_at)
        sim = check(mat, [("deliver", arr, 7), ("deliver", [ping], 7)], 4)
        assert sim.clock(0)[1] == 11 + bad_at - 1 and sim.delivered == 1 + bad_at
        assert sim.queue(0, 1) == [100 + i for i in range(bad_at, n)]


def test_tile_edges_at_every_group_width(mat):
    for n_dc in (2, 3, 5, 9, 17, 32):
        per = 64 >> (n_dc - 1).bit_length()
        for n in (per - 1, per, per + 1, 2 * per + 1):
            arr = [txn(0, 10, {1: 5}, 1)] + [txn(0, 11 + i, {n_dc - 1: 5 if i % 2 else 0}, 100 + i) for i in range(n)]
            check(mat, [("deliver", arr, 7), ("deliver", [txn(n_dc - 1, 5, ping=True), txn(1, 5, ping=True)], 7)], n_dc, own=0)


def test_chain_of_300_links_in_one_call(mat):
    arr, ping, want = depcases.chain(300)
    dev = mat.dep_buffer(4, 0, 1, 601)
    try:
        assert dev.deliver(arr, 100) == [[]]
        assert dev.clock(0) == {1: 0, 2: 1} and dev.size()[0] == 600
        assert dev.deliver([ping], 100) == [want]
        assert dev.clock(0) == {1: 599, 2: 600, 3: 1} and dev.size()[0] == 0
    finally:
        dev.close()
    check(mat, [("deliver", arr + [ping], 100)], 4)


def test_order_quirk_under_both_orders(mat):
    by = {c[0]: c for c in CASES}
    for name, want in (("late-bump", [[], [], [1]]), ("late-bump-reversed", [[], [1], []]),
                       ("late-bump-mirrored", [[], [1]]), ("late-bump-mirrored-reversed", [[], []])):
        _, n_dc, own, order, steps = by[name]
        dev = mat.dep_buffer(n_dc, own, 1, 8, order)
        try:
            assert [dev.deliver([s[0]], s[1])[0] for s in steps] == want, name
            # the whole history in one call delivers the same transactions in the same order
        finally:
            dev.close()
        check(mat, [("deliver", [s[0] for s in steps], 100)], n_dc, own, 1, order)


def test_values_at_the_edges(mat):
    m, h = U64_MAX, 2 ** 63
    check(mat, [("deliver", [txn(1, m, {2: m, 0: m}, 1), txn(2, 1, {1: m - 1}, 2), txn(2, m, tag=3, ping=True)], m),
                ("deliver", [txn(1, h, {2: h}, 4), txn(2, h, {1: 1}, 5), txn(1, 1, {0: 1}, 6)], 0),
                ("deliver", [txn(1, 2, {0: 1}, 7)], 1)], 3)
    # a blocked transaction with timestamp 1: clock 0 with the presence bit set
    sim = check(mat, [("deliver", [txn(1, 1, {2: 1}, 1)], 0)], 3)
    assert sim.clock(0) == {1: 0}
    # decreasing timestamps in one queue: the clock goes down
    sim = check(mat, [("deliver", [txn(1, 9, tag=1), txn(1, 4, tag=2), txn(1, 3, {2: 1}, 3), txn(1, 1, tag=4, ping=True)], 0),
                      ("deliver", [txn(2, 1, ping=True)], 0)], 3)
    assert sim.clock(0) == {1: 1, 2: 1}
    # the own DC as an origin: the only way the stored clock gains its entry
    sim = check(mat, [("deliver", [txn(1, 5, {0: 7}, 1)], 7), ("deliver", [txn(0, 6, {1: 5}, 2), txn(0, 9, {1: 6}, 3)], 7)], 3)
    assert sim.clock(0) == {1: 5, 0: 8}
    # a dependency on the own entry that now meets only at the next call
    sim = check(mat, [("deliver", [txn(1, 5, {0: 101}, 1), txn(2, 3, {1: 5}, 2)], 100), ("deliver", [], 101),
                      ("deliver", [txn(1, 6, tag=3, ping=True)], 101)], 3)
    assert sim.delivered == 2


def test_pings_and_control(mat):
    script = [("deliver", [txn(1, 5, tag=1, ping=True), txn(1, 6, {2: 3}, 2)], 10), ("drop_ping", True),
              ("deliver", [txn(2, 3, tag=3, ping=True)], 10), ("drop_ping", False), ("deliver", [txn(2, 2, tag=4, ping=True)], 10),
              ("set_clock", 0, {0: 4, 2: 3}), ("deliver", [txn(3, 1, tag=5, ping=True)], 10),
              ("set_clock", 0, {}), ("deliver", [txn(1, 9, {3: 1}, 6)], 10)]
    check(mat, script, 4)
    rng = random.Random(9)
    arr = depcases.random_history(rng, 5, 3, 150, p_ping=0.3)
    script = depcases.split_calls(arr, [17], 10 ** 9)
    script.insert(3, ("drop_ping", True))
    script.insert(5, ("set_clock", 1, {0: 3, 2: 40, 4: 1}))
    script.insert(7, ("drop_ping", False))
    script.insert(8, ("set_clock", 2, {}))
    check(mat, script, 5, 0, 3)


def test_invalid_batches_and_capacity_leave_the_state_untouched(mat):
    dev, sim = mat.dep_buffer(3, 0, 2, 4), Model(3, 0, 2)
    try:
        first = [txn(1, 5, {2: 9}, 1), txn(2, 3, {1: 9}, 2, part=1)]
        assert dev.deliver(first, 1) == sim.deliver(first, 1)
        before = depcases.state_of(dev, 3, 2)
        for bad_tx, bits in (((2, 1, 1, {}, False, 9), abi.AM_DEP_BAD_PART), ((0, 3, 1, {}, False, 9), abi.AM_DEP_BAD_DC),
                             ((0, 1, 0, {}, False, 9), abi.AM_DEP_BAD_TIME), ((7, 9, 0, {}, False, 9), 7)):
            with pytest.raises(abi.AmError) as e:
                dev.deliver([txn(2, 9, tag=8, ping=True), bad_tx], 1)
            assert (e.value.rc, e.value.bad) == (abi.AM_ERR_INVALID, bits)
            assert depcases.state_of(dev, 3, 2) == before == sim.state() and dev.size() == (2, 4)
        with pytest.raises(abi.AmError) as e:
            dev.deliver([txn(1, 6 + i, {2: 9}, 10 + i) for i in range(3)], 1)
        assert e.value.rc == abi.AM_ERR_CAPACITY and depcases.state_of(dev, 3, 2) == before
        with pytest.raises(abi.AmError) as e:
            dev.reserve(1)
        assert e.value.rc == abi.AM_ERR_INVALID
        vc0, pres0 = dev.clocks()
        dev.reserve(64)
        assert dev.clocks() == (vc0, pres0) and dev.size() == (2, 64) and depcases.state_of(dev, 3, 2) == before
        more = [txn(1, 6 + i, {2: 9}, 10 + i) for i in range(3)] + [txn(2, 9, tag=20, ping=True), txn(1, 9, tag=21, ping=True, part=1)]
        assert dev.deliver(more, 1) == sim.deliver(more, 1)
        assert depcases.state_of(dev, 3, 2) == sim.state()
        assert dev.deliver([(0, 0, 0, {}, True, 0)], 1) == [[], []]  # a ping with timestamp 0 is legal
        sim.deliver([(0, 0, 0, {}, True, 0)], 1)
        # the two host-side verdicts, through the ABI: cap_out one short, and 2^32 arrivals
        import ctypes
        import numpy as np
        from antidote_amd.oplog import DepTxns
        held = [txn(1, 50, {2: 99}, 30), txn(2, 60, {1: 99}, 31, part=1)]
        assert dev.deliver(held, 1) == sim.deliver(held, 1)
        before, queued = depcases.state_of(dev, 3, 2), dev.size()[0]
        assert before == sim.state() and queued > 0
        b = DepTxns(3, [txn(2, 30, tag=40, ping=True), txn(1, 30, tag=41, ping=True)])
        off, tag = np.full(3, 77, np.uint64), np.full(queued + 2, 77, np.uint64)
        n, bad = ctypes.c_uint64(5), ctypes.c_uint32()
        s = b.as_struct()
        for fn in (mat.L.am_dep_deliver_host, mat.L.am_dep_deliver):  # refused before a pointer is followed
            assert fn(dev.handle, ctypes.byref(s), 1, queued + 1, off.ctypes.data, tag.ctypes.data, ctypes.byref(n),
                      ctypes.byref(bad)) == abi.AM_ERR_INVALID
            huge = abi.am_dep_txns()
            huge.n_tx = 1 << 32
            assert fn(dev.handle, ctypes.byref(huge), 1, 1 << 33, off.ctypes.data, tag.ctypes.data, ctypes.byref(n),
                      ctypes.byref(bad)) == abi.AM_ERR_INVALID
        assert set(off) == {77} and set(tag) == {77} and n.value == 5
        assert depcases.state_of(dev, 3, 2) == before and dev.size() == (queued, 64)
        dev.clear()
        assert depcases.state_of(dev, 3, 2) == ([{}, {}], {}) and dev.size() == (0, 64)
        assert dev.deliver(first, 1) == Model(3, 0, 2).deliver(first, 1)
        for args in ((0, 0, 1, 4), (33, 0, 1, 4), (3, 3, 1, 4), (3, 0, 0, 4), (3, 0, 1, 0)):
            with pytest.raises(abi.AmError):
                mat.dep_buffer(*args)
        with pytest.raises(abi.AmError):
            mat.dep_buffer(3, 0, 1, 4, [0, 1, 1])
    finally:
        dev.close()


def test_one_readback_per_call_and_the_clock_matrix_feeds_the_gst_merge(mat):
    import numpy as np
    dev, sim = mat.dep_buffer(3, 0, 4, 64), Model(3, 0, 4)
    try:
        arr = depcases.random_history(random.Random(2), 3, 4, 60, p_ping=0.2)
        for i in range(0, 60, 20):
            assert dev.deliver(arr[i:i + 20], 10 ** 9) == sim.deliver(arr[i:i + 20], 10 ** 9)
        assert dev.readbacks() == 3
        vc = np.asarray([[sim.clock(p).get(d, 0) for d in range(3)] for p in range(4)], np.uint64)
        pres = np.asarray([sum(1 << d for d in sim.clock(p)) for p in range(4)], np.uint32)
        want = np.zeros(4, np.uint64)
        assert mat.L.am_gst_local_min_host(3, 4, vc.ctypes.data, pres.ctypes.data, None, want.ctypes.data) == 0
        assert dev.gst_lanes() == [int(x) for x in want]
    finally:
        dev.close()
