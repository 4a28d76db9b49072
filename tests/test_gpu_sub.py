"""The device subscriber buffer (am_sub, materializer.SubBuffer) against tests/subsim.py served one row at
a time: the delivered tags per partition in order, the gaps in order, the five counters, and every
stream's last, mode and queue.  No tolerances.  The sizes are the smallest at which the kernels can go
wrong: more partitions than a wave has lanes, queues around the 64-entry tile, calls around 64 rows."""
import ctypes
import random

import numpy as np
import pytest

from antidote_amd import abi
from tests import depcases, subcases
from tests.subcases import Model, end, ping, rt, t
from tests.subsim import BUFFERING, NORMAL

pytestmark = pytest.mark.gpu

U64_MAX = subcases.U64_MAX
CASES = subcases.hand_cases()


@pytest.fixture(scope="module")
def mat():
    from antidote_amd.materializer import Materializer
    m = Materializer(0)
    yield m
    m.close()


def check(mat, script, n_dc, n_part=1, logging=True, cap=None):
    """The script on the device and on SubSim: the outputs of every call, then every stream."""
    n = sum(len(c[1]) for c in script if c[0] == "process")
    dev, sim = mat.sub_buffer(n_dc, n_part, cap or max(n, 1), logging), Model(n_dc, n_part, logging)
    try:
        for i, cmd in enumerate(script):
            got, want = subcases.serve(dev, [cmd]), subcases.serve(sim, [cmd])
            assert got == want, (i, cmd[0], got, want)
        assert subcases.state_of(dev, n_dc, n_part) == sim.state()
        assert dev.size()[0] == sim.size()[0]
        return sim
    finally:
        dev.close()


def three_ways(mat, rows, n_dc, n_part=1, logging=True, before=()):
    """One call per row, the whole history in one call, and two calls split at every position: all equal
    SubSim served one row at a time."""
    before = list(before)
    check(mat, before + [("process", [r]) for r in rows], n_dc, n_part, logging)
    want = Model(n_dc, n_part, logging)
    subcases.serve(want, before)
    per = [want.process([r]) for r in rows]

    def joined(part):
        return ([sum((o[0][p] for o in part), []) for p in range(n_part)], sum((o[1] for o in part), []),
                {k: (part[-1][2][k] if k == "queued" else sum(o[2][k] for o in part)) for k in subcases.COUNTS})

    for cut in range(len(rows) + 1):
        dev = mat.sub_buffer(n_dc, n_part, len(rows) + 16, logging)
        try:
            subcases.serve(dev, before)
            got = [dev.process(rows[:cut]), dev.process(rows[cut:])]
            for g, part in ((got[0], per[:cut]), (got[1], per[cut:])):
                if part:
                    assert g == joined(part), cut
                else:
                    assert g[0] == [[] for _ in range(n_part)] and g[1] == [] and g[2]["delivered"] == 0, cut
            assert subcases.state_of(dev, n_dc, n_part) == want.state(), cut
        finally:
            dev.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_cases_literal_outputs(mat, case):
    _, n_dc, logging, steps, dropped, unexpected = case
    dev = mat.sub_buffer(n_dc, 1, len(steps), logging)
    try:
        seen = [0, 0]
        for s in steps:
            if s[0] != "row":
                subcases.serve(dev, [s])
                continue
            _, row, tags, gap, (dc, last, mode, queue) = s
            got, gaps, cnt = dev.process([row])
            assert got == [tags] and gaps == ([gap] if gap else [])
            assert dev.stream(0, dc) == (last, mode, queue)
            assert cnt["delivered"] == len(tags) and cnt["gaps"] == len(gaps) and cnt["queued"] == dev.size()[0]
            seen[0] += cnt["dropped"]
            seen[1] += cnt["unexpected"]
        assert seen == [dropped, unexpected]
    finally:
        dev.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_batching_invariance_of_the_hand_cases(mat, case):
    """The control commands of a case move to its front when that does not change its meaning (set_last
    of an untouched stream); the unreachable-dc case flips its mask mid-history and is served in the two
    halves the flip separates."""
    _, n_dc, logging, steps, _, _ = case
    ctl = [i for i, s in enumerate(steps) if s[0] != "row"]
    if case[0] == "unreachable-dc":
        first = subcases.hand_rows(steps[:ctl[1]])
        three_ways(mat, first, n_dc, 1, logging, before=[steps[0]])
        three_ways(mat, subcases.hand_rows(steps[ctl[1]:]), n_dc, 1, logging,
                   before=[steps[0], ("process", first), steps[ctl[1]]])
        return
    three_ways(mat, subcases.hand_rows(steps), n_dc, 1, logging, before=[steps[i] for i in ctl])


@pytest.mark.parametrize("seed", range(6))
def test_batching_invariance_of_random_histories(mat, seed):
    rng = random.Random(70 + seed)
    n_dc, n_part = rng.choice([1, 2, 3]), rng.choice([1, 2])
    if seed % 2:
        rows = subcases.random_rows(rng, n_dc, n_part, rng.randint(12, 16))
    else:
        rows = subcases.lossy_history(rng, n_dc, n_part, 12, p_loss=0.25, p_dup=0.2)[0][:16]
    assert 12 <= len(rows) <= 16
    three_ways(mat, rows, n_dc, n_part, logging=seed != 3)


@pytest.mark.parametrize("n_part", [1, 2, 65])
@pytest.mark.parametrize("n_dc", [1, 3, 32])
def test_random_lossy_histories(mat, n_dc, n_part):
    """Calls of 0, 1, 2, 63, 64, 65 and 200 rows, each size at least once as a full call; 5 % loss, 5 %
    duplicates, 10 % pings; responses answer the sim's own gaps 1..20 rows later.  The conditions on the
    inputs are SubSim's own figures."""
    sizes = [0, 1, 2, 63, 64, 65, 200]
    length = 600 if n_part == 1 else 3000
    rows, gen, sent = subcases.lossy_history(random.Random(n_dc * 131 + n_part), n_dc, n_part, length)
    script = subcases.split_calls(rows, sizes)
    assert [len(c[1]) for c in script[:len(sizes)]] == sizes
    sim = check(mat, script, n_dc, n_part)
    s = sim.sim
    print("rows %d gaps %d dropped %d released %d delivered %d sent %d" % (len(rows), sim.total_gaps, s.dropped, s.released,
                                                                          s.delivered, sent))
    assert sim.total_gaps * 100 >= len(rows)
    assert s.dropped * 100 >= len(rows)
    assert s.released >= sim.total_gaps
    assert s.delivered * 10 >= sent * 9


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_tile_edges_released_by_one_response(mat, n):
    rows, e = subcases.tile_history(n)
    sim = check(mat, [("process", rows), ("process", [e])], 2)
    assert sim.stream(0, 1) == (6 + n, NORMAL, []) and sim.sim.delivered == n + 2
    check(mat, [("process", rows + [e])], 2)
    for at in sorted({0, 62, 63, 64, n - 1} & set(range(n))):
        rows, e = subcases.tile_history(n, dup_at=at)
        sim = check(mat, [("process", rows), ("process", [e])], 2)
        assert sim.sim.dropped == 1 and sim.sim.delivered == n + 1 and sim.stream(0, 1)[1:] == (NORMAL, [])
        rows, e = subcases.tile_history(n, hole_at=at)
        sim = check(mat, [("process", rows), ("process", [e])], 2)
        assert sim.stream(0, 1)[1:] == (BUFFERING, [100 + i for i in range(at, n)]) and sim.total_gaps == 2
        check(mat, [("process", rows + [e, e])], 2)


def test_more_streams_than_lanes_with_one_row_each(mat):
    n_part, n_dc = 67, 3
    rows = [t(0, 1 + p, 1000 + p * n_dc + d, dc=d, part=p) for p in range(n_part) for d in range(n_dc)]
    random.Random(1).shuffle(rows)
    sim = check(mat, [("process", rows)], n_dc, n_part)
    assert sim.sim.delivered == n_part * n_dc
    # then one hole on every stream, and one lone response end for each
    holes = [t(9 + p, 10 + p, 5000 + p * n_dc + d, dc=d, part=p) for p in range(n_part) for d in range(n_dc)]
    ends = [end(d, p) for p in reversed(range(n_part)) for d in range(n_dc)]
    sim = check(mat, [("process", rows), ("process", holes), ("process", ends)], n_dc, n_part)
    assert sim.total_gaps == n_part * n_dc and sim.sim.delivered == 2 * n_part * n_dc


BAD_ROWS = (((0, 2, 1, 0, 1, 1, {}, False, 9), abi.AM_SUB_BAD_PART), ((0, 0, 3, 0, 1, 1, {}, False, 9), abi.AM_SUB_BAD_DC),
            ((0, 0, 1, 0, 1, 0, {}, False, 9), abi.AM_SUB_BAD_TIME), ((1, 0, 1, 0, 1, 0, {}, False, 9), abi.AM_SUB_BAD_TIME),
            ((3, 0, 1, 0, 1, 1, {}, False, 9), abi.AM_SUB_BAD_KIND), ((9, 7, 9, 0, 1, 0, {}, False, 9), 15))


def test_failing_calls_leave_streams_queues_and_outputs_untouched(mat):
    dev, sim = mat.sub_buffer(3, 2, 4), Model(3, 2)
    try:
        first = [t(0, 2, 1), t(5, 6, 2), t(4, 5, 3, dc=2, part=1)]
        assert dev.process(first) == sim.process(first)
        before = subcases.state_of(dev, 3, 2)
        assert before == sim.state() and dev.size() == (2, 4)
        for bad_row, bits in BAD_ROWS:
            with pytest.raises(abi.AmError) as e:
                dev.process([end(1, 0), bad_row])
            assert (e.value.rc, e.value.bad) == (abi.AM_ERR_INVALID, bits)
            assert subcases.state_of(dev, 3, 2) == before and dev.size() == (2, 4)
        with pytest.raises(abi.AmError) as e:
            dev.process([t(6 + i, 7 + i, 10 + i) for i in range(3)])
        assert e.value.rc == abi.AM_ERR_CAPACITY and subcases.state_of(dev, 3, 2) == before
        # the host-side refusals through the ABI: cap_out one short, cap_gaps one short, 2^31 rows
        from antidote_amd.oplog import SubRows
        b = SubRows(3, [ping(2, 40), ping(2, 41)])
        s = b.as_struct()
        off, cnt = np.full(3, 77, np.uint64), np.full(5, 77, np.uint64)
        cols = [np.full(8, 77, dt) for dt in (np.uint32, np.uint8, np.uint64, np.uint64, np.uint8, np.uint64)]
        out = abi.am_dep_txns()
        out.part, out.dc, out.timestamp, out.ping, out.tag = (cols[i].ctypes.data for i in (0, 1, 2, 4, 5))
        osnap = np.full(24, 77, np.uint64)
        out.snap_vc = osnap.ctypes.data
        gcols = [np.full(8, 77, dt) for dt in (np.uint32, np.uint8, np.uint64, np.uint64)]
        g = abi.am_sub_gaps()
        g.part, g.dc, g.from_, g.to = (c.ctypes.data for c in gcols)
        bad = ctypes.c_uint32()
        huge = abi.am_sub_rows()
        huge.n_rows = 1 << 31
        for fn in (mat.L.am_sub_process_host, mat.L.am_sub_process):  # refused before a pointer is followed
            for cap_out, cap_gaps, rows in ((3, 2, s), (4, 1, s), (1 << 33, 1 << 33, huge)):
                assert fn(dev.handle, ctypes.byref(rows), cap_out, off.ctypes.data, ctypes.byref(out), cap_gaps, ctypes.byref(g),
                          cnt.ctypes.data, ctypes.byref(bad)) == abi.AM_ERR_INVALID
        assert set(off) == {77} and set(cnt) == {77} and all(set(c) == {77} for c in cols + gcols + [osnap])
        assert subcases.state_of(dev, 3, 2) == before and dev.size() == (2, 4)
        # every AM_SUB_BAD_* batch (found by the first kernel) and the capacity refusal, through the ABI
        # with the same sentinel-filled outputs: nothing is written
        for bad_row, bits in BAD_ROWS:
            rb = SubRows(3, [end(1, 0), bad_row])
            sb = rb.as_struct()
            assert mat.L.am_sub_process_host(dev.handle, ctypes.byref(sb), 4, off.ctypes.data, ctypes.byref(out), 2, ctypes.byref(g),
                                             cnt.ctypes.data, ctypes.byref(bad)) == abi.AM_ERR_INVALID
            assert bad.value == bits
        rc3 = SubRows(3, [t(6 + i, 7 + i, 10 + i) for i in range(3)])
        sc = rc3.as_struct()
        assert mat.L.am_sub_process_host(dev.handle, ctypes.byref(sc), 5, off.ctypes.data, ctypes.byref(out), 3, ctypes.byref(g),
                                         cnt.ctypes.data, ctypes.byref(bad)) == abi.AM_ERR_CAPACITY
        assert set(off) == {77} and set(cnt) == {77} and all(set(c) == {77} for c in cols + gcols + [osnap])
        assert subcases.state_of(dev, 3, 2) == before and dev.size() == (2, 4)
        # reserve mid-history, then the refused rows go through
        with pytest.raises(abi.AmError) as e:
            dev.reserve(1)
        assert e.value.rc == abi.AM_ERR_INVALID
        dev.reserve(64)
        assert dev.size() == (2, 64) and subcases.state_of(dev, 3, 2) == before
        more = [t(6 + i, 7 + i, 10 + i) for i in range(3)] + [rt(2, 5, 20), end(), end(2, 1), t(0, 4, 21, dc=2, part=1)]
        assert dev.process(more) == sim.process(more)
        assert subcases.state_of(dev, 3, 2) == sim.state()
        assert dev.process([ping(9, 30), end(0, 0)]) == sim.process([ping(9, 30), end(0, 0)])  # timestamp 0 is legal on these
        assert dev.process([]) == sim.process([])
        dev.clear()
        assert subcases.state_of(dev, 3, 2) == {} and dev.size() == (0, 64)
        assert dev.process(first) == Model(3, 2).process(first)
        for args in ((0, 1, 4), (33, 1, 4), (3, 0, 4), (3, 1, 0), (3, 1, (1 << 30) + 1)):
            with pytest.raises(abi.AmError):
                mat.sub_buffer(*args)
    finally:
        dev.close()


def test_reserve_mid_history_and_clear(mat):
    rows, _, _ = subcases.lossy_history(random.Random(5), 3, 2, 300, p_loss=0.1)
    dev, sim = mat.sub_buffer(3, 2, 40), Model(3, 2)
    try:
        for i in range(0, len(rows), 30):
            if i in (90, 210):   # with 9 and with 12 entries queued
                assert dev.size()[0] > 0
                dev.reserve(dev.size()[0] + (30 if i == 90 else 100))
            if i == 180:
                dev.clear(), sim.clear()
                assert subcases.state_of(dev, 3, 2) == {} and dev.size()[0] == 0
            assert dev.process(rows[i:i + 30]) == sim.process(rows[i:i + 30]), i
            assert subcases.state_of(dev, 3, 2) == sim.state(), i
    finally:
        dev.close()


def test_a_reachable_mask_flipped_between_calls(mat):
    rows, _, _ = subcases.lossy_history(random.Random(8), 4, 3, 400, p_loss=0.1)
    script = subcases.split_calls(rows, [37])
    masks = [[0, 1, 2, 3], [0, 2], [], [1, 3], [3]]
    for i in range(len(script) - 1, 0, -1):
        script.insert(i, ("set_reachable", masks[i % len(masks)]))
    sim = check(mat, script, 4, 3)
    assert sim.total_gaps > 0 and any(s.mode == NORMAL and s.queue for s in sim.sim.streams.values())
    assert sim.sim.unexpected > 0   # responses that find their stream in normal mode


def test_one_readback_per_call(mat):
    rows, _, _ = subcases.lossy_history(random.Random(2), 3, 4, 90)
    dev, sim = mat.sub_buffer(3, 4, 128), Model(3, 4)
    try:
        for i in range(0, 90, 30):
            assert dev.process(rows[i:i + 30]) == sim.process(rows[i:i + 30])
        assert dev.stats() == {"readbacks": 3}
        dev.process([])
        dev.stream(0, 0), dev.size()
        assert dev.stats() == {"readbacks": 3}
    finally:
        dev.close()


def dep_state(dep, n_dc, n_part):
    return depcases.state_of(dep, n_dc, n_part)


def chained_history(rng, n_dc, n_part, length):
    """A lossy history whose transactions carry dependencies am_dep has to wait for: the snapshot of a
    transaction names the other DCs' timestamps, which are the per-stream message counts."""
    rows, _, _ = subcases.lossy_history(rng, n_dc, n_part, length, p_loss=0.08)
    out = []
    for r in rows:
        snap = {k: rng.randint(0, r[5] + 2) for k in range(1, n_dc) if k != r[2] and rng.random() < 0.5} if not r[7] else {}
        out.append(r[:6] + (snap,) + r[7:])
    return out


@pytest.mark.parametrize("n_dc,n_part", [(3, 2), (8, 65), (1, 1)])
def test_deliver_into_equals_subsim_then_depsim(mat, n_dc, n_part):
    rows = chained_history(random.Random(n_dc + n_part), n_dc, n_part, 700)
    sub, dep = mat.sub_buffer(n_dc, n_part, 256), mat.dep_buffer(n_dc, 0, n_part, 4096)
    msub, mdep = Model(n_dc, n_part), depcases.Model(n_dc, 0, n_part)
    try:
        sizes, i, c, held = [0, 1, 64, 65, 200, 2, 63], 0, 0, 0
        while i < len(rows):
            part = rows[i:i + sizes[c % len(sizes)]]
            now = 3 + c
            got, want = sub.deliver_into(dep, part, now), msub.deliver_into(mdep, part, now)
            assert got == want, (c, got, want)
            held = max(held, sum(len(q) for q in mdep.state()[1].values()))
            i += len(part)
            c += 1
        assert subcases.state_of(sub, n_dc, n_part) == msub.state()
        assert dep_state(dep, n_dc, n_part) == mdep.state()
        assert sub.size()[0] == msub.size()[0] and dep.size()[0] == sum(len(q) for q in mdep.state()[1].values())
        assert mdep.delivered > 0 and msub.total_gaps > 0
        assert held > 0 if n_dc > 1 else held == 0   # transactions waited in the dependency buffer: the gate was exercised
    finally:
        sub.close(), dep.close()


def test_deliver_into_refusals_leave_both_states_untouched(mat):
    sub, dep = mat.sub_buffer(3, 2, 16), mat.dep_buffer(3, 0, 2, 6)
    msub, mdep = Model(3, 2), depcases.Model(3, 0, 2)
    others = [mat.dep_buffer(3, 0, 3, 64), mat.dep_buffer(4, 0, 2, 64)]
    try:
        first = [t(0, 2, 1, snap={2: 9}), t(5, 6, 2), t(0, 1, 3, dc=2, part=1, snap={1: 9})]
        assert sub.deliver_into(dep, first, 5) == msub.deliver_into(mdep, first, 5)
        before = (subcases.state_of(sub, 3, 2), dep_state(dep, 3, 2), sub.size(), dep.size())
        assert before[2][0] == 1 and before[3][0] == 2
        for other in others:   # another n_part, another n_dc
            with pytest.raises(abi.AmError) as e:
                sub.deliver_into(other, [t(6, 7, 4)], 5)
            assert e.value.rc == abi.AM_ERR_INVALID and other.size()[0] == 0
        with pytest.raises(abi.AmError) as e:   # 2 queued in dep + 1 queued here + 4 rows > 6
            sub.deliver_into(dep, [t(6 + i, 7 + i, 10 + i) for i in range(4)], 5)
        assert e.value.rc == abi.AM_ERR_CAPACITY
        with pytest.raises(abi.AmError) as e:
            sub.deliver_into(dep, [t(6, 7, 4), (0, 0, 1, 7, 8, 0, {}, False, 5)], 5)
        assert (e.value.rc, e.value.bad) == (abi.AM_ERR_INVALID, abi.AM_SUB_BAD_TIME)
        assert (subcases.state_of(sub, 3, 2), dep_state(dep, 3, 2), sub.size(), dep.size()) == before
        assert before[0] == msub.state() and before[1] == mdep.state()
        # cap_out one below the joint bound, through the ABI
        from antidote_amd.oplog import SubRows
        one = SubRows(3, [t(6, 7, 4)])
        s = one.as_struct()
        off, tag, cnt = np.full(3, 77, np.uint64), np.full(8, 77, np.uint64), np.full(5, 77, np.uint64)
        gcols = [np.full(4, 77, dt) for dt in (np.uint32, np.uint8, np.uint64, np.uint64)]
        g = abi.am_sub_gaps()
        g.part, g.dc, g.from_, g.to = (c.ctypes.data for c in gcols)
        n, bad = ctypes.c_uint64(5), ctypes.c_uint32()
        for fn in (mat.L.am_sub_deliver_host, mat.L.am_sub_deliver):
            assert fn(sub.handle, dep.handle, ctypes.byref(s), 5, 3, off.ctypes.data, tag.ctypes.data, ctypes.byref(n), 1,
                      ctypes.byref(g), cnt.ctypes.data, ctypes.byref(bad)) == abi.AM_ERR_INVALID
        assert set(off) == {77} and set(tag) == {77} and set(cnt) == {77} and n.value == 5
        assert (subcases.state_of(sub, 3, 2), dep_state(dep, 3, 2), sub.size(), dep.size()) == before
        rest = [rt(2, 5, 20, snap={2: 1}), end(), ping(6, 21, ts=9, dc=2, part=0)]
        assert sub.deliver_into(dep, rest, 5) == msub.deliver_into(mdep, rest, 5)
        assert subcases.state_of(sub, 3, 2) == msub.state() and dep_state(dep, 3, 2) == mdep.state()
    finally:
        sub.close(), dep.close()
        for o in others:
            o.close()


def test_device_column_entry_with_torch_tensors(mat):
    """am_sub_deliver on device columns: torch owns the rows and the outputs, nothing is staged."""
    import torch
    from antidote_amd.oplog import SubRows
    n_dc, n_part = 3, 5
    rows = chained_history(random.Random(11), n_dc, n_part, 300)
    b = SubRows(n_dc, rows)
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()  # noqa: E731
    cols = {k: dev(getattr(b, k)) for k in ("kind", "part", "dc", "prev_opid", "last_opid", "timestamp", "snap_vc", "ping", "tag")}
    s = abi.am_sub_rows()
    s.n_rows = b.n_rows
    for k, v in cols.items():
        setattr(s, k, v.data_ptr())
    cap = b.n_rows
    off, tag = torch.zeros(n_part + 1, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    gp, gd = torch.zeros(cap, dtype=torch.int32, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    gf, gt = torch.zeros(cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    g = abi.am_sub_gaps()
    g.part, g.dc, g.from_, g.to = gp.data_ptr(), gd.data_ptr(), gf.data_ptr(), gt.data_ptr()
    torch.cuda.synchronize()
    sub, dep = mat.sub_buffer(n_dc, n_part, cap), mat.dep_buffer(n_dc, 0, n_part, cap)
    msub, mdep = Model(n_dc, n_part), depcases.Model(n_dc, 0, n_part)
    try:
        n, bad, cnt = ctypes.c_uint64(), ctypes.c_uint32(), np.zeros(5, np.uint64)
        rc = mat.L.am_sub_deliver(sub.handle, dep.handle, ctypes.byref(s), 7, cap, off.data_ptr(), tag.data_ptr(), ctypes.byref(n),
                                  cap, ctypes.byref(g), cnt.ctypes.data, ctypes.byref(bad))
        assert rc == 0 and bad.value == 0
        mat.sync()
        want, wgaps, wcnt = msub.deliver_into(mdep, rows, 7)
        o = off.cpu().numpy().view(np.uint64)
        tg = tag.cpu().numpy().view(np.uint64)
        assert [[int(x) for x in tg[int(o[p]):int(o[p + 1])]] for p in range(n_part)] == want
        assert n.value == sum(len(w) for w in want) > 0
        assert dict(zip(subcases.COUNTS, (int(x) for x in cnt))) == wcnt
        ng = wcnt["gaps"]
        got_gaps = list(zip(gp.cpu().numpy()[:ng].tolist(), gd.cpu().numpy()[:ng].tolist(),
                            gf.cpu().numpy().view(np.uint64)[:ng].tolist(), gt.cpu().numpy().view(np.uint64)[:ng].tolist()))
        assert got_gaps == wgaps and ng > 0
        assert subcases.state_of(sub, n_dc, n_part) == msub.state() and dep_state(dep, n_dc, n_part) == mdep.state()
    finally:
        sub.close(), dep.close()
