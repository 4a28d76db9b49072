"""The inputs of tests/test_gpu_lagwidth.py, checked without a GPU: the hand-made logs of
tests/lagwidth_cases.py do reach what the GPU cases claim.  Computed in numpy from the host logs by
the definition of the lag view and of the per-key lag width (lagwidth_cases.definition) and by the
window rule as the kernel walks it (lagwidth_cases.window_lists): the widths, the window lists'
lengths, which ops sit at cin + w and at cin + w + 1, the bound c' - w of a sure-in op around 0, the
segments a bound is carried across, and the batches' hand-offs and error statuses."""
import numpy as np
import pytest

from antidote_amd import abi
from antidote_amd.oplog import HostBatch, Read
from oracle import amo
from tests import randlog
from tests.lagwidth_cases import LIST_WIDTHS, T0, WMAX, case, definition, window_lists

PARAMS = [(abi.AM_AWSET, 8), (abi.AM_MVREG, 8), (abi.AM_AWSET, 3)]


def cin_of(view, k, clock):
    return min(int(clock[d]) - int(view["K"][k]) + int(view["lb"][k][d]) for d in range(len(clock)))


@pytest.mark.parametrize("t,n_dc", PARAMS)
def test_batch_inputs(t, n_dc):
    keys, log, clocks, v = case("batch", t, n_dc)
    assert len(keys) == 40 and all(int(o) % 32 for o in log.key_off[1:-1])  # neighbours share bitmap words
    w = v["width"]
    first = [int(x) for x in w[:32]]
    # widths 0, 1 and 0xFFFF side by side in the first batch of 32, and no two neighbours alike
    assert any(first[i:i + 3] == [0, 1, WMAX] for i in range(30))
    assert all(first[i] != first[i + 1] for i in range(31))
    assert v["routed"][4] and w[4] == WMAX and int(v["routed"].sum()) == 1
    assert len(keys[22]) == 0 and w[22] == WMAX  # an empty key: no op in the view
    # the planted escapes: not in the view, the key's width what its other ops give
    a = [int(x) for x in log.key_off]
    for k, wk in ((9, 1), (12, 8000), (19, 63), (37, 0)):
        mid = a[k] + len(keys[k]) // 2
        assert not v["inview"][mid] and v["inview"][a[k]:a[k + 1]].sum() == len(keys[k]) - 1 and w[k] == wk
    # ... and among the window ops of a read: the escaped op's commit word inside the window's range
    hit = 0
    for k in (9, 12, 19, 37):
        mid = a[k] + len(keys[k]) // 2
        for clock in clocks:
            lst = window_lists(log, v, k, clock)[0]
            hit += len(lst) > 0 and v["ct"][lst].min() < v["ct"][mid] < v["ct"][lst].max()
    assert hit >= 2
    # the narrow windows list fewer ops than the 16-bit window on the same reads
    own = sum(len(s) for k in range(40) if len(keys[k]) for c in clocks for s in window_lists(log, v, k, c))
    wide = sum(len(s) for k in range(40) if len(keys[k]) for c in clocks for s in window_lists(log, v, k, c, WMAX))
    assert 0 < own < wide // 2, (own, wide)


@pytest.mark.parametrize("t,n_dc", PARAMS)
def test_list_inputs(t, n_dc):
    keys, log, clocks, v = case("lists", t, n_dc)
    w = v["width"]
    assert [int(w[k]) for k in sorted(LIST_WIDTHS)] == [LIST_WIDTHS[k] for k in sorted(LIST_WIDTHS)]
    at = {k: [keys[k][200].commit_time] * n_dc for k in range(6)}
    sizes = {k: len(window_lists(log, v, k, at[k])[0]) for k in range(4)}
    assert sizes == {0: 1, 1: 63, 2: 64, 3: 65}, sizes
    assert all(len(window_lists(log, v, k, [T0 - 80_000] * n_dc)[0]) == 0 for k in range(6))
    assert all(c in clocks for c in at.values()) and [T0 - 80_000] * n_dc in clocks
    # ops exactly at cin + w and at cin + w + 1 (key 4), at cin + w alone (key 5); cin is the clock's
    # entry at the committing DC, so the op at cin is op 200
    for k, nxt in ((4, True), (5, False)):
        cin = cin_of(v, k, at[k])
        a, b = int(log.key_off[k]), int(log.key_off[k + 1])
        c = v["ct"][a:b] - int(v["K"][k])
        assert c[200] == cin
        assert (c == cin + int(w[k])).sum() == 1 and ((c == cin + int(w[k]) + 1).sum() == 1) == nxt
        lst = window_lists(log, v, k, at[k])[0]
        assert (v["ct"][lst] - int(v["K"][k])).max() == cin + int(w[k])  # the last op the window holds
    # the early key: time base 0, commit words 7999, 8000, 8001 sure-in under the three last clocks
    assert int(v["K"][6]) == 0 and [op.commit_time for op in keys[6][:3]] == [7999, 8000, 8001]
    assert [cin_of(v, 6, c) - int(w[6]) for c in clocks[-3:]] == [-1, 0, 1]


def test_segment_inputs():
    t, n_dc = abi.AM_AWSET, 8
    keys, log, clocks, v = case("segments", t, n_dc)
    assert len(keys[0]) == 1100 and int(log.key_off[0]) == 0 and len(keys[5]) == 4200 and len(keys[9]) >= 1500
    a, b = int(log.key_off[5]), int(log.key_off[6])
    assert (b - 1 - (a & ~31)) // 256 >= 16  # more than 16 tiles: the long key's escape marks walk the key
    assert v["width"][0] == 320 and v["width"][5] == 640 and v["width"][9] == 0
    two = carried = 0
    for k in (0, 5, 9):
        for clock in clocks:
            segs = window_lists(log, v, k, clock)
            cin = cin_of(v, k, clock)
            two += sum(1 for s in segs if len(s)) >= 2  # the window spans a segment edge
            sure_newer = False
            lo = int(log.key_off[k])
            t0 = lo & ~31
            nseg = len(segs)
            for i, s in enumerate(segs):  # newest first
                first = t0 + (nseg - 1 - i) * 1024
                p = np.arange(max(first, lo), min(first + 1024, int(log.key_off[k + 1])))
                carried += sure_newer and len(s) > 0
                sure_newer |= bool((v["ct"][p] - int(v["K"][k]) <= cin).any())
    assert two >= 2 and carried >= 2, (two, carried)


@pytest.mark.parametrize("t", [abi.AM_AWSET, abi.AM_MVREG])
def test_sparse_inputs(t):
    n_dc = 8
    keys, log, clocks, v = case("sparse", t, n_dc)
    lens = [len(k) for k in keys]
    assert len(keys) == 69 and all(64 < lens[i] <= 8192 for i in (0, 31, 32))
    assert min(lens) <= 20 and max(lens) > 8192
    assert int(v["routed"].sum()) == 2 and v["routed"][10] and v["routed"][46]
    reads = [Read(k, t, {d: clocks[0][d] for d in range(n_dc)}) for k in range(len(keys))]
    ref = amo.materialize(log, HostBatch(n_dc, reads, randlog.caps_for(reads, n_dc, 512)))
    bad = [i for i in range(len(keys)) if ref.result(i)[0] != "ok"]
    assert {14, 66} <= set(bad) <= {6, 14, 38, 66}, bad
    # every batch: eligible reads of several widths, apart from each other
    for b in (range(0, 32), range(32, 64), range(64, 69)):
        elig = [i for i in b if 64 < lens[i] <= 8192 and not v["routed"][i] and i not in (14, 66)]
        assert len(elig) >= 3 and len({int(v["width"][i]) for i in elig}) >= 2 and any(i not in elig for i in b)


def test_definition_on_random_logs():
    """The definition itself on logs of tests/randlog (lags of 1 .. 12 us): every op in the view, the
    width the largest lag above the bases, 0xFFFF for an empty key."""
    import random
    rng = random.Random(10_300)
    from antidote_amd.oplog import HostLog
    for n_dc in (1, 3, 8):
        keys = [randlog.rand_key_ops(rng, abi.AM_AWSET, n_dc, rng.choice([0, 5, 64, 300])) for _ in range(24)]
        v = definition(HostLog(n_dc, keys, key_types=[abi.AM_AWSET] * 24))
        for k, ops in enumerate(keys):
            if not ops:
                assert v["width"][k] == WMAX
                continue
            lag = np.array([[0 if d == op.commit_dc else op.commit_time - op.snap[d] for op in ops] for d in range(n_dc)])
            assert v["width"][k] == int((lag - lag.min(axis=1)[:, None]).max()) <= 12
