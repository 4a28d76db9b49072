"""bench.py --dump-outputs (bench.dump_outputs): the float64 .npy files decode to exactly the
result columns the read batch holds -- 64-bit columns from their 32-bit halves, set pairs and
bounded-counter entries padded to the widest read with zeros past each read's set_len -- for
every read or for a fixed, ascending sample of them when they exceed the byte budget, the same
from call to call.  Host-resident batches filled with random columns stand in for a step's."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bench
from antidote_amd import abi
from antidote_amd.devbatch import DeviceReads

N = 3000


def _batch(kind, seed):
    g = torch.Generator().manual_seed(seed)

    def rnd(t, hi):
        if t.dtype == torch.int64:  # every bit pattern, the sign bit included
            v = torch.randint(-(1 << 63), (1 << 63) - 1, t.shape, generator=g, dtype=torch.int64)
        else:
            v = torch.randint(0, hi, t.shape, generator=g, dtype=torch.int64).to(t.dtype)
        t.copy_(v)

    types = None
    if kind == "aw":
        type_, nd, cap = abi.AM_AWSET, 8, 64
    elif kind == "lww":
        type_, nd, cap = abi.AM_LWW, 3, 1
    else:  # MV register / bounded counter mix: two value capacities (8 and D^2 + D) in one batch
        type_, nd, cap = 0, 16, 8
        types = torch.where(torch.arange(N) % 2 == 0, abi.AM_MVREG, abi.AM_BCOUNTER).to(torch.uint8)
    r = DeviceReads(N, nd, type_, [7] * nd, device="cpu", set_cap=cap, types=types)
    for name, hi in (("status", 1), ("last_ct_pres", 1 << nd), ("last_ct_ignore", 2), ("is_new_ss", 2),
                     ("count", 1 << 20), ("flags", 256), ("vflag", 2), ("new_last_op", 0), ("last_ct", 0), ("v0", 0),
                     ("v1", 0)):
        rnd(getattr(r, name), hi)
    if r.set_len is not None:
        caps = (r.set_off[1:] - r.set_off[:-1])
        r.set_len.copy_((torch.rand(N, generator=g) * (caps + 1).to(torch.float32)).to(torch.int64).clamp(max=caps))
        rnd(r.set_a, 0)  # the words past set_len too: they must not reach the files
        rnd(r.set_b, 0)
    return SimpleNamespace(reads=r, mat=SimpleNamespace(sync=lambda: None))


def _load(d):
    cols = {f.name[:-4]: np.load(f) for f in sorted(d.iterdir())}
    assert all(a.dtype == np.float64 for a in cols.values())
    return cols


def _u64(cols, name):
    return (cols[name + "_hi"].astype(np.uint64) << np.uint64(32)) | cols[name + "_lo"].astype(np.uint64)


@pytest.mark.parametrize("kind", ["aw", "lww", "mvbc"])
@pytest.mark.parametrize("sampled", [False, True], ids=["all", "sampled"])
def test_dump_outputs_decodes_to_the_read_batch(tmp_path, monkeypatch, kind, sampled):
    budget = 1 << 18 if sampled else bench.DUMP_BUDGET
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    st = _batch(kind, 11)
    bench.dump_outputs(st, str(tmp_path / "a"))
    bench.dump_outputs(_batch(kind, 11), str(tmp_path / "b"))
    cols, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(cols) == sorted(again) and all(np.array_equal(cols[k], again[k]) for k in cols)
    assert sum(a.nbytes for a in cols.values()) <= budget
    idx = cols["read_index"].astype(np.int64)
    assert (len(idx) < N) == sampled and len(idx) > 20
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < N
    host = st.reads.host()
    for c in ("status", "last_ct_pres", "last_ct_ignore", "is_new_ss", "count", "flags", "vflag"):
        assert np.array_equal(cols[c], host[c][idx].astype(np.float64)), c
    assert np.array_equal(_u64(cols, "new_last_op"), host["new_last_op"][idx].view(np.uint64))
    assert np.array_equal(_u64(cols, "last_ct"), host["last_ct"][:, idx])
    assert np.array_equal(_u64(cols, "v0"), host["v0"][idx].view(np.uint64))
    assert np.array_equal(_u64(cols, "v1"), host["v1"][idx])
    if kind == "lww":
        assert "set_len" not in cols
        return
    r = st.reads
    sl, so = r.set_len.numpy(), r.set_off.numpy()
    sa, sb = r.set_a.numpy().view(np.uint64), r.set_b.numpy().view(np.uint64)
    assert np.array_equal(cols["set_len"], sl[idx].astype(np.float64)) and sl[idx].max() > 0
    da, db = _u64(cols, "set_a"), _u64(cols, "set_b")
    assert da.shape == (len(idx), int(np.diff(so).max()))
    for row, k in enumerate(idx):
        m, o = int(sl[k]), int(so[k])
        assert np.array_equal(da[row, :m], sa[o:o + m]) and np.array_equal(db[row, :m], sb[o:o + m])
        assert not da[row, m:].any() and not db[row, m:].any()
