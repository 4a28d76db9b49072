"""The generator's GST-cadence clocks (am_synth_params.gst_ppm, csrc/synth.h am_syn_snap_g):
gst_ppm = 0 leaves the log bit for bit as recorded in tests/golden/synth_default_digest.json
(digests taken before gst_ppm existed); a GST key keeps its commit times, payloads and own-DC
entries while every remote entry trails the commit by the stable snapshot's 0.1-1.2 s and
takes few distinct values per (commit DC, DC); the oracle harness runs on such logs."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import bench
from antidote_amd import abi, synth
from antidote_amd.oplog import HostBatch, Read
from oracle import amo
from tests import fullpop, randlog

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_default_digest.json")
P = 1_000_000  # the stable snapshot's merge period, us (synth.h AM_SYN_GST_P)


def _small(cfg_name, n_keys, ops=None):
    cfg = dict(bench.CONFIGS[cfg_name])
    cfg["n_keys"] = n_keys
    if ops:
        cfg["ops"] = ops
    if cfg.get("total_ops"):
        cfg["total_ops"] = n_keys * 64
        cfg["hot_cap"] = 2048
    return cfg, bench.synth_params(cfg)


def _digest(log) -> dict:
    n = log.n_ops
    cols = {"key_off": log.key_off, "key_type": log.key_type[:log.n_keys], "op_meta": log.op_meta[:n],
            "commit_time": log.commit_time[:n], "snap_vc": log.snap_vc[:, :n], "p0": log.p0[:n], "p1": log.p1[:n]}
    if log.has_var:
        cols["var_off"] = log.var_off
        cols["var_data"] = log.var_data[:log.n_var]
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in cols.items()}


SHAPES = {"c3": (24, 256), "c4": (3000, None), "c5": (1500, None)}


def default_digests() -> dict:
    out = {}
    for name, (nk, ops) in SHAPES.items():
        _, p = _small(name, nk, ops)
        out[name] = _digest(synth.host_log(p, 0, nk))
        p.esc_ppm = 100000
        out[name + "_escape"] = _digest(synth.host_log(p, 0, nk))
    return out


def test_gst_off_is_todays_log():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = default_digests()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    _, p = _small("c4", 16)
    assert p.gst_ppm == 0 and ctypes.sizeof(p) == 72  # the struct's size is unchanged


def test_gst_ppm_above_a_million_is_rejected():
    _, p = _small("c4", 16)
    p.gst_ppm = 1_000_001
    with pytest.raises(abi.AmError):
        synth.host_log(p, 0, 16)
    q = synth.params(16, 3, abi.AM_PN, ops_per_key=4, gst_ppm=1_000_000)
    assert q.gst_ppm == 1_000_000
    synth.host_log(q, 0, 16)


@pytest.mark.parametrize("cfg_name,nk,ops,esc", [("c3", 24, 1024, 0), ("c4", 3000, None, 0), ("c5", 1500, None, 0),
                                                  ("c4", 3000, None, 100000)])
def test_every_key_gst(cfg_name, nk, ops, esc):
    _, p = _small(cfg_name, nk, ops)
    p.esc_ppm = esc
    base = synth.host_log(p, 0, nk)
    p.gst_ppm = 1_000_000
    log = synth.host_log(p, 0, nk)
    n, nd = log.n_ops, p.n_dc
    assert n == base.n_ops and (log.key_off == base.key_off).all() and (log.key_type == base.key_type).all()
    assert (log.commit_time == base.commit_time).all() and (log.op_meta == base.op_meta).all()
    assert (log.p0 == base.p0).all() and (log.p1 == base.p1).all()
    if log.has_var:
        assert (log.var_off == base.var_off).all() and (log.var_data == base.var_data).all()
    ct = log.commit_time[:n]
    cdc = (log.op_meta[:n] & 0x1F).astype(np.int64)
    ops_i = np.arange(n)
    own = log.snap_vc[cdc, ops_i]
    assert (own == base.snap_vc[cdc, ops_i]).all()  # the transaction start: unchanged
    assert (own < ct).all()
    hi = 1_200_000 + (p.max_lag + 1) * 1000
    # an escaped entry (esc_ppm) sits 2^33 us further back, on top
    esc_lag = (base.snap_vc[:, :n] != synth.host_log(_no_esc(p, 0), 0, nk).snap_vc[:, :n]) if esc else None
    for d in range(nd):
        remote = cdc != d
        lag = (ct - log.snap_vc[d, :n]).astype(np.int64)
        if esc:
            lag = lag - np.where(esc_lag[d], 1 << 33, 0)
        assert (lag[remote] >= 100_000).all() and (lag[remote] < hi).all(), (d, lag[remote].min(), lag[remote].max())
        for c in range(nd):
            if c == d:
                continue
            x = log.snap_vc[d, :n][cdc == c].astype(np.int64)
            if esc:
                x = x + np.where(esc_lag[d][cdc == c], 1 << 33, 0)
            if len(x):
                t0 = own[cdc == c].astype(np.int64)
                span = int(t0.max() - t0.min())
                assert len(np.unique(x)) <= span // P + 2, (c, d, len(np.unique(x)))
                assert len(np.unique(np.diff(np.unique(x)) % P)) <= 1  # whole periods apart


def _no_esc(p, gst):
    q = abi.am_synth_params.from_buffer_copy(p)
    q.esc_ppm, q.gst_ppm = 0, gst
    return q


def test_gst_key_share():
    _, p = _small("c4", 4000)
    base = synth.host_log(p, 0, 4000)
    p.gst_ppm = 250_000
    log = synth.host_log(p, 0, 4000)
    assert (log.commit_time == base.commit_time).all()
    changed = (log.snap_vc != base.snap_vc).any(axis=0)[:log.n_ops]
    ko = log.key_off.astype(np.int64)
    per_key = np.add.reduceat(changed.astype(np.int64), ko[:-1])
    lens = np.diff(ko)
    # a key is GST as a whole: every op with a remote DC changed (D = 3: every op), or none
    assert ((per_key == 0) | (per_key == lens)).all()
    share = (per_key > 0).mean()
    assert 0.22 <= share <= 0.28, share


@pytest.mark.parametrize("cfg_name,gst,esc", [("c3", 1_000_000, 0), ("c4", 1_000_000, 0), ("c5", 1_000_000, 0),
                                              ("c4", 250_000, 100000)])
def test_oracle_chunk_matches_hostbatch_on_gst_logs(cfg_name, gst, esc):
    _, p = _small(cfg_name, 96 if cfg_name != "c3" else 24)
    cfg = bench.CONFIGS[cfg_name]
    p.esc_ppm, p.gst_ppm = esc, gst
    clock = synth.read_clock(p, bench.Q)
    cap = max(cfg["set_cap"], 1)
    k0, nk = 5, 17
    got = fullpop.oracle_chunk(p, k0, nk, clock, cap)
    hlog = synth.host_log(p, k0, nk)
    reads = [Read(k, int(hlog.key_type[k]), {d: clock[d] for d in range(p.n_dc)}) for k in range(nk)]
    ref = amo.materialize(hlog, HostBatch(p.n_dc, reads, randlog.caps_for(reads, p.n_dc, cap)))
    for i in range(nk):
        assert int(got["status"][i]) == int(ref.status[i])
        for c in fullpop.COMMON_COLS:
            assert int(got[c][i]) == int(getattr(ref, c)[i]), (c, i)
        assert (got["last_ct"][:, i] == ref.last_ct[:, i]).all()
        t = int(got["key_type"][i])
        if t in (abi.AM_AWSET, abi.AM_MVREG, abi.AM_BCOUNTER):
            o, n = int(got["set_off"][i]), int(got["set_len"][i])
            ro = int(ref.o_set_off[i])
            assert n == int(ref.o_set_len[i])
            assert (got["set_a"][o:o + n] == ref.o_set_a[ro:ro + n]).all()
            assert (got["set_b"][o:o + n] == ref.o_set_b[ro:ro + n]).all()
        for c in fullpop.VALUE_COLS.get(t, ()):
            assert int(got[c][i]) == int(getattr(ref, c)[i]), (c, i)
