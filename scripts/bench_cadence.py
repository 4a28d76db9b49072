#!/usr/bin/env python3
"""The fresh-read step of a bench.py config under GST-cadence snapshot clocks.

    python scripts/bench_cadence.py --config c3 --gst-ppm 1000000 [--steps 20 --warmup 3]

Builds the config's synthetic store at full size with am_synth_params.gst_ppm set (csrc/synth.h
am_syn_snap_g: that share of the keys carries the reference's stable-snapshot cadence in its
remote entries), without a zone index (AM_INDEX_NONE, the op-streaming headline), and times the
step exactly as bench.py does: bench.Step and bench.measure are reused unchanged -- the same
timer calls, Q, steps and warm-up.  Prints one JSON line: ms per step, the store's view counters
(am_store_view_stats) and the library path.  AM_LIB selects the library (antidote_amd/abi.py), so
an A/B of two builds is two processes (scripts/build_variant.sh builds the second library).  A
library from before am_store_view_stats reports null counters."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from antidote_amd import abi  # noqa: E402
from antidote_amd.materializer import Materializer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=["c3", "c4", "c5"])
    ap.add_argument("--gst-ppm", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)    # bench.py's defaults
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    torch.cuda.set_device(0)
    cfg = dict(bench.CONFIGS[args.config])
    mat = Materializer(0)
    uid = (ctypes.c_char * 128)()
    abi.check(mat.L.am_comm_unique_id(uid), "am_comm_unique_id")
    comm = ctypes.c_void_p()
    sys.stdout.flush()
    saved = os.dup(1)  # RCCL prints its banner on stdout; keep stdout for the one JSON line
    os.dup2(2, 1)
    try:
        rc = mat.L.am_comm_init(mat.ctx, 0, 1, uid, ctypes.byref(comm))
    finally:
        os.dup2(saved, 1)
        os.close(saved)
    abi.check(rc, "am_comm_init")

    def barrier():
        torch.cuda.synchronize()
        mat.sync()

    # bench.Step builds its parameters through bench.synth_params: the same parameters, plus gst_ppm
    plain = bench.synth_params

    def with_gst(c, rank=0, world=1):
        p = plain(c, rank, world)
        p.gst_ppm = args.gst_ppm
        return p

    bench.synth_params = with_gst
    try:
        st = bench.Step(mat, comm, cfg, 0, 1, abi.AM_INDEX_NONE)
    finally:
        bench.synth_params = plain
    stats = None
    if hasattr(st.store, "view_stats") and hasattr(mat.L, "am_store_view_stats"):
        stats = st.store.view_stats()
    m = bench.measure(st, "fresh", args.steps, args.warmup, barrier, None, full=False)
    out = {"config": args.config, "gst_ppm": args.gst_ppm, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": m["dt"] / args.steps * 1e3, "ops": st.n_ops,
           "gops_per_s": st.n_ops * args.steps / m["dt"] / 1e9, "view_stats": stats,
           "lib": os.path.abspath(abi.LIB_PATH)}
    st.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
