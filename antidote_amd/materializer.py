"""Host mirror of the reference's materializer interface over the HIP library.

    clocksi_materializer:materialize/4  (src/clocksi_materializer.erl:82-101)
        -> Materializer.materialize(type, txid, min_snapshot_time, response)
    materializer_vnode:read/6 batched   (src/materializer_vnode.erl:96-102)
        -> Materializer.read_batch(store, reads)
    materializer_vnode:op_insert_gc/3 + prune_ops/2 (src/materializer_vnode.erl:565-647)
        -> Store.update(new_log, prune)
    materializer_vnode:load_from_log_to_tables/2 + load_ops/2 (:288-319)
        -> Materializer.load_ops(n_dc, ops_by_key, key_types) (a Vnode)
    materializer_vnode:get_from_snapshot_log/3 -> logging_vnode:get_up_to_time/5
        -> PartitionLog.read(reads, horizon); Materializer.vnode(n_dc, n_keys, logged=True)
    stable_time_functions:get_min_time/1 + meta_data_sender:update_stable/3
        -> antidote_amd.gst

Every call runs the HIP kernels of libantidote_mat.so (no CPU path exists).
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

from . import abi
from .oplog import Commits, DepTxns, Effects, Finishes, HostBatch, HostLog, Op, Prepares, Read, SubRows, Updates, WriteSet

IGNORE = None


class Store:
    """A device-resident op log (one partition's ops cache in HBM)."""

    def __init__(self, mat: "Materializer", handle: ctypes.c_void_p, n_dc: int, owned: bool = True):
        self.mat, self.handle, self.n_dc, self.owned = mat, handle, n_dc, owned

    def device_log(self) -> abi.am_op_log:
        s = abi.am_op_log()
        abi.check(abi.lib().am_store_log(self.handle, ctypes.byref(s)), "am_store_log")
        return s

    def update(self, new_log: Optional[HostLog] = None, prune: Any = None):
        """Op-cache ingestion + GC (am_store_update): returns (new Store, gc_flags[n_keys]).

        prune: None, a SnapshotCache (its snapshot_insert_gc thresholds, computed on the
        device by am_snapcache_gc_threshold), host arrays (mask[n_keys], thr_vc[n_dc][n_keys],
        thr_pres[n_keys]), or the same as device buffers (Materializer.device_array).  new_log: ops appended per key (op_insert_gc/3), ids assigned."""
        import numpy as np
        L = self.mat.L
        n_keys = int(self.device_log().n_keys)
        bufs: List[_DevBuf] = []
        tmp_store = None
        try:
            flags = _DevBuf(self.mat, max(n_keys, 1))
            bufs.append(flags)
            mask = thr = pres = None
            if isinstance(prune, SnapshotCache):
                if prune.n_keys != n_keys:  # thresholds are laid out [d * n_keys + k] per cache key
                    raise abi.AmError(f"am_store_update: snapshot cache has {prune.n_keys} keys, "
                                      f"the store {n_keys} (rc={abi.AM_ERR_INVALID})")
                mask, thr, pres = (_DevBuf(self.mat, max(n_keys, 1)), _DevBuf(self.mat, max(n_keys, 1) * 8 * self.n_dc),
                                   _DevBuf(self.mat, max(n_keys, 1) * 4))
                bufs += [mask, thr, pres]
                abi.check(L.am_snapcache_gc_threshold(self.mat.ctx, prune.handle, mask.ptr, thr.ptr, pres.ptr),
                          "am_snapcache_gc_threshold")
            elif prune is not None and isinstance(prune[0], _DevBuf):
                mask, thr, pres = prune        # device-resident (caller-owned)
            elif prune is not None:
                m, t, pr = prune
                mask = _DevBuf.of(self.mat, np.ascontiguousarray(m, np.uint8))
                thr = _DevBuf.of(self.mat, np.ascontiguousarray(t, np.uint64))
                pres = _DevBuf.of(self.mat, np.ascontiguousarray(pr, np.uint32))
                bufs += [mask, thr, pres]
            new_dev = None
            if new_log is not None:
                tmp_store = self.mat.store(new_log)
                new_dev = tmp_store.device_log()
            h = ctypes.c_void_p()
            abi.check(L.am_store_update(self.mat.ctx, self.handle, ctypes.byref(new_dev) if new_dev is not None else None,
                                        mask.ptr if mask else None, thr.ptr if thr else None,
                                        pres.ptr if pres else None, flags.ptr, ctypes.byref(h)), "am_store_update")
            out = np.zeros(max(n_keys, 1), np.uint8)
            flags.download(out)
            return Store(self.mat, h, self.n_dc), out[:n_keys]
        finally:
            for b in bufs:
                b.free()
            if tmp_store is not None:
                tmp_store.close()

    def index(self, level: int = abi.AM_INDEX_SUMMARIES):
        """Drop and rebuild the store's zone index at `level` (am_store_index: AM_INDEX_NONE,
        _ZONES bounds only, _EXACT + exact marks, _SUMMARIES + group summaries, the default)."""
        abi.check(self.mat.L.am_store_index(self.mat.ctx, self.handle, int(level)), "am_store_index")

    def view_stats(self) -> Dict[str, int]:
        """Counters of the store's views as they are now (am_store_view_stats): ops, ops escaped
        from the packed view, lag-only escaped ops, packed-routed keys and their ops."""
        out = (ctypes.c_uint64 * abi.AM_VIEW_STAT_N)()
        abi.check(self.mat.L.am_store_view_stats(self.mat.ctx, self.handle, out), "am_store_view_stats")
        return dict(zip(abi.VIEW_STATS, (int(x) for x in out)))

    def lag_width(self):
        """The store's per-key lag widths (am_store_lag_width) as a numpy u16 array [n_keys];
        raises on a store without a lag view."""
        import numpy as np
        out = np.zeros(max(1, int(self.device_log().n_keys)), np.uint16)
        abi.check(self.mat.L.am_store_lag_width(self.mat.ctx, self.handle, out.ctypes.data), "am_store_lag_width")
        return out[: int(self.device_log().n_keys)]

    def reserve(self) -> "Store":
        """A copy with room for appends per key (am_store_reserve), the layout am_store_apply
        updates in place."""
        h = ctypes.c_void_p()
        abi.check(self.mat.L.am_store_reserve(self.mat.ctx, self.handle, ctypes.byref(h)), "am_store_reserve")
        return Store(self.mat, h, self.n_dc)

    def apply(self, keys: Sequence[int], new_log: Optional[HostLog] = None, prune: Any = None):
        """In-place ingestion + GC of the touched keys only (am_store_apply).  new_log: CSR over
        the touched keys (entry i appends to keys[i]); prune: (mask[n_keys], thr_vc[n_dc][n_keys],
        thr_pres[n_keys]) host arrays or device buffers.  Returns (applied, gc_flags[len(keys)]);
        applied False: some key outgrew its room and nothing was written."""
        import numpy as np
        L = self.mat.L
        m = len(keys)
        ka = np.ascontiguousarray(keys, np.uint64)
        n_keys = int(self.device_log().n_keys)
        if m and (int(ka.max()) >= n_keys or len(np.unique(ka)) != m):
            raise abi.AmError(f"am_store_apply: touched keys must be distinct and < {n_keys} (rc={abi.AM_ERR_INVALID})")
        if new_log is not None and new_log.n_keys != m:
            raise abi.AmError(f"am_store_apply: the new-op log has {new_log.n_keys} keys for {m} touched keys "
                              f"(rc={abi.AM_ERR_INVALID})")
        bufs: List[_DevBuf] = []
        tmp_store = None
        try:
            kb = _DevBuf.of(self.mat, ka)
            flags = _DevBuf(self.mat, max(m, 1))
            bufs += [kb, flags]
            mask = thr = pres = None
            if prune is not None and isinstance(prune[0], _DevBuf):
                mask, thr, pres = prune
            elif prune is not None:
                mask, thr, pres = (_DevBuf.of(self.mat, np.ascontiguousarray(prune[0], np.uint8)),
                                   _DevBuf.of(self.mat, np.ascontiguousarray(prune[1], np.uint64)),
                                   _DevBuf.of(self.mat, np.ascontiguousarray(prune[2], np.uint32)))
                bufs += [mask, thr, pres]
            new_dev = None
            if new_log is not None:
                tmp_store = self.mat.store(new_log)
                new_dev = tmp_store.device_log()
            ap = ctypes.c_int(0)
            abi.check(L.am_store_apply(self.mat.ctx, self.handle, m, kb.ptr,
                                       ctypes.byref(new_dev) if new_dev is not None else None,
                                       mask.ptr if mask else None, thr.ptr if thr else None, pres.ptr if pres else None,
                                       flags.ptr, ctypes.byref(ap)), "am_store_apply")
            out = np.zeros(max(m, 1), np.uint8)
            flags.download(out)
            return bool(ap.value), out[:m]
        finally:
            for b in bufs:
                b.free()
            if tmp_store is not None:
                tmp_store.close()

    def relabel(self, old, new):
        """Apply a codec relabel map (Codec.take_relabel) to the store's label words in place."""
        import numpy as np
        o, n = np.ascontiguousarray(old, np.uint64), np.ascontiguousarray(new, np.uint64)
        abi.check(self.mat.L.am_store_relabel(self.mat.ctx, self.handle, o.ctypes.data, n.ctypes.data, len(o)),
                  "am_store_relabel")

    def download(self) -> Dict[str, Any]:
        """The device log's columns as numpy arrays (for parity checks); op_id is always
        filled (dense ids from key_id_base when the store keeps no explicit column)."""
        import numpy as np
        s = self.device_log()
        nk, n, nd = int(s.n_keys), int(s.n_ops), int(s.n_dc)
        stride = int(s.snap_stride) or n

        def get(ptr, count, dt):
            a = np.zeros(max(count, 1), dt)
            if ptr and count:
                abi.check(self.mat.L.am_memcpy_d2h(self.mat.ctx, a.ctypes.data, ptr, count * a.itemsize), "d2h")
            return a[:count]
        key_off = get(s.key_off, nk + 1, np.uint64)
        out = {"key_off": key_off, "key_type": get(s.key_type, nk, np.uint8),
               "key_flags": get(s.key_flags, nk, np.uint8) if s.key_flags else np.zeros(nk, np.uint8),
               "op_meta": get(s.op_meta, n, np.uint8), "commit_time": get(s.commit_time, n, np.uint64),
               "snap_vc": get(s.snap_vc, nd * stride, np.uint64).reshape(nd, stride)[:, :n] if n else np.zeros((nd, 0), np.uint64),
               "snap_pres": get(s.snap_pres, n, np.uint32) if s.snap_pres else None,
               "op_txid": get(s.op_txid, n, np.uint64) if s.op_txid else None,
               "p0": get(s.p0, n, np.uint64), "p1": get(s.p1, n, np.uint64),
               "var_off": get(s.var_off, n + 1, np.uint64) if s.var_off else None,
               "var_data": get(s.var_data, int(s.n_var), np.uint64) if s.var_off else None,
               "explicit_op_id": bool(s.op_id)}
        key_end = get(s.key_end, nk, np.uint64) if s.key_end else key_off[1:]
        if s.op_id:
            out["op_id"] = get(s.op_id, n, np.uint64)
        else:
            idb = get(s.key_id_base, nk, np.uint64) if s.key_id_base else np.ones(nk, np.uint64)
            ids = np.zeros(n, np.uint64)
            for k in range(nk):
                o0, o1 = int(key_off[k]), int(key_end[k])
                ids[o0:o1] = np.arange(o1 - o0, dtype=np.uint64) + idb[k]
            out["op_id"] = ids
        if s.key_end:  # a vnode store's room for appends: the used ops only, as a dense CSR
            sel = np.concatenate([np.arange(int(key_off[k]), int(key_end[k]), dtype=np.int64) for k in range(nk)]
                                 + [np.zeros(0, np.int64)])
            dense_off = np.zeros(nk + 1, np.uint64)
            dense_off[1:] = np.cumsum((key_end - key_off[:-1]).astype(np.uint64))
            for c in ("op_meta", "commit_time", "snap_pres", "op_txid", "p0", "p1", "op_id"):
                if out[c] is not None:
                    out[c] = out[c][sel]
            out["snap_vc"] = out["snap_vc"][:, sel]
            if out["var_off"] is not None:
                vo, vd = out["var_off"], out["var_data"]
                words = [vd[int(vo[p]):int(vo[p + 1])] for p in sel]
                lens = np.array([len(w) for w in words], np.uint64)
                out["var_off"] = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
                out["var_data"] = np.concatenate(words + [np.zeros(0, np.uint64)]).astype(np.uint64)
            out["key_off"] = dense_off
        return out

    def close(self):
        if self.handle:
            if self.owned and self.mat.ctx:  # a closed context already released its memory
                abi.lib().am_store_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DevBuf:
    """A device allocation through the library's own allocator (am_dev_alloc)."""

    def __init__(self, mat: "Materializer", nbytes: int):
        self.mat, self.nbytes, self.p = mat, nbytes, ctypes.c_void_p()
        abi.check(mat.L.am_dev_alloc(mat.ctx, nbytes, ctypes.byref(self.p)), "am_dev_alloc")

    @property
    def ptr(self):
        return self.p.value

    @classmethod
    def of(cls, mat, arr):
        b = cls(mat, max(arr.nbytes, 1))
        if arr.nbytes:
            abi.check(mat.L.am_memcpy_h2d(mat.ctx, b.ptr, arr.ctypes.data, arr.nbytes), "am_memcpy_h2d")
        return b

    def download(self, arr):
        abi.check(self.mat.L.am_memcpy_d2h(self.mat.ctx, arr.ctypes.data, self.ptr, min(arr.nbytes, self.nbytes)),
                  "am_memcpy_d2h")

    def free(self):
        if self.p:
            self.mat.L.am_dev_free(self.mat.ctx, self.p)
            self.p = ctypes.c_void_p()


def _cache_snapshots(mat, sc, n_dc: int, key: int, type_: int):
    """A snapshot cache's dict for a key: [(clock, last_op_id, value)] newest first (values as
    HostBatch.value renders them), or None before the key's first read."""
    import numpy as np
    nd, cap = n_dc, abi.AM_SNAPSHOT_THRESHOLD
    n = ctypes.c_uint32()
    vc = np.zeros(cap * nd, np.uint64)
    pres = np.zeros(cap, np.uint32)
    lo = np.zeros(cap, np.int64)
    v0 = np.zeros(cap, np.int64)
    v1 = np.zeros(cap, np.uint64)
    vf = np.zeros(cap, np.uint8)
    L = mat.L
    abi.check(L.am_snapcache_get(mat.ctx, sc, key, ctypes.byref(n), vc.ctypes.data, pres.ctypes.data,
                                 lo.ctypes.data, v0.ctypes.data, v1.ctypes.data, vf.ctypes.data), "am_snapcache_get")
    if n.value == abi.AM_SNAPCACHE_ABSENT:
        return None
    out = []
    for e in range(n.value):
        clock = {d: int(vc[e * nd + d]) for d in range(nd) if (int(pres[e]) >> d) & 1}
        if type_ == abi.AM_PN:
            val: Any = int(v0[e])
        elif type_ == abi.AM_LWW:
            val = (int(v0[e:e + 1].view(np.uint64)[0]), int(v1[e]), bool(vf[e]))
        else:
            nw = ctypes.c_uint32()
            abi.check(L.am_snapcache_get_value(mat.ctx, sc, key, e, 0, ctypes.byref(nw), None, None, None),
                      "am_snapcache_get_value")
            m = max(int(nw.value), 1)
            a, b, p = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint8)
            abi.check(L.am_snapcache_get_value(mat.ctx, sc, key, e, m, ctypes.byref(nw), a.ctypes.data,
                                               b.ctypes.data, p.ctypes.data), "am_snapcache_get_value")
            w = int(nw.value)
            if type_ == abi.AM_BCOUNTER:
                from .oplog import bc_dicts
                val = bc_dicts([(int(a[j]), int(b[j])) for j in range(w)], nd)
            else:
                val = [(int(a[j]), int(b[j])) for j in range(w)]
        out.append((clock, int(lo[e]), val))
    return out


class SnapshotCache:
    """A partition's snapshot cache on the device: reads run materializer_vnode:internal_read/7
    (src/materializer_vnode.erl:371-376) -- base from the cache, materialize/4, write-back."""

    def __init__(self, mat: "Materializer", store: "Store", n_keys: int):
        self.mat, self.store, self.n_keys = mat, store, int(n_keys)
        self.handle = ctypes.c_void_p()
        abi.check(mat.L.am_snapcache_create(mat.ctx, store.n_dc, n_keys, ctypes.byref(self.handle)),
                  "am_snapcache_create")

    def read(self, reads: Sequence[Read], set_capacity=None) -> HostBatch:
        """internal_read/7 (ShouldGC = false) for reads of distinct keys; read.base_* are ignored.
        Per read: ('ok', Value, ...) or ('error', AM_ERR_COLD_PATH) when the log would be read."""
        hb = HostBatch(self.store.n_dc, reads, set_capacity)
        b, r = hb.structs()
        abi.check(self.mat.L.am_snapcache_read_host(self.mat.ctx, self.handle, self.store.handle, ctypes.byref(b),
                                                    ctypes.byref(r)), "am_snapcache_read_host")
        return hb

    def snapshots(self, key: int, type_: int):
        """[(clock, last_op_id, value)] newest first, or None before the key's first read."""
        return _cache_snapshots(self.mat, self.handle, self.store.n_dc, key, type_)

    def relabel(self, old, new):
        """Apply a codec relabel map to the cache (key types from the store it serves)."""
        import numpy as np
        o, n = np.ascontiguousarray(old, np.uint64), np.ascontiguousarray(new, np.uint64)
        abi.check(self.mat.L.am_snapcache_relabel(self.mat.ctx, self.handle, self.store.device_log().key_type,
                                                  o.ctypes.data, n.ctypes.data, len(o)), "am_snapcache_relabel")

    def entries(self, key: int):
        """[(clock, last_op_id, v0, v1, vflag)] newest first, or None before the key's first read."""
        import numpy as np
        nd, cap = self.store.n_dc, abi.AM_SNAPSHOT_THRESHOLD
        n = ctypes.c_uint32()
        vc = np.zeros(cap * nd, np.uint64)
        pres = np.zeros(cap, np.uint32)
        lo = np.zeros(cap, np.int64)
        v0 = np.zeros(cap, np.int64)
        v1 = np.zeros(cap, np.uint64)
        vf = np.zeros(cap, np.uint8)
        abi.check(self.mat.L.am_snapcache_get(self.mat.ctx, self.handle, key, ctypes.byref(n), vc.ctypes.data,
                                              pres.ctypes.data, lo.ctypes.data, v0.ctypes.data, v1.ctypes.data,
                                              vf.ctypes.data), "am_snapcache_get")
        if n.value == abi.AM_SNAPCACHE_ABSENT:
            return None
        out = []
        for e in range(n.value):
            clock = {d: int(vc[e * nd + d]) for d in range(nd) if (int(pres[e]) >> d) & 1}
            out.append((clock, int(lo[e]), int(v0[e]), int(v1[e]), int(vf[e])))
        return out

    def close(self):
        if self.handle:
            if self.mat.ctx:
                self.mat.L.am_snapcache_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class PartitionLog:
    """The partition's log in HBM (am_plog): the committed transactions in commit order, and the
    cold read logging_vnode:get_up_to_time/5 + materialize/4 serve from it
    (src/logging_vnode.erl:522-545, 676-779; src/materializer_vnode.erl:415-419)."""

    def __init__(self, mat: "Materializer", n_dc: int, cap_tx: int = 1024, cap_eff: int = 4096, cap_var: int = 4096,
                 borrowed: Optional[ctypes.c_void_p] = None):
        self.mat, self.n_dc, self.owned = mat, n_dc, borrowed is None
        self.handle = ctypes.c_void_p() if borrowed is None else borrowed  # borrowed: a logged Vnode's log
        if borrowed is None:
            abi.check(mat.L.am_plog_create(mat.ctx, n_dc, cap_tx, cap_eff, cap_var, ctypes.byref(self.handle)),
                      "am_plog_create")

    def append(self, transactions):
        """A batch of committed transactions behind the log (am_plog_append_host): a Commits, or
        what Commits takes.  An invalid batch raises and leaves the log as it was."""
        cm = transactions if isinstance(transactions, Commits) else Commits(self.n_dc, transactions)
        s = cm.as_struct()
        abi.check(self.mat.L.am_plog_append_host(self.handle, ctypes.byref(s)), "am_plog_append_host")

    def size(self) -> Tuple[int, int, int]:
        """(transactions, effects, variable words) in the log."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        abi.check(self.mat.L.am_plog_size(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "am_plog_size")
        return int(a.value), int(b.value), int(c.value)

    def key_ops(self, key: int, horizon: Optional[int] = None) -> List[int]:
        """The global effect indices of the key's chain among the first `horizon` transactions
        (None: the whole log), oldest first, whatever their clocks (am_plog_key_ops)."""
        import numpy as np
        n_tx, n_eff, _ = self.size()
        out = np.zeros(max(n_eff, 1), np.uint64)
        n = ctypes.c_uint64()
        abi.check(self.mat.L.am_plog_key_ops(self.handle, key, n_tx if horizon is None else horizon, n_eff,
                                             out.ctypes.data, ctypes.byref(n)), "am_plog_key_ops")
        return [int(x) for x in out[:int(n.value)]]

    def read(self, reads: Sequence[Read], horizon: Optional[Sequence[int]] = None, set_capacity=None) -> HostBatch:
        """Every read served from the log (am_plog_read_host; read.base_* are ignored): the key's
        logged effects among the first horizon[i] transactions (None: the whole log) whose
        transaction's snapshot_time is vectorclock:le the read clock, ids 0, 1, ... oldest first,
        materialized from new() under the clock {}."""
        import numpy as np
        hb = HostBatch(self.n_dc, reads, set_capacity)
        b, r = hb.structs()
        hz = np.ascontiguousarray(horizon, np.uint64) if horizon is not None else None
        abi.check(self.mat.L.am_plog_read_host(self.mat.ctx, self.handle, ctypes.byref(b),
                                               hz.ctypes.data if hz is not None else None, ctypes.byref(r)),
                  "am_plog_read_host")
        return hb

    def close(self):
        if self.handle:
            if self.owned and self.mat.ctx:
                self.mat.L.am_plog_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class Vnode:
    """One partition's materializer_vnode state on the device (am_vnode): the ops cache and the
    snapshot cache, driven by op_insert_gc/3 and internal_read/7 with the reference's GC
    (src/materializer_vnode.erl:371-376, 515-563, 622-647).  logged: the vnode keeps the
    partition's log (am_vnode_create_logged): commits are appended to it, and a read no cached
    snapshot serves is read from it (get_from_snapshot_log) instead of ending as AM_ERR_COLD_PATH."""

    def __init__(self, mat: "Materializer", n_dc: int, n_keys: int, logged: bool = False):
        self.mat, self.n_dc, self.n_keys, self.logged = mat, n_dc, n_keys, logged
        self.handle = ctypes.c_void_p()
        if logged:
            abi.check(mat.L.am_vnode_create_logged(mat.ctx, n_dc, n_keys, ctypes.byref(self.handle)),
                      "am_vnode_create_logged")
        else:
            abi.check(mat.L.am_vnode_create(mat.ctx, n_dc, n_keys, ctypes.byref(self.handle)), "am_vnode_create")

    @property
    def log(self) -> Optional[PartitionLog]:
        """The vnode's partition log (borrowed: valid while the vnode is), or None for a plain vnode."""
        h = ctypes.c_void_p()
        abi.check(self.mat.L.am_vnode_log(self.handle, ctypes.byref(h)), "am_vnode_log")
        return PartitionLog(self.mat, self.n_dc, borrowed=h) if h else None

    def insert(self, ops_by_key: Sequence[Sequence[Op]], key_types: Sequence[int]):
        """op_insert_gc/3 for every op (each key's ops oldest -> newest; op ids are assigned).  A
        logged vnode raises (AM_ERR_UNSUPPORTED): a per-key log has no commit order."""
        log = HostLog(self.n_dc, ops_by_key, key_types=key_types)
        s = log.as_struct()
        abi.check(self.mat.L.am_vnode_insert_host(self.handle, ctypes.byref(s)), "am_vnode_insert_host")
        self.n_keys = max(self.n_keys, len(ops_by_key))  # keys past the key space grow it

    def commit(self, transactions):
        """clocksi_vnode:commit/5 -> update_materializer/3 for a batch of committed transactions
        (am_vnode_commit_host): op_insert_gc/3 for every effect, the op log built on the device.
        transactions: a Commits, or what Commits takes -- [(dc, commit_time, snap, txid, [(key,
        type, effect), ...])].  Host work is O(batch), whatever the vnode's key count."""
        cm = transactions if isinstance(transactions, Commits) else Commits(self.n_dc, transactions)
        s = cm.as_struct()
        abi.check(self.mat.L.am_vnode_commit_host(self.handle, ctypes.byref(s)), "am_vnode_commit_host")
        if cm.n_eff:
            self.n_keys = max(self.n_keys, int(cm.key[:cm.n_eff].max()) + 1)  # keys past the key space grow it

    def read(self, reads: Sequence[Read], should_gc: Optional[Sequence[bool]] = None, set_capacity=None) -> HostBatch:
        """internal_read/7 per read (read.base_* ignored).  A read with no cached snapshot at or
        below its clock takes the log path: a logged vnode serves it from its log; on a plain vnode
        (logged=False) the status ('error', AM_ERR_COLD_PATH) remains and the caller reads the log."""
        import numpy as np
        hb = HostBatch(self.n_dc, reads, set_capacity)
        b, r = hb.structs()
        sg = np.ascontiguousarray([1 if x else 0 for x in should_gc], np.uint8) if should_gc is not None else None
        abi.check(self.mat.L.am_vnode_read_host(self.handle, ctypes.byref(b), sg.ctypes.data if sg is not None else None,
                                                ctypes.byref(r)), "am_vnode_read_host")
        return hb

    def key_info(self, key: int):
        """(Length, ListLen, OpCounter) of the key's ops-cache tuple."""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        abi.check(self.mat.L.am_vnode_key_info(self.handle, key, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                  "am_vnode_key_info")
        return int(a.value), int(b.value), int(c.value)

    def stats(self):
        """(whole-store rebuilds, in-place applies) of the ops cache's ingestion and GC."""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        abi.check(self.mat.L.am_vnode_stats(self.handle, ctypes.byref(a), ctypes.byref(b)), "am_vnode_stats")
        return int(a.value), int(b.value)

    def relabel(self, old, new):
        """Apply a codec relabel map (Codec.take_relabel) to the ops cache and snapshot cache."""
        import numpy as np
        o, n = np.ascontiguousarray(old, np.uint64), np.ascontiguousarray(new, np.uint64)
        abi.check(self.mat.L.am_vnode_relabel(self.handle, o.ctypes.data, n.ctypes.data, len(o)), "am_vnode_relabel")

    def _parts(self):
        st, sc = ctypes.c_void_p(), ctypes.c_void_p()
        abi.check(self.mat.L.am_vnode_parts(self.handle, ctypes.byref(st), ctypes.byref(sc)), "am_vnode_parts")
        return st, sc

    def store(self) -> Store:
        """The ops cache as a borrowed Store: valid until the next insert or read (a read's GC can
        rebuild the store when a key outgrows its room for appends)."""
        st, _ = self._parts()
        return Store(self.mat, st, self.n_dc, owned=False)

    def op_ids(self, key: int) -> List[int]:
        """The op ids in the key's ops cache, oldest first."""
        import numpy as np
        st, _ = self._parts()
        d = abi.am_op_log()  # the vnode's store is borrowed: no Store wrapper (it would destroy it)
        abi.check(self.mat.L.am_store_log(st, ctypes.byref(d)), "am_store_log")
        L = self.mat.L
        ko = np.zeros(2, np.uint64)
        abi.check(L.am_memcpy_d2h(self.mat.ctx, ko.ctypes.data, d.key_off + key * 8, 16), "am_memcpy_d2h")
        if d.key_end:
            abi.check(L.am_memcpy_d2h(self.mat.ctx, ko[1:].ctypes.data, d.key_end + key * 8, 8), "am_memcpy_d2h")
        n = int(ko[1] - ko[0])
        if n == 0:
            return []
        if d.op_id:
            ids = np.zeros(n, np.uint64)
            abi.check(L.am_memcpy_d2h(self.mat.ctx, ids.ctypes.data, d.op_id + int(ko[0]) * 8, n * 8), "am_memcpy_d2h")
            return [int(x) for x in ids]
        base = np.ones(1, np.uint64)
        if d.key_id_base:
            abi.check(L.am_memcpy_d2h(self.mat.ctx, base.ctypes.data, d.key_id_base + key * 8, 8), "am_memcpy_d2h")
        return [int(base[0]) + i for i in range(n)]

    def snapshots(self, key: int, type_: int):
        """[(clock, last_op_id, value)] newest first, or None before the key's first read."""
        _, sc = self._parts()
        return _cache_snapshots(self.mat, sc, self.n_dc, key, type_)

    def close(self):
        if self.handle:
            if self.mat.ctx:
                self.mat.L.am_vnode_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class Certifier:
    """The partition's write-write certification in HBM (am_cert): prepared_tx and committed_tx of
    clocksi_vnode (src/clocksi_vnode.erl:450-632) and the read servers' two checks
    (src/clocksi_readitem_server.erl:236-264), for batches.  Arguments and returns are CertSim's
    (tests/certsim.py).  A call that fails raises abi.AmError with the code in .rc (AM_ERR_INVALID: a
    malformed batch; AM_ERR_CAPACITY: more live entries than cap_entries or more committed keys than
    cap_keys) and leaves the tables as they were; only reserve() changes the capacities."""

    def __init__(self, mat: "Materializer", cap_keys: int, cap_entries: int, record_commits: bool = True):
        self.mat, self.handle = mat, ctypes.c_void_p()
        self._check(mat.L.am_cert_create(mat.ctx, cap_keys, cap_entries, 1 if record_commits else 0,
                                         ctypes.byref(self.handle)), "am_cert_create")

    @staticmethod
    def _check(rc: int, what: str):
        if rc != 0:
            msg = abi.lib().am_last_error()
            e = abi.AmError(f"{what} failed rc={rc}: {msg.decode() if msg else ''}")
            e.rc = rc
            raise e

    def prepare(self, txs) -> List[int]:
        """[(txid, start_time, prepare_time, certify, [key, ...])] (or a Prepares) -> statuses: AM_OK,
        AM_ERR_WRITE_CONFLICT or AM_ERR_NO_UPDATES, as if served one at a time in batch order."""
        import numpy as np
        b = txs if isinstance(txs, Prepares) else Prepares(txs)
        s, st = b.as_struct(), np.zeros(max(b.n_tx, 1), np.int32)
        self._check(self.mat.L.am_cert_prepare_host(self.handle, ctypes.byref(s), st.ctypes.data), "am_cert_prepare_host")
        return [int(x) for x in st[:b.n_tx]]

    def finish(self, txs) -> List[int]:
        """[(txid, commit_time, committed, [key, ...])] (or a Finishes) -> statuses: AM_OK or
        AM_ERR_NO_UPDATES.  commit/5 with committed, abort/2 without."""
        import numpy as np
        b = txs if isinstance(txs, Finishes) else Finishes(txs)
        s, st = b.as_struct(), np.zeros(max(b.n_tx, 1), np.int32)
        self._check(self.mat.L.am_cert_finish_host(self.handle, ctypes.byref(s), st.ctypes.data), "am_cert_finish_host")
        return [int(x) for x in st[:b.n_tx]]

    def read_ready(self, reads, now: int) -> List[int]:
        """[(key, start_time)] -> the wait in ms before each read may be served (0: ready)."""
        import numpy as np
        n = len(reads)
        k = np.asarray([int(r[0]) for r in reads] or [0], np.uint64)
        t = np.asarray([int(r[1]) for r in reads] or [0], np.uint64)
        w = np.zeros(max(n, 1), np.uint64)
        self._check(self.mat.L.am_cert_read_ready_host(self.handle, n, k.ctypes.data, t.ctypes.data, int(now),
                                                       w.ctypes.data), "am_cert_read_ready_host")
        return [int(x) for x in w[:n]]

    def min_prepared(self) -> Optional[int]:
        t, p = ctypes.c_uint64(), ctypes.c_int()
        self._check(self.mat.L.am_cert_min_prepared(self.handle, ctypes.byref(t), ctypes.byref(p)), "am_cert_min_prepared")
        return int(t.value) if p.value else None

    def key_info(self, key: int):
        """(commit time or 0, [(txid, prepare time)] sorted by (time, txid))."""
        import numpy as np
        cap = 64
        while True:
            ct, n = ctypes.c_uint64(), ctypes.c_uint64()
            tx, tm = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
            rc = self.mat.L.am_cert_key_info(self.handle, int(key), ctypes.byref(ct), cap, tx.ctypes.data, tm.ctypes.data,
                                             ctypes.byref(n))
            if rc == abi.AM_ERR_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            self._check(rc, "am_cert_key_info")
            return int(ct.value), [(int(tx[i]), int(tm[i])) for i in range(int(n.value))]

    def reserve(self, cap_keys: int, cap_entries: int):
        self._check(self.mat.L.am_cert_reserve(self.handle, cap_keys, cap_entries), "am_cert_reserve")

    def size(self) -> Tuple[int, int, int, int]:
        """(committed keys, live prepared entries, cap_keys, cap_entries)"""
        v = [ctypes.c_uint64() for _ in range(4)]
        self._check(self.mat.L.am_cert_size(self.handle, *[ctypes.byref(x) for x in v]), "am_cert_size")
        return tuple(int(x.value) for x in v)

    def stats(self) -> Dict[str, int]:
        """Counters since create: resolve rounds, status-block readbacks, compactions."""
        v = [ctypes.c_uint64() for _ in range(3)]
        self._check(self.mat.L.am_cert_stats(self.handle, *[ctypes.byref(x) for x in v]), "am_cert_stats")
        return dict(zip(("rounds", "readbacks", "compactions"), (int(x.value) for x in v)))

    def close(self):
        if self.handle:
            if self.mat.ctx:
                self.mat.L.am_cert_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class DepBuffer:
    """The dependency buffers of every partition a GPU owns, in HBM (am_dep): inter_dc_dep_vnode's
    queues, try_store/2 and partition clock (src/inter_dc_dep_vnode.erl:94-154, 187-238), for batches
    of arrivals.  tests/depsim.py restates the reference; deliver() returns, per partition, what
    serving the batch one arrival at a time through it returns.  A call that fails raises abi.AmError
    with the code in .rc and the validity bits in .bad, and leaves queues and clocks as they were."""

    def __init__(self, mat: "Materializer", n_dc: int, own_dc: int, n_part: int, cap_queued: int, order=None):
        import numpy as np
        self.mat, self.handle = mat, ctypes.c_void_p()
        self.n_dc, self.own_dc, self.n_part = n_dc, own_dc, n_part
        o = np.ascontiguousarray(order, np.uint8) if order is not None else None
        if o is not None and len(o) != n_dc:
            raise ValueError("order must name every DC once")
        self._check(mat.L.am_dep_create(mat.ctx, n_dc, own_dc, n_part, cap_queued, o.ctypes.data if o is not None else None,
                                        ctypes.byref(self.handle)), "am_dep_create")

    @staticmethod
    def _check(rc: int, what: str, bad: int = 0):
        if rc != 0:
            msg = abi.lib().am_last_error()
            e = abi.AmError(f"{what} failed rc={rc}: {msg.decode() if msg else ''}")
            e.rc, e.bad = rc, bad
            raise e

    def deliver(self, txs, now: int) -> List[List[int]]:
        """[(part, dc, timestamp, snapshot, ping, tag)] (or a DepTxns) -> per partition the tags of the
        transactions delivered by this call, in delivery order."""
        import numpy as np
        b = txs if isinstance(txs, DepTxns) else DepTxns(self.n_dc, txs)
        queued, _ = self.size()
        cap_out = queued + b.n_tx
        off, tag = np.zeros(self.n_part + 1, np.uint64), np.zeros(max(cap_out, 1), np.uint64)
        s, n, bad = b.as_struct(), ctypes.c_uint64(), ctypes.c_uint32()
        rc = self.mat.L.am_dep_deliver_host(self.handle, ctypes.byref(s), int(now), cap_out, off.ctypes.data, tag.ctypes.data,
                                            ctypes.byref(n), ctypes.byref(bad))
        self._check(rc, "am_dep_deliver_host", int(bad.value))
        return [[int(x) for x in tag[int(off[p]):int(off[p + 1])]] for p in range(self.n_part)]

    def set_clock(self, part: int, vc: Dict[int, int]):
        """set_dependency_clock: the partition's clock becomes vc."""
        import numpy as np
        row, pres = np.zeros(self.n_dc, np.uint64), 0
        for d, v in vc.items():
            row[d], pres = v, pres | (1 << d)
        self._check(self.mat.L.am_dep_set_clock(self.handle, part, row.ctypes.data, pres), "am_dep_set_clock")

    def set_drop_ping(self, on: bool):
        self._check(self.mat.L.am_dep_set_drop_ping(self.handle, 1 if on else 0), "am_dep_set_drop_ping")

    def clear(self):
        """Every queue emptied and every clock new, as after the vnodes' init/1."""
        self._check(self.mat.L.am_dep_clear(self.handle), "am_dep_clear")

    def clock(self, part: int) -> Dict[int, int]:
        import numpy as np
        row, pres = np.zeros(self.n_dc, np.uint64), ctypes.c_uint32()
        self._check(self.mat.L.am_dep_clock_host(self.handle, part, row.ctypes.data, ctypes.byref(pres)), "am_dep_clock_host")
        return {d: int(row[d]) for d in range(self.n_dc) if (pres.value >> d) & 1}

    def queue(self, part: int, dc: int) -> List[int]:
        """The queued tags of one (partition, DC), oldest first."""
        import numpy as np
        cap = 64
        while True:
            n, tag = ctypes.c_uint64(), np.zeros(cap, np.uint64)
            rc = self.mat.L.am_dep_queue(self.handle, part, dc, cap, tag.ctypes.data, ctypes.byref(n))
            if rc == abi.AM_ERR_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            self._check(rc, "am_dep_queue")
            return [int(x) for x in tag[:int(n.value)]]

    def clocks(self) -> Tuple[int, int]:
        """Device addresses of the clock matrix [n_part][n_dc] and the presence words [n_part]."""
        vc, pres = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self.mat.L.am_dep_clocks(self.handle, ctypes.byref(vc), ctypes.byref(pres)), "am_dep_clocks")
        return int(vc.value), int(pres.value)

    def gst_lanes(self) -> List[int]:
        """am_gst_local_min over this buffer's clock matrix, read in place: the n_dc + 1 lanes the
        node's GST merge starts from (absent DC = 2^64 - 1)."""
        import numpy as np
        vc, pres = self.clocks()
        host = np.zeros(self.n_dc + 1, np.uint64)
        lanes = self.mat.device_array(host)
        try:
            abi.check(self.mat.L.am_gst_local_min(self.mat.ctx, self.n_dc, self.n_part, vc, pres, None, lanes.ptr),
                      "am_gst_local_min")
            self.mat.sync()
            lanes.download(host)
            return [int(x) for x in host]
        finally:
            lanes.free()

    def reserve(self, cap_queued: int):
        self._check(self.mat.L.am_dep_reserve(self.handle, cap_queued), "am_dep_reserve")

    def size(self) -> Tuple[int, int]:
        """(queued entries, cap_queued)"""
        v = [ctypes.c_uint64() for _ in range(2)]
        self._check(self.mat.L.am_dep_size(self.handle, *[ctypes.byref(x) for x in v]), "am_dep_size")
        return tuple(int(x.value) for x in v)

    def readbacks(self) -> int:
        v = ctypes.c_uint64()
        self._check(self.mat.L.am_dep_stats(self.handle, ctypes.byref(v)), "am_dep_stats")
        return int(v.value)

    def close(self):
        if self.handle:
            if self.mat.ctx:
                self.mat.L.am_dep_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class SubBuffer:
    """The subscriber buffers of every partition a GPU owns, in HBM (am_sub): one inter_dc_sub_buf state
    machine per (partition, origin DC) stream (src/inter_dc_sub_buf.erl:57-162), for batches of rows.
    tests/subsim.py restates the reference; process() returns what serving the batch one row at a time
    through it returns.  A call that fails raises abi.AmError with the code in .rc and the validity bits
    in .bad, and leaves streams and queues as they were."""

    def __init__(self, mat: "Materializer", n_dc: int, n_part: int, cap_queued: int, logging_enabled: bool = True):
        self.mat, self.handle = mat, ctypes.c_void_p()
        self.n_dc, self.n_part = n_dc, n_part
        self._check(mat.L.am_sub_create(mat.ctx, n_dc, n_part, cap_queued, 1 if logging_enabled else 0, ctypes.byref(self.handle)),
                    "am_sub_create")

    _check = staticmethod(DepBuffer._check)

    @staticmethod
    def _gaps(n: int):
        import numpy as np
        cols = (np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint64),
                np.zeros(max(n, 1), np.uint64))
        g = abi.am_sub_gaps()
        g.part, g.dc, g.from_, g.to = (c.ctypes.data for c in cols)
        return cols, g

    def process(self, rows, columns: bool = False):
        """[(kind, part, dc, prev_opid, last_opid, timestamp, snapshot, ping, tag)] (or a SubRows) ->
        (per partition the delivered tags in delivery order, the gaps [(part, dc, from, to)] in
        triggering-row order, the counters {delivered, gaps, dropped, unexpected, queued}).  With
        columns=True the first element is instead the delivered transactions as a DepTxns, partition-major,
        and a fourth element holds its offsets [n_part + 1]."""
        import numpy as np
        b = rows if isinstance(rows, SubRows) else SubRows(self.n_dc, rows)
        queued, _ = self.size()
        cap_out = queued + b.n_rows
        m = max(cap_out, 1)
        off = np.zeros(self.n_part + 1, np.uint64)
        part, dc, ts = np.zeros(m, np.uint32), np.zeros(m, np.uint8), np.zeros(m, np.uint64)
        snap, ping, tag = np.zeros((m, self.n_dc), np.uint64), np.zeros(m, np.uint8), np.zeros(m, np.uint64)
        out = abi.am_dep_txns()
        out.part, out.dc, out.timestamp, out.snap_vc, out.ping, out.tag = (a.ctypes.data for a in (part, dc, ts, snap, ping, tag))
        gcols, g = self._gaps(b.n_rows)
        s, cnt, bad = b.as_struct(), np.zeros(5, np.uint64), ctypes.c_uint32()
        rc = self.mat.L.am_sub_process_host(self.handle, ctypes.byref(s), cap_out, off.ctypes.data, ctypes.byref(out), b.n_rows,
                                            ctypes.byref(g), cnt.ctypes.data, ctypes.byref(bad))
        self._check(rc, "am_sub_process_host", int(bad.value))
        counters = dict(zip(abi.SUB_COUNTS, (int(x) for x in cnt)))
        gaps = [(int(gcols[0][i]), int(gcols[1][i]), int(gcols[2][i]), int(gcols[3][i])) for i in range(counters["gaps"])]
        nd = counters["delivered"]
        if columns:
            return DepTxns.from_columns(self.n_dc, part[:nd], dc[:nd], ts[:nd], snap[:nd], ping[:nd], tag[:nd]), gaps, counters, off
        return [[int(x) for x in tag[int(off[p]):int(off[p + 1])]] for p in range(self.n_part)], gaps, counters

    def deliver_into(self, dep: DepBuffer, rows, now: int):
        """process(rows), then dep.deliver of what came out in order, without the columns leaving HBM
        (am_sub_deliver) -> (per partition the tags am_dep delivered, the gaps, the counters)."""
        import numpy as np
        b = rows if isinstance(rows, SubRows) else SubRows(self.n_dc, rows)
        cap_out = dep.size()[0] + self.size()[0] + b.n_rows
        off, tag = np.zeros(self.n_part + 1, np.uint64), np.zeros(max(cap_out, 1), np.uint64)
        gcols, g = self._gaps(b.n_rows)
        s, cnt, bad, n = b.as_struct(), np.zeros(5, np.uint64), ctypes.c_uint32(), ctypes.c_uint64()
        rc = self.mat.L.am_sub_deliver_host(self.handle, dep.handle, ctypes.byref(s), int(now), cap_out, off.ctypes.data,
                                            tag.ctypes.data, ctypes.byref(n), b.n_rows, ctypes.byref(g), cnt.ctypes.data,
                                            ctypes.byref(bad))
        self._check(rc, "am_sub_deliver_host", int(bad.value))
        counters = dict(zip(abi.SUB_COUNTS, (int(x) for x in cnt)))
        gaps = [(int(gcols[0][i]), int(gcols[1][i]), int(gcols[2][i]), int(gcols[3][i])) for i in range(counters["gaps"])]
        return [[int(x) for x in tag[int(off[p]):int(off[p + 1])]] for p in range(self.n_part)], gaps, counters

    def set_last(self, part: int, dc: int, opid: int):
        """last_observed_opid of one stream: what request_op_id/3 returned after a restart."""
        self._check(self.mat.L.am_sub_set_last(self.handle, part, dc, int(opid)), "am_sub_set_last")

    def set_reachable(self, dcs):
        """The DCs whose log reader answers: an iterable of DC indices, or a bit mask."""
        mask = dcs if isinstance(dcs, int) else sum(1 << d for d in set(dcs))
        self._check(self.mat.L.am_sub_set_reachable(self.handle, mask & 0xFFFFFFFF), "am_sub_set_reachable")

    def clear(self):
        """Every queue emptied and every stream at last = 0 in normal mode."""
        self._check(self.mat.L.am_sub_clear(self.handle), "am_sub_clear")

    def stream(self, part: int, dc: int) -> Tuple[int, int, List[int]]:
        """(last_observed_opid, mode, the queued tags oldest first) of one stream."""
        import numpy as np
        cap = 64
        while True:
            last, mode, n, tag = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64(), np.zeros(cap, np.uint64)
            rc = self.mat.L.am_sub_stream(self.handle, part, dc, ctypes.byref(last), ctypes.byref(mode), cap, tag.ctypes.data,
                                          ctypes.byref(n))
            if rc == abi.AM_ERR_CAPACITY and n.value > cap:
                cap = int(n.value)
                continue
            self._check(rc, "am_sub_stream")
            return int(last.value), int(mode.value), [int(x) for x in tag[:int(n.value)]]

    def reserve(self, cap_queued: int):
        self._check(self.mat.L.am_sub_reserve(self.handle, cap_queued), "am_sub_reserve")

    def size(self) -> Tuple[int, int]:
        """(queued entries, cap_queued)"""
        v = [ctypes.c_uint64() for _ in range(2)]
        self._check(self.mat.L.am_sub_size(self.handle, *[ctypes.byref(x) for x in v]), "am_sub_size")
        return tuple(int(x.value) for x in v)

    def stats(self) -> Dict[str, int]:
        """Counters since create: status-block readbacks."""
        v = ctypes.c_uint64()
        self._check(self.mat.L.am_sub_stats(self.handle, ctypes.byref(v)), "am_sub_stats")
        return {"readbacks": int(v.value)}

    def close(self):
        if self.handle:
            if self.mat.ctx:
                self.mat.L.am_sub_destroy(self.handle)
            self.handle = ctypes.c_void_p()


class Materializer:
    """A context on one GPU (device index = local rank)."""

    def __init__(self, device: int = 0):
        self.L = abi.lib()
        self.ctx = ctypes.c_void_p()
        abi.check(self.L.am_ctx_open(device, ctypes.byref(self.ctx)), "am_ctx_open")
        self.device = device

    def close(self):
        if self.ctx:
            self.L.am_ctx_close(self.ctx)
            self.ctx = ctypes.c_void_p()

    def sync(self):
        abi.check(self.L.am_ctx_sync(self.ctx), "am_ctx_sync")

    # ---- ops cache ----
    def store(self, log: HostLog) -> Store:
        h = ctypes.c_void_p()
        s = log.as_struct()
        abi.check(self.L.am_store_create(self.ctx, ctypes.byref(s), ctypes.byref(h)), "am_store_create")
        return Store(self, h, log.n_dc)

    def device_array(self, arr) -> "_DevBuf":
        """A caller-owned copy of a host array in HBM (free with .free())."""
        import numpy as np
        return _DevBuf.of(self, np.ascontiguousarray(arr))

    def load_ops(self, n_dc: int, ops_by_key: Sequence[Sequence[Op]], key_types) -> "Vnode":
        """load_from_log_to_tables/2 -> load_ops/2 (src/materializer_vnode.erl:288-319): every
        committed op of every key, in log order, through op_insert_gc/3 -- ids 1, 2, ... per
        key and the write-triggered GC reads (snapshots cached, ops pruned, ListLen resized)
        exactly as the reference replays its log.  Returns the partition's Vnode."""
        vn = Vnode(self, n_dc, len(ops_by_key))
        vn.insert(ops_by_key, key_types)
        return vn

    def synth_store(self, params: abi.am_synth_params) -> Store:
        h = ctypes.c_void_p()
        abi.check(self.L.am_synth_store(self.ctx, ctypes.byref(params), ctypes.byref(h)), "am_synth_store")
        return Store(self, h, params.n_dc)

    # ---- the hot path ----
    def read_batch(self, store: Store, reads: Sequence[Read], set_capacity=None) -> HostBatch:
        """materializer_vnode:read/6 -> materialize/4 for a batch of keys (host memory in/out)."""
        hb = HostBatch(store.n_dc, reads, set_capacity)
        b, r = hb.structs()
        abi.check(self.L.am_materialize_host(self.ctx, store.handle, ctypes.byref(b), ctypes.byref(r)),
                  "am_materialize_host")
        return hb

    # ---- snapshot cache (materializer_vnode snapshot_cache-P in HBM) ----
    def snapshot_cache(self, store: Store, n_keys: int) -> "SnapshotCache":
        return SnapshotCache(self, store, n_keys)

    def vnode(self, n_dc: int, n_keys: int, logged: bool = False) -> Vnode:
        return Vnode(self, n_dc, n_keys, logged)

    def certifier(self, cap_keys: int, cap_entries: int, record_commits: bool = True) -> Certifier:
        return Certifier(self, cap_keys, cap_entries, record_commits)

    def dep_buffer(self, n_dc: int, own_dc: int, n_part: int, cap_queued: int, order=None) -> DepBuffer:
        return DepBuffer(self, n_dc, own_dc, n_part, cap_queued, order)

    def sub_buffer(self, n_dc: int, n_part: int, cap_queued: int, logging_enabled: bool = True) -> SubBuffer:
        return SubBuffer(self, n_dc, n_part, cap_queued, logging_enabled)

    def partition_log(self, n_dc: int, cap_tx: int = 1024, cap_eff: int = 4096, cap_var: int = 4096) -> PartitionLog:
        return PartitionLog(self, n_dc, cap_tx, cap_eff, cap_var)

    def materialize(self, type_: int, txid: Optional[int], min_snapshot_time: Dict[int, int],
                    ops_newest_first: Sequence[Tuple[int, Op]], base_clock: Optional[Dict[int, int]] = None,
                    base_last_op: int = 0, base_value: Any = None, n_dc: Optional[int] = None):
        """clocksi_materializer:materialize/4 for one key, with the #snapshot_get_response{} given
        as its parts (ops list newest first, as the reference passes it)."""
        ops = [op for _, op in reversed(list(ops_newest_first))]
        ids = [i for i, _ in reversed(list(ops_newest_first))]
        for op, i in zip(ops, ids):
            op.op_id = i
        dcs = set(min_snapshot_time) | set(base_clock or {})
        for op in ops:
            dcs |= set(op.snap) | {op.commit_dc}
        nd = n_dc or (max(dcs) + 1 if dcs else 1)
        log = HostLog(nd, [ops], key_types=[type_])
        st = self.store(log)
        try:
            hb = self.read_batch(st, [Read(0, type_, dict(min_snapshot_time), txid, base_clock, base_last_op,
                                           base_value)])
            return hb.result(0)
        finally:
            st.close()

    def materialize_eager(self, n_dc: int, entries: Sequence[Tuple[int, Any, Sequence[Any]]],
                          set_capacity: Optional[Sequence[int]] = None,
                          in_status: Optional[Sequence[int]] = None) -> HostBatch:
        """materializer:materialize_eager/3 (src/materializer.erl:62-70) for a batch (host memory in
        and out, am_materialize_eager_host).  entries: [(Type, Snapshot, [Effect])], the snapshot as
        Read.base_value takes it (None = Type:new()), the effects oldest first as encode_effect
        takes them ("bad": an effect Type:update/2 raises on).  in_status: per entry, a failed
        snapshot read's status to pass through.  Returns a HostBatch whose status[i] / value(i)
        are entry i's outcome."""
        ws = WriteSet([(i, t, effs) for i, (t, _, effs) in enumerate(entries)])
        return self.materialize_eager_rows(n_dc, [(t, base) for t, base, _ in entries], ws, set_capacity, in_status)

    def materialize_eager_rows(self, n_dc: int, values: Sequence[Tuple[int, Any]], ws: WriteSet,
                               set_capacity: Optional[Sequence[int]] = None,
                               in_status: Optional[Sequence[int]] = None) -> HostBatch:
        """The same over a value batch [(Type, Snapshot)] and a WriteSet whose entries name rows
        of it (am_writeset.row); in_status per row of the value batch.  Entry i of the returned
        HostBatch is write-set entry i's outcome."""
        import numpy as np
        hin = HostBatch(n_dc, [Read(i, t, {}, base_value=base) for i, (t, base) in enumerate(values)])
        hout = HostBatch(n_dc, [Read(i, t, {}) for i, (_, t, _) in enumerate(ws.entries)], set_capacity)
        if not ws.entries:
            return hout
        b, _ = hin.structs()
        _, r = hout.structs()
        w = ws.as_struct()
        ist = np.ascontiguousarray(in_status, np.int32) if in_status is not None else None
        abi.check(self.L.am_materialize_eager_host(self.ctx, n_dc, ctypes.byref(w), ctypes.byref(b.base),
                                                   ist.ctypes.data if ist is not None else None,
                                                   ctypes.byref(r.value), hout.status.ctypes.data),
                  "am_materialize_eager_host")
        return hout

    # ---- downstream generation (clocksi_downstream:generate_downstream_op/6) ----
    @staticmethod
    def downstream_capacity(hin: HostBatch, ups: Updates) -> int:
        """An upper bound of the effects' variable words: per update the row's pairs (every token
        once) plus a header per state element and per requested element, and the add tokens."""
        cap = 0
        for i, (r, _, _) in enumerate(ups.entries):
            cap += 4 * int(hin.b_set_len[r]) + 4 * int(ups.var_off[i + 1] - ups.var_off[i])
        return cap

    def generate_downstream(self, n_dc: int, values: Sequence[Tuple[int, Any]], updates, tokens=None,
                            in_status: Optional[Sequence[int]] = None, var_cap: Optional[int] = None):
        """Type:downstream/2 for a batch on the device (am_generate_downstream_host).  values:
        [(Type, Snapshot)] as materialize_eager_rows takes them; updates: [(row, type, update)]
        (oplog.Updates' shapes, rows distinct) or an Updates; tokens: a callable returning fresh
        interned tokens.  Returns ([effect | ('error', status)], avail[n_up], Effects)."""
        import numpy as np
        ups = updates if isinstance(updates, Updates) else Updates(updates, tokens)
        hin = HostBatch(n_dc, [Read(i, t, {}, base_value=base) for i, (t, base) in enumerate(values)])
        eff = Effects(ups, self.downstream_capacity(hin, ups) if var_cap is None else var_cap)
        b, _ = hin.structs()
        u, e = ups.as_struct(), eff.as_struct()
        ist = np.ascontiguousarray(in_status, np.int32) if in_status is not None else None
        abi.check(self.L.am_generate_downstream_host(self.ctx, n_dc, ctypes.byref(u), ctypes.byref(b.base),
                                                     ist.ctypes.data if ist is not None else None, ctypes.byref(e),
                                                     eff.status.ctypes.data), "am_generate_downstream_host")
        return eff.effects(), [int(a) for a in eff.avail[:ups.n_up]], eff

    def update_rounds(self, n_dc: int, values: Sequence[Tuple[int, Any]], tx_updates, tokens=None,
                      set_capacity: int = 4096) -> list:
        """A transaction's updates [(row, type, update)], repeated rows allowed, in order: the
        reference generates them one after another, each seeing the write set so far
        (src/clocksi_interactive_coord.erl:986).  Here round j takes every row's j-th update (rows
        distinct within a round), and after each round that round's effects are folded into the
        values with materialize_eager_rows.  Returns the effects in update order."""
        vals = list(values)
        seen: Dict[int, int] = {}
        rounds: List[List[int]] = []
        for q, (r, _, _) in enumerate(tx_updates):
            j = seen.get(r, 0)
            seen[r] = j + 1
            if j == len(rounds):
                rounds.append([])
            rounds[j].append(q)
        out: List[Any] = [None] * len(tx_updates)
        for sel in rounds:
            effs, _, eff = self.generate_downstream(n_dc, vals, [tx_updates[q] for q in sel], tokens)
            for q, e in zip(sel, effs):
                out[q] = e
            ok = [i for i, e in enumerate(effs) if not (isinstance(e, tuple) and e and e[0] == "error")]
            if not ok:
                continue
            ws = WriteSet([(eff.updates.entries[i][0], eff.updates.entries[i][1], [effs[i]]) for i in ok])
            hb = self.materialize_eager_rows(n_dc, vals, ws, [set_capacity] * len(ok))
            for k, i in enumerate(ok):
                if int(hb.status[k]) != 0:
                    raise abi.AmError(f"update_rounds: folding update {sel[i]} failed (status {int(hb.status[k])})")
                r, t = eff.updates.entries[i][0], eff.updates.entries[i][1]
                vals[r] = (t, hb.value(k))
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
