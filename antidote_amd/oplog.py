"""Host-side encoding of the reference's ops cache into the HBM structure-of-arrays
layout of include/antidote_mat.h (am_op_log), read batches (am_read_batch) and
their decoding (am_read_result).

This is the ingestion side of materializer_vnode:op_insert_gc/3
(src/materializer_vnode.erl:622-647): one #clocksi_payload{} (include/antidote.hrl:197-204)
becomes one row of the op columns; ops of a key stay oldest -> newest, as in the
ETS tuple (slots FIRST_OP..FIRST_OP+Length-1, include/antidote.hrl:81-90).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi

U64 = np.uint64


@dataclass
class Op:
    """One committed effect (#clocksi_payload{}) with DCs already mapped to indices."""
    type: int
    commit_dc: int
    commit_time: int
    snap: Dict[int, int]                 # snapshot_time as {dc_index: time}
    effect: Any                          # see encode_effect
    txid: Optional[int] = None
    op_id: Optional[int] = None
    bad: bool = False                    # Type:update/2 raises on this effect


def encode_effect(type_: int, eff) -> Tuple[int, int, int, List[int]]:
    """-> (kind, p0, p1, var words).  Effect shapes (antidote_crdt downstream effects):
    PN int | LWW (ts, value) | MV ('assign', value, token, [overridden]) or ('reset', [overridden])
    | AWSET [(elem, [add_tokens], [remove_tokens]), ...] sorted by elem
    | BCOUNTER ('increment', V, id) | ('decrement', V, id) | ('transfer', V, to, from)."""
    if type_ == abi.AM_PN:
        return 0, int(eff) & 0xFFFFFFFFFFFFFFFF, 0, []
    if type_ == abi.AM_LWW:
        ts, val = eff
        return 0, int(ts), int(val), []
    if type_ == abi.AM_MVREG:
        if eff[0] == "reset":
            return 1, 0, 0, [int(t) for t in eff[1]]
        _, val, tok, ovr = eff
        return 0, int(val), int(tok), [int(t) for t in ovr]
    if type_ == abi.AM_AWSET:
        words: List[int] = []
        for elem, add, rm in eff:
            words += [int(elem), len(add), len(rm)] + [int(t) for t in add] + [int(t) for t in rm]
        return 0, 0, 0, words
    if type_ == abi.AM_BCOUNTER:
        kind = {"increment": 0, "decrement": 1, "transfer": 2}[eff[0]]
        if kind == 2:
            _, v, to, frm = eff
        else:
            _, v, frm = eff
            to = frm
        return kind, int(v) & 0xFFFFFFFFFFFFFFFF, int(frm) | (int(to) << 8), []
    raise ValueError(type_)


class HostLog:
    """SoA op log in host memory (numpy), the layout am_store_create uploads."""

    def __init__(self, n_dc: int, keys: Sequence[Sequence[Op]], key_types: Optional[Sequence[int]] = None,
                 key_id_base: Optional[Sequence[int]] = None, partial: Optional[bool] = None):
        if not 1 <= n_dc <= abi.AM_MAX_DC:
            raise ValueError("n_dc out of range")
        self.n_dc = n_dc
        n_keys = len(keys)
        lens = [len(k) for k in keys]
        n_ops = int(sum(lens))
        self.n_keys, self.n_ops = n_keys, n_ops
        self.key_off = np.zeros(n_keys + 1, U64)
        self.key_off[1:] = np.cumsum(lens, dtype=U64)
        self.key_type = np.zeros(max(n_keys, 1), np.uint8)
        self.key_flags = np.zeros(max(n_keys, 1), np.uint8)
        n_alloc = max(n_ops, 1)
        self.op_meta = np.zeros(n_alloc, np.uint8)
        self.commit_time = np.zeros(n_alloc, U64)
        self.snap_vc = np.zeros((n_dc, n_alloc), U64)
        self.snap_pres = np.zeros(n_alloc, np.uint32)
        self.p0 = np.zeros(n_alloc, U64)
        self.p1 = np.zeros(n_alloc, U64)
        self.var_off = np.zeros(n_ops + 1, U64)
        var: List[int] = []
        all_mask = (1 << n_dc) - 1
        need_pres = False
        has_txid = any(op.txid is not None for k in keys for op in k)
        has_opid = any(op.op_id is not None for k in keys for op in k)
        self.op_txid = np.zeros(n_alloc, U64) if has_txid else None
        self.op_id = np.zeros(n_alloc, U64) if has_opid else None
        self.key_id_base = np.asarray(key_id_base, U64) if key_id_base is not None else None
        q = 0
        for k, ops in enumerate(keys):
            types = {op.type for op in ops}
            if key_types is not None:
                self.key_type[k] = key_types[k]
            elif ops:
                self.key_type[k] = ops[0].type
            if len(types) > 1 or (key_types is not None and types and types != {key_types[k]}):
                self.key_flags[k] |= abi.AM_KEY_MIXED_TYPES
            for op in ops:
                kind, p0, p1, words = encode_effect(op.type, op.effect) if not op.bad else (0, 0, 0, [])
                self.op_meta[q] = abi.make_meta(op.commit_dc, kind, op.bad)
                self.commit_time[q] = op.commit_time
                pres = 0
                for d, t in op.snap.items():
                    self.snap_vc[d, q] = t
                    pres |= 1 << d
                self.snap_pres[q] = pres
                if pres != all_mask:
                    need_pres = True
                self.p0[q] = p0
                self.p1[q] = p1
                var += words
                self.var_off[q + 1] = len(var)
                if has_txid:
                    self.op_txid[q] = 0 if op.txid is None else op.txid
                if has_opid:
                    self.op_id[q] = op.op_id
                q += 1
        if partial is False:
            need_pres = False
        if not need_pres and partial is not True:
            self.snap_pres = None
        self.var_data = np.asarray(var if var else [0], U64)
        self.n_var = len(var)
        self.has_var = self.n_var > 0
        self._struct = None

    def as_struct(self) -> abi.am_op_log:
        s = abi.am_op_log()
        s.n_dc, s.n_keys, s.n_ops, s.n_var = self.n_dc, self.n_keys, self.n_ops, self.n_var
        s.snap_stride = self.snap_vc.shape[1]
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        s.key_off, s.key_id_base, s.key_type, s.key_flags = (p(self.key_off), p(self.key_id_base),
                                                             p(self.key_type), p(self.key_flags))
        s.op_meta, s.commit_time, s.snap_vc, s.snap_pres = (p(self.op_meta), p(self.commit_time),
                                                            p(self.snap_vc), p(self.snap_pres))
        s.op_txid, s.op_id, s.p0, s.p1 = p(self.op_txid), p(self.op_id), p(self.p0), p(self.p1)
        s.var_off = p(self.var_off) if self.has_var else None
        s.var_data = p(self.var_data) if self.has_var else None
        self._struct = s
        return s


@dataclass
class Read:
    """Inputs of one materialize/4 call for one key of the log."""
    key: int
    type: int
    clock: Dict[int, int]                        # MinSnapshotTime
    txid: Optional[int] = None                   # None = ignore
    base_clock: Optional[Dict[int, int]] = None  # None = ignore
    base_last_op: int = 0
    base_value: Any = None                       # None = Type:new()


def _pres(clock: Dict[int, int]) -> int:
    m = 0
    for d in clock:
        m |= 1 << d
    return m


def bc_pairs(value, n_dc: int) -> List[Tuple[int, int]]:
    """A bounded counter's ({(From, To): N}, {Id: N}) as the ABI's (slot, value) entries: P at
    From*n_dc+To, then D at n_dc*n_dc+Id, slot order (include/antidote_mat.h am_values)."""
    pdict, ddict = value
    out = [(f * n_dc + t, int(v)) for (f, t), v in pdict.items()] + [(n_dc * n_dc + d, int(v)) for d, v in ddict.items()]
    return [(s, int(np.array([v], np.int64).view(np.uint64)[0])) for s, v in sorted(out)]


def bc_dicts(pairs, n_dc: int):
    """The inverse of bc_pairs: (slot, value-bits) entries -> ({(From, To): N}, {Id: N})."""
    pd, dd = {}, {}
    for s, v in pairs:
        x = int(np.array([v], np.uint64).view(np.int64)[0])
        if s < n_dc * n_dc:
            pd[(s // n_dc, s % n_dc)] = x
        else:
            dd[s - n_dc * n_dc] = x
    return pd, dd


class HostBatch:
    """am_read_batch + am_read_result in host memory."""

    def __init__(self, n_dc: int, reads: Sequence[Read], set_capacity: Optional[Sequence[int]] = None):
        n = len(reads)
        self.n, self.n_dc, self.reads = n, n_dc, list(reads)
        self.key = np.asarray([r.key for r in reads] or [0], U64)
        self.type = np.asarray([r.type for r in reads] or [0], np.uint8)
        types = {r.type for r in reads}
        self.type_hint = types.pop() if len(types) == 1 else 0
        self.read_vc = np.zeros((n_dc, max(n, 1)), U64)
        self.read_pres = np.zeros(max(n, 1), np.uint32)
        self.txid = np.zeros(max(n, 1), U64)
        self.txid_valid = np.zeros(max(n, 1), np.uint8)
        self.base_ignore = np.ones(max(n, 1), np.uint8)
        self.base_vc = np.zeros((n_dc, max(n, 1)), U64)
        self.base_pres = np.zeros(max(n, 1), np.uint32)
        self.base_last_op = np.zeros(max(n, 1), np.int64)
        self.b_v0 = np.zeros(max(n, 1), np.int64)
        self.b_v1 = np.zeros(max(n, 1), U64)
        self.b_vflag = np.ones(max(n, 1), np.uint8)
        base_pairs: List[List[Tuple[int, int]]] = []
        for i, r in enumerate(reads):
            for d, t in r.clock.items():
                self.read_vc[d, i] = t
            self.read_pres[i] = _pres(r.clock)
            if r.txid is not None:
                self.txid[i] = r.txid
                self.txid_valid[i] = 1
            if r.base_clock is not None:
                self.base_ignore[i] = 0
                for d, t in r.base_clock.items():
                    self.base_vc[d, i] = t
                self.base_pres[i] = _pres(r.base_clock)
            self.base_last_op[i] = r.base_last_op
            pairs: List[Tuple[int, int]] = []
            bv = r.base_value
            if bv is not None:
                if r.type == abi.AM_PN:
                    self.b_v0[i] = bv
                elif r.type == abi.AM_LWW:
                    ts, val, isbin = bv
                    self.b_v0[i] = np.array([ts], np.uint64).view(np.int64)[0]
                    self.b_v1[i] = val
                    self.b_vflag[i] = 1 if isbin else 0
                elif r.type == abi.AM_AWSET:  # the orddict in state order (elems ascending)
                    pairs = [(int(a), int(b)) for a, b in bv]
                elif r.type == abi.AM_MVREG:  # a sorted list of {Value, Token}
                    pairs = sorted((int(a), int(b)) for a, b in bv)
                elif r.type == abi.AM_BCOUNTER:  # the P / D orddicts as (slot, value) entries
                    pairs = bc_pairs(bv, n_dc)
            base_pairs.append(pairs)
        self.has_txid = any(r.txid is not None for r in reads)
        self.has_base = any(r.base_clock is not None for r in reads)
        # base set CSR
        lens = [len(p) for p in base_pairs]
        self.b_set_off = np.zeros(n + 1, U64)
        self.b_set_off[1:] = np.cumsum(lens, dtype=U64) if n else []
        flat = [x for p in base_pairs for x in p]
        self.b_set_len = np.asarray(lens or [0], np.uint32)
        self.b_set_a = np.asarray([a for a, _ in flat] or [0], U64)
        self.b_set_b = np.asarray([b for _, b in flat] or [0], U64)
        # results
        self.status = np.full(max(n, 1), 99, np.int32)
        self.new_last_op = np.zeros(max(n, 1), np.int64)
        self.last_ct = np.zeros((n_dc, max(n, 1)), U64)
        self.last_ct_pres = np.zeros(max(n, 1), np.uint32)
        self.last_ct_ignore = np.zeros(max(n, 1), np.uint8)
        self.is_new_ss = np.zeros(max(n, 1), np.uint8)
        self.count = np.zeros(max(n, 1), np.uint32)
        self.flags = np.zeros(max(n, 1), np.uint8)
        self.v0 = np.zeros(max(n, 1), np.int64)
        self.v1 = np.zeros(max(n, 1), U64)
        self.vflag = np.zeros(max(n, 1), np.uint8)
        # default room per read: 64 set pairs; every orddict entry of a bounded counter
        caps = (list(set_capacity) if set_capacity is not None else
                [max(64, n_dc * n_dc + n_dc) if r.type == abi.AM_BCOUNTER else 64 for r in reads])
        self.o_set_off = np.zeros(n + 1, U64)
        self.o_set_off[1:] = np.cumsum(caps, dtype=U64) if n else []
        tot = int(self.o_set_off[-1]) if n else 0
        self.o_set_len = np.zeros(max(n, 1), np.uint32)
        self.o_set_a = np.zeros(max(tot, 1), U64)
        self.o_set_b = np.zeros(max(tot, 1), U64)

    def structs(self):
        p = lambda a: a.ctypes.data  # noqa: E731
        b = abi.am_read_batch()
        b.n_reads, b.per_read_clock, b.type_hint = self.n, 1, self.type_hint
        b.key, b.type, b.read_vc, b.read_pres = p(self.key), p(self.type), p(self.read_vc), p(self.read_pres)
        if self.has_txid:
            b.txid, b.txid_valid = p(self.txid), p(self.txid_valid)
        b.base_ignore = p(self.base_ignore)
        b.base_vc, b.base_pres, b.base_last_op = p(self.base_vc), p(self.base_pres), p(self.base_last_op)
        bv = b.base
        bv.v0, bv.v1, bv.vflag = p(self.b_v0), p(self.b_v1), p(self.b_vflag)
        bv.set_off, bv.set_len, bv.set_a, bv.set_b = (p(self.b_set_off), p(self.b_set_len), p(self.b_set_a),
                                                      p(self.b_set_b))
        r = abi.am_read_result()
        r.status, r.new_last_op, r.last_ct, r.last_ct_pres = (p(self.status), p(self.new_last_op), p(self.last_ct),
                                                              p(self.last_ct_pres))
        r.last_ct_ignore, r.is_new_ss, r.count, r.flags = (p(self.last_ct_ignore), p(self.is_new_ss),
                                                           p(self.count), p(self.flags))
        rv = r.value
        rv.v0, rv.v1, rv.vflag = p(self.v0), p(self.v1), p(self.vflag)
        rv.set_off, rv.set_len, rv.set_a, rv.set_b = (p(self.o_set_off), p(self.o_set_len), p(self.o_set_a),
                                                      p(self.o_set_b))
        self._keep = (b, r)
        return b, r

    # ---- decoding ----
    def value(self, i: int):
        t = self.reads[i].type
        if t == abi.AM_PN:
            return int(self.v0[i])
        if t == abi.AM_LWW:
            return (int(self.v0[i:i + 1].view(np.uint64)[0]), int(self.v1[i]), bool(self.vflag[i]))
        if t in (abi.AM_AWSET, abi.AM_MVREG):
            o, n = int(self.o_set_off[i]), int(self.o_set_len[i])
            return [(int(self.o_set_a[o + j]), int(self.o_set_b[o + j])) for j in range(n)]
        if t == abi.AM_BCOUNTER:
            o, n = int(self.o_set_off[i]), int(self.o_set_len[i])
            return bc_dicts([(int(self.o_set_a[o + j]), int(self.o_set_b[o + j])) for j in range(n)], self.n_dc)
        raise ValueError(t)

    def result(self, i: int):
        """('ok', Value, NewLastOp, LastOpCt, IsNewSS, Count, flags) or ('error', status)."""
        st = int(self.status[i])
        if st != 0:
            return ("error", st)
        ct = None if self.last_ct_ignore[i] else {d: int(self.last_ct[d, i]) for d in range(self.n_dc)
                                                   if (int(self.last_ct_pres[i]) >> d) & 1}
        return ("ok", self.value(i), int(self.new_last_op[i]), ct, bool(self.is_new_ss[i]), int(self.count[i]),
                int(self.flags[i]))


class WriteSet:
    """am_writeset in host memory: the reading transactions' own effects for some rows of a value
    batch (reverse_and_filter_updates_per_key/2's output per key, src/clocksi_vnode.erl:660-668).

    entries: [(row, type, [effect, ...])], each effect list in application order (oldest first),
    effects shaped as encode_effect takes them; an effect given as the string "bad" is one
    Type:update/2 raises on (AM_META_BAD)."""

    def __init__(self, entries: Sequence[Tuple[int, int, Sequence[Any]]]):
        self.entries = [(int(r), int(t), list(e)) for r, t, e in entries]
        n = len(self.entries)
        self.n_ws = n
        self.row = np.asarray([r for r, _, _ in self.entries] or [0], U64)
        self.type = np.asarray([t for _, t, _ in self.entries] or [0], np.uint8)
        self.eff_off = np.zeros(n + 1, U64)
        meta: List[int] = []
        p0: List[int] = []
        p1: List[int] = []
        var: List[int] = []
        var_off = [0]
        for i, (_, t, effs) in enumerate(self.entries):
            for eff in effs:
                bad = isinstance(eff, str) and eff == "bad"
                kind, a, b, words = (0, 0, 0, []) if bad else encode_effect(t, eff)
                meta.append(abi.make_meta(0, kind, bad))
                p0.append(a & 0xFFFFFFFFFFFFFFFF)
                p1.append(b & 0xFFFFFFFFFFFFFFFF)
                var += [w & 0xFFFFFFFFFFFFFFFF for w in words]
                var_off.append(len(var))
            self.eff_off[i + 1] = len(meta)
        self.n_eff, self.n_var = len(meta), len(var)
        self.eff_meta = np.asarray(meta or [0], np.uint8)
        self.p0 = np.asarray(p0 or [0], U64)
        self.p1 = np.asarray(p1 or [0], U64)
        self.var_off = np.asarray(var_off, U64)
        self.var_data = np.asarray(var or [0], U64)

    def as_struct(self) -> abi.am_writeset:
        s = abi.am_writeset()
        s.n_ws, s.n_eff, s.n_var = self.n_ws, self.n_eff, self.n_var
        p = lambda a: a.ctypes.data  # noqa: E731
        s.row, s.type, s.eff_off, s.eff_meta = p(self.row), p(self.type), p(self.eff_off), p(self.eff_meta)
        s.p0, s.p1, s.var_off, s.var_data = p(self.p0), p(self.p1), p(self.var_off), p(self.var_data)
        self._struct = s
        return s

    def effect(self, i: int, j: int) -> Tuple[int, int, int, List[int]]:
        """Effect j of entry i decoded from the columns: (meta, p0, p1, var words)."""
        q = int(self.eff_off[i]) + j
        return (int(self.eff_meta[q]), int(self.p0[q]), int(self.p1[q]),
                [int(w) for w in self.var_data[int(self.var_off[q]):int(self.var_off[q + 1])]])

    @classmethod
    def from_columns(cls, row, type_, eff_off, eff_meta, p0, p1, var_off, var_data, entries) -> "WriteSet":
        """A write set over columns already in the ABI's encoding (Effects.as_writeset)."""
        ws = cls.__new__(cls)
        ws.entries = entries
        ws.n_ws, ws.n_eff, ws.n_var = len(entries), int(eff_off[-1]), int(var_off[-1])
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        ws.row, ws.type, ws.eff_off = c(row, U64), c(type_, np.uint8), np.ascontiguousarray(eff_off, U64)
        ws.eff_meta, ws.p0, ws.p1 = c(eff_meta, np.uint8), c(p0, U64), c(p1, U64)
        ws.var_off, ws.var_data = np.ascontiguousarray(var_off, U64), c(var_data, U64)
        return ws


def _u64(x: int) -> int:
    return int(x) & 0xFFFFFFFFFFFFFFFF


def _i64(x: int) -> int:
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >> 63 else x


def decode_effect(type_: int, meta: int, p0: int, p1: int, words: Sequence[int]):
    """The inverse of encode_effect: an effect's columns -> the shape encode_effect takes."""
    kind = (meta >> 5) & 3
    words = [int(w) for w in words]
    if type_ == abi.AM_PN:
        return _i64(p0)
    if type_ == abi.AM_LWW:
        return (int(p0), int(p1))
    if type_ == abi.AM_MVREG:
        return ("reset", words) if kind == 1 else ("assign", int(p0), int(p1), words)
    if type_ == abi.AM_AWSET:
        out, q = [], 0
        while q < len(words):
            e, na, nr = words[q:q + 3]
            out.append((e, words[q + 3:q + 3 + na], words[q + 3 + na:q + 3 + na + nr]))
            q += 3 + na + nr
        return out
    if type_ == abi.AM_BCOUNTER:
        frm, to = int(p1) & 0xFF, (int(p1) >> 8) & 0xFF
        if kind == 2:
            return ("transfer", _i64(p0), to, frm)
        return ("increment" if kind == 0 else "decrement", _i64(p0), frm)
    raise ValueError(type_)


class Updates:
    """am_updates in host memory: client updates for some rows of a value batch, the input of
    generate_downstream_op/6 (src/clocksi_downstream.erl:41-68).

    entries: [(row, type, update)].  Updates per type (labels are u64, as the codec interns them):
      PN        ("increment", N) | ("decrement", N)
      LWW       ("assign", ts, value)               ts = the caller's make_micro_epoch()
      AWSET     ("add", E) | ("add_all", [E]) | ("remove", E) | ("remove_all", [E]) | ("reset",)
      MVREG     ("assign", Value) | ("reset",)
      BCOUNTER  ("increment", (N, Dc)) | ("decrement", (N, Dc)) | ("transfer", (N, To, From))
    The element lists are sorted and deduplicated here (lists:usort).  tokens: a callable returning
    one fresh interned token per call -- one per added element (in element order) and one per MV
    assign; self.tokens[i] lists the ones update i took.  An update given as ("raw", op, a0, a1,
    [words]) is encoded as is (malformed inputs)."""

    def __init__(self, entries: Sequence[Tuple[int, int, Sequence[Any]]], tokens=None):
        self.entries = [(int(r), int(t), tuple(u)) for r, t, u in entries]
        n = len(self.entries)
        self.n_up = n
        row, typ, op, a0, a1, var, var_off = [], [], [], [], [], [], [0]
        self.tokens: List[List[int]] = []

        def fresh():
            if tokens is None:
                raise ValueError("an add / assign update needs fresh tokens")
            return int(tokens())
        for r, t, u in self.entries:
            o, x, y, words, took = self._encode(t, u, fresh)
            row.append(r), typ.append(t), op.append(o), a0.append(_u64(x)), a1.append(_u64(y))
            var += [_u64(w) for w in words]
            var_off.append(len(var))
            self.tokens.append(took)
        self.n_var = len(var)
        self.row = np.asarray(row or [0], U64)
        self.type = np.asarray(typ or [0], np.uint8)
        self.op = np.asarray(op or [0], np.uint8)
        self.a0, self.a1 = np.asarray(a0 or [0], U64), np.asarray(a1 or [0], U64)
        self.var_off = np.asarray(var_off, U64)
        self.var_data = np.asarray(var or [0], U64)

    @staticmethod
    def _encode(t: int, u, fresh):
        name = u[0]
        if name == "raw":
            return int(u[1]), u[2], u[3], list(u[4]), []
        if t == abi.AM_PN:
            return {"increment": abi.AM_UP_PN_INCREMENT, "decrement": abi.AM_UP_PN_DECREMENT}[name], u[1], 0, [], []
        if t == abi.AM_LWW:
            if name != "assign":
                raise ValueError(u)
            return abi.AM_UP_LWW_ASSIGN, u[1], u[2], [], []
        if t == abi.AM_AWSET:
            if name == "reset":
                return abi.AM_UP_AW_RESET, 0, 0, [], []
            elems = [u[1]] if name in ("add", "remove") else list(u[1])
            elems = sorted({_u64(e) for e in elems})
            if name in ("add", "add_all"):
                took = [fresh() for _ in elems]
                return abi.AM_UP_AW_ADD, 0, 0, [w for e, k in zip(elems, took) for w in (e, k)], took
            if name in ("remove", "remove_all"):
                return abi.AM_UP_AW_REMOVE, 0, 0, elems, []
            raise ValueError(u)
        if t == abi.AM_MVREG:
            if name == "reset":
                return abi.AM_UP_MV_RESET, 0, 0, [], []
            if name != "assign":
                raise ValueError(u)
            tok = fresh()
            return abi.AM_UP_MV_ASSIGN, u[1], tok, [], [tok]
        if t == abi.AM_BCOUNTER:
            if name == "transfer":
                amount, to, frm = u[1]
                return abi.AM_UP_BC_TRANSFER, amount, int(frm) | (int(to) << 8), [], []
            amount, dc = u[1]
            return {"increment": abi.AM_UP_BC_INCREMENT, "decrement": abi.AM_UP_BC_DECREMENT}[name], amount, dc, [], []
        raise ValueError(t)

    def as_struct(self) -> abi.am_updates:
        s = abi.am_updates()
        s.n_up, s.n_var = self.n_up, self.n_var
        p = lambda a: a.ctypes.data  # noqa: E731
        s.row, s.type, s.op, s.a0, s.a1 = p(self.row), p(self.type), p(self.op), p(self.a0), p(self.a1)
        s.var_off, s.var_data = p(self.var_off), p(self.var_data)
        self._struct = s
        return s


class Effects:
    """am_effects in host memory for n_up updates, and its decoding: effect i in the shape
    encode_effect takes, or ('error', status)."""

    def __init__(self, updates: Updates, var_cap: int):
        n = updates.n_up
        self.updates, self.n_up, self.var_cap = updates, n, int(var_cap)
        self.eff_off = np.zeros(n + 1, U64)
        self.eff_meta = np.zeros(max(n, 1), np.uint8)
        self.p0, self.p1 = np.zeros(max(n, 1), U64), np.zeros(max(n, 1), U64)
        self.var_off = np.zeros(n + 1, U64)
        self.var_data = np.zeros(max(self.var_cap, 1), U64)
        self.n_var = np.zeros(1, U64)
        self.avail = np.zeros(max(n, 1), np.int64)
        self.status = np.full(max(n, 1), 99, np.int32)

    def as_struct(self) -> abi.am_effects:
        s = abi.am_effects()
        s.var_cap = self.var_cap
        p = lambda a: a.ctypes.data  # noqa: E731
        s.eff_off, s.eff_meta, s.p0, s.p1 = p(self.eff_off), p(self.eff_meta), p(self.p0), p(self.p1)
        s.var_off, s.var_data, s.n_var, s.avail = p(self.var_off), p(self.var_data), p(self.n_var), p(self.avail)
        self._struct = s
        return s

    def words(self, i: int) -> List[int]:
        return [int(w) for w in self.var_data[int(self.var_off[i]):int(self.var_off[i + 1])]]

    def effect(self, i: int):
        st = int(self.status[i])
        if st != 0:
            return ("error", st)
        return decode_effect(self.updates.entries[i][1], int(self.eff_meta[i]), int(self.p0[i]), int(self.p1[i]),
                             self.words(i))

    def effects(self) -> list:
        return [self.effect(i) for i in range(self.n_up)]

    def as_writeset(self) -> WriteSet:
        """The updates' rows and types with these columns as the write set they are (n_ws = n_eff
        = n_up); a failed update's effect carries AM_META_BAD."""
        n = self.n_up
        ents = [(r, t, ["bad" if self.status[i] != 0 else self.effect(i)])
                for i, (r, t, _) in enumerate(self.updates.entries)]
        nv = int(self.var_off[n])
        return WriteSet.from_columns(self.updates.row[:n], self.updates.type[:n], self.eff_off, self.eff_meta[:n],
                                     self.p0[:n], self.p1[:n], self.var_off, self.var_data[:nv], ents)


class Commits:
    """am_commits in host memory: a batch of committed transactions, in the order the vnode commits
    them, as clocksi_vnode:commit/5 -> update_materializer/3 (src/clocksi_vnode.erl:499-531,
    634-657) and inter_dc_dep_vnode (src/inter_dc_dep_vnode.erl:150-152) hand them to the
    materializer.

    transactions: [(dc, commit_time, snap, txid, [(key, type, effect), ...])] -- the commit DC index
    (the own DC, or a remote transaction's origin), TxCommitTime, vec_snapshot_time as {dc: time},
    the am_txid id or None, and the effects oldest first, shaped as encode_effect takes them (the
    string "bad": one Type:update/2 raises on).  snap_pres is kept only when some snapshot lacks a
    DC, txid only when some transaction has one (0 for the others) -- among the transactions that
    have effects, so the columns are those of a HostLog of the same ops."""

    def __init__(self, n_dc: int, transactions: Sequence[Tuple[int, int, Dict[int, int], Optional[int], Sequence[Any]]]):
        txs = [(int(d), int(ct), dict(sn), tx, list(effs)) for d, ct, sn, tx, effs in transactions]
        key, typ, meta, p0, p1, var, var_off = [], [], [], [], [], [], [0]
        for _, _, _, _, effs in txs:
            for k, t, eff in effs:
                bad = isinstance(eff, str) and eff == "bad"
                kind, a, b, words = (0, 0, 0, []) if bad else encode_effect(t, eff)
                key.append(int(k)), typ.append(int(t)), meta.append(abi.make_meta(0, kind, bad))
                p0.append(_u64(a)), p1.append(_u64(b))
                var += [_u64(w) for w in words]
                var_off.append(len(var))
        self._init_columns(n_dc, [(d, ct, sn, tx, len(effs)) for d, ct, sn, tx, effs in txs], key, typ, meta, p0, p1,
                           var_off, var)

    @classmethod
    def from_columns(cls, n_dc: int, transactions, key, type_, eff_meta, p0, p1, var_off, var_data) -> "Commits":
        """A batch over effect columns already in the ABI's encoding (what am_generate_downstream /
        am_update_objects_* wrote, unchanged).  transactions: [(dc, commit_time, snap, txid,
        n_effects)], their effects consecutive in the columns."""
        c = cls.__new__(cls)
        c._init_columns(n_dc, [(int(d), int(ct), dict(sn), tx, int(ne)) for d, ct, sn, tx, ne in transactions],
                        key, type_, eff_meta, p0, p1, var_off, var_data)
        return c

    def _init_columns(self, n_dc, txs, key, typ, meta, p0, p1, var_off, var):
        if not 1 <= n_dc <= abi.AM_MAX_DC:
            raise ValueError("n_dc out of range")
        nt = len(txs)
        self.n_dc, self.n_tx = n_dc, nt
        self.dc = np.asarray([d for d, _, _, _, _ in txs] or [0], np.uint8)
        self.commit_time = np.asarray([ct for _, ct, _, _, _ in txs] or [0], U64)
        self.snap_vc = np.zeros((max(nt, 1), n_dc), U64)
        self.snap_pres = np.zeros(max(nt, 1), np.uint32)
        for i, (_, _, sn, _, _) in enumerate(txs):
            for d, t in sn.items():
                self.snap_vc[i, d] = t
            self.snap_pres[i] = _pres(sn)
        # (a transaction without effects leaves no op: it decides neither column)
        self.has_pres = any(ne and int(p) != (1 << n_dc) - 1 for p, (_, _, _, _, ne) in zip(self.snap_pres, txs))
        self.has_txid = any(ne and tx is not None for _, _, _, tx, ne in txs)
        self.txid = np.asarray([0 if tx is None else int(tx) for _, _, _, tx, _ in txs] or [0], U64)
        self.eff_off = np.zeros(nt + 1, U64)
        self.eff_off[1:] = np.cumsum([ne for _, _, _, _, ne in txs], dtype=U64) if nt else []
        n = int(self.eff_off[-1])
        self.n_eff = n
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        self.key, self.type, self.eff_meta = c(key, U64), c(typ, np.uint8), c(meta, np.uint8)
        self.p0, self.p1 = c(p0, U64), c(p1, U64)
        self.var_off = np.ascontiguousarray(var_off, U64)
        self.n_var = int(self.var_off[n]) if len(self.var_off) > n else 0
        self.var_data = c(var, U64)
        self.has_var = True  # as_struct(var=False) drops the columns (no effect has variable words)
        if len(self.key) < n or len(self.var_off) != n + 1:
            raise ValueError("effect columns shorter than the transactions' effect counts")

    def as_struct(self) -> abi.am_commits:
        s = abi.am_commits()
        s.n_tx, s.n_eff, s.n_var = self.n_tx, self.n_eff, self.n_var if self.has_var else 0
        p = lambda a: a.ctypes.data  # noqa: E731
        s.dc, s.commit_time, s.snap_vc = p(self.dc), p(self.commit_time), p(self.snap_vc)
        s.snap_pres = p(self.snap_pres) if self.has_pres else None
        s.txid = p(self.txid) if self.has_txid else None
        s.eff_off, s.key, s.type, s.eff_meta = p(self.eff_off), p(self.key), p(self.type), p(self.eff_meta)
        s.p0, s.p1 = p(self.p0), p(self.p1)
        s.var_off = p(self.var_off) if self.has_var else None
        s.var_data = p(self.var_data) if self.has_var else None
        self._struct = s
        return s

    def effect(self, q: int) -> Tuple[int, int, int, List[int]]:
        """Batch effect q decoded from the columns: (meta, p0, p1, var words)."""
        return (int(self.eff_meta[q]), int(self.p0[q]), int(self.p1[q]),
                [int(w) for w in self.var_data[int(self.var_off[q]):int(self.var_off[q + 1])]])

    def ops_by_key(self) -> Dict[int, List[Op]]:
        """The batch as the ops update_materializer/3 inserts, per key in commit order (decoded from
        the columns): what Vnode.insert / HostLog take for the same batch."""
        out: Dict[int, List[Op]] = {}
        for t in range(self.n_tx):
            snap = {d: int(self.snap_vc[t, d]) for d in range(self.n_dc) if (int(self.snap_pres[t]) >> d) & 1}
            for q in range(int(self.eff_off[t]), int(self.eff_off[t + 1])):
                meta, a, b, words = self.effect(q)
                bad = bool(meta & abi.AM_META_BAD)
                ty = int(self.type[q])
                out.setdefault(int(self.key[q]), []).append(
                    Op(ty, int(self.dc[t]), int(self.commit_time[t]), snap,
                       None if bad else decode_effect(ty, meta, a, b, words),
                       int(self.txid[t]) if self.has_txid else None, bad=bad))
        return out

    def reference_log(self) -> Dict[str, Any]:
        """A numpy restatement of am_commit_build's output: keys (distinct, ascending), the CSR
        columns over them and src.  A key's ops are ordered by (transaction, effect in the
        transaction) -- a stable sort by key; op_meta = the transaction's dc | the effect's kind and
        AM_META_BAD bits; key_type = the type of the key's first op; key_flags =
        AM_KEY_MIXED_TYPES when the key's ops disagree."""
        n, nt, nd = self.n_eff, self.n_tx, self.n_dc
        tx_of = np.repeat(np.arange(nt, dtype=np.int64), np.diff(self.eff_off.astype(np.int64))) if nt else \
            np.zeros(0, np.int64)
        key = self.key[:n]
        order = np.argsort(key, kind="stable")
        ks = key[order]
        head = np.ones(n, bool)
        head[1:] = ks[1:] != ks[:-1]
        kidx = np.cumsum(head) - 1
        types = self.type[:n][order]
        key_type = types[head]
        key_flags = np.zeros(int(head.sum()), np.uint8)
        key_flags[kidx[types != key_type[kidx]]] = abi.AM_KEY_MIXED_TYPES
        tx = tx_of[order]
        vo = self.var_off.astype(np.int64) if self.has_var else np.zeros(n + 1, np.int64)
        lens = (vo[1:] - vo[:-1])[order]
        out_vo = np.zeros(n + 1, U64)
        out_vo[1:] = np.cumsum(lens, dtype=U64)
        words = [self.var_data[vo[s]:vo[s + 1]] for s in order]
        return {
            "keys": ks[head].astype(U64),
            "key_off": np.concatenate([np.flatnonzero(head), [n]]).astype(U64),
            "key_type": key_type.astype(np.uint8), "key_flags": key_flags,
            "op_meta": ((self.dc[:nt][tx] & 0x1F) | (self.eff_meta[:n][order] & 0xE0)).astype(np.uint8),
            "commit_time": self.commit_time[:nt][tx].astype(U64),
            "snap_vc": np.ascontiguousarray(self.snap_vc[:nt][tx].T.reshape(nd, n), U64),
            "snap_pres": self.snap_pres[:nt][tx].astype(np.uint32) if self.has_pres else None,
            "op_txid": self.txid[:nt][tx].astype(U64) if self.has_txid else None,
            "p0": self.p0[:n][order].astype(U64), "p1": self.p1[:n][order].astype(U64),
            "var_off": out_vo,
            "var_data": np.concatenate(words + [np.zeros(0, U64)]).astype(U64),
            "src": order.astype(np.uint32),
        }


def _pair_columns(write_sets):
    """key_off [n_tx+1] and key [n_pairs] of a batch's write sets, in batch order."""
    key_off = np.zeros(len(write_sets) + 1, U64)
    if write_sets:
        key_off[1:] = np.cumsum([len(w) for w in write_sets], dtype=U64)
    keys = [_u64(k) for w in write_sets for k in w]
    return key_off, np.asarray(keys or [0], U64), len(keys)


class Prepares:
    """am_prepares in host memory: a batch of clocksi_vnode:prepare/6 requests in the order the vnode
    serves them.  txs: [(txid, start_time, prepare_time, certify, [key, ...])], the tuples
    CertSim.prepare takes; keys, TxIds and times are any u64.  A write set keeps its repeats (the
    certifier enters a key once)."""

    def __init__(self, txs: Sequence[Tuple[int, int, int, bool, Sequence[int]]]):
        txs = [(int(x), int(s), int(p), bool(c), [int(k) for k in ks]) for x, s, p, c, ks in txs]
        self.n_tx = len(txs)
        col = lambda i, dt: np.asarray([t[i] for t in txs] or [0], dt)  # noqa: E731
        self.txid, self.start_time, self.prepare_time = col(0, U64), col(1, U64), col(2, U64)
        self.certify = col(3, np.uint8)
        self.key_off, self.key, self.n_pairs = _pair_columns([t[4] for t in txs])

    @classmethod
    def from_columns(cls, txid, start_time, prepare_time, certify, key_off, key) -> "Prepares":
        """A batch over columns already in the ABI's layout (key_off [n_tx+1], key [n_pairs])."""
        b = cls.__new__(cls)
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        b.n_tx = len(txid)
        b.txid, b.start_time, b.prepare_time, b.certify = c(txid, U64), c(start_time, U64), c(prepare_time, U64), c(certify, np.uint8)
        b.key_off = np.ascontiguousarray(key_off, U64)
        b.n_pairs = len(key)
        b.key = c(key, U64)
        if len(b.key_off) != b.n_tx + 1:
            raise ValueError("key_off must hold n_tx + 1 offsets")
        return b

    def transactions(self):
        """The batch back as CertSim.prepare's tuples."""
        o = self.key_off
        return [(int(self.txid[t]), int(self.start_time[t]), int(self.prepare_time[t]), bool(self.certify[t]),
                 [int(k) for k in self.key[int(o[t]):int(o[t + 1])]]) for t in range(self.n_tx)]

    def as_struct(self) -> abi.am_prepares:
        s = abi.am_prepares()
        s.n_tx, s.n_pairs = self.n_tx, self.n_pairs
        p = lambda a: a.ctypes.data  # noqa: E731
        s.txid, s.start_time, s.prepare_time, s.certify = p(self.txid), p(self.start_time), p(self.prepare_time), p(self.certify)
        s.key_off, s.key = p(self.key_off), p(self.key)
        return s


class DepTxns:
    """am_dep_txns in host memory: a batch of arrivals at the dependency buffer, in the order
    inter_dc_dep_vnode:handle_transaction/1 receives them.  txs: [(part, dc, timestamp, snapshot, ping,
    tag)], snapshot a dict DC -> time (a DC it lacks goes in as 0); times and tags are any u64."""

    def __init__(self, n_dc: int, txs: Sequence[Tuple[int, int, int, Dict[int, int], bool, int]]):
        self.n_dc, self.n_tx = n_dc, len(txs)
        col = lambda i, dt: np.asarray([int(t[i]) for t in txs] or [0], dt)  # noqa: E731
        self.part, self.dc, self.timestamp = col(0, np.uint32), col(1, np.uint8), col(2, U64)
        self.ping, self.tag = col(4, np.uint8), col(5, U64)
        self.snap_vc = np.zeros((max(self.n_tx, 1), n_dc), U64)
        for i, t in enumerate(txs):
            for d, v in t[3].items():
                self.snap_vc[i, d] = v

    @classmethod
    def from_columns(cls, n_dc: int, part, dc, timestamp, snap_vc, ping, tag) -> "DepTxns":
        """A batch over columns already in the ABI's layout (snap_vc [n_tx][n_dc])."""
        b = cls.__new__(cls)
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        b.n_dc, b.n_tx = n_dc, len(part)
        b.part, b.dc, b.timestamp, b.ping, b.tag = c(part, np.uint32), c(dc, np.uint8), c(timestamp, U64), c(ping, np.uint8), c(tag, U64)
        b.snap_vc = np.ascontiguousarray(snap_vc, U64).reshape(-1, n_dc) if b.n_tx else np.zeros((1, n_dc), U64)
        if b.n_tx and b.snap_vc.shape[0] != b.n_tx:
            raise ValueError("snap_vc must hold n_tx rows of n_dc entries")
        return b

    def transactions(self):
        """The batch back as its tuples (a snapshot entry of 0 reads as absent)."""
        return [(int(self.part[t]), int(self.dc[t]), int(self.timestamp[t]),
                 {d: int(v) for d, v in enumerate(self.snap_vc[t]) if v}, bool(self.ping[t]), int(self.tag[t]))
                for t in range(self.n_tx)]

    def as_struct(self) -> abi.am_dep_txns:
        s = abi.am_dep_txns()
        s.n_tx = self.n_tx
        p = lambda a: a.ctypes.data  # noqa: E731
        s.part, s.dc, s.timestamp, s.snap_vc, s.ping, s.tag = (p(self.part), p(self.dc), p(self.timestamp), p(self.snap_vc),
                                                               p(self.ping), p(self.tag))
        return s


class SubRows:
    """am_sub_rows in host memory: a batch of rows at the subscriber buffer, in arrival order.  rows:
    [(kind, part, dc, prev_opid, last_opid, timestamp, snapshot, ping, tag)], kind one of abi.AM_SUB_*,
    snapshot a dict DC -> time (a DC it lacks goes in as 0); op ids, times and tags are any u64."""

    def __init__(self, n_dc: int, rows: Sequence[Tuple[int, int, int, int, int, int, Dict[int, int], bool, int]]):
        self.n_dc, self.n_rows = n_dc, len(rows)
        col = lambda i, dt: np.asarray([int(t[i]) for t in rows] or [0], dt)  # noqa: E731
        self.kind, self.part, self.dc = col(0, np.uint8), col(1, np.uint32), col(2, np.uint8)
        self.prev_opid, self.last_opid, self.timestamp = col(3, U64), col(4, U64), col(5, U64)
        self.ping, self.tag = col(7, np.uint8), col(8, U64)
        self.snap_vc = np.zeros((max(self.n_rows, 1), n_dc), U64)
        for i, t in enumerate(rows):
            for d, v in t[6].items():
                self.snap_vc[i, d] = v

    @classmethod
    def from_columns(cls, n_dc: int, kind, part, dc, prev_opid, last_opid, timestamp, snap_vc, ping, tag) -> "SubRows":
        """A batch over columns already in the ABI's layout (snap_vc [n_rows][n_dc])."""
        b = cls.__new__(cls)
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        b.n_dc, b.n_rows = n_dc, len(kind)
        b.kind, b.part, b.dc = c(kind, np.uint8), c(part, np.uint32), c(dc, np.uint8)
        b.prev_opid, b.last_opid, b.timestamp = c(prev_opid, U64), c(last_opid, U64), c(timestamp, U64)
        b.ping, b.tag = c(ping, np.uint8), c(tag, U64)
        b.snap_vc = np.ascontiguousarray(snap_vc, U64).reshape(-1, n_dc) if b.n_rows else np.zeros((1, n_dc), U64)
        if b.n_rows and b.snap_vc.shape[0] != b.n_rows:
            raise ValueError("snap_vc must hold n_rows rows of n_dc entries")
        return b

    def rows(self):
        """The batch back as its tuples (a snapshot entry of 0 reads as absent)."""
        return [(int(self.kind[t]), int(self.part[t]), int(self.dc[t]), int(self.prev_opid[t]), int(self.last_opid[t]),
                 int(self.timestamp[t]), {d: int(v) for d, v in enumerate(self.snap_vc[t]) if v}, bool(self.ping[t]),
                 int(self.tag[t])) for t in range(self.n_rows)]

    def as_struct(self) -> abi.am_sub_rows:
        s = abi.am_sub_rows()
        s.n_rows = self.n_rows
        p = lambda a: a.ctypes.data  # noqa: E731
        s.kind, s.part, s.dc, s.prev_opid, s.last_opid = p(self.kind), p(self.part), p(self.dc), p(self.prev_opid), p(self.last_opid)
        s.timestamp, s.snap_vc, s.ping, s.tag = p(self.timestamp), p(self.snap_vc), p(self.ping), p(self.tag)
        return s


class Finishes:
    """am_finishes in host memory: a batch of commit/5 and abort/2 clean-ups (clean_and_notify/3).
    txs: [(txid, commit_time, committed, [key, ...])], the tuples CertSim.finish takes."""

    def __init__(self, txs: Sequence[Tuple[int, int, bool, Sequence[int]]]):
        txs = [(int(x), int(ct), bool(c), [int(k) for k in ks]) for x, ct, c, ks in txs]
        self.n_tx = len(txs)
        col = lambda i, dt: np.asarray([t[i] for t in txs] or [0], dt)  # noqa: E731
        self.txid, self.commit_time, self.committed = col(0, U64), col(1, U64), col(2, np.uint8)
        self.key_off, self.key, self.n_pairs = _pair_columns([t[3] for t in txs])

    @classmethod
    def from_columns(cls, txid, commit_time, committed, key_off, key) -> "Finishes":
        """A batch over columns already in the ABI's layout (key_off [n_tx+1], key [n_pairs])."""
        b = cls.__new__(cls)
        c = lambda a, dt: np.ascontiguousarray(a if len(a) else [0], dt)  # noqa: E731
        b.n_tx = len(txid)
        b.txid, b.commit_time, b.committed = c(txid, U64), c(commit_time, U64), c(committed, np.uint8)
        b.key_off = np.ascontiguousarray(key_off, U64)
        b.n_pairs = len(key)
        b.key = c(key, U64)
        if len(b.key_off) != b.n_tx + 1:
            raise ValueError("key_off must hold n_tx + 1 offsets")
        return b

    def transactions(self):
        """The batch back as CertSim.finish's tuples."""
        o = self.key_off
        return [(int(self.txid[t]), int(self.commit_time[t]), bool(self.committed[t]),
                 [int(k) for k in self.key[int(o[t]):int(o[t + 1])]]) for t in range(self.n_tx)]

    def as_struct(self) -> abi.am_finishes:
        s = abi.am_finishes()
        s.n_tx, s.n_pairs = self.n_tx, self.n_pairs
        p = lambda a: a.ctypes.data  # noqa: E731
        s.txid, s.commit_time, s.committed = p(self.txid), p(self.commit_time), p(self.committed)
        s.key_off, s.key = p(self.key_off), p(self.key)
        return s
