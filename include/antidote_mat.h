/*
 * antidote_mat.h -- C ABI of the MI355X batched CRDT snapshot materializer.
 *
 * Drop-in boundary for the AntidoteDB Cure/ClockSI snapshot-read hot path.
 * Every entry point names the reference interface it replaces (paths are
 * relative to the reference tree, SmallEndian/antidote):
 *
 *   am_materialize          clocksi_materializer:materialize/4
 *                           (src/clocksi_materializer.erl:82-101), batched over keys;
 *                           called from materializer_vnode:materialize_snapshot/7
 *                           (src/materializer_vnode.erl:469-509, call at :478)
 *   am_store_create         the per-partition ETS ops cache laid out in HBM
 *                           (materializer_vnode:op_insert_gc/3 appends,
 *                           src/materializer_vnode.erl:622-647; tuple layout
 *                           include/antidote.hrl:81-90)
 *   am_gst_local_min        stable_time_functions:get_min_time/1 over the local
 *                           partitions (src/stable_time_functions.erl:51-85)
 *   am_gst_allreduce        the node-to-node broadcast + merge of meta_data_sender
 *                           (src/meta_data_sender.erl:232-255) as one RCCL min
 *                           all-reduce over xGMI
 *   am_gst_finalize         meta_data_sender:update_stable/3 with
 *                           stable_time_functions:update_func_min/2
 *                           (src/meta_data_sender.erl:342-356,
 *                           src/stable_time_functions.erl:42-48) and the gr-mode
 *                           broadcast of dc_utilities:get_stable_snapshot/0
 *                           (src/dc_utilities.erl:246-279)
 *   am_snapcache_read       materializer_vnode:internal_read/7 with the snapshot cache
 *                           in HBM: get_from_snapshot_cache/5, vector_orddict:
 *                           get_smaller/2 + insert_bigger/3, materialize_snapshot/7,
 *                           internal_store_ss/4 (src/materializer_vnode.erl:342-509,
 *                           src/vector_orddict.erl:75-140)
 *   am_store_update         op-cache ingestion + GC: materializer_vnode:op_insert_gc/3
 *                           appends (src/materializer_vnode.erl:622-647) and prune_ops/2
 *                           + check_filter/7 (:565-604) as one batched log rebuild
 *   am_snapcache_gc_threshold  the prune threshold of snapshot_insert_gc/4 (:515-535):
 *                           vectorclock:min over the first SNAPSHOT_MIN cached snapshots
 *   am_vnode_insert_host    one partition's materializer_vnode state: op_insert_gc/3 with
 *   am_vnode_read_host      its write-triggered GC read (src/materializer_vnode.erl:622-647),
 *                           internal_read/7 with ShouldGC (:371-376), load_ops/2 (:312-319)
 *   am_vnode_commit_host    clocksi_vnode:commit/5 -> update_materializer/3 (src/clocksi_vnode.erl:
 *   am_commit_build         499-531, 634-657): a batch of committed transactions' effects, the op log
 *                           over the touched keys built on the device
 *   am_plog_read            materializer_vnode:get_from_snapshot_log/3 -> logging_vnode:
 *   am_vnode_create_logged  get_up_to_time/5 (src/materializer_vnode.erl:415-419, src/logging_vnode.erl:
 *                           522-545, 676-779): the partition's log in HBM, the read no cached
 *                           snapshot serves rebuilt from it
 *   am_read_objects_submit  clocksi_interactive_coord's read_objects fan-out over a GPU's
 *                           partitions (src/clocksi_interactive_coord.erl:732-747,
 *                           src/clocksi_readitem_server.erl:217-228) as one async batch
 *   am_materialize_eager    clocksi_materializer:materialize_eager/3 (src/clocksi_materializer.erl:
 *                           272-274, src/materializer.erl:62-70), batched: a snapshot plus the
 *                           reading transaction's own effects, as clocksi_vnode:read_data_item/5
 *                           (src/clocksi_vnode.erl:99-107) and clocksi_downstream:
 *                           generate_downstream_op/6 (src/clocksi_downstream.erl:41-68) call it
 *   am_read_objects_ws_*    the read_objects fan-out with apply_tx_updates_to_snapshot/4
 *                           (src/clocksi_interactive_coord.erl:486-507, 883-894) on the device
 *   am_generate_downstream  clocksi_downstream:generate_downstream_op/6 (src/clocksi_downstream.erl:
 *   am_update_objects_*     41-68), batched: Type:downstream/2 on the state read, on the device
 *   am_key_partition        log_utilities:get_key_partition/1 + convert_key/1: integer
 *   am_key_partition_bytes  keys, binaries (list_to_integer text or SHA-1 chash_key) and
 *                           other terms (src/log_utilities.erl:60-79,100-118)
 *   am_codec_*              Erlang terms of CRDT states <-> order-preserving u64 labels
 *                           (the NIF's term conversion)
 *
 * Conventions
 *   - Plain C, POD structure-of-arrays, no framework types.  Status codes
 *     mirror the reference's error conventions: {error, {unexpected_operation,
 *     Effect, Type}} (src/materializer.erl:52-58) and
 *     erlang:error(corrupted_ops_cache) (src/clocksi_materializer.erl:190-191).
 *   - A vectorclock (a dict DcId -> time in the reference, hex vectorclock 0.1.0)
 *     is a dense array of n_dc u64 lanes plus a presence bitmask (bit d set =
 *     DC d is a key of the dict).  DC ids are mapped by the caller to indices
 *     0..n_dc-1 in ascending Erlang term order (so sorted [{Dc, T}] renderings
 *     match).  n_dc <= AM_MAX_DC.
 *   - "ignore" (an atom in the reference) is an explicit flag.
 *   - Device entry points take DEVICE pointers and run on the context's HIP
 *     stream, asynchronously but for the data-dependent counter readbacks each
 *     one documents (am_materialize: at most two); the *_host variants take host
 *     memory and block.
 */
#ifndef ANTIDOTE_MAT_H
#define ANTIDOTE_MAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AM_ABI_VERSION 15
#define AM_MAX_DC 32

/* CRDT types (the reference's type atoms) */
enum am_type {
  AM_PN = 1,        /* antidote_crdt_counter_pn   */
  AM_LWW = 2,       /* antidote_crdt_register_lww */
  AM_AWSET = 3,     /* antidote_crdt_set_aw       */
  AM_MVREG = 4,     /* antidote_crdt_register_mv  */
  AM_BCOUNTER = 5   /* antidote_crdt_counter_b    */
};

/* Per-read status.  >0: the reference's {error, _} / exception outcomes. <0: API errors. */
enum am_status {
  AM_OK = 0,
  AM_ERR_CORRUPTED_OPS_CACHE = 1,   /* erlang:error(corrupted_ops_cache)            */
  AM_ERR_UNEXPECTED_OPERATION = 2,  /* {error, {unexpected_operation, Effect, Type}}*/
  AM_ERR_OVERFLOW = 3,              /* result outside int64 (Erlang would bignum)   */
  AM_ERR_CAPACITY = 4,              /* set result larger than the caller's capacity */
  AM_ERR_COLD_PATH = 5,             /* no cached snapshot at or below the read clock:
                                       get_from_snapshot_log (the log, not the cache); a vnode
                                       with a log (am_vnode_create_logged) serves the read */
  AM_ERR_NO_PERMISSIONS = 6,        /* {error, no_permissions} (am_generate_downstream)     */
  AM_ERR_WRITE_CONFLICT = 7,        /* {error, write_conflict} (am_cert_prepare)             */
  AM_ERR_NO_UPDATES = 8,            /* {error, no_updates} (am_cert_prepare / am_cert_finish) */
  AM_ERR_INVALID = -1,
  AM_ERR_HIP = -2,
  AM_ERR_RCCL = -3,
  AM_ERR_NOMEM = -4,
  AM_ERR_UNSUPPORTED = -5
};

/* per-read informational flags */
#define AM_FLAG_MISSING_DC_LOGGED 0x1u  /* logger:error("Could not find DC in SS"), src/clocksi_materializer.erl:246 */

/* op_meta byte: commit DC index, effect sub-kind, invalid-effect marker */
#define AM_META_DC(m) ((unsigned)(m)&0x1Fu)
#define AM_META_KIND(m) (((unsigned)(m) >> 5) & 0x3u)
#define AM_META_BAD 0x80u /* Type:update/2 raises on this effect */
#define AM_MAKE_META(dc, kind, bad) ((uint8_t)(((dc)&0x1F) | (((kind)&3) << 5) | ((bad) ? 0x80 : 0)))

/* effect sub-kinds */
#define AM_MV_ASSIGN 0 /* {Value, Token, Overridden}  */
#define AM_MV_RESET 1  /* {reset, Overridden}         */
#define AM_BC_INCREMENT 0 /* {{increment, V}, Id}      -> P[{Id,Id}] += V   */
#define AM_BC_DECREMENT 1 /* {{decrement, V}, Id}      -> D[Id] += V        */
#define AM_BC_TRANSFER 2  /* {{transfer, V, To}, From} -> P[{From,To}] += V */

/* key_flags */
#define AM_KEY_MIXED_TYPES 0x1u /* the key's log holds ops of more than one type */

/*
 * The per-partition ops cache as structure-of-arrays (one "log" = one
 * materializer_vnode ops_cache table).  Ops of key k occupy
 * [key_off[k], key_off[k+1]) oldest -> newest, exactly the ETS tuple order
 * (slot FIRST_OP .. FIRST_OP+Length-1).  Payload encoding per type:
 *   PN        p0 = int64 delta
 *   LWW       p0 = timestamp, p1 = value (u64)
 *   MVREG     p0 = value, p1 = token, var = overridden tokens (kind ASSIGN|RESET)
 *   AWSET     var = entries [elem, n_add, n_rm, add_tok..., rm_tok...]...,
 *             entries sorted by elem, elems unique within one effect
 *   BCOUNTER  p0 = int64 amount, p1 = from | (to << 8), kind in op_meta
 */
typedef struct am_op_log {
  uint32_t n_dc;
  uint32_t _pad;
  uint64_t n_keys;
  uint64_t n_ops;
  uint64_t n_var;
  uint64_t snap_stride;        /* elements between the DC columns of snap_vc; 0 => n_ops */
  const uint64_t *key_off;     /* [n_keys+1]                                        */
  const uint64_t *key_id_base; /* [n_keys] op id of the key's oldest op; NULL => 1   */
  const uint8_t *key_type;     /* [n_keys] am_type                                   */
  const uint8_t *key_flags;    /* [n_keys] or NULL                                   */
  const uint8_t *op_meta;      /* [n_ops]                                            */
  const uint64_t *commit_time; /* [n_ops] commit_time = {DcId, CT}: the CT           */
  const uint64_t *snap_vc;     /* [n_dc][snap_stride] snapshot_time, DC-major        */
  const uint32_t *snap_pres;   /* [n_ops] presence of snapshot_time keys; NULL=all   */
  const uint64_t *op_txid;     /* [n_ops] or NULL (never equal to a read's TxId)     */
  const uint64_t *op_id;       /* [n_ops] or NULL (dense ids from key_id_base)       */
  const uint64_t *p0;          /* [n_ops]                                            */
  const uint64_t *p1;          /* [n_ops]                                            */
  const uint64_t *var_off;     /* [n_ops+1] or NULL                                  */
  const uint64_t *var_data;    /* [n_var]                                            */
  /* Packed streaming view (logs without snap_pres), built on the device by am_store_create /
   * am_store_update / am_synth_store (NULL in host logs).  The op's commit vector
   * X = snapshot_time with X[dc] = commit_time (the clock is_op_in_snapshot/7 compares) is
   * stored relative to a per-key time base:
   *   pk_vc[d][p] = X[d] - key_tbase[k]   as u32 in [0, 2^32 - 2]
   * key_tbase[k] = (the smallest entry of the key's first op that lies within 2^31 of its
   * commit time) - 2^30, saturating at 0.  An op with an entry outside the window, or
   * carrying AM_META_BAD, has pk_vc[0][p] = AM_PK_ESC and is read from the full columns
   * above.  The inclusion test then runs on u32 (one compare and one max per DC) and
   * streams 4 * n_dc bytes per op: 32 B at D = 8 instead of 72 B. */
  const uint64_t *key_tbase;   /* [n_keys]                                           */
  const uint32_t *pk_vc;       /* [n_dc][snap_stride]                                */
  /* Token-group view (add-wins set and MV register keys), built on the device with the
   * packed view (am_store_create / am_store_update / am_synth_store).  Every effect is
   * flattened to births and kills of tokens:
   *   AW  add token t of elem e -> birth of (e, t);  remove token t of elem e -> kill of (e, t)
   *   MV  {Value, Token, _}      -> birth of (Value, Token); overridden token t -> kill of t
   * A key's distinct kill keys (AW (elem, token), MV token) are its GROUPS, numbered in the
   * reference's output order: AW by elem, then newest birth first (ToAdd ++ Current), MV by
   * (Value, Token) (insert_sorted); groups without a birth last.  One u32 record per
   * birth / EFFECTIVE kill (one that follows its group's birth: a kill in the birth's own op
   * or earlier never removes the token; every kill of a group with no birth in the log, whose
   * token only a cached base can hold), a key's records contiguous and in op order,
   * [rec_key_off[k], rec_key_off[k+1]):
   *   rec_g = op index within the key (bits 0-15) | kill << 16 | group << 17, or 0xFFFFFFFF
   *           for a kill slot that is not effective
   * and group g of key k is the pair grp[2 (rec_key_off[k] + g) + {0, 1}] (AW (elem, token), MV
   * (Value, Token); MV groups without a birth (~0, token)).  key_ngrp[k] = number of groups,
   * or AM_NGRP_NONE when the key is materialized from var_data instead (more than
   * AM_GRP_MAX_REC records or 2^16 ops, or a log outside the closed form: a token born
   * twice).  A materialization then streams the ops (inclusion), the records (born / killed
   * bits per group) and only the surviving groups' pairs, with no sort.  Ops carrying
   * AM_META_BAD produce no record; an op whose variable payload is malformed (Type:update/2
   * would raise) gets AM_META_BAD set in op_meta and is escaped in the packed view. */
  uint64_t n_rec;
  const uint64_t *rec_key_off; /* [n_keys+1]                                         */
  const uint32_t *rec_g;       /* [n_rec]                                            */
  const uint64_t *grp;         /* [n_rec][2], 16-byte aligned: one load per survivor */
  const uint32_t *key_ngrp;    /* [n_keys]                                           */
  /* Room for appends (the ETS tuple's ListLen slack, src/materializer_vnode.erl:540-560; vnode
   * stores only, NULL elsewhere).  With key_end set, key k's ops are [key_off[k], key_end[k])
   * and [key_end[k], key_off[k+1]) is free room that am_store_apply fills in place (always at
   * least one free slot: var_off[key_end[k]] ends the key's last op's words); with rec_key_end
   * set, its records are [rec_key_off[k], rec_key_end[k]) with room up to rec_key_off[k+1]
   * (group g still at grp[2 (rec_key_off[k] + g)]).  Every reader takes a key's end from
   * key_end when present, else key_off[k+1]. */
  const uint64_t *key_end;     /* [n_keys] or NULL                                   */
  const uint64_t *rec_key_end; /* [n_keys] or NULL                                   */
  /* Group-mask view (built with the token-group view): for the ops of a grouped key with at
   * most 32 groups, gmask[p] = the groups op p births (bits 0-31) | the groups it EFFECTIVELY
   * kills (bits 32-63) -- the key's records folded per op, so a short read ORs one word per
   * included op instead of testing records; 0 for every other op.  NULL in host logs. */
  const uint64_t *gmask;       /* [n_ops] or NULL                                    */
  /* Zone map (device stores, NULL in host logs): per block z of AM_ZONE_OPS consecutive op
   * slots [z * AM_ZONE_OPS, (z + 1) * AM_ZONE_OPS) of the columns, zone_vc[d * n_zones + z] >=
   * X[d] of every op in the block (X = the commit vector is_op_in_snapshot/7 compares;
   * n_zones = ceil(snap_stride or n_ops / AM_ZONE_OPS)).  An upper bound, kept by every writer
   * (a GC may leave it above the surviving ops).  A read with a base snapshot skips a block
   * whose bound is vectorclock:le the base clock: none of its ops is a candidate
   * (belongs_to_snapshot_op/3), so none counts, none is applied and none bounds NewLastOp --
   * the ops already folded into the cached snapshot are not streamed again.
   * Row n_dc, zone_vc[n_dc * n_zones + z] = 1 marks an EXACT block: all its slots are used ops
   * of one key, none escaped from the packed view or invalid, and the bound is their maximum.
   * A read whose clock covers an exact block's bound includes every op of it: its inclusion
   * bits, count and LastOpCt maxima come from the mark and the bound, without the ops' commit
   * vectors.
   * Rows n_dc + 1 .. n_dc + 3 (zone_gsum non-NULL): an exact block of a grouped add-wins-set /
   * MV-register key with at most AM_GRP_MAX_REC groups has its group summary at word
   * zone_vc[(n_dc + 1) * n_zones + z] of zone_gsum (else ~0 -- rows n_dc + 2 and n_dc + 3 are
   * then meaningless), its records end (exclusive, a rec_g index) at row n_dc + 2 and its records
   * begin at row n_dc + 3.  Row n_dc + 4 is the block's summary slot, (capacity in words << 48) |
   * word offset, or 0: a block inside a grouped key's op range (room included) owns one, so
   * am_store_apply can rewrite the summary in place when the block becomes exact again.
   * Maintenance: am_store_apply recomputes, for every block inside a key it writes (room
   * included), the exact maxima over the used slots, the mark, and the summary when the key's
   * new group count fits the slot (else row n_dc + 1 = ~0); a block shared with another key only
   * has its bound raised.  am_store_index drops or (re)builds the whole index. */
  const uint64_t *zone_vc;
  /* Zone group summaries (device stores, or NULL): for such a block, ceil(G/32) born words then
   * ceil(G/32) killed words over the key's G groups -- the OR of its ops' token-group records,
   * so a read including the whole block sets those bits without streaming its records. */
  const uint32_t *zone_gsum;
  /* Birth-ordered pairs (device stores with the token-group view, or NULL): for a birth
   * record rec_g[i] of a grouped key, prec[2 i + {0, 1}] = its group's pair (grp above); other
   * slots unspecified.  Records are in op order, so the groups that survive a read -- in an
   * add-wins set the newest add of each element, in an MV register the newest assigns --
   * have their births close together here, while in grp (output order) they lie a group run
   * apart: the record pass gathers a survivor's pair through its birth record. */
  const uint64_t *prec;        /* [n_rec][2] or NULL                                 */
  /* Escape rows (device stores with the packed view and n_dc >= 2, or NULL): an op escaped from
   * the packed view (pk_vc[0][p] == AM_PK_ESC) with pk_vc[1][p] = i > 0 has its full-width
   * inputs of is_op_in_snapshot/7 in row i - 1 of 2 + n_dc words: commit time, op_meta, then
   * snapshot_time entries by DC -- one contiguous row instead of n_dc + 2 column lines.  An
   * escaped op with pk_vc[1][p] == 0 (written in place since the rows were built) reads the
   * columns.  Escapes are ops with an entry outside the key's 2^32-us window (a DC whose entry
   * lags, e.g. behind a partition) or an invalid effect. */
  const uint64_t *esc_rows;    /* [n_esc][2 + n_dc] or NULL                           */
  /* Lag view (device stores with the packed view, n_dc <= 16, or NULL): an op's commit vector
   * as its commit time and one 16-bit lag per DC, so the inclusion test streams 4 + 2 * n_dc
   * bytes per op instead of 4 * n_dc (20 B at D = 8, not 32):
   *   lag_ct[p]     = commit_time - key_tbase[k]   (u32), or AM_PK_ESC when the op is escaped
   *                   from the packed view or one of its lags does not fit
   *   lag[d][p]     = (commit_time - X[d]) - key_lag[k][d]   in [0, 0xFFFF]   (X[dc] = ct: lag 0)
   *   key_lag[k][d] = the smallest commit_time - X[d] over the key's packed ops (int32)
   * so X[d] - key_tbase[k] = lag_ct[p] - key_lag[k][d] - lag[d][p].  Lags fit when a
   * transaction's snapshot entries trail its commit within a 65 ms band per (key, DC); the
   * reference's remote entries come from the stable snapshot, 0.1-1.2 s behind in 1 s steps
   * (src/clocksi_interactive_coord.erl:905-910), and do not.  Hence two rules.
   * Reader contract:
   *  - Two-level escape.  lag_ct[p] == AM_PK_ESC says only that the lag view does not hold op p.
   *    If pk_vc[0][p] != AM_PK_ESC (a lag-only escape) the op is evaluated from its packed entries
   *    X[d] = key_tbase[k] + pk_vc[d][p]; only an op escaped from the packed view reads its escape
   *    row or the full columns.
   *  - Routing.  A key whose lag-only escapes exceed AM_LAG_ROUTE_NUM / AM_LAG_ROUTE_DEN of its
   *    packed ops, or whose lag bases do not fit (INT32_MIN, INT32_MAX], is packed-routed: key_lag[k][0] ==
   *    AM_LAG_ROUTED, every lag_ct of the key is AM_PK_ESC, and the rest of its key_lag row and
   *    its lag columns are unspecified.  Readers test the mark before using the row and stream
   *    the key's packed view.
   * Maintained by every writer (am_store_apply rewrites a touched key's columns and its key_lag
   * row, mark included, and sets lag_ct = AM_PK_ESC on the slots a shrunk key frees).
   * A store also keeps, outside this struct, each key's lag width: an upper bound of the lags of
   * the key's ops the view holds (am_store_lag_width).  A read of the store's own log -- these
   * three pointers as am_store_log gives them, on the store's context -- sizes its commit-word
   * window by it; any other log (caller-built, or with a copied key_lag row) is read with the
   * format's 16 bits.  The results are the same either way. */
  const uint32_t *lag_ct;      /* [snap_stride]                                       */
  const uint16_t *lag;         /* [n_dc][snap_stride]                                 */
  const int32_t *key_lag;      /* [n_keys][n_dc]                                      */
  /* Group-span view (ABI 14; device stores with the token-group view, or NULL): a FRESH read (no
   * base snapshot) keeps a group iff its birth op is included and none of its effective kills
   * is, and in a causal history a token has at most one effective kill, so one word per BORN
   * group holds what the read needs.  key_nspan[k] = NB, the number of born groups of key k, or
   * AM_NSPAN_NONE when the key has no span view (key_ngrp[k] is AM_NGRP_NONE or carries
   * AM_NGRP_BIG, a group has two or more effective kill records, or the key has 65535 or more
   * ops): such a key is read through rec_g.  The spans reuse the record offsets (NB <= the key's
   * record slots, append room included): for the i-th birth of key k in record (= op) order,
   *   gspan[rec_key_off[k] + i] = birth op | kill op << 16   (op indices within the key; kill
   *                               op == birth op: no effective kill -- one always has a later op)
   *   gsrc[rec_key_off[k] + i]  = group index (its output rank, the g of grp) | birth record
   *                               index << 16 (the record of prec), read for survivors only
   * Every reader gives the same result with any of the three NULL (then through rec_g).
   * Maintained by every writer (am_store_apply copies a touched key's spans and key_nspan). */
  const uint32_t *key_nspan;   /* [n_keys]                                            */
  const uint32_t *gspan;       /* [n_rec]                                             */
  const uint32_t *gsrc;        /* [n_rec]                                             */
} am_op_log;
#define AM_ZONE_OPS 256u
#define AM_GMASK_MAX_GRP 32u
#define AM_REC_KILL (1u << 16)
#define AM_REC_OP(m) ((m) & 0xFFFFu)
#define AM_REC_GRP(m) ((m) >> 17)
#define AM_NGRP_NONE 0xFFFFFFFFu
#define AM_NSPAN_NONE 0xFFFFFFFFu
#define AM_GRP_MAX_REC 2048u
/* Chunked token-group view of a hot MV-register key (more than AM_BIG_MIN_OPS ops): its groups
 * are built with device-wide sorts instead of one workgroup's LDS, key_ngrp[k] = G |
 * AM_NGRP_BIG (G < AM_BIG_MAX_GRP), and its record range is laid out per AM_BIG_CHUNK ops:
 *   rec_g[rec_key_off[k] + c], c = 0..nch   the chunk table: record offset (relative to
 *                                           rec_key_off[k]) of the first record of key op
 *                                           c * AM_BIG_CHUNK; entry nch ends the last chunk
 *                                           (nch = ceil(ops / AM_BIG_CHUNK))
 *   then one record per birth / effective kill, in op order:
 *     op within its chunk (bits 0-9) | kill << 10 | group << 11, or 0xFFFFFFFF
 * Groups and their pairs (grp) are as above; an effective kill always follows its group's
 * birth, so a group survives a read iff its birth is included and no kill of it is. */
#define AM_NGRP_BIG 0x80000000u
#define AM_BIG_MIN_OPS (AM_GRP_MAX_REC / 2)
#define AM_BIG_CHUNK 1024u
#define AM_BIG_MAX_GRP (1u << 21)
#define AM_BREC_OP(m) ((m) & 0x3FFu)
#define AM_BREC_KILL (1u << 10)
#define AM_BREC_GRP(m) ((m) >> 11)
#define AM_PK_ESC 0xFFFFFFFFu
/* the packed-routed mark of a key (key_lag[k][0]) and the routing share */
#define AM_LAG_ROUTED INT32_MIN
#define AM_LAG_ROUTE_NUM 1u
#define AM_LAG_ROUTE_DEN 8u

/*
 * CRDT values (base snapshots in, materialized values out), SoA over reads.
 *   PN        v0
 *   LWW       v0 = ts (as u64 bits), v1 = value, vflag = 1 for the initial
 *             {0, <<>>} value (a binary sorts above every integer)
 *   AWSET     CSR of (elem, token) pairs: the orddict [{Elem, Tokens}] flattened in
 *             the reference's order (elems ascending, each token list in list order,
 *             the newest add first)
 *   MVREG     CSR of (value, token) pairs sorted (insert_sorted).  set_off[n+1] gives
 *             each read's capacity, set_len[n] the used length.
 *   BCOUNTER  the same CSR, one (slot, value) pair per orddict entry (present iff it was
 *             ever updated): the P orddict {From,To} -> N at slot From*n_dc+To, then the D
 *             orddict Id -> N at slot n_dc*n_dc+Id, each in key order (set_a = slot,
 *             set_b = the int64 value) -- only the touched entries, as the reference's
 *             orddicts hold them (src/bcounter_mgr.erl:80-97 effects), at most
 *             n_dc*n_dc + n_dc per read
 */
typedef struct am_values {
  int64_t *v0;
  uint64_t *v1;
  uint8_t *vflag;
  const uint64_t *set_off;
  uint32_t *set_len;
  uint64_t *set_a;
  uint64_t *set_b;
} am_values;

/* One batch of snapshot reads: the materialize/4 inputs per key. */
typedef struct am_read_batch {
  uint64_t n_reads;
  uint32_t per_read_clock; /* 0: one MinSnapshotTime for the whole batch; 1: one per read */
  uint32_t type_hint;      /* am_type when every read has that type (fast path); 0 = mixed */
  const uint64_t *key;        /* [n] key index into the log                          */
  const uint8_t *type;        /* [n] requested Type                                  */
  const uint64_t *read_vc;    /* [n_dc] or [n_dc][n] MinSnapshotTime                 */
  const uint32_t *read_pres;  /* [1] or [n]                                          */
  const uint64_t *txid;       /* [n] TxId, or NULL => every read's TxId is ignore    */
  const uint8_t *txid_valid;  /* [n] or NULL (all valid when txid != NULL)           */
  /* base snapshot: #snapshot_get_response{snapshot_time, materialized_snapshot} */
  const uint8_t *base_ignore; /* [n] 1 => snapshot_time = ignore; NULL => all ignore  */
  const uint64_t *base_vc;    /* [n_dc][n]                                            */
  const uint32_t *base_pres;  /* [n]                                                  */
  const int64_t *base_last_op;/* [n] or NULL => 0                                     */
  am_values base;             /* NULL members => the type's new() value               */
} am_read_batch;

/* materialize/4 outputs: {ok, Value, NewLastOp, LastOpCt, IsNewSS, Count} */
typedef struct am_read_result {
  int32_t *status;         /* [n] am_status                                */
  int64_t *new_last_op;    /* [n] NewLastOp                                */
  uint64_t *last_ct;       /* [n_dc][n] LastOpCt                           */
  uint32_t *last_ct_pres;  /* [n]                                          */
  uint8_t *last_ct_ignore; /* [n] 1 => LastOpCt = ignore                   */
  uint8_t *is_new_ss;      /* [n]                                          */
  uint32_t *count;         /* [n] number of effects applied                */
  uint8_t *flags;          /* [n] AM_FLAG_*                                */
  am_values value;
} am_read_result;

typedef struct am_ctx am_ctx;     /* device + HIP stream + scratch             */
typedef struct am_store am_store; /* a device-resident op log (one partition)  */
typedef struct am_comm am_comm;   /* RCCL communicator for the GST all-reduce  */

/* ---- context ---- */
int am_abi_version(void);
int am_ctx_open(int device, am_ctx **out);
int am_ctx_close(am_ctx *ctx);
void *am_ctx_stream(am_ctx *ctx);           /* hipStream_t */
int am_ctx_sync(am_ctx *ctx);
const char *am_last_error(void);            /* thread-local message of the last failure */
int am_timer_start(am_ctx *ctx);             /* hipEventRecord on the ctx stream         */
int am_timer_stop(am_ctx *ctx, float *ms);   /* records, syncs, returns elapsed ms       */
/* Counters of the context's kernels (synchronizes the stream): AM_STAT_OPS_SKIPPED = ops whose
 * commit vectors a read did not stream because their zone is inside its base snapshot
 * (am_op_log.zone_vc).  reset != 0 zeroes the counter after reading it. */
#define AM_STAT_OPS_SKIPPED 0
/* token-group records a read did not stream because their zones' group summaries stood in
 * for them (am_op_log.zone_gsum), and the summary words it read instead */
#define AM_STAT_RECS_SKIPPED 1
#define AM_STAT_GSUM_WORDS 2
int am_ctx_stat(am_ctx *ctx, int which, uint64_t *value, int reset);

/* ---- device memory helpers (the NIF owns no framework allocator) ---- */
int am_dev_alloc(am_ctx *ctx, size_t bytes, void **out);
int am_dev_free(am_ctx *ctx, void *p);
int am_memcpy_h2d(am_ctx *ctx, void *dst, const void *src, size_t bytes);
int am_memcpy_d2h(am_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ---- ops cache in HBM ---- */
/* Upload a host op log into device memory owned by the store. */
int am_store_create(am_ctx *ctx, const am_op_log *host_log, am_store **out);
/* Device view of the store (pointers are device pointers). */
int am_store_log(const am_store *st, am_op_log *out);
int am_store_destroy(am_store *st);
/* The zone index of a device store (am_op_log.zone_vc / zone_gsum): level AM_INDEX_NONE drops it,
 * AM_INDEX_ZONES keeps the per-block upper bounds only (base-snapshot reads skip the blocks
 * inside their base; no exact marks), AM_INDEX_EXACT adds the exact marks (fresh reads take an
 * exact block inside their clock whole), AM_INDEX_SUMMARIES adds the group summaries (the
 * default every store builder leaves).  Rebuilds from the op columns; blocks until done.
 * It frees and replaces the store's zone_vc / zone_gsum buffers: an am_op_log obtained from
 * am_store_log before the call holds stale pointers and must be fetched again. */
#define AM_INDEX_NONE 0
#define AM_INDEX_ZONES 1
#define AM_INDEX_EXACT 2
#define AM_INDEX_SUMMARIES 3
int am_store_index(am_ctx *ctx, am_store *st, int level);
/* Counters of the store's views, computed by a kernel over the views as they are now (not
 * cached: true after am_store_apply); blocks until done.  A store without a lag view reports
 * zeros for the last three. */
#define AM_VIEW_STAT_OPS 0           /* ops in the store                                      */
#define AM_VIEW_STAT_PK_ESC 1        /* ops escaped from the packed view                      */
#define AM_VIEW_STAT_LAG_ONLY_ESC 2  /* ops in the packed view with a lag that does not fit   */
#define AM_VIEW_STAT_ROUTED_KEYS 3   /* packed-routed keys (key_lag[k][0] == AM_LAG_ROUTED)   */
#define AM_VIEW_STAT_ROUTED_OPS 4    /* ops of those keys                                     */
#define AM_VIEW_STAT_N 5
int am_store_view_stats(am_ctx *ctx, const am_store *st, uint64_t out[AM_VIEW_STAT_N]);
/* The store's per-key lag widths -> host_out [n_keys]: for each key an upper bound (as built: the
 * maximum) of lag[d][p] over its ops in the lag view (lag_ct[p] != AM_PK_ESC) and d < n_dc; 0xFFFF
 * for a packed-routed key and a key with no op in the view.  Current after am_store_apply; blocks
 * until done.  AM_ERR_INVALID for a store without a lag view. */
int am_store_lag_width(am_ctx *ctx, const am_store *st, uint16_t *host_out);

/* ---- the hot path ---- */
/* Device pointers; runs on the ctx stream.  Asynchronous except for two data-dependent
 * counter readbacks: a mixed-type batch reads the lane tier's hand-off count once (and
 * returns there when every read was short), and a batch whose set / bounded-counter reads
 * reach the big-read tier reads that tier's count once to size its scratch. */
int am_materialize(am_ctx *ctx, const am_op_log *dev_log, const am_read_batch *dev_batch,
                   am_read_result *dev_res);
/* Host pointers for batch/result; the log is the store's device log.  Blocks. */
int am_materialize_host(am_ctx *ctx, const am_store *st, const am_read_batch *host_batch,
                        am_read_result *host_res);

/* ---- snapshot cache (materializer_vnode snapshot_cache-P) ----
 * Replaces get_from_snapshot_cache/5 + materialize_snapshot/7 + internal_store_ss/4 +
 * snapshot_insert_gc/4 around materialize/4, i.e. materializer_vnode:internal_read/7
 * (src/materializer_vnode.erl:371-376, 384-413, 469-509, 342-364, 515-563) and vector_orddict
 * get_smaller / insert_bigger (src/vector_orddict.erl:75-87, 127-140): per key at most
 * AM_SNAPSHOT_THRESHOLD snapshots, newest first, in HBM.  Every type's value: PN / LWW in
 * the entry, set pairs and bounded-counter slots in a device value pool. */
#define AM_SNAPSHOT_THRESHOLD 10   /* src/materializer_vnode.erl:37 */
#define AM_SNAPSHOT_MIN 3          /* :39 */
#define AM_MIN_OP_STORE_SS 5       /* :47 */
#define AM_SNAPCACHE_ABSENT 0xFFFFFFFFu
typedef struct am_snapcache am_snapcache;
int am_snapcache_create(am_ctx *ctx, uint32_t n_dc, uint64_t n_keys, am_snapcache **out);
int am_snapcache_destroy(am_snapcache *cache);
/* internal_read/7 (ShouldGC = false) for a batch of reads: each read's base comes from the
 * cache (the batch's base members are ignored), materialize/4 runs on it, and the result is
 * written back under materialize_snapshot/7's policy.  Per read status: AM_ERR_COLD_PATH
 * when no cached snapshot is vectorclock:le the read clock; AM_ERR_INVALID for a key read
 * a second time in the same batch (the first read, by index, owns the key; am_vnode_read
 * serves repeated keys in batch order).  The log's n_keys must equal the cache's.  Device
 * pointers; synchronizes once to size the value pool when the batch holds set or
 * bounded-counter reads. */
int am_snapcache_read(am_ctx *ctx, am_snapcache *cache, const am_op_log *dev_log, const am_read_batch *dev_batch,
                      am_read_result *dev_res);
/* The same with internal_read's ShouldGC per read (should_gc [n] or NULL = all false).  When
 * snapshot_insert_gc/4 runs for a key (its dict reached AM_SNAPSHOT_THRESHOLD, or ShouldGC),
 * the dict keeps its newest AM_SNAPSHOT_MIN entries and, if gc_mask is given, gc_mask[key] =
 * 1 with the prune threshold (vectorclock:min over the kept entries) in thr_vc[n_dc][n_keys]
 * / thr_pres[n_keys]: exactly the prune arguments of am_store_update (gc_mask is cleared
 * first). */
int am_snapcache_read_gc(am_ctx *ctx, am_snapcache *cache, const am_op_log *dev_log, const am_read_batch *dev_batch,
                         const uint8_t *should_gc, am_read_result *dev_res, uint8_t *gc_mask, uint64_t *thr_vc,
                         uint32_t *thr_pres);
/* The same with host batch/result (blocks). */
int am_snapcache_read_host(am_ctx *ctx, am_snapcache *cache, const am_store *st, const am_read_batch *host_batch,
                           am_read_result *host_res);
/* One key's entries (newest first) to host arrays of AM_SNAPSHOT_THRESHOLD (vc: x n_dc);
 * *n_entries = AM_SNAPCACHE_ABSENT before the key's first read.  NULL arrays are skipped. */
int am_snapcache_get(am_ctx *ctx, const am_snapcache *cache, uint64_t key, uint32_t *n_entries, uint64_t *vc,
                     uint32_t *pres, int64_t *last_op, int64_t *v0, uint64_t *v1, uint8_t *vflag);
/* Entry e's pool words (set pairs a/b; bounded-counter slot values a + presence pres, P slots
 * From*n_dc+To then D slots): *n_words, at most cap_words copied to the host arrays. */
int am_snapcache_get_value(am_ctx *ctx, const am_snapcache *cache, uint64_t key, uint32_t e, uint32_t cap_words,
                           uint32_t *n_words, uint64_t *a, uint64_t *b, uint8_t *pres);

/* A forced snapshot_insert_gc/4 on every cached key (src/materializer_vnode.erl:519-536): the
 * dict keeps its newest min(n, SNAPSHOT_MIN) entries and Thr = the reference's fold over them
 * (:523-527): Acc = the oldest kept clock, then Acc = vectorclock:min([CT1, Acc]) for each entry
 * newest first, where min([V1, V2]) lowers each DC of V1 to min(V1[dc], V2[dc]) with a DC
 * missing from V2 read as 0 (so while the initial {} snapshot is kept nothing is pruned; evidence
 * in oracle/ref_materializer.py vc_min2).  Device outputs: mask[n_keys] (1 = the key has
 * a threshold), thr_vc[n_dc][n_keys], thr_pres[n_keys] -- exactly the prune arguments of
 * am_store_update (so ops are only pruned below snapshots that stay cached).  n_keys is the
 * cache's: hand the outputs only to am_store_update of a store with the same key count (the
 * thr_vc stride; am_snapcache_read already requires it, Store.update checks it). */
int am_snapcache_gc_threshold(am_ctx *ctx, am_snapcache *cache, uint8_t *mask, uint64_t *thr_vc,
                              uint32_t *thr_pres);

/* ---- one partition's materializer_vnode state: ops cache + snapshot cache ----
 * am_vnode_insert_host runs op_insert_gc/3 (src/materializer_vnode.erl:622-647) for every op
 * of host_ops (a host log over the vnode's keys, each key's ops oldest -> newest; a log over
 * more keys grows the vnode's key space first -- the new keys' tuples appear with their first
 * op, :624-629 -- reads of keys past the key space are AM_ERR_INVALID):
 * NewId = OpCounter + 1, and when Length >= ListLen or NewId rem 50 == 0 the GC read
 * internal_read(Key, Type, Op.snapshot_time, ignore, [], true) runs first (store the
 * snapshot, snapshot_insert_gc/4: keep SNAPSHOT_MIN snapshots, prune_ops below their min,
 * resize ListLen); load_ops/2 (:312-319) replays the log through this call.
 * am_vnode_read_host runs internal_read/7 (:371-376) for a host batch (should_gc [n] or
 * NULL), repeated keys served in batch order.  Reads whose dict reaches SNAPSHOT_THRESHOLD
 * GC the same way.  Both block.  The ops cache keeps room for appends per key: a batch touching
 * a few keys is applied in place at O(those keys' ops) (am_store_apply); a key that outgrows its
 * room rebuilds the store once, regrowing every key's room (am_vnode_stats counts both). */
typedef struct am_vnode am_vnode;
int am_vnode_create(am_ctx *ctx, uint32_t n_dc, uint64_t n_keys, am_vnode **out);
int am_vnode_destroy(am_vnode *v);
int am_vnode_insert_host(am_vnode *v, const am_op_log *host_ops);
int am_vnode_read_host(am_vnode *v, const am_read_batch *host_batch, const uint8_t *should_gc,
                       am_read_result *host_res);
/* the vnode's current store and snapshot cache (borrowed; the store changes on GC) */
int am_vnode_parts(am_vnode *v, am_store **st, am_snapcache **sc);
/* ingestion counters: whole-store rebuilds (a key outgrew its room for appends, or the first
 * insert) and in-place applies of the touched keys (am_store_apply, the common case) */
int am_vnode_stats(am_vnode *v, uint64_t *rebuilds, uint64_t *in_place);
/* the ops-cache tuple header of a key: {Length, ListLen} and OpCounter (element 3) */
int am_vnode_key_info(am_vnode *v, uint64_t key, uint64_t *length, uint64_t *list_len, uint64_t *op_counter);

/* ---- read_objects: one transaction's reads over a node's partitions, one call ----
 * clocksi_interactive_coord's read_objects fan-out (src/clocksi_interactive_coord.erl:
 * 732-747) sends one read per key to its partition's read server, which calls
 * materializer_vnode:read/6 (src/clocksi_readitem_server.erl:217-228).  Here the partitions
 * a GPU owns share one vnode whose key space concatenates theirs: partition p owns vnode
 * keys [part_key_base[p], part_key_base[p+1]).  Request i reads partition part[i]'s local
 * key host_batch->key[i]; every request of every partition is ONE internal_read/7 batch
 * (snapshot cache, materialize/4, write-back), results in request order (repeated keys in
 * request order).  A request outside its partition's range gets AM_ERR_INVALID.
 * am_read_objects_submit returns at once; the read runs on a worker thread and
 * am_ticket_wait returns its status (and frees the ticket).  Every buffer the batch and the
 * result point to must stay valid until then. */
typedef struct am_ticket am_ticket;
int am_read_objects_host(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                         const am_read_batch *host_batch, am_read_result *host_res);
int am_read_objects_submit(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                           const am_read_batch *host_batch, am_read_result *host_res, am_ticket **out);
int am_ticket_wait(am_ticket *t);

/* ---- read-your-writes: materialize_eager/3 on the device (am_eager.hip, ABI 15) ----
 * materializer:materialize_eager(Type, Snapshot, Effects) (src/materializer.erl:62-70) folds a
 * transaction's own effects for a key into the snapshot it read: no clocks, no inclusion test,
 * no op log.  clocksi_vnode:read_data_item/5 (src/clocksi_vnode.erl:99-107) does it to every
 * read of a key the transaction wrote, with the effects reverse_and_filter_updates_per_key/2
 * (:660-668) returns; the coordinator does it to every read_objects reply
 * (apply_tx_updates_to_snapshot/4, src/clocksi_interactive_coord.erl:883-894).
 *
 * The reading transactions' own effects, for n_ws rows of a value batch.  Effects use am_op_log's
 * payload encoding (kind and AM_META_BAD in eff_meta, DC bits ignored; p0, p1; var words). */
typedef struct am_writeset {
  uint64_t n_ws, n_eff, n_var;
  const uint64_t *row;      /* [n_ws] row in the input values / status, distinct            */
  const uint8_t  *type;     /* [n_ws] am_type of that read                                  */
  const uint64_t *eff_off;  /* [n_ws+1] entry i's effects, in APPLICATION order (oldest     */
                            /* first: reverse_and_filter_updates_per_key's output)          */
  const uint8_t  *eff_meta; /* [n_eff] */
  const uint64_t *p0, *p1;  /* [n_eff] */
  const uint64_t *var_off;  /* [n_eff+1] or NULL */
  const uint64_t *var_data; /* [n_var] */
} am_writeset;
/* Limits of one entry's write set (add-wins set and MV register): the tokens its effects insert
 * (births: every AW add token, one per MV assign), the tokens they drop (kills: every AW remove
 * token, every MV overridden token) and its effects.  An entry beyond them gets AM_ERR_CAPACITY.
 * The base value has no limit: it is streamed, never held on chip. */
#define AM_EAGER_MAX_BIRTHS 1024u
#define AM_EAGER_MAX_KILLS 2048u
#define AM_EAGER_MAX_EFFECTS 32767u
/* Base pairs streamed per pass by the two kernel shapes: one wavefront per entry whose write set
 * has at most AM_EAGER_SMALL_WORDS effects + variable words (and, for a bounded counter, at most
 * AM_EAGER_SMALL_SLOTS slots n_dc * n_dc + n_dc), else one 256-thread workgroup. */
#define AM_EAGER_TILE_WAVE 64u
#define AM_EAGER_TILE_WG 256u
#define AM_EAGER_SMALL_WORDS 128u
#define AM_EAGER_SMALL_SLOTS 128u
/* Entry i of dev_out / out_status = materialize_eager(type[i], the value at row[i] of dev_in,
 * entry i's effects).  dev_out has n_ws rows (its own set_off capacities); dev_in is not written
 * (NULL members => the type's new() value).  Device pointers (the structs themselves live in
 * host memory); asynchronous on the context stream, no host readback.
 *   in_status[row[i]] != AM_OK      out_status[i] is a copy of it, the output row is empty: the
 *                                   {error, Reason} pass-through of src/clocksi_vnode.erl:105-106
 *   AM_ERR_UNEXPECTED_OPERATION     an effect carries AM_META_BAD or a malformed variable payload
 *                                   (the store builder's rule); wins over every other code, as
 *                                   the reference stops at the first bad effect
 *   AM_ERR_OVERFLOW                 a PN / bounded-counter result outside int64 (summed exactly
 *                                   in 128 bits)
 *   AM_ERR_CAPACITY                 the result exceeds the row's set_off capacity, or the entry
 *                                   the limits above
 *   AM_ERR_INVALID                  an unknown type, effect offsets outside the write set, or a
 *                                   set / bounded-counter entry without set columns in dev_out
 * A row with an error status holds no value (set_len 0).
 * Per type (the reference's Type:update/2): PN the sum; LWW erlang:max(Effect, State); bounded
 * counter the keyed sums of the P / D slots, a slot present once an effect touched it; add-wins
 * set and MV register the closed form of am_sets.hip with the base pairs as births before the
 * first effect -- a birth survives unless a kill of the same token (set: and element) comes at a
 * strictly later effect.  Set order: elements ascending, within one element the newest effect's
 * add tokens first (in the effect's order), the base tokens last in base order; MV order:
 * (value, token), equal pairs once.  As in am_sets.hip the closed form differs from the list
 * semantics only when a live token is added again (both copies are kept). */
int am_materialize_eager(am_ctx *ctx, uint32_t n_dc, const am_writeset *dev_ws, const am_values *dev_in,
                         const int32_t *in_status /* or NULL */, am_values *dev_out, int32_t *out_status);
/* The same with host pointers; blocks.  Only the rows named by host_ws->row are read. */
int am_materialize_eager_host(am_ctx *ctx, uint32_t n_dc, const am_writeset *host_ws, const am_values *host_in,
                              const int32_t *in_status /* or NULL */, am_values *host_out, int32_t *out_status);
/* am_read_objects_host / _submit, then the value and status of the requests host_ws->row names
 * are replaced by the eager result (capacity: host_res's own set_off), on the device before the
 * result is copied back; every other result column stays the snapshot read's.  host_ws == NULL
 * or n_ws == 0: exactly am_read_objects_host / _submit.  host_ws and its arrays must stay valid
 * until the call (the ticket's wait) returns. */
int am_read_objects_ws_host(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                            const am_read_batch *host_batch, const am_writeset *host_ws, am_read_result *host_res);
int am_read_objects_ws_submit(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                              const am_read_batch *host_batch, const am_writeset *host_ws, am_read_result *host_res,
                              am_ticket **out);

/* ---- downstream generation on the device (am_downstream.hip) ----
 * clocksi_downstream:generate_downstream_op/6 (src/clocksi_downstream.erl:41-68) for a batch: a
 * client update plus the state it read (the snapshot with the transaction's own writes folded in,
 * am_materialize_eager / am_read_objects_ws_*) becomes the effect Type:downstream/2 returns, in
 * am_writeset's / am_op_log's payload encoding.  The states never leave the device.
 *
 * Update op codes per type and their arguments:
 *   PN        AM_UP_PN_INCREMENT / _DECREMENT    a0 = N (int64)
 *   LWW       AM_UP_LWW_ASSIGN                   a0 = timestamp (the caller's make_micro_epoch()),
 *                                                a1 = value
 *   AWSET     AM_UP_AW_ADD      var = [elem, token] pairs, elems strictly ascending (add, add_all
 *                               after lists:usort; one fresh token per element)
 *             AM_UP_AW_REMOVE   var = elems, strictly ascending (remove, remove_all)
 *             AM_UP_AW_RESET    no arguments
 *   MVREG     AM_UP_MV_ASSIGN   a0 = value, a1 = the fresh token;  AM_UP_MV_RESET  no arguments
 *   BCOUNTER  AM_UP_BC_INCREMENT / _DECREMENT    a0 = N (int64), a1 = DC index
 *             AM_UP_BC_TRANSFER                  a0 = N, a1 = from | (to << 8)
 * Tokens come from the caller, fresh and interned through the codec before the call. */
#define AM_UP_PN_INCREMENT 0
#define AM_UP_PN_DECREMENT 1
#define AM_UP_LWW_ASSIGN 0
#define AM_UP_AW_ADD 0
#define AM_UP_AW_REMOVE 1
#define AM_UP_AW_RESET 2
#define AM_UP_MV_ASSIGN 0
#define AM_UP_MV_RESET 1
#define AM_UP_BC_INCREMENT 0
#define AM_UP_BC_DECREMENT 1
#define AM_UP_BC_TRANSFER 2
typedef struct am_updates {          /* one client update per entry */
  uint64_t n_up, n_var;
  const uint64_t *row;               /* [n_up] row of the input values / in_status, distinct */
  const uint8_t  *type;              /* [n_up] am_type */
  const uint8_t  *op;                /* [n_up] AM_UP_* */
  const uint64_t *a0, *a1;           /* [n_up] scalar arguments (table above) */
  const uint64_t *var_off;           /* [n_up+1] or NULL (no update has variable arguments) */
  const uint64_t *var_data;          /* [n_var] set elements / [elem, token] pairs */
} am_updates;
/* out: one effect per update.  row and type of the updates together with these columns are a
 * valid am_writeset with n_ws = n_eff = n_up (eff_off = 0..n_up) and n_var = var_cap (a bound of
 * *n_var, which can stay on the device): device pointers go straight into am_materialize_eager,
 * or into a dev_new log's payload columns. */
typedef struct am_effects {
  uint64_t var_cap;
  uint64_t *eff_off;                 /* [n_up+1] = 0..n_up */
  uint8_t  *eff_meta; uint64_t *p0, *p1;   /* [n_up] */
  uint64_t *var_off;                 /* [n_up+1] */
  uint64_t *var_data;                /* [var_cap] */
  uint64_t *n_var;                   /* [1] words needed */
  int64_t  *avail;                   /* [n_up] or NULL */
} am_effects;
/* A 256-thread workgroup instead of a wavefront writes an effect that copies more than this many
 * state pairs whole (an add-wins-set reset, an MV assign / reset): one full workgroup pass. */
#define AM_DS_TILE_WG 256u
/* Effect i / out_status[i] = Type:downstream(update i, the value at row[i] of dev_in).  Three
 * steps on the context stream with no host readback: sizes and statuses, an exclusive scan into
 * var_off (total in *n_var), the fill.  dev_in is not written.  Effects (the reference's rules;
 * antidote_crdt's downstream/2 is not vendored, DESIGN.md 4c''):
 *   PN        p0 = N / -N, no state read         LWW  p0 = timestamp, p1 = value, no state read
 *   AWSET     add / remove: per requested element {E, [Token] or [], the current tokens of E};
 *             reset: {E, [], Tokens} for every element of the state, in state order
 *   MVREG     AM_MV_ASSIGN p0 = value, p1 = token / AM_MV_RESET; var = every token of the state
 *   BCOUNTER  AM_BC_INCREMENT p0 = N, p1 = dc | dc << 8; an increment of N < 0 is a decrement of
 *             -N (src/bcounter_mgr.erl:89-90); AM_BC_DECREMENT / AM_BC_TRANSFER when
 *             localPermissions(dc / from) >= N, else AM_ERR_NO_PERMISSIONS (:120-129).
 *             avail[i] (if given) = the local permissions for decrements and transfers
 *             (bcounter_mgr queues Amount - Available on a refusal), 0 for every other update
 * Statuses:
 *   in_status[row[i]] != AM_OK    copied to out_status[i] for set / MV / bounded-counter updates
 *                                 ({error, {gen_downstream_read_failed, Reason}},
 *                                 src/clocksi_downstream.erl:51-52); PN and LWW ignore it
 *   AM_ERR_INVALID                an unknown type or op (wins over the pass-through); set
 *                                 elements not strictly ascending or argument offsets outside
 *                                 var_data; a bounded-counter amount <= 0 after the sign rule; a DC
 *                                 index >= n_dc; a set / MV / bounded-counter update whose input
 *                                 lacks set columns; and for EVERY update of the call when two
 *                                 updates name one row (two updates of one key are two calls with
 *                                 an eager fold between them, src/clocksi_interactive_coord.erl:986)
 *   AM_ERR_OVERFLOW               negating INT64_MIN; local permissions outside int64 (summed
 *                                 exactly in 128 bits)
 *   AM_ERR_NO_PERMISSIONS         {error, no_permissions}
 *   AM_ERR_CAPACITY               *n_var > var_cap: every update that needs variable words gets it
 *                                 and no variable word is written; *n_var holds the needed total
 * An update with a non-OK status has no variable words (var_off[i+1] == var_off[i]) and
 * AM_META_BAD in eff_meta[i], so its effect can never be applied half-written. */
int am_generate_downstream(am_ctx *ctx, uint32_t n_dc, const am_updates *dev_up, const am_values *dev_in,
                           const int32_t *in_status /* or NULL */, am_effects *dev_eff, int32_t *out_status);
/* The same with host pointers; blocks.  Only the rows the updates name are read.  A repeated row
 * makes the call itself return AM_ERR_INVALID. */
int am_generate_downstream_host(am_ctx *ctx, uint32_t n_dc, const am_updates *host_up, const am_values *host_in,
                                const int32_t *in_status /* or NULL */, am_effects *host_eff, int32_t *out_status);
/* The coordinator-level call: am_read_objects_ws_host / _submit of the batch (request i is row i;
 * host_ws or NULL: the transaction's write set so far), the values left in the device result with
 * set_off [n_reads + 1] as their capacities, then am_generate_downstream of host_up on them.  Only
 * the effects, out_status [n_up] and avail come back (one readback of *n_var sizes the copy).  The
 * requests must name distinct keys (AM_ERR_INVALID otherwise).  Every buffer must stay valid
 * until the call (the ticket's wait) returns. */
int am_update_objects_host(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                           const am_read_batch *host_batch, const uint64_t *set_off, const am_writeset *host_ws,
                           const am_updates *host_up, am_effects *host_eff, int32_t *out_status);
int am_update_objects_submit(am_vnode *v, uint32_t n_parts, const uint64_t *part_key_base, const uint32_t *part,
                             const am_read_batch *host_batch, const uint64_t *set_off, const am_writeset *host_ws,
                             const am_updates *host_up, am_effects *host_eff, int32_t *out_status, am_ticket **out);

/* ---- commit on the device (am_commit.hip) ----
 * clocksi_vnode:commit/5 -> update_materializer/3 (src/clocksi_vnode.erl:499-531, 634-657) stamps
 * every effect of a transaction with {DcId, TxCommitTime}, its vec_snapshot_time and its TxId and
 * hands it to materializer_vnode:update/2 -> op_insert_gc/3; inter_dc_dep_vnode does the same for a
 * remote transaction under its own commit DC (src/inter_dc_dep_vnode.erl:150-152).  A batch of
 * committed transactions goes in as it is -- one row per transaction, one row per effect in
 * am_effects' / am_writeset's columns, `key` where the write set has `row` -- and the device turns
 * it into the CSR op log over the touched keys that am_store_apply takes as dev_new. */
typedef struct am_commits {      /* committed transactions, in the order the vnode commits them */
  uint64_t n_tx, n_eff, n_var;
  const uint8_t  *dc;            /* [n_tx] commit DC index (own DC, or a remote txn's origin)   */
  const uint64_t *commit_time;   /* [n_tx]                                                       */
  const uint64_t *snap_vc;       /* [n_tx][n_dc] vec_snapshot_time, transaction-major            */
  const uint32_t *snap_pres;     /* [n_tx] or NULL = every DC present                            */
  const uint64_t *txid;          /* [n_tx] am_txid ids, or NULL                                  */
  const uint64_t *eff_off;       /* [n_tx+1] transaction t's effects, oldest first               */
  const uint64_t *key;           /* [n_eff] vnode key                                            */
  const uint8_t  *type;          /* [n_eff] am_type                                              */
  const uint8_t  *eff_meta; const uint64_t *p0, *p1;   /* [n_eff] as am_effects / am_writeset    */
  const uint64_t *var_off, *var_data;                  /* [n_eff+1] or NULL, [n_var]             */
} am_commits;
/* The device buffers am_commit_build writes, supplied by the caller (n_eff and n_var are known on
 * the host before the call): cap_ops >= n_eff, cap_var >= n_var, snap_stride >= cap_ops. */
typedef struct am_commit_log {
  uint64_t cap_ops, cap_var, snap_stride;
  uint64_t *keys;                /* [cap_ops] the distinct keys, ascending                       */
  uint64_t *key_off;             /* [cap_ops+1]                                                  */
  uint8_t  *key_type, *key_flags;/* [cap_ops]                                                    */
  uint8_t  *op_meta;             /* [cap_ops]                                                    */
  uint64_t *commit_time;         /* [cap_ops]                                                    */
  uint64_t *snap_vc;             /* [n_dc][snap_stride] DC-major                                 */
  uint32_t *snap_pres;           /* [cap_ops]; written when the batch has snap_pres              */
  uint64_t *op_txid;             /* [cap_ops]; written when the batch has txid                   */
  uint64_t *p0, *p1;             /* [cap_ops]                                                    */
  uint64_t *var_off;             /* [cap_ops+1]                                                  */
  uint64_t *var_data;            /* [cap_var]                                                    */
  uint32_t *src;                 /* [cap_ops] the batch effect index of each output op           */
} am_commit_log;
/* *bad of am_commit_build: why the batch is invalid */
#define AM_COMMIT_BAD_DC 0x1u       /* a transaction's dc >= n_dc                                 */
#define AM_COMMIT_BAD_EFF_OFF 0x2u  /* eff_off decreasing, not starting at 0 or not ending at n_eff */
#define AM_COMMIT_BAD_VAR_OFF 0x4u  /* var_off decreasing or beyond n_var                         */
#define AM_COMMIT_BAD_TYPE 0x8u     /* an unknown am_type                                         */
#define AM_COMMIT_BAD_KEY 0x10u     /* a key with bits at or above key_bits set                   */
/* Device pointers in dev_commits and out (the structs themselves live in host memory); runs on the
 * context stream with ONE readback, a status block holding *n_touched and *bad.  On AM_OK
 * *out_log is the am_op_log over out's buffers (n_keys = *n_touched, n_ops = n_eff; snap_pres /
 * op_txid NULL when the batch has none), ready as am_store_apply's dev_new with out->keys:
 *   order      a key's ops by (transaction index, effect index in the transaction): a stable sort
 *              by key alone (update_materializer's lists:reverse + foldl across serial commits);
 *              two effects of one transaction on one key stay two ops, in order
 *   op_meta    the transaction's dc in the DC bits | the effect's kind and AM_META_BAD bits;
 *              commit_time, snap_pres, op_txid broadcast from the transaction; snap_vc transposed
 *   key_type   the type of the key's first op in the batch; key_flags = AM_KEY_MIXED_TYPES when
 *              the key's ops in the batch disagree
 *   src[q]     the batch effect index of output op q
 * key_bits: the radix sort covers the low key_bits bits of the keys (1..64, the bits the batch's
 * largest key needs; 64 always works).  AM_ERR_INVALID (*bad says why, nothing in out is to be
 * used): dc >= n_dc, eff_off not non-decreasing from 0 to n_eff, var_off decreasing or beyond
 * n_var, an unknown type, a key above key_bits, n_eff >= 2^32, capacities below the batch.
 * n_tx == 0 or n_eff == 0: AM_OK with *n_touched = 0. */
int am_commit_build(am_ctx *ctx, uint32_t n_dc, const am_commits *dev_commits, uint32_t key_bits,
                    const am_commit_log *out, am_op_log *out_log, uint64_t *n_touched, uint32_t *bad /* or NULL */);
/* op_insert_gc/3 for every effect of a host batch, as am_vnode_insert_host does for the same ops
 * given as a host log (ids OpCounter+1.., the write-triggered GC reads with the trigger op's
 * snapshot_time, ListLen resizing, in-place apply or one rebuild, growth of the key space to the
 * batch's largest key + 1, am_vnode_stats), at O(batch) on the host: the batch is uploaded,
 * am_commit_build runs, and only the touched keys, their counts and src come back to plan the GC
 * rounds.  An invalid batch returns AM_ERR_INVALID and leaves the vnode as it was.  Blocks. */
int am_vnode_commit_host(am_vnode *v, const am_commits *host_commits);

/* ---- the partition log in HBM and the cold read (am_plog.hip) ----
 * materializer_vnode:get_from_snapshot_log/3 -> logging_vnode:get_up_to_time/5
 * (src/materializer_vnode.erl:415-419, src/logging_vnode.erl:522-545, 586-591, 676-779): a read with
 * no cached snapshot at or below its clock (AM_ERR_COLD_PATH above) is answered from the partition's
 * log.  The log here is the sequence of commit batches (am_commits) as am_vnode_commit_host takes
 * them -- the committed content of disk_log, in the order the commit records were appended; durability
 * stays with the caller.  Append-only and transaction-major: per transaction dc, commit_time, one
 * snap_vc row, snap_pres (every DC when the batch has none) and txid (0 when the batch has none); per
 * effect key, type, eff_meta, p0, p1, its variable words, and a 16-byte link {the previous effect on
 * the same key, the effect's transaction}, so a key's effects are a chain from its newest one.
 * Capacities double (small ones are legal); an append costs O(batch) on host and device. */
typedef struct am_plog am_plog;
int am_plog_create(am_ctx *ctx, uint32_t n_dc, uint64_t cap_tx, uint64_t cap_eff, uint64_t cap_var, am_plog **out);
int am_plog_destroy(am_plog *plog);
/* A host batch behind the log; transactions without effects count (a horizon is a number of
 * transactions).  Validated as am_commit_build validates: an invalid batch returns AM_ERR_INVALID and
 * leaves the log as it was.  Blocks. */
int am_plog_append_host(am_plog *plog, const am_commits *host_commits);
/* transactions, effects and variable words in the log (NULL outputs are skipped) */
int am_plog_size(const am_plog *plog, uint64_t *n_tx, uint64_t *n_eff, uint64_t *n_var);
/* Test accessor: the global effect indices of key's chain among the first `horizon` transactions,
 * oldest first, not filtered by any clock, to the host array eff_idx [cap]; *n = their number
 * (AM_ERR_CAPACITY when cap is smaller: nothing is written). */
int am_plog_key_ops(am_plog *plog, uint64_t key, uint64_t horizon, uint64_t cap, uint64_t *eff_idx, uint64_t *n);
/* Every read of the batch served from the log, whatever a snapshot cache holds (the batch's base
 * members are ignored): for read r, among the first horizon[r] transactions (dev_horizon [n], or NULL
 * = the whole log; when op_insert_gc/3 of transaction i's ops runs its GC read the log holds
 * transactions 0..i, so that read's horizon is i + 1), every effect on the read's key, in log order,
 * whose transaction's snapshot_time is vectorclock:le the read clock (over the keys of both, a missing
 * entry 0; the snapshot_time itself, not the commit-substituted vector) is an op; the survivors get
 * ids 0, 1, 2, ... oldest first and are materialized (materialize/4) from new(Type) with
 * last_op_id 0 under the snapshot clock {} -- a clock, not ignore, so LastOpCt is never ignore.
 * Outputs are am_materialize's: a type mismatch among the survivors is AM_ERR_CORRUPTED_OPS_CACHE, an
 * included bad effect AM_ERR_UNEXPECTED_OPERATION, a survivor outside the read clock lowers
 * NewLastOp to its id - 1 (-1 for id 0); effects that fail the filter are absent altogether.  A read
 * without survivors gives AM_OK, new(), NewLastOp 0, LastOpCt {}, IsNewSS 0, Count 0.
 * Three kernels and two scans build a plain am_op_log over "keys" = the reads (one readback of its
 * sizes), which am_materialize's tiers read as it is: O(the read keys' logged effects) on the
 * device, O(reads) on the host, whatever the log's length.  Device pointers. */
int am_plog_read(am_ctx *ctx, am_plog *plog, const am_read_batch *dev_batch, const uint64_t *dev_horizon,
                 am_read_result *dev_res);
/* The same with host batch, horizons and result; blocks. */
int am_plog_read_host(am_ctx *ctx, am_plog *plog, const am_read_batch *host_batch, const uint64_t *host_horizon,
                      am_read_result *host_res);
/* A vnode that keeps its partition's log: it answers every internal_read/7 the reference answers.
 * am_vnode_create's vnode behaves exactly as before, AM_ERR_COLD_PATH included.  On a logged vnode
 *   am_vnode_commit_host   appends the batch to the log first (append_commit before
 *                          update_materializer, src/clocksi_vnode.erl:517-519; the remote path
 *                          likewise, src/inter_dc_dep_vnode.erl:146-152), the chain links from the
 *                          am_commit_build output it makes anyway; each GC read of op_insert_gc/3
 *                          carries the horizon of its trigger op's transaction, so a GC read that
 *                          goes cold sees the log as the reference's does.  An invalid batch leaves
 *                          the log and the vnode unchanged.
 *   am_vnode_read_host, am_read_objects_*, am_read_objects_ws_*, am_update_objects_*
 *                          a read with no cached snapshot at or below its clock is read from the
 *                          whole log (am_plog_read's rules) before the write set and the updates
 *                          see its row, and its snapshot is stored as materialize_snapshot/7
 *                          stores a response that is not the newest snapshot: iff ShouldGC, through
 *                          internal_store_ss/4 -> insert_bigger -> snapshot_insert_gc/4 as for any
 *                          read (last_op_id in log ids, as the reference does).  A round with a log
 *                          pays one small readback to learn whether any read went cold.
 *   am_vnode_insert_host   AM_ERR_UNSUPPORTED, the vnode as it was: a per-key host log has no commit
 *                          order.
 *   am_vnode_relabel       also maps the log's label words, by each effect's type.
 * am_vnode_log: the vnode's log (borrowed; NULL for a plain vnode). */
int am_vnode_create_logged(am_ctx *ctx, uint32_t n_dc, uint64_t n_keys, am_vnode **out);
int am_vnode_log(am_vnode *v, am_plog **plog);

/* ---- the partition's write-write certification (am_cert.hip) ----
 * clocksi_vnode:prepare/6, certification_check/4, commit/5's committed_tx insert and clean_prepared/3
 * (src/clocksi_vnode.erl:450-632) and the read servers' check_clock/4 + check_prepared_list/3
 * (src/clocksi_readitem_server.erl:236-264), for batches: a call leaves the tables, and returns the
 * statuses, that serving the batch's transactions one at a time in batch order gives.  Keys, TxIds and
 * times are opaque u64, every value legal.  Two open-addressed tables in HBM, sized by am_cert_create /
 * am_cert_reserve and by nothing else: committed (key -> commit time; cap_keys keys) and prepared (a
 * multimap key -> (txid, prepare time); cap_entries live entries after any number of prepare / finish
 * cycles -- removals leave tombstones, which a prepare compacts away before it runs when they crowd
 * the table).  record_commits = 0: no commit time is recorded (the reference's txn_cert off).
 * Per-transaction statuses: AM_OK, AM_ERR_WRITE_CONFLICT, AM_ERR_NO_UPDATES.
 *   prepare   a certifying transaction conflicts when a key has committed[k] > start_time, holds a
 *             prepared entry of any transaction, or is named by an earlier transaction of the batch
 *             that ended AM_OK; no conflict and no keys: AM_ERR_NO_UPDATES; else one entry
 *             (txid, prepare_time) per distinct key that has no entry of this TxId yet
 *   finish    no keys: AM_ERR_NO_UPDATES; else committed[k] = commit_time for every key when committed
 *             (the last transaction of the batch wins), and the entry (k, txid) leaves every key
 * A malformed batch (key_off not non-decreasing from 0 to n_pairs; 2^32 or more pairs or transactions)
 * returns AM_ERR_INVALID; a prepare whose AM_OK transactions need more than cap_entries live entries,
 * or a finish that needs more than cap_keys committed keys, returns AM_ERR_CAPACITY; both leave the
 * tables and dev_status untouched (the device decides before its first insert).  The structs live in
 * host memory; the plain calls take device columns and leave their work on the context's stream, the
 * _host twins take host columns and block. */
#define AM_CERT_SPIN_WAIT_MS 10 /* ?SPIN_WAIT, include/antidote.hrl:53 */
typedef struct am_cert am_cert;
typedef struct am_prepares {
  uint64_t n_tx, n_pairs;
  const uint64_t *txid, *start_time, *prepare_time; /* [n_tx] */
  const uint8_t *certify;                           /* [n_tx] */
  const uint64_t *key_off;                          /* [n_tx+1] */
  const uint64_t *key;                              /* [n_pairs] */
} am_prepares;
typedef struct am_finishes {
  uint64_t n_tx, n_pairs;
  const uint64_t *txid, *commit_time; /* [n_tx] */
  const uint8_t *committed;           /* [n_tx] */
  const uint64_t *key_off;            /* [n_tx+1] */
  const uint64_t *key;                /* [n_pairs] */
} am_finishes;
int am_cert_create(am_ctx *ctx, uint64_t cap_keys, uint64_t cap_entries, int record_commits, am_cert **out);
int am_cert_destroy(am_cert *cert);
/* New capacities (the only call that allocates table memory): new buffers, a rehash kernel, a stream
 * synchronize, then the old buffers are freed.  AM_ERR_INVALID below the live content.  Blocks. */
int am_cert_reserve(am_cert *cert, uint64_t cap_keys, uint64_t cap_entries);
int am_cert_prepare(am_cert *cert, const am_prepares *dev, int32_t *dev_status);
int am_cert_prepare_host(am_cert *cert, const am_prepares *host, int32_t *host_status);
int am_cert_finish(am_cert *cert, const am_finishes *dev, int32_t *dev_status);
int am_cert_finish_host(am_cert *cert, const am_finishes *host, int32_t *host_status);
/* wait_ms[i]: (start - now) div 1000 + 1 when start > now; else AM_CERT_SPIN_WAIT_MS when the key holds
 * a prepared entry with time <= start; else 0 */
int am_cert_read_ready(am_cert *cert, uint64_t n, const uint64_t *dev_key, const uint64_t *dev_start, uint64_t now,
                       uint64_t *dev_wait_ms);
int am_cert_read_ready_host(am_cert *cert, uint64_t n, const uint64_t *host_key, const uint64_t *host_start,
                            uint64_t now, uint64_t *host_wait_ms);
/* get_min_prep/1: the smallest prepare time in the table; *present = 0 when it is empty.  Blocks. */
int am_cert_min_prepared(am_cert *cert, uint64_t *time, int *present);
/* Test accessor: the key's commit time (0 = none) and its prepared entries sorted by (time, txid) to
 * the host arrays txid / time [cap]; *n = their number (AM_ERR_CAPACITY when cap is smaller: the
 * arrays are not written).  Blocks. */
int am_cert_key_info(am_cert *cert, uint64_t key, uint64_t *commit_time, uint64_t cap, uint64_t *txid, uint64_t *time,
                     uint64_t *n);
int am_cert_size(am_cert *cert, uint64_t *committed_keys, uint64_t *prepared_entries, uint64_t *cap_keys,
                 uint64_t *cap_entries);
/* counters since create (NULL outputs are skipped): resolve rounds launched, status-block readbacks,
 * compactions of the prepared table */
int am_cert_stats(am_cert *cert, uint64_t *rounds, uint64_t *readbacks, uint64_t *compactions);

/* ---- remote delivery: the dependency buffer of every partition a GPU owns (am_dep.hip) ----
 * inter_dc_dep_vnode's queues, try_store/2 and partition clock (src/inter_dc_dep_vnode.erl:94-154,
 * 187-238), for batches of arrivals: one FIFO per (partition, origin DC), every queued transaction gated
 * on its partition's vectorclock.  A call leaves the queues and clocks, and returns the deliveries, that
 * serving the batch one arrival at a time in batch order gives (tests/depsim.py restates the reference):
 * an arrival is pushed to its queue, then rounds visit the DCs in `order`, storing each queue's heads
 * while they pass (a ping always passes; a transaction passes when clock[own_dc := now][dc := 0] >=
 * snapshot[dc := 0]; a pass sets clock[dc] = timestamp, a failing head sets clock[dc] = timestamp - 1,
 * both sets, not maxima) until a round stores nothing.  Where the reference leaves a choice open:
 * `order` is given at create (NULL = ascending) where the reference folds over dict:fetch_keys/1; one
 * `now` (microseconds) holds for every arrival of a call; the clock matrix in HBM is always current
 * where update_clock/3 publishes every 100 ms; a non-ping transaction with timestamp 0 is invalid
 * (timestamp - 1 has no u64 form); n_tx == 0 changes nothing.
 * The state lives in HBM and is sized by am_dep_create / am_dep_reserve only: cap_queued entries over
 * all queues.  AM_ERR_INVALID (*bad says why: a partition or DC out of range, timestamp 0 on a
 * transaction; also n_tx >= 2^32 or cap_out < queued + n_tx) and AM_ERR_CAPACITY (queued + n_tx >
 * cap_queued, decided on the host before any kernel) leave queues, clocks and outputs untouched.
 * The struct lives in host memory; am_dep_deliver takes device columns and outputs and leaves its work
 * on the context's stream except for one readback of a status block (validity bits, *n_delivered, the
 * new queued count); am_dep_deliver_host takes host columns and outputs and blocks.  Delivered non-ping
 * transactions' tags come back partition-major: partition p's are out_tag[out_off[p] .. out_off[p+1]),
 * in delivery order. */
typedef struct am_dep am_dep;
typedef struct am_dep_txns {          /* arrivals, in the order handle_transaction/1 receives them */
  uint64_t n_tx;
  const uint32_t *part;               /* [n_tx] partition index < n_part                         */
  const uint8_t  *dc;                 /* [n_tx] origin DC index (#interdc_txn.dcid)              */
  const uint64_t *timestamp;          /* [n_tx]                                                  */
  const uint64_t *snap_vc;            /* [n_tx][n_dc] transaction-major, as am_commits.snap_vc;
                                         a DC absent from the snapshot goes in as 0 (ge reads a
                                         missing entry as 0: the two are the same to try_store)  */
  const uint8_t  *ping;               /* [n_tx] or NULL = none: 1 = log_records == []            */
  const uint64_t *tag;                /* [n_tx] the caller's handle, returned on delivery        */
} am_dep_txns;
#define AM_DEP_BAD_PART 0x1u
#define AM_DEP_BAD_DC   0x2u
#define AM_DEP_BAD_TIME 0x4u          /* timestamp 0 on a transaction that is not a ping */
/* n_dc in 1..32, own_dc < n_dc, n_part >= 1, cap_queued in 1..2^30, order [n_dc] a permutation of the
 * DC indices or NULL: anything else is AM_ERR_INVALID. */
int am_dep_create(am_ctx *ctx, uint32_t n_dc, uint32_t own_dc, uint32_t n_part, uint64_t cap_queued,
                  const uint8_t *order, am_dep **out);
int am_dep_destroy(am_dep *dep);
/* A new capacity (besides create the only call that allocates queue memory): new buffers are filled, the
 * stream is synchronized, then the old buffers are freed.  AM_ERR_INVALID below the queued count.
 * Blocks.  The clock matrix does not move. */
int am_dep_reserve(am_dep *dep, uint64_t cap_queued);
/* set_dependency_clock: partition part's clock becomes host_vc [n_dc] with the presence bits pres.  Blocks. */
int am_dep_set_clock(am_dep *dep, uint32_t part, const uint64_t *host_vc, uint32_t pres);
int am_dep_set_drop_ping(am_dep *dep, int on);
/* A vnode restart (init/1, :88-90): every queue emptied, every clock new; drop_ping and the capacity stay.
 * Frees nothing.  Blocks. */
int am_dep_clear(am_dep *dep);
/* dev_out_off [n_part + 1], dev_out_tag [cap_out], cap_out >= queued + n_tx; bad may be NULL. */
int am_dep_deliver(am_dep *dep, const am_dep_txns *dev, uint64_t now, uint64_t cap_out, uint64_t *dev_out_off,
                   uint64_t *dev_out_tag, uint64_t *n_delivered, uint32_t *bad);
int am_dep_deliver_host(am_dep *dep, const am_dep_txns *host, uint64_t now, uint64_t cap_out, uint64_t *host_out_off,
                        uint64_t *host_out_tag, uint64_t *n_delivered, uint32_t *bad);
/* Device pointers to the clock matrix [n_part][n_dc] and the presence words [n_part], the layout
 * am_gst_local_min takes: borrowed, valid until destroy, not moved by reserve; an absent entry holds 0.
 * Calls on the same context stream are ordered. */
int am_dep_clocks(am_dep *dep, const uint64_t **part_vc, const uint32_t **part_pres);
/* Test accessors, both block: one partition's clock to host memory; the queued tags of one (partition,
 * DC), oldest first, to the host array tag [cap] (*n = their number; AM_ERR_CAPACITY when cap is
 * smaller: the array is not written). */
int am_dep_clock_host(am_dep *dep, uint32_t part, uint64_t *vc, uint32_t *pres);
int am_dep_queue(am_dep *dep, uint32_t part, uint32_t dc, uint64_t cap, uint64_t *tag, uint64_t *n);
int am_dep_size(am_dep *dep, uint64_t *queued, uint64_t *cap_queued);
/* status-block readbacks of am_dep_deliver since create */
int am_dep_stats(am_dep *dep, uint64_t *readbacks);

/* ---- remote ordering: the subscriber buffer of every partition a GPU owns (am_sub.hip) ----
 * One inter_dc_sub_buf state machine per (partition, origin DC) stream (src/inter_dc_sub_buf.erl:57-162,
 * src/inter_dc_sub_vnode.erl:84-94), for batches of arrivals: what produces the order in which
 * inter_dc_dep_vnode:handle_transaction/1 -- am_dep_deliver -- receives transactions.  A stream holds
 * last_observed_opid, a mode (normal | buffering) and a FIFO.  A call leaves the streams, and returns the
 * outputs, that serving the batch's rows one at a time in batch order gives (tests/subsim.py restates
 * the reference):
 *   AM_SUB_TXN       {txn, Txn}: pushed; in normal mode process_queue/1 then runs
 *   AM_SUB_RESP_TXN  one transaction of a {log_reader_resp, Txns}: in buffering mode delivered at once,
 *                    uncompared; in normal mode not delivered and counted as unexpected
 *   AM_SUB_RESP_END  ends a response (an empty response is a lone RESP_END; the row's transaction
 *                    columns are ignored): in buffering mode last := the queue head's prev_opid (unchanged
 *                    when the queue is empty), then process_queue/1; in normal mode counted as unexpected
 * process_queue/1 compares the head's prev_opid with last: equal delivers (last := last_opid; for a ping
 * prev_opid, whatever the last_opid column holds), smaller drops a duplicate, greater emits the gap
 * (part, dc, last + 1, prev_opid) and sets buffering -- or, when the DC is not in the reachable mask,
 * stays normal with the head kept for the stream's next TXN row, or, with logging disabled, delivers.
 * Where the reference leaves a choice open: a stream starts at last = 0 (am_sub_set_last loads what
 * request_op_id/3 returned); query/3's outcome is the reachable mask (default: every DC);
 * logging_enabled is read at create; a TXN / RESP_TXN row that is not a ping with timestamp 0 makes the
 * batch invalid (am_dep could not take it); n_rows == 0 changes nothing.
 * The state lives in HBM and is sized by am_sub_create / am_sub_reserve only.  AM_ERR_INVALID (*bad says
 * why; also n_rows >= 2^31, cap_out < queued + n_rows, cap_gaps < n_rows) and AM_ERR_CAPACITY (queued +
 * n_rows > cap_queued, decided on the host before any kernel) leave streams, queues and outputs
 * untouched.  The structs live in host memory; the device calls take device columns and leave their
 * work on the context's stream except for one readback of a status block (validity bits and the five
 * counters); the _host calls take host columns and block. */
typedef struct am_sub am_sub;
typedef struct am_sub_rows {          /* rows in arrival order */
  uint64_t n_rows;
  const uint8_t  *kind;               /* [n] AM_SUB_TXN | AM_SUB_RESP_TXN | AM_SUB_RESP_END              */
  const uint32_t *part;               /* [n] partition index < n_part                                   */
  const uint8_t  *dc;                 /* [n] origin DC index < n_dc                                     */
  const uint64_t *prev_opid;          /* [n] #interdc_txn.prev_log_opid#op_number.local                 */
  const uint64_t *last_opid;          /* [n] inter_dc_txn:last_log_opid/1's local; ignored for a ping   */
  const uint64_t *timestamp;          /* [n] carried for am_dep                                         */
  const uint64_t *snap_vc;            /* [n][n_dc] as am_dep_txns.snap_vc                               */
  const uint8_t  *ping;               /* [n] or NULL = none: 1 = log_records == []                      */
  const uint64_t *tag;                /* [n] the caller's handle                                        */
} am_sub_rows;
typedef struct am_sub_gaps {          /* [cap_gaps] each: the ranges to ask the origin's log reader for */
  uint32_t *part;
  uint8_t  *dc;
  uint64_t *from, *to;
} am_sub_gaps;
#define AM_SUB_TXN 0
#define AM_SUB_RESP_TXN 1
#define AM_SUB_RESP_END 2
#define AM_SUB_BAD_PART 0x1u
#define AM_SUB_BAD_DC   0x2u
#define AM_SUB_BAD_TIME 0x4u          /* timestamp 0 on a TXN / RESP_TXN row that is not a ping */
#define AM_SUB_BAD_KIND 0x8u
#define AM_SUB_NORMAL 0
#define AM_SUB_BUFFERING 1
/* counts[5] of a call */
#define AM_SUB_N_DELIVERED 0
#define AM_SUB_N_GAPS 1
#define AM_SUB_N_DROPPED 2
#define AM_SUB_N_UNEXPECTED 3
#define AM_SUB_N_QUEUED 4             /* the new total over all queues */
/* n_dc in 1..32, n_part >= 1, cap_queued in 1..2^30: anything else is AM_ERR_INVALID. */
int am_sub_create(am_ctx *ctx, uint32_t n_dc, uint32_t n_part, uint64_t cap_queued, int logging_enabled, am_sub **out);
int am_sub_destroy(am_sub *sub);
/* A new capacity (besides create the only call that allocates queue memory).  AM_ERR_INVALID below the
 * queued count.  Blocks. */
int am_sub_reserve(am_sub *sub, uint64_t cap_queued);
/* A vnode restart: every queue emptied, every stream at last = 0 in normal mode; the reachable mask,
 * logging_enabled and the capacity stay.  Frees nothing.  Blocks. */
int am_sub_clear(am_sub *sub);
/* last_observed_opid of one stream (what request_op_id/3 returned after a restart).  Blocks. */
int am_sub_set_last(am_sub *sub, uint32_t part, uint32_t dc, uint64_t opid);
/* bit d: query/3 to DC d answers ok */
int am_sub_set_reachable(am_sub *sub, uint32_t dc_mask);
/* Delivered transactions come back partition-major as the columns of am_dep_txns: partition p's are
 * entries [out_off[p], out_off[p+1]), ordered by the row that triggered the delivery, then by queue
 * order.  dev_out_off [n_part + 1]; dev_out: the caller's columns of cap_out >= queued + n_rows entries
 * (n_tx is ignored, a NULL column is skipped); the gaps in triggering-row order, cap_gaps >= n_rows;
 * counts [5] (host); bad may be NULL. */
int am_sub_process(am_sub *sub, const am_sub_rows *dev, uint64_t cap_out, uint64_t *dev_out_off, const am_dep_txns *dev_out,
                   uint64_t cap_gaps, const am_sub_gaps *dev_gaps, uint64_t *counts, uint32_t *bad);
int am_sub_process_host(am_sub *sub, const am_sub_rows *host, uint64_t cap_out, uint64_t *host_out_off,
                        const am_dep_txns *host_out, uint64_t cap_gaps, const am_sub_gaps *host_gaps, uint64_t *counts,
                        uint32_t *bad);
/* am_sub_process into library scratch, then am_dep_deliver on those device columns: the transactions
 * never visit the host.  All or nothing: before any kernel, sub and dep must share the context, n_part
 * and n_dc (AM_ERR_INVALID), dep.queued + sub.queued + n_rows must fit dep's cap_queued
 * (AM_ERR_CAPACITY) and cap_out must reach that bound (AM_ERR_INVALID).  The outputs are
 * am_dep_deliver's (dev_out_off [n_part + 1], dev_out_tag [cap_out], *n_delivered by am_dep) and this
 * buffer's gaps and counts. */
int am_sub_deliver(am_sub *sub, am_dep *dep, const am_sub_rows *dev, uint64_t now, uint64_t cap_out, uint64_t *dev_out_off,
                   uint64_t *dev_out_tag, uint64_t *n_delivered, uint64_t cap_gaps, const am_sub_gaps *dev_gaps,
                   uint64_t *counts, uint32_t *bad);
int am_sub_deliver_host(am_sub *sub, am_dep *dep, const am_sub_rows *host, uint64_t now, uint64_t cap_out,
                        uint64_t *host_out_off, uint64_t *host_out_tag, uint64_t *n_delivered, uint64_t cap_gaps,
                        const am_sub_gaps *host_gaps, uint64_t *counts, uint32_t *bad);
/* Test accessor: one stream's last_observed_opid, mode (AM_SUB_NORMAL | AM_SUB_BUFFERING) and queued
 * tags, oldest first, to the host array tag [cap] (*n = their number; AM_ERR_CAPACITY when cap is
 * smaller: the array is not written).  Blocks. */
int am_sub_stream(am_sub *sub, uint32_t part, uint32_t dc, uint64_t *last, uint32_t *mode, uint64_t cap, uint64_t *tag,
                  uint64_t *n);
int am_sub_size(am_sub *sub, uint64_t *queued, uint64_t *cap_queued);
/* status-block readbacks of am_sub_process / am_sub_deliver since create */
int am_sub_stats(am_sub *sub, uint64_t *readbacks);

/* ---- op-cache ingestion + garbage collection ----
 * Builds a new store from `st` (st is unchanged; destroy it when no read uses it):
 *   1. prune_ops/2 (src/materializer_vnode.erl:565-604): for keys with prune_mask[k] != 0
 *      only ops with materializer:belongs_to_snapshot_op(Thr_k, CommitTime, SnapshotTime)
 *      (src/materializer.erl:102-106) survive, in order, keeping their op ids;
 *   2. op_insert_gc/3 (:622-647): the ops of dev_new (CSR over the same keys, oldest ->
 *      newest; its op_id column is ignored) are appended with ids OpCounter+1, +2, ...
 * Either step may be skipped (dev_new / prune_mask NULL).  Device pointers: prune_mask
 * [n_keys], thr_vc [n_dc][n_keys], thr_pres [n_keys]; gc_flags [n_keys] (or NULL) receives
 * AM_GC_* per key.  Differences from the ETS tuple: no ListLen sizing (the log is exactly
 * sized), and a key whose ops are all pruned keeps 0 ops (flag AM_GC_PRUNED_ALL) where
 * prune_ops keeps element(FIRST_OP+Len), a 0 placeholder (:580-583).  Blocks. */
#define AM_GC_PRUNED_ALL 0x1u  /* check_filter kept nothing (NewSize == 0, :580), empty logs too */
#define AM_GC_TRIGGER 0x2u     /* some NewId rem OPS_THRESHOLD == 0: op_insert_gc would have
                                  run a GC read (:635) -- the caller's cue to prune next    */
#define AM_OPS_THRESHOLD 50    /* src/materializer_vnode.erl:41 */
int am_store_update(am_ctx *ctx, const am_store *st, const am_op_log *dev_new, const uint8_t *prune_mask,
                    const uint64_t *thr_vc, const uint32_t *thr_pres, uint8_t *gc_flags, am_store **out);

/* In-place ingestion + GC (the vnode's path; src/materializer_vnode.erl:515-647 per touched key).
 * am_store_reserve: a copy of st whose keys have room for appends (key_end / rec_key_end set: a
 * quarter of each key's ops and at least 4 free op slots, variable words and records in
 * proportion), the ETS tuple's ListLen slack (:540-560).  Blocks.
 * am_store_apply: on a store with room, the same prune + append as am_store_update, for the
 * n_touched keys keys[] (device, distinct) only, written into their room in place: dev_new is
 * CSR over the n_touched keys (entry i = keys[i]; or NULL), prune_mask / thr_vc / thr_pres are
 * over the store's n_keys as in am_store_update (or NULL), gc_flags [n_touched] (device, or
 * NULL) receives AM_GC_*.  Cost O(the touched keys' ops).  *applied = 0 when some touched key
 * would outgrow its room (or the store has none): nothing is written, and the caller rebuilds
 * with am_store_update (+ am_store_reserve).  Readers of the store must not run concurrently
 * (the context lock serializes library calls).  Blocks.  A call that fails (AM_ERR_INVALID: a
 * touched key outside the store or repeated) writes nothing into the store; gc_flags is then
 * unspecified. */
int am_store_reserve(am_ctx *ctx, const am_store *st, am_store **out);
int am_store_apply(am_ctx *ctx, am_store *st, uint64_t n_touched, const uint64_t *keys, const am_op_log *dev_new,
                   const uint8_t *prune_mask, const uint64_t *thr_vc, const uint32_t *thr_pres, uint8_t *gc_flags,
                   int *applied);

/* ---- GST (global stable time) ---- */
/* lanes[0..n_dc-1] = per-DC min over the partitions that have the DC (absent = UINT64_MAX);
 * if any partition is undefined every present lane is 0 (get_min_time's rule);
 * lanes[n_dc] = 1 (defined).  Device pointers: part_vc [n_part][n_dc] (partition-major),
 * part_pres [n_part], part_undef [n_part] (or NULL). */
int am_gst_local_min(am_ctx *ctx, uint32_t n_dc, uint32_t n_part, const uint64_t *part_vc,
                     const uint32_t *part_pres, const uint8_t *part_undef, uint64_t *lanes);
/* RCCL communicator (one process per GPU). */
int am_comm_unique_id(void *id_out /* 128 bytes */);
int am_comm_init(am_ctx *ctx, int rank, int nranks, const void *id /* 128 bytes */, am_comm **out);
int am_comm_destroy(am_comm *comm);
/* In place element-wise min of n_dc+1 u64 lanes across ranks (ncclMin/ncclUint64). */
int am_gst_allreduce(am_comm *comm, uint64_t *lanes, uint32_t n_dc);
/* Turn merged lanes into the stable snapshot: undefined => present lanes 0; then the
 * monotone update against last (last_vc/last_pres device, updated in place);
 * gr != 0 additionally replicates the min over present DCs to every present DC
 * (the value a reader gets from get_stable_snapshot/0).  out_vc/out_pres receive the
 * snapshot a reader would use; changed (device u8) = update_stable's Bool. */
int am_gst_finalize(am_ctx *ctx, uint32_t n_dc, const uint64_t *lanes, uint64_t *last_vc,
                    uint32_t *last_pres, int gr, uint64_t *out_vc, uint32_t *out_pres,
                    uint8_t *changed);

/* CPU twins of am_gst_local_min / the all-reduce's element-wise min / am_gst_finalize, compiled
 * from the same per-DC code as the kernels (am_gst.hip): host pointers, no device.  A node
 * whose GST merge runs on the host (and the multi-process tests, which exchange lanes over
 * gloo) gets the device path's exact encoding and rules. */
int am_gst_local_min_host(uint32_t n_dc, uint32_t n_part, const uint64_t *part_vc, const uint32_t *part_pres,
                          const uint8_t *part_undef, uint64_t *lanes);
int am_gst_merge_lanes_host(uint32_t n_dc, const uint64_t *in, uint64_t *inout);  /* inout = min(in, inout), n_dc+1 lanes */
int am_gst_finalize_host(uint32_t n_dc, const uint64_t *lanes, uint64_t *last_vc, uint32_t *last_pres, int gr,
                         uint64_t *out_vc, uint32_t *out_pres, uint8_t *changed);

/* ---- sharding ---- */
/* 0-based partition position for integer keys: abs(K) rem n_partitions. */
uint32_t am_key_partition(int64_t key, uint32_t n_partitions);
/* The same for keys passed as bytes (log_utilities:convert_key/1, src/log_utilities.erl:
 * 100-118): AM_KEY_BINARY -- the key is a binary; its text, if list_to_integer accepts it
 * ([+-]?[0-9]+, any length), gives abs(Int) rem n, else the SHA-1 chash_key path;
 * AM_KEY_TERM -- bytes = term_to_binary(Key) of a key that is neither an integer nor a
 * binary (chash_key({?BUCKET, term_to_binary(Key)})).  chash_key(B) = SHA-1 of
 * term_to_binary({<<"antidote">>, B}); crypto:bytes_to_integer of it rem n. */
#define AM_KEY_BINARY 0
#define AM_KEY_TERM 1
uint32_t am_key_partition_bytes(const uint8_t *bytes, uint64_t len, int kind, uint32_t n_partitions);
/* riak_core_util:chash_key({<<"antidote">>, B}) for a binary B: 20-byte SHA-1 digest */
int am_chash_key(const uint8_t *bytes, uint64_t len, uint8_t out[20]);

/* ---- term codec (am_codec.hip) ----
 * Order-preserving interning of Erlang terms (external term format, enif_term_to_binary)
 * into the u64 LABELS the device holds for LWW values, MV values and tokens, and add-wins-set
 * elements and tokens: label order == Erlang term order, so the device's sorted outputs are
 * the reference's orddict order, and am_codec_term turns labels back into terms.  One codec
 * per partition (or node); thread-safe.  Labels lie in [1, 2^64-2].  Supported terms:
 * integers, floats, atoms, tuples, lists (proper and improper), binaries and bitstrings;
 * maps, pids, ports, references and funs give AM_ERR_UNSUPPORTED.  Terms that compare equal
 * (1 and 1.0) share one label.
 * When a call needs room that the label space no longer has between two neighbours, every
 * label is re-spread (order kept) and *relabeled is set: take the old -> new map with
 * am_codec_take_relabel and apply it with am_store_relabel / am_snapcache_relabel /
 * am_vnode_relabel to every structure holding labels BEFORE putting this call's labels on
 * the device.  Until the map is taken, am_codec_intern fails with AM_ERR_INVALID. */
typedef struct am_codec am_codec;
#define AM_CODEC_ABSENT 1 /* am_codec_lookup: the term was never interned */
int am_codec_create(am_codec **out);
int am_codec_destroy(am_codec *c);
int am_codec_intern(am_codec *c, uint64_t n, const uint8_t *const *terms, const uint64_t *lens, uint64_t *labels,
                    int *relabeled);
int am_codec_lookup(am_codec *c, const uint8_t *term, uint64_t len, uint64_t *label);
/* the term of a label (external term format); *len always set; AM_ERR_CAPACITY if cap < len */
int am_codec_term(am_codec *c, uint64_t label, uint8_t *buf, uint64_t cap, uint64_t *len);
uint64_t am_codec_size(am_codec *c);
/* pending relabel map, old labels increasing; old/new NULL: *n = its size only */
int am_codec_take_relabel(am_codec *c, uint64_t *old_labels, uint64_t *new_labels, uint64_t cap, uint64_t *n);
/* Erlang term order of two encoded terms: *out = -1, 0, 1 */
int am_codec_compare(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb, int *out);
/* apply a relabel map (host arrays from am_codec_take_relabel) in place: the store's LWW
 * values, MV values and tokens, AW elements and tokens, and its token-group view */
int am_store_relabel(am_ctx *ctx, am_store *st, const uint64_t *old_labels, const uint64_t *new_labels, uint64_t n);
/* the same for a snapshot cache: LWW values and the set pairs in the value pool; key_type is
 * the device key-type column of the store the cache serves ([n_keys]) */
int am_snapcache_relabel(am_ctx *ctx, am_snapcache *c, const uint8_t *key_type, const uint64_t *old_labels,
                         const uint64_t *new_labels, uint64_t n);
/* both, for a vnode's ops cache and snapshot cache */
int am_vnode_relabel(am_vnode *v, const uint64_t *old_labels, const uint64_t *new_labels, uint64_t n);

/* ---- transaction ids (am_txid.hip) ----
 * is_op_in_snapshot/7 compares TxIds for equality only: TxId == Op#clocksi_payload.txid
 * (src/clocksi_materializer.erl:232).  #tx_id{local_start_time, server_pid}
 * (include/antidote.hrl:192-195) holds a pid, so TxIds are NOT labelled by the ordered codec:
 * am_txid_intern maps the external term format of a TxId (enif_term_to_binary, pids, ports and
 * references included) to a dense u64 id, the op_txid / am_read_batch.txid words.  Every
 * encoding of one term gets one id (the bytes are canonicalised first); ids start at 1, are
 * never reordered, relabeled or reused.  am_txid_forget drops an ended transaction's entry.
 * Thread-safe.  Maps and funs: AM_ERR_UNSUPPORTED.
 * Lifetime: a reader's TxId (am_txid_intern) is HELD until am_txid_forget; an op's TxId
 * (am_txid_intern_op, stamped with the op's commit_time {DcId, CT}, DcId as a DC index) is
 * dropped by am_txid_expire once the stable snapshot covers CT and no reader holds it -- the
 * transaction has committed everywhere, so no live read carries it (ops replicated from other
 * DCs, whose TxIds no local coordinator forgets, leave the map this way).  Replaces the
 * #clocksi_payload.txid bookkeeping of materializer_vnode:update/2 (src/materializer_vnode.erl:106-110)
 * and the TxId test of is_op_in_snapshot/7 (src/clocksi_materializer.erl:232). */
typedef struct am_txids am_txids;
int am_txid_create(am_txids **out);
int am_txid_destroy(am_txids *t);
int am_txid_intern(am_txids *t, const uint8_t *term, uint64_t len, uint64_t *id);
int am_txid_intern_op(am_txids *t, const uint8_t *term, uint64_t len, uint32_t dc, uint64_t ct, uint64_t *id);
/* AM_CODEC_ABSENT when the TxId was never interned (or was forgotten / expired) */
int am_txid_lookup(am_txids *t, const uint8_t *term, uint64_t len, uint64_t *id);
int am_txid_forget(am_txids *t, const uint8_t *term, uint64_t len);
/* drop the unheld op entries whose commit time the stable snapshot (stable_vc[n_dc], presence
 * bits stable_pres: the GST, stable_time_functions:get_min_time/1) covers; *dropped (or NULL) */
int am_txid_expire(am_txids *t, uint32_t n_dc, const uint64_t *stable_vc, uint32_t stable_pres, uint64_t *dropped);
uint64_t am_txid_size(am_txids *t);
/* the canonical encoding the map keys on (131-prefixed); *out_len always set */
int am_txid_canonical(const uint8_t *term, uint64_t len, uint8_t *buf, uint64_t cap, uint64_t *out_len);

/* ---- synthetic op logs (bench + parity; counter-based, regenerable per key) ---- */
typedef struct am_synth_params {
  uint64_t seed;
  uint64_t n_keys;
  uint32_t ops_per_key;  /* uniform log length (ignored when zipf_milli != 0)  */
  uint32_t n_dc;
  uint32_t type;         /* am_type, or 0 for mixed (40/20/20/20 PN/LWW/AW/MV),
                            or 6 for MV register + bounded counter (50/50)    */
  uint32_t key_base;     /* global index of key 0 (for sharding)               */
  uint32_t max_lag;      /* snapshot lag in ops (concurrency window)           */
  uint32_t zipf_milli;   /* Zipf exponent x1000 for key popularity; 0 = uniform */
  uint64_t total_ops;    /* Zipf: target total ops over all keys               */
  uint32_t hot_cap;      /* Zipf: cap on one key's log length                  */
  uint32_t universe;     /* AW-set element universe per key (power of two)     */
  uint64_t part_mask;    /* 0: local key k is global key key_base + k.  Else the
                            riak_core partitions (of 64) this GPU owns: local key
                            k is the k-th integer key >= key_base whose partition
                            am_key_partition(key, 64) = key mod 64 is in the mask */
  uint32_t esc_ppm;      /* ops (per 10^6) whose snapshot_time holds one remote DC's entry
                            2^33 us behind: outside the packed view's window (escaped ops) */
  uint32_t gst_ppm;      /* keys (per 10^6) whose ops carry the reference's stable-snapshot cadence:
                            remote entries 0.1-1.2 s behind the commit, in 1 s steps (synth.h
                            am_syn_snap_g); 0: every entry trails its commit by milliseconds */
} am_synth_params;
#define AM_SYNTH_MV_BC 6
/* Device log owned by the returned store. */
int am_synth_store(am_ctx *ctx, const am_synth_params *p, am_store **out);
/* The read clock the generator's quantile q selects (q in [0,1]); host output [n_dc]. */
int am_synth_read_clock(const am_synth_params *p, double q, uint64_t *out_vc);
/* The global key of local key k (see part_mask). */
uint64_t am_synth_key(const am_synth_params *p, uint64_t k);
/* Regenerate keys [k0, k0+nk) on the host into caller buffers sized by
 * am_synth_host_sizes (for parity checks against the oracle). */
int am_synth_host_sizes(const am_synth_params *p, uint64_t k0, uint64_t nk, uint64_t *n_ops,
                        uint64_t *n_var);
int am_synth_host(const am_synth_params *p, uint64_t k0, uint64_t nk, am_op_log *out_host_bufs);

#ifdef __cplusplus
}
#endif
#endif /* ANTIDOTE_MAT_H */
