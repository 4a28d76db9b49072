// am_group_split.h -- the split fresh read of the token-group wave tier: k_grp_incl (op stream ->
// inclusion bitmap + scalar outputs), then one record pass (k_grp_spans over the group-span view,
// or k_grp_recs over the records), and their launcher.  Part of am_group.h, which includes it
// after the wave-tier definitions it uses (GMeta / read_meta, wave_takes, VG, VWORDS).
#pragma once

namespace amk_grp {

// ---------------------------------------------------------------- split fresh read, pass 1
// A fresh read (the batch clock, no base, no TxId; packed view, no zone index) in two passes:
// k_grp_incl streams the read's commit vectors -- 256-op tiles, one 16-byte load per DC and lane,
// the wave's only live state the tile and the partials -- and writes its inclusion bits into the
// global bitmap ibm (bit p = op slot p) and its scalar outputs {NewLastOp, LastOpCt, IsNewSS,
// Count, status}; k_grp_spans (k_grp_recs for a log without the span view) then reads the groups'
// spans (records) against those bits and gathers the survivors.  A wave takes 32 CONSECUTIVE
// reads at a time and their scalar outputs leave through LDS as one coalesced store per column
// (single-lane stores of reads far apart write partial lines of the output columns, each line
// written back once per writer).  Ops outside the streamed view (escaped ops, rare) are evaluated
// once per batch, after its reads' tile loops: a read that met any leaves its lanes' escape marks
// in a scratch row (escr: 512 bytes per read slot of the wave, written for such reads only) and
// its in-view partials in the LDS rows, and the deferred phase ORs the included escaped ops into
// the bitmap and merges their partials in before the outputs are derived.
constexpr uint32_t IWB = 32;  // reads per wave batch
__device__ __forceinline__ uint32_t wave_min_u32_v(uint32_t v) {
#define S_(C) v = min(v, dpp32<C>(v));
  AMK_ROW_STEPS(S_)
#undef S_
  v = min(v, (uint32_t)__shfl_xor((int)v, 16, WAVE));
  return min(v, (uint32_t)__shfl_xor((int)v, 32, WAVE));
}
// A read's slot: where its ops and outputs are, and its set-up (am_iw_read_setup, am_inclwin.h) --
// the packed thresholds and, for the lag instantiation, the key's lag bases and the window's
// limits -- computed by the batch's lane j for read j, 32 reads in one pass and their keys' lag
// bases in one load latency, and read back wave-uniform when the wave comes to the read.
constexpr uint32_t SLOT_NEVER = 1u, SLOT_MISS = 2u;  // fl: PkRead::never, PkRead::miss != 0
constexpr uint32_t SLOT_LW_SHIFT = 16;  // fl's upper half (LAG): the key's lag width, for the read loop's raise
struct ISlotHead {
  uint64_t off0, K, idb;
  uint32_t r, nops;
};
template <int DMAX, bool LAG>
struct alignas(16) ISlot : ISlotHead {
  uint32_t thr[DMAX];
  uint32_t fl;
};
template <int DMAX>
struct alignas(16) ISlot<DMAX, true> : ISlotHead {
  uint32_t thr[DMAX];
  uint32_t lb[DMAX];
  uint32_t lbm, cin_lim, out_lim, fl;  // (lbm: the int32 in u32)
};
constexpr int SEGT = 4;               // 256-op tiles per segment of the lag instantiation
constexpr uint32_t SEGOPS = SEGT * 256;  // ops per segment, and the most entries of its window list
// per-lane LastOpCt maxima, transposed for the reduction; the lag instantiation's window list (u16
// op indices within the segment, newest first) lives in the same bytes -- the maxima are written
// when the list is done -- next to the segment's staged bitmap words
template <int DMAX, bool LAG>
struct ISred {
  uint32_t mx[DMAX][WAVE];
};
template <int DMAX>
struct ISred<DMAX, true> {
  union {
    uint32_t mx[DMAX][WAVE];
    uint16_t list[SEGOPS];
  };
  uint32_t stage[SEGOPS / 32];
};
template <int DMAX, bool LAG>
struct ISmem : ISred<DMAX, LAG> {
  ISlot<DMAX, LAG> slot[IWB];
  // the batch's partials, by read: the in-view values as the tile loop leaves them, then merged
  // with the escaped ops' (the deferred phase); the outputs are derived from them once, as the
  // batch leaves
  uint32_t ct[DMAX][IWB];       // the in-view LastOpCt maxima above the slot's K (u32, as the view's
                                // entries; FLAG_INVIEW: any), not yet masked by the presence.  The
                                // escaped ops' maxima are 64-bit and rare: they wait in the read's
                                // scratch row (escr) and are merged as the columns are stored
  uint64_t mex[IWB];            // the first excluded op's slot (NONE: none)
  uint32_t count[IWB], pres[IWB];
  uint32_t flags[IWB];          // with FLAG_BAD and FLAG_INVIEW
};
constexpr uint32_t FLAG_INVIEW = 0x200u;  // the read included an op of the streamed view: ct holds its maxima

// ops [g, g + OPL) of the lane (OPL consecutive slots, g OPL-aligned), their entries x those of
// the packed view (pk_ent) or rebuilt from the lag view where they are used (lag_ent, am_wave.h):
// inclusion bits (is_op_in_snapshot/7 against the batch clock: every entry X[d] - K <= S[d] - K)
// and the partials.  RANGE: the tile may hold slots outside [off0, off1); escaped ops
// (x.esc(k) == AM_PK_ESC) are left to the caller (esc bit k).
template <int DMAX, int OPL, bool RANGE, class Ent>
__device__ __forceinline__ uint32_t incl_tile(const Ent &x, const PkRead<DMAX> &pk, uint64_t g, uint64_t off0,
                                              uint64_t off1, uint32_t (&mx)[DMAX], uint32_t &esc, uint32_t &cand) {
  uint32_t ib = 0;
#pragma unroll
  for (int k = 0; k < OPL; ++k) {
    const bool e = x.esc(k) == AM_PK_ESC;
    const bool inr = !RANGE || (g + k >= off0 && g + k < off1);
    bool in = inr && !e;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) in = in && x(k, d) <= pk.thr[d];
    esc |= (uint32_t)(inr && e) << k;
    cand |= (uint32_t)(inr && !e) << k;
    if (in) {
#pragma unroll
      for (int d = 0; d < DMAX; ++d) mx[d] = max(mx[d], x(k, d));
    }
    ib |= (uint32_t)in << k;
  }
  return ib;
}

// the per-lane maxima a wave left in smx (transposed, synced) -> lane l: DC (l & 7)'s maximum.
// Lane 8 d + c takes DC d's entries of lanes 8 c .. 8 c + 7, then an 8-lane max.
template <int DMAX>
__device__ __forceinline__ uint32_t mx_reduce(const uint32_t (*smx)[WAVE], uint32_t lane) {
  uint32_t m = 0;
  {
    const uint32_t d = lane >> 3, c = lane & 7u;
    if (d < (uint32_t)DMAX) {
      const u32x4 a0 = *(const u32x4 *)&smx[d][8 * c], a1 = *(const u32x4 *)&smx[d][8 * c + 4];
      m = max(max(max(a0.x, a0.y), max(a0.z, a0.w)), max(max(a1.x, a1.y), max(a1.z, a1.w)));
    }
    // lanes ^ 1, ^ 2, then the other quad of the eight (row_half_mirror): no lane addresses,
    // which the compiler would compute once per batch and hold across the tile loop
    m = max(m, dpp32<0xB1>(m));
    m = max(m, dpp32<0x4E>(m));
    m = max(m, dpp32<0x141>(m));
  }
  // from lane 8 d (its address from the opaque lane number, for the same reason)
  uint32_t ql = lane;
  asm volatile("" : "+v"(ql));
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ql & 7u) << 5), (int)m);
}

// LAG: the read streams the lag view (am_op_log.lag_ct / lag / key_lag, 4 + 2 D bytes per op)
// and rebuilds each packed entry X[d] - K = lag_ct - key_lag[d] - lag[d] in u32 (exact: the entry
// fits u32 for every op the view holds); else the packed view (4 D bytes per op)
//
// The lag instantiation does not evaluate the window ops (am_inclwin.h) in the tile loop, densely
// and per tile: a segment of four tiles is classified from its commit words alone, its window ops
// are compacted into a per-wave LDS list and evaluated in rounds of 64, one op per lane (a 4-byte
// and nd 2-byte gathers per op), their bits ORed into bitmap words staged in LDS.  A C3 read has
// ~75 window ops among 1024: two rounds instead of two dense window tiles, and one dependent step
// (commit words -> lags) instead of one per window tile.
//
// Waves per SIMD, by clock width D.  The per-read loop holds the segment loop only: escaped ops
// are evaluated after the batch's loop, where no tile state is live, and what the batch's set-up
// and outputs derive from the lane number is computed per batch (sl_, ol), so neither weighs on
// the loop's registers.  LAG (a segment's commit words, then a round's lags and the maxima):
// five waves without a vector spill at D = 8 (at six, 80 VGPRs, it spills 9-12).  Packed (the
// tile's D x 4 entries): 97 VGPRs at D = 8, four waves.  A read's set-up (thresholds, lag bases,
// window limits) is not in the loop either: the batch's lane j computes read j's into the slot.
//
// The lag instantiation takes one more argument than the packed one (X: const uint16_t *lagw, the
// store's per-key lag widths, am_internal.h am_lagw_find; null: 0xFFFF for every key).  The window
// of a read is sized by its key's width (am_inclwin.h): lane j loads it with the key's lag bases,
// so the slot's out_lim is the tight one, and the read loop takes it from the slot's fl for the
// raise without loads.  The packed instantiation's argument block is as it was.
#ifndef AM_INCL_WAVES
#define AM_INCL_WAVES(D) 4
#endif
#ifndef AM_INCL_LAG_WAVES
#define AM_INCL_LAG_WAVES(D) 5
#endif
__device__ __forceinline__ const uint16_t *incl_lagw() { return nullptr; }
__device__ __forceinline__ const uint16_t *incl_lagw(const uint16_t *p) { return p; }
template <int DMAX, int TYPE, bool EXACT, bool LAG, class... X>
__global__ void __launch_bounds__(BLOCK, LAG ? AM_INCL_LAG_WAVES(DMAX) : AM_INCL_WAVES(DMAX)) k_grp_incl(am_log_arg LA, am_read_batch B, am_read_result R, am_sel S,
                                                       am_retry next, am_retry routed, uint32_t short_opl,
                                                       uint32_t *ibm, uint64_t *escr, X... xa) {
  static_assert(sizeof...(X) == (LAG ? 1 : 0), "the lag instantiation takes the lag widths, the packed one nothing");
  const am_op_log L = LA.log();
  const uint16_t *const lagw = incl_lagw(xa...);
  constexpr int OPL = 4;
  constexpr uint64_t TILE = (uint64_t)WAVE * OPL;
  constexpr uint32_t LPW = 32 / OPL;
  __shared__ ISmem<DMAX, LAG> smem[NW];
  ISmem<DMAX, LAG> &sm = smem[threadIdx.x >> 6];
  ISlot<DMAX, LAG> *sl = sm.slot;
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t nd = EXACT ? (uint32_t)DMAX : L.n_dc;
  const uint64_t stride = L.snap_stride ? L.snap_stride : L.n_ops;
  const uint32_t sel0 = S.idx ? uniform_u32(S.range[0]) : 0u;
  const uint64_t nsel = S.idx ? (uint64_t)(uniform_u32(S.range[1]) - sel0) : B.n_reads;
  const uint64_t W = (uint64_t)gridDim.x * NW;
  const uint64_t gw = (uint64_t)blockIdx.x * NW + uniform_u32(threadIdx.x >> 6);
  const uint64_t n = B.n_reads;
  const uint32_t allmask = nd >= 32 ? 0xFFFFFFFFu : ((1u << nd) - 1u);

  for (uint64_t b0 = gw * IWB; b0 < nsel; b0 += (uint64_t)IWB * W) {
    // ---- lane j < IWB: read b0 + j -> slot j (errors and hand-offs leave here) ----
    // (sl_: the lane number, opaque to the compiler -- what the batch's set-up and outputs derive
    //  from it is computed where it is used, per batch, not once per kernel and then held in
    //  registers across the tile loop, whose budget has no room for it)
    uint32_t sl_ = lane, sopl = short_opl;  // (sopl: the same for the mask wave_takes makes of it)
    asm volatile("" : "+v"(sl_));
    asm volatile("" : "+s"(sopl));
    const uint64_t ii = b0 + sl_;
    bool elig = false, hand = false, route = false;
    uint64_t rr = 0;
    // the batch's one clock (no bases / TxIds), read per batch: the reads' set-up below is its only
    // use on this path, so it is not live across the reads' loops
    ReadU<DMAX> u;
    read_inputs<DMAX, false, true>(L, nd, B, 0, u);
    if (sl_ < IWB && ii < nsel) {
      GMeta mm;
      read_meta(L, B, S.idx ? (uint64_t)S.idx[sel0 + ii] : ii, TYPE, mm);
      rr = mm.r;
      if (mm.st != AM_OK) {
        R.status[mm.r] = mm.st, R.flags[mm.r] = 0;
      } else if (!wave_takes(L, B, mm, sopl)) {
        hand = true;
      } else if (LAG && routed.list && L.key_lag[mm.key * nd] == AM_LAG_ROUTED) {
        route = true;  // a packed-routed key: the packed instantiation's (launch_split)
      } else {
        elig = true;
        // the read's set-up, one read per lane: the clock against this key's time base and lag bases
        const uint64_t K = L.key_tbase[mm.key];
        uint32_t lbk[DMAX], thr[DMAX];
        if (LAG) {
#pragma unroll
          for (int d = 0; d < DMAX; ++d) lbk[d] = d < (int)nd ? (uint32_t)L.key_lag[mm.key * nd + d] : 0u;
        }
        const uint32_t lw = (LAG && lagw) ? (uint32_t)lagw[mm.key] : (uint32_t)AM_IW_LAG_MAX;  // the key's lag width
        am_iw_read rs;
        am_iw_read_setup_w(u.S, u.spres, u.allmask, K, LAG ? lbk : nullptr, nd, (uint32_t)DMAX, lw, thr, &rs);
        ISlot<DMAX, LAG> &w = sl[sl_];
        w.off0 = mm.off0, w.K = K, w.idb = L.key_id_base ? L.key_id_base[mm.key] : 1;
        w.r = (uint32_t)mm.r, w.nops = (uint32_t)(mm.off1 - mm.off0);
#pragma unroll
        for (int d = 0; d < DMAX; ++d) w.thr[d] = thr[d];
        w.fl = (rs.never ? SLOT_NEVER : 0u) | (rs.miss ? SLOT_MISS : 0u) | (LAG ? lw << SLOT_LW_SHIFT : 0u);
        if constexpr (LAG) {
#pragma unroll
          for (int d = 0; d < DMAX; ++d) w.lb[d] = lbk[d];
          w.lbm = (uint32_t)rs.lbm, w.cin_lim = rs.cin_lim, w.out_lim = rs.out_lim;
        }
      }
    }
    const uint64_t hm = __ballot(hand);
    if (hm) {
      uint32_t base = 0;
      if (sl_ == 0) base = atomicAdd(next.count, (uint32_t)__popcll(hm));
      base = uniform_u32(base);
      if (hand) next.list[base + (uint32_t)__popcll(hm & ((1ull << sl_) - 1ull))] = (uint32_t)rr;
    }
    if (LAG) retry_append(routed, route, (uint32_t)rr, sl_);
    const uint64_t emask = __ballot(elig);
    uint32_t escmask = 0;  // the batch's reads with escaped ops (wave-uniform): the deferred phase's
    uint64_t *const escw = escr + (gw * IWB) * WAVE;  // this wave's escape-mark rows, one per slot
    wave_sync();

    for (uint64_t em = emask; em; em &= em - 1) {
      const uint32_t j = (uint32_t)__builtin_ctzll(em);
      const uint64_t off0 = uniform_u64(sl[j].off0), off1 = off0 + uniform_u32(sl[j].nops);
      // the read's set-up, from its slot (wave-uniform): no load from memory stands before the
      // read's first commit words
      PkRead<DMAX> pk;
#pragma unroll
      for (int d = 0; d < DMAX; ++d) pk.thr[d] = uniform_u32(sl[j].thr[d]);
      const uint32_t sfl = uniform_u32(sl[j].fl);
      pk.never = (sfl & SLOT_NEVER) != 0;  // (the lag instantiation's is in its limits)
      uint32_t lb[DMAX];  // the key's lag bases (LAG)
      if constexpr (LAG) {
#pragma unroll
        for (int d = 0; d < DMAX; ++d) lb[d] = uniform_u32(sl[j].lb[d]);
      }
      uint32_t cnt = 0, minex = 0xFFFFFFFFu, anyc = 0, anyesc = 0;
      uint32_t mxr = 0;  // (LAG) lane l: DC (l & 7)'s maximum over the segments so far
      uint64_t escm = 0;  // the lane's escaped ops: bit OPL * tile + k (the first 64 / OPL tiles)
      const uint64_t t0 = off0 & ~31ull;  // 32-op aligned: lane groups of LPW fill whole bitmap words
      if constexpr (LAG) {
        static_assert(OPL == 4 && TILE == 256 && SEGOPS == SEGT * TILE, "list entries: tile, lane, op of four");
        // The commit word alone decides most ops (am_inclwin.h): only ops in the window
        // in_lim <= c < out_lim need their lags.  The read is cut into segments of SEGT tiles,
        // walked newest first (a C3 read is one segment), and a segment goes in phases:
        //  1. its commit words, all tiles in flight together; the bound without loads over the
        //     whole segment; then every op's class -- sure-IN bits into the staged words, escape
        //     marks and partials as the tile loop of the packed view leaves them;
        //  2. its window ops appended to the wave's list, newest first;
        //  3. the list in rounds, one op per lane: the op's commit word and nd u16 lags gathered,
        //     its entries rebuilt and tested, its bit ORed into the staged word, its entries folded
        //     into the lane's maxima.  Each round raises cmax from the lanes' maxima; the next
        //     round's entries are classified again first and those now IN take no loads;
        //  4. the staged words stored, the maxima reduced into mxr (lane d: DC d).
        // An older segment starts from the cmax the newer ones reached.
        // The window's state is u32 limits (am_inclwin.h): in_lim = min(cin_lim, cmax_lim), and
        // since cin_lim is fixed the running bound is kept already capped -- cmax_lim starts at 0
        // and a raise is a max, so min(cin_lim, max(in_lim, raise)) is the same value.
        const int32_t lbm = (int32_t)uniform_u32(sl[j].lbm);  // the smallest lag base: the rounds' bound in u32 above it
        const uint32_t cin_lim = uniform_u32(sl[j].cin_lim), out_lim = uniform_u32(sl[j].out_lim);
        const uint32_t lw = sfl >> SLOT_LW_SHIFT;  // the key's lag width: a sure-in op c raises the bound to c - lw
        uint32_t in_lim = 0;
        const uint32_t lo = (uint32_t)(off0 - t0), nops = (uint32_t)(off1 - off0);  // the read's ops: [lo, lo + nops) from t0
        uint16_t *const list = sm.list;
        uint32_t *const stage = sm.stage;
        const uint32_t nt = (uint32_t)((off1 - 1 - t0) / TILE) + 1u;
        for (uint32_t sg = (nt + SEGT - 1) / SEGT; sg-- > 0;) {
          const uint64_t sb = t0 + (uint64_t)sg * SEGOPS;
          const uint32_t sr = sg * SEGOPS;  // sb - t0
          // ---- 1. commit words, the bound without loads, classes ----
          uint32_t c[SEGT][OPL];
#pragma unroll
          for (int k = 0; k < SEGT; ++k) {
            const uint64_t g = sb + (uint64_t)k * TILE + (uint64_t)lane * OPL;
#pragma unroll
            for (int i = 0; i < OPL; ++i) c[k][i] = 0;
            if (g < off1) ld_n32<OPL>(L.lag_ct + g, c[k]);
          }
          if (in_lim < cin_lim) {
            uint32_t sure = 0;  // 1 + the lane's largest c <= cin (AM_PK_ESC lies above every cin_lim)
#pragma unroll
            for (int k = 0; k < SEGT; ++k)
#pragma unroll
              for (int i = 0; i < OPL; ++i) {
                const uint32_t q = sr + (uint32_t)k * (uint32_t)TILE + lane * OPL + (uint32_t)i;
                if (q - lo < nops && c[k][i] < cin_lim) sure = max(sure, c[k][i] + 1u);
              }
            const uint32_t m = uniform_u32(wave_max_u32_v(sure));
            if (m) in_lim = min(cin_lim, am_iw_lim_raise(in_lim, am_iw_lim_sure_w(m - 1u, lw)));
          }
          uint32_t nl = 0;  // list entries (wave-uniform)
          auto classify = [&](const int k, const uint32_t (&ck)[OPL]) {
            const uint64_t t = sb + (uint64_t)k * TILE;
            if (t >= off1) return;
            const uint32_t q = sr + (uint32_t)k * (uint32_t)TILE + lane * OPL;  // the lane's first op, from t0
            uint32_t *const sw = stage + k * (int)(TILE / 32) + lane / LPW;
            const bool whole = t >= off0 && t + TILE <= off1;
            if (whole) {  // a whole tile of included ops below every maximum, or of excluded ops
              const uint32_t ch = max(max(ck[0], ck[1]), max(ck[2], ck[3]));  // (AM_PK_ESC is the largest word)
              const uint32_t cl = min(min(ck[0], ck[1]), min(ck[2], ck[3]));
              const bool in = !__ballot(ch >= in_lim);
              if (in || !__ballot(cl < out_lim || ch == AM_PK_ESC)) {
                if (in) cnt += OPL;
                else minex = min(minex, q);
                anyc |= (1u << OPL) - 1u;
                if (lane % LPW == 0) *sw = in ? ~0u : 0u;
                return;
              }
            }
            uint32_t esc = 0, cand = 0, ib = 0, win = 0;
#pragma unroll
            for (int i = 0; i < OPL; ++i) {
              const bool inr = whole || q + (uint32_t)i - lo < nops;
              const int cl = am_iw_class32(ck[i], in_lim, out_lim);
              esc |= (uint32_t)(inr && cl == AM_IW_ESCAPED) << i;
              cand |= (uint32_t)(inr && cl != AM_IW_ESCAPED) << i;
              ib |= (uint32_t)(inr && cl == AM_IW_IN) << i;
              win |= (uint32_t)(inr && cl == AM_IW_WINDOW) << i;
            }
            cnt += (uint32_t)__popc(ib);
            anyc |= cand;
            anyesc |= esc;
            const uint32_t ti = q / (uint32_t)TILE;
            if (esc) escm |= ti < 64 / OPL ? (uint64_t)esc << (OPL * ti) : ~0ull;  // ~0: walk the key
            const uint32_t ex = cand & ~ib & ~win;  // excluded by the commit word
            if (ex) minex = min(minex, q + (uint32_t)__builtin_ctz(ex));
            uint32_t word = ib << (OPL * (lane % LPW));
#pragma unroll
            for (uint32_t xo = 1; xo < LPW; xo <<= 1) word |= (uint32_t)__shfl_xor((int)word, (int)xo);
            if (lane % LPW == 0) *sw = word;
            // ---- 2. the tile's window ops onto the list, in descending op order ----
            if (__ballot(win != 0)) {
              const uint32_t pc = (uint32_t)__popc(win);
              const uint32_t inc = wave_incl_scan_u32(pc, lane);
              const uint32_t tot = lane_u32(inc, WAVE - 1);
              uint32_t pos = nl + tot - inc;
#pragma unroll
              for (int i = OPL - 1; i >= 0; --i)
                if ((win >> i) & 1u) list[pos++] = (uint16_t)((uint32_t)k * (uint32_t)TILE + lane * OPL + (uint32_t)i);
              nl += tot;
            }
          };
#pragma unroll
          for (int k = SEGT - 1; k >= 0; --k) classify(k, c[k]);
          wave_sync();
          // ---- 3. rounds ----
          if (nl) {
            uint32_t mx[DMAX];  // the lane's maxima over its included window ops of this segment
#pragma unroll
            for (int d = 0; d < DMAX; ++d) mx[d] = 0;
            // (loads are not predicated: a lane without an entry reads the segment's first slot)
            const uint32_t *const cseg = L.lag_ct + sb;
            const uint16_t *const lseg = L.lag + sb;
            uint32_t cn = cseg[lane < nl ? (uint32_t)list[lane] : 0u];  // the coming round's commit words
            auto round = [&](const uint32_t r0, auto first) {
              const uint32_t i = r0 + lane;
              const bool v = i < nl;
              const uint32_t e = v ? (uint32_t)list[min(i, SEGOPS - 1u)] : 0u;
              const uint32_t cc = cn;
              uint32_t nx = 0;
              if (r0 + WAVE < nl) nx = cseg[i + WAVE < nl ? (uint32_t)list[min(i + WAVE, SEGOPS - 1u)] : 0u];
              bool need = v, sin = false;  // the first round's entries were classified just now
              if constexpr (!decltype(first)::value) {
                const int cl = am_iw_class32(cc, in_lim, out_lim);
                sin = v && cl == AM_IW_IN, need = v && cl == AM_IW_WINDOW;
              }
              bool in = false;
              if (decltype(first)::value || __ballot(need)) {
                uint32_t lg[DMAX];
#pragma unroll
                for (int d = 0; d < DMAX; ++d) lg[d] = d < (int)nd ? (uint32_t)(lseg + (uint64_t)d * stride)[e] : 0u;
                // (pad DCs d >= nd: c - lb[d] with lb = 0 lies under the always-passing pad threshold)
                in = need;
#pragma unroll
                for (int d = 0; d < DMAX; ++d) {
                  lg[d] = cc - (lb[d] + lg[d]);
                  in = in && lg[d] <= pk.thr[d];
                }
#pragma unroll
                for (int d = 0; d < DMAX; ++d) mx[d] = max(mx[d], in ? lg[d] : 0u);
              }
              cn = nx;
              const bool inc = in || sin;
              if (inc) atomicOr(stage + (e >> 5), 1u << (e & 31u));
              cnt += (uint32_t)inc;
              if (v && !inc) minex = min(minex, sr + e);
              if (__ballot(in)) {
                // any lane's maxima bound every lane's: min_d (mx[d] + lb[d]), in u32 above the
                // smallest base (a saturated sum is a smaller bound, which is safe)
                uint32_t f = 0xFFFFFFFFu;
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                  if (d < (int)nd) f = am_iw_fold32(f, mx[d], lb[d], lbm);
                in_lim = min(cin_lim, am_iw_lim_raise(in_lim, am_iw_lim_of32(uniform_u32(wave_max_u32_v(f)), lbm)));
              }
            };
            round(0u, std::true_type{});
            for (uint32_t r0 = WAVE; r0 < nl; r0 += WAVE) round(r0, std::false_type{});
            wave_sync();  // the list is done: its bytes take the maxima
#pragma unroll
            for (int d = 0; d < DMAX; ++d) sm.mx[d][lane] = mx[d];
          }
          // ---- 4. the staged words out (lane w: ops [sb + 32 w, + 32)) ----
          {
            uint32_t wl = lane;  // (opaque, as sl_ above)
            asm volatile("" : "+v"(wl));
            const uint64_t w0 = sb + 32ull * wl;
            if (wl < SEGOPS / 32 && w0 < off1) {
              const uint32_t word = stage[wl];
              if (w0 >= off0 && w0 + 32 <= off1) {
                ibm[w0 >> 5] = word;
              } else {  // a word shared with a neighbouring key: only this read's bits change
                const uint32_t blo = off0 > w0 ? (uint32_t)(off0 - w0) : 0u;
                const uint32_t bhi = off1 < w0 + 32 ? (uint32_t)(off1 - w0) : 32u;
                const uint32_t mask = (bhi >= 32 ? ~0u : ((1u << bhi) - 1u)) & ~((1u << blo) - 1u);
                atomicAnd(ibm + (w0 >> 5), ~mask);
                atomicOr(ibm + (w0 >> 5), word & mask);
              }
            }
          }
          wave_sync();
          if (nl) mxr = max(mxr, mx_reduce<DMAX>(sm.mx, lane));
          wave_sync();  // list, staged words and maxima are rewritten by the next segment
        }
      } else {
        uint32_t mx[DMAX];  // the lane's LastOpCt maxima
#pragma unroll
        for (int d = 0; d < DMAX; ++d) mx[d] = 0;
        // one tile's inclusion bits -> partials, escape marks and the bitmap words
        auto tile_out = [&](uint64_t t, uint64_t g, uint32_t ib, uint32_t esc, uint32_t cand) {
          if (pk.never) ib = 0;
          cnt += (uint32_t)__popc(ib);
          anyc |= cand;
          anyesc |= esc;
          const uint64_t ti = (t - t0) / TILE;
          if (esc) escm |= ti < 64 / OPL ? (uint64_t)esc << (OPL * ti) : ~0ull;  // ~0: walk the key
          const uint32_t ex = cand & ~ib;
          if (ex) minex = min(minex, (uint32_t)(g - t0) + (uint32_t)__builtin_ctz(ex));
          uint32_t word = ib << (OPL * (lane % LPW));
  #pragma unroll
          for (uint32_t xo = 1; xo < LPW; xo <<= 1) word |= (uint32_t)__shfl_xor((int)word, (int)xo);
          const uint64_t w0 = g & ~31ull;  // this lane group's word: ops [w0, w0 + 32)
          if (lane % LPW == 0 && w0 < off1) {
            if (w0 >= off0 && w0 + 32 <= off1) {
              ibm[w0 >> 5] = word;
            } else {  // a word shared with a neighbouring key: only this read's bits change
              const uint32_t lo = off0 > w0 ? (uint32_t)(off0 - w0) : 0u;
              const uint32_t hi = off1 < w0 + 32 ? (uint32_t)(off1 - w0) : 32u;
              const uint32_t mask = (hi >= 32 ? ~0u : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
              atomicAnd(ibm + (w0 >> 5), ~mask);
              atomicOr(ibm + (w0 >> 5), word & mask);
            }
          }
        };
        for (uint64_t t = t0; t < off1; t += TILE) {
          const uint64_t g = t + (uint64_t)lane * OPL;
          uint32_t esc = 0, cand = 0;
          const bool whole = t >= off0 && t + TILE <= off1;
          uint32_t x[OPL][DMAX];
#pragma unroll
          for (int d = 0; d < DMAX; ++d) {
            uint32_t q[OPL] = {};
            if (d < (int)nd && g < off1) ld_n32<OPL>(L.pk_vc + (uint64_t)d * stride + g, q);
#pragma unroll
            for (int k = 0; k < OPL; ++k) x[k][d] = q[k];
          }
          const uint32_t ib = whole ? incl_tile<DMAX, OPL, false>(pk_ent(x), pk, g, off0, off1, mx, esc, cand)
                                    : incl_tile<DMAX, OPL, true>(pk_ent(x), pk, g, off0, off1, mx, esc, cand);
          tile_out(t, g, ib, esc, cand);
        }
#pragma unroll
        for (int d = 0; d < DMAX; ++d) sm.mx[d][lane] = mx[d];  // for the reduction below
      }
      // ---- the read's scalar outputs: LastOpCt maxima reduced through LDS (mx_reduce; the lag
      //      instantiation's are reduced already, per segment), the rest by DPP ----
      const uint32_t count_p = wave_sum_u32_v(cnt);
      minex = wave_min_u32_v(minex);
      const bool cands = __ballot(anyc != 0) != 0;
      const bool escs = __ballot(anyesc != 0) != 0;
      uint32_t mxd = mxr;
      if constexpr (!LAG) {
        wave_sync();
        mxd = mx_reduce<DMAX>(sm.mx, lane);
      }
      // the read's in-view partials into the batch's LDS rows (slot j).  Ops outside the streamed
      // view (rare) are not evaluated here: the read leaves its lanes' escape marks in the wave's
      // scratch row j and its bit in escmask, and the deferred phase below merges them in
      uint32_t cl_ = lane;  // (opaque, as sl_ above: the row's address is not held across the loops)
      asm volatile("" : "+v"(cl_));
      if (cl_ < nd) sm.ct[cl_][j] = mxd;
      if (lane == 0) {
        sm.flags[j] = ((cands && (sfl & SLOT_MISS)) ? (uint32_t)AM_FLAG_MISSING_DC_LOGGED : 0u) | (count_p ? FLAG_INVIEW : 0u);
        sm.count[j] = count_p;
        sm.pres[j] = count_p ? allmask : 0u;
        sm.mex[j] = minex == 0xFFFFFFFFu ? NONE : t0 + minex;
      }
      if (escs) {
        escw[(uint64_t)j * WAVE + lane] = escm;
        escmask |= 1u << j;
      }
      wave_sync();  // sm.mx is rewritten by the next read
    }
    // ---- the deferred phase: the escaped ops of the batch's reads that met any, through the
    //      escape reader; the included ones' bits are ORed into the bitmap and their partials
    //      merged into the read's row.  No tile state is live here, so the D-wide u64 values of
    //      esc_load / eval_op do not weigh on the tile loop's registers ----
    if (escmask) {
      __builtin_amdgcn_s_waitcnt(0);  // the batch's bitmap words and mark rows are out
      read_inputs<DMAX, false, true>(L, nd, B, 0, u);  // the clock again: not held across the reads' loops
    }
    for (uint32_t xm = escmask; xm; xm &= xm - 1) {
      const uint32_t j = (uint32_t)__builtin_ctz(xm);
      const uint64_t off0 = uniform_u64(sl[j].off0), off1 = off0 + uniform_u32(sl[j].nops);
      const uint64_t K = uniform_u64(sl[j].K), t0 = off0 & ~31ull;
      const uint64_t escm = escw[(uint64_t)j * WAVE + lane];
      Acc<DMAX> a;
      a.reset();
      // The lane's own escaped ops, marked by the tile loop: no second walk of the key.  A long
      // key's late tiles have no mark bits (a lane's ~0): the wave walks the escape marks of the
      // view it streamed instead, lane l the slots off0 + l, + 64, ...  One evaluation site serves
      // both (two inlined copies of esc_load / eval_op cost the packed instantiation its fourth
      // wave); cur is the marks left, or the walk's next slot.
      const bool walk = __ballot(escm == ~0ull) != 0;
      const uint32_t *const escv = LAG ? L.lag_ct : L.pk_vc;
      for (uint64_t cur = walk ? off0 + lane : escm;;) {
        uint64_t p;
        if (walk) {
          while (cur < off1 && escv[cur] != AM_PK_ESC) cur += WAVE;
          if (cur >= off1) break;
          p = cur, cur += WAVE;
        } else {
          if (!cur) break;
          const uint32_t b = (uint32_t)__builtin_ctzll(cur);
          cur &= cur - 1;
          p = t0 + (uint64_t)(b / OPL) * TILE + (uint64_t)lane * OPL + b % OPL;
        }
        uint64_t sv[DMAX], ct;
        uint32_t meta;
        esc_load<DMAX>(L, nd, stride, p, LAG ? K : NONE, sv, ct, meta);
        if (eval_op<DMAX, false>(u, meta, ct, sv, u.allmask, false, p, a) && !(meta & AM_META_BAD))
          atomicOr(&ibm[p >> 5], 1u << (p & 31));
      }
      const uint32_t ecount = wave_sum_u32_v(a.count), eflags = wave_or_u32_v(a.flags);
      const uint32_t epres = wave_or_u32_v(a.pres);
      const uint64_t emex = wave_min_u64_v(a.min_excl);
      uint64_t emx = 0;  // lane d: DC d's maximum over the included escaped ops
#pragma unroll
      for (int d = 0; d < DMAX; ++d) {
        if (d >= (int)nd) continue;
        const uint64_t am = wave_max_u64_v(a.mx[d]);
        if ((uint32_t)d == lane) emx = am;
      }
      // the escaped ops' maxima are full-width (an escaped entry may lie below K, or 2^32 and more
      // above it): they take the read's scratch row, whose marks are consumed, lane d: DC d
      if (lane < nd) escw[(uint64_t)j * WAVE + lane] = emx;
      if (lane == 0) {
        sm.flags[j] |= eflags;
        sm.count[j] += ecount;
        sm.pres[j] |= epres;
        sm.mex[j] = umin64(sm.mex[j], emex);
      }
    }
    if (escmask) __builtin_amdgcn_s_waitcnt(0);  // the escaped ops' maxima are out: another lane reads them
    wave_sync();
    // ---- the batch's outputs, derived from the merged partials: one coalesced store per column
    //      (lane j: read b0 + j) ----
    uint32_t ol = lane;  // (opaque, as sl_ above)
    asm volatile("" : "+v"(ol));
    if (ol < IWB && (((uint32_t)emask >> ol) & 1u)) {
      const uint64_t r = sl[ol].r;
      const uint32_t flags = sm.flags[ol];
      const int32_t st = (flags & FLAG_BAD) ? AM_ERR_UNEXPECTED_OPERATION : AM_OK;
      R.status[r] = st;
      R.flags[r] = (uint8_t)(flags & 0xFFu);
      if (st == AM_OK) {
        const uint32_t c = sm.count[ol];
        const uint32_t opres = c == 0 ? 0u : sm.pres[ol];  // (count 0: base ignore)
        const uint64_t off0 = sl[ol].off0;
        R.new_last_op[r] = new_last_op_b(L, sl[ol].idb, off0, off0 + sl[ol].nops, sm.mex[ol]);
        R.last_ct_ignore[r] = c == 0 ? 1 : 0;
        R.last_ct_pres[r] = opres;
        R.is_new_ss[r] = c > 0;
        R.count[r] = c;
        // the columns: the slot's K under the in-view maxima, and the escaped ops' merged in 64 bits
        const uint64_t K = sl[ol].K;
        const bool inview = (flags & FLAG_INVIEW) != 0, esc = ((escmask >> ol) & 1u) != 0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
          if (d < (int)nd) {
            uint64_t v = inview ? K + sm.ct[d][ol] : 0;
            if (esc) v = umax64(v, escw[(uint64_t)ol * WAVE + d]);
            R.last_ct[(uint64_t)d * n + r] = ((opres >> d) & 1u) ? v : 0;
          }
      }
    }
    wave_sync();  // the slots are rewritten by the next batch
  }
}

// ---------------------------------------------------------------- split fresh read, pass 2
// The record pass: the groups of the reads k_grp_incl took, against its bitmap, and the
// survivors' pairs.  Two kernels over one skeleton (rec_pass): k_grp_spans reads the group-span
// view, k_grp_recs the records.  Latency-bound (a read is a few KB), so a wave keeps the NEXT
// read's bitmap words and first span / record loads in flight while it applies this read's and
// gathers its survivors; LDS per wave is a few KB (survivor list in rounds), so ~5 waves per SIMD.
constexpr uint32_t RLIST = 256;  // survivor-list entries per gather round
struct RSlot {
  uint64_t off0, rk0, ooff;
  uint32_t r, nops, nrec, G, ocap, nb;  // nb (k_grp_spans): the key's spans; AM_NSPAN_NONE: by the nrec records
};
struct RSmem {
  // per group: born / an effective kill included (k_grp_spans sets born for the alive groups
  // only -- its kill test is per span -- and killed for its reads by records)
  uint32_t born[VG / 32], killed[VG / 32];
  uint32_t incl[VWORDS];
  uint16_t list[RLIST];
  uint16_t bri[VG];  // per group: its birth record (from the read's rk0), set with its born bit
  RSlot slot[IWB];
};
// The record rule of a fresh read, one record: x (record i of its read, 0xFFFFFFFF: a dead slot)
// against the read's LDS bitmap (bit = op + sh) sets its group's born or killed bit, a birth
// also the group's birth record.  (k_grp_recs, and k_grp_spans for its keys without spans.)
__device__ __forceinline__ void rec_apply(uint32_t x, uint32_t i, uint32_t sh, const uint32_t *incl, uint32_t *born,
                                          uint32_t *killed, uint16_t *bri) {
  if (x == 0xFFFFFFFFu) return;
  const uint32_t bit = AM_REC_OP(x) + sh;
  if (!((incl[bit >> 5] >> (bit & 31)) & 1u)) return;
  const uint32_t g = AM_REC_GRP(x);
  atomicOr(((x & AM_REC_KILL) ? killed : born) + (g >> 5), 1u << (g & 31));
  if (!(x & AM_REC_KILL)) bri[g] = (uint16_t)i;  // a group's one birth
}

// The skeleton of a record pass; s is the wave's LDS.  A kernel brings its inner loop:
//   Pre             a read's prefetched inputs: .w, one bitmap word per lane, and the kernel's loads
//   pre(j, p)       issue the kernel's loads of read j of the slot table: its first spans / records,
//                   from rk0 & ~3
//   apply(p, j, rk0, G, sh)  read j's spans / records, the first from p, against the LDS bitmap
//                   (bit = op + sh) -> born / killed bits and birth records
//   alive(w)        word w of the alive groups, from born / killed
// SPANS: the slots carry the key's span count (nb).
template <int TYPE, bool SPANS, class Pre, class FPre, class FApply, class FAlive>
__device__ __forceinline__ void rec_pass(const am_op_log &L, const am_read_batch &B, am_read_result &R, const am_sel &S,
                                         uint32_t short_opl, const uint32_t *ibm, RSmem &s, uint32_t lane, FPre pre,
                                         FApply apply, FAlive alive) {
  const uint32_t sel0 = S.idx ? uniform_u32(S.range[0]) : 0u;
  const uint64_t nsel = S.idx ? (uint64_t)(uniform_u32(S.range[1]) - sel0) : B.n_reads;
  const uint64_t W = (uint64_t)gridDim.x * NW;
  const uint64_t gw = (uint64_t)blockIdx.x * NW + uniform_u32(threadIdx.x >> 6);
  const uint64_t *const pairs = L.prec ? L.prec : L.grp;
  // read j of the slot table a read ahead: its bitmap words [t0 / 32, ...) (lane i: word i, the
  // first 64), then the kernel's first loads
  auto prefetch = [&](uint32_t j, Pre &p) {
    const uint64_t off0 = s.slot[j].off0, t0 = off0 & ~31ull;
    const uint32_t nw = (uint32_t)((off0 + s.slot[j].nops - t0 + 31) / 32);
    p.w = lane < nw ? ibm[(t0 >> 5) + lane] : 0u;
    pre(j, p);
  };

  for (uint64_t b0 = gw * IWB; b0 < nsel; b0 += (uint64_t)IWB * W) {
    // ---- lane j < IWB: read b0 + j -> slot j (the reads k_grp_incl took and left ok) ----
    const uint64_t ii = b0 + lane;
    bool ok = false;
    if (lane < IWB && ii < nsel) {
      GMeta mm;
      read_meta(L, B, S.idx ? (uint64_t)S.idx[sel0 + ii] : ii, TYPE, mm);
      ok = mm.st == AM_OK && wave_takes(L, B, mm, short_opl) && R.status[mm.r] == AM_OK;
      if (ok) {
        RSlot &w = s.slot[lane];
        const uint64_t o0 = R.value.set_off[mm.r], o1 = R.value.set_off[mm.r + 1];
        w.off0 = mm.off0, w.rk0 = mm.rk0, w.ooff = o0;
        w.r = (uint32_t)mm.r, w.nops = (uint32_t)(mm.off1 - mm.off0), w.nrec = (uint32_t)(mm.rk1 - mm.rk0);
        if (SPANS) {  // (a count beyond the key's record slots is no span view)
          const uint32_t nb = L.key_nspan[mm.key];
          w.nb = nb > w.nrec ? AM_NSPAN_NONE : nb;
        }
        w.G = mm.G, w.ocap = o1 - o0 < 0xFFFFFFFFull ? (uint32_t)(o1 - o0) : 0xFFFFFFFFu;
      }
    }
    uint64_t em = __ballot(ok);
    wave_sync();
    Pre cur;
    if (em) prefetch((uint32_t)__builtin_ctzll(em), cur);
    uint32_t setlen = 0;  // lane j: read j's survivor count
    int32_t cap_err = 0;  // lane j: read j overflowed its capacity
    for (; em; em &= em - 1) {
      const uint32_t j = (uint32_t)__builtin_ctzll(em);
      const uint64_t off0 = uniform_u64(s.slot[j].off0), rk0 = uniform_u64(s.slot[j].rk0);
      const uint64_t off1 = off0 + uniform_u32(s.slot[j].nops);
      const uint32_t G = uniform_u32(s.slot[j].G);
      const uint64_t t0 = off0 & ~31ull;
      const uint32_t sh = (uint32_t)(off0 - t0), nw = (uint32_t)((off1 - t0 + 31) / 32);
      // this read's bitmap into LDS (words past the first 64 straight from memory: long logs)
      if (lane < nw) s.incl[lane] = cur.w;
      for (uint32_t i = WAVE + lane; i < nw; i += WAVE) s.incl[i] = ibm[(t0 >> 5) + i];
      for (uint32_t g = lane; g < (G + 31) / 32; g += WAVE) s.born[g] = 0, s.killed[g] = 0;
      const Pre now = cur;
      // the next read's inputs in flight from here on
      const uint64_t rest = em & (em - 1);
      if (rest) prefetch((uint32_t)__builtin_ctzll(rest), cur);
      wave_sync();
      apply(now, j, rk0, G, sh);
      wave_sync();
      // ---- survivors in group order: lane w owns alive word w; listed in rounds of RLIST ----
      const uint32_t aw = lane < (G + 31) / 32 ? alive(lane) : 0u;
      const uint32_t cnt = (uint32_t)__popc(aw);
      // (the scan's lane number opaque, as sl_ in k_grp_incl: its per-step lane masks are computed
      //  here, not once per batch and then held in registers across the reads' inner loops)
      uint32_t ql = lane;
      asm volatile("" : "+v"(ql));
      const uint32_t inc = wave_incl_scan_u32(cnt, ql);
      const uint32_t ns = (uint32_t)__shfl((int)inc, 63, WAVE);
      const uint64_t ooff = uniform_u64(s.slot[j].ooff);
      const uint32_t ocap = uniform_u32(s.slot[j].ocap);
      const uint32_t nput = ns < ocap ? ns : ocap;
      for (uint32_t base = 0; base < nput; base += RLIST) {
        uint32_t o = inc - cnt;
        for (uint32_t bits = aw; bits; bits &= bits - 1, ++o)
          if (o >= base && o < base + RLIST) s.list[o - base] = (uint16_t)(lane * 32 + __builtin_ctz(bits));
        wave_sync();
        const uint32_t end = nput - base < RLIST ? nput - base : RLIST;
        for (uint32_t j0 = 0; j0 < end; j0 += 2 * WAVE) {
          const uint32_t j1 = j0 + lane, j2 = j1 + WAVE;
          u64x2 p1 = {0, 0}, p2 = {0, 0};
          // a survivor's pair through its birth record (prec: births close together in op
          // order) rather than its group slot (grp: one group run apart in output order)
          if (j1 < end) p1 = *(const u64x2 *)(pairs + 2 * (rk0 + (L.prec ? s.bri[s.list[j1]] : s.list[j1])));
          if (j2 < end) p2 = *(const u64x2 *)(pairs + 2 * (rk0 + (L.prec ? s.bri[s.list[j2]] : s.list[j2])));
          if (j1 < end) R.value.set_a[ooff + base + j1] = p1.x, R.value.set_b[ooff + base + j1] = p1.y;
          if (j2 < end) R.value.set_a[ooff + base + j2] = p2.x, R.value.set_b[ooff + base + j2] = p2.y;
        }
        wave_sync();
      }
      if (lane == j) setlen = ns, cap_err = ns > ocap;
      wave_sync();
    }
    // ---- the batch's outputs (lane j: read b0 + j): set_len, or the capacity status ----
    if (ok) {
      const uint64_t r = s.slot[lane].r;
      if (cap_err) R.status[r] = AM_ERR_CAPACITY;
      else R.value.set_len[r] = setlen;
    }
    wave_sync();  // the slots are rewritten by the next batch
  }
}

// k_grp_recs: one u32 record per birth and kill slot, two chunks of them prefetched per read
constexpr uint32_t RCH = 512;  // records per chunk: two 16-byte loads per lane
struct RPre {  // a read's prefetched inputs: one bitmap word and two record chunks per lane
  uint32_t w;
  u32x4 c[4];
};

template <int DMAX, int TYPE>
__global__ void __launch_bounds__(BLOCK, 5) k_grp_recs(am_log_arg LA, am_read_batch B, am_read_result R, am_sel S,
                                                       uint32_t short_opl, const uint32_t *ibm) {
  const am_op_log L = LA.log();
  __shared__ RSmem smem[NW];
  RSmem &s = smem[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & (WAVE - 1);

  // records [q0, q0 + 2 RCH) of a read whose records end at rk1 (q0 a multiple of 4)
  auto ld_recs = [&](uint64_t q0, uint64_t rk1, u32x4 (&c)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t q = q0 + (uint64_t)k * 4 * WAVE + 4 * lane;
      c[k] = q < rk1 ? *(const u32x4 *)(L.rec_g + q) : u32x4{~0u, ~0u, ~0u, ~0u};
    }
  };
  auto pre = [&](uint32_t j, RPre &p) {
    const uint64_t rk0 = s.slot[j].rk0;
    ld_recs(rk0 & ~3ull, rk0 + s.slot[j].nrec, p.c);
  };
  // two chunks of records from q0 -> born / killed bits
  auto apply4 = [&](const u32x4 (&c)[4], uint64_t q0, uint64_t rk0, uint64_t rk1, uint32_t sh) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t q = q0 + (uint64_t)k * 4 * WAVE + 4 * lane;
      const uint32_t xs[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (xs[e] == 0xFFFFFFFFu || q + e < rk0 || q + e >= rk1) continue;
        rec_apply(xs[e], (uint32_t)(q + e - rk0), sh, s.incl, s.born, s.killed, s.bri);
      }
    }
  };
  // the two prefetched chunks, then the rest two chunks at a time
  auto apply = [&](const RPre &p, uint32_t j, uint64_t rk0, uint32_t, uint32_t sh) {
    const uint64_t rk1 = rk0 + uniform_u32(s.slot[j].nrec), qa = rk0 & ~3ull;
    apply4(p.c, qa, rk0, rk1, sh);
    for (uint64_t q0 = qa + 2 * RCH; q0 < rk1; q0 += 2 * RCH) {
      u32x4 c[4];
      ld_recs(q0, rk1, c);
      apply4(c, q0, rk0, rk1, sh);
    }
  };
  rec_pass<TYPE, false, RPre>(L, B, R, S, short_opl, ibm, s, lane, pre, apply,
                              [&](uint32_t w) { return s.born[w] & ~s.killed[w]; });
}

// k_grp_spans: the group-span view (include/antidote_mat.h key_nspan / gspan / gsrc) -- one word
// per BORN group (birth op | kill op << 16) instead of one record per birth and kill slot.  A
// fresh read has no base, so a group is alive iff its birth op is included and its one effective
// kill (if any) is not; only an alive group reads its gsrc word (group | birth record << 16) and
// sets its LDS bit: one atomicOr per survivor.  The outputs are k_grp_recs's, bit for bit.
// A read of a key without spans (AM_NSPAN_NONE: a group with two effective kills, ...) streams
// the key's records here instead, by rec_apply without the prefetch: such keys are rare
// (concurrent removes of one token), and a second launch for them, or a list of them, costs every
// batch more than they do.
constexpr int SPRE = 4;  // prefetched 16-byte span loads per lane: the first 1024 spans of a read
struct SPre {  // a read's prefetched inputs: one bitmap word and SPRE span loads per lane
  uint32_t w;
  u32x4 c[SPRE];
};

template <int DMAX, int TYPE>
__global__ void __launch_bounds__(BLOCK, 5) k_grp_spans(am_op_log L, am_read_batch B, am_read_result R, am_sel S,
                                                        uint32_t short_opl, const uint32_t *ibm) {
  __shared__ RSmem smem[NW];
  RSmem &s = smem[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  constexpr uint32_t SCH = (uint32_t)SPRE * 4 * WAVE;  // spans per pass of the wave

  // spans [q0, q0 + SCH) of a read whose spans are [rk0, rk1) (lane i: four consecutive words per
  // load, q0 a multiple of 4)
  auto ld_spans = [&](uint64_t q0, uint64_t rk1, u32x4 (&c)[SPRE]) {
#pragma unroll
    for (int k = 0; k < SPRE; ++k) {
      const uint64_t q = q0 + (uint64_t)k * 4 * WAVE + 4 * lane;
      c[k] = q < rk1 ? *(const u32x4 *)(L.gspan + q) : u32x4{0, 0, 0, 0};
    }
  };
  auto pre = [&](uint32_t j, SPre &p) {
    const uint64_t rk0 = s.slot[j].rk0;
    const uint32_t nb = s.slot[j].nb;
    ld_spans(rk0 & ~3ull, rk0 + (nb == AM_NSPAN_NONE ? 0u : nb), p.c);
  };
  // one pass of spans against the LDS bitmap (bit = op + sh): the alive ones' gsrc words are
  // loaded together (independent loads, one wait), then their bits and birth records set
  auto apply1 = [&](const u32x4 (&c)[SPRE], uint64_t q0, uint64_t rk0, uint64_t rk1, uint32_t sh) {
    uint32_t src[SPRE * 4];
    uint32_t am = 0;
#pragma unroll
    for (int k = 0; k < SPRE; ++k) {
      const uint64_t q = q0 + (uint64_t)k * 4 * WAVE + 4 * lane;
      const uint32_t xs[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool inr = q + e >= rk0 && q + e < rk1;  // (a word of a neighbouring key is not looked at)
        const uint32_t x = inr ? xs[e] : 0u;
        const uint32_t b = (x & 0xFFFFu) + sh, kl = (x >> 16) + sh;
        const bool inb = (s.incl[b >> 5] >> (b & 31)) & 1u, ink = (s.incl[kl >> 5] >> (kl & 31)) & 1u;
        const bool al = inr && inb && (kl == b || !ink);
        src[4 * k + e] = al ? L.gsrc[q + e] : 0u;
        am |= (uint32_t)al << (4 * k + e);
      }
    }
#pragma unroll
    for (int i = 0; i < SPRE * 4; ++i)
      if ((am >> i) & 1u) {
        const uint32_t g = src[i] & 0xFFFFu;
        atomicOr(s.born + (g >> 5), 1u << (g & 31));
        s.bri[g] = (uint16_t)(src[i] >> 16);  // a group's one birth
      }
  };
  // the prefetched pass, then the rest a pass at a time
  auto apply = [&](const SPre &p, uint32_t j, uint64_t rk0, uint32_t G, uint32_t sh) {
    const uint32_t nbj = uniform_u32(s.slot[j].nb);
    const bool byrec = nbj == AM_NSPAN_NONE;
    const uint64_t rk1 = rk0 + (byrec ? 0u : nbj), qa = rk0 & ~3ull;
    apply1(p.c, qa, rk0, rk1, sh);
    for (uint64_t q0 = qa + SCH; q0 < rk1; q0 += SCH) {
      u32x4 c[SPRE];
      ld_spans(q0, rk1, c);
      apply1(c, q0, rk0, rk1, sh);
    }
    if (byrec) {  // rare: the key's records by rec_apply, then born = born and not killed
      const uint32_t nrec = uniform_u32(s.slot[j].nrec);
      for (uint32_t i = lane; i < nrec; i += WAVE) rec_apply(L.rec_g[rk0 + i], i, sh, s.incl, s.born, s.killed, s.bri);
      wave_sync();
      for (uint32_t g = lane; g < (G + 31) / 32; g += WAVE) s.born[g] &= ~s.killed[g];
    }
  };
  rec_pass<TYPE, true, SPre>(L, B, R, S, short_opl, ibm, s, lane, pre, apply, [&](uint32_t w) { return s.born[w]; });
}

// ---------------------------------------------------------------- launcher
// the split fresh read: k_grp_incl (op stream -> inclusion bitmap + scalars), then the record /
// survivor pass: k_grp_spans when the log has the group-span view (key_nspan, gspan and gsrc all
// set; a caller that nulls one gets k_grp_recs), else k_grp_recs
template <int D, int TYPE, bool EXACT>
int launch_split(am_ctx *ctx, const am_op_log *L, const am_read_batch *B, am_read_result *R, am_sel S,
                 am_retry next, uint32_t short_opl) {
  const uint64_t stride = L->snap_stride ? L->snap_stride : L->n_ops;
  void *ibm = nullptr;
  if (int rc = am_ctx_scratch(ctx, AM_SCR_INCL, (stride / 32 + 4) * 4, &ibm)) return rc;
  // the lag view when the log has it: 4 + 2 D bytes of commit vector per op instead of 4 D
  const bool lag = L->lag_ct && L->lag && L->key_lag;
  const bool spans = L->key_nspan && L->gspan && L->gsrc;
  // per kernel: each grid is sized by its own (occ_i[LAG]: the two inclusion instantiations
  // have their own launch bounds)
  static int occ_i[2] = {0, 0}, occ_w = 0, occ_s = 0;
  const uint64_t want = (B->n_reads + NW * IWB - 1) / (NW * IWB);  // a wave per IWB reads
  // the packed instantiation's grid, the first launch's, the record pass's
  const uint64_t bp = grp_grid(ctx, occ_i[0], k_grp_incl<D, TYPE, EXACT, false>, BLOCK, 0, 2, want);
  const uint64_t bi =
      lag ? grp_grid(ctx, occ_i[1], k_grp_incl<D, TYPE, EXACT, true, const uint16_t *>, BLOCK, 0, 2, want) : bp;
  const uint64_t bw = spans ? grp_grid(ctx, occ_s, k_grp_spans<D, TYPE>, BLOCK, 0, 1, want)
                            : grp_grid(ctx, occ_w, k_grp_recs<D, TYPE>, BLOCK, 0, 1, want);
  if (bi == 0) return AM_OK;
  // the escape-mark rows of the inclusion pass: 64 lanes x 8 bytes per read slot of every wave of
  // the larger grid (the two launches run one after the other and share them); a store without
  // escaped ops never touches them
  void *escv = nullptr;
  if (int rc = am_ctx_scratch(ctx, AM_SCR_ESCM, (bi > bp ? bi : bp) * NW * IWB * WAVE * sizeof(uint64_t), &escv))
    return rc;
  uint64_t *const escr = (uint64_t *)escv;
  if (lag) {
    // the reads of packed-routed keys leave the lag instantiation through a list; the packed
    // instantiation takes exactly those (an empty list: its blocks return at once)
    am_retry routed;
    am_sel rsel;
    if (int rc = am_route_list(ctx, B->n_reads, &routed, &rsel)) return rc;
    // the store's per-key lag widths when the log's lag view is a store's of this context (null:
    // the format's 16 bits for every key)
    const uint16_t *const lagw = am_lagw_find(ctx, L);
    hipLaunchKernelGGL((k_grp_incl<D, TYPE, EXACT, true, const uint16_t *>), dim3((unsigned)bi), dim3(BLOCK), 0,
                       ctx->stream, *L, *B, *R, S, next, routed, short_opl, (uint32_t *)ibm, escr, lagw);
    hipLaunchKernelGGL((k_grp_incl<D, TYPE, EXACT, false>), dim3((unsigned)bp), dim3(BLOCK), 0, ctx->stream, *L, *B,
                       *R, rsel, next, am_retry{}, short_opl, (uint32_t *)ibm, escr);
  } else {
    hipLaunchKernelGGL((k_grp_incl<D, TYPE, EXACT, false>), dim3((unsigned)bp), dim3(BLOCK), 0, ctx->stream, *L, *B,
                       *R, S, next, am_retry{}, short_opl, (uint32_t *)ibm, escr);
  }
  if (spans) {
    hipLaunchKernelGGL((k_grp_spans<D, TYPE>), dim3((unsigned)bw), dim3(BLOCK), 0, ctx->stream, *L, *B, *R, S,
                       short_opl, (const uint32_t *)ibm);
  } else {
    hipLaunchKernelGGL((k_grp_recs<D, TYPE>), dim3((unsigned)bw), dim3(BLOCK), 0, ctx->stream, *L, *B, *R, S,
                       short_opl, (const uint32_t *)ibm);
  }
  AM_HIP(hipGetLastError());
  return AM_OK;
}

}  // namespace amk_grp
