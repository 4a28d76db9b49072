// Appended to the parent commit's am_pack.hip by scripts/build_cadence_base.sh (the baseline library of
// scripts/bench_cadence.py, BASELINE.md "GST-cadence clocks"): the counters of am_store_view_stats
// over the parent's views, which have no routing, so that this tree's abi.py loads the library.
namespace {
__global__ void k_view_stats_base(am_op_log L, unsigned long long *out) {
  unsigned long long ops = 0, esc = 0, lonly = 0;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < L.n_keys; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t o0 = L.key_off[k], o1 = am_kend(L, k);
    for (uint64_t p = o0; p < o1; ++p) {
      const bool pk = !L.pk_vc || L.pk_vc[p] != AM_PK_ESC;
      esc += !pk;
      lonly += L.lag_ct && pk && L.lag_ct[p] == AM_PK_ESC;
    }
    ops += o1 - o0;
  }
  atomicAdd(out + 0, ops), atomicAdd(out + 1, esc), atomicAdd(out + 2, lonly);
}
}  // namespace
extern "C" int am_store_view_stats(am_ctx *c, const am_store *st, uint64_t *out) {
  if (!c || !st || st->ctx != c || !out) return AM_ERR_INVALID;
  AM_LOCK(c);
  AM_HIP(hipSetDevice(c->device));
  for (int i = 0; i < 5; ++i) out[i] = 0;
  const am_op_log &d = st->dev;
  if (!d.n_keys || !d.key_off) return AM_OK;
  void *cnt = nullptr;
  if (int rc = am_ctx_scratch(c, AM_SCR_MISC, 256, &cnt)) return rc;
  AM_HIP(hipMemsetAsync(cnt, 0, 40, c->stream));
  hipLaunchKernelGGL(k_view_stats_base, dim3(1024), dim3(256), 0, c->stream, d, (unsigned long long *)cnt);
  AM_HIP(hipGetLastError());
  return am_ctx_fetch(c, cnt, 5, out);
}
