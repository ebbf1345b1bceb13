// csrc/mvr_outlier.hip -- pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval on the GPU (gfx950); the rules are
// written next to mvr_cloud_statistical_outlier_removal / mvr_cloud_radius_outlier_removal in mvr_hip.h.
//
//   1. finite flags and the count of the finite points (the one read-back before the search).  A cloud that holds
//      non-finite points is searched through a compacted copy of its finite ones (a NaN or an infinity must not reach the
//      bounding box or a cell computation of the grid build); results are written back by original index.
//   2. the search, one thread per query in the order of the cloud's model grid (ensure_model_grid; the helpers of
//      mvr_knn_walk.h), the query itself skipped by index:
//      * mean distance: the shell walk (knn_shell_walk) with its f64 stopping bound, but the k-best list is KMAX 32-bit keys --
//        the bits of the non-negative f32 d2, which order as unsigned integers.  No index: the result does not depend on how
//        ties are broken, so the walk stops as soon as every unvisited cell is AT or beyond the k-th d2.  An insertion is
//        L[i] = max(L[i - 1], min(key, L[i])) with compile-time indices: two 32-bit operations per entry where the 64-bit
//        list needs two 64-bit compares and two 64-bit selects.  For k < KMAX the leading KMAX - k entries hold 0; a key
//        of 0 (an exact duplicate of the query) lands behind them because min / max keep the earlier entry on a tie, and
//        only the last k entries are summed.  The thread sums sqrtf(d2) of its own list in f64, ascending, and writes one
//        f32: no list goes to memory.
//      * neighbour count: the ball walk (knn_ball_walk) with a counter.
//   3. statistics (mean distances only): two f64 reductions in a FIXED order -- a block sums a contiguous chunk of the
//      points (strided per thread, then an LDS tree), one block sums the partials -- first the mean, then the squared
//      deviations from it; the threshold is formed on the device.  No float atomics: bit-identical from run to run.
//   4. a flag per point from the threshold or the count, the selected indices, ascending (select_flagged), one small
//      read-back (count and statistics), then the gather of points and normals (gather_kept).
// Scratch arrays come out of the context's arena (Ctx::dn_arena), as in mvr_voxel.hip.  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {
namespace {

constexpr int kOutlThreads = kKnnThreads;
constexpr unsigned kOutlSumBlocks = 1024;     // most partial sums of a reduction (a function of n alone: the summation order is fixed)
constexpr uint32_t kListInit = 0xFFFFFFFFu;   // above the bits of every d2 (+inf is 0x7F800000; finite points give no NaN)

struct OutlArgs {
  KnnSlot S;                       // the cloud searched against itself (nrm / curv / oidx / od2 unused)
  const uint32_t *remap;           // set: the searched cloud is the compacted finite points, remap[i] = index in the source
  float *mean_dist;                // out, by source index
  uint32_t *count;                 // out, by source index
  int k;
  float r2;
};

// fin[i], the per-point result preset to what a non-finite point gets (NaN bits / 0), counters[0] += finite points
__global__ void __launch_bounds__(kOutlThreads) outl_finite_kernel(const float4 *__restrict__ p, size_t n, uint8_t *__restrict__ fin,
                                                                   uint32_t *__restrict__ val, uint32_t preset, uint32_t *__restrict__ counters)
{
  __shared__ uint32_t s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * kOutlThreads + threadIdx.x;
  bool f = false;
  if (i < n) {
    f = finite3(p[i]);
    fin[i] = f ? 1 : 0;
    val[i] = preset;
  }
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, (uint32_t)__popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(&counters[0], s_cnt);
}

// the ordered list: insert `key` (which is below L[KMAX - 1]); every index is a compile-time constant
template <int KMAX>
__device__ __forceinline__ void outl_insert(uint32_t (&L)[KMAX], const uint32_t key)
{
#pragma unroll
  for (int i = KMAX - 1; i > 0; --i) L[i] = max(L[i - 1], min(key, L[i]));
  L[0] = min(key, L[0]);
}

// the visitor of the shell walk that keeps the k smallest d2 to OTHER points
template <int KMAX, bool FMA>
struct OutlList {
  uint32_t (&L)[KMAX];
  const KnnSlot &S;
  const float4 q;
  const uint32_t qi;
  __device__ __forceinline__ void visit(const float4 p, const uint32_t j)
  {
    const uint32_t key = knn_index_of(S, p, j) == qi ? kListInit : __float_as_uint(knn_dist2<FMA>(p, q));      // the query itself: never below the k-th
    if (key < L[KMAX - 1]) outl_insert<KMAX>(L, key);
  }
  __device__ __forceinline__ bool full() const { return L[KMAX - 1] != kListInit; }
  // at or beyond the k-th distance: a tie could only replace an equal value
  __device__ __forceinline__ bool beyond(const double b2) const { return b2 >= (double)__uint_as_float(L[KMAX - 1]); }
};

// mean distance to the k nearest other points
template <int KMAX, bool FMA>
__global__ void __launch_bounds__(kOutlThreads) outl_mean_dist_kernel(OutlArgs a)
{
  float4 q; uint32_t qi;
  if (!knn_query(a.S, &q, &qi)) return;
  const int k = a.k;
  uint32_t L[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) L[i] = i < KMAX - k ? 0u : kListInit;
  OutlList<KMAX, FMA> v{L, a.S, q, qi};
  knn_shell_walk(a.S, q, v);
  // the caller runs this kernel only when the cloud holds at least k other points, and every query is finite: the list is full
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
    if (i >= KMAX - k) sum += (double)sqrtf(__uint_as_float(L[i]));
  a.mean_dist[a.remap ? a.remap[qi] : qi] = (float)(sum / (double)k);
}

// the number of other points with d2 <= r2
template <bool FMA>
__global__ void __launch_bounds__(kOutlThreads) outl_count_kernel(OutlArgs a)
{
  float4 q; uint32_t qi;
  if (!knn_query(a.S, &q, &qi)) return;
  uint32_t cnt = 0;
  knn_ball_walk<FMA>(a.S, q, a.r2, [&](const float4 p, const uint32_t j) { if (knn_index_of(a.S, p, j) != qi) ++cnt; });
  a.count[a.remap ? a.remap[qi] : qi] = cnt;
}

// ---- statistics: stats[0] = mean, [1] = stddev, [2] = threshold
__device__ __forceinline__ double outl_block_sum(double v)
{
  __shared__ double s[kOutlThreads];
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = kOutlThreads / 2; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
  return s[0];
}

// PASS 0: partial[b] = sum of the mean distances of block b's chunk; PASS 1: of their squared deviations from stats[0]
template <int PASS>
__global__ void __launch_bounds__(kOutlThreads) outl_sum_kernel(const float *__restrict__ md, const uint8_t *__restrict__ fin, size_t n, size_t chunk,
                                                                const double *__restrict__ stats, double *__restrict__ partial)
{
  const size_t b0 = (size_t)blockIdx.x * chunk, b1 = b0 + chunk < n ? b0 + chunk : n;
  const double mean = PASS ? stats[0] : 0.0;
  double acc = 0.0;
  for (size_t i = b0 + threadIdx.x; i < b1; i += kOutlThreads) {
    if (!fin[i]) continue;
    const double v = (double)md[i] - mean;
    acc += PASS ? v * v : v;
  }
  const double tot = outl_block_sum(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <int PASS>
__global__ void __launch_bounds__(kOutlThreads) outl_final_kernel(const double *__restrict__ partial, unsigned nb, double n_valid, double stddev_mul,
                                                                  double *__restrict__ stats)
{
  double acc = 0.0;
  for (unsigned i = threadIdx.x; i < nb; i += kOutlThreads) acc += partial[i];
  const double tot = outl_block_sum(acc);
  if (threadIdx.x) return;
  if (PASS == 0) stats[0] = tot / n_valid;
  else {
    const double sd = sqrt(tot / (n_valid - 1.0));      // one point: 0 / 0 = NaN, as PCL
    stats[1] = sd;
    stats[2] = stats[0] + stddev_mul * sd;
  }
}

// sel[i]: point i goes to the output.  thr null: every finite point is an inlier (no point has a mean distance)
__global__ void __launch_bounds__(kOutlThreads) outl_flag_dist_kernel(const float *__restrict__ md, const uint8_t *__restrict__ fin, size_t n,
                                                                      const double *__restrict__ thr, int negative, uint8_t *__restrict__ sel)
{
  const size_t i = (size_t)blockIdx.x * kOutlThreads + threadIdx.x;
  if (i >= n) return;
  bool in = fin[i] != 0;
  if (in && thr) in = !((double)md[i] > thr[2]);
  sel[i] = (in != (negative != 0)) ? 1 : 0;
}

__global__ void __launch_bounds__(kOutlThreads) outl_flag_count_kernel(const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ fin, size_t n,
                                                                       uint32_t min_neighbors, int negative, uint8_t *__restrict__ sel)
{
  const size_t i = (size_t)blockIdx.x * kOutlThreads + threadIdx.x;
  if (i >= n) return;
  const bool in = fin[i] != 0 && cnt[i] >= min_neighbors;
  sel[i] = (in != (negative != 0)) ? 1 : 0;
}

template <bool FMA>
void launch_search(int kmax, const OutlArgs &a, hipStream_t st)
{
  const dim3 grid(blocks_for(a.S.nq, kOutlThreads)), block(kOutlThreads);
  switch (kmax) {
    case 0:  hipLaunchKernelGGL(outl_count_kernel<FMA>, grid, block, 0, st, a); break;
    case 8:  hipLaunchKernelGGL((outl_mean_dist_kernel<8, FMA>), grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL((outl_mean_dist_kernel<16, FMA>), grid, block, 0, st, a); break;
    case 32: hipLaunchKernelGGL((outl_mean_dist_kernel<32, FMA>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((outl_mean_dist_kernel<64, FMA>), grid, block, 0, st, a); break;
  }
}

// the compacted copy of the finite points: lives for one call
struct WorkCloud {
  Cloud cl; hipStream_t stream;
  explicit WorkCloud(hipStream_t s) : stream(s) {}
  ~WorkCloud() { if (cl.pts) { (void)hipStreamSynchronize(stream); (void)hipFree(cl.pts); } }
};

// both filters: k > 0 = mean distances over the k nearest, k == 0 = neighbour counts within sqrt(r2)
int outlier_filter(Ctx *c, Cloud &dst, Cloud &src, int k, double stddev_mul, float r2, uint32_t min_neighbors, bool negative, bool fma,
                   size_t *n_out, uint32_t *kept_index, void *per_point, mvr_sor_stats *stats)
{
  const size_t n = src.n;
  const bool normals = src.has_normals, dist = k > 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double hs[4] = {nan, nan, nan, 0.0};
  size_t n_valid = 0, kept = 0;
  if (int rc = knn_cloud_ok(c, src, "outlier removal")) return rc;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "outlier removal reads back");
    size_t sel_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    const unsigned nb = std::min(kOutlSumBlocks, blocks_for(n, kOutlThreads));
    const size_t chunk = (n + nb - 1) / nb;
    Carver plan;
    plan.plan<uint8_t>(n); plan.plan<uint8_t>(n); plan.plan<uint32_t>(n); plan.plan<unsigned long long>(n); plan.plan<uint32_t>(n);
    plan.plan<uint32_t>(4); plan.plan<double>(nb); plan.plan<double>(4); plan.plan<float4>(n); plan.plan<uint32_t>(n); plan.plan<char>(sel_bytes);
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    uint8_t *fin = s.take<uint8_t>(n), *sel = s.take<uint8_t>(n);
    uint32_t *val = s.take<uint32_t>(n);
    unsigned long long *list = s.take<unsigned long long>(n);
    uint32_t *remap = s.take<uint32_t>(n), *counters = s.take<uint32_t>(4);
    double *partial = s.take<double>(nb), *dstats = s.take<double>(4);
    float4 *out = s.take<float4>(n);
    uint32_t *d_index = s.take<uint32_t>(n);
    char *tmp = s.take<char>(sel_bytes);
    // 1. finite points
    const float fnan = std::numeric_limits<float>::quiet_NaN();
    uint32_t preset = 0, hc[4] = {0, 0, 0, 0};
    if (dist) std::memcpy(&preset, &fnan, 4);
    MVR_HIP_TRY(c, hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(outl_finite_kernel, dim3(blocks_for(n, kOutlThreads)), dim3(kOutlThreads), 0, c->stream, src.pts, n, fin, val, preset, counters);
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t nf = hc[0];
    WorkCloud wc(c->stream);
    Cloud *work = &src;
    const uint32_t *d_remap = nullptr;
    // 2. the search, when there is anything to find: a mean distance needs k OTHER finite points
    const bool run = dist ? nf >= (size_t)k + 1 : nf > 0;
    if (run && nf < n) {
      if (int rc = select_flagged(c, tmp, sel_bytes, fin, n, list, counters + 1)) return rc;
      if (int rc = cloud_reserve(c, wc.cl, nf, false)) return rc;
      if (int rc = launch_gather(c, src.pts, list, nf, wc.cl.pts, remap)) return rc;
      wc.cl.n = nf;
      work = &wc.cl; d_remap = remap;
    }
    if (run) {
      OutlArgs a{};
      if (int rc = fill_target(c, *work, a.S)) return rc;
      fill_queries(*work, a.S);
      a.remap = d_remap; a.mean_dist = reinterpret_cast<float *>(val); a.count = val; a.k = k; a.r2 = r2;
      if (fma) launch_search<true>(dist ? kmax_bucket(k) : 0, a, c->stream);
      else launch_search<false>(dist ? kmax_bucket(k) : 0, a, c->stream);
      MVR_HIP_TRY(c, hipGetLastError());
    }
    // 3. statistics and flags
    const float *md = reinterpret_cast<const float *>(val);
    if (dist && run) {
      n_valid = nf;
      hipLaunchKernelGGL(outl_sum_kernel<0>, dim3(nb), dim3(kOutlThreads), 0, c->stream, md, fin, n, chunk, dstats, partial);
      hipLaunchKernelGGL(outl_final_kernel<0>, dim3(1), dim3(kOutlThreads), 0, c->stream, partial, nb, (double)nf, stddev_mul, dstats);
      hipLaunchKernelGGL(outl_sum_kernel<1>, dim3(nb), dim3(kOutlThreads), 0, c->stream, md, fin, n, chunk, dstats, partial);
      hipLaunchKernelGGL(outl_final_kernel<1>, dim3(1), dim3(kOutlThreads), 0, c->stream, partial, nb, (double)nf, stddev_mul, dstats);
    }
    if (dist) hipLaunchKernelGGL(outl_flag_dist_kernel, dim3(blocks_for(n, kOutlThreads)), dim3(kOutlThreads), 0, c->stream, md, fin, n,
                                 run ? dstats : (const double *)nullptr, negative ? 1 : 0, sel);
    else hipLaunchKernelGGL(outl_flag_count_kernel, dim3(blocks_for(n, kOutlThreads)), dim3(kOutlThreads), 0, c->stream, val, fin, n, min_neighbors, negative ? 1 : 0, sel);
    MVR_HIP_TRY(c, hipGetLastError());
    // 4. the selected indices, ascending; the one read-back of the chain
    if (int rc = select_flagged(c, tmp, sel_bytes, sel, n, list, counters + 2)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    if (dist && run) MVR_HIP_TRY(c, hipMemcpyAsync(hs, dstats, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (per_point) MVR_HIP_TRY(c, hipMemcpyAsync(per_point, val, n * 4, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    kept = hc[2];
    // 5. the output
    if (int rc = gather_kept(c, dst, src.pts, normals ? src.nrm : nullptr, list, kept, out, d_index)) return rc;
    if (kept_index && kept) MVR_HIP_TRY(c, hipMemcpyAsync(kept_index, d_index, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // kept_index is complete on return, and the arena is free again
  }
  finish_dst(c, dst, kept, normals);
  if (n_out) *n_out = kept;
  if (stats) { stats->mean = hs[0]; stats->stddev = hs[1]; stats->threshold = hs[2]; stats->n_valid = n_valid; }
  return MVR_OK;
}

}  // namespace

}  // namespace mvr

using namespace mvr;

API int mvr_cloud_statistical_outlier_removal(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_sor_params *p, size_t *n_out,
                                              uint32_t *kept_index, float *mean_dist, mvr_sor_stats *stats)
{
  if (!ctx || !p || !slot_ok(dst_slot) || !slot_ok(src_slot)) return MVR_E_ARG;
  if (p->mean_k < 1 || p->mean_k > MVR_MAX_KNN || !std::isfinite(p->stddev_mul)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return outlier_filter(c, c->slots[dst_slot], c->slots[src_slot], p->mean_k, p->stddev_mul, 0.f, 0u, p->negative != 0, p->fma_dist != 0, n_out,
                        kept_index, mean_dist, stats);
}

API int mvr_cloud_radius_outlier_removal(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_ror_params *p, size_t *n_out,
                                         uint32_t *kept_index, uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(dst_slot) || !slot_ok(src_slot)) return MVR_E_ARG;
  if (!(std::isfinite(p->radius) && p->radius > 0.0) || p->min_neighbors < 0) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return outlier_filter(c, c->slots[dst_slot], c->slots[src_slot], 0, 0.0, (float)(p->radius * p->radius), (uint32_t)p->min_neighbors,
                        p->negative != 0, p->fma_dist != 0, n_out, kept_index, neighbor_count, nullptr);
}
