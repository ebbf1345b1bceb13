// csrc/mvr_fpfh.hip -- pcl::FPFHEstimation (radius search, the cloud its own search surface) on the GPU (gfx950); the rules F1-F8
// are written next to mvr_cloud_fpfh in mvr_hip.h.
//
// One thread per query, in the order of the cloud's model grid (ensure_model_grid; the helpers of mvr_knn_walk.h), so the 64
// lanes of a wave are neighbours on the surface and walk the same cells.  Every table a walk reads lies in GRID order, so a
// neighbour found at grid position j has its normal and its SPFH row at j and the neighbours of one cell are consecutive rows:
//   1. valid_normals_kernel (mvr_pair_features.h, where the pair features F3 / F4 stand that mvr_pfh.hip shares) copies the
//      slot's normals from index order to grid order; w = 1 marks a valid point (finite coordinates and a finite normal),
//      w = 0 an invalid one, which every later walk skips.
//   2. fpfh_spfh_kernel: the ball walk (knn_ball_walk) computes the three f32 pair features of every neighbour and counts them
//      into 3 x 11 bins.  The bin index is a runtime value, and a runtime-indexed private array lives in scratch memory
//      (mvr_knn.hip), so the 33 u32 counters of a thread lie in LDS as hist[bin][thread]: lane t reads and writes the address
//      bin * 256 + t, which is bank t mod 32 whatever its bin -- no two lanes of a 32-lane group share a bank -- and the
//      counters are private, so plain read-modify-write is enough.  33 KiB per block of 256.  The row, scaled by
//      100 / (n_i - 1), is written at the query's grid position.
//   3. fpfh_weight_kernel: the same walk; per neighbour the 33 floats of its SPFH row times 1 / d2 (f32), added in f64 to
//      33 bin and 3 block sums that are registers (compile-time indices).  The signature is written by source index.
//   4. fpfh_rows_kernel moves the SPFH table from grid order to index order when the caller asked for it.
// mvr_cloud_fpfh_at (rules Q1-Q8) answers chosen queries over a surface, with the SPFH ON DEMAND, as PCL's computeSPFHSignatures
// does for the union of the queries' neighbours: after step 1, the marking walk (at_mark_kernel, mvr_at.hip) takes the ball of
// every query of the query array (at_queries, mvr_knn_walk.h), counts n_i and stores need[j] = 1 for every valid neighbour at grid position j (plain stores of one
// constant; racing stores of the same value need no atomic); hipCUB's flagged selection lists the needed positions in ascending
// order (the lanes of a wave stay neighbours on the surface); step 2 runs over that list -- the same kernel, its position taken
// from the list -- and step 3 over the query array, writing by output row.  The SPFH table stays [n_surface][33] by grid
// position.  INVARIANT: a row that was not computed is never read -- step 3 reads row j only for a valid neighbour j of some
// query, and the mark kernel, which makes the same walk with the same test, marked every such j.  A row is the surface point's
// own SPFH in the surface, so a query at a surface point gets the bits mvr_cloud_fpfh gives that point (Q5).
// No atomics and a fixed walk order: bit-identical from run to run on one grid.  Compiled with -ffp-contract=off (every f32
// operation of the pair features is rounded as written).
#include <cmath>
#include <cstring>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_pair_features.h"

namespace mvr {
namespace {

constexpr int kFpfhThreads = kKnnThreads;
constexpr int kBins = MVR_FPFH_BINS, kRow = 3 * MVR_FPFH_BINS;

struct FpfhArgs {
  KnnSlot S;                       // the cloud searched against itself; at, in the mark and weight steps: the query array over the surface
  const float4 *src_nrm;           // the slot's normals, by index
  float4 *gn;                      // normals by grid position, w = 1 for a valid point, else 0
  float *spfh;                     // [n][33] by grid position
  float *out;                      // [n][33] by index: the signature
  uint32_t *count;                 // n_i by index (at: by output row, written by the mark step; null in the SPFH step)
  float r2;
  int at;                          // mvr_cloud_fpfh_at: a query is valid iff finite (Q2), an empty neighbourhood gives NaN (Q4)
  const unsigned long long *list;  // the SPFH step of at: the grid positions to compute, n_list of them; null: all S.nq
  uint32_t n_list;
};

template <bool FMA>
__global__ void __launch_bounds__(kFpfhThreads) fpfh_spfh_kernel(FpfhArgs a)
{
  __shared__ uint32_t hist[kRow * kFpfhThreads];      // [bin][thread]: private counters, every lane on its own bank
  const KnnSlot &S = a.S;
  const uint32_t tid = threadIdx.x, t = blockIdx.x * kFpfhThreads + tid;
  if (t >= (a.list ? a.n_list : S.nq)) return;
  const uint32_t pos = a.list ? (uint32_t)a.list[t] : t;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  const float4 ni = a.gn[pos];
  float *row = a.spfh + (size_t)pos * kRow;
  if (ni.w == 0.f) {                                  // F1 (an invalid query walks nothing)
#pragma unroll
    for (int k = 0; k < kRow; ++k) row[k] = __builtin_nanf("");
    if (a.count) a.count[qi] = 0u;
    return;
  }
#pragma unroll
  for (int k = 0; k < kRow; ++k) hist[k * kFpfhThreads + tid] = 0u;
  uint32_t n = 0;
  knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 p, const uint32_t j) {
    const float4 nj = a.gn[j];
    if (nj.w == 0.f) return;
    ++n;
    if (j == pos) return;
    float f1, f2, f3;
    if (!pair_features(q, ni, p, nj, &f1, &f2, &f3)) return;      // F3
    int b1, b2, b3;
    pair_bins<kBins>(f1, f2, f3, &b1, &b2, &b3);                  // F4, F5
    hist[b1 * kFpfhThreads + tid] += 1u;
    hist[(kBins + b2) * kFpfhThreads + tid] += 1u;
    hist[(2 * kBins + b3) * kFpfhThreads + tid] += 1u;
  });
  const float scale = n > 1u ? 100.0f / (float)(n - 1u) : 0.f;
#pragma unroll
  for (int k = 0; k < kRow; ++k) row[k] = (float)hist[k * kFpfhThreads + tid] * scale;
  if (a.count) a.count[qi] = n;
}

template <bool FMA>
__global__ void __launch_bounds__(kFpfhThreads) fpfh_weight_kernel(FpfhArgs a)
{
  const KnnSlot &S = a.S;
  const uint32_t pos = blockIdx.x * kFpfhThreads + threadIdx.x;
  if (pos >= S.nq) return;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  float *out = a.out + (size_t)qi * kRow;
  if (a.at ? a.count[qi] == 0u : a.gn[pos].w == 0.f) {      // (at: an invalid query walked nothing and counted 0)
#pragma unroll
    for (int k = 0; k < kRow; ++k) out[k] = __builtin_nanf("");
    return;
  }
  double acc[kRow], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kRow; ++k) acc[k] = 0.0;
  knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 p, const uint32_t j) {
    if (a.gn[j].w == 0.f) return;
    const float d2 = knn_dist2<FMA>(p, q);
    if (d2 == 0.f) return;                            // (the query itself among them)
    const float w = 1.0f / d2;
    if (!isfinite(w)) return;
    const float *r = a.spfh + (size_t)j * kRow;
#pragma unroll
    for (int k = 0; k < kRow; ++k) {
      const double val = (double)(r[k] * w);
      acc[k] += val;
      sum[k / kBins] += val;
    }
  });
#pragma unroll
  for (int k = 0; k < kRow; ++k) {
    const double s = sum[k / kBins];
    out[k] = s != 0.0 ? (float)(acc[k] * (100.0 / s)) : 0.f;
  }
}

// the SPFH table from grid order to index order: one thread per float
__global__ void __launch_bounds__(kFpfhThreads) fpfh_rows_kernel(FpfhArgs a, float *__restrict__ by_index)
{
  const KnnSlot &S = a.S;
  const size_t e = (size_t)blockIdx.x * kFpfhThreads + threadIdx.x;
  if (e >= (size_t)S.nq * kRow) return;
  const uint32_t pos = (uint32_t)(e / kRow), k = (uint32_t)(e % kRow);
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(S.qs[pos].w);
  by_index[(size_t)qi * kRow + k] = a.spfh[e];
}

int fpfh_cloud(Ctx *c, Cloud &cl, const mvr_fpfh_params &p, float *fpfh, float *spfh, uint32_t *neighbor_count)
{
  const size_t n = cl.n;
  if (!cl.has_normals && n > 0) return set_error(c, MVR_E_ARG, "fpfh: the slot has no normals");
  if (int rc = knn_cloud_ok(c, cl, "fpfh")) return rc;
  if (n == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "fpfh reads back");
  FpfhArgs a{};
  if (int rc = fill_target(c, cl, a.S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
  fill_queries(cl, a.S);
  const size_t m = n * (size_t)kRow;
  Carver plan;
  plan.plan<float4>(n); plan.plan<float>(m); plan.plan<float>(m); plan.plan<uint32_t>(n); plan.plan<float>(spfh ? m : 1);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  a.src_nrm = cl.nrm;
  a.gn = s.take<float4>(n);
  a.spfh = s.take<float>(m);
  a.out = s.take<float>(m);
  a.count = s.take<uint32_t>(n);
  float *rows = s.take<float>(spfh ? m : 1);
  a.r2 = clamp_r2(p.radius);
  const dim3 grid(blocks_for(n, kFpfhThreads)), block(kFpfhThreads);
  hipLaunchKernelGGL(valid_normals_kernel<kFpfhThreads>, grid, block, 0, c->stream, a.S, a.src_nrm, a.gn);
  MVR_HIP_TRY(c, hipGetLastError());
  if (p.fma_dist) hipLaunchKernelGGL(fpfh_spfh_kernel<true>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(fpfh_spfh_kernel<false>, grid, block, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  if (p.fma_dist) hipLaunchKernelGGL(fpfh_weight_kernel<true>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(fpfh_weight_kernel<false>, grid, block, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  if (spfh) {
    hipLaunchKernelGGL(fpfh_rows_kernel, dim3(blocks_for(m, kFpfhThreads)), block, 0, c->stream, a, rows);
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipMemcpyAsync(spfh, rows, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (fpfh) MVR_HIP_TRY(c, hipMemcpyAsync(fpfh, a.out, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (neighbor_count) MVR_HIP_TRY(c, hipMemcpyAsync(neighbor_count, a.count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  return MVR_OK;
}

// the events of tune key "at_clock": five marks on the stream around the four stages
struct StageClock {
  hipEvent_t ev[5] = {};
  int n = 0;
  bool on;
  explicit StageClock(bool o) : on(o) {}
  ~StageClock() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
  void mark(hipStream_t st)
  {
    if (on && n < 5 && hipEventCreate(&ev[n]) == hipSuccess) { (void)hipEventRecord(ev[n], st); ++n; }
  }
  void read(float *ms) const      // (after the stream was waited for)
  {
    for (int i = 0; i < 4; ++i) { ms[i] = 0.f; if (i + 1 < n) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]); }
  }
};

// the queries of rules Q1 / Q2 -- the points `indices` of qc (null: all of them) -- over the surface cl; the refusals are the caller's
int fpfh_at_cloud(Ctx *c, Cloud &cl, const Cloud &qc, const uint32_t *indices, size_t n_indices, const mvr_fpfh_params &p, float *fpfh,
                  uint32_t *neighbor_count)
{
  const size_t ns = cl.n, rows = indices ? n_indices : qc.n;
  c->fpfh_at_marked = 0;
  if (rows == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "fpfh reads back");
  FpfhArgs a{};
  if (int rc = fill_target(c, cl, a.S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
  fill_queries(cl, a.S);
  const KnnSlot self = a.S;
  AtQueries Q;
  if (int rc = at_queries(c, qc, &qc == &cl, indices, n_indices, self, &Q)) return rc;
  const size_t m = rows * (size_t)kRow;
  size_t sel_bytes = 0;
  if (ns > 0)
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, ns, nullptr, nullptr)) return rc;
  Carver plan;
  plan.plan<float4>(ns); plan.plan<float>(ns * (size_t)kRow); plan.plan<float>(m); plan.plan<uint32_t>(rows); plan.plan<uint8_t>(ns);
  plan.plan<unsigned long long>(ns); plan.plan<uint32_t>(1); plan.plan<char>(sel_bytes);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  a.src_nrm = cl.nrm;
  a.gn = s.take<float4>(ns);
  a.spfh = s.take<float>(ns * (size_t)kRow);
  a.out = s.take<float>(m);
  a.count = s.take<uint32_t>(rows);
  uint8_t *need = s.take<uint8_t>(ns);
  unsigned long long *list = s.take<unsigned long long>(ns);
  uint32_t *d_listed = s.take<uint32_t>(1);
  char *sel_tmp = s.take<char>(sel_bytes);
  a.r2 = clamp_r2(p.radius);
  a.at = 1;
  const dim3 block(kFpfhThreads), qgrid(blocks_for(rows, kFpfhThreads));
  FpfhArgs aq = a;                                        // the mark and weight steps: the query array over the surface
  aq.S.qs = Q.q; aq.S.q_by_pos = 0u; aq.S.nq = (uint32_t)rows;
  uint32_t listed = 0;
  if (ns > 0) {
    hipLaunchKernelGGL(valid_normals_kernel<kFpfhThreads>, dim3(blocks_for(ns, kFpfhThreads)), block, 0, c->stream, self, a.src_nrm, a.gn);
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipMemsetAsync(need, 0, ns, c->stream));
  }
  StageClock clock(c->at_clock != 0);
  clock.mark(c->stream);
  if (int rc = launch_at_mark(c, aq.S, a.gn, a.r2, p.fma_dist != 0, a.count, need)) return rc;
  clock.mark(c->stream);
  if (ns > 0) {
    if (int rc = select_flagged(c, sel_tmp, sel_bytes, need, ns, list, d_listed)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(&listed, d_listed, sizeof listed, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->fpfh_at_marked = listed;
  clock.mark(c->stream);
  if (listed) {
    FpfhArgs as = a;                                      // the SPFH step: the surface against itself, at the listed positions
    as.count = nullptr; as.list = list; as.n_list = listed;
    const dim3 sgrid(blocks_for(listed, kFpfhThreads));
    if (p.fma_dist) hipLaunchKernelGGL(fpfh_spfh_kernel<true>, sgrid, block, 0, c->stream, as);
    else hipLaunchKernelGGL(fpfh_spfh_kernel<false>, sgrid, block, 0, c->stream, as);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  clock.mark(c->stream);
  if (p.fma_dist) hipLaunchKernelGGL(fpfh_weight_kernel<true>, qgrid, block, 0, c->stream, aq);
  else hipLaunchKernelGGL(fpfh_weight_kernel<false>, qgrid, block, 0, c->stream, aq);
  MVR_HIP_TRY(c, hipGetLastError());
  clock.mark(c->stream);
  if (fpfh) MVR_HIP_TRY(c, hipMemcpyAsync(fpfh, a.out, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (neighbor_count) MVR_HIP_TRY(c, hipMemcpyAsync(neighbor_count, a.count, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  clock.read(c->fpfh_at_ms);
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API int mvr_cloud_fpfh(mvr_ctx *ctx, int slot, const mvr_fpfh_params *p, float *fpfh, float *spfh, uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(slot)) return MVR_E_ARG;
  if (!(std::isfinite(p->radius) && p->radius > 0.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return fpfh_cloud(c, c->slots[slot], *p, fpfh, spfh, neighbor_count);
}

API int mvr_cloud_fpfh_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot, const mvr_fpfh_params *p, float *fpfh,
                          uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(q_slot) || !slot_ok(surface_slot)) return MVR_E_ARG;
  if (!(std::isfinite(p->radius) && p->radius > 0.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[q_slot], &t = c->slots[surface_slot];
  if (!indices && q_slot == surface_slot) return fpfh_cloud(c, t, *p, fpfh, nullptr, neighbor_count);      // Q8
  if (!t.has_normals && t.n > 0) return set_error(c, MVR_E_ARG, "fpfh: the surface slot has no normals");
  if (int rc = knn_cloud_ok(c, q, "fpfh")) return rc;
  if (int rc = knn_cloud_ok(c, t, "fpfh")) return rc;
  if (int rc = at_indices_ok(c, q, indices, n_indices, "fpfh")) return rc;
  return fpfh_at_cloud(c, t, q, indices, n_indices, *p, fpfh, neighbor_count);
}
