// csrc/mvr_sac.hip -- pcl::SACSegmentation (SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC) and pcl::ExtractIndices
// on the GPU (gfx950); the rules P1-P12 are written next to mvr_cloud_segment_plane in mvr_hip.h.
//
// The chunked RANSAC -- the draws, the counting kernel, the host's replay of PCL's loop -- is mvr_ransac.h; what this file adds:
//   1. sac_valid_kernel + select_flagged: the valid points' indices, ascending, and their number (one read-back per call).
//   2. per chunk: sac_hypotheses_kernel, one thread per attempt -- draws, the three points through the list of valid indices,
//      the plane of P3 and the test of P4 --, then the counting kernel over PlaneModel (an item is a point's x, y, z of its
//      16-byte record, a hypothesis one float4 plane, four per step; an invalid point has a non-finite distance), then ONE
//      read-back of the chunk's records and counts.
//   3. sac_flag_kernel: P5 for one plane, read from device memory (the refined plane never visits the host in between);
//      sac_moments_kernel + sac_fit_kernel: the fixed-order f64 sums of P10 and the Jacobi fit of mvr_plane.h.
//   4. the tail of every filter that keeps a subset: select_flagged, gather_kept, finish_dst (mvr_denoise.hip).
// Everything runs on the context's stream; the work arrays come out of the context's arena (Ctx::dn_arena).
#include <cmath>
#include <cstring>
#include <vector>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_plane.h"
#include "mvr_ransac.h"

namespace mvr {
namespace {

// P5
template <bool FMA>
__device__ __forceinline__ float sac_distance(const float ca, const float cb, const float cc, const float cd, const float x, const float y,
                                              const float z)
{
  float t = ca * x;
  if (FMA) { t = fmaf(cb, y, t); t = fmaf(cc, z, t); }
  else { t = t + cb * y; t = t + cc * z; }
  return t + cd;
}

// the plane to the counting kernel of mvr_ransac.h
struct PlaneModel {
  static constexpr int kHypPerStep = 4, kBlocksPerCu = 8;
  struct Item { float x, y, z; };
  using Hyp = float4;
  static __device__ __forceinline__ Item item(const float4 *__restrict__ pts, uint32_t i, bool pad)
  {
    const float4 p = pts[i];
    return {pad ? NAN : p.x, p.y, p.z};
  }
  static __device__ __forceinline__ Hyp hyp(const float4 *__restrict__ coef, uint32_t h) { return coef[h]; }
  template <bool FMA>
  static __device__ __forceinline__ bool inlier(const Hyp c, const Item p, float bound)
  {
    return fabsf(sac_distance<FMA>(c.x, c.y, c.z, c.w, p.x, p.y, p.z)) < bound;
  }
};

// what the host reads back of an attempt
struct SacHyp { float coef[4]; uint32_t sample[3]; int status; };
static_assert(sizeof(SacHyp) == 32, "SacHyp is read back as it is");

__global__ void sac_valid_kernel(const float4 *__restrict__ p, size_t n, uint8_t *__restrict__ valid)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) valid[i] = finite3(p[i]) ? 1 : 0;
}

struct HypArgs {
  const float4 *pts; const unsigned long long *vlist; uint32_t nv;
  uint64_t seed, t0; uint32_t count;
  int model; double ax, ay, az, na, cos_eps;      // P4: the axis, its length and cos(eps_angle)
  SacHyp *hyp; float4 *coef; uint32_t *counts;
};

__global__ void __launch_bounds__(64) sac_hypotheses_kernel(HypArgs a)
{
  const uint32_t h = blockIdx.x * 64 + threadIdx.x;
  if (h >= a.count) {      // the planes that pad the chunk to a multiple of PlaneModel::kHypPerStep: nobody's inlier
    if (h < ransac_padded<PlaneModel>(a.count)) a.coef[h] = make_float4(NAN, NAN, NAN, NAN);
    return;
  }
  uint32_t r[3];
  ransac_draw3(a.seed, a.t0 + h, a.nv, r);      // P2
  SacHyp out;
  out.sample[0] = (uint32_t)a.vlist[r[0]]; out.sample[1] = (uint32_t)a.vlist[r[1]]; out.sample[2] = (uint32_t)a.vlist[r[2]];
  const float4 p0 = a.pts[out.sample[0]], p1 = a.pts[out.sample[1]], p2 = a.pts[out.sample[2]];
  // P3
  const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z, e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float len2 = (nx * nx + ny * ny) + nz * nz, len = sqrtf(len2);
  const float ca = nx / len, cb = ny / len, cc = nz / len;
  const float cd = -((ca * p0.x + cb * p0.y) + cc * p0.z);
  int status = (len2 > 0.f && isfinite(ca) && isfinite(cb) && isfinite(cc) && isfinite(cd)) ? 1 : 0;
  if (status == 1 && a.model == 1) {      // P4
    const double da = ca, db = cb, dc = cc;
    const double cs = fabs((da * a.ax + db * a.ay) + dc * a.az) / (sqrt((da * da + db * db) + dc * dc) * a.na);
    if (cs < a.cos_eps) status = 3;
  }
  out.coef[0] = status ? ca : 0.f; out.coef[1] = status ? cb : 0.f; out.coef[2] = status ? cc : 0.f; out.coef[3] = status ? cd : 0.f;
  out.status = status;
  a.hyp[h] = out;
  // what the counting kernel scores: a skipped or invalid attempt has no inliers (P3, P4), so its plane is NaN there
  a.coef[h] = status == 1 ? make_float4(ca, cb, cc, cd) : make_float4(NAN, NAN, NAN, NAN);
  a.counts[h] = 0u;
}

template <bool FMA>
__global__ void sac_flag_kernel(const float4 *__restrict__ pts, size_t n, const float4 *__restrict__ coef, float bound, uint8_t *__restrict__ flag,
                                uint8_t *__restrict__ nflag)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 c = *coef, p = pts[i];
  const bool in = PlaneModel::inlier<FMA>(c, {p.x, p.y, p.z}, bound);
  flag[i] = in ? 1 : 0;
  nflag[i] = in ? 0 : 1;
}

// P10: one row of ten partial sums (count, first and second moments about q) per block of 256 consecutive original indices
constexpr int kSacMoments = 10;
__global__ void __launch_bounds__(256) sac_moments_kernel(const float4 *__restrict__ pts, size_t n, const uint8_t *__restrict__ flag, const float4 *__restrict__ qp,
                                                          double *__restrict__ partials)
{
  __shared__ double sh[kSacMoments][256];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t tid = threadIdx.x;
  double v[kSacMoments];
#pragma unroll
  for (int k = 0; k < kSacMoments; ++k) v[k] = 0.0;
  if (i < n && flag[i]) {
    const float4 p = pts[i], q = *qp;
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    v[0] = 1.0; v[1] = dx; v[2] = dy; v[3] = dz;
    v[4] = dx * dx; v[5] = dx * dy; v[6] = dx * dz; v[7] = dy * dy; v[8] = dy * dz; v[9] = dz * dz;
  }
#pragma unroll
  for (int k = 0; k < kSacMoments; ++k) sh[k][tid] = v[k];
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int k = 0; k < kSacMoments; ++k) sh[k][tid] += sh[k][tid + s];
    __syncthreads();
  }
  if (tid < (uint32_t)kSacMoments) partials[(size_t)blockIdx.x * kSacMoments + tid] = sh[tid][0];
}

// what the fit leaves on the device: fit[0] = the RANSAC plane (written by the host), fit[1] = the final plane
struct SacFit { float4 plane[2]; float4 q; uint32_t ransac_inliers, refined; };

// One block.  The partials are added in ascending order by one lane per moment (P10), which is a chain of dependent f64 additions;
// what need not wait is the memory: the block copies kSacFitRows rows at a time into LDS with coalesced loads, and the ten lanes
// add from there (the merged object has 9 400 rows: one lane reading them from global memory took 1.5 ms).
constexpr int kSacFitThreads = 256, kSacFitRows = 256;
__global__ void __launch_bounds__(kSacFitThreads) sac_fit_kernel(const double *__restrict__ partials, uint32_t blocks, SacFit *fit)
{
  __shared__ double stage[kSacFitRows * kSacMoments];
  __shared__ double sum[kSacMoments];
  double s = 0.0;
  for (uint32_t base = 0; base < blocks; base += kSacFitRows) {
    const uint32_t rows = blocks - base < (uint32_t)kSacFitRows ? blocks - base : (uint32_t)kSacFitRows;
    for (uint32_t e = threadIdx.x; e < rows * kSacMoments; e += kSacFitThreads) stage[e] = partials[(size_t)base * kSacMoments + e];
    __syncthreads();
    if (threadIdx.x < (uint32_t)kSacMoments) {
#pragma unroll 8
      for (uint32_t r = 0; r < rows; ++r) s += stage[r * kSacMoments + threadIdx.x];      // ascending
    }
    __syncthreads();
  }
  if (threadIdx.x < (uint32_t)kSacMoments) sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float4 r = fit->plane[0], q = fit->q;
  float4 out = r;
  uint32_t refined = 0u;
  if (sum[0] >= 3.0) {
    Moments M;
    M.cnt = sum[0]; M.sx = sum[1]; M.sy = sum[2]; M.sz = sum[3];
    M.xx = sum[4]; M.xy = sum[5]; M.xz = sum[6]; M.yy = sum[7]; M.yz = sum[8]; M.zz = sum[9];
    const PlaneFit f = plane_fit(M);
    double nx = f.nx, ny = f.ny, nz = f.nz;
    if ((nx * (double)r.x + ny * (double)r.y) + nz * (double)r.z < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double mx = (double)q.x + f.m0, my = (double)q.y + f.m1, mz = (double)q.z + f.m2;
    const double d = -((nx * mx + ny * my) + nz * mz);
    const float4 o = make_float4((float)nx, (float)ny, (float)nz, (float)d);
    if (isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(o.w)) { out = o; refined = 1u; }
  }
  fit->plane[1] = out;
  fit->ransac_inliers = (uint32_t)sum[0];
  fit->refined = refined;
}

__global__ void sac_low_words_kernel(const unsigned long long *__restrict__ list, size_t n, uint32_t *__restrict__ out)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = (uint32_t)list[k];
}

int launch_flags(Ctx *c, bool fma, const float4 *pts, size_t n, const float4 *coef, float bound, uint8_t *flag, uint8_t *nflag)
{
  if (fma) hipLaunchKernelGGL(sac_flag_kernel<true>, dim3(blocks_for(n, 256)), dim3(256), 0, c->stream, pts, n, coef, bound, flag, nflag);
  else hipLaunchKernelGGL(sac_flag_kernel<false>, dim3(blocks_for(n, 256)), dim3(256), 0, c->stream, pts, n, coef, bound, flag, nflag);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

// the arrays of the tail, carved after whatever the caller took
struct TailArrays { unsigned long long *list, *nlist; uint32_t *counters; float4 *stage; uint32_t *d_index; char *tmp; size_t sel_bytes; };
void plan_tail(Carver &plan, size_t n, size_t sel_bytes)
{
  plan.plan<unsigned long long>(n); plan.plan<unsigned long long>(n); plan.plan<uint32_t>(4); plan.plan<float4>(n); plan.plan<uint32_t>(n);
  plan.plan<char>(sel_bytes);
}
TailArrays take_tail(Carver &s, size_t n, size_t sel_bytes)
{
  TailArrays t;
  t.list = s.take<unsigned long long>(n); t.nlist = s.take<unsigned long long>(n); t.counters = s.take<uint32_t>(4);
  t.stage = s.take<float4>(n); t.d_index = s.take<uint32_t>(n); t.tmp = s.take<char>(sel_bytes); t.sel_bytes = sel_bytes;
  return t;
}

int segment_cloud(Ctx *c, Cloud *dst, Cloud &src, const mvr_sac_params &p, mvr_sac_result *res, size_t *n_out, uint32_t *inlier_index,
                  uint8_t *inlier_flag, mvr_sac_trace *trace, size_t trace_cap)
{
  const size_t n = src.n;
  const bool normals = src.has_normals, fma = p.fma_dist != 0, negative = p.negative != 0;
  if (int rc = knn_cloud_ok(c, src, "segment_plane")) return rc;
  mvr_sac_result R;
  std::memset(&R, 0, sizeof R);
  R.best_attempt = -1;
  R.k = 1.0;
  size_t out_n = 0;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "segment_plane reads back");
    size_t sel_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    const size_t blocks = (n + 255) / 256;
    Carver plan;
    plan.plan<uint8_t>(n); plan.plan<unsigned long long>(n); plan.plan<uint8_t>(n); plan.plan<uint8_t>(n);
    plan.plan<char>(RansacChunk<SacHyp>::kBytes); plan.plan<float4>(kRansacMaxChunk); plan.plan<double>(blocks * kSacMoments);
    plan.plan<SacFit>(1);
    plan_tail(plan, n, sel_bytes);
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    uint8_t *valid = s.take<uint8_t>(n);
    unsigned long long *vlist = s.take<unsigned long long>(n);
    uint8_t *flag = s.take<uint8_t>(n), *nflag = s.take<uint8_t>(n);
    char *chunk_dev = s.take<char>(RansacChunk<SacHyp>::kBytes);
    const RansacChunk<SacHyp> dev(chunk_dev);
    float4 *d_coef = s.take<float4>(kRansacMaxChunk);
    double *partials = s.take<double>(blocks * kSacMoments);
    SacFit *d_fit = s.take<SacFit>(1);
    TailArrays t = take_tail(s, n, sel_bytes);
    const float bound = f32_at_least(p.threshold);

    // P1
    hipLaunchKernelGGL(sac_valid_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, c->stream, src.pts, n, valid);
    MVR_HIP_TRY(c, hipGetLastError());
    if (int rc = select_flagged(c, t.tmp, sel_bytes, valid, n, vlist, t.counters)) return rc;
    uint32_t nv = 0;
    MVR_HIP_TRY(c, hipMemcpyAsync(&nv, t.counters, sizeof nv, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));

    // P7 over the chunks of P8
    RansacLoop loop(p.max_iterations, std::log(1.0 - p.probability), nv, c->sac_chunk);
    SacHyp best_hyp;
    std::memset(&best_hyp, 0, sizeof best_hyp);
    if (nv >= 3u) {
      HypArgs a{};
      a.pts = src.pts; a.vlist = vlist; a.nv = nv; a.seed = p.seed; a.model = p.model;
      a.ax = p.axis[0]; a.ay = p.axis[1]; a.az = p.axis[2];
      a.na = p.model == 1 ? std::sqrt((a.ax * a.ax + a.ay * a.ay) + a.az * a.az) : 1.0;
      a.cos_eps = p.model == 1 ? std::cos(p.eps_angle) : 0.0;
      a.hyp = dev.rec; a.coef = d_coef; a.counts = dev.counts;
      std::vector<char> host_mem(RansacChunk<SacHyp>::kBytes);
      const RansacChunk<SacHyp> host(host_mem.data());
      while (loop.more()) {
        a.count = loop.next_chunk();
        a.t0 = (uint64_t)loop.attempt;
        hipLaunchKernelGGL(sac_hypotheses_kernel, dim3(blocks_for(ransac_padded<PlaneModel>(a.count), 64)), dim3(64), 0, c->stream, a);
        MVR_HIP_TRY(c, hipGetLastError());
        if (int rc = ransac_launch_count<PlaneModel>(c, fma, src.pts, n, d_coef, a.count, bound, dev.counts)) return rc;
        MVR_HIP_TRY(c, hipMemcpyAsync(host_mem.data(), chunk_dev, host_mem.size(), hipMemcpyDeviceToHost, c->stream));
        MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
        loop.replay(
            a.count, [&](uint32_t h) { return host.rec[h].status; }, [&](uint32_t h) { return host.counts[h]; },
            [&](uint32_t h) { best_hyp = host.rec[h]; },
            [&](uint32_t h, long long attempt, int status, uint32_t count, double k) {
              if (!trace || (size_t)attempt >= trace_cap) return;
              const SacHyp &H = host.rec[h];
              mvr_sac_trace &T = trace[attempt];
              T.status = status;
              for (int j = 0; j < 3; ++j) T.sample[j] = H.sample[j];
              for (int j = 0; j < 4; ++j) T.coefficients[j] = H.coef[j];
              T.inliers = count;
              T.k = k;
            });
      }
    }
    R.iterations = (int)loop.iterations; R.skipped = (int)loop.skipped; R.attempts = (int)loop.attempt; R.k = loop.k;
    R.found = loop.best_count > 0 ? 1 : 0;
    SacFit hf;
    std::memset(&hf, 0, sizeof hf);
    if (R.found) {
      R.best_attempt = (int)loop.best;
      // P9, P10
      hf.plane[0] = hf.plane[1] = make_float4(best_hyp.coef[0], best_hyp.coef[1], best_hyp.coef[2], best_hyp.coef[3]);
      MVR_HIP_TRY(c, hipMemcpyAsync(d_fit, &hf, sizeof hf, hipMemcpyHostToDevice, c->stream));
      MVR_HIP_TRY(c, hipMemcpyAsync(&d_fit->q, src.pts + best_hyp.sample[0], sizeof(float4), hipMemcpyDeviceToDevice, c->stream));      // P10's q
      if (int rc = launch_flags(c, fma, src.pts, n, &d_fit->plane[0], bound, flag, nflag)) return rc;
      if (p.optimize) {
        hipLaunchKernelGGL(sac_moments_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, src.pts, n, flag, &d_fit->q, partials);
        hipLaunchKernelGGL(sac_fit_kernel, dim3(1), dim3(kSacFitThreads), 0, c->stream, partials, (uint32_t)blocks, d_fit);
        MVR_HIP_TRY(c, hipGetLastError());
        if (int rc = launch_flags(c, fma, src.pts, n, &d_fit->plane[1], bound, flag, nflag)) return rc;
      }
    } else {
      MVR_HIP_TRY(c, hipMemsetAsync(flag, 0, n, c->stream));
      MVR_HIP_TRY(c, hipMemsetAsync(nflag, 1, n, c->stream));
    }
    // P11
    uint32_t hc[2] = {0, 0};
    if (int rc = select_flagged(c, t.tmp, sel_bytes, flag, n, t.list, t.counters)) return rc;
    if (dst && negative)
      if (int rc = select_flagged(c, t.tmp, sel_bytes, nflag, n, t.nlist, t.counters + 1)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, t.counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    if (R.found) MVR_HIP_TRY(c, hipMemcpyAsync(&hf, d_fit, sizeof hf, hipMemcpyDeviceToHost, c->stream));
    if (inlier_flag) MVR_HIP_TRY(c, hipMemcpyAsync(inlier_flag, flag, n, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t inliers = hc[0];
    R.inliers = (uint32_t)inliers;
    if (R.found) {
      const float4 f = hf.plane[1], r = hf.plane[0];
      R.coefficients[0] = f.x; R.coefficients[1] = f.y; R.coefficients[2] = f.z; R.coefficients[3] = f.w;
      R.ransac_coefficients[0] = r.x; R.ransac_coefficients[1] = r.y; R.ransac_coefficients[2] = r.z; R.ransac_coefficients[3] = r.w;
      R.ransac_inliers = p.optimize ? hf.ransac_inliers : (uint32_t)inliers;
    }
    if (inlier_index && inliers) {
      hipLaunchKernelGGL(sac_low_words_kernel, dim3(blocks_for(inliers, 256)), dim3(256), 0, c->stream, t.list, inliers, t.d_index);
      MVR_HIP_TRY(c, hipGetLastError());
      MVR_HIP_TRY(c, hipMemcpyAsync(inlier_index, t.d_index, inliers * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    out_n = negative ? n - inliers : inliers;
    if (dst)
      if (int rc = gather_kept(c, *dst, src.pts, normals ? src.nrm : nullptr, negative ? t.nlist : t.list, out_n, t.stage, nullptr)) return rc;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // inlier_index is complete on return, and the arena is free again
  }
  if (dst) finish_dst(c, *dst, out_n, normals);
  *res = R;
  if (n_out) *n_out = out_n;
  return MVR_OK;
}

int extract_cloud(Ctx *c, Cloud &dst, Cloud &src, const uint32_t *index, size_t count, bool negative, size_t *n_out)
{
  const size_t n = src.n;
  const bool normals = src.has_normals;
  if (int rc = knn_cloud_ok(c, src, "extract_indices")) return rc;
  for (size_t k = 0; k < count; ++k)
    if (index[k] >= n) return set_error(c, MVR_E_ARG, "extract_indices: an index is outside the source");
  size_t kept = 0;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "extract_indices reads back");
    size_t sel_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    Carver plan;
    plan.plan<uint8_t>(n); plan.plan<uint32_t>(count);
    plan_tail(plan, n, sel_bytes);
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    uint8_t *flag = s.take<uint8_t>(n);
    uint32_t *d_in = s.take<uint32_t>(count);
    TailArrays t = take_tail(s, n, sel_bytes);
    MVR_HIP_TRY(c, hipMemsetAsync(flag, negative ? 1 : 0, n, c->stream));
    if (count) {
      MVR_HIP_TRY(c, hipMemcpyAsync(d_in, index, count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      if (int rc = launch_mark(c, d_in, count, (uint8_t)(negative ? 0 : 1), flag)) return rc;
    }
    uint32_t hc = 0;
    if (int rc = select_flagged(c, t.tmp, sel_bytes, flag, n, t.list, t.counters)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(&hc, t.counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the caller's index array has been read by now, too)
    kept = hc;
    if (int rc = gather_kept(c, dst, src.pts, normals ? src.nrm : nullptr, t.list, kept, t.stage, nullptr)) return rc;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  finish_dst(c, dst, kept, normals);
  if (n_out) *n_out = kept;
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API int mvr_cloud_segment_plane(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_sac_params *p, mvr_sac_result *result, size_t *n_out,
                                uint32_t *inlier_index, uint8_t *inlier_flag, mvr_sac_trace *trace, size_t trace_cap)
{
  if (!ctx || !p || !result || !slot_ok(src_slot) || !(dst_slot == -1 || slot_ok(dst_slot))) return MVR_E_ARG;
  if (p->model < 0 || p->model > 1 || !(std::isfinite(p->threshold) && p->threshold > 0.0)) return MVR_E_ARG;
  if (p->max_iterations < 1 || p->max_iterations > (1 << 24) || !(p->probability > 0.0 && p->probability < 1.0)) return MVR_E_ARG;
  if (p->model == 1) {
    const double *a = p->axis;
    if (!std::isfinite(a[0]) || !std::isfinite(a[1]) || !std::isfinite(a[2]) || (a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0)) return MVR_E_ARG;
    if (!(p->eps_angle > 0.0 && p->eps_angle <= M_PI / 2)) return MVR_E_ARG;
  }
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return segment_cloud(c, dst_slot < 0 ? nullptr : &c->slots[dst_slot], c->slots[src_slot], *p, result, n_out, inlier_index, inlier_flag, trace,
                       trace_cap);
}

API int mvr_cloud_extract_indices(mvr_ctx *ctx, int dst_slot, int src_slot, const uint32_t *index, size_t count, int negative, size_t *n_out)
{
  if (!ctx || !slot_ok(src_slot) || !slot_ok(dst_slot) || (!index && count)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return extract_cloud(c, c->slots[dst_slot], c->slots[src_slot], index, count, negative != 0, n_out);
}
