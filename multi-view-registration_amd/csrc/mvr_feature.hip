// csrc/mvr_feature.hip -- what consumes the FPFH and PFH signatures (gfx950): exact k-NN in feature space, the scores of many
// posed copies of one cloud against a target, and pcl::SampleConsensusPrerejective on top of the two.  The rules M1-M3, S1-S2 and
// A1-A6 are written next to mvr_feature_knn / mvr_pose_scores / mvr_align_prerejective in mvr_hip.h.
//
//   * feature_knn_kernel (mvr_feature_knn.h): an all-pairs distance kernel in DIM = 33 (FPFH) or 125 (PFH) dimensions, a
//     template of the row length.  One query per thread, its DIM features in registers; the block stages a tile of target rows in LDS (rows padded
//     to a multiple of four floats, 36 or 128, so a row is nine or thirty-two 16-byte reads at an address the whole wave
//     shares: a broadcast, no bank conflict); the k-best list is the register list of mvr_knn.hip (64-bit keys,
//     compile-time indices, bucketed by kmax_bucket).  blockIdx.y splits the TARGET, so that 5 000 queries -- 20 blocks -- still
//     fill the chip; every split writes its k best keys and feature_merge_kernel merges them under the same total order (the
//     keys are distinct, so the k smallest of the union do not depend on the split).  A row with a non-finite component gives
//     a non-finite d2, whose key is never below the empty key: rule M3 costs no test.
//   * pose_score_kernel: one thread per (pose, source point), the points of a pose in the source's grid order (the lanes of a
//     wave are neighbours and walk the same cells of the target's grid).  The thread poses its point with the arithmetic of
//     transform_f32_kernel and walks the ball of max_dist around it (knn_ball_walk), keeping the minimum key.  The block adds
//     its 256 values in a fixed tree and writes one partial; pose_sum_kernel adds a pose's partials in ascending order.
//   * prerej_hypotheses_kernel: one thread per iteration -- draws, matches, polygon test, and the gather of the sampled points
//     the host's 3 x 3 SVD needs.
// Compiled with -ffp-contract=off: every f32 operation of M1 is rounded as written.
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvr_internal.h"
#include "mvr_feature_knn.h"
#include "mvr_knn_walk.h"

namespace mvr {
namespace {

constexpr int kMaxSplit = 64;
constexpr int kScoreThreads = kKnnThreads;

// ------------------------------------------------------------------ feature k-NN

template <int KMAX>
__global__ void __launch_bounds__(kFeatThreads) feature_merge_kernel(const nnkey_t *__restrict__ part, const uint32_t nq, const int splits, const int k,
                                                                     uint32_t *__restrict__ oidx, float *__restrict__ od2)
{
  const uint32_t qi = blockIdx.x * kFeatThreads + threadIdx.x;
  if (qi >= nq) return;
  nnkey_t L[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) L[i] = i < KMAX - k ? 0ull : kKnnKeyEmpty;
  for (int s = 0; s < splits; ++s) {
    const nnkey_t *in = part + ((size_t)s * nq + qi) * (size_t)k;
    for (int j = 0; j < k; ++j) {
      const nnkey_t key = in[j];
      if (!(key < L[KMAX - 1])) break;      // (a split's list is ascending: nothing further of it gets in)
      knn_insert<KMAX>(L, key);
    }
  }
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    if (i >= KMAX - k) {
      const size_t o = (size_t)qi * k + (size_t)(i - (KMAX - k));
      if (oidx) oidx[o] = L[i] == kKnnKeyEmpty ? kNone : (uint32_t)L[i];
      if (od2) od2[o] = __uint_as_float((uint32_t)(L[i] >> 32));      // (the empty key carries +inf)
    }
  }
}

template <int KMAX>
void launch_merge(hipStream_t st, unsigned qblocks, const nnkey_t *part, uint32_t nq, int splits, int k, uint32_t *oidx, float *od2)
{
  hipLaunchKernelGGL(feature_merge_kernel<KMAX>, dim3(qblocks), dim3(kFeatThreads), 0, st, part, nq, splits, k, oidx, od2);
}

// the k-NN table of nq device rows in nt device rows of dim floats (feat_dim_ok), into device tables (either may be null); queued
// on the context's stream (the partial lists are freed after a wait for it)
int feature_knn_device(Ctx *c, const float *dq, size_t nq, const float *dt, size_t nt, int dim, int k, uint32_t *didx, float *dd2)
{
  if (nq == 0) return MVR_OK;
  if (nq > 0x7FFFFFF0ull || nt > 0x7FFFFFF0ull) return set_error(c, MVR_E_ARG, "feature_knn: table too large");
  const unsigned qblocks = blocks_for(nq, kFeatThreads);
  // the split: enough blocks for two per compute unit, a split no shorter than four tiles, the partial lists within 256 MiB
  size_t splits = c->feat_split > 0 ? (size_t)c->feat_split : ((size_t)2 * (size_t)std::max(c->n_cu, 1) + qblocks - 1) / qblocks;
  splits = std::min<size_t>(splits, kMaxSplit);
  if (c->feat_split <= 0) splits = std::min<size_t>(splits, std::max<size_t>(nt / (4 * kFeatTile), 1));
  splits = std::min<size_t>(splits, std::max<size_t>(((size_t)256 << 20) / (nq * (size_t)k * sizeof(nnkey_t)), 1));
  splits = std::max<size_t>(splits, 1);
  size_t rows = (nt + splits - 1) / splits;
  rows = std::max<size_t>((rows + kFeatTile - 1) / kFeatTile * kFeatTile, kFeatTile);
  splits = std::max<size_t>((nt + rows - 1) / rows, 1);
  DevBuf part;
  if (part.alloc(splits * nq * (size_t)k * sizeof(nnkey_t)) != hipSuccess) return set_error(c, MVR_E_NOMEM, "feature_knn: out of device memory");
  const dim3 grid(qblocks, (unsigned)splits);
  nnkey_t *pp = part.as<nnkey_t>();
  // (the 125-float instantiations stand in mvr_pfh.hip and the 352-float kernel in mvr_shot.hip, beside the descriptors they
  // serve: this file holds the 33-float ones)
  if (dim == kShotDim) launch_feature_knn_shot(c->stream, grid, dq, (uint32_t)nq, dt, (uint32_t)nt, (uint32_t)rows, k, pp);
  else if (dim == kPfhDim) launch_feature_knn_pfh(c->stream, grid, dq, (uint32_t)nq, dt, (uint32_t)nt, (uint32_t)rows, k, pp);
  else launch_feature_knn<kFpfhDim>(c->stream, grid, dq, (uint32_t)nq, dt, (uint32_t)nt, (uint32_t)rows, k, pp);
  switch (kmax_bucket(k)) {
    case 8:  launch_merge<8>(c->stream, qblocks, pp, (uint32_t)nq, (int)splits, k, didx, dd2); break;
    case 16: launch_merge<16>(c->stream, qblocks, pp, (uint32_t)nq, (int)splits, k, didx, dd2); break;
    case 32: launch_merge<32>(c->stream, qblocks, pp, (uint32_t)nq, (int)splits, k, didx, dd2); break;
    default: launch_merge<64>(c->stream, qblocks, pp, (uint32_t)nq, (int)splits, k, didx, dd2); break;
  }
  MVR_HIP_TRY(c, hipGetLastError());
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MVR_OK;
}

// ------------------------------------------------------------------ pose scores

struct ScoreArgs {
  KnnSlot S;                       // queries: the source in its grid order; target: the target's own grid
  const float *T;                  // [count][16] column-major, device
  uint32_t pose0;                  // first pose of this launch (blockIdx.y counts from it)
  float r2;                        // the ball: the least f32 not below max_dist^2
  double md2;                      // max_dist^2
  double *psum; uint32_t *pcnt;    // [poses of the launch][blocks]
  uint32_t *inliers; double *error;      // [count]
  uint32_t nblk;
};

template <bool FMA>
__global__ void __launch_bounds__(kScoreThreads) pose_score_kernel(ScoreArgs a)
{
  __shared__ double ssum[kScoreThreads];
  __shared__ uint32_t scnt[kScoreThreads];
  const KnnSlot &S = a.S;
  const uint32_t tid = threadIdx.x, pos = blockIdx.x * kScoreThreads + tid;
  double v = 0.0;
  uint32_t in = 0u;
  if (pos < S.nq) {
    const float *T = a.T + (size_t)(a.pose0 + blockIdx.y) * 16;
    const float4 p = S.qs[pos];
    float4 q;      // transform_f32_kernel's arithmetic
    q.x = ((T[0] * p.x + T[4] * p.y) + T[8] * p.z) + T[12];
    q.y = ((T[1] * p.x + T[5] * p.y) + T[9] * p.z) + T[13];
    q.z = ((T[2] * p.x + T[6] * p.y) + T[10] * p.z) + T[14];
    q.w = 1.0f;
    nnkey_t best = kKeyInit;
    knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 t, const uint32_t j) {
      const nnkey_t key = ((nnkey_t)__float_as_uint(knn_dist2<FMA>(t, q)) << 32) | knn_index_of(S, t, j);
      best = key < best ? key : best;
    });
    if (best != kKeyInit) {
      const double d2 = (double)__uint_as_float((uint32_t)(best >> 32));
      if (d2 < a.md2) { v = d2; in = 1u; }      // S1: strictly
    }
  }
  ssum[tid] = v; scnt[tid] = in;
  __syncthreads();
#pragma unroll
  for (int s = kScoreThreads / 2; s > 0; s >>= 1) {      // a fixed tree: the same sum whatever the launch
    if (tid < (uint32_t)s) { ssum[tid] += ssum[tid + s]; scnt[tid] += scnt[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    const size_t o = (size_t)blockIdx.y * a.nblk + blockIdx.x;
    a.psum[o] = ssum[0]; a.pcnt[o] = scnt[0];
  }
}

__global__ void __launch_bounds__(kScoreThreads) pose_sum_kernel(ScoreArgs a, const uint32_t nposes)
{
  const uint32_t h = blockIdx.x * kScoreThreads + threadIdx.x;
  if (h >= nposes) return;
  double s = 0.0; uint32_t n = 0u;
  for (uint32_t b = 0; b < a.nblk; ++b) { s += a.psum[(size_t)h * a.nblk + b]; n += a.pcnt[(size_t)h * a.nblk + b]; }
  a.inliers[a.pose0 + h] = n;
  a.error[a.pose0 + h] = n ? s / (double)n : DBL_MAX;
}

// `count` device poses scored into device arrays; queued on the context's stream, waited for before return
int pose_scores_device(Ctx *c, Cloud &src, Cloud &tgt, const float *dT, size_t count, double max_dist, bool fma, uint32_t *dinl, double *derr)
{
  if (count == 0) return MVR_OK;
  if (int rc = knn_cloud_ok(c, src, "pose_scores")) return rc;
  if (int rc = knn_cloud_ok(c, tgt, "pose_scores")) return rc;
  ScoreArgs a{};
  if (int rc = fill_target(c, tgt, a.S)) return rc;
  if (&src != &tgt && src.n >= 4) {      // the source's own grid gives its points their walking order
    bool ok = false;
    if (int rc = ensure_model_grid(c, src, &ok)) return rc;
  }
  fill_queries(src, a.S);
  a.T = dT;
  a.md2 = max_dist * max_dist;
  a.r2 = clamp_r2(max_dist);
  if ((double)a.r2 < a.md2 && a.r2 < std::numeric_limits<float>::max()) a.r2 = std::nextafterf(a.r2, std::numeric_limits<float>::infinity());
  a.nblk = std::max(blocks_for(src.n, kScoreThreads), 1u);
  a.inliers = dinl; a.error = derr;
  const size_t chunk = std::min<size_t>((size_t)std::max(c->score_chunk, 1), count);
  DevBuf ps, pc;
  if (ps.alloc(chunk * a.nblk * sizeof(double)) != hipSuccess || pc.alloc(chunk * a.nblk * sizeof(uint32_t)) != hipSuccess)
    return set_error(c, MVR_E_NOMEM, "pose_scores: out of device memory");
  a.psum = ps.as<double>(); a.pcnt = pc.as<uint32_t>();
  for (size_t h0 = 0; h0 < count; h0 += chunk) {
    const unsigned m = (unsigned)std::min(chunk, count - h0);
    a.pose0 = (uint32_t)h0;
    const dim3 grid(a.nblk, m);
    if (fma) hipLaunchKernelGGL(pose_score_kernel<true>, grid, dim3(kScoreThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(pose_score_kernel<false>, grid, dim3(kScoreThreads), 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(pose_sum_kernel, dim3(blocks_for(m, kScoreThreads)), dim3(kScoreThreads), 0, c->stream, a, m);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MVR_OK;
}

// ------------------------------------------------------------------ hypotheses

constexpr int kMaxSamples = MVR_PREREJ_MAX_SAMPLES;

// (prerej_mix / prerej_draw, rule A2: mvr_internal.h -- the plane segmentation draws with them too)

struct HypArgs {
  const float4 *sp, *tp;           // the slots' points by index
  const uint32_t *elig; uint32_t ne;
  const uint32_t *knn; int k;      // [ne][k]
  int nr, iters;
  uint64_t seed;
  float sim2;
  int *status;                     // [iters]
  uint32_t *src, *tgt;             // [iters][8]
  float4 *gs, *gt;                 // [iters][8]: the sampled points, gathered
};

template <bool FMA>
__global__ void __launch_bounds__(kKnnThreads) prerej_hypotheses_kernel(HypArgs a)
{
  const uint32_t i = blockIdx.x * kKnnThreads + threadIdx.x;
  if (i >= (uint32_t)a.iters) return;
  uint32_t pos[kMaxSamples], sorted[kMaxSamples];
  float4 ps[kMaxSamples], pt[kMaxSamples];
  bool matched = true;
  for (int j = 0; j < a.nr; ++j) {
    uint32_t r = prerej_draw(a.seed, i, (uint64_t)j, (uint64_t)(a.ne - (uint32_t)j));      // A2
    int at = 0;
    for (; at < j && r >= sorted[at]; ++at) ++r;
    for (int m = j; m > at; --m) sorted[m] = sorted[m - 1];
    sorted[at] = r;
    pos[j] = r;
  }
  for (int j = 0; j < a.nr; ++j) {
    const uint32_t s = a.elig[pos[j]];
    const uint32_t *list = a.knn + (size_t)pos[j] * a.k;
    uint32_t kk = 0;
    while (kk < (uint32_t)a.k && list[kk] != kNone) ++kk;      // A3 (the non-empty entries lead the list)
    const uint32_t m = kk ? list[prerej_draw(a.seed, i, (uint64_t)(8 + j), (uint64_t)kk)] : kNone;
    matched = matched && kk != 0u;
    ps[j] = a.sp[s];
    pt[j] = kk ? a.tp[m] : make_float4(0.f, 0.f, 0.f, 0.f);
    a.src[(size_t)i * kMaxSamples + j] = s;
    a.tgt[(size_t)i * kMaxSamples + j] = m;
    a.gs[(size_t)i * kMaxSamples + j] = ps[j];
    a.gt[(size_t)i * kMaxSamples + j] = pt[j];
  }
  for (int j = a.nr; j < kMaxSamples; ++j) { a.src[(size_t)i * kMaxSamples + j] = kNone; a.tgt[(size_t)i * kMaxSamples + j] = kNone; }
  int status = 2;
  if (matched) {
    status = 1;
    for (int j = 0; j < a.nr; ++j) {      // A4
      const int n = j + 1 == a.nr ? 0 : j + 1;
      const float ds = knn_dist2<FMA>(ps[j], ps[n]), dt = knn_dist2<FMA>(pt[j], pt[n]);
      const float sim = ds < dt ? ds / dt : dt / ds;
      if (!(sim >= a.sim2)) status = 0;
    }
  }
  a.status[i] = status;
}

// A5: the estimator of mvr_icp_align on n pairs in sample order (f64 means, centred covariance / n, Umeyama without scaling)
void pose_from_pairs(const float4 *p, const float4 *q, int n, float T[16])
{
  double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0}, sigma[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < n; ++j) {
    ms[0] += (double)p[j].x; ms[1] += (double)p[j].y; ms[2] += (double)p[j].z;
    mt[0] += (double)q[j].x; mt[1] += (double)q[j].y; mt[2] += (double)q[j].z;
  }
  for (int a = 0; a < 3; ++a) { ms[a] /= (double)n; mt[a] /= (double)n; }
  for (int j = 0; j < n; ++j) {
    const double dp[3] = {(double)p[j].x - ms[0], (double)p[j].y - ms[1], (double)p[j].z - ms[2]};
    const double dq[3] = {(double)q[j].x - mt[0], (double)q[j].y - mt[1], (double)q[j].z - mt[2]};
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) sigma[3 * r + k] += dq[r] * dp[k];
  }
  for (int e = 0; e < 9; ++e) sigma[e] /= (double)n;
  umeyama_from_moments(ms, mt, sigma, T, nullptr);
}

double ms_since(const std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int align_prerejective(Ctx *c, Cloud &src, Cloud &tgt, const float *src_feat, const float *tgt_feat, const int dim, const mvr_prerej_params &p,
                       const float *guess, mvr_prerej_result *res, mvr_prerej_trace *trace)
{
  const size_t ns = src.n, nt = tgt.n, iters = (size_t)p.max_iterations, row_len = (size_t)dim;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memset(res, 0, sizeof *res);
  res->best_iteration = -1;
  res->error = DBL_MAX;
  std::memcpy(res->T, guess ? guess : I, sizeof I);
  if (trace) {
    std::memset(trace, 0, iters * sizeof *trace);
    for (size_t i = 0; i < iters; ++i) {
      trace[i].status = 2;
      for (int j = 0; j < kMaxSamples; ++j) trace[i].src[j] = trace[i].tgt[j] = kNone;
    }
  }
  c->prerej_ms[0] = c->prerej_ms[1] = c->prerej_ms[2] = 0.0;
  if (int rc = knn_cloud_ok(c, src, "align_prerejective")) return rc;
  if (int rc = knn_cloud_ok(c, tgt, "align_prerejective")) return rc;
  MVR_MAY_BLOCK(c, "align_prerejective reads back");
  auto t0 = std::chrono::steady_clock::now();
  // A1: the eligible source points and their feature rows, packed
  std::vector<float4> hp(ns);
  if (ns) MVR_HIP_TRY(c, hipMemcpyAsync(hp.data(), src.pts, ns * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<uint32_t> elig;
  std::vector<float> qrows;
  for (size_t i = 0; i < ns; ++i) {
    bool ok = std::isfinite(hp[i].x) && std::isfinite(hp[i].y) && std::isfinite(hp[i].z);
    const float *row = src_feat + i * row_len;
    for (size_t b = 0; b < row_len && ok; ++b) ok = std::isfinite(row[b]);
    if (!ok) continue;
    elig.push_back((uint32_t)i);
    qrows.insert(qrows.end(), row, row + row_len);
  }
  const size_t ne = elig.size();
  // the scores of the guess and of the surviving poses: one table, the guess first
  std::vector<float> poses;
  std::vector<size_t> pose_iter;      // the iteration of a pose (the guess: SIZE_MAX)
  if (guess) { poses.insert(poses.end(), guess, guess + 16); pose_iter.push_back(SIZE_MAX); }
  std::vector<int> status(iters, 2);
  if (ne >= (size_t)p.nr_samples && iters > 0) {
    // A3: the k-NN table of the eligible rows
    DevBuf dq, dt, dknn, delig, dstat, dsrc, dtgt, dgs, dgt;
    const size_t hyp = iters * kMaxSamples;
    if (dq.alloc(ne * row_len * 4) != hipSuccess || dt.alloc(nt * row_len * 4) != hipSuccess || dknn.alloc(ne * (size_t)p.k * 4) != hipSuccess ||
        delig.alloc(ne * 4) != hipSuccess || dstat.alloc(iters * 4) != hipSuccess || dsrc.alloc(hyp * 4) != hipSuccess ||
        dtgt.alloc(hyp * 4) != hipSuccess || dgs.alloc(hyp * sizeof(float4)) != hipSuccess || dgt.alloc(hyp * sizeof(float4)) != hipSuccess)
      return set_error(c, MVR_E_NOMEM, "align_prerejective: out of device memory");
    MVR_HIP_TRY(c, hipMemcpyAsync(dq.p, qrows.data(), ne * row_len * 4, hipMemcpyHostToDevice, c->stream));
    if (nt) MVR_HIP_TRY(c, hipMemcpyAsync(dt.p, tgt_feat, nt * row_len * 4, hipMemcpyHostToDevice, c->stream));
    MVR_HIP_TRY(c, hipMemcpyAsync(delig.p, elig.data(), ne * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = feature_knn_device(c, dq.as<float>(), ne, dt.as<float>(), nt, dim, p.k, dknn.as<uint32_t>(), nullptr)) return rc;
    c->prerej_ms[0] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    // A2-A4 for every iteration in one launch, the sampled points gathered on the way
    HypArgs a{};
    a.sp = src.pts; a.tp = tgt.pts; a.elig = delig.as<uint32_t>(); a.ne = (uint32_t)ne; a.knn = dknn.as<uint32_t>(); a.k = p.k;
    a.nr = p.nr_samples; a.iters = (int)iters; a.seed = p.seed; a.sim2 = (float)(p.similarity * p.similarity);
    a.status = dstat.as<int>(); a.src = dsrc.as<uint32_t>(); a.tgt = dtgt.as<uint32_t>(); a.gs = dgs.as<float4>(); a.gt = dgt.as<float4>();
    const dim3 grid(blocks_for(iters, kKnnThreads));
    if (p.fma_dist) hipLaunchKernelGGL(prerej_hypotheses_kernel<true>, grid, dim3(kKnnThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(prerej_hypotheses_kernel<false>, grid, dim3(kKnnThreads), 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
    std::vector<uint32_t> hsrc(hyp), htgt(hyp);
    std::vector<float4> hgs(hyp), hgt(hyp);
    MVR_HIP_TRY(c, hipMemcpyAsync(status.data(), dstat.p, iters * 4, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipMemcpyAsync(hgs.data(), dgs.p, hyp * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipMemcpyAsync(hgt.data(), dgt.p, hyp * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    if (trace) {
      MVR_HIP_TRY(c, hipMemcpyAsync(hsrc.data(), dsrc.p, hyp * 4, hipMemcpyDeviceToHost, c->stream));
      MVR_HIP_TRY(c, hipMemcpyAsync(htgt.data(), dtgt.p, hyp * 4, hipMemcpyDeviceToHost, c->stream));
    }
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    // A5: the surviving poses, compacted
    for (size_t i = 0; i < iters; ++i) {
      if (trace) {
        trace[i].status = status[i];
        std::memcpy(trace[i].src, hsrc.data() + i * kMaxSamples, sizeof trace[i].src);
        std::memcpy(trace[i].tgt, htgt.data() + i * kMaxSamples, sizeof trace[i].tgt);
      }
      if (status[i] == 0) ++res->rejected;
      if (status[i] != 1) continue;
      float T[16];
      pose_from_pairs(hgs.data() + i * kMaxSamples, hgt.data() + i * kMaxSamples, p.nr_samples, T);
      poses.insert(poses.end(), T, T + 16);
      pose_iter.push_back(i);
      ++res->scored;
    }
    c->prerej_ms[1] = ms_since(t0);
  } else {
    c->prerej_ms[0] = ms_since(t0);
  }
  // A6
  t0 = std::chrono::steady_clock::now();
  const size_t np = pose_iter.size();
  if (np == 0) return MVR_OK;
  DevBuf dT, dinl, derr;
  if (dT.alloc(np * 64) != hipSuccess || dinl.alloc(np * 4) != hipSuccess || derr.alloc(np * 8) != hipSuccess)
    return set_error(c, MVR_E_NOMEM, "align_prerejective: out of device memory");
  MVR_HIP_TRY(c, hipMemcpyAsync(dT.p, poses.data(), np * 64, hipMemcpyHostToDevice, c->stream));
  if (int rc = pose_scores_device(c, src, tgt, dT.as<float>(), np, p.max_dist, p.fma_dist != 0, dinl.as<uint32_t>(), derr.as<double>())) return rc;
  std::vector<uint32_t> inl(np);
  std::vector<double> err(np);
  MVR_HIP_TRY(c, hipMemcpy(inl.data(), dinl.p, np * 4, hipMemcpyDeviceToHost));
  MVR_HIP_TRY(c, hipMemcpy(err.data(), derr.p, np * 8, hipMemcpyDeviceToHost));
  double lowest = DBL_MAX;
  for (size_t h = 0; h < np; ++h) {
    const size_t i = pose_iter[h];
    if (trace && i != SIZE_MAX) {
      trace[i].inliers = inl[h]; trace[i].error = err[h];
      std::memcpy(trace[i].T, poses.data() + 16 * h, 64);
    }
    const double fraction = ns ? (double)inl[h] / (double)ns : 0.0;
    if (fraction >= p.inlier_fraction && err[h] < lowest) {
      lowest = err[h];
      res->converged = 1;
      res->best_iteration = i == SIZE_MAX ? -1 : (int)i;
      res->inliers = inl[h];
      res->error = err[h];
      std::memcpy(res->T, poses.data() + 16 * h, 64);
    }
  }
  c->prerej_ms[2] = ms_since(t0);
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API int mvr_feature_knn(mvr_ctx *ctx, const float *q, size_t nq, const float *t, size_t nt, int dim, int k, uint32_t *idx, float *d2)
{
  if (!ctx || !feat_dim_ok(dim) || k < 1 || k > MVR_MAX_KNN || (!q && nq) || (!t && nt)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  if (nq == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "feature_knn reads back");
  const size_t m = nq * (size_t)k, row_len = (size_t)dim;
  DevBuf dq, dt, di, dd;
  if (dq.alloc(nq * row_len * 4) != hipSuccess || dt.alloc(nt * row_len * 4) != hipSuccess || di.alloc(m * 4) != hipSuccess || dd.alloc(m * 4) != hipSuccess)
    return set_error(c, MVR_E_NOMEM, "mvr_feature_knn: out of device memory");
  MVR_HIP_TRY(c, hipMemcpyAsync(dq.p, q, nq * row_len * 4, hipMemcpyHostToDevice, c->stream));
  if (nt) MVR_HIP_TRY(c, hipMemcpyAsync(dt.p, t, nt * row_len * 4, hipMemcpyHostToDevice, c->stream));
  if (int rc = feature_knn_device(c, dq.as<float>(), nq, dt.as<float>(), nt, dim, k, di.as<uint32_t>(), dd.as<float>())) return rc;
  if (idx) MVR_HIP_TRY(c, hipMemcpy(idx, di.p, m * 4, hipMemcpyDeviceToHost));
  if (d2) MVR_HIP_TRY(c, hipMemcpy(d2, dd.p, m * 4, hipMemcpyDeviceToHost));
  return MVR_OK;
}

API int mvr_pose_scores(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *T, size_t count, double max_dist, int fma_dist,
                        uint32_t *inliers, double *error)
{
  if (!ctx || !slot_ok(src_slot) || !slot_ok(tgt_slot) || (!T && count) || !(std::isfinite(max_dist) && max_dist > 0.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  if (count == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "pose_scores reads back");
  DevBuf dT, dinl, derr;
  if (dT.alloc(count * 64) != hipSuccess || dinl.alloc(count * 4) != hipSuccess || derr.alloc(count * 8) != hipSuccess)
    return set_error(c, MVR_E_NOMEM, "mvr_pose_scores: out of device memory");
  MVR_HIP_TRY(c, hipMemcpyAsync(dT.p, T, count * 64, hipMemcpyHostToDevice, c->stream));
  if (int rc = pose_scores_device(c, c->slots[src_slot], c->slots[tgt_slot], dT.as<float>(), count, max_dist, fma_dist != 0, dinl.as<uint32_t>(),
                                  derr.as<double>())) return rc;
  if (inliers) MVR_HIP_TRY(c, hipMemcpy(inliers, dinl.p, count * 4, hipMemcpyDeviceToHost));
  if (error) MVR_HIP_TRY(c, hipMemcpy(error, derr.p, count * 8, hipMemcpyDeviceToHost));
  return MVR_OK;
}

API int mvr_align_prerejective_dim(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *src_feat, const float *tgt_feat, int dim,
                                   const mvr_prerej_params *p, const float *guess, mvr_prerej_result *result, mvr_prerej_trace *trace)
{
  if (!ctx || !p || !result || !src_feat || !tgt_feat || !slot_ok(src_slot) || !slot_ok(tgt_slot) || !feat_dim_ok(dim)) return MVR_E_ARG;
  if (p->max_iterations < 0 || p->nr_samples < 3 || p->nr_samples > kMaxSamples || p->k < 1 || p->k > MVR_MAX_KNN) return MVR_E_ARG;
  if (!(p->similarity >= 0.0 && p->similarity < 1.0) || !(std::isfinite(p->max_dist) && p->max_dist > 0.0) ||
      !(p->inlier_fraction > 0.0 && p->inlier_fraction <= 1.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return align_prerejective(c, c->slots[src_slot], c->slots[tgt_slot], src_feat, tgt_feat, dim, *p, guess, result, trace);
}

API int mvr_align_prerejective(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *src_feat, const float *tgt_feat,
                               const mvr_prerej_params *p, const float *guess, mvr_prerej_result *result, mvr_prerej_trace *trace)
{
  return mvr_align_prerejective_dim(ctx, src_slot, tgt_slot, src_feat, tgt_feat, kFpfhDim, p, guess, result, trace);
}
