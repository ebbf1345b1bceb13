// csrc/mvr_reject_sac.hip -- pcl::registration::CorrespondenceRejectorSampleConsensus on the GPU (gfx950); the rules C1-C12 are
// written next to mvr_reject_sample_consensus in mvr_hip.h.
//
// A stage of the rejector chain (mvr_reject.hip) that works on the same table -- match[i] = the live match of source point i or
// -1 -- but needs the points, and a RANSAC loop whose length depends on what its attempts find.  The chunked RANSAC -- the
// draws, the counting kernel, the host's replay of PCL's loop -- is mvr_ransac.h, shared with mvr_sac.hip; what this file adds:
//   1. rsac_valid_kernel + select_flagged + rsac_gather_kernel, once per stage: the valid live pairs (C1) in ascending query
//      index, gathered into a dense array of two 16-byte records per pair, (p_i, bits of i) and (q_j, bits of j).  The random
//      gather of q_j is paid here once, not once per chunk.  nv and the number live come home in one read-back.
//   2. per chunk: rsac_hypotheses_kernel, one thread per attempt -- the draws of C2 through the compacted pairs, the three pairs'
//      coordinates and indices --; ONE read-back; the host solves the attempts (C3: the estimator of the ICP, host SVD) and
//      uploads the chunk's matrices as one block, padded with NaN matrices (a skipped attempt is a NaN matrix too: nobody's
//      inlier); the counting kernel over RigidModel (an item is a compacted pair, six floats; a hypothesis the three float4
//      rows of T, two per step); ONE read-back of the counts.
//   3. rsac_flag_kernel: C9 / C10 for ONE T read from device memory, over the table itself (an invalid pair gives a non-finite
//      d2 and fails): the table of the survivors, their number, and how many entries differ from the round before.  The refit
//      of C10 is launch_moments2 over that table -- the sums the align entries take -- and the host SVD.
//   4. the surviving table replaces match[], and the stage's W_OUT word is copied from the device counter: the stage record
//      rides to the host with the others.
// Everything runs on the context's stream; the work arrays come out of the context's arena (Ctx::dn_arena).
#include <cmath>
#include <cstring>
#include <vector>

#include "mvr_internal.h"
#include "mvr_ransac.h"

namespace mvr {
namespace {

constexpr int kRsThreads = 256;      // the block of this file's own kernels

// what the host reads back of an attempt: the three sampled pairs, in sample order
struct RsacHyp { float p[9], q[9]; uint32_t query[3], match[3]; };
static_assert(sizeof(RsacHyp) == 96, "RsacHyp is read back as it is");

// device words of a stage
enum { C_NV = 0, C_LIVE = 1, C_CNT_A = 2, C_DIFF_A = 3, C_CNT_B = 4, C_DIFF_B = 5, C_WORDS = 8 };

// the block's sums of a and b added to dst_a / dst_b with one atomic each (none when a sum is 0)
__device__ __forceinline__ void block_add2(uint32_t a, uint32_t b, uint32_t *dst_a, uint32_t *dst_b)
{
  __shared__ uint32_t wa[kRsThreads / 64], wb[kRsThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  if ((threadIdx.x & 63) == 0) { wa[threadIdx.x >> 6] = a; wb[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sa = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < kRsThreads / 64; ++w) { sa += wa[w]; sb += wb[w]; }
    if (sa) atomicAdd(dst_a, sa);
    if (sb && dst_b) atomicAdd(dst_b, sb);
  }
}

// C1
__global__ void __launch_bounds__(kRsThreads)
rsac_valid_kernel(const float4 *__restrict__ src, const float4 *__restrict__ tgt, const int32_t *__restrict__ match, size_t ns,
                  uint8_t *__restrict__ valid, uint32_t *__restrict__ words)
{
  uint32_t live = 0;
  const size_t stride = (size_t)gridDim.x * kRsThreads;
  for (size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x; i < ns; i += stride) {
    const int32_t j = match[i];
    bool ok = false;
    if (j >= 0) { ++live; ok = finite3(src[i]) && finite3(tgt[j]); }
    valid[i] = ok ? 1 : 0;
  }
  block_add2(live, 0u, &words[C_LIVE], nullptr);
}

__global__ void __launch_bounds__(kRsThreads)
rsac_gather_kernel(const float4 *__restrict__ src, const float4 *__restrict__ tgt, const int32_t *__restrict__ match,
                   const unsigned long long *__restrict__ vlist, const uint32_t *__restrict__ words, float4 *__restrict__ pairs)
{
  const size_t nv = words[C_NV], stride = (size_t)gridDim.x * kRsThreads;
  for (size_t k = (size_t)blockIdx.x * kRsThreads + threadIdx.x; k < nv; k += stride) {
    const uint32_t i = (uint32_t)vlist[k];
    const int32_t j = match[i];
    float4 p = src[i], q = tgt[j];
    p.w = __uint_as_float(i); q.w = __uint_as_float((uint32_t)j);
    pairs[2 * k] = p; pairs[2 * k + 1] = q;
  }
}

// C2, and the samples' coordinates for the host's solve
__global__ void __launch_bounds__(64)
rsac_hypotheses_kernel(const float4 *__restrict__ pairs, uint32_t nv, uint64_t seed, uint64_t t0, uint32_t count, RsacHyp *__restrict__ hyp,
                       uint32_t *__restrict__ counts)
{
  const uint32_t h = blockIdx.x * 64 + threadIdx.x;
  if (h >= count) return;
  uint32_t r[3];
  ransac_draw3(seed, t0 + h, nv, r);
  RsacHyp out;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const float4 p = pairs[2 * (size_t)r[s]], q = pairs[2 * (size_t)r[s] + 1];
    out.p[3 * s] = p.x; out.p[3 * s + 1] = p.y; out.p[3 * s + 2] = p.z;
    out.q[3 * s] = q.x; out.q[3 * s + 1] = q.y; out.q[3 * s + 2] = q.z;
    out.query[s] = __float_as_uint(p.w); out.match[s] = __float_as_uint(q.w);
  }
  hyp[h] = out;
  counts[h] = 0u;
}

// C4 + C5: rows r0, r1, r2 of T (x, y, z: the rotation's row; w: the translation's entry)
template <bool FMA>
__device__ __forceinline__ float rsac_d2(const float4 r0, const float4 r1, const float4 r2, const float px, const float py, const float pz,
                                         const float qx, const float qy, const float qz)
{
  const float x = ((r0.x * px + r0.y * py) + r0.z * pz) + r0.w;
  const float y = ((r1.x * px + r1.y * py) + r1.z * pz) + r1.w;
  const float z = ((r2.x * px + r2.y * py) + r2.z * pz) + r2.w;
  const float dx = x - qx, dy = y - qy, dz = z - qz;
  if (FMA) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  return (dx * dx + dy * dy) + dz * dz;
}

// the rigid motion to the counting kernel of mvr_ransac.h
struct RigidModel {
  static constexpr int kHypPerStep = 2, kBlocksPerCu = 4;
  struct Item { float px, py, pz, qx, qy, qz; };
  struct Hyp { float4 r0, r1, r2; };
  static __device__ __forceinline__ Item item(const float4 *__restrict__ pairs, uint32_t k, bool pad)
  {
    const float4 p = pairs[2 * (size_t)k], q = pairs[2 * (size_t)k + 1];
    return {pad ? NAN : p.x, p.y, p.z, q.x, q.y, q.z};
  }
  static __device__ __forceinline__ Hyp hyp(const float4 *__restrict__ rows, uint32_t h)
  {
    return {rows[(size_t)h * 3u], rows[(size_t)h * 3u + 1u], rows[(size_t)h * 3u + 2u]};
  }
  template <bool FMA>
  static __device__ __forceinline__ bool inlier(const Hyp T, const Item m, float bound)
  {
    return rsac_d2<FMA>(T.r0, T.r1, T.r2, m.px, m.py, m.pz, m.qx, m.qy, m.qz) < bound;
  }
};

// C9 / C10 for the T at `rows`: m_out = the table of its inliers; cnt[0] += their number, cnt[1] += the entries that differ from m_prev
template <bool FMA>
__global__ void __launch_bounds__(kRsThreads)
rsac_flag_kernel(const float4 *__restrict__ src, const float4 *__restrict__ tgt, const int32_t *__restrict__ match, size_t ns,
                 const float4 *__restrict__ rows, float bound, int32_t *__restrict__ m_out, const int32_t *__restrict__ m_prev,
                 uint32_t *__restrict__ cnt)
{
  const float4 r0 = rows[0], r1 = rows[1], r2 = rows[2];
  uint32_t kept = 0, diff = 0;
  const size_t stride = (size_t)gridDim.x * kRsThreads;
  for (size_t i = (size_t)blockIdx.x * kRsThreads + threadIdx.x; i < ns; i += stride) {
    const int32_t j = match[i];
    int32_t o = -1;
    if (j >= 0) {
      const float4 p = src[i], q = tgt[j];
      if (RigidModel::inlier<FMA>({r0, r1, r2}, {p.x, p.y, p.z, q.x, q.y, q.z}, bound)) { o = j; ++kept; }
    }
    m_out[i] = o;
    if (m_prev && m_prev[i] != o) ++diff;
  }
  block_add2(kept, diff, &cnt[0], &cnt[1]);
}

inline unsigned stride_blocks(size_t n) { return (unsigned)std::min<size_t>(std::max<size_t>((n + kRsThreads - 1) / kRsThreads, 1), 1024); }

int launch_flags(Ctx *c, bool fma, const float4 *src, const float4 *tgt, const int32_t *match, size_t ns, const float4 *rows, float bound,
                 int32_t *m_out, const int32_t *m_prev, uint32_t *cnt)
{
  MVR_HIP_TRY(c, hipMemsetAsync(cnt, 0, 2 * sizeof(uint32_t), c->stream));
  if (fma) hipLaunchKernelGGL(rsac_flag_kernel<true>, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, match, ns, rows, bound, m_out, m_prev, cnt);
  else hipLaunchKernelGGL(rsac_flag_kernel<false>, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, match, ns, rows, bound, m_out, m_prev, cnt);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

// C3: rule A5's estimator on the three pairs in sample order
void pose_from_samples(const RsacHyp &H, float T[16])
{
  double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0}, sigma[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < 3; ++j)
    for (int a = 0; a < 3; ++a) { ms[a] += (double)H.p[3 * j + a]; mt[a] += (double)H.q[3 * j + a]; }
  for (int a = 0; a < 3; ++a) { ms[a] /= 3.0; mt[a] /= 3.0; }
  for (int j = 0; j < 3; ++j) {
    double dp[3], dq[3];
    for (int a = 0; a < 3; ++a) { dp[a] = (double)H.p[3 * j + a] - ms[a]; dq[a] = (double)H.q[3 * j + a] - mt[a]; }
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) sigma[3 * r + k] += dq[r] * dp[k];
  }
  for (int e = 0; e < 9; ++e) sigma[e] /= 3.0;
  umeyama_from_moments(ms, mt, sigma, T, nullptr);
}

bool finite16(const float T[16])
{
  for (int k = 0; k < 16; ++k) if (!std::isfinite(T[k])) return false;
  return true;
}

// column-major 4 x 4 -> the three rows the kernels read
void rows_of(const float T[16], float4 rows[3])
{
  for (int r = 0; r < 3; ++r) rows[r] = make_float4(T[r], T[r + 4], T[r + 8], T[r + 12]);
}

}  // namespace

void reject_sac_identity(mvr_rej_sac_result *R)
{
  std::memset(R, 0, sizeof *R);
  R->best_attempt = -1;
  R->k = 1.0;
  for (int k = 0; k < 4; ++k) R->T[5 * k] = R->ransac_T[5 * k] = 1.0f;
}

int reject_sac_stage(Ctx *c, const mvr_rejector &r, bool fma, const float4 *src, const float4 *tgt, int32_t *match, size_t ns, uint32_t *stage,
                     mvr_rej_sac_trace *trace, size_t trace_cap)
{
  MVR_MAY_BLOCK(c, "the sample-consensus rejector reads back");
  if (!src || !tgt) return set_error(c, MVR_E_ARG, "the sample-consensus rejector needs the points of both clouds");
  const long long max_it = r.max_iterations ? (long long)r.max_iterations : 1000ll;
  const float bound = f32_at_least(r.value * r.value);
  mvr_rej_sac_result R;
  reject_sac_identity(&R);

  size_t sel_bytes = 0;
  if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, ns, nullptr, nullptr)) return rc;
  constexpr size_t kRowsPerChunk = (size_t)kRansacMaxChunk * 3;
  Carver plan;
  plan.plan<uint8_t>(ns); plan.plan<unsigned long long>(ns); plan.plan<float4>(2 * ns); plan.plan<int32_t>(ns); plan.plan<int32_t>(ns);
  plan.plan<char>(RansacChunk<RsacHyp>::kBytes); plan.plan<float4>(kRowsPerChunk); plan.plan<uint32_t>(C_WORDS);
  plan.plan<float4>(3); plan.plan<double>(32); plan.plan<char>(sel_bytes);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  uint8_t *valid = s.take<uint8_t>(ns);
  unsigned long long *vlist = s.take<unsigned long long>(ns);
  float4 *pairs = s.take<float4>(2 * ns);
  int32_t *m_tab[2] = {s.take<int32_t>(ns), nullptr};
  m_tab[1] = s.take<int32_t>(ns);
  const RansacChunk<RsacHyp> dev(s.take<char>(RansacChunk<RsacHyp>::kBytes));
  float4 *d_rows = s.take<float4>(kRowsPerChunk);
  uint32_t *words = s.take<uint32_t>(C_WORDS);
  float4 *d_T = s.take<float4>(3);
  double *d_mom = s.take<double>(32);
  char *sel_tmp = s.take<char>(sel_bytes);

  // C1
  MVR_HIP_TRY(c, hipMemsetAsync(words, 0, C_WORDS * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(rsac_valid_kernel, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, (const int32_t *)match, ns, valid, words);
  MVR_HIP_TRY(c, hipGetLastError());
  if (int rc = select_flagged(c, sel_tmp, sel_bytes, valid, ns, vlist, words + C_NV)) return rc;
  hipLaunchKernelGGL(rsac_gather_kernel, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, (const int32_t *)match,
                     (const unsigned long long *)vlist, (const uint32_t *)words, pairs);
  MVR_HIP_TRY(c, hipGetLastError());
  uint32_t hw[2] = {0, 0};
  MVR_HIP_TRY(c, hipMemcpyAsync(hw, words, sizeof hw, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t nv = hw[C_NV];
  R.live = hw[C_LIVE]; R.valid = nv;

  // C7 over the chunks
  RansacLoop loop(max_it, std::log(1.0 - 0.99), nv, c->rej_sac_chunk);
  float best_T[16];
  RsacHyp best_hyp;
  std::memset(best_T, 0, sizeof best_T);
  std::memset(&best_hyp, 0, sizeof best_hyp);
  if (nv >= 3u) {
    std::vector<char> host_mem(RansacChunk<RsacHyp>::kBytes);
    const RansacChunk<RsacHyp> host(host_mem.data());
    std::vector<float> h_T((size_t)kRansacMaxChunk * 16);
    std::vector<int> h_status(kRansacMaxChunk);
    std::vector<float4> h_rows(kRowsPerChunk);
    while (loop.more()) {
      const uint32_t count = loop.next_chunk(), n_pad = ransac_padded<RigidModel>(count);
      hipLaunchKernelGGL(rsac_hypotheses_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, c->stream, (const float4 *)pairs, nv, (uint64_t)r.seed,
                         (uint64_t)loop.attempt, count, dev.rec, dev.counts);
      MVR_HIP_TRY(c, hipGetLastError());
      MVR_HIP_TRY(c, hipMemcpyAsync(host.rec, dev.rec, (size_t)count * sizeof(RsacHyp), hipMemcpyDeviceToHost, c->stream));
      MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (uint32_t h = 0; h < n_pad; ++h) {      // C3
        float *T = &h_T[(size_t)h * 16];
        bool ok = false;
        if (h < count) { pose_from_samples(host.rec[h], T); ok = finite16(T); h_status[h] = ok ? 1 : 0; }
        if (ok) rows_of(T, &h_rows[(size_t)h * 3]);
        else for (int e = 0; e < 3; ++e) h_rows[(size_t)h * 3 + e] = make_float4(NAN, NAN, NAN, NAN);
      }
      MVR_HIP_TRY(c, hipMemcpyAsync(d_rows, h_rows.data(), (size_t)n_pad * 3 * sizeof(float4), hipMemcpyHostToDevice, c->stream));
      if (int rc = ransac_launch_count<RigidModel>(c, fma, pairs, nv, d_rows, count, bound, dev.counts)) return rc;
      MVR_HIP_TRY(c, hipMemcpyAsync(host.counts, dev.counts, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
      loop.replay(
          count, [&](uint32_t h) { return h_status[h]; }, [&](uint32_t h) { return host.counts[h]; },
          [&](uint32_t h) { best_hyp = host.rec[h]; std::memcpy(best_T, &h_T[(size_t)h * 16], sizeof best_T); },
          [&](uint32_t h, long long attempt, int status, uint32_t cnt, double k) {
            if (!trace || (size_t)attempt >= trace_cap) return;
            const RsacHyp &H = host.rec[h];
            mvr_rej_sac_trace &Tr = trace[attempt];
            std::memset(&Tr, 0, sizeof Tr);
            Tr.status = status;
            for (int j = 0; j < 3; ++j) { Tr.query[j] = H.query[j]; Tr.match[j] = H.match[j]; }
            if (status == 1) { std::memcpy(Tr.T, &h_T[(size_t)h * 16], sizeof Tr.T); Tr.inliers = cnt; }
            Tr.k = k;
          });
    }
  }
  R.iterations = (int)loop.iterations; R.skipped = (int)loop.skipped; R.attempts = (int)loop.attempt; R.k = loop.k;
  R.found = loop.best_count >= 3 ? 1 : 0;      // C8
  if (!R.found) {
    R.inliers = R.live;
    MVR_HIP_TRY(c, hipMemcpyAsync(stage, words + C_LIVE, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  } else {
    R.best_attempt = (int)loop.best;
    std::memcpy(R.ransac_T, best_T, sizeof best_T);
    std::memcpy(R.T, best_T, sizeof best_T);
    // C9
    float4 rows[3];
    rows_of(best_T, rows);
    int cur = 0;
    uint32_t hc[2] = {0, 0};
    MVR_HIP_TRY(c, hipMemcpyAsync(d_T, rows, sizeof rows, hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_flags(c, fma, src, tgt, match, ns, d_T, bound, m_tab[cur], nullptr, words + C_CNT_A)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, words + C_CNT_A, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((long long)hc[0] != loop.best_count) return set_error(c, MVR_E_HIP, "sample-consensus rejector: the best attempt's count and its inliers disagree");
    R.ransac_inliers = R.inliers = hc[0];
    if (r.refine) {      // C10
      const double origin[3] = {(double)best_hyp.q[0], (double)best_hyp.q[1], (double)best_hyp.q[2]};
      for (long long round = 1;; ++round) {
        R.refine_rounds = (int)round;
        if (int rc = launch_moments2(c, src, tgt, m_tab[cur], nullptr, nullptr, 0, ns, origin, d_mom)) return rc;
        mvr_pair_moments2_t m2;
        static_assert(sizeof m2 == 32 * sizeof(double), "moments2 layout");
        MVR_HIP_TRY(c, hipMemcpyAsync(&m2, d_mom, sizeof m2, hipMemcpyDeviceToHost, c->stream));
        MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
        mvr_pair_moments_t mom;
        float Tr[16];
        if (mvr_moments_from_moments2(&m2, &mom) != MVR_OK) break;
        umeyama_from_moments(mom.mean_src, mom.mean_tgt, mom.sigma, Tr, nullptr);
        if (!finite16(Tr)) break;
        rows_of(Tr, rows);
        const int nxt = cur ^ 1;
        uint32_t *cw = words + (nxt ? C_CNT_B : C_CNT_A);
        MVR_HIP_TRY(c, hipMemcpyAsync(d_T, rows, sizeof rows, hipMemcpyHostToDevice, c->stream));
        if (int rc = launch_flags(c, fma, src, tgt, match, ns, d_T, bound, m_tab[nxt], m_tab[cur], cw)) return rc;
        MVR_HIP_TRY(c, hipMemcpyAsync(hc, cw, sizeof hc, hipMemcpyDeviceToHost, c->stream));
        MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (hc[0] < 3u) break;
        const bool same = hc[1] == 0u;
        if (same || round >= max_it) {
          cur = nxt; R.inliers = hc[0];
          std::memcpy(R.T, Tr, sizeof Tr);
          break;
        }
        cur = nxt; R.inliers = hc[0];
        std::memcpy(R.T, Tr, sizeof Tr);
      }
    }
    MVR_HIP_TRY(c, hipMemcpyAsync(match, m_tab[cur], ns * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    MVR_HIP_TRY(c, hipMemcpyAsync(stage, words + (cur ? C_CNT_B : C_CNT_A), sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  }
  c->last_sac = R;
  c->last_sac_set = true;
  return MVR_OK;
}

}  // namespace mvr
