// csrc/mvr_reject_sac.hip -- pcl::registration::CorrespondenceRejectorSampleConsensus on the GPU (gfx950); the rules C1-C12 are
// written next to mvr_reject_sample_consensus in mvr_hip.h.
//
// A stage of the rejector chain (mvr_reject.hip) that works on the same table -- match[i] = the live match of source point i or
// -1 -- but needs the points, and a RANSAC loop whose length depends on what its attempts find.  The shape is mvr_sac.hip's: the
// attempts do not depend on each other (C2: attempt t's samples are a pure function of the seed and t), so they are generated and
// scored a CHUNK at a time and the host replays PCL's loop over the chunk's counts (C7).
//   1. rsac_valid_kernel + select_flagged + rsac_gather_kernel, once per stage: the valid live pairs (C1) in ascending query
//      index, gathered into a dense array of two 16-byte records per pair, (p_i, bits of i) and (q_j, bits of j).  The random
//      gather of q_j is paid here once, not once per chunk.  nv and the number live come home in one read-back.
//   2. per chunk: rsac_hypotheses_kernel, one thread per attempt -- the draws of C2 through the compacted pairs, the three pairs'
//      coordinates and indices --; ONE read-back; the host solves the attempts (C3: the estimator of the ICP, host SVD) and
//      uploads the chunk's matrices as one block, three float4 rows each, padded with NaN matrices to a multiple of
//      kRsHypPerStep (a skipped attempt is a NaN matrix too: nobody's inlier); rsac_count_kernel, the hot path; ONE read-back
//      of the counts.
//      rsac_count_kernel scores every compacted pair against every attempt of the chunk in one pass: a thread keeps kRsPpt pairs
//      in registers (six floats each; a tile of 1024 pairs per block).  The twelve floats of an attempt are the same for every
//      lane and their address depends on the loop counter alone, so they are scalar loads into scalar registers, kRsHypPerStep
//      attempts per step.  The inliers of a wave are counted by a ballot and a scalar population count per pair; lane
//      (attempt mod 64) keeps the running count of that attempt in a register, one register per 64 attempts of the chunk (the
//      template parameter G).  After a block's last tile the waves add their registers into LDS (one integer LDS atomic per wave
//      and 64 attempts) and the block adds the non-zero sums to the global counts (one integer atomic per block and attempt).
//      No floating-point atomics, no scratch memory.  The pairs that pad the last tile are NaN and fail the comparison.
//   3. rsac_flag_kernel: C9 / C10 for ONE T read from device memory, over the table itself (an invalid pair gives a non-finite
//      d2 and fails): the table of the survivors, their number, and how many entries differ from the round before.  The refit
//      of C10 is launch_moments2 over that table -- the sums the align entries take -- and the host SVD.
//   4. the surviving table replaces match[], and the stage's W_OUT word is copied from the device counter: the stage record
//      rides to the host with the others.
// Everything runs on the context's stream; the work arrays come out of the context's arena (Ctx::dn_arena).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvr_internal.h"

namespace mvr {
namespace {

constexpr int kRsThreads = 256, kRsPpt = 4, kRsTile = kRsThreads * kRsPpt;
constexpr int kRsMaxChunk = 256;       // 64 attempts per register of rsac_count_kernel, at most 4 of them
// "rej_sac_chunk" = 0: 64 attempts for a stage's first chunk, 256 from then on.  Measured (profiles/reject_sac_bench.json): a
// chunk's cost is its two round trips, not its attempts, until the list has millions of pairs; an all-inlier list stops after
// one attempt, which is what the short first chunk is for.
constexpr int kRsFirstChunk = 64;
constexpr int kRsHypPerStep = 2;       // matrices read per step of the counting kernel's attempt loop
static_assert(kRsMaxChunk % kRsHypPerStep == 0 && 64 % kRsHypPerStep == 0, "the padded chunk fits the arrays and the registers");
inline uint32_t rsac_padded(uint32_t count) { return (count + kRsHypPerStep - 1u) / kRsHypPerStep * kRsHypPerStep; }

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
  const uint64_t t = t0 + h;
  const uint32_t r0 = prerej_draw(seed, t, 0, (uint64_t)nv);
  uint32_t r1 = prerej_draw(seed, t, 1, (uint64_t)(nv - 1u));
  if (r1 >= r0) ++r1;
  const uint32_t lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
  uint32_t r2 = prerej_draw(seed, t, 2, (uint64_t)(nv - 2u));
  if (r2 >= lo) ++r2;
  if (r2 >= hi) ++r2;
  const uint32_t r[3] = {r0, r1, r2};
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

template <int G, bool FMA>
__global__ void __launch_bounds__(kRsThreads) rsac_count_kernel(const float4 *__restrict__ pairs, uint32_t nv, const float4 *__restrict__ rows,
                                                                uint32_t n_hyp, uint32_t n_pad, float bound, uint32_t *__restrict__ counts)
{
  __shared__ uint32_t s_cnt[G * 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t k = tid; k < (uint32_t)(G * 64); k += kRsThreads) s_cnt[k] = 0u;
  uint32_t acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0u;
  const uint32_t tiles = (nv + (uint32_t)kRsTile - 1u) / (uint32_t)kRsTile;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // eight independent loads, none behind a branch: past the end the last pair is read and replaced by NaN (never an inlier)
    float px[kRsPpt], py[kRsPpt], pz[kRsPpt], qx[kRsPpt], qy[kRsPpt], qz[kRsPpt];
#pragma unroll
    for (int j = 0; j < kRsPpt; ++j) {
      const uint32_t k = tile * (uint32_t)kRsTile + (uint32_t)j * kRsThreads + tid;
      const size_t kk = k < nv ? k : nv - 1u;
      const float4 p = pairs[2 * kk], q = pairs[2 * kk + 1];
      px[j] = k < nv ? p.x : NAN; py[j] = p.y; pz[j] = p.z; qx[j] = q.x; qy[j] = q.y; qz[j] = q.z;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t h0 = (uint32_t)g * 64u, hn = n_pad > h0 ? (n_pad - h0 < 64u ? n_pad - h0 : 64u) : 0u;
      for (uint32_t hh = 0; hh < hn; hh += kRsHypPerStep) {
        float4 r[kRsHypPerStep][3];      // the same addresses in every lane: scalar loads, all issued before the first is used
#pragma unroll
        for (int u = 0; u < kRsHypPerStep; ++u)
#pragma unroll
          for (int e = 0; e < 3; ++e) r[u][e] = rows[(size_t)(h0 + hh + (uint32_t)u) * 3u + (uint32_t)e];
#pragma unroll
        for (int u = 0; u < kRsHypPerStep; ++u) {
          uint32_t cnt = 0u;
#pragma unroll
          for (int j = 0; j < kRsPpt; ++j)
            cnt += (uint32_t)__popcll(__ballot(rsac_d2<FMA>(r[u][0], r[u][1], r[u][2], px[j], py[j], pz[j], qx[j], qy[j], qz[j]) < bound));
          acc[g] += lane == hh + (uint32_t)u ? cnt : 0u;
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g)
    if (acc[g]) atomicAdd(&s_cnt[g * 64 + (int)lane], acc[g]);
  __syncthreads();
  for (uint32_t k = tid; k < n_hyp; k += kRsThreads)
    if (s_cnt[k]) atomicAdd(&counts[k], s_cnt[k]);
}

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
      if (rsac_d2<FMA>(r0, r1, r2, p.x, p.y, p.z, q.x, q.y, q.z) < bound) { o = j; ++kept; }
    }
    m_out[i] = o;
    if (m_prev && m_prev[i] != o) ++diff;
  }
  block_add2(kept, diff, &cnt[0], &cnt[1]);
}

inline unsigned stride_blocks(size_t n) { return (unsigned)std::min<size_t>(std::max<size_t>((n + kRsThreads - 1) / kRsThreads, 1), 1024); }

template <int G>
void launch_count_g(Ctx *c, bool fma, unsigned blocks, const float4 *pairs, uint32_t nv, const float4 *rows, uint32_t n_hyp, uint32_t n_pad,
                    float bound, uint32_t *counts)
{
  if (fma) hipLaunchKernelGGL((rsac_count_kernel<G, true>), dim3(blocks), dim3(kRsThreads), 0, c->stream, pairs, nv, rows, n_hyp, n_pad, bound, counts);
  else hipLaunchKernelGGL((rsac_count_kernel<G, false>), dim3(blocks), dim3(kRsThreads), 0, c->stream, pairs, nv, rows, n_hyp, n_pad, bound, counts);
}

int launch_count(Ctx *c, bool fma, const float4 *pairs, uint32_t nv, const float4 *rows, uint32_t n_hyp, float bound, uint32_t *counts)
{
  const size_t tiles = ((size_t)nv + kRsTile - 1) / kRsTile;
  const unsigned blocks = (unsigned)std::min<size_t>(tiles, (size_t)std::max(c->n_cu, 1) * 4);
  const uint32_t n_pad = rsac_padded(n_hyp);
  if (n_hyp <= 64u) launch_count_g<1>(c, fma, blocks, pairs, nv, rows, n_hyp, n_pad, bound, counts);
  else if (n_hyp <= 128u) launch_count_g<2>(c, fma, blocks, pairs, nv, rows, n_hyp, n_pad, bound, counts);
  else launch_count_g<4>(c, fma, blocks, pairs, nv, rows, n_hyp, n_pad, bound, counts);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

int launch_flags(Ctx *c, bool fma, const float4 *src, const float4 *tgt, const int32_t *match, size_t ns, const float4 *rows, float bound,
                 int32_t *m_out, const int32_t *m_prev, uint32_t *cnt)
{
  MVR_HIP_TRY(c, hipMemsetAsync(cnt, 0, 2 * sizeof(uint32_t), c->stream));
  if (fma) hipLaunchKernelGGL(rsac_flag_kernel<true>, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, match, ns, rows, bound, m_out, m_prev, cnt);
  else hipLaunchKernelGGL(rsac_flag_kernel<false>, dim3(stride_blocks(ns)), dim3(kRsThreads), 0, c->stream, src, tgt, match, ns, rows, bound, m_out, m_prev, cnt);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

// the smallest f32 that is >= t: for an f32 v, (double)v < t  <=>  v < that
float f32_at_least(double t)
{
  float f = (float)t;
  if ((double)f < t) f = std::nextafterf(f, INFINITY);
  return f;
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
  constexpr size_t kRowsPerChunk = (size_t)kRsMaxChunk * 3;
  Carver plan;
  plan.plan<uint8_t>(ns); plan.plan<unsigned long long>(ns); plan.plan<float4>(2 * ns); plan.plan<int32_t>(ns); plan.plan<int32_t>(ns);
  plan.plan<char>(kRsMaxChunk * (sizeof(RsacHyp) + sizeof(uint32_t))); plan.plan<float4>(kRowsPerChunk); plan.plan<uint32_t>(C_WORDS);
  plan.plan<float4>(3); plan.plan<double>(32); plan.plan<char>(sel_bytes);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  uint8_t *valid = s.take<uint8_t>(ns);
  unsigned long long *vlist = s.take<unsigned long long>(ns);
  float4 *pairs = s.take<float4>(2 * ns);
  int32_t *m_tab[2] = {s.take<int32_t>(ns), nullptr};
  m_tab[1] = s.take<int32_t>(ns);
  char *chunk_dev = s.take<char>(kRsMaxChunk * (sizeof(RsacHyp) + sizeof(uint32_t)));      // the records, then the counts
  RsacHyp *d_hyp = reinterpret_cast<RsacHyp *>(chunk_dev);
  uint32_t *d_counts = reinterpret_cast<uint32_t *>(chunk_dev + kRsMaxChunk * sizeof(RsacHyp));
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
  long long best_count = -1, best = -1;
  float best_T[16];
  RsacHyp best_hyp;
  std::memset(best_T, 0, sizeof best_T);
  std::memset(&best_hyp, 0, sizeof best_hyp);
  if (nv >= 3u) {
    std::vector<char> host(kRsMaxChunk * (sizeof(RsacHyp) + sizeof(uint32_t)));
    const RsacHyp *h_hyp = reinterpret_cast<const RsacHyp *>(host.data());
    const uint32_t *h_counts = reinterpret_cast<const uint32_t *>(host.data() + kRsMaxChunk * sizeof(RsacHyp));
    std::vector<float> h_T((size_t)kRsMaxChunk * 16);
    std::vector<int> h_status(kRsMaxChunk);
    std::vector<float4> h_rows(kRowsPerChunk);
    const long long max_skip = 10ll * max_it;
    const double log_p = std::log(1.0 - 0.99);
    long long iterations = 0, skipped = 0, attempt = 0;
    double k = 1.0;
    bool stop = false, first = true;
    while (!stop && (double)iterations < k && skipped < max_skip) {
      // no chunk is longer than what the loop can still consume
      const long long room = (max_it + 1 - iterations) + (max_skip - skipped);
      const long long want = c->rej_sac_chunk > 0 ? c->rej_sac_chunk : (first ? kRsFirstChunk : kRsMaxChunk);
      const uint32_t count = (uint32_t)std::min<long long>(want, room), n_pad = rsac_padded(count);
      first = false;
      hipLaunchKernelGGL(rsac_hypotheses_kernel, dim3(blocks_for(count, 64)), dim3(64), 0, c->stream, (const float4 *)pairs, nv, (uint64_t)r.seed,
                         (uint64_t)attempt, count, d_hyp, d_counts);
      MVR_HIP_TRY(c, hipGetLastError());
      MVR_HIP_TRY(c, hipMemcpyAsync(host.data(), d_hyp, (size_t)count * sizeof(RsacHyp), hipMemcpyDeviceToHost, c->stream));
      MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (uint32_t h = 0; h < n_pad; ++h) {      // C3
        float *T = &h_T[(size_t)h * 16];
        bool ok = false;
        if (h < count) { pose_from_samples(h_hyp[h], T); ok = finite16(T); h_status[h] = ok ? 1 : 0; }
        if (ok) rows_of(T, &h_rows[(size_t)h * 3]);
        else for (int e = 0; e < 3; ++e) h_rows[(size_t)h * 3 + e] = make_float4(NAN, NAN, NAN, NAN);
      }
      MVR_HIP_TRY(c, hipMemcpyAsync(d_rows, h_rows.data(), (size_t)n_pad * 3 * sizeof(float4), hipMemcpyHostToDevice, c->stream));
      if (int rc = launch_count(c, fma, pairs, nv, d_rows, count, bound, d_counts)) return rc;
      MVR_HIP_TRY(c, hipMemcpyAsync(host.data() + kRsMaxChunk * sizeof(RsacHyp), d_counts, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (uint32_t h = 0; h < count && (double)iterations < k && skipped < max_skip; ++h, ++attempt) {
        const RsacHyp &H = h_hyp[h];
        const int status = h_status[h];
        const uint32_t cnt = status == 1 ? h_counts[h] : 0u;
        if (status == 0) ++skipped;
        else {
          if ((long long)cnt > best_count) {
            best_count = cnt; best = attempt; best_hyp = H;
            std::memcpy(best_T, &h_T[(size_t)h * 16], sizeof best_T);
            const double w = (double)best_count / (double)nv;
            const double pno = std::min(std::max(1.0 - w * w * w, DBL_EPSILON), 1.0 - DBL_EPSILON);
            k = log_p / std::log(pno);
          }
          ++iterations;
          if (iterations > max_it) stop = true;
        }
        if (trace && (size_t)attempt < trace_cap) {
          mvr_rej_sac_trace &Tr = trace[attempt];
          std::memset(&Tr, 0, sizeof Tr);
          Tr.status = status;
          for (int j = 0; j < 3; ++j) { Tr.query[j] = H.query[j]; Tr.match[j] = H.match[j]; }
          if (status == 1) { std::memcpy(Tr.T, &h_T[(size_t)h * 16], sizeof Tr.T); Tr.inliers = cnt; }
          Tr.k = k;
        }
        if (stop) { ++attempt; break; }
      }
    }
    R.iterations = (int)iterations; R.skipped = (int)skipped; R.attempts = (int)attempt; R.k = k;
  }
  R.found = best_count >= 3 ? 1 : 0;      // C8
  if (!R.found) {
    R.inliers = R.live;
    MVR_HIP_TRY(c, hipMemcpyAsync(stage, words + C_LIVE, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  } else {
    R.best_attempt = (int)best;
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
    if ((long long)hc[0] != best_count) return set_error(c, MVR_E_HIP, "sample-consensus rejector: the best attempt's count and its inliers disagree");
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
