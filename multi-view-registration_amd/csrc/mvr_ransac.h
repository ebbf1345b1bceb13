// csrc/mvr_ransac.h -- what the chunked RANSACs share: mvr_sac.hip (plane segmentation, rules P2 / P7) and mvr_reject_sac.hip
// (the sample-consensus rejector, rules C2 / C7).  Device and host code: include it from a .hip file only.
//
// RANSAC is a sequential loop over attempts whose length depends on what the attempts find.  The attempts themselves do not
// depend on each other (attempt t's samples are a pure function of the seed and t: ransac_draw3), so they are generated and
// scored a CHUNK at a time and the host replays PCL's loop over the chunk's counts (RansacLoop); what lies beyond the stopping
// point is dropped.  How a chunk's hypotheses are made stays with each model; what a model is to the counting kernel is a small
// struct of constants and __device__ __forceinline__ statics:
//   kHypPerStep, kBlocksPerCu     hypotheses read per step of the attempt loop; blocks per CU of the launch
//   Item, item(data, i, pad)      what a thread keeps of item i of the float4 array `data`; pad: i is the last item, read in place
//                                 of one past the end, and its x becomes NaN (never an inlier)
//   Hyp, hyp(hyps, h)             hypothesis h of the float4 array `hyps`; h depends on the loop counter alone
//   inlier<FMA>(hyp, item, bound) the model's test
//
// ransac_count_kernel scores every item against every attempt of the chunk in one pass over the data: a thread keeps kRansacPpt
// items in registers (a tile of 1024 per block, all loads in flight); a hypothesis is the same for every lane, and its address
// depends on the loop counter alone, so it is read by a scalar load into scalar registers, never per lane, kHypPerStep of them
// per step of the loop (a chunk's hypotheses are padded with NaN ones to a multiple of that, ransac_padded; attempts that are
// skipped or invalid are NaN too, so their device counts are 0).  The inliers of a wave are counted by a ballot and a scalar
// population count per item, so the count of (wave, attempt) is a scalar; lane (attempt mod 64) of the wave keeps the running
// count of that attempt in a register, one register per 64 attempts of the chunk (the template parameter G).  After a block's
// last tile the waves add their registers into LDS (one integer LDS atomic per wave and 64 attempts) and the block adds the
// non-zero sums to the global counts (one integer atomic per block and attempt).  No floating-point atomics, no scratch memory.
// An invalid item fails the comparison by itself, and so do the NaN items that pad the last tile.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "mvr_internal.h"

namespace mvr {
namespace {

constexpr int kRansacThreads = 256, kRansacPpt = 4, kRansacTile = kRansacThreads * kRansacPpt;
constexpr int kRansacMaxChunk = 256;       // 64 attempts per register of ransac_count_kernel, at most 4 of them
// the tune keys' 0: 64 attempts for the first chunk, kRansacMaxChunk from then on.  Measured (profiles/reject_sac_bench.json): a
// chunk's cost is its round trips, not its attempts, until there are millions of items; a consensus of everything stops after
// one attempt, which is what the short first chunk is for.
constexpr int kRansacFirstChunk = 64;

// the smallest f32 that is >= t: for an f32 v, (double)v < t  <=>  v < that
inline float f32_at_least(double t)
{
  float f = (float)t;
  if ((double)f < t) f = std::nextafterf(f, INFINITY);
  return f;
}

// P2 / C2: three distinct ranks below nv, each draw over what the earlier ones left, skipping over them in ascending order
__host__ __device__ inline void ransac_draw3(uint64_t seed, uint64_t t, uint32_t nv, uint32_t r[3])
{
  const uint32_t r0 = prerej_draw(seed, t, 0, (uint64_t)nv);
  uint32_t r1 = prerej_draw(seed, t, 1, (uint64_t)(nv - 1u));
  if (r1 >= r0) ++r1;
  const uint32_t lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
  uint32_t r2 = prerej_draw(seed, t, 2, (uint64_t)(nv - 2u));
  if (r2 >= lo) ++r2;
  if (r2 >= hi) ++r2;
  r[0] = r0; r[1] = r1; r[2] = r2;
}

// a chunk's hypotheses, padded to what the counting kernel reads
template <class Model>
__host__ __device__ inline uint32_t ransac_padded(uint32_t count)
{
  static_assert(kRansacMaxChunk % Model::kHypPerStep == 0 && 64 % Model::kHypPerStep == 0, "the padded chunk fits the arrays and the registers");
  return (count + Model::kHypPerStep - 1u) / Model::kHypPerStep * Model::kHypPerStep;
}

template <class Model, int G, bool FMA>
__global__ void __launch_bounds__(kRansacThreads) ransac_count_kernel(const float4 *__restrict__ data, uint32_t n, const float4 *__restrict__ hyps,
                                                                      uint32_t n_hyp, float bound, uint32_t *__restrict__ counts)
{
  constexpr int kStep = Model::kHypPerStep;
  __shared__ uint32_t s_cnt[G * 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t k = tid; k < (uint32_t)(G * 64); k += kRansacThreads) s_cnt[k] = 0u;
  uint32_t acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = 0u;
  const uint32_t tiles = (n + (uint32_t)kRansacTile - 1u) / (uint32_t)kRansacTile, n_pad = ransac_padded<Model>(n_hyp);
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    typename Model::Item item[kRansacPpt];      // independent loads, none behind a branch
#pragma unroll
    for (int j = 0; j < kRansacPpt; ++j) {
      const uint32_t i = tile * (uint32_t)kRansacTile + (uint32_t)j * kRansacThreads + tid;
      item[j] = Model::item(data, i < n ? i : n - 1u, !(i < n));
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t h0 = (uint32_t)g * 64u, hn = n_pad > h0 ? (n_pad - h0 < 64u ? n_pad - h0 : 64u) : 0u;
      for (uint32_t hh = 0; hh < hn; hh += kStep) {
        typename Model::Hyp hyp[kStep];      // the same addresses in every lane: scalar loads, all issued before the first is used
#pragma unroll
        for (int u = 0; u < kStep; ++u) hyp[u] = Model::hyp(hyps, h0 + hh + (uint32_t)u);
#pragma unroll
        for (int u = 0; u < kStep; ++u) {
          uint32_t cnt = 0u;
#pragma unroll
          for (int j = 0; j < kRansacPpt; ++j) cnt += (uint32_t)__popcll(__ballot(Model::template inlier<FMA>(hyp[u], item[j], bound)));
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
  for (uint32_t k = tid; k < n_hyp; k += kRansacThreads)
    if (s_cnt[k]) atomicAdd(&counts[k], s_cnt[k]);
}

// counts[h] += the inliers of hypothesis h < n_hyp among the n items; hyps holds ransac_padded<Model>(n_hyp) hypotheses
template <class Model>
int ransac_launch_count(Ctx *c, bool fma, const float4 *data, size_t n, const float4 *hyps, uint32_t n_hyp, float bound, uint32_t *counts)
{
  using Kernel = void (*)(const float4 *, uint32_t, const float4 *, uint32_t, float, uint32_t *);
  const Kernel kernels[3][2] = {{ransac_count_kernel<Model, 1, false>, ransac_count_kernel<Model, 1, true>},
                                {ransac_count_kernel<Model, 2, false>, ransac_count_kernel<Model, 2, true>},
                                {ransac_count_kernel<Model, 4, false>, ransac_count_kernel<Model, 4, true>}};
  const size_t tiles = (n + kRansacTile - 1) / kRansacTile;
  const unsigned blocks = (unsigned)std::min<size_t>(tiles, (size_t)std::max(c->n_cu, 1) * Model::kBlocksPerCu);
  hipLaunchKernelGGL(kernels[n_hyp <= 64u ? 0 : n_hyp <= 128u ? 1 : 2][fma ? 1 : 0], dim3(blocks), dim3(kRansacThreads), 0, c->stream, data, (uint32_t)n,
                     hyps, n_hyp, bound, counts);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

// what is read back of a chunk: a record per attempt, then the counts, one block of memory (one copy brings both home)
template <class Rec>
struct RansacChunk {
  static constexpr size_t kBytes = kRansacMaxChunk * (sizeof(Rec) + sizeof(uint32_t));
  Rec *rec;
  uint32_t *counts;
  explicit RansacChunk(char *base) : rec(reinterpret_cast<Rec *>(base)), counts(reinterpret_cast<uint32_t *>(base + kRansacMaxChunk * sizeof(Rec))) {}
};

// P7 / C7: PCL's loop, replayed over the chunks.  The caller makes next_chunk() attempts from `attempt` on while more().
struct RansacLoop {
  long long max_it;
  double log_p;          // log(1 - probability)
  uint32_t nv;           // the items the samples are drawn from
  int chunk;             // the tune key: attempts per chunk, 0 = kRansacFirstChunk, then kRansacMaxChunk
  long long iterations = 0, skipped = 0, attempt = 0;
  double k = 1.0;
  bool stop = false;
  long long best_count = -1, best = -1;

  RansacLoop(long long max_it_, double log_p_, uint32_t nv_, int chunk_) : max_it(max_it_), log_p(log_p_), nv(nv_), chunk(chunk_) {}
  long long max_skip() const { return 10ll * max_it; }
  bool more() const { return !stop && (double)iterations < k && skipped < max_skip(); }
  uint32_t next_chunk() const
  {
    // no chunk is longer than what the loop can still consume
    const long long room = (max_it + 1 - iterations) + (max_skip() - skipped);
    const long long want = chunk > 0 ? chunk : (attempt == 0 ? kRansacFirstChunk : kRansacMaxChunk);
    return (uint32_t)std::min<long long>(want, room);
  }
  // status_of(h): 0 = skipped, 1 = counted, anything else = an iteration without inliers; count_of(h): what the kernel counted;
  // on_best(h): h is the best so far; on_attempt(h, attempt, status, count, k): every attempt the loop consumes, k after it
  template <class StatusOf, class CountOf, class OnBest, class OnAttempt>
  void replay(uint32_t count, StatusOf status_of, CountOf count_of, OnBest on_best, OnAttempt on_attempt)
  {
    for (uint32_t h = 0; h < count && more(); ++h, ++attempt) {
      const int status = status_of(h);
      const uint32_t cnt = status == 1 ? count_of(h) : 0u;
      if (status == 0) ++skipped;
      else {
        if ((long long)cnt > best_count) {
          best_count = cnt; best = attempt;
          on_best(h);
          const double w = (double)best_count / (double)nv;
          const double pno = std::min(std::max(1.0 - w * w * w, DBL_EPSILON), 1.0 - DBL_EPSILON);
          k = log_p / std::log(pno);
        }
        ++iterations;
        if (iterations > max_it) stop = true;
      }
      on_attempt(h, attempt, status, cnt, k);
      if (stop) { ++attempt; break; }
    }
  }
};

}  // namespace
}  // namespace mvr
