// csrc/mvr_reject.hip -- pcl::registration::CorrespondenceRejector{Distance, MedianDistance, Trimmed, SurfaceNormal, OneToOne}
// on the GPU (gfx950); the rules R1-R10 are written next to mvr_correspondences_rejected in mvr_hip.h.
//
// The chain works on the table an ICP iteration's search leaves on the device -- keys[i] = d2 bits << 32 | match, match[i] =
// the accepted match or -1, one entry per source point -- in place: a rejected entry gets match = -1, and the sums launch that
// follows (moments2_kernel / p2plane_kernel) reads the rewritten match[].  Nothing comes to the host in between: every count
// and threshold a later launch needs is a word of Ctx::rej_row, and the words ride to the host with the iteration's sums.
//
//   MEDIAN / TRIMMED  exact order statistic of the live d2: non-negative floats order as their uint32 patterns, so the k-th
//                     smallest is found by a radix select over the patterns, 11 / 11 / 10 bits in three levels.  A level is
//                     two launches: rej_hist_kernel (per-block LDS histogram over a grid-stride pass, ONE integer global
//                     atomic per non-empty bin per block) and rej_scan_kernel (one block: scans the bins, writes the chosen
//                     prefix and the rank that is left, clears the bins).  Levels hand over at launch boundaries.
//   TRIMMED's ties    everything below the selected value is kept; of the entries EQUAL to it the first `need` in ascending
//                     query index.  rej_tie_count_kernel counts the equals of consecutive index ranges (one per block),
//                     rej_trim_kernel sums the counts of the blocks before its own and ranks its equals by ballot / popcount.
//   ONE_TO_ONE        atomicMin of (d2 bits << 32 | query) per matched target, a pass that keeps the winners, and a pass that
//                     puts the touched words back to ~0: the table is as large as the target but only what the matches touch
//                     is ever written.
//   SAMPLE_CONSENSUS  the one stage that needs the points and the host: mvr_reject_sac.hip (rules C1-C12).  It synchronises the
//                     stream; the stages around it queue as before and its W_OUT word rides with theirs.
// Counts are integer atomics (one per block), so every result is independent of the launch shape and of arrival order.
#include "mvr_internal.h"

namespace mvr {

namespace {

constexpr int kRejT = 256;              // threads per block of every kernel here
constexpr int kRejMaxBlocks = 1024;     // grid-stride passes

enum { W_OUT = 0, W_THR = 1, W_PREFIX = 2, W_RANK = 3, W_NONE = 4 };

__device__ __forceinline__ uint32_t d2_bits(nnkey_t k) { return (uint32_t)(k >> 32); }

// the block's sum of `v` added to *dst with one atomic (none when the sum is 0)
__device__ __forceinline__ void block_count_add(uint32_t v, uint32_t *dst)
{
  __shared__ uint32_t wsum[kRejT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kRejT / 64; ++w) s += wsum[w];
    if (s) atomicAdd(dst, s);
  }
}

__global__ void __launch_bounds__(kRejT) rej_init_kernel(uint32_t *__restrict__ words, int n_words, const double *__restrict__ found,
                                                          uint32_t found_host)
{
  for (int k = threadIdx.x; k < n_words; k += kRejT) words[k] = 0u;
  __syncthreads();
  if (threadIdx.x == 0) words[0] = found ? (uint32_t)*found : found_host;
}

// R2 / R3 / R5: a predicate per live entry
template <int KIND>
__global__ void __launch_bounds__(kRejT)
rej_apply_kernel(const nnkey_t *__restrict__ keys, int32_t *__restrict__ match, size_t ns, double value, const float4 *__restrict__ snrm,
                 const float4 *__restrict__ tnrm, uint32_t *__restrict__ stage)
{
  double cut = value;
  if (KIND == MVR_REJ_MEDIAN) cut = (double)__uint_as_float(stage[W_THR]) * value;
  uint32_t kept = 0;
  const size_t stride = (size_t)gridDim.x * kRejT;
  for (size_t i = (size_t)blockIdx.x * kRejT + threadIdx.x; i < ns; i += stride) {
    const int32_t j = match[i];
    if (j < 0) continue;
    bool keep;
    if (KIND == MVR_REJ_SURFACE_NORMAL) {
      const float4 n = snrm[i], t = tnrm[j];
      const float dot = __fadd_rn(__fadd_rn(__fmul_rn(n.x, t.x), __fmul_rn(n.y, t.y)), __fmul_rn(n.z, t.z));
      keep = (double)dot > cut;                                                       // (a NaN fails)
    } else {
      const double d2 = (double)__uint_as_float(d2_bits(keys[i]));
      keep = (KIND == MVR_REJ_DISTANCE) ? (d2 < cut) : (d2 <= cut);
    }
    if (keep) ++kept; else match[i] = -1;
  }
  block_count_add(kept, &stage[W_OUT]);
}

// one level of the radix select: the live entries whose pattern continues the prefix chosen so far, by their next bits
__global__ void __launch_bounds__(kRejT)
rej_hist_kernel(const nnkey_t *__restrict__ keys, const int32_t *__restrict__ match, size_t ns, int level, const uint32_t *__restrict__ stage,
                uint32_t *__restrict__ hist)
{
  __shared__ uint32_t h[kRejHistBins];
  for (int b = threadIdx.x; b < kRejHistBins; b += kRejT) h[b] = 0u;
  __syncthreads();
  const uint32_t prefix = level ? stage[W_PREFIX] : 0u;
  const size_t stride = (size_t)gridDim.x * kRejT;
  for (size_t i = (size_t)blockIdx.x * kRejT + threadIdx.x; i < ns; i += stride) {
    if (match[i] < 0) continue;
    const uint32_t bits = d2_bits(keys[i]);
    if (level == 0) atomicAdd(&h[bits >> 21], 1u);
    else if (level == 1) { if ((bits >> 21) == (prefix >> 21)) atomicAdd(&h[(bits >> 10) & 0x7FFu], 1u); }
    else if ((bits >> 10) == (prefix >> 10)) atomicAdd(&h[bits & 0x3FFu], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kRejHistBins; b += kRejT) {
    const uint32_t v = h[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

// ... and its one-block scan: the bin that holds the wanted rank extends the prefix; the rank inside that bin goes on to the
// next level; the bins are cleared for it.  Level 0 first derives the rank from the number live (R3: m / 2; R4: min(nv, m) - 1).
__global__ void __launch_bounds__(kRejT)
rej_scan_kernel(int level, int kind, double value, uint32_t min_corr, const uint32_t *__restrict__ live_in, uint32_t *__restrict__ stage,
                uint32_t *__restrict__ hist)
{
  __shared__ uint32_t sums[kRejT], excl[kRejT];
  constexpr int kPer = kRejHistBins / kRejT;
  uint32_t rank, none, prefix;
  if (level == 0) {
    const uint32_t m = *live_in;
    none = 0u; rank = 0u; prefix = 0u;
    if (m == 0u) none = 1u;
    else if (kind == MVR_REJ_MEDIAN) rank = m / 2u;
    else {
      const double f = floor(value * (double)m);
      uint32_t nv = f >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)f;
      if (nv < min_corr) nv = min_corr;
      if (nv == 0u) none = 1u; else rank = (nv < m ? nv : m) - 1u;
    }
  } else { prefix = stage[W_PREFIX]; rank = stage[W_RANK]; none = stage[W_NONE]; }
  uint32_t bin[kPer], s = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) { bin[k] = hist[threadIdx.x * kPer + k]; s += bin[k]; }
#pragma unroll
  for (int k = 0; k < kPer; ++k) hist[threadIdx.x * kPer + k] = 0u;
  sums[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < kRejT; ++t) { excl[t] = run; run += sums[t]; }
    if (level == 0) { stage[W_PREFIX] = 0u; stage[W_RANK] = rank; stage[W_NONE] = none; }
  }
  __syncthreads();
  uint32_t lo = excl[threadIdx.x];
  if (!none && rank >= lo && rank - lo < s) {            // exactly one thread: the bins hold rank + 1 entries or more
    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      if (rank - lo < bin[k]) {
        prefix |= (uint32_t)(threadIdx.x * kPer + k) << shift;
        stage[W_PREFIX] = prefix; stage[W_RANK] = rank - lo;
        if (level == 2) stage[W_THR] = prefix;
        break;
      }
      lo += bin[k];
    }
  }
  if (none && level == 2 && threadIdx.x == 0) { stage[W_THR] = 0u; stage[W_PREFIX] = 0u; stage[W_RANK] = 0u; }
}

// R4's tie rule, first half: how many live entries EQUAL the selected value lie in each block's range of consecutive indices
__global__ void __launch_bounds__(kRejT)
rej_tie_count_kernel(const nnkey_t *__restrict__ keys, const int32_t *__restrict__ match, size_t ns, size_t chunk, const uint32_t *__restrict__ stage,
                     uint32_t *__restrict__ tie)
{
  __shared__ uint32_t total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  const uint32_t val = stage[W_PREFIX];
  const size_t b0 = (size_t)blockIdx.x * chunk, b1 = b0 + chunk < ns ? b0 + chunk : ns;
  uint32_t n = 0;
  for (size_t i = b0 + threadIdx.x; i < b1; i += kRejT)
    if (match[i] >= 0 && d2_bits(keys[i]) == val) ++n;
  block_count_add(n, &total);
  __syncthreads();
  if (threadIdx.x == 0) tie[blockIdx.x] = total;
}

// ... second half: keep what lies below the value, and of the equals those whose rank in ascending query index is below `need`
__global__ void __launch_bounds__(kRejT)
rej_trim_kernel(const nnkey_t *__restrict__ keys, int32_t *__restrict__ match, size_t ns, size_t chunk, uint32_t *__restrict__ stage,
                const uint32_t *__restrict__ tie)
{
  __shared__ uint32_t wsum[kRejT / 64], base_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // exclusive sum of the equals in the blocks before this one
  uint32_t before = 0;
  for (unsigned b = threadIdx.x; b < blockIdx.x; b += kRejT) before += tie[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  if (lane == 0) wsum[wave] = before;
  __syncthreads();
  if (threadIdx.x == 0) { uint32_t s = 0; for (int w = 0; w < kRejT / 64; ++w) s += wsum[w]; base_s = s; }
  __syncthreads();
  uint32_t running = base_s;
  const uint32_t val = stage[W_PREFIX];
  const uint32_t need = stage[W_NONE] ? 0u : stage[W_RANK] + 1u;
  const size_t b0 = (size_t)blockIdx.x * chunk, b1 = b0 + chunk < ns ? b0 + chunk : ns;
  uint32_t kept = 0;
  for (size_t t0 = b0; t0 < b1; t0 += kRejT) {          // (uniform over the block: chunk is a multiple of the block)
    const size_t i = t0 + threadIdx.x;
    bool live = false, eq = false;
    uint32_t bits = 0;
    if (i < b1 && match[i] >= 0) { live = true; bits = d2_bits(keys[i]); eq = bits == val; }
    const unsigned long long mask = __ballot(eq);
    __syncthreads();                                      // (wsum of the tile before has been read)
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t r = running + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), tile = 0;
#pragma unroll
    for (int w = 0; w < kRejT / 64; ++w) { if (w < wave) r += wsum[w]; tile += wsum[w]; }
    running += tile;
    if (live) {
      if (bits < val || (eq && r < need)) ++kept; else match[i] = -1;
    }
  }
  __syncthreads();
  block_count_add(kept, &stage[W_OUT]);
}

// R6
__global__ void __launch_bounds__(kRejT)
rej_oto_min_kernel(const nnkey_t *__restrict__ keys, const int32_t *__restrict__ match, size_t ns, nnkey_t *__restrict__ win)
{
  const size_t stride = (size_t)gridDim.x * kRejT;
  for (size_t i = (size_t)blockIdx.x * kRejT + threadIdx.x; i < ns; i += stride) {
    const int32_t j = match[i];
    if (j >= 0) atomicMin(&win[j], (keys[i] & 0xFFFFFFFF00000000ull) | (nnkey_t)i);
  }
}

__global__ void __launch_bounds__(kRejT)
rej_oto_keep_kernel(const nnkey_t *__restrict__ keys, int32_t *__restrict__ match, size_t ns, const nnkey_t *__restrict__ win,
                    uint32_t *__restrict__ stage)
{
  uint32_t kept = 0;
  const size_t stride = (size_t)gridDim.x * kRejT;
  for (size_t i = (size_t)blockIdx.x * kRejT + threadIdx.x; i < ns; i += stride) {
    const int32_t j = match[i];
    if (j < 0) continue;
    if (win[j] == ((keys[i] & 0xFFFFFFFF00000000ull) | (nnkey_t)i)) ++kept; else match[i] = -1;
  }
  block_count_add(kept, &stage[W_OUT]);
}

// every word a live match can have touched is the word of some key's match, live or rejected: back to "no winner"
__global__ void __launch_bounds__(kRejT)
rej_oto_clear_kernel(const nnkey_t *__restrict__ keys, size_t ns, size_t nt, nnkey_t *__restrict__ win)
{
  const size_t stride = (size_t)gridDim.x * kRejT;
  for (size_t i = (size_t)blockIdx.x * kRejT + threadIdx.x; i < ns; i += stride) {
    const uint32_t j = (uint32_t)keys[i];
    if (j != kNone && (size_t)j < nt) win[j] = kKeyInit;
  }
}

inline unsigned stride_blocks(size_t n) { return (unsigned)std::min<size_t>(std::max<size_t>((n + kRejT - 1) / kRejT, 1), kRejMaxBlocks); }

}  // namespace

int ensure_reject_state(Ctx *c, size_t nt, bool one_to_one)
{
  if (!c->rej_row) {
    MVR_MAY_BLOCK(c, "the rejectors' state is not allocated yet");
    MVR_HIP_TRY(c, hipMalloc(&c->rej_row, kRejRowBytes));
    MVR_HIP_TRY(c, hipMemsetAsync(c->rej_row, 0, kRejRowBytes, c->stream));
  }
  if (!c->rej_host) MVR_HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&c->rej_host), kRejCopyBytes, hipHostMallocDefault));
  if (one_to_one) {
    const size_t had = c->rej_win_cap;
    if (int rc = ensure(c, c->rej_win, c->rej_win_cap, std::max<size_t>(nt, 1))) return rc;
    if (c->rej_win_cap != had || c->rej_win_dirty) {
      if (int rc = launch_fill_u64(c, c->rej_win, c->rej_win_cap, kKeyInit)) return rc;
      c->rej_win_dirty = false;
    }
  }
  return MVR_OK;
}

int launch_reject_chain(Ctx *c, const mvr_rejector *chain, int n_chain, const nnkey_t *keys, int32_t *match, size_t ns, size_t nt,
                        const float4 *snrm, const float4 *tnrm, const double *found, uint32_t found_host, const float4 *spts, const float4 *tpts,
                        bool fma, mvr_rej_sac_trace *sac_trace, size_t sac_trace_cap)
{
  uint32_t *words = reinterpret_cast<uint32_t *>(c->rej_row + kRejRowDoubles);
  uint32_t *hist = words + kRejCopyWords, *tie = hist + kRejHistBins;
  ProfScope ps(c, MVR_K_GLUE, 12.0 * (double)ns * (double)(n_chain + 1));
  hipLaunchKernelGGL(rej_init_kernel, dim3(1), dim3(kRejT), 0, c->stream, words, kRejCopyWords + kRejHistBins, found, found_host);
  const unsigned blocks = stride_blocks(ns);
  // TRIMMED's blocks take consecutive ranges of whole tiles
  const size_t tiles = (ns + kRejT - 1) / kRejT;
  const unsigned tie_blocks = (unsigned)std::min<size_t>(std::max<size_t>(tiles, 1), kRejTieBlocks);
  const size_t chunk = ((tiles + tie_blocks - 1) / tie_blocks) * kRejT;
  for (int s = 0; s < n_chain && ns; ++s) {
    const mvr_rejector &r = chain[s];
    uint32_t *stage = words + kRejHeadWords + s * kRejStageWords;
    const uint32_t *live_in = s ? stage - kRejStageWords + W_OUT : words;
    switch (r.kind) {
      case MVR_REJ_DISTANCE:
        hipLaunchKernelGGL(rej_apply_kernel<MVR_REJ_DISTANCE>, dim3(blocks), dim3(kRejT), 0, c->stream, keys, match, ns, r.value * r.value, snrm, tnrm, stage);
        break;
      case MVR_REJ_SURFACE_NORMAL:
        hipLaunchKernelGGL(rej_apply_kernel<MVR_REJ_SURFACE_NORMAL>, dim3(blocks), dim3(kRejT), 0, c->stream, keys, match, ns, r.value, snrm, tnrm, stage);
        break;
      case MVR_REJ_MEDIAN:
      case MVR_REJ_TRIMMED:
        for (int level = 0; level < 3; ++level) {
          hipLaunchKernelGGL(rej_hist_kernel, dim3(blocks), dim3(kRejT), 0, c->stream, keys, (const int32_t *)match, ns, level, (const uint32_t *)stage, hist);
          hipLaunchKernelGGL(rej_scan_kernel, dim3(1), dim3(kRejT), 0, c->stream, level, r.kind, r.value, r.min_correspondences, live_in, stage, hist);
        }
        if (r.kind == MVR_REJ_MEDIAN)
          hipLaunchKernelGGL(rej_apply_kernel<MVR_REJ_MEDIAN>, dim3(blocks), dim3(kRejT), 0, c->stream, keys, match, ns, r.value, snrm, tnrm, stage);
        else {
          hipLaunchKernelGGL(rej_tie_count_kernel, dim3(tie_blocks), dim3(kRejT), 0, c->stream, keys, (const int32_t *)match, ns, chunk, (const uint32_t *)stage, tie);
          hipLaunchKernelGGL(rej_trim_kernel, dim3(tie_blocks), dim3(kRejT), 0, c->stream, keys, match, ns, chunk, stage, (const uint32_t *)tie);
        }
        break;
      case MVR_REJ_ONE_TO_ONE:
        if (!c->rej_win || c->rej_win_cap < nt) return set_error(c, MVR_E_ARG, "the one-to-one table is not allocated");
        c->rej_win_dirty = true;
        hipLaunchKernelGGL(rej_oto_min_kernel, dim3(blocks), dim3(kRejT), 0, c->stream, keys, (const int32_t *)match, ns, c->rej_win);
        hipLaunchKernelGGL(rej_oto_keep_kernel, dim3(blocks), dim3(kRejT), 0, c->stream, keys, match, ns, (const nnkey_t *)c->rej_win, stage);
        hipLaunchKernelGGL(rej_oto_clear_kernel, dim3(blocks), dim3(kRejT), 0, c->stream, keys, ns, nt, c->rej_win);
        MVR_HIP_TRY(c, hipGetLastError());
        c->rej_win_dirty = false;
        break;
      case MVR_REJ_SAMPLE_CONSENSUS:
        if (int rc = reject_sac_stage(c, r, fma, spts, tpts, match, ns, stage, sac_trace, sac_trace_cap)) return rc;
        break;
      default:
        return set_error(c, MVR_E_ARG, "unknown rejector kind");
    }
  }
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

}  // namespace mvr
