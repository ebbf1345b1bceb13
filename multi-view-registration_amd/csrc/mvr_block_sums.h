// csrc/mvr_block_sums.h -- the fixed-order f64 sums shared by the reduction kernels (mvr_reduce.hip, mvr_gicp.hip): per-lane
// accumulators, a wave sum by DPP row shifts, one LDS hop across the 4 waves, a partial row per block in HBM and a one-block
// final sum over the rows in a fixed order -- bitwise reproducible run to run (no float atomics).  Device code: include it
// from a .hip file only, inside no namespace.
#pragma once
#include "mvr_internal.h"

namespace mvr {
namespace {

constexpr int kRT = 256;          // threads per reduction block
constexpr int kMaxBlocks = 1024;  // partial rows

// Sum of a double over the 64 lanes of a wave, the same value in every lane, without the LDS crossbar: an inclusive
// scan inside each row of 16 lanes by DPP row shifts (lanes shifted in from outside the row read as 0), then the four row
// totals -- lanes 15, 31, 47, 63 -- are read as scalars and added in order.  (`__shfl_down` of a double is two
// `ds_bpermute` per step: the 29 sums of the moments kernel cost 348 of them per wave and made that kernel LDS-bound,
// 59 us for the 12 pairs of a ring step.)  Fixed order, so the sums are reproducible run to run.
__device__ __forceinline__ double dpp_row_shr(double v, int ctrl)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  int lo = (int)(unsigned)b, hi = (int)(unsigned)(b >> 32);
  switch (ctrl) {      // the control word is an immediate
    case 1: lo = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xF, 0xF, true); break;
    case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xF, 0xF, true); break;
    case 4: lo = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xF, 0xF, true); break;
    default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xF, 0xF, true); hi = __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xF, 0xF, true); break;
  }
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
__device__ __forceinline__ double lane_value(double v, int lane)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}
__device__ __forceinline__ double wave_sum(double v)
{
  v += dpp_row_shr(v, 1);
  v += dpp_row_shr(v, 2);
  v += dpp_row_shr(v, 4);
  v += dpp_row_shr(v, 8);
  return ((lane_value(v, 15) + lane_value(v, 31)) + lane_value(v, 47)) + lane_value(v, 63);
}

// block-wide sums of K per-thread doubles -> row `blockIdx.x` of partials
template <int K>
__device__ __forceinline__ void block_partials_at(const double (&acc)[K], double *__restrict__ partials, unsigned row)
{
  __shared__ double lds[kRT / 64][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) lds[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double s = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRT / 64; ++w) s += lds[w][threadIdx.x];
    partials[(size_t)row * K + threadIdx.x] = s;
  }
}

template <int K>
__device__ __forceinline__ void block_partials(const double (&acc)[K], double *__restrict__ partials)
{
  __shared__ double lds[kRT / 64][K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) lds[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double s = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRT / 64; ++w) s += lds[w][threadIdx.x];
    partials[(size_t)blockIdx.x * K + threadIdx.x] = s;
  }
}

// fixed-order sum of `rows` partial rows of K doubles (one block, K <= 32).
// Thread (g, k) = (tid / 32, tid % 32) adds rows g, g+8, ... of column k, so a
// row is read as one contiguous run of K doubles; the 8 row groups are then
// added in a fixed order -> bitwise reproducible.
template <int K>
__device__ __forceinline__ void sum_rows(const double *__restrict__ partials, int rows, double (&out)[K],
                                         double * /*unused*/)
{
  static_assert(K <= 32, "sum_rows: K <= 32");
  constexpr int KP = (K <= 8) ? 8 : ((K <= 16) ? 16 : 32);   // columns padded to a power of two
  constexpr int G = kRT / KP;                                 // row groups
  __shared__ double grp[G][KP];
  __shared__ double tot[32];
  const int g = threadIdx.x / KP, k = threadIdx.x % KP;
  double s = 0.0;
  if (k < K) {
#pragma unroll 8
    for (int r = g; r < rows; r += G) s += partials[(size_t)r * K + k];
  }
  grp[g][k] = s;
  __syncthreads();
  if (threadIdx.x < K) {
    double t = grp[0][threadIdx.x];
#pragma unroll
    for (int gg = 1; gg < G; ++gg) t += grp[gg][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < K; ++kk) out[kk] = tot[kk];
}

inline int reduce_blocks(const Ctx *c, size_t n)
{
  const size_t want = (n + kRT - 1) / kRT;
  // few partial rows keep the single-block final sum short; 2 blocks per CU
  // already put > 8 MB of 16-byte loads in flight
  const size_t cap = std::min<size_t>(kMaxBlocks, (size_t)c->n_cu);
  return (int)std::max<size_t>(1, std::min(want, cap));
}

}  // namespace
}  // namespace mvr
