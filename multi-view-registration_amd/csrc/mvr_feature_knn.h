// csrc/mvr_feature_knn.h -- the all-pairs distance kernel of mvr_feature_knn (rules M1-M3 in mvr_hip.h), a template of the row
// length, and its launch by list size.  csrc/mvr_feature.hip, where the kernel is described and its partial lists are merged,
// instantiates the 33-float rows of FPFH; csrc/mvr_pfh.hip the 125-float rows of PFH.  The 352-float rows of SHOT have a kernel of
// their own in csrc/mvr_shot.hip (this one keeps the query row in registers, which does not scale to them).  Not installed.
#pragma once

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {

constexpr int kFpfhDim = 3 * MVR_FPFH_BINS, kPfhDim = MVR_PFH_DIM, kShotDim = MVR_SHOT_DIM;      // the row lengths served: 33, 125 and 352
constexpr int feat_pad(int dim) { return (dim + 3) / 4 * 4; }            // floats per staged row: 16-byte aligned (36, 128)
constexpr int kFeatTile = 64;                    // target rows per LDS tile (9 KiB at 33 floats, 32 KiB at 125)
constexpr int kFeatThreads = 256;
inline bool feat_dim_ok(int dim) { return dim == kFpfhDim || dim == kPfhDim || dim == kShotDim; }

// part: [split][nq][k] keys, each list ascending
template <int KMAX, int DIM>
__global__ void __launch_bounds__(kFeatThreads) feature_knn_kernel(const float *__restrict__ q, const uint32_t nq, const float *__restrict__ t,
                                                                   const uint32_t nt, const uint32_t rows_per_split, const int k,
                                                                   nnkey_t *__restrict__ part)
{
  constexpr int kFeatDim = DIM, kFeatPad = feat_pad(DIM);
  __shared__ __attribute__((aligned(16))) float tile[kFeatTile * kFeatPad];
  const uint32_t tid = threadIdx.x, qi = blockIdx.x * kFeatThreads + tid;
  const bool live = qi < nq;
  float f[kFeatDim];
#pragma unroll
  for (int b = 0; b < kFeatDim; ++b) f[b] = live ? q[(size_t)qi * kFeatDim + b] : 0.f;
  nnkey_t L[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) L[i] = i < KMAX - k ? 0ull : kKnnKeyEmpty;
  const uint32_t t0 = min((uint32_t)blockIdx.y * rows_per_split, nt), t1 = min(t0 + rows_per_split, nt);
  for (uint32_t base = t0; base < t1; base += kFeatTile) {
    const uint32_t rows = min((uint32_t)kFeatTile, t1 - base);
    const float *src = t + (size_t)base * kFeatDim;
    for (uint32_t e = tid; e < rows * kFeatDim; e += kFeatThreads) tile[(e / kFeatDim) * kFeatPad + e % kFeatDim] = src[e];
    __syncthreads();
    if (live) {
      for (uint32_t r = 0; r < rows; ++r) {
        const float4 *row4 = reinterpret_cast<const float4 *>(tile + r * kFeatPad);
        float acc = 0.f;      // M1
#pragma unroll
        for (int g = 0; g < kFeatDim / 4; ++g) {
          const float4 v = row4[g];
          float d;
          d = f[4 * g] - v.x;     acc = acc + d * d;
          d = f[4 * g + 1] - v.y; acc = acc + d * d;
          d = f[4 * g + 2] - v.z; acc = acc + d * d;
          d = f[4 * g + 3] - v.w; acc = acc + d * d;
        }
#pragma unroll
        for (int b = kFeatDim / 4 * 4; b < kFeatDim; ++b) {
          const float d = f[b] - tile[r * kFeatPad + b];
          acc = acc + d * d;
        }
        const nnkey_t key = ((nnkey_t)__float_as_uint(acc) << 32) | (nnkey_t)(base + r);
        if (key < L[KMAX - 1]) knn_insert<KMAX>(L, key);
      }
    }
    __syncthreads();
  }
  if (!live) return;
  nnkey_t *out = part + ((size_t)blockIdx.y * nq + qi) * (size_t)k;
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
    if (i >= KMAX - k) out[i - (KMAX - k)] = L[i];
}

// grid: (blocks of queries, splits of the target)
template <int DIM>
void launch_feature_knn(hipStream_t st, dim3 grid, const float *q, uint32_t nq, const float *t, uint32_t nt, uint32_t rows_per_split, int k,
                        nnkey_t *part)
{
  const dim3 block(kFeatThreads);
  switch (kmax_bucket(k)) {
    case 8:  hipLaunchKernelGGL((feature_knn_kernel<8, DIM>), grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    case 16: hipLaunchKernelGGL((feature_knn_kernel<16, DIM>), grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    case 32: hipLaunchKernelGGL((feature_knn_kernel<32, DIM>), grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    default: hipLaunchKernelGGL((feature_knn_kernel<64, DIM>), grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
  }
}
// launch_feature_knn<kPfhDim>, compiled in mvr_pfh.hip
void launch_feature_knn_pfh(hipStream_t st, dim3 grid, const float *q, uint32_t nq, const float *t, uint32_t nt, uint32_t rows_per_split, int k,
                            nnkey_t *part);
// the kernel for rows of kShotDim floats, in mvr_shot.hip: the same grid, the same partial lists
void launch_feature_knn_shot(hipStream_t st, dim3 grid, const float *q, uint32_t nq, const float *t, uint32_t nt, uint32_t rows_per_split, int k,
                             nnkey_t *part);

}  // namespace mvr
