// csrc/mvr_pair_features.h -- pcl::computePairFeatures and the bin of a scaled feature, written once for the two descriptors
// built on them (mvr_fpfh.hip: rule F3 / F4 of mvr_cloud_fpfh; mvr_pfh.hip: rules P3 / P4 of mvr_cloud_pfh), so that both bin
// one pair identically at the same split count; and the kernel that lays a slot's normals out in its grid order with the
// validity mark both walks skip by.  Every translation unit that includes this is compiled with -ffp-contract=off: each f32
// operation is rounded as written.  Not installed.
#pragma once

#include <cmath>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {

__device__ __forceinline__ float dot3(const float ax, const float ay, const float az, const float bx, const float by, const float bz)
{
  return (ax * bx + ay * by) + az * bz;
}

// F4: the bin of a scaled coordinate x in [0, 1], BINS per feature, clamped to 0..BINS - 1 (a NaN goes to 0)
template <int BINS>
__device__ __forceinline__ int pair_bin(const double x) { return (int)fmin(fmax(floor((double)BINS * x), 0.0), (double)(BINS - 1)); }

// F3 for the pair (i, j): q / ni the point and normal in the role of "i", p / nj those of "j" (w of each is not looked at).
// false: the pair has no features (f4 == 0 or |v| == 0).
__device__ __forceinline__ bool pair_features(const float4 q, const float4 ni, const float4 p, const float4 nj, float *f1, float *f2, float *f3)
{
  float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
  const float f4 = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
  if (f4 == 0.f) return false;
  const float a1 = dot3(ni.x, ni.y, ni.z, dx, dy, dz) / f4, a2 = dot3(nj.x, nj.y, nj.z, dx, dy, dz) / f4;
  const bool swap = fabsf(a1) < fabsf(a2);
  const float n1x = swap ? nj.x : ni.x, n1y = swap ? nj.y : ni.y, n1z = swap ? nj.z : ni.z;
  const float n2x = swap ? ni.x : nj.x, n2y = swap ? ni.y : nj.y, n2z = swap ? ni.z : nj.z;
  *f3 = swap ? -a2 : a1;
  if (swap) { dx = -dx; dy = -dy; dz = -dz; }
  float vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
  const float vn = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
  if (vn == 0.f) return false;
  vx /= vn; vy /= vn; vz /= vn;
  const float wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  *f2 = dot3(vx, vy, vz, n2x, n2y, n2z);
  *f1 = atan2f(dot3(wx, wy, wz, n2x, n2y, n2z), dot3(n1x, n1y, n1z, n2x, n2y, n2z));
  return true;
}

// F4 on the three features: the bins b1, b2, b3 of f1, f2, f3, each in 0..BINS - 1
template <int BINS>
__device__ __forceinline__ void pair_bins(const float f1, const float f2, const float f3, int *b1, int *b2, int *b3)
{
  const float d_pi = (float)(1.0 / (2.0 * M_PI));
  *b1 = pair_bin<BINS>(((double)f1 + M_PI) * (double)d_pi);
  *b2 = pair_bin<BINS>(((double)f2 + 1.0) * 0.5);
  *b3 = pair_bin<BINS>(((double)f3 + 1.0) * 0.5);
}

// the slot's normals from index order to the order of S.qs (grid order, or index order without a grid); w = 1 marks a valid
// point (finite coordinates and a finite normal), w = 0 an invalid one, which every later walk skips (F1 / P1)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) valid_normals_kernel(const KnnSlot S, const float4 *__restrict__ src_nrm, float4 *__restrict__ gn)
{
  const uint32_t pos = blockIdx.x * THREADS + threadIdx.x;
  if (pos >= S.nq) return;
  const float4 p = S.qs[pos];
  const float4 n = src_nrm[S.q_by_pos ? pos : __float_as_uint(p.w)];
  const bool ok = finite3(p) && finite3(n);
  gn[pos] = make_float4(n.x, n.y, n.z, ok ? 1.f : 0.f);
}

}  // namespace mvr
