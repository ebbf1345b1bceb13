// csrc/mvr_plane.h -- the plane through a neighbourhood, shared by the kernels that fit one (mvr_knn.hip: normals; mvr_mls.hip:
// moving least squares; mvr_iss.hip: the eigenvalues of a scatter alone): f64 moments of the neighbours about the query point, the 3 x 3 symmetric eigenproblem by cyclic Jacobi,
// the pick of the smallest eigenvalue's eigenvector, the curvature and the f32 orientation of the normal.  Every index is a compile-time constant: the matrices stay in
// registers.  Not installed.
#pragma once

#include "mvr_internal.h"

namespace mvr {

// ---- the 3 x 3 symmetric eigenproblem in f64: cyclic Jacobi (A is destroyed, V = eigenvectors in columns)
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&V)[3][3])
{
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = fabs(theta) > 1.0e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double vp = V[r][P], vq = V[r][Q];
    V[r][P] = c * vp - s * vq;
    V[r][Q] = s * vp + c * vq;
  }
}

// f64 moments of the neighbours about the query point
struct Moments {
  double cnt = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
  __device__ __forceinline__ void add(const float4 p, const float4 q)
  {
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    cnt += 1.0; sx += dx; sy += dy; sz += dz;
    xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
  }
};

// the plane of at least one neighbour: mean (relative to the query point), unit normal = eigenvector of the smallest eigenvalue
// of the covariance (divided by the count), that eigenvalue and the sum of the three
struct PlaneFit {
  double m0, m1, m2, nx, ny, nz, lmin, sum;
};

__device__ __forceinline__ PlaneFit plane_fit(const Moments &M)
{
  PlaneFit f;
  const double inv = 1.0 / M.cnt, m0 = M.sx * inv, m1 = M.sy * inv, m2 = M.sz * inv;
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  A[0][0] = M.xx * inv - m0 * m0; A[0][1] = A[1][0] = M.xy * inv - m0 * m1; A[0][2] = A[2][0] = M.xz * inv - m0 * m2;
  A[1][1] = M.yy * inv - m1 * m1; A[1][2] = A[2][1] = M.yz * inv - m1 * m2; A[2][2] = M.zz * inv - m2 * m2;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (!(off > 1.0e-40 * dia)) break;                      // (an all-zero matrix ends here too)
    jacobi_rot<0, 1, 2>(A, V);
    jacobi_rot<0, 2, 1>(A, V);
    jacobi_rot<1, 2, 0>(A, V);
  }
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  // the column of the smallest eigenvalue, picked by 0 / 1 weights (a select between array elements becomes a select between
  // their ADDRESSES, which sends A and V to scratch memory)
  const double w0 = (l0 <= l1 && l0 <= l2) ? 1.0 : 0.0, w1 = (w0 == 0.0 && l1 <= l2) ? 1.0 : 0.0, w2 = 1.0 - w0 - w1;
  f.lmin = w0 * l0 + w1 * l1 + w2 * l2;
  const double nx = w0 * V[0][0] + w1 * V[0][1] + w2 * V[0][2], ny = w0 * V[1][0] + w1 * V[1][1] + w2 * V[1][2],
               nz = w0 * V[2][0] + w1 * V[2][1] + w2 * V[2][2];
  const double nn = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
  f.nx = nx * nn; f.ny = ny * nn; f.nz = nz * nn;
  f.sum = l0 + l1 + l2;
  f.m0 = m0; f.m1 = m1; f.m2 = m2;
  return f;
}

// ---- eigenvalues only (mvr_iss.hip): the rotation of jacobi_rot on the matrix alone, the same arithmetic
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rot_values(double (&A)[3][3])
{
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = fabs(theta) > 1.0e150 ? 0.5 / theta : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
}

// the eigenvalues e1 >= e2 >= e3 of the scatter matrix of the moments -- the second sums as they are, about the query point,
// NOT divided by the count and not centred on the mean (pcl::ISSKeypoint3D::getScatterMatrix).  The order is taken with
// fmin / fmax between values (no array element is selected by a runtime index).  fmin / fmax drop a NaN, so a non-finite
// diagonal makes all three NaN: the caller's test that they are finite sees it.
struct Eigenvalues3 {
  double e1, e2, e3;
};

__device__ __forceinline__ Eigenvalues3 scatter_eigenvalues(const Moments &M)
{
  double A[3][3];
  A[0][0] = M.xx; A[0][1] = A[1][0] = M.xy; A[0][2] = A[2][0] = M.xz;
  A[1][1] = M.yy; A[1][2] = A[2][1] = M.yz; A[2][2] = M.zz;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (!(off > 1.0e-40 * dia)) break;                      // (an all-zero matrix ends here too)
    jacobi_rot_values<0, 1, 2>(A);
    jacobi_rot_values<0, 2, 1>(A);
    jacobi_rot_values<1, 2, 0>(A);
  }
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  const double hi = fmax(l0, l1), lo = fmin(l0, l1);
  Eigenvalues3 e;
  if (!(isfinite(l0) && isfinite(l1) && isfinite(l2))) { e.e1 = e.e2 = e.e3 = __builtin_nan(""); return e; }
  e.e1 = fmax(hi, l2);
  e.e2 = fmax(lo, fmin(hi, l2));
  e.e3 = fmin(lo, l2);
  return e;
}

// PCL's curvature of a fitted plane: the smallest eigenvalue's share of the three
__device__ __forceinline__ float plane_curvature(const PlaneFit &f) { return f.sum != 0.0 ? (float)(fabs(f.lmin) / f.sum) : 0.f; }

// flipNormalTowardsViewpoint: the normal, already rounded to f32, turned to the side of the direction r (towards the viewpoint,
// or along a reference normal) with PCL's f32 test, cos < 0 strictly
__device__ __forceinline__ float4 plane_normal_towards(float fx, float fy, float fz, const float rx, const float ry, const float rz)
{
  float cs = rx * fx;
  cs = cs + ry * fy;
  cs = cs + rz * fz;
  if (cs < 0.f) { fx = -fx; fy = -fy; fz = -fz; }
  return make_float4(fx, fy, fz, 0.f);
}

}  // namespace mvr
