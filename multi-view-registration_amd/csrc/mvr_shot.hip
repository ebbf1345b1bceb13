// csrc/mvr_shot.hip -- pcl::SHOTEstimation (SHOT352) with its own local reference frames (pcl::SHOTLocalReferenceFrameEstimation)
// on the GPU (gfx950), over the cloud itself or at chosen queries over a search surface; the rules L1-L7 and H1-H9 are written
// next to mvr_cloud_shot in mvr_hip.h.  At the end the matcher's kernel for rows of 352 floats.
//
// SHOT is linear in the neighbourhood and needs no neighbour list: ONE WAVE PER QUERY (a block is one wave), the queries in the
// order of the surface's grid (or of the sorted query array of mvr_at.hip), and the cooperative ball walk of mvr_pfh.hip restated
// with every lane CONSUMING the neighbour it loaded instead of staging it (PFH's walk hands out staging slots; this one hands
// every lane its own point and an "inside" flag, so that the callers can ballot).  Three passes:
//   1. shot_lrf_kernel, first walk: the seven f64 sums of L3 per lane in walk order, then the fixed tree of wave_sum
//      (mvr_block_sums.h); every lane then solves the 3 x 3 eigenproblem with the cyclic Jacobi of mvr_plane.h;
//   2. the same kernel, second walk: the sign counts of L5 by ballot and the tie sums by the same tree; lane 0 writes the frame;
//   3. shot_desc_kernel: the frame is read back as the nine f32 (L6), each lane computes the amounts of its neighbour (H3-H6) in
//      f64 with the device libm (sqrt, acos, atan2) and adds them as 2^-32 fixed point with 64-bit integer LDS atomics into a
//      352-entry histogram (2.75 KiB per wave); the norm of H8 is one ascending f64 sum that every lane repeats.
// Passes 1 and 2 are skipped when the caller passes frames.  They are not shared with pass 3 when lrf_radius == radius: the
// surface points differ (L1 needs no normal, H1 does).  The sums are integers: S depends on no order (H7).
// Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvr_block_sums.h"
#include "mvr_feature_knn.h"
#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_pair_features.h"
#include "mvr_plane.h"

namespace mvr {
namespace {

constexpr int kLanes = 64;                       // a block is one wave
constexpr int kDim = MVR_SHOT_DIM, kShape = 11, kVolumes = 32;
constexpr uint32_t kMinNeighbors = 5u;           // L2, H2
static_assert(kShape * kVolumes == kDim, "32 volumes of 11 shape slots");
// pcl/features/shot.h: PST_RAD_45, PST_RAD_90, PST_RAD_135, PST_RAD_PI_7_8
constexpr double kRad45 = 0.78539816339744830961566084581988, kRad90 = 1.5707963267948966192313216916398,
                 kRad135 = 2.3561944901923449288469825374596, kRad7_8 = 2.7488935718910690836548129603691;

struct ShotArgs {
  KnnSlot S;                       // the surface as target; its own points as queries, or (at) the query array
  const float4 *gn;                // the surface's normals in the order of S.gt, w = 1 for a valid point (H1); null: frames alone
  int at;                          // the queries are a query array: valid iff finite (Q2)
  int q_by_gn;                     // self mode of the descriptor call: the query is valid iff gn says so (H1)
  float r2_lrf, r2;
  double R_lrf, R, R12, R14, R34;  // radius; (R / 2), (R / 4), (R * 3) / 4 as PCL computes them
  float *lrf;                      // [rows][9] by row
  uint32_t *lrf_count;             // n of L2 by row
  unsigned long long *sums;        // [rows][352] by row, or null
  float *out;                      // [rows][352] by row, or null
  uint32_t *ncount;                // n_i of H2 by row
};

// the cooperative ball walk of one wave around q: f(in, p, nj) is called by EVERY lane of the wave for every 64 grid positions
// of every cell row of the ball (uniform control flow: f may ballot); `in` says that the lane holds a target point p with
// d2 <= r2 (NORMALS: and a valid normal nj).  Returns the number of such points.
template <bool FMA, bool NORMALS, class F>
__device__ __forceinline__ uint32_t shot_walk(const KnnSlot &S, const float4 *__restrict__ gn, const float4 q, const float r2, F &&f)
{
  if (S.nt == 0 || !finite3(q)) return 0u;
  const uint32_t lane = threadIdx.x;
  int x0, x1, y0, y1, z0, z1;
  knn_ball_cells(S, q, r2, &x0, &x1, &y0, &y1, &z0, &z1);
  uint32_t n = 0;
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      uint32_t s, e;
      knn_row_range(S, x0, x1, y, z, &s, &e);
      for (uint32_t base = s; base < e; base += kLanes) {
        const uint32_t j = base + lane;
        bool in = false;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), nj = p;
        if (j < e) {
          p = S.gt[j];
          if (knn_dist2<FMA>(p, q) <= r2) {
            if (NORMALS) { nj = gn[j]; in = nj.w != 0.f; }
            else in = true;
          }
        }
        n += (uint32_t)__popcll(__ballot(in));
        f(in, p, nj);
      }
    }
  return n;
}

__device__ __forceinline__ double dot3d(const double ax, const double ay, const double az, const double bx, const double by, const double bz)
{
  return (ax * bx + ay * by) + az * bz;
}

// L4: the unit eigenvectors of the smallest (z) and of the largest (x) eigenvalue of the symmetric C, two DIFFERENT columns of
// the Jacobi basis whatever the eigenvalues (an isotropic neighbourhood still gets an orthonormal frame)
__device__ __forceinline__ void shot_axes(const double (&M)[7], double (&ax)[3], double (&az)[3])
{
  const double W = M[6];
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  A[0][0] = M[0] / W; A[0][1] = A[1][0] = M[1] / W; A[0][2] = A[2][0] = M[2] / W;
  A[1][1] = M[3] / W; A[1][2] = A[2][1] = M[4] / W; A[2][2] = M[5] / W;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
    if (!(off > 1.0e-40 * dia)) break;
    jacobi_rot<0, 1, 2>(A, V);
    jacobi_rot<0, 2, 1>(A, V);
    jacobi_rot<1, 2, 0>(A, V);
  }
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  // columns picked by 0 / 1 weights (mvr_plane.h: a select between array elements would send A and V to scratch)
  const bool s0 = l0 <= l1 && l0 <= l2, s1 = !s0 && l1 <= l2, s2 = !s0 && !s1;
  const bool b0 = (s1 && l0 >= l2) || (s2 && l0 >= l1), b1 = (s0 && l1 >= l2) || (s2 && !(l0 >= l1)), b2 = !b0 && !b1;
  const double w0 = s0 ? 1.0 : 0.0, w1 = s1 ? 1.0 : 0.0, w2 = s2 ? 1.0 : 0.0;
  const double u0 = b0 ? 1.0 : 0.0, u1 = b1 ? 1.0 : 0.0, u2 = b2 ? 1.0 : 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    az[r] = w0 * V[r][0] + w1 * V[r][1] + w2 * V[r][2];
    ax[r] = u0 * V[r][0] + u1 * V[r][1] + u2 * V[r][2];
  }
  const double nz = 1.0 / sqrt(dot3d(az[0], az[1], az[2], az[0], az[1], az[2])), nx = 1.0 / sqrt(dot3d(ax[0], ax[1], ax[2], ax[0], ax[1], ax[2]));
#pragma unroll
  for (int r = 0; r < 3; ++r) { az[r] *= nz; ax[r] *= nx; }
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) shot_lrf_kernel(ShotArgs a)
{
  const KnnSlot &S = a.S;
  const uint32_t pos = blockIdx.x;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  const bool valid = a.q_by_gn ? a.gn[pos].w != 0.f : finite3(q);      // L1 / H1 (an invalid query walks nothing)
  const double R = a.R_lrf;
  const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
  float F[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = __builtin_nanf("");
  uint32_t n = 0;
  if (valid) {
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // L3: xx xy xz yy yz zz, W
    shot_walk<FMA, false>(S, nullptr, q, a.r2_lrf, [&](const bool in0, const float4 p, const float4) {
      const bool in = in0 && !(p.x == q.x && p.y == q.y && p.z == q.z);      // L2: a point AT the query is skipped, as in PCL
      n += (uint32_t)__popcll(__ballot(in));
      if (!in) return;
      const double vx = (double)p.x - qx, vy = (double)p.y - qy, vz = (double)p.z - qz;
      const double w = R - sqrt(dot3d(vx, vy, vz, vx, vy, vz));
      const double wx = w * vx, wy = w * vy, wz = w * vz;
      acc[0] += wx * vx; acc[1] += wx * vy; acc[2] += wx * vz; acc[3] += wy * vy; acc[4] += wy * vz; acc[5] += wz * vz; acc[6] += w;
    });
    double M[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) M[e] = wave_sum(acc[e]);      // L7: the same value in every lane
    bool ok = n >= kMinNeighbors && M[6] != 0.0;
#pragma unroll
    for (int e = 0; e < 7; ++e) ok = ok && isfinite(M[e]);
    if (ok) {                                                  // (uniform: n and M are)
      double ax[3], az[3];
      shot_axes(M, ax, az);
      uint32_t plus_x = 0u, plus_z = 0u;                       // L5
      double sx = 0.0, sz = 0.0;
      shot_walk<FMA, false>(S, nullptr, q, a.r2_lrf, [&](const bool in0, const float4 p, const float4) {
        const bool in = in0 && !(p.x == q.x && p.y == q.y && p.z == q.z);
        const double vx = (double)p.x - qx, vy = (double)p.y - qy, vz = (double)p.z - qz;
        const double dx = dot3d(vx, vy, vz, ax[0], ax[1], ax[2]), dz = dot3d(vx, vy, vz, az[0], az[1], az[2]);
        plus_x += (uint32_t)__popcll(__ballot(in && dx >= 0.0));
        plus_z += (uint32_t)__popcll(__ballot(in && dz >= 0.0));
        if (in) {
          const double w = R - sqrt(dot3d(vx, vy, vz, vx, vy, vz));
          sx += w * dx; sz += w * dz;
        }
      });
      sx = wave_sum(sx); sz = wave_sum(sz);
      const bool neg_x = 2u * plus_x < n || (2u * plus_x == n && sx < 0.0), neg_z = 2u * plus_z < n || (2u * plus_z == n && sz < 0.0);
      if (neg_x) { ax[0] = -ax[0]; ax[1] = -ax[1]; ax[2] = -ax[2]; }
      if (neg_z) { az[0] = -az[0]; az[1] = -az[1]; az[2] = -az[2]; }
      const double yx = az[1] * ax[2] - az[2] * ax[1], yy = az[2] * ax[0] - az[0] * ax[2], yz = az[0] * ax[1] - az[1] * ax[0];      // L6: y = z x x
      F[0] = (float)ax[0]; F[1] = (float)ax[1]; F[2] = (float)ax[2];
      F[3] = (float)yx; F[4] = (float)yy; F[5] = (float)yz;
      F[6] = (float)az[0]; F[7] = (float)az[1]; F[8] = (float)az[2];
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 9; ++e) fin = fin && isfinite(F[e]);
      if (!fin) {
#pragma unroll
        for (int e = 0; e < 9; ++e) F[e] = __builtin_nanf("");
      }
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.lrf[(size_t)qi * 9 + e] = F[e];
    a.lrf_count[qi] = n;
  }
}

// H7: an amount as 2^-32 fixed point (a negative rounding, and a NaN, give 0)
__device__ __forceinline__ unsigned long long shot_fix(const double w)
{
  return w > 0.0 ? (unsigned long long)floor(w * 4294967296.0 + 0.5) : 0ull;
}
__device__ __forceinline__ void shot_put(unsigned long long *hist, const int vol, const int k, const double w)
{
  const uint32_t slot = (uint32_t)(kShape * vol + k);
  if (slot < (uint32_t)kDim) atomicAdd(&hist[slot], shot_fix(w));      // (every slot the rules name is inside; the test costs nothing)
}

// H3-H6 for one neighbour: v = p - q in f64, nj its normal, X / Y / Z the frame
__device__ __forceinline__ void shot_add(const ShotArgs &a, const double vx, const double vy, const double vz, const float4 nj, const double (&fr)[9],
                                         unsigned long long *hist)
{
  const double d = sqrt(dot3d(vx, vy, vz, vx, vy, vz));
  if (d == 0.0) return;                                                 // H2
  double c = dot3d((double)nj.x, (double)nj.y, (double)nj.z, fr[6], fr[7], fr[8]);      // H4
  if (!isfinite(c)) return;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  double x = dot3d(vx, vy, vz, fr[0], fr[1], fr[2]), y = dot3d(vx, vy, vz, fr[3], fr[4], fr[5]), z = dot3d(vx, vy, vz, fr[6], fr[7], fr[8]);      // H3
  if (fabs(x) < 1.0e-30) x = 0.0;
  if (fabs(y) < 1.0e-30) y = 0.0;
  if (fabs(z) < 1.0e-30) z = 0.0;
  // H5: the sector by PCL's sign tests (no libm call decides a volume)
  const int bit4 = (y > 0.0 || (y == 0.0 && x < 0.0)) ? 1 : 0;
  const int bit3 = (x > 0.0 || (x == 0.0 && y > 0.0)) ? 1 - bit4 : bit4;
  int vol = ((bit4 << 3) + (bit3 << 2)) << 1;
  if (x * y > 0.0 || x == 0.0) vol += fabs(x) >= fabs(y) ? 0 : 4;
  else vol += fabs(x) > fabs(y) ? 4 : 0;
  const int sector = vol >> 2;
  const bool outer = d > a.R12;
  vol += (z > 0.0 ? 1 : 0) + (outer ? 2 : 0);
  const double bin = ((1.0 + c) * 10.0) / 2.0;
  const int step = (int)floor(bin + 0.5);
  const double t = bin - (double)step;
  double home = 1.0 - fabs(t);                                          // H6 (a)
  if (t > 0.0) shot_put(hist, vol, (step + 1) % 10, t);
  else if (t < 0.0) shot_put(hist, vol, (step + 9) % 10, -t);
  if (outer) {                                                          // (b)
    const double u = (d - a.R34) / a.R12;
    if (d > a.R34) home += 1.0 - u;
    else { home += 1.0 + u; shot_put(hist, vol - 2, step, -u); }
  } else {
    const double u = (d - a.R14) / a.R12;
    if (d < a.R14) home += 1.0 + u;
    else { home += 1.0 - u; shot_put(hist, vol + 2, step, u); }
  }
  double ic = z / d;                                                    // (c)
  ic = ic < -1.0 ? -1.0 : (ic > 1.0 ? 1.0 : ic);
  const double inc = acos(ic);
  if (inc > kRad90 || (fabs(inc - kRad90) < 1.0e-30 && z <= 0.0)) {
    const double u = (inc - kRad135) / kRad90;
    if (inc > kRad135) home += 1.0 - u;
    else { home += 1.0 + u; shot_put(hist, vol + 1, step, -u); }
  } else {
    const double u = (inc - kRad45) / kRad90;
    if (inc < kRad45) home += 1.0 + u;
    else { home += 1.0 - u; shot_put(hist, vol - 1, step, u); }
  }
  if (y != 0.0 || x != 0.0) {                                           // (d)
    const double az = atan2(y, x);
    double u = (az - (-kRad7_8 + kRad45 * (double)sector)) / kRad45;
    u = fmax(-0.5, fmin(u, 0.5));
    if (u > 0.0) { home += 1.0 - u; shot_put(hist, (vol + 4) % kVolumes, step, u); }
    else { home += 1.0 + u; shot_put(hist, (vol + 28) % kVolumes, step, -u); }
  }
  shot_put(hist, vol, step, home);                                      // (e)
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) shot_desc_kernel(ShotArgs a)
{
  __shared__ unsigned long long hist[kDim];
  const KnnSlot &S = a.S;
  const uint32_t pos = blockIdx.x, lane = threadIdx.x;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  bool ok = a.at ? finite3(q) : a.gn[pos].w != 0.f;                     // H1
  double fr[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) { fr[e] = (double)a.lrf[(size_t)qi * 9 + e]; ok = ok && isfinite(fr[e]); }      // L6: the f32 frame
  for (uint32_t h = lane; h < (uint32_t)kDim; h += kLanes) hist[h] = 0ull;
  __syncthreads();
  uint32_t n = 0;
  if (ok) {                                                             // (uniform)
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    n = shot_walk<FMA, true>(S, a.gn, q, a.r2, [&](const bool in, const float4 p, const float4 nj) {
      if (in) shot_add(a, (double)p.x - qx, (double)p.y - qy, (double)p.z - qz, nj, fr, hist);
    });
  }
  __syncthreads();
  const bool row = ok && n >= kMinNeighbors;                            // H2
  double norm2 = 0.0;                                                   // H8: ascending b, every lane the same sum
  if (row)                                                              // (also with no output asked for: a timing with NULL outputs includes it)
    for (int b = 0; b < kDim; ++b) { const double s = (double)hist[b]; norm2 += s * s; }
  const double norm = sqrt(norm2);
  for (uint32_t h = lane; h < (uint32_t)kDim; h += kLanes) {
    const unsigned long long s = row ? hist[h] : 0ull;
    if (a.sums) a.sums[(size_t)qi * kDim + h] = s;
    if (a.out) a.out[(size_t)qi * kDim + h] = row && norm != 0.0 ? (float)((double)s / norm) : __builtin_nanf("");
  }
  if (lane == 0) a.ncount[qi] = ok ? n : 0u;
}

// qc null: every point of the cloud cl against cl itself.  Else the queries of rules Q1 / Q2 -- the points `indices` of qc (null:
// all of them) -- over the surface cl.  desc false: the frames alone (ncount = n of L2).  The refusals are the caller's.
int shot_cloud(Ctx *c, Cloud &cl, const mvr_shot_params &p, const bool desc, const float *lrf_in, float *shot, float *lrf_out,
               unsigned long long *sums, uint32_t *neighbor_count, const Cloud *qc = nullptr, const uint32_t *indices = nullptr, size_t n_indices = 0)
{
  const size_t ns = cl.n, n = !qc ? ns : indices ? n_indices : qc->n;      // surface points; queries = output rows
  if (n == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "shot reads back");
  const bool fma = p.fma_dist != 0;
  const double R = p.radius, Rl = p.lrf_radius != 0.0 ? p.lrf_radius : p.radius;
  ShotArgs a{};
  a.at = qc ? 1 : 0;
  a.q_by_gn = desc && !qc ? 1 : 0;
  a.R = R; a.R12 = R / 2.0; a.R14 = R / 4.0; a.R34 = (R * 3.0) / 4.0; a.R_lrf = Rl;
  a.r2 = clamp_r2(R); a.r2_lrf = clamp_r2(Rl);
  AtQueries Q;
  if (int rc = fill_target(c, cl, a.S)) return rc;        // (before the arena is carved: the grid build uses the context's buffers)
  fill_queries(cl, a.S);
  const KnnSlot self = a.S;                                // the surface walking itself: the order of gn
  if (qc) {
    if (int rc = at_queries(c, *qc, desc && qc == &cl, indices, n_indices, a.S, &Q)) return rc;
    a.S.qs = Q.q; a.S.q_by_pos = 0u; a.S.nq = (uint32_t)n;
  }
  const size_t rows = n * (size_t)kDim;
  Carver plan;
  plan.plan<float4>(ns); plan.plan<float>(n * 9); plan.plan<uint32_t>(n); plan.plan<uint32_t>(n);
  plan.plan<float>(shot ? rows : 1); plan.plan<unsigned long long>(sums ? rows : 1);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  float4 *gn = s.take<float4>(ns);
  a.lrf = s.take<float>(n * 9);
  a.lrf_count = s.take<uint32_t>(n);
  a.ncount = s.take<uint32_t>(n);
  a.out = s.take<float>(shot ? rows : 1);
  a.sums = s.take<unsigned long long>(sums ? rows : 1);
  if (!shot) a.out = nullptr;
  if (!sums) a.sums = nullptr;
  a.gn = desc ? gn : nullptr;
  const dim3 grid((unsigned)n), block(kLanes);
  if (desc && ns > 0) {
    hipLaunchKernelGGL(valid_normals_kernel<kKnnThreads>, dim3(blocks_for(ns, kKnnThreads)), dim3(kKnnThreads), 0, c->stream, self, cl.nrm, gn);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  if (lrf_in) {
    MVR_HIP_TRY(c, hipMemcpyAsync(a.lrf, lrf_in, n * 9 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  } else {
    if (fma) hipLaunchKernelGGL(shot_lrf_kernel<true>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(shot_lrf_kernel<false>, grid, block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  if (desc) {
    if (fma) hipLaunchKernelGGL(shot_desc_kernel<true>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(shot_desc_kernel<false>, grid, block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  if (shot) MVR_HIP_TRY(c, hipMemcpyAsync(shot, a.out, rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (sums) MVR_HIP_TRY(c, hipMemcpyAsync(sums, a.sums, rows * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (lrf_out) MVR_HIP_TRY(c, hipMemcpyAsync(lrf_out, a.lrf, n * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (neighbor_count)
    MVR_HIP_TRY(c, hipMemcpyAsync(neighbor_count, desc ? a.ncount : a.lrf_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  return MVR_OK;
}

bool shot_params_ok(const mvr_shot_params *p)
{
  return p && std::isfinite(p->radius) && p->radius > 0.0 && std::isfinite(p->lrf_radius) && p->lrf_radius >= 0.0;
}

// ------------------------------------------------------------------ the matcher at 352 floats
// feature_knn_kernel (mvr_feature_knn.h) keeps the query row in registers and a 64-row tile in LDS: at 352 floats that is 352
// registers and 88 KiB.  This kernel turns it round: the thread keeps the PARTIAL SUMS of one tile of 16 target rows (22 KiB of
// LDS) and walks the dimension in chunks of 8 floats -- two 16-byte loads of its query row, which stays in the caches (its 1.4 KiB
// are re-read once per tile, 48 VALU operations per loaded float), and two 16-byte LDS reads per target row at an address the
// whole wave shares.  Each pair's sum still adds its 352 terms in ascending b, in f32, uncontracted (M1); the keys, the k-best
// list, the split over blockIdx.y and the merge are those of mvr_feature.hip.
constexpr int kWideTile = 16, kWideRow4 = kShotDim / 4;
static_assert(kShotDim % 8 == 0 && kFeatTile % kWideTile == 0, "chunks of 8 floats; a split is whole tiles");

template <int KMAX>
__global__ void __launch_bounds__(kFeatThreads) feature_knn_wide_kernel(const float *__restrict__ q, const uint32_t nq, const float *__restrict__ t,
                                                                        const uint32_t nt, const uint32_t rows_per_split, const int k,
                                                                        nnkey_t *__restrict__ part)
{
  __shared__ float4 tile[kWideTile * kWideRow4];
  const uint32_t tid = threadIdx.x, qi = blockIdx.x * kFeatThreads + tid;
  const bool live = qi < nq;
  const float4 *qrow = reinterpret_cast<const float4 *>(q + (size_t)(live ? qi : 0u) * kShotDim);      // (nq > 0: row 0 exists)
  nnkey_t L[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) L[i] = i < KMAX - k ? 0ull : kKnnKeyEmpty;
  const uint32_t t0 = min((uint32_t)blockIdx.y * rows_per_split, nt), t1 = min(t0 + rows_per_split, nt);
  for (uint32_t base = t0; base < t1; base += kWideTile) {
    const uint32_t rows = min((uint32_t)kWideTile, t1 - base);
    const float4 *src = reinterpret_cast<const float4 *>(t + (size_t)base * kShotDim);
    for (uint32_t e = tid; e < rows * kWideRow4; e += kFeatThreads) tile[e] = src[e];
    __syncthreads();
    float acc[kWideTile];      // M1 (rows past `rows` hold an earlier tile: computed, never looked at)
#pragma unroll
    for (int r = 0; r < kWideTile; ++r) acc[r] = 0.f;
    for (int g = 0; g < kWideRow4; g += 2) {
      const float4 fa = qrow[g], fb = qrow[g + 1];
#pragma unroll
      for (int r = 0; r < kWideTile; ++r) {
        const float4 va = tile[r * kWideRow4 + g], vb = tile[r * kWideRow4 + g + 1];
        float d;
        d = fa.x - va.x; acc[r] = acc[r] + d * d;
        d = fa.y - va.y; acc[r] = acc[r] + d * d;
        d = fa.z - va.z; acc[r] = acc[r] + d * d;
        d = fa.w - va.w; acc[r] = acc[r] + d * d;
        d = fb.x - vb.x; acc[r] = acc[r] + d * d;
        d = fb.y - vb.y; acc[r] = acc[r] + d * d;
        d = fb.z - vb.z; acc[r] = acc[r] + d * d;
        d = fb.w - vb.w; acc[r] = acc[r] + d * d;
      }
    }
    if (live) {
#pragma unroll
      for (int r = 0; r < kWideTile; ++r) {
        const nnkey_t key = ((nnkey_t)__float_as_uint(acc[r]) << 32) | (nnkey_t)(base + (uint32_t)r);
        if ((uint32_t)r < rows && key < L[KMAX - 1]) knn_insert<KMAX>(L, key);
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

}  // namespace

// the matcher's kernels for rows of 352 floats (launched from mvr_feature.hip); grid: (blocks of queries, splits of the target)
void launch_feature_knn_shot(hipStream_t st, dim3 grid, const float *q, uint32_t nq, const float *t, uint32_t nt, uint32_t rows_per_split, int k,
                             nnkey_t *part)
{
  const dim3 block(kFeatThreads);
  switch (kmax_bucket(k)) {
    case 8:  hipLaunchKernelGGL(feature_knn_wide_kernel<8>, grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    case 16: hipLaunchKernelGGL(feature_knn_wide_kernel<16>, grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    case 32: hipLaunchKernelGGL(feature_knn_wide_kernel<32>, grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
    default: hipLaunchKernelGGL(feature_knn_wide_kernel<64>, grid, block, 0, st, q, nq, t, nt, rows_per_split, k, part); break;
  }
}

}  // namespace mvr

using namespace mvr;

API int mvr_cloud_shot_lrf(mvr_ctx *ctx, int slot, const mvr_shot_params *p, float *lrf, uint32_t *neighbor_count)
{
  if (!ctx || !slot_ok(slot) || !shot_params_ok(p)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &cl = c->slots[slot];
  if (int rc = knn_cloud_ok(c, cl, "shot_lrf")) return rc;
  return shot_cloud(c, cl, *p, false, nullptr, nullptr, lrf, nullptr, neighbor_count);
}

API int mvr_cloud_shot(mvr_ctx *ctx, int slot, const mvr_shot_params *p, const float *lrf_in, float *shot, float *lrf_out, unsigned long long *sums,
                       uint32_t *neighbor_count)
{
  if (!ctx || !slot_ok(slot) || !shot_params_ok(p)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &cl = c->slots[slot];
  if (!cl.has_normals && cl.n > 0) return set_error(c, MVR_E_ARG, "shot: the slot has no normals");
  if (int rc = knn_cloud_ok(c, cl, "shot")) return rc;
  return shot_cloud(c, cl, *p, true, lrf_in, shot, lrf_out, sums, neighbor_count);
}

API int mvr_cloud_shot_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot, const mvr_shot_params *p,
                          const float *lrf_in, float *shot, float *lrf_out, unsigned long long *sums, uint32_t *neighbor_count)
{
  if (!ctx || !slot_ok(q_slot) || !slot_ok(surface_slot) || !shot_params_ok(p)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[q_slot], &t = c->slots[surface_slot];
  if (!t.has_normals && t.n > 0) return set_error(c, MVR_E_ARG, "shot: the surface slot has no normals");
  if (int rc = knn_cloud_ok(c, q, "shot")) return rc;
  if (int rc = knn_cloud_ok(c, t, "shot")) return rc;
  if (int rc = at_indices_ok(c, q, indices, n_indices, "shot")) return rc;
  if (!indices && q_slot == surface_slot) return shot_cloud(c, t, *p, true, lrf_in, shot, lrf_out, sums, neighbor_count);      // Q8
  return shot_cloud(c, t, *p, true, lrf_in, shot, lrf_out, sums, neighbor_count, &q, indices, n_indices);
}
