// csrc/mvr_mls.hip -- pcl::MovingLeastSquares (upsampling NONE, the SIMPLE projection, polynomial order at most 2) on the GPU
// (gfx950); the rules are written next to mvr_cloud_mls in mvr_hip.h.
//
// One thread per query, in the order of the cloud's model grid (ensure_model_grid; the helpers of mvr_knn_walk.h), so the 64
// lanes of a wave are neighbours on the surface and walk the same cells:
//   1. the ball walk (knn_ball_walk) accumulates the f64 moments of the neighbours about the query point; cyclic
//      Jacobi gives the plane (mvr_plane.h).  Fewer than 3 neighbours: the point is dropped.
//   2. order 2 and at least 6 neighbours: the SAME walk a second time (the cells' lines are in L1 / L2 from the first)
//      accumulates, in f64, the 15 monomial sums and the 6 right-hand sums of the weighted bivariate fit about the projected
//      query.  Everything is taken relative to the query point: the projected query is q + t n with t = (mean - q) . n, a
//      neighbour's offset from it (p - q) - t n, so no sum ever sees the magnitude of the coordinates.
//   3. the 6 x 6 normal equations are solved by Cholesky in registers: the loops are fully unrolled, every index a compile-time
//      constant (a runtime-indexed private array lives in scratch memory: mvr_knn.hip).  A pivot that is not finite and
//      positive, or a coefficient that is not finite, abandons the fit; the plane result stands.
//   4. the results are written by SOURCE index into arrays of the context's arena (Ctx::dn_arena), with a keep flag;
//      select_flagged gives the kept indices, ascending; gather_kept moves points and normals.
// No atomics and a fixed walk order: bit-identical from run to run on one grid.  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_plane.h"

namespace mvr {
namespace {

constexpr int kMlsThreads = kKnnThreads;

struct MlsArgs {
  KnnSlot S;                       // the cloud searched against itself (nrm / curv / oidx / od2 unused)
  const float4 *src_nrm;           // orient 1: the source slot's normals, by index
  float4 *out_pts, *out_nrm;       // by source index; out_nrm only with `normals`
  float *curv;                     // by source index
  uint8_t *keep;                   // by source index: the point is in the output
  double sqr_gauss;
  float r2, vp[3];
  int normals, orient;
};

// the 21 sums of the weighted fit of f over the basis 1, b, b^2, a, ab, a^2: s<i><j> = sum of w a^i b^j, r* = the same times f
struct MlsSums {
  double s00 = 0.0, s10 = 0.0, s01 = 0.0, s20 = 0.0, s11 = 0.0, s02 = 0.0, s30 = 0.0, s21 = 0.0, s12 = 0.0, s03 = 0.0,
         s40 = 0.0, s31 = 0.0, s22 = 0.0, s13 = 0.0, s04 = 0.0;
  double r00 = 0.0, r01 = 0.0, r02 = 0.0, r10 = 0.0, r11 = 0.0, r20 = 0.0;
  __device__ __forceinline__ void add(const double w, const double a, const double b, const double f)
  {
    const double wa = w * a, wb = w * b, waa = wa * a, wab = wa * b, wbb = wb * b;
    const double waaa = waa * a, waab = waa * b, wabb = wab * b, wbbb = wbb * b;
    s00 += w; s10 += wa; s01 += wb; s20 += waa; s11 += wab; s02 += wbb;
    s30 += waaa; s21 += waab; s12 += wabb; s03 += wbbb;
    s40 += waaa * a; s31 += waaa * b; s22 += waab * b; s13 += wabb * b; s04 += wbbb * b;
    r00 += w * f; r01 += wb * f; r02 += wbb * f; r10 += wa * f; r11 += wab * f; r20 += waa * f;
  }
};

// the normal equations A c = r over the basis 1, b, b^2, a, ab, a^2 by Cholesky (A = L L^T); false: a pivot was not finite and
// positive, or -- a pivot may be positive and still as small as a denormal -- one of the coefficients the result is made of
// (c0, c1, c3) is not finite.  Fully unrolled: A, y and c are registers.
__device__ __forceinline__ bool mls_solve(const MlsSums &m, double (&c)[6])
{
  double A[6][6], y[6];
  A[0][0] = m.s00;
  A[1][0] = m.s01; A[1][1] = m.s02;
  A[2][0] = m.s02; A[2][1] = m.s03; A[2][2] = m.s04;
  A[3][0] = m.s10; A[3][1] = m.s11; A[3][2] = m.s12; A[3][3] = m.s20;
  A[4][0] = m.s11; A[4][1] = m.s12; A[4][2] = m.s13; A[4][3] = m.s21; A[4][4] = m.s22;
  A[5][0] = m.s20; A[5][1] = m.s21; A[5][2] = m.s22; A[5][3] = m.s30; A[5][4] = m.s31; A[5][5] = m.s40;
  y[0] = m.r00; y[1] = m.r01; y[2] = m.r02; y[3] = m.r10; y[4] = m.r11; y[5] = m.r20;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= A[j][k] * A[j][k];
    ok = ok && s > 0.0 && isfinite(s);
    const double d = sqrt(s);
    A[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
      A[i][j] = t / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {                 // L y = r
    double t = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= A[i][k] * y[k];
    y[i] = t / A[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {                // L^T c = y
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= A[k][i] * c[k];
    c[i] = t / A[i][i];
  }
  return ok && isfinite(c[0]) && isfinite(c[1]) && isfinite(c[3]);
}

// POLY: the call asked for order 2 (a point with fewer than 6 neighbours still gets the plane alone)
template <bool FMA, bool POLY>
__global__ void __launch_bounds__(kMlsThreads) mls_kernel(MlsArgs a)
{
  const KnnSlot &S = a.S;
  // (knn_query, written out: through the helper the order-2 kernel takes two more registers than this)
  const uint32_t pos = blockIdx.x * kMlsThreads + threadIdx.x;
  if (pos >= S.nq) return;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  Moments M;      // (a non-finite query walks nothing: no neighbours, dropped)
  knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 p, uint32_t) { M.add(p, q); });
  if (M.cnt < 3.0) { a.keep[qi] = 0; return; }
  const PlaneFit f = plane_fit(M);
  const double t = f.m0 * f.nx + f.m1 * f.ny + f.m2 * f.nz;      // the projected query is q + t n
  double h = t, nx = f.nx, ny = f.ny, nz = f.nz;                  // the output: q + h n, and its normal
  if (POLY && M.cnt >= 6.0) {
    // u: a unit vector orthogonal to n, built from the axis n leans on least; v = n x u, so u x v = n
    const double ax = fabs(f.nx), ay = fabs(f.ny), az = fabs(f.nz);
    const bool px = ax <= ay && ax <= az, py = !px && ay <= az;
    double ux = px ? 0.0 : (py ? -f.nz : -f.ny), uy = px ? -f.nz : (py ? 0.0 : f.nx), uz = px ? f.ny : (py ? f.nx : 0.0);
    const double un = 1.0 / sqrt(ux * ux + uy * uy + uz * uz);
    ux *= un; uy *= un; uz *= un;
    const double vx = f.ny * uz - f.nz * uy, vy = f.nz * ux - f.nx * uz, vz = f.nx * uy - f.ny * ux;
    const double tx = t * f.nx, ty = t * f.ny, tz = t * f.nz, ig = -1.0 / a.sqr_gauss;
    MlsSums m;
    knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 p, uint32_t) {
      const double dx = ((double)p.x - (double)q.x) - tx, dy = ((double)p.y - (double)q.y) - ty, dz = ((double)p.z - (double)q.z) - tz;
      const double w = exp((dx * dx + dy * dy + dz * dz) * ig);
      m.add(w, dx * ux + dy * uy + dz * uz, dx * vx + dy * vy + dz * vz, dx * f.nx + dy * f.ny + dz * f.nz);
    });
    double c[6];
    if (mls_solve(m, c)) {
      h = t + c[0];
      if (a.normals) {
        const double gx = f.nx - c[3] * ux - c[1] * vx, gy = f.ny - c[3] * uy - c[1] * vy, gz = f.nz - c[3] * uz - c[1] * vz;
        const double gn = 1.0 / sqrt(gx * gx + gy * gy + gz * gz);
        nx = gx * gn; ny = gy * gn; nz = gz * gn;
      }
    }
  }
  a.out_pts[qi] = make_float4((float)((double)q.x + h * f.nx), (float)((double)q.y + h * f.ny), (float)((double)q.z + h * f.nz), 1.f);
  a.curv[qi] = plane_curvature(f);
  a.keep[qi] = 1;
  if (a.normals) {
    // the f32 flip of mvr_cloud_estimate_normals, against the viewpoint seen from the source point or against its normal
    float rx, ry, rz;
    if (a.orient) { const float4 s = a.src_nrm[qi]; rx = s.x; ry = s.y; rz = s.z; }
    else { rx = a.vp[0] - q.x; ry = a.vp[1] - q.y; rz = a.vp[2] - q.z; }
    a.out_nrm[qi] = plane_normal_towards((float)nx, (float)ny, (float)nz, rx, ry, rz);
  }
}

__global__ void __launch_bounds__(kMlsThreads) mls_gather_curv_kernel(const float *__restrict__ in, const unsigned long long *__restrict__ list, size_t kept,
                                                                      float *__restrict__ out)
{
  const size_t k = (size_t)blockIdx.x * kMlsThreads + threadIdx.x;
  if (k < kept) out[k] = in[(uint32_t)list[k]];
}

int mls_cloud(Ctx *c, Cloud &dst, Cloud &src, const mvr_mls_params &p, size_t *n_out, uint32_t *kept_index, float *curvature)
{
  const size_t n = src.n;
  const bool computed = p.compute_normals != 0, normals = computed || src.has_normals;
  size_t kept = 0;
  if (p.orient == 1 && !src.has_normals) return set_error(c, MVR_E_ARG, "mls: orient 1 needs the source slot's normals");
  if (int rc = knn_cloud_ok(c, src, "mls")) return rc;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "mls reads back");
    size_t sel_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    MlsArgs a{};
    if (int rc = fill_target(c, src, a.S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
    fill_queries(src, a.S);
    Carver plan;
    plan.plan<uint8_t>(n); plan.plan<unsigned long long>(n); plan.plan<uint32_t>(4); plan.plan<float4>(n); plan.plan<float4>(n); plan.plan<float>(n);
    plan.plan<float4>(n); plan.plan<uint32_t>(n); plan.plan<float>(n); plan.plan<char>(sel_bytes);
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    uint8_t *keep = s.take<uint8_t>(n);
    unsigned long long *list = s.take<unsigned long long>(n);
    uint32_t *counters = s.take<uint32_t>(4);
    float4 *o_pts = s.take<float4>(n), *o_nrm = s.take<float4>(n);
    float *o_curv = s.take<float>(n);
    float4 *out = s.take<float4>(n);
    uint32_t *d_index = s.take<uint32_t>(n);
    float *curv_out = s.take<float>(n);
    char *tmp = s.take<char>(sel_bytes);
    // 1. the fit, by source index
    a.src_nrm = src.nrm; a.out_pts = o_pts; a.out_nrm = o_nrm; a.curv = o_curv; a.keep = keep;
    a.sqr_gauss = p.sqr_gauss_param != 0.0 ? p.sqr_gauss_param : p.radius * p.radius;
    a.r2 = clamp_r2(p.radius);
    for (int j = 0; j < 3; ++j) a.vp[j] = p.viewpoint[j];
    a.normals = computed ? 1 : 0; a.orient = p.orient;
    const dim3 grid(blocks_for(n, kMlsThreads)), block(kMlsThreads);
    const bool fma = p.fma_dist != 0, poly = p.order == 2;
    if (fma) { if (poly) hipLaunchKernelGGL((mls_kernel<true, true>), grid, block, 0, c->stream, a); else hipLaunchKernelGGL((mls_kernel<true, false>), grid, block, 0, c->stream, a); }
    else { if (poly) hipLaunchKernelGGL((mls_kernel<false, true>), grid, block, 0, c->stream, a); else hipLaunchKernelGGL((mls_kernel<false, false>), grid, block, 0, c->stream, a); }
    MVR_HIP_TRY(c, hipGetLastError());
    // 2. the kept indices, ascending; the one read-back
    uint32_t hc[4] = {0, 0, 0, 0};
    if (int rc = select_flagged(c, tmp, sel_bytes, keep, n, list, counters)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    kept = hc[0];
    // 3. the output.  Every result lies in the arena, so an in-place call gathers straight into the slot -- except the source's
    // own normals, which follow their points through a copy as in the outlier filters
    if (int rc = gather_kept(c, dst, o_pts, computed ? o_nrm : normals ? src.nrm : nullptr, list, kept, out, d_index)) return rc;
    if (curvature && kept) {
      hipLaunchKernelGGL(mls_gather_curv_kernel, dim3(blocks_for(kept, kMlsThreads)), dim3(kMlsThreads), 0, c->stream, o_curv, list, kept, curv_out);
      MVR_HIP_TRY(c, hipGetLastError());
      MVR_HIP_TRY(c, hipMemcpyAsync(curvature, curv_out, kept * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    if (kept_index && kept) MVR_HIP_TRY(c, hipMemcpyAsync(kept_index, d_index, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  }
  finish_dst(c, dst, kept, normals);
  if (n_out) *n_out = kept;
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API int mvr_cloud_mls(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_mls_params *p, size_t *n_out, uint32_t *kept_index, float *curvature)
{
  if (!ctx || !p || !slot_ok(dst_slot) || !slot_ok(src_slot)) return MVR_E_ARG;
  if (!(std::isfinite(p->radius) && p->radius > 0.0) || !(std::isfinite(p->sqr_gauss_param) && p->sqr_gauss_param >= 0.0)) return MVR_E_ARG;
  if (p->order < 0 || p->order > 2 || p->orient < 0 || p->orient > 1) return MVR_E_ARG;
  for (int j = 0; j < 3; ++j) if (!std::isfinite(p->viewpoint[j])) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return mls_cloud(c, c->slots[dst_slot], c->slots[src_slot], *p, n_out, kept_index, curvature);
}
