// csrc/mvr_ndt.hip -- pcl::NormalDistributionsTransform on the GPU (gfx950); the rules N1-N12 are written next to mvr_ndt_align
// in mvr_hip.h.  The Newton loop (N7-N9) is host code in mvr_align.hip; this file holds what it calls:
//   ndt_build_cells   the target's voxels through the f32 index and sort of mvr_voxel.hip (voxel_sorted_index), then
//     ndt_cell_kernel   a wave per voxel: mean, centred covariance (two passes, lane l over sorted positions l, l + 64, ...,
//                       then the fixed-order wave sum), 3 x 3 Jacobi, inflated eigenvalues, C^-1 (N3);
//     flagged selection + ndt_gather_kernel: the kept cells in ascending voxel index, and the dense table voxel -> cell;
//   ndt_eval          ndt_sums_kernel (a thread per source point, grid-stride; the 27 candidates in ascending voxel index, found
//                     in the dense table or by a binary search per (j, k) row of the lattice; 29 f64 accumulators, block
//                     partials) + ndt_final_kernel (one block adds the rows in fixed order) + a 232-byte read-back.
// No float atomics: every sum is bit-identical from run to run, and the two lookups visit the same cells in the same order.
// An evaluation reads 16 bytes per source point and up to 27 x 72 bytes of cells that neighbouring points share (L2); it is
// f64-ALU-bound.  Compiled with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvr_internal.h"
#include "mvr_block_sums.h"
#include "mvr_plane.h"

namespace mvr {

namespace {

constexpr int kCellThreads = 256, kCellWaves = kCellThreads / 64;

__global__ __launch_bounds__(kCellThreads) void ndt_vstart_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ vid, size_t nf,
                                                                   uint32_t *__restrict__ vstart)
{
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nf) return;
  if (head[j]) vstart[vid[j] - 1u] = (uint32_t)j;
}

// N3, a wave per voxel (grid-stride over the voxels; their number is the last entry of the scan).  Every lane of the wave
// reaches every wave_sum: the loop over voxels and the test on the count are wave-uniform.
__global__ __launch_bounds__(kCellThreads) void ndt_cell_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ sidx,
                                                                 const uint32_t *__restrict__ vid, const uint32_t *__restrict__ vstart, size_t nf,
                                                                 const float4 *__restrict__ pts, uint32_t min_points, double mult,
                                                                 uint8_t *__restrict__ flag, unsigned long long *__restrict__ vkey,
                                                                 uint32_t *__restrict__ vcnt, double *__restrict__ vmean, double *__restrict__ vicov)
{
  const uint32_t nv = vid[nf - 1];
  const uint32_t lane = threadIdx.x & 63u, nw = gridDim.x * kCellWaves;
  for (uint32_t v = blockIdx.x * kCellWaves + (threadIdx.x >> 6); v < nv; v += nw) {
    const uint32_t b = vstart[v], e = v + 1u < nv ? vstart[v + 1u] : (uint32_t)nf, cnt = e - b;
    if (cnt < min_points) continue;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t k = b + lane; k < e; k += 64u) {
      const float4 p = pts[sidx[k]];
      s0 += (double)p.x; s1 += (double)p.y; s2 += (double)p.z;
    }
    const double n = (double)cnt;
    const double m0 = wave_sum(s0) / n, m1 = wave_sum(s1) / n, m2 = wave_sum(s2) / n;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (uint32_t k = b + lane; k < e; k += 64u) {
      const float4 p = pts[sidx[k]];
      const double dx = (double)p.x - m0, dy = (double)p.y - m1, dz = (double)p.z - m2;
      xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    const double f = ((n - 1.0) / n) * (1.0 / n);
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    A[0][0] = f * wave_sum(xx); A[0][1] = A[1][0] = f * wave_sum(xy); A[0][2] = A[2][0] = f * wave_sum(xz);
    A[1][1] = f * wave_sum(yy); A[1][2] = A[2][1] = f * wave_sum(yz); A[2][2] = f * wave_sum(zz);
    for (int sweep = 0; sweep < 12; ++sweep) {
      const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
      const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
      if (!(off > 1.0e-40 * dia)) break;                      // (an all-zero matrix ends here too)
      jacobi_rot<0, 1, 2>(A, V);
      jacobi_rot<0, 2, 1>(A, V);
      jacobi_rot<1, 2, 0>(A, V);
    }
    const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
    const double lmax = fmax(fmax(l0, l1), l2);
    if (!(isfinite(l0) && isfinite(l1) && isfinite(l2) && lmax > 0.0)) continue;      // (coincident points: dropped)
    const double fl = mult * lmax;
    const double i0 = 1.0 / fmax(l0, fl), i1 = 1.0 / fmax(l1, fl), i2 = 1.0 / fmax(l2, fl);
    if (lane != 0u) continue;
    flag[v] = 1;
    vkey[v] = key[b];
    vcnt[v] = cnt;
    vmean[3 * (size_t)v + 0] = m0; vmean[3 * (size_t)v + 1] = m1; vmean[3 * (size_t)v + 2] = m2;
    double *o = vicov + 6 * (size_t)v;
    o[0] = ((V[0][0] * V[0][0]) * i0 + (V[0][1] * V[0][1]) * i1) + (V[0][2] * V[0][2]) * i2;
    o[1] = ((V[0][0] * V[1][0]) * i0 + (V[0][1] * V[1][1]) * i1) + (V[0][2] * V[1][2]) * i2;
    o[2] = ((V[0][0] * V[2][0]) * i0 + (V[0][1] * V[2][1]) * i1) + (V[0][2] * V[2][2]) * i2;
    o[3] = ((V[1][0] * V[1][0]) * i0 + (V[1][1] * V[1][1]) * i1) + (V[1][2] * V[1][2]) * i2;
    o[4] = ((V[1][0] * V[2][0]) * i0 + (V[1][1] * V[2][1]) * i1) + (V[1][2] * V[2][2]) * i2;
    o[5] = ((V[2][0] * V[2][0]) * i0 + (V[2][1] * V[2][1]) * i1) + (V[2][2] * V[2][2]) * i2;
  }
}

// the kept voxels (list: ascending voxel numbers, *count of them) -> the cell arrays; table (dense route) gets the cell number
__global__ __launch_bounds__(kCellThreads) void ndt_gather_kernel(const unsigned long long *__restrict__ list, const uint32_t *__restrict__ count,
                                                                   const unsigned long long *__restrict__ vkey, const uint32_t *__restrict__ vcnt,
                                                                   const double *__restrict__ vmean, const double *__restrict__ vicov,
                                                                   unsigned long long *__restrict__ ckey, uint32_t *__restrict__ ccnt,
                                                                   double *__restrict__ cmean, double *__restrict__ cicov, size_t cap,
                                                                   uint32_t *__restrict__ table, unsigned long long table_size)
{
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= *count || k >= cap) return;
  const size_t v = (size_t)list[k];
  const unsigned long long key = vkey[v];
  ckey[k] = key;
  ccnt[k] = vcnt[v];
  for (int a = 0; a < 3; ++a) cmean[3 * k + a] = vmean[3 * v + a];
  for (int a = 0; a < 6; ++a) cicov[6 * k + a] = vicov[6 * v + a];
  if (table && key < table_size) table[key] = (uint32_t)k;
}

struct NdtGeom {
  float inv, minbf[3];
  long long div[3];
  uint32_t n_cells;
};

// N6 for one counted candidate
__device__ __forceinline__ void ndt_pair(const double *__restrict__ mean, const double *__restrict__ icov, uint32_t cell, const double y[3],
                                         const double JA[3][3], const double KK[6][3], double d1, double d2, double r2, double (&acc)[29])
{
  const double *m = mean + 3 * (size_t)cell;
  const double dx = y[0] - m[0], dy = y[1] - m[1], dz = y[2] - m[2];
  if (!((dx * dx + dy * dy) + dz * dz <= r2)) return;
  const double *ci = icov + 6 * (size_t)cell;
  const double c00 = ci[0], c01 = ci[1], c02 = ci[2], c11 = ci[3], c12 = ci[4], c22 = ci[5];
  const double v0 = (c00 * dx + c01 * dy) + c02 * dz, v1 = (c01 * dx + c11 * dy) + c12 * dz, v2 = (c02 * dx + c12 * dy) + c22 * dz;
  const double q = (dx * v0 + dy * v1) + dz * v2;
  const double e = exp(-(d2 * q) / 2.0), w = d2 * e;
  if (!(w >= 0.0 && w <= 1.0)) return;                               // PCL's guard; a NaN fails it too
  const double f = d1 * w;
  double a[6] = {v0, v1, v2, 0.0, 0.0, 0.0}, CJ[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[3 + k] = (v0 * JA[k][0] + v1 * JA[k][1]) + v2 * JA[k][2];
    CJ[k][0] = (c00 * JA[k][0] + c01 * JA[k][1]) + c02 * JA[k][2];
    CJ[k][1] = (c01 * JA[k][0] + c11 * JA[k][1]) + c12 * JA[k][2];
    CJ[k][2] = (c02 * JA[k][0] + c12 * JA[k][1]) + c22 * JA[k][2];
  }
  const double C[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
  int t = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                                      // rows of the translation
#pragma unroll
    for (int c = r; c < 3; ++c) acc[t++] += f * (C[r][c] - d2 * a[r] * a[c]);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[t++] += f * (CJ[k][r] - d2 * a[r] * a[3 + k]);
  }
  int kk = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)                                        // rows of the angles
#pragma unroll
    for (int c = r; c < 3; ++c) {
      const double jcj = (JA[r][0] * CJ[c][0] + JA[r][1] * CJ[c][1]) + JA[r][2] * CJ[c][2];
      const double vk = (v0 * KK[kk][0] + v1 * KK[kk][1]) + v2 * KK[kk][2];
      acc[t++] += f * ((jcj - d2 * a[3 + r] * a[3 + c]) + vk);
      ++kk;
    }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[21 + k] += f * a[k];
  acc[27] += 1.0;
  acc[28] += -d1 * e;
}

template <bool DENSE>
__global__ void __launch_bounds__(kRT)
ndt_sums_kernel(const float4 *__restrict__ src, size_t n, NdtPose P, NdtGeom g, const uint32_t *__restrict__ table,
                const unsigned long long *__restrict__ ckey, const double *__restrict__ mean, const double *__restrict__ icov,
                double *__restrict__ partials)
{
  double acc[29];
#pragma unroll
  for (int k = 0; k < 29; ++k) acc[k] = 0.0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float4 p = src[i];
    const double px = p.x, py = p.y, pz = p.z;
    // N4: x = G x_raw, x~ = x - o, y = R x~ + o + t
    const double xt[3] = {(((P.G[0] * px + P.G[1] * py) + P.G[2] * pz) + P.G[9]) - P.o[0],
                          (((P.G[3] * px + P.G[4] * py) + P.G[5] * pz) + P.G[10]) - P.o[1],
                          (((P.G[6] * px + P.G[7] * py) + P.G[8] * pz) + P.G[11]) - P.o[2]};
    double y[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) y[a] = (((P.R[3 * a] * xt[0] + P.R[3 * a + 1] * xt[1]) + P.R[3 * a + 2] * xt[2]) + P.o[a]) + P.t[a];
    if (!(isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]))) continue;      // N1: a non-finite source point contributes nothing
    // N5: the home voxel by the f32 rule; an axis whose h lies outside [-1, div] has no candidate
    const float hf0 = floorf((float)y[0] * g.inv) - g.minbf[0], hf1 = floorf((float)y[1] * g.inv) - g.minbf[1],
                hf2 = floorf((float)y[2] * g.inv) - g.minbf[2];
    if (!(hf0 >= -1.f && hf0 <= (float)g.div[0] && hf1 >= -1.f && hf1 <= (float)g.div[1] && hf2 >= -1.f && hf2 <= (float)g.div[2])) continue;
    const long long h0 = (long long)hf0, h1 = (long long)hf1, h2 = (long long)hf2;
    const long long ilo = h0 > 0 ? h0 - 1 : 0, ihi = h0 + 1 < g.div[0] ? h0 + 1 : g.div[0] - 1;
    if (ilo > ihi) continue;
    double JA[3][3], KK[6][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) JA[k][a] = (P.D[k][3 * a] * xt[0] + P.D[k][3 * a + 1] * xt[1]) + P.D[k][3 * a + 2] * xt[2];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) KK[k][a] = (P.DD[k][3 * a] * xt[0] + P.DD[k][3 * a + 1] * xt[1]) + P.DD[k][3 * a + 2] * xt[2];
#pragma unroll 1
    for (long long k = h2 - 1; k <= h2 + 1; ++k) {
      if (k < 0 || k >= g.div[2]) continue;
#pragma unroll 1
      for (long long j = h1 - 1; j <= h1 + 1; ++j) {
        if (j < 0 || j >= g.div[1]) continue;
        const unsigned long long base = (unsigned long long)((k * g.div[1] + j) * g.div[0]);
        if (DENSE) {
#pragma unroll 1
          for (long long ii = ilo; ii <= ihi; ++ii) {
            const uint32_t cell = table[base + (unsigned long long)ii];
            if (cell != kNone) ndt_pair(mean, icov, cell, y, JA, KK, P.d1, P.d2, P.r2, acc);
          }
        } else {
          const unsigned long long first = base + (unsigned long long)ilo, last = base + (unsigned long long)ihi;
          uint32_t lo = 0, hi = g.n_cells;                              // the first kept key >= first
          while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (ckey[mid] < first) lo = mid + 1u; else hi = mid;
          }
#pragma unroll 1
          for (; lo < g.n_cells && ckey[lo] <= last; ++lo) ndt_pair(mean, icov, lo, y, JA, KK, P.d1, P.d2, P.r2, acc);
        }
      }
    }
  }
  block_partials<29>(acc, partials);
}

__global__ void __launch_bounds__(kRT) ndt_final_kernel(const double *__restrict__ partials, int rows, double *__restrict__ out)
{
  double s[29];
  sum_rows<29>(partials, rows, s, nullptr);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 29; ++k) out[k] = s[k];      // (constant indices: s[] stays in registers)
}

}  // namespace

int ndt_build_cells(Ctx *c, const Cloud &tgt, const mvr_ndt_params *p, NdtCells *cells)
{
  *cells = NdtCells();
  cells->lat.nf = 0; cells->lat.pass = false;
  const size_t n = tgt.n;
  if (n == 0) return MVR_OK;
  if (n > 0xFFFFFFF0ull) return set_error(c, MVR_E_ARG, "NDT: target too large for 32-bit indices");
  const size_t max_cells = n / 3 + 1;
  size_t sel_bytes = 0;
  if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
  Carver plan;
  voxel_sorted_plan(c, n, plan);
  plan.plan<uint32_t>(n); plan.plan<uint8_t>(n); plan.plan<unsigned long long>(n); plan.plan<uint32_t>(n);
  plan.plan<double>(3 * n); plan.plan<double>(6 * n); plan.plan<unsigned long long>(n); plan.plan<uint32_t>(4); plan.plan<char>(sel_bytes);
  plan.plan<unsigned long long>(max_cells); plan.plan<uint32_t>(max_cells); plan.plan<double>(3 * max_cells); plan.plan<double>(6 * max_cells);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  VoxSorted vs;
  if (int rc = voxel_sorted_index(c, tgt, (float)p->resolution, s, &cells->lat, &vs)) return rc;
  const VoxLattice &L = cells->lat;
  if (L.nf == 0) return MVR_OK;
  if (L.pass) return set_error(c, MVR_E_ARG, "NDT: the voxel lattice of the target is too large for this resolution (rule 3 of mvr_cloud_voxel_grid)");
  const size_t nf = L.nf;
  uint32_t *vstart = s.take<uint32_t>(n);
  uint8_t *flag = s.take<uint8_t>(n);
  unsigned long long *vkey = s.take<unsigned long long>(n);
  uint32_t *vcnt = s.take<uint32_t>(n);
  double *vmean = s.take<double>(3 * n), *vicov = s.take<double>(6 * n);
  unsigned long long *list = s.take<unsigned long long>(n);
  uint32_t *count = s.take<uint32_t>(4);
  char *sel_tmp = s.take<char>(sel_bytes);
  unsigned long long *ckey = s.take<unsigned long long>(max_cells);
  uint32_t *ccnt = s.take<uint32_t>(max_cells);
  double *cmean = s.take<double>(3 * max_cells), *cicov = s.take<double>(6 * max_cells);
  // the dense table, when the lattice is small enough (div0 div1 div2 <= 2^63 by rule 3)
  const unsigned __int128 lattice = (unsigned __int128)L.div[0] * L.div[1] * L.div[2];
  uint32_t *table = nullptr;
  if (c->ndt_dense_max > 0 && lattice <= (unsigned __int128)c->ndt_dense_max) {
    if (int rc = ensure(c, c->ndt_table, c->ndt_table_cap, (size_t)lattice)) return rc;
    table = c->ndt_table;
    MVR_HIP_TRY(c, hipMemsetAsync(table, 0xFF, (size_t)lattice * sizeof(uint32_t), c->stream));
  }
  const uint32_t min_points = (uint32_t)std::max(3, p->min_points_per_voxel);
  MVR_HIP_TRY(c, hipMemsetAsync(flag, 0, nf, c->stream));
  MVR_HIP_TRY(c, hipMemsetAsync(count, 0, 4 * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(ndt_vstart_kernel, dim3(blocks_for(nf, kCellThreads)), dim3(kCellThreads), 0, c->stream, vs.head, vs.vid, nf, vstart);
  const unsigned cell_blocks = (unsigned)std::min<size_t>(blocks_for(nf, kCellWaves), (size_t)std::max(1, c->n_cu) * 16);
  hipLaunchKernelGGL(ndt_cell_kernel, dim3(cell_blocks), dim3(kCellThreads), 0, c->stream, vs.key, vs.idx, vs.vid, vstart, nf, tgt.pts, min_points,
                     p->min_covar_eigvalue_mult, flag, vkey, vcnt, vmean, vicov);
  MVR_HIP_TRY(c, hipGetLastError());
  size_t b = sel_bytes;
  if (int rc = select_flagged(c, sel_tmp, b, flag, nf, list, count)) return rc;
  hipLaunchKernelGGL(ndt_gather_kernel, dim3(blocks_for(max_cells, kCellThreads)), dim3(kCellThreads), 0, c->stream, list, count, vkey, vcnt, vmean,
                     vicov, ckey, ccnt, cmean, cicov, max_cells, table, (unsigned long long)lattice);
  MVR_HIP_TRY(c, hipGetLastError());
  uint32_t hc = 0;
  MVR_HIP_TRY(c, hipMemcpyAsync(&hc, count, sizeof hc, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((size_t)hc > max_cells) return set_error(c, MVR_E_HIP, "NDT: more kept cells than a third of the points");
  cells->key = ckey; cells->count = ccnt; cells->mean = cmean; cells->icov = cicov; cells->n = hc; cells->table = table;
  return MVR_OK;
}

int ndt_eval(Ctx *c, const Cloud &src, const NdtCells &cells, const NdtPose &P, double out[29])
{
  for (int k = 0; k < 29; ++k) out[k] = 0.0;
  if (src.n == 0 || cells.n == 0) return MVR_OK;
  if (src.pts_stale) return set_error(c, MVR_E_ARG, "NDT: the source's points are not current (pipelined run)");
  if (int rc = ensure(c, c->partials, c->partials_cap, (size_t)kMaxBlocks * 32)) return rc;
  const VoxLattice &L = cells.lat;
  NdtGeom g;
  g.inv = L.inv[0];
  for (int a = 0; a < 3; ++a) { g.minbf[a] = L.minbf[a]; g.div[a] = (long long)L.div[a]; }
  g.n_cells = cells.n;
  const int blocks = reduce_blocks(c, src.n);
  ProfScope ps(c, MVR_K_REDUCE, 16.0 * (double)src.n);
  if (cells.table)
    hipLaunchKernelGGL(ndt_sums_kernel<true>, dim3(blocks), dim3(kRT), 0, c->stream, src.pts, src.n, P, g, cells.table, cells.key, cells.mean,
                       cells.icov, c->partials);
  else
    hipLaunchKernelGGL(ndt_sums_kernel<false>, dim3(blocks), dim3(kRT), 0, c->stream, src.pts, src.n, P, g, cells.table, cells.key, cells.mean,
                       cells.icov, c->partials);
  hipLaunchKernelGGL(ndt_final_kernel, dim3(1), dim3(kRT), 0, c->stream, c->partials, blocks, c->moments);
  MVR_HIP_TRY(c, hipGetLastError());
  if (int rc = read_moments(c, 29)) return rc;
  std::memcpy(out, c->h_moments, 29 * sizeof(double));
  return MVR_OK;
}

}  // namespace mvr
