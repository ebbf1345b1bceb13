// csrc/mvr_mc.hip -- pcl::MarchingCubesHoppe (gfx950): the mesh of a cloud with oriented normals; the rules M1-M15 are written
// next to mvr_cloud_marching_cubes_hoppe in mvr_hip.h, the case tables in mvr_mc_tables.h.
//
//   1. Search: the exact nearest point of every lattice vertex, as a (d2 bits << 32 | index) key per vertex.  Three routes, one
//      answer.  With a cap (dist_ignore > 0) one thread per vertex -- consecutive threads consecutive z, so a wave's queries are
//      neighbours -- walks the cloud's own grid shell by shell (knn_shell_walk) with a one-entry list that starts "full" at the
//      cap: the walk ends as soon as no unvisited cell can hold a point below it.  Without a cap a vertex in the middle of a
//      hollow object is hundreds of shells from the surface, and the shell walk would look up millions of cells for it: the
//      lattice is written out as a query set instead, a slab of whole x-planes (at most 2^23 vertices) at a time, and answered
//      by the culled search behind mvr_nn (launch_nn_cull: the slab is a cloud of its own, with its ordering and boxes), which
//      is built for unbounded queries.  That search has no rule for a target with a non-finite point: such a cloud, and the
//      brute-force mode of the context, take the tiled exact search of mvr_nn.hip (launch_nn) instead, in launches of at most
//      2^38 point pairs each, since a launch cannot be pre-empted.
//   2. Values: one thread per vertex turns its key into the signed distance of M5.
//   3. Classify: one thread per cell reads its eight values and writes the cell's triangle count (a byte); the block adds its
//      cells and triangles to two device totals (integer atomics).  hipCUB's flagged selection lists the non-empty cells in
//      order; the host reads the totals -- the one wait before the output is sized.
//   4. Offsets: an exclusive sum over the listed cells' counts, 64-bit.
//   5. Emit: one thread per LISTED cell (the surface crosses O(res^2) of res^3 cells: the waves stay dense) writes its triangles
//      at its offset, M7-M9, and with weld the 64-bit key (edge key << 32 | soup position) of every corner.
//   6. Weld: one radix sort of those keys; the first of every edge key is the corner that used the edge first (the low word
//      orders a key's group by soup position).  A flag per SOUP POSITION marks those first uses, and an exclusive sum over the
//      soup positions numbers them -- "in order of first use" is the order of the soup, so no second sort.  A running maximum
//      over the sorted keys' head positions tells every corner its group's head; a last kernel scatters the indices and the
//      welded positions.
// Every arithmetic operation of M2-M8 is a single rounded f32 operation (__fadd_rn and friends; the file is compiled with
// -ffp-contract=off as well).  Nothing here writes a cloud.  All device memory comes from the pool (DevBuf).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include <hipcub/hipcub.hpp>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_mc_tables.h"

namespace mvr {
namespace {

constexpr int kMcThreads = 256;
constexpr uint32_t kMcSlab = 1u << 23;                      // lattice vertices of one query set of the exact searches
constexpr unsigned long long kMcTiledPairs = 1ull << 38;    // point pairs of one launch of the tiled search: some tens of milliseconds

struct McLattice {
  float lo[3], size[3];
  uint32_t res[3];
  uint32_t nv, ncell;              // lattice vertices (<= 2^27), cells
  float iso, cap;                  // cap: dist_ignore when > 0, else 0
};

struct McTotals {
  unsigned long long tris;
  uint32_t cells, pad;
};

// M4
__device__ __forceinline__ float mc_coord(const McLattice &L, const int a, const uint32_t i) { return __fadd_rn(L.lo[a], __fmul_rn(L.size[a], (float)i)); }

__device__ __forceinline__ float4 mc_vertex(const McLattice &L, const uint32_t v)
{
  const uint32_t z = v % L.res[2], xy = v / L.res[2], y = xy % L.res[1], x = xy / L.res[1];
  return make_float4(mc_coord(L, 0, x), mc_coord(L, 1, y), mc_coord(L, 2, z), 0.f);
}

// the offsets of corner i (M6) as bits: x of corners 1 2 5 6, y of 4..7, z of 2 3 6 7
__device__ __forceinline__ uint32_t mc_ox(const uint32_t i) { return (0x66u >> i) & 1u; }
__device__ __forceinline__ uint32_t mc_oy(const uint32_t i) { return (0xF0u >> i) & 1u; }
__device__ __forceinline__ uint32_t mc_oz(const uint32_t i) { return (0xCCu >> i) & 1u; }
// the two corners of edge e (M8)
__device__ __forceinline__ uint32_t mc_edge_a(const uint32_t e) { return e < 8u ? e : e - 8u; }
__device__ __forceinline__ uint32_t mc_edge_b(const uint32_t e) { return e < 4u ? ((e + 1u) & 3u) : (e < 8u ? 4u + ((e + 1u) & 3u) : e - 4u); }

// the lattice vertices v0 .. v0 + n as a query set
__global__ void __launch_bounds__(kMcThreads) mc_lattice_kernel(McLattice L, uint32_t v0, uint32_t n, float4 *q)
{
  const uint32_t k = blockIdx.x * kMcThreads + threadIdx.x;
  if (k < n) { float4 p = mc_vertex(L, v0 + k); p.w = 1.f; q[k] = p; }
}

__global__ void __launch_bounds__(kMcThreads) mc_count_bad_kernel(const float4 *pts, uint32_t n, uint32_t *count)
{
  const uint32_t i = blockIdx.x * kMcThreads + threadIdx.x;
  if (i < n && !finite3(pts[i])) atomicAdd(count, 1u);
}

// the one-entry list of the shell walk: `best` starts at the empty key, or at (cap, index 0) -- below which exactly the keys
// with d2 < cap lie
template <bool FMA>
struct McNearest {
  nnkey_t best;
  const KnnSlot &S;
  const float4 q;
  __device__ __forceinline__ void visit(const float4 p, const uint32_t j)
  {
    const nnkey_t key = ((nnkey_t)__float_as_uint(knn_dist2<FMA>(p, q)) << 32) | knn_index_of(S, p, j);
    if (key < best) best = key;
  }
  __device__ __forceinline__ bool full() const { return best != kKnnKeyEmpty; }
  // strictly beyond: a cell AT the distance may hold a tie with a lower index
  __device__ __forceinline__ bool beyond(const double b2) const { return b2 > (double)__uint_as_float((uint32_t)(best >> 32)); }
};

template <bool FMA>
__global__ void __launch_bounds__(kMcThreads) mc_walk_kernel(KnnSlot S, McLattice L, nnkey_t start, nnkey_t *keys)
{
  const uint32_t v = blockIdx.x * kMcThreads + threadIdx.x;
  if (v >= L.nv) return;
  McNearest<FMA> vis{start, S, mc_vertex(L, v)};
  knn_shell_walk(S, vis.q, vis);
  keys[v] = vis.best == start ? kKeyInit : vis.best;
}

// M5
__global__ void __launch_bounds__(kMcThreads) mc_value_kernel(McLattice L, const nnkey_t *keys, const float4 *pts, const float4 *nrm, uint32_t n,
                                                              float *grid)
{
  const uint32_t v = blockIdx.x * kMcThreads + threadIdx.x;
  if (v >= L.nv) return;
  const nnkey_t key = keys[v];
  const uint32_t j = (uint32_t)key;
  const float d2 = __uint_as_float((uint32_t)(key >> 32));
  float val = __builtin_nanf("");
  if (j < n && !(L.cap > 0.f && !(d2 < L.cap))) {
    const float4 q = mc_vertex(L, v), p = pts[j], m = nrm[j];
    const float norm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(m.x, m.x), __fmul_rn(m.y, m.y)), __fmul_rn(m.z, m.z)));
    if (!isnan(m.x) && norm > 0.5f) {
      const float dx = __fsub_rn(q.x, p.x), dy = __fsub_rn(q.y, p.y), dz = __fsub_rn(q.z, p.z);
      val = __fadd_rn(__fadd_rn(__fmul_rn(m.x, dx), __fmul_rn(m.y, dy)), __fmul_rn(m.z, dz));
    }
  }
  grid[v] = val;
}

// the cell of this number (M6's order), the 1-D index of its corner 0, and its cube index; false: a NaN corner
__device__ __forceinline__ bool mc_cube(const McLattice &L, const float *grid, const uint32_t cell, uint32_t *x, uint32_t *y, uint32_t *z,
                                        uint32_t *base, uint32_t *cube)
{
  const uint32_t cz = L.res[2] - 1u, cy = L.res[1] - 1u;
  *z = cell % cz;
  const uint32_t xy = cell / cz;
  *y = xy % cy;
  *x = xy / cy;
  *base = (*x * L.res[1] + *y) * L.res[2] + *z;
  uint32_t cb = 0;
  bool ok = true;
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) {
    const float val = grid[*base + (mc_ox(i) * L.res[1] + mc_oy(i)) * L.res[2] + mc_oz(i)];
    ok = ok && !isnan(val);
    if (val < L.iso) cb |= 1u << i;
  }
  *cube = cb;
  return ok;
}

__global__ void __launch_bounds__(kMcThreads) mc_classify_kernel(McLattice L, const float *grid, uint8_t *cnt, McTotals *totals)
{
  __shared__ uint32_t s_tris, s_cells;
  if (threadIdx.x == 0) { s_tris = 0u; s_cells = 0u; }
  __syncthreads();
  const uint32_t cell = blockIdx.x * kMcThreads + threadIdx.x;
  if (cell < L.ncell) {
    uint32_t x, y, z, base, cube, n = 0;
    if (mc_cube(L, grid, cell, &x, &y, &z, &base, &cube))
      while (n < 5u && kMcTriTable[cube][3u * n] >= 0) ++n;
    cnt[cell] = (uint8_t)n;
    if (n) { atomicAdd(&s_tris, n); atomicAdd(&s_cells, 1u); }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cells) {
    atomicAdd(&totals->tris, (unsigned long long)s_tris);
    atomicAdd(&totals->cells, s_cells);
  }
}

// the listed cells' counts as 64-bit addends, one more entry of 0 behind them
__global__ void __launch_bounds__(kMcThreads) mc_len_kernel(const unsigned long long *list, const uint8_t *cnt, uint32_t m, unsigned long long *len)
{
  const uint32_t k = blockIdx.x * kMcThreads + threadIdx.x;
  if (k < m) len[k] = cnt[list[k]];
  else if (k == m) len[k] = 0ull;
}

// M7-M9 (and M13's keys): soup = 9 floats per triangle; wkeys (weld) one key per soup vertex
__global__ void __launch_bounds__(kMcThreads) mc_emit_kernel(McLattice L, const float *grid, const unsigned long long *list, const unsigned long long *off,
                                                             uint32_t m, unsigned long long total, float *soup, unsigned long long *wkeys)
{
  const uint32_t k = blockIdx.x * kMcThreads + threadIdx.x;
  if (k >= m) return;
  uint32_t x, y, z, base, cube;
  if (!mc_cube(L, grid, (uint32_t)list[k], &x, &y, &z, &base, &cube)) return;
  const float x0 = mc_coord(L, 0, x), y0 = mc_coord(L, 1, y), z0 = mc_coord(L, 2, z);
  const float x1 = __fadd_rn(x0, L.size[0]), y1 = __fadd_rn(y0, L.size[1]), z1 = __fadd_rn(z0, L.size[2]);
  unsigned long long at = off[k] * 3ull;      // soup vertices before this cell's
  for (uint32_t r = 0; r < 15u; ++r) {
    const int e8 = kMcTriTable[cube][r];
    if (e8 < 0) break;
    if (at >= total * 3ull) break;            // (the count and the fill see the same values: never)
    const uint32_t e = (uint32_t)e8, a = mc_edge_a(e), b = mc_edge_b(e);
    const uint32_t ax = mc_ox(a), ay = mc_oy(a), az = mc_oz(a), bx = mc_ox(b), by = mc_oy(b), bz = mc_oz(b);
    const float va = grid[base + (ax * L.res[1] + ay) * L.res[2] + az], vb = grid[base + (bx * L.res[1] + by) * L.res[2] + bz];
    const float mu = __fdiv_rn(__fsub_rn(L.iso, va), __fsub_rn(vb, va));
    const float pax = ax ? x1 : x0, pay = ay ? y1 : y0, paz = az ? z1 : z0;
    const float pbx = bx ? x1 : x0, pby = by ? y1 : y0, pbz = bz ? z1 : z0;
    float *o = soup + at * 3ull;
    o[0] = __fadd_rn(pax, __fmul_rn(mu, __fsub_rn(pbx, pax)));
    o[1] = __fadd_rn(pay, __fmul_rn(mu, __fsub_rn(pby, pay)));
    o[2] = __fadd_rn(paz, __fmul_rn(mu, __fsub_rn(pbz, paz)));
    if (wkeys) {
      const uint32_t axis = ax != bx ? 0u : (ay != by ? 1u : 2u);
      const uint32_t low = base + ((ax & bx) * L.res[1] + (ay & by)) * L.res[2] + (az & bz);
      wkeys[at] = ((unsigned long long)(3u * low + axis) << 32) | (unsigned long long)(uint32_t)at;
    }
    ++at;
  }
}

// sorted keys -> first[soup position] = 1 at the first use of an edge, head[i] = i there and 0 elsewhere
__global__ void __launch_bounds__(kMcThreads) mc_weld_mark_kernel(const unsigned long long *sorted, uint32_t n, uint32_t *first, uint32_t *head)
{
  const uint32_t i = blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = sorted[i];
  const bool h = i == 0u || (uint32_t)(sorted[i - 1u] >> 32) != (uint32_t)(key >> 32);
  if ((uint32_t)key < n) first[(uint32_t)key] = h ? 1u : 0u;      // (every soup position has exactly one key: always)
  head[i] = h ? i : 0u;
}

// head: the running maximum of the above = where corner i's group begins; newid: the exclusive sum of first[]
__global__ void __launch_bounds__(kMcThreads) mc_weld_scatter_kernel(const unsigned long long *sorted, uint32_t n, const uint32_t *head,
                                                                     const uint32_t *newid, const float *soup, uint32_t *indices, float *welded)
{
  const uint32_t i = blockIdx.x * kMcThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t pos = (uint32_t)sorted[i], h = head[i], hpos = (uint32_t)sorted[h];
  if (pos >= n || hpos >= n) return;                                   // (never: see mc_weld_mark_kernel)
  const uint32_t id = newid[hpos];
  indices[pos] = id;
  if (h == i) {
    welded[3ull * id] = soup[3ull * pos];
    welded[3ull * id + 1ull] = soup[3ull * pos + 1ull];
    welded[3ull * id + 2ull] = soup[3ull * pos + 2ull];
  }
}

// the wall clock of the stages (tune "mc_clock"): waits for the stream, then books the time since the previous mark
struct McClock {
  Ctx *c;
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  int mark(int stage)
  {
    if (!c->mc_clock) return MVR_OK;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const auto now = std::chrono::steady_clock::now();
    c->mc_ms[stage] += std::chrono::duration<double, std::milli>(now - last).count();
    last = now;
    return MVR_OK;
  }
};

int copy_home(Ctx *c, void *dst, const void *src, size_t bytes)
{
  if (!dst || !bytes) return MVR_OK;
  MVR_HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API void mvr_mc_default_params(mvr_mc_params *p)
{
  if (!p) return;
  p->res[0] = p->res[1] = p->res[2] = 32;
  p->iso_level = 0.f; p->percentage_extend_grid = 0.f; p->dist_ignore = -1.f; p->weld = 0; p->fma_dist = 0;
}

API int mvr_mc_case(int cube, uint16_t *edges, int8_t tri[16])
{
  if (cube < 0 || cube > 255) return MVR_E_ARG;
  if (edges) *edges = kMcEdgeTable[cube];
  if (tri) std::memcpy(tri, kMcTriTable[cube], 16);
  return MVR_OK;
}

API int mvr_cloud_marching_cubes_hoppe(mvr_ctx *ctx, int slot, const mvr_mc_params *p, float *grid_out, float *vertices, size_t capacity,
                                       uint32_t *indices, uint64_t *n_triangles, uint64_t *n_vertices)
{
  const char *fn = "mvr_cloud_marching_cubes_hoppe";
  if (!ctx) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  if (!p) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: no parameters");
  if (!slot_ok(slot)) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: a slot number outside 0..MVR_MAX_SLOTS - 1");
  unsigned long long nv = 1ull;
  for (int a = 0; a < 3; ++a) {
    if (p->res[a] < 2) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: a grid resolution below 2");
    nv *= (unsigned long long)p->res[a];      // (three factors below 2^31: below 2^93 only in theory -- checked after each)
    if (nv > MVR_MC_MAX_VERTICES) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: more than 2^27 lattice vertices");
  }
  if (!std::isfinite(p->iso_level) || !std::isfinite(p->percentage_extend_grid) || p->percentage_extend_grid < 0.f || std::isnan(p->dist_ignore))
    return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: iso_level / percentage_extend_grid must be finite (the latter >= 0), dist_ignore not NaN");
  if (p->weld && vertices && !indices) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: weld needs the index array");
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &cl = c->slots[slot];
  if (int rc = knn_cloud_ok(c, cl, fn)) return rc;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  auto nothing = [&]() {      // no lattice value is a number: no cell emits
    if (grid_out) for (unsigned long long v = 0; v < nv; ++v) grid_out[v] = nan;
    if (n_triangles) *n_triangles = 0;
    if (n_vertices) *n_vertices = 0;
    return MVR_OK;
  };
  if (cl.n == 0) return nothing();
  if (!cl.has_normals) return set_error(c, MVR_E_ARG, "mvr_cloud_marching_cubes_hoppe: the slot has no normals");
  MVR_MAY_BLOCK(c, "marching cubes reads back");
  for (double &ms : c->mc_ms) ms = 0.0;
  c->mc_route_used = 0;

  // M2, M3 on the host, in f32
  float bb[6];
  if (int rc = cloud_bbox(c, cl.pts, cl.n, bb, true)) return rc;
  if (!(bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5])) return nothing();      // no finite point
  McLattice L{};
  for (int a = 0; a < 3; ++a) {
    float lower = bb[a], upper = bb[3 + a];
    const float half = 0.5f * p->percentage_extend_grid;
    const float ext = half * (upper - lower);
    lower = lower - ext;
    upper = upper + ext;
    L.lo[a] = lower;
    L.size[a] = (upper - lower) / (float)p->res[a];
    L.res[a] = (uint32_t)p->res[a];
  }
  L.nv = (uint32_t)nv;
  L.ncell = (L.res[0] - 1u) * (L.res[1] - 1u) * (L.res[2] - 1u);
  L.iso = p->iso_level;
  L.cap = p->dist_ignore > 0.f ? p->dist_ignore : 0.f;
  const bool fma = p->fma_dist != 0;
  const dim3 block(kMcThreads), vgrid(blocks_for(L.nv, kMcThreads)), cgrid(blocks_for(L.ncell, kMcThreads));
  auto nomem = [&]() { return set_error(c, MVR_E_NOMEM, "mvr_cloud_marching_cubes_hoppe: out of device memory"); };
  McClock clock{c};

  // 1. the search
  DevBuf keys, grid;
  if (keys.alloc((size_t)L.nv * sizeof(nnkey_t)) != hipSuccess || grid.alloc((size_t)L.nv * sizeof(float)) != hipSuccess) return nomem();
  // (a cloud with a non-finite point has no rule under the culled search: mvr_nn in mvr_hip.h)
  int route = c->mc_route ? c->mc_route : (L.cap > 0.f ? 1 : 2);
  if (route == 2 && c->nn_mode == 0) route = 3;
  if (route == 2) {
    DevBuf cnt;
    uint32_t bad_points = 0;
    if (cnt.alloc(sizeof(uint32_t)) != hipSuccess) return nomem();
    MVR_HIP_TRY(c, hipMemsetAsync(cnt.p, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(mc_count_bad_kernel, dim3(blocks_for(cl.n, kMcThreads)), block, 0, c->stream, cl.pts, (uint32_t)cl.n, cnt.as<uint32_t>());
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipMemcpyAsync(&bad_points, cnt.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bad_points) route = 3;
  }
  c->mc_route_used = route;
  if (route == 1) {
    KnnSlot S{};
    if (int rc = fill_target(c, cl, S)) return rc;
    const nnkey_t start = L.cap > 0.f ? ((nnkey_t)__builtin_bit_cast(uint32_t, L.cap) << 32) : kKnnKeyEmpty;
    if (fma) hipLaunchKernelGGL(mc_walk_kernel<true>, vgrid, block, 0, c->stream, S, L, start, keys.as<nnkey_t>());
    else hipLaunchKernelGGL(mc_walk_kernel<false>, vgrid, block, 0, c->stream, S, L, start, keys.as<nnkey_t>());
    MVR_HIP_TRY(c, hipGetLastError());
  } else if (route == 2) {
    // the lattice, a slab of whole x-planes at a time, as a cloud of its own through the culled search: what mvr_nn does
    // for a query slot (the scratch cloud of mvr_fitness; its ordering and boxes are rebuilt per slab)
    if (int rc = launch_fill_u64(c, keys.as<nnkey_t>(), L.nv, kKeyInit)) return rc;
    if (int rc = ensure_index(c, cl)) return rc;
    Cloud &q = c->slots[kScratchTmp];
    const uint32_t plane = L.res[1] * L.res[2];
    const uint32_t planes = std::max<uint32_t>(1u, kMcSlab / plane);
    for (uint32_t x0 = 0; x0 < L.res[0]; x0 += planes) {
      const uint32_t v0 = x0 * plane, nq = std::min(planes, L.res[0] - x0) * plane;
      q.n = 0; q.has_normals = false; q.segs.clear();
      new_point_set(c, q);
      if (int rc = cloud_reserve(c, q, nq, false)) return rc;
      hipLaunchKernelGGL(mc_lattice_kernel, dim3(blocks_for(nq, kMcThreads)), block, 0, c->stream, L, v0, nq, q.pts);
      MVR_HIP_TRY(c, hipGetLastError());
      q.n = nq;
      if (int rc = ensure_index(c, q)) return rc;
      if (int rc = launch_nn_cull(c, q, 0, nq, nullptr, cl, INFINITY, fma, keys.as<nnkey_t>() + v0)) return rc;
    }
    q.n = 0;
    new_point_set(c, q);
  } else {
    // the tiled exact search, in launches of a bounded number of point pairs (a launch cannot be pre-empted)
    DevBuf lattice;
    const uint32_t per = (uint32_t)std::min<unsigned long long>(kMcSlab, std::max<unsigned long long>(kNNThreads * 8ull, kMcTiledPairs / cl.n));
    if (lattice.alloc((size_t)std::min(per, L.nv) * sizeof(float4)) != hipSuccess) return nomem();
    if (int rc = launch_fill_u64(c, keys.as<nnkey_t>(), L.nv, kKeyInit)) return rc;
    for (uint32_t v0 = 0; v0 < L.nv; v0 += per) {
      const uint32_t nq = std::min(per, L.nv - v0);
      hipLaunchKernelGGL(mc_lattice_kernel, dim3(blocks_for(nq, kMcThreads)), block, 0, c->stream, L, v0, nq, lattice.as<float4>());
      MVR_HIP_TRY(c, hipGetLastError());
      if (int rc = launch_nn(c, lattice.as<float4>(), 0, nq, nullptr, nullptr, cl.pts, cl.n, fma, keys.as<nnkey_t>() + v0)) return rc;
    }
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the query set is freed here
  }
  if (int rc = clock.mark(0)) return rc;

  // 2. the values
  hipLaunchKernelGGL(mc_value_kernel, vgrid, block, 0, c->stream, L, keys.as<nnkey_t>(), cl.pts, cl.nrm, (uint32_t)cl.n, grid.as<float>());
  MVR_HIP_TRY(c, hipGetLastError());
  if (int rc = clock.mark(1)) return rc;

  // 3. the cells: counts, totals, the list of the non-empty ones
  DevBuf cnt, list, small, sel_tmp;
  size_t sel_bytes = 0;
  if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, L.ncell, nullptr, nullptr)) return rc;
  if (cnt.alloc(L.ncell) != hipSuccess || list.alloc((size_t)L.ncell * sizeof(unsigned long long)) != hipSuccess ||
      small.alloc(sizeof(McTotals) + 256) != hipSuccess || sel_tmp.alloc(sel_bytes) != hipSuccess)
    return nomem();
  McTotals *d_tot = small.as<McTotals>();
  uint32_t *d_sel = reinterpret_cast<uint32_t *>(small.as<char>() + 64);
  MVR_HIP_TRY(c, hipMemsetAsync(small.p, 0, sizeof(McTotals) + 256, c->stream));
  hipLaunchKernelGGL(mc_classify_kernel, cgrid, block, 0, c->stream, L, grid.as<float>(), cnt.as<uint8_t>(), d_tot);
  MVR_HIP_TRY(c, hipGetLastError());
  if (int rc = select_flagged(c, sel_tmp.p, sel_bytes, cnt.as<uint8_t>(), L.ncell, list.as<unsigned long long>(), d_sel)) return rc;
  McTotals tot{};
  MVR_HIP_TRY(c, hipMemcpyAsync(&tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const unsigned long long T = tot.tris;
  const uint32_t m = tot.cells;
  if (n_triangles) *n_triangles = T;
  if (n_vertices) *n_vertices = 3ull * T;
  char msg[192];
  if (vertices && T > capacity) {
    std::snprintf(msg, sizeof msg, "mvr_cloud_marching_cubes_hoppe: capacity %zu is short of the %llu triangles (rule M11)", capacity, T);
    return set_error(c, MVR_E_ARG, msg);
  }
  if (vertices && p->weld && 3ull * T >= (1ull << 31)) {
    std::snprintf(msg, sizeof msg, "mvr_cloud_marching_cubes_hoppe: %llu triangles are too many to weld (rule M13)", T);
    return set_error(c, MVR_E_ARG, msg);
  }
  if (!vertices || T == 0) {
    if (int rc = clock.mark(2)) return rc;
    if (int rc = copy_home(c, grid_out, grid.p, (size_t)L.nv * sizeof(float))) return rc;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return clock.mark(5);
  }

  // 4. the offsets
  DevBuf len, off, scan_tmp;
  size_t scan_bytes = 0;
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(m + 1u), c->stream));
  if (len.alloc((size_t)(m + 1u) * 8) != hipSuccess || off.alloc((size_t)(m + 1u) * 8) != hipSuccess || scan_tmp.alloc(scan_bytes) != hipSuccess) return nomem();
  hipLaunchKernelGGL(mc_len_kernel, dim3(blocks_for((size_t)m + 1u, kMcThreads)), block, 0, c->stream, list.as<unsigned long long>(), cnt.as<uint8_t>(), m,
                     len.as<unsigned long long>());
  MVR_HIP_TRY(c, hipGetLastError());
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp.p, scan_bytes, len.as<unsigned long long>(), off.as<unsigned long long>(), (int)(m + 1u), c->stream));
  if (int rc = clock.mark(2)) return rc;

  // 5. the triangles
  const size_t nsoup = (size_t)(3ull * T);      // soup vertices
  DevBuf soup, wkeys;
  if (soup.alloc(nsoup * 3 * sizeof(float)) != hipSuccess) return nomem();
  if (p->weld && wkeys.alloc(nsoup * sizeof(unsigned long long)) != hipSuccess) return nomem();
  hipLaunchKernelGGL(mc_emit_kernel, dim3(blocks_for(m, kMcThreads)), block, 0, c->stream, L, grid.as<float>(), list.as<unsigned long long>(),
                     off.as<unsigned long long>(), m, T, soup.as<float>(), p->weld ? wkeys.as<unsigned long long>() : nullptr);
  MVR_HIP_TRY(c, hipGetLastError());
  if (int rc = clock.mark(3)) return rc;

  if (!p->weld) {
    if (int rc = copy_home(c, grid_out, grid.p, (size_t)L.nv * sizeof(float))) return rc;
    if (int rc = copy_home(c, vertices, soup.p, nsoup * 3 * sizeof(float))) return rc;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return clock.mark(5);
  }

  // 6. the weld
  const uint32_t ns = (uint32_t)nsoup;
  DevBuf sorted, first, head, newid, welded, didx, tmp;
  if (sorted.alloc(nsoup * 8) != hipSuccess || first.alloc(nsoup * 4) != hipSuccess || head.alloc(nsoup * 4) != hipSuccess ||
      newid.alloc(nsoup * 4) != hipSuccess || welded.alloc(nsoup * 3 * sizeof(float)) != hipSuccess || didx.alloc(nsoup * 4) != hipSuccess)
    return nomem();
  int key_bits = 1;
  while (key_bits < 32 && (3ull * nv) >> key_bits) ++key_bits;      // the bits an edge key 3 * vertex + axis can occupy
  size_t b_sort = 0, b_max = 0, b_sum = 0;
  MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, b_sort, wkeys.as<unsigned long long>(), sorted.as<unsigned long long>(), (int)ns, 0, 32 + key_bits,
                                                   c->stream));
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveScan(nullptr, b_max, head.as<uint32_t>(), head.as<uint32_t>(), hipcub::Max(), (int)ns, c->stream));
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, b_sum, first.as<uint32_t>(), newid.as<uint32_t>(), (int)ns, c->stream));
  if (tmp.alloc(std::max(b_sort, std::max(b_max, b_sum))) != hipSuccess) return nomem();
  size_t b = b_sort;
  MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(tmp.p, b, wkeys.as<unsigned long long>(), sorted.as<unsigned long long>(), (int)ns, 0, 32 + key_bits, c->stream));
  const dim3 sgrid(blocks_for(ns, kMcThreads));
  hipLaunchKernelGGL(mc_weld_mark_kernel, sgrid, block, 0, c->stream, sorted.as<unsigned long long>(), ns, first.as<uint32_t>(), head.as<uint32_t>());
  MVR_HIP_TRY(c, hipGetLastError());
  b = b_max;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveScan(tmp.p, b, head.as<uint32_t>(), head.as<uint32_t>(), hipcub::Max(), (int)ns, c->stream));
  b = b_sum;
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, b, first.as<uint32_t>(), newid.as<uint32_t>(), (int)ns, c->stream));
  hipLaunchKernelGGL(mc_weld_scatter_kernel, sgrid, block, 0, c->stream, sorted.as<unsigned long long>(), ns, head.as<uint32_t>(), newid.as<uint32_t>(),
                     soup.as<float>(), didx.as<uint32_t>(), welded.as<float>());
  MVR_HIP_TRY(c, hipGetLastError());
  uint32_t last_id = 0, last_first = 0;
  MVR_HIP_TRY(c, hipMemcpyAsync(&last_id, newid.as<uint32_t>() + (ns - 1u), 4, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipMemcpyAsync(&last_first, first.as<uint32_t>() + (ns - 1u), 4, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t nw = (size_t)last_id + last_first;
  if (int rc = clock.mark(4)) return rc;
  if (n_vertices) *n_vertices = nw;
  if (int rc = copy_home(c, grid_out, grid.p, (size_t)L.nv * sizeof(float))) return rc;
  if (int rc = copy_home(c, vertices, welded.p, nw * 3 * sizeof(float))) return rc;
  if (int rc = copy_home(c, indices, didx.p, nsoup * 4)) return rc;
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return clock.mark(5);
}
