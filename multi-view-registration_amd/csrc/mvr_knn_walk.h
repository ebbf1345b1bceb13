// csrc/mvr_knn_walk.h -- the walks of a cloud's model grid around a query, each written once, for the kernels that search a
// neighbourhood (mvr_knn.hip: k-NN lists and normals; mvr_outlier.hip: mean neighbour distances and neighbour counts;
// mvr_mls.hip: moving least squares; mvr_fpfh.hip: FPFH descriptors; mvr_feature.hip: the scores of posed copies;
// mvr_radius.hip: the radius lists themselves):
//   * knn_shell_walk: shells of cells outward from the query's cell until a visitor's k-best list is full and every unvisited
//     cell lies beyond it (the f64 bound of knn_unvisited_bound);
//   * knn_ball_walk: every point within a radius of the query, in grid order (knn_ball_any: the same ball, left at the first
//     point a predicate holds for).
// Around them the search side of a slot, the query of a thread, the cell lookup of the compact table, the row ranges, the
// library's f32 distance, and the host-side checks every caller makes; at the end what mvr_boundary.hip and mvr_iss.hip share (the
// boundary launch and the template of the ISS saliency kernel).  Not installed.
#pragma once

#include <limits>
#include <string>

#include "mvr_internal.h"
#include "mvr_plane.h"

namespace mvr {

struct KnnSlot {
  const float4 *qs;                // queries: grid order with w = bits(index) -- or, with q_by_pos, index order
  const float4 *gt;                // target points: grid order with w = bits(index) -- or, without a grid (dir null), index order
  const float4 *tpts;              // target points in index order (k-mode normals read the neighbours from here)
  const uint32_t *dir, *recs;      // compact cell starts of the target grid (CellGrid); dir null: one cell [0, nt)
  float4 *nrm;                     // normals out, by query index
  float *curv;                     // optional: curvature out, by query index
  uint32_t *oidx; float *od2;      // k-NN out: [nq][k] by query index
  float lo[3], inv_h;
  int dim[3];
  uint32_t nq, nt, q_by_pos, blk0;
};

constexpr int kKnnThreads = 256;   // the block of every kernel that takes its query with knn_query
constexpr uint32_t kSegOcc = 0x80000000u;
// the empty entry of a k-best list of (d2 bits << 32 | index) keys: d2 = +inf, index 0.  Every key with a FINITE d2 is below
// it, every key with d2 = +inf or NaN (either sign: the bits of a NaN are above those of +inf) is not -- so the one test
// `key < L[KMAX - 1]` of the candidate loop also keeps the non-finite target points out (mvr_hip.h: the non-finite rule).
constexpr nnkey_t kKnnKeyEmpty = 0x7F80000000000000ull;
// the ordered k-best list of such keys (ascending, the k-th entry last): insert `key` (which is below L[KMAX - 1]); every index is a compile-time constant
template <int KMAX>
__device__ __forceinline__ void knn_insert(nnkey_t (&L)[KMAX], const nnkey_t key)
{
#pragma unroll
  for (int i = KMAX - 1; i > 0; --i) L[i] = key < L[i - 1] ? L[i - 1] : (key < L[i] ? key : L[i]);
  L[0] = key < L[0] ? key : L[0];
}

// the query of this thread: by position in the slot's block range, its index from w in grid order; false: past the end
__device__ __forceinline__ bool knn_query(const KnnSlot &S, float4 *q, uint32_t *qi)
{
  const uint32_t pos = (blockIdx.x - S.blk0) * kKnnThreads + threadIdx.x;
  if (pos >= S.nq) return false;
  *q = S.qs[pos];
  *qi = S.q_by_pos ? pos : __float_as_uint(q->w);
  return true;
}
// the cell-start lookup of the compact table (the same encoding as cell_start_of in mvr_grid.hip)
__device__ __forceinline__ uint32_t knn_cell_start(const KnnSlot &S, uint32_t c)
{
  const uint32_t d = S.dir[c >> 5];
  return (d & kSegOcc) ? S.recs[((d & ~kSegOcc) << 5) + (c & 31u)] : d;
}
__device__ __forceinline__ int knn_cell_of(float x, float lo, float inv_h, int dim)
{
  // the grid build's own assignment (mvr_grid.hip: cell_of): monotone in x, clamped to the grid
  const float f = floorf((x - lo) * inv_h);
  return (int)fminf(fmaxf(f, 0.f), (float)(dim - 1));
}
template <bool FMA>
__device__ __forceinline__ float knn_dist2(const float4 t, const float4 q)
{
  const float dx = t.x - q.x, dy = t.y - q.y, dz = t.z - q.z;
  if (FMA) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  float r = dx * dx;
  r = r + dy * dy;
  r = r + dz * dz;
  return r;
}

// the grid positions where the cells [x0, x1] of row (y, z) begin and end (no grid: the one cell [0, nt))
__device__ __forceinline__ void knn_row_range(const KnnSlot &S, int x0, int x1, int y, int z, uint32_t *s, uint32_t *e)
{
  if (!S.dir) { *s = 0u; *e = S.nt; return; }
  const uint32_t c0 = (uint32_t)((z * S.dim[1] + y) * S.dim[0] + x0);
  *s = knn_cell_start(S, c0);
  *e = knn_cell_start(S, c0 + (uint32_t)(x1 - x0) + 1u);
}

// the nearest an unvisited cell can be once the box of cells [x0, x1] x [y0, y1] x [z0, z1] around the query is visited (lo_* /
// hi_*: the grid has cells beyond that side): the gap between the query and the box on those sides, in cells of the grid's own
// f32 inverse edge (f64), less a margin every rounding fits in -- the f32 cell assignment of a point (relative 2^-22 of its
// offset from lo, plus an ulp of the coordinate) and the f32 distance (the 1e-5 of d2 the callers take off): 1e-6 of the
// magnitudes involved is ten times that.  Squared and reduced by that 1e-5 it is compared with the k-th d2.
__device__ __forceinline__ double knn_unvisited_bound(const KnnSlot &S, const float4 q, int x0, int x1, int y0, int y1, int z0, int z1,
                                                      bool lo_x, bool hi_x, bool lo_y, bool hi_y, bool lo_z, bool hi_z)
{
  const double ih = (double)S.inv_h;
  const double ux = ((double)q.x - (double)S.lo[0]) * ih, uy = ((double)q.y - (double)S.lo[1]) * ih, uz = ((double)q.z - (double)S.lo[2]) * ih;
  double g = 1.0e300;
  if (lo_x) g = fmin(g, ux - (double)x0);
  if (hi_x) g = fmin(g, (double)(x1 + 1) - ux);
  if (lo_y) g = fmin(g, uy - (double)y0);
  if (hi_y) g = fmin(g, (double)(y1 + 1) - uy);
  if (lo_z) g = fmin(g, uz - (double)z0);
  if (hi_z) g = fmin(g, (double)(z1 + 1) - uz);
  const double mag = fabs((double)q.x) + fabs((double)q.y) + fabs((double)q.z) + fabs((double)S.lo[0]) + fabs((double)S.lo[1]) +
                     fabs((double)S.lo[2]) + (double)(S.dim[0] + S.dim[1] + S.dim[2]) / ih;
  return g / ih - (1.0e-6 * mag + 1.0e-6 / ih);
}

// the cells the ball of radius sqrt(r2) around q overlaps: the radius widened by the same margins as the bound above (f32 cell
// arithmetic is monotone); without a grid the one cell
__device__ __forceinline__ void knn_ball_cells(const KnnSlot &S, const float4 q, float r2, int *x0, int *x1, int *y0, int *y1, int *z0, int *z1)
{
  *x0 = *x1 = *y0 = *y1 = *z0 = *z1 = 0;
  if (!S.dir) return;
  const float mag = fabsf(q.x) + fabsf(q.y) + fabsf(q.z) + fabsf(S.lo[0]) + fabsf(S.lo[1]) + fabsf(S.lo[2]) +
                    (float)(S.dim[0] + S.dim[1] + S.dim[2]) / S.inv_h;
  const float rad = sqrtf(r2) * 1.0001f + 1.0e-5f * mag;
  *x0 = knn_cell_of(q.x - rad, S.lo[0], S.inv_h, S.dim[0]); *x1 = knn_cell_of(q.x + rad, S.lo[0], S.inv_h, S.dim[0]);
  *y0 = knn_cell_of(q.y - rad, S.lo[1], S.inv_h, S.dim[1]); *y1 = knn_cell_of(q.y + rad, S.lo[1], S.inv_h, S.dim[1]);
  *z0 = knn_cell_of(q.z - rad, S.lo[2], S.inv_h, S.dim[2]); *z1 = knn_cell_of(q.z + rad, S.lo[2], S.inv_h, S.dim[2]);
}

// the index of the target point p at grid position j (no grid: the points lie in index order)
__device__ __forceinline__ uint32_t knn_index_of(const KnnSlot &S, const float4 p, const uint32_t j) { return S.dir ? __float_as_uint(p.w) : j; }

// The shell walk: Chebyshev shells of cells outward from the query's cell (shell s = the cells at distance s), every point of
// a shell handed to the visitor as v.visit(p, j), j = the point's grid position (knn_index_of gives its index).  After a shell
// the walk ends when the whole grid is seen, or when the visitor's list is full -- v.full() -- and every unvisited cell lies
// beyond it: v.beyond(b2), b2 = the square of knn_unvisited_bound less 1e-5 of itself, in f64.  Whether "beyond" includes "at"
// is the visitor's rule (a tie that can still change the result must be visited).  A non-finite query or an empty target
// walks nothing.
template <class V>
__device__ __forceinline__ void knn_shell_walk(const KnnSlot &S, const float4 q, V &v)
{
  if (S.nt == 0 || !finite3(q)) return;
  const int cx = knn_cell_of(q.x, S.lo[0], S.inv_h, S.dim[0]), cy = knn_cell_of(q.y, S.lo[1], S.inv_h, S.dim[1]),
            cz = knn_cell_of(q.z, S.lo[2], S.inv_h, S.dim[2]);
  for (int s = 0;; ++s) {
    const int x0 = cx - s, x1 = cx + s, y0 = cy - s, y1 = cy + s, z0 = cz - s, z1 = cz + s;
    const int ya = max(y0, 0), yb = min(y1, S.dim[1] - 1), za = max(z0, 0), zb = min(z1, S.dim[2] - 1);
    // the shell's rows one after the other: on a face of the shell the whole row [x0, x1], inside it the row's two end cells
    // (ONE loop and one candidate loop: every copy of a visitor's unrolled insertion costs registers and code)
    for (int r = 0, nr = (yb - ya + 1) * (zb - za + 1) * 2; r < nr; ++r) {
      const int part = r & 1, y = ya + (r >> 1) % (yb - ya + 1), z = za + (r >> 1) / (yb - ya + 1);
      const bool face = z == z0 || z == z1 || y == y0 || y == y1;
      int a, b;
      if (face) {
        if (part) continue;
        a = max(x0, 0); b = min(x1, S.dim[0] - 1);
      } else {
        a = b = part ? x1 : x0;
        if (a < 0 || a >= S.dim[0]) continue;
      }
      uint32_t j, e;
      knn_row_range(S, a, b, y, z, &j, &e);
      for (; j < e; ++j) {
        v.visit(S.gt[j], j);
      }
    }
    if (!S.dir) return;                                               // one cell: all of it seen
    const bool lo_x = x0 > 0, hi_x = x1 < S.dim[0] - 1, lo_y = y0 > 0, hi_y = y1 < S.dim[1] - 1, lo_z = z0 > 0, hi_z = z1 < S.dim[2] - 1;
    if (!(lo_x || hi_x || lo_y || hi_y || lo_z || hi_z)) return;      // the whole grid seen
    if (!v.full()) continue;
    const double b = knn_unvisited_bound(S, q, x0, x1, y0, y1, z0, z1, lo_x, hi_x, lo_y, hi_y, lo_z, hi_z);
    if (b > 0.0 && v.beyond(b * b * (1.0 - 1.0e-5))) return;          // (a NaN on either side: never)
  }
}

// The ball walk: f(p, j) for every target point p (j = its grid position) with d2 <= r2 in the library's f32 distance, cell rows in
// z, y order and grid order within a row -- the same points in the same order every time it is called with the same
// arguments.  Against a finite r2 (clamp_r2) a non-finite p, with d2 = +inf or NaN, fails the test.  A non-finite query or
// an empty target walks nothing.
template <bool FMA, class F>
__device__ __forceinline__ void knn_ball_walk(const KnnSlot &S, const float4 q, const float r2, F &&f)
{
  if (S.nt == 0 || !finite3(q)) return;
  int x0, x1, y0, y1, z0, z1;
  knn_ball_cells(S, q, r2, &x0, &x1, &y0, &y1, &z0, &z1);
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      uint32_t j, e;
      knn_row_range(S, x0, x1, y, z, &j, &e);
      for (; j < e; ++j) {
        const float4 p = S.gt[j];
        if (knn_dist2<FMA>(p, q) <= r2) f(p, j);
      }
    }
}

// The same ball, asked a question: whether pred(p, j) holds for any point of it.  It ends at the first that does.
template <bool FMA, class P>
__device__ __forceinline__ bool knn_ball_any(const KnnSlot &S, const float4 q, const float r2, P &&pred)
{
  if (S.nt == 0 || !finite3(q)) return false;
  int x0, x1, y0, y1, z0, z1;
  knn_ball_cells(S, q, r2, &x0, &x1, &y0, &y1, &z0, &z1);
  for (int z = z0; z <= z1; ++z)
    for (int y = y0; y <= y1; ++y) {
      uint32_t j, e;
      knn_row_range(S, x0, x1, y, z, &j, &e);
      for (; j < e; ++j) {
        const float4 p = S.gt[j];
        if (knn_dist2<FMA>(p, q) <= r2 && pred(p, j)) return true;
      }
    }
  return false;
}

// ---- the host side
// (float)(radius * radius), kept finite: a d2 of +inf -- a non-finite neighbour, or an f32 overflow -- is never <= r2
inline float clamp_r2(double radius) { return (float)std::min(radius * radius, (double)std::numeric_limits<float>::max()); }

// what every entry point checks of a cloud before it walks it (`fn`: its name for the error text): indices fit the 31 bits the
// walks and their callers leave them, and pts[] are what the cloud holds (a pipelined run leaves them out: Cloud::pts_stale)
inline int knn_cloud_ok(Ctx *c, const Cloud &cl, const char *fn)
{
  if (cl.n > 0x7FFFFFF0ull) return set_error(c, MVR_E_ARG, (std::string(fn) + ": cloud too large").c_str());
  if (cl.pts_stale) return set_error(c, MVR_E_ARG, (std::string(fn) + ": the cloud's points are not current (pipelined run)").c_str());
  return MVR_OK;
}

inline int kmax_bucket(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }

// the search side of a slot (a cloud that passed knn_cloud_ok): its grid over the current coordinates when it can have one,
// else one cell over the points
inline int fill_target(Ctx *c, Cloud &t, KnnSlot &S)
{
  S.gt = t.pts; S.tpts = t.pts; S.dir = nullptr; S.recs = nullptr; S.nt = (uint32_t)t.n;
  for (int j = 0; j < 3; ++j) { S.lo[j] = 0.f; S.dim[j] = 1; }
  S.inv_h = 0.f;
  if (t.n == 0) return MVR_OK;
  bool ok = false;
  bool no_finite = false;
  if (int rc = ensure_model_grid(c, t, &ok, &no_finite)) return rc;
  if (no_finite) S.nt = 0;            // nobody's neighbour, all of them: an empty target (no query scans it)
  if (!ok) return MVR_OK;
  const CellGrid &g = *t.mgrid;
  S.gt = g.graw; S.dir = g.dir; S.recs = g.recs; S.inv_h = g.inv_h;
  for (int j = 0; j < 3; ++j) { S.lo[j] = g.lo[j]; S.dim[j] = g.dim[j]; }
  return MVR_OK;
}
// the query side: grid order when the cloud has a grid (the lanes of a wave are then neighbours), else index order
inline void fill_queries(const Cloud &q, KnnSlot &S)
{
  const bool grid = q.mgrid && q.mgrid_ok && q.mgrid->n == q.n && q.n > 0;
  S.qs = grid ? q.mgrid->graw : q.pts;
  S.q_by_pos = grid ? 0u : 1u;
  S.nq = (uint32_t)q.n;
}

// the k-NN lists of a cloud (n > 0, past knn_cloud_ok) in itself into device tables [n][k] by index (mvr_knn.hip); queued
int knn_self_device(Ctx *c, Cloud &cl, int k, bool fma, uint32_t *didx, float *dd2);
// the same for queries that are not the target's own points: the lists of S.qs in S's target into S.oidx / S.od2, [nq][k] by
// the query's index (w of the query, or its position with q_by_pos); queued
int knn_device(Ctx *c, const KnnSlot &S, int k, bool fma);

// ---- the query side of the entries that answer chosen queries over a search surface (mvr_at.hip; mvr_cloud_estimate_normals_at,
// mvr_cloud_fpfh_at, mvr_cloud_pfh_at; rules Q1-Q8 in mvr_hip.h).  A query is a position and the output row it answers: q[r] =
// {x, y, z, bits of the row}, so every walk kernel takes it as it takes a point of a grid (KnnSlot::qs with q_by_pos = 0).
// A query that is invalid under Q2 gets NaN coordinates: it walks nothing, and every entry gives an invalid query the row of
// an empty neighbourhood.  The rows are sorted by the cell of the SURFACE's grid the query falls in (one hipCUB pair sort; tune
// key "at_sort" = 0 leaves it out), so the lanes of a wave, or consecutive waves, walk the same cells.  The order changes no
// result: every row is written by its own number.
struct AtQueries {
  DevBuf buf;
  const float4 *q = nullptr;
  size_t rows = 0;
};
// Q1's refusal (an index >= n_q), on the host, before any GPU work
int at_indices_ok(Ctx *c, const Cloud &q, const uint32_t *indices, size_t n_indices, const char *fn);
// indices: host, or null for every point of q.  with_normals: Q2's same-slot case (a query with a non-finite normal is invalid).
// S: the surface (fill_target).  `indices` is copied before the call returns; the kernels are queued on the context's stream.
int at_queries(Ctx *c, const Cloud &q, bool with_normals, const uint32_t *indices, size_t n_indices, const KnnSlot &S, AtQueries *out);
// the marking walk: S = the query array over the surface, gn = the surface's normals in the order of S.gt with the validity mark in
// w; count[row] = the query's valid neighbours, need[j] = 1 at the grid position of each (need: S.nt bytes, cleared by the caller)
int launch_at_mark(Ctx *c, const KnnSlot &S, const float4 *gn, float r2, bool fma, uint32_t *count, uint8_t *need);

// the radius lists of the points of q in t (both past knn_cloud_ok; rules RS1-RS11 at mvr_radius_search in mvr_hip.h) as CSR
// tables that stay on the device (mvr_radius.hip): offsets[nq + 1] by query index, idx / d2 [total].  The tables belong to the
// struct (pool allocations, freed with it); the work is queued on the context's stream, which the call waits for once, to
// read `total`.
struct RadiusLists {
  unsigned long long *offsets = nullptr;
  uint32_t *idx = nullptr;
  float *d2 = nullptr;
  size_t nq = 0, total = 0;
  bool counted = false;              // offsets and total are valid (also when the call then refused: RS7, RS8)
  RadiusLists() = default;
  RadiusLists(const RadiusLists &) = delete;
  RadiusLists &operator=(const RadiusLists &) = delete;
  ~RadiusLists();
};
// fill false: the count alone (offsets, total).  capacity: the entries the caller has room for (RS7; SIZE_MAX: no limit)
int radius_search_device(Ctx *c, Cloud &q, Cloud &t, const mvr_radius_params &p, bool fill, size_t capacity, RadiusLists *out);

// pcl::BoundaryEstimation over a filled slot (mvr_boundary.hip; rules B1-B5 at mvr_cloud_boundary in mvr_hip.h), queued on the
// context's stream: flag / max_gap / count by index, flag_grid by the query's grid position (the position a later walk of the
// same slot finds the point at); each of the four may be null.  nrm: the cloud's normals, by index.
int launch_boundary(Ctx *c, const KnnSlot &S, const float4 *nrm, float r2, float angle_threshold, uint32_t min_neighbors, bool fma,
                    uint8_t *flag, uint8_t *flag_grid, float *max_gap, uint32_t *count);
bool boundary_angle_ok(double angle_threshold);      // B6: [MVR_BOUNDARY_MIN_ANGLE, 2 pi)

// ---- the saliency kernel of pcl::ISSKeypoint3D (rules K3, K4 and K9-K11 at mvr_cloud_iss_keypoints in mvr_hip.h) and the
// arguments of the detector's kernels.  It is a template of two parameters that two files instantiate -- mvr_iss.hip the
// detector without a border, mvr_boundary.hip the one that first looks for an edge point within the border radius -- and it
// stands in this header, which every object is rebuilt after, so that the two can never disagree about IssArgs.
constexpr int kIssThreads = kKnnThreads;

struct IssArgs {
  KnnSlot S;                       // the cloud searched against itself (nrm / curv / oidx / od2 unused; blk0 = 0)
  double *sal_grid;                // saliency by grid position
  double *sal;                     // saliency by index
  uint32_t *salient_count;         // by index
  uint32_t *nms_count;             // by index
  uint8_t *flag;                   // by index: a keypoint
  double gamma_21, gamma_32;
  uint32_t min_neighbors;
  float r2_salient, r2_nms;
  // the BORDER instantiation only
  const uint8_t *edge_grid;        // K9's flags by grid position
  uint8_t *border;                 // K10's flags by index
  float r2_border;
};

template <bool FMA, bool BORDER>
__global__ void __launch_bounds__(kIssThreads) iss_saliency_kernel(IssArgs a)
{
  const KnnSlot &S = a.S;
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  const uint32_t pos = blockIdx.x * kIssThreads + threadIdx.x;
  if constexpr (BORDER) {
    const bool border = knn_ball_any<FMA>(S, q, a.r2_border, [&](const float4, const uint32_t j) { return a.edge_grid[j] != 0; });
    a.border[qi] = border ? 1 : 0;
    if (border) {      // K11
      a.sal_grid[pos] = 0.0;
      a.sal[qi] = 0.0;
      a.salient_count[qi] = 0u;
      return;
    }
  }
  Moments M;      // (a non-finite query walks nothing: K1)
  uint32_t n = 0;
  knn_ball_walk<FMA>(S, q, a.r2_salient, [&](const float4 p, uint32_t) { M.add(p, q); ++n; });
  double s = 0.0;
  if (n >= a.min_neighbors) {
    const Eigenvalues3 e = scatter_eigenvalues(M);
    const bool finite = isfinite(e.e1) && isfinite(e.e2) && isfinite(e.e3);
    // K4 (a NaN ratio, 0 / 0 included, fails its test)
    if (finite && e.e3 >= 0.0 && e.e2 / e.e1 < a.gamma_21 && e.e3 / e.e2 < a.gamma_32 && e.e3 > 0.0) s = e.e3;
  }
  a.sal_grid[pos] = s;
  a.sal[qi] = s;
  a.salient_count[qi] = n;
}

// the BORDER instantiations (mvr_boundary.hip), over n = a.S.nq queries, queued on the context's stream
int launch_iss_saliency_border(Ctx *c, const IssArgs &a, bool fma);

}  // namespace mvr
