// csrc/mvr_knn.hip -- exact k-nearest-neighbour search and PCL-style normal estimation (gfx950).
//
// pcl::NormalEstimation (computePointNormal / solvePlaneParameters / flipNormalTowardsViewpoint) is a neighbour search per
// point plus a 3 x 3 symmetric eigenproblem.  Both run here, one thread per query:
//
//   * grid: the uniform grid of a cloud over its OWN current coordinates (ensure_model_grid, mvr_grid.hip: compact cell
//     starts, points in grid order with w = bits of the point's index).  The queries are taken in that grid order too, so
//     the 64 lanes of a wave are neighbours on the surface and walk the same cells; results are scattered back by index.
//     A cloud too small for a grid (n < 4) or without one (a shard) is searched as ONE cell over its points in index order.
//   * k-NN walk (knn_shell_walk, mvr_knn_walk.h): shells of cells outward from the query's cell (Chebyshev shell s = the cells at distance s).  The walk
//     stops when the list is full and every unvisited cell lies beyond the current k-th distance -- the gap between the
//     query and the visited box, taken in f64 in cell units of the grid's own f32 inverse edge, minus a margin that covers
//     every rounding of the cell assignment and of the f32 distance.  A cell at exactly that distance is
//     still visited: a candidate that ties the k-th d2 with a lower index must get in.  Exact, never approximate.
//   * the k-best list: KMAX 64-bit keys (d2 bits << 32 | index: unsigned order = (d2, index) lexicographic) in registers,
//     inserted with compile-time indices only (a runtime-indexed private array would live in scratch).  For k < KMAX the
//     leading KMAX - k entries hold the key 0, which no insertion moves: the live list is always the TAIL, its k-th entry
//     the last register.
//   * normals, k mode: the list is finished first, then the neighbours' coordinates are read again (their lines are in
//     L1 / L2 from the walk) into f64 moments about the query point; radius mode accumulates the moments while it walks.
//   * 3 x 3 solve: cyclic Jacobi in f64 (a few sweeps reach the f64 rounding level on a 3 x 3), normal = eigenvector of the
//     smallest eigenvalue, curvature = |l0| / (l0 + l1 + l2); the normal is rounded to f32 and flipped towards the viewpoint
//     with PCL's f32 test (cos < 0 strictly).
// Every slot of a call is served by one launch (concatenated query ranges, the block knows its slot); the neighbour lists of
// the normals path never leave registers.  Compiled with -ffp-contract=off (the distance is the library's f32 expression).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_plane.h"

namespace mvr {
namespace {

constexpr int kKnnSlots = 16;      // slots per launch (kernel argument by value)

struct KnnBatch {
  KnnSlot s[kKnnSlots];
  int n_slots, k;
  float r2;                        // radius mode: (float)(radius * radius)
  float vp[3];
};
static_assert(sizeof(KnnBatch) <= 4096, "KnnBatch travels as a kernel argument");

// the slot of this block (uniform: a slot's blocks are consecutive)
__device__ __forceinline__ int knn_slot_of(const KnnBatch &b)
{
  int si = 0;
  for (int j = 1; j < b.n_slots; ++j)
    if (blockIdx.x >= b.s[j].blk0) si = j;
  return si;
}

// the visitor of the shell walk that keeps the exact k-best list of query q: KMAX - k leading zero keys, then the k best
// (kKnnKeyEmpty where the target has fewer FINITE points within a finite f32 d2; a non-finite query has none)
template <int KMAX, bool FMA>
struct KnnList {
  nnkey_t (&L)[KMAX];
  const KnnSlot &S;
  const float4 q;
  __device__ __forceinline__ void visit(const float4 p, const uint32_t j)
  {
    const nnkey_t key = ((nnkey_t)__float_as_uint(knn_dist2<FMA>(p, q)) << 32) | knn_index_of(S, p, j);
    if (key < L[KMAX - 1]) knn_insert<KMAX>(L, key);
  }
  __device__ __forceinline__ bool full() const { return L[KMAX - 1] != kKnnKeyEmpty; }
  // strictly beyond the k-th distance: a cell AT it is still visited, since a candidate that ties the k-th d2 with a lower
  // index must get in
  __device__ __forceinline__ bool beyond(const double b2) const { return b2 > (double)__uint_as_float((uint32_t)(L[KMAX - 1] >> 32)); }
};

template <int KMAX, bool FMA>
__device__ __forceinline__ void knn_walk(const KnnSlot &S, const float4 q, const int k, nnkey_t (&L)[KMAX])
{
#pragma unroll
  for (int i = 0; i < KMAX; ++i) L[i] = i < KMAX - k ? 0ull : kKnnKeyEmpty;
  KnnList<KMAX, FMA> v{L, S, q};
  knn_shell_walk(S, q, v);
}

// moments about the query point -> unit normal (f32, oriented) and curvature; fewer than 3 neighbours: NaN
__device__ __forceinline__ void plane_from_moments(const KnnSlot &S, const KnnBatch &b, const float4 q, const uint32_t qi, const Moments &M)
{
  float4 out; float curv;
  if (M.cnt < 3.0) {
    out = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.f);
    curv = __builtin_nanf("");
  } else {
    const PlaneFit f = plane_fit(M);      // (mvr_plane.h: f64 covariance, cyclic Jacobi, the smallest eigenvalue's eigenvector)
    curv = plane_curvature(f);
    out = plane_normal_towards((float)f.nx, (float)f.ny, (float)f.nz, b.vp[0] - q.x, b.vp[1] - q.y, b.vp[2] - q.z);
  }
  S.nrm[qi] = out;
  if (S.curv) S.curv[qi] = curv;
}

// k-NN lists out to memory
template <int KMAX, bool FMA>
__global__ void __launch_bounds__(kKnnThreads) knn_kernel(KnnBatch b)
{
  const KnnSlot &S = b.s[knn_slot_of(b)];
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  nnkey_t L[KMAX];
  knn_walk<KMAX, FMA>(S, q, b.k, L);
  uint32_t *oi = S.oidx + (size_t)qi * b.k;
  float *od = S.od2 + (size_t)qi * b.k;
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    if (i >= KMAX - b.k) {
      const bool none = L[i] == kKnnKeyEmpty;
      oi[i - (KMAX - b.k)] = none ? kNone : (uint32_t)L[i];
      od[i - (KMAX - b.k)] = __uint_as_float((uint32_t)(L[i] >> 32));      // (the empty key carries +inf)
    }
  }
}

// normals, k mode: the list in registers, then the moments of its entries
template <int KMAX, bool FMA>
__global__ void __launch_bounds__(kKnnThreads) normals_knn_kernel(KnnBatch b)
{
  const KnnSlot &S = b.s[knn_slot_of(b)];
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  nnkey_t L[KMAX];
  knn_walk<KMAX, FMA>(S, q, b.k, L);
  Moments M;
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    if (i >= KMAX - b.k && L[i] != kKnnKeyEmpty) M.add(S.tpts[(uint32_t)L[i]], q);
  }
  plane_from_moments(S, b, q, qi, M);
}

// normals, radius mode: every point with d2 <= r2, moments accumulated during the walk (no list)
template <bool FMA>
__global__ void __launch_bounds__(kKnnThreads) normals_radius_kernel(KnnBatch b)
{
  const KnnSlot &S = b.s[knn_slot_of(b)];
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  Moments M;      // (a non-finite query walks nothing: no neighbours, a NaN normal)
  knn_ball_walk<FMA>(S, q, b.r2, [&](const float4 p, uint32_t) { M.add(p, q); });
  plane_from_moments(S, b, q, qi, M);
}

template <bool FMA>
void launch_knn_fma(int kmax, int mode, dim3 grid, hipStream_t st, const KnnBatch &b)
{
  // mode 0: k-NN lists, 1: normals k mode, 2: normals radius mode
  if (mode == 2) { hipLaunchKernelGGL(normals_radius_kernel<FMA>, grid, dim3(kKnnThreads), 0, st, b); return; }
  switch (kmax) {
    case 8:  if (mode == 0) hipLaunchKernelGGL((knn_kernel<8, FMA>), grid, dim3(kKnnThreads), 0, st, b); else hipLaunchKernelGGL((normals_knn_kernel<8, FMA>), grid, dim3(kKnnThreads), 0, st, b); break;
    case 16: if (mode == 0) hipLaunchKernelGGL((knn_kernel<16, FMA>), grid, dim3(kKnnThreads), 0, st, b); else hipLaunchKernelGGL((normals_knn_kernel<16, FMA>), grid, dim3(kKnnThreads), 0, st, b); break;
    case 32: if (mode == 0) hipLaunchKernelGGL((knn_kernel<32, FMA>), grid, dim3(kKnnThreads), 0, st, b); else hipLaunchKernelGGL((normals_knn_kernel<32, FMA>), grid, dim3(kKnnThreads), 0, st, b); break;
    default: if (mode == 0) hipLaunchKernelGGL((knn_kernel<64, FMA>), grid, dim3(kKnnThreads), 0, st, b); else hipLaunchKernelGGL((normals_knn_kernel<64, FMA>), grid, dim3(kKnnThreads), 0, st, b); break;
  }
}

int run_batches(Ctx *c, std::vector<KnnSlot> &all, KnnBatch proto, int kmax, int mode, bool fma)
{
  for (size_t b0 = 0; b0 < all.size(); b0 += kKnnSlots) {
    KnnBatch b = proto;
    b.n_slots = (int)std::min<size_t>(kKnnSlots, all.size() - b0);
    unsigned blocks = 0;
    for (int j = 0; j < b.n_slots; ++j) {
      b.s[j] = all[b0 + (size_t)j];
      b.s[j].blk0 = blocks;
      blocks += (b.s[j].nq + kKnnThreads - 1) / kKnnThreads;
    }
    if (!blocks) continue;
    if (fma) launch_knn_fma<true>(kmax, mode, dim3(blocks), c->stream, b);
    else launch_knn_fma<false>(kmax, mode, dim3(blocks), c->stream, b);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  return MVR_OK;
}

}  // namespace

int knn_device(Ctx *c, const KnnSlot &S, int k, bool fma)
{
  std::vector<KnnSlot> all{S};
  KnnBatch proto{};
  proto.k = k;
  return run_batches(c, all, proto, kmax_bucket(k), 0, fma);
}

// the k-NN lists of a cloud (n > 0, past knn_cloud_ok) in itself -- what mvr_knn gives for q_slot == t_slot -- into the device
// tables didx / dd2, [n][k] by index; queued on the context's stream (mvr_pfh.hip: the k-neighbour mode)
int knn_self_device(Ctx *c, Cloud &cl, int k, bool fma, uint32_t *didx, float *dd2)
{
  KnnSlot S{};
  if (int rc = fill_target(c, cl, S)) return rc;
  fill_queries(cl, S);
  S.oidx = didx; S.od2 = dd2;
  std::vector<KnnSlot> all{S};
  KnnBatch proto{};
  proto.k = k;
  return run_batches(c, all, proto, kmax_bucket(k), 0, fma);
}

}  // namespace mvr

using namespace mvr;

API int mvr_knn(mvr_ctx *ctx, int qs, int ts, int k, int fma, uint32_t *idx, float *d2)
{
  if (!ctx || !slot_ok(qs) || !slot_ok(ts) || k < 1 || k > MVR_MAX_KNN) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[qs], &t = c->slots[ts];
  if (q.n == 0) return MVR_OK;
  if (int rc = knn_cloud_ok(c, q, "mvr_knn")) return rc;
  if (int rc = knn_cloud_ok(c, t, "mvr_knn")) return rc;
  KnnSlot S{};
  if (int rc = fill_target(c, t, S)) return rc;
  if (qs != ts && q.n >= 4) {      // the queries' own grid gives them their walking order
    bool ok = false;
    if (int rc = ensure_model_grid(c, q, &ok)) return rc;
  }
  fill_queries(q, S);
  const size_t m = q.n * (size_t)k;
  uint32_t *didx = nullptr; float *dd2 = nullptr;
  MVR_HIP_TRY(c, hipMalloc(&didx, m * 4));
  if (hipMalloc(&dd2, m * 4) != hipSuccess) { (void)hipFree(didx); return set_error(c, MVR_E_NOMEM, "mvr_knn: out of device memory"); }
  S.oidx = didx; S.od2 = dd2;
  std::vector<KnnSlot> all{S};
  KnnBatch proto{};
  proto.k = k;
  int rc = run_batches(c, all, proto, kmax_bucket(k), 0, fma != 0);
  hipError_t e = hipSuccess;
  if (!rc && idx) e = hipMemcpyAsync(idx, didx, m * 4, hipMemcpyDeviceToHost, c->stream);
  if (!rc && e == hipSuccess && d2) e = hipMemcpyAsync(d2, dd2, m * 4, hipMemcpyDeviceToHost, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  (void)hipFree(didx); (void)hipFree(dd2);
  if (rc) return rc;
  if (e != hipSuccess) return set_error(c, MVR_E_HIP, "mvr_knn copy", e);
  if (e2 != hipSuccess) return set_error(c, MVR_E_HIP, "mvr_knn sync", e2);
  return MVR_OK;
}

API int mvr_cloud_estimate_normals(mvr_ctx *ctx, int count, const int *slots, const mvr_normal_params *p, float *const *curvature)
{
  if (!ctx || !slots || !p || count < 0) return MVR_E_ARG;
  const bool kmode = p->k != 0, rmode = p->radius != 0.0;
  if (kmode == rmode || p->k < 0 || p->k > MVR_MAX_KNN || !(p->radius >= 0.0) || std::isinf(p->radius)) return MVR_E_ARG;
  for (int j = 0; j < 3; ++j) if (!std::isfinite(p->viewpoint[j])) return MVR_E_ARG;
  for (int i = 0; i < count; ++i) {
    if (!slot_ok(slots[i])) return MVR_E_ARG;
    for (int j = 0; j < i; ++j) if (slots[j] == slots[i]) return MVR_E_ARG;
  }
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  std::vector<KnnSlot> all;
  std::vector<int> used;
  size_t curv_total = 0;
  for (int i = 0; i < count; ++i) {
    Cloud &cl = c->slots[slots[i]];
    if (cl.n == 0) continue;
    if (int rc = knn_cloud_ok(c, cl, "mvr_cloud_estimate_normals")) return rc;
    KnnSlot S{};
    if (int rc = fill_target(c, cl, S)) return rc;
    fill_queries(cl, S);
    if (curvature && curvature[i]) curv_total += cl.n;
    all.push_back(S); used.push_back(i);
  }
  if (all.empty()) return MVR_OK;
  // normal buffers (after every grid is built: ensure() may wait for the stream)
  for (size_t j = 0; j < all.size(); ++j) {
    Cloud &cl = c->slots[slots[used[j]]];
    cl.has_normals = false;
    if (int rc = ensure(c, cl.nrm, cl.nrm_cap, cl.n)) return rc;
    all[j].nrm = cl.nrm;
  }
  float *dcurv = nullptr;
  if (curv_total) MVR_HIP_TRY(c, hipMalloc(&dcurv, curv_total * 4));
  size_t off = 0;
  for (size_t j = 0; j < all.size(); ++j)
    if (curvature && curvature[used[j]]) { all[j].curv = dcurv + off; off += all[j].nq; }
  KnnBatch proto{};
  proto.k = p->k;
  proto.r2 = clamp_r2(p->radius);
  for (int j = 0; j < 3; ++j) proto.vp[j] = p->viewpoint[j];
  int rc = run_batches(c, all, proto, kmode ? kmax_bucket(p->k) : 8, kmode ? 1 : 2, p->fma_dist != 0);
  hipError_t e = hipSuccess;
  for (size_t j = 0; j < all.size() && !rc && e == hipSuccess; ++j)
    if (all[j].curv) e = hipMemcpyAsync(curvature[used[j]], all[j].curv, (size_t)all[j].nq * 4, hipMemcpyDeviceToHost, c->stream);
  const hipError_t e2 = hipStreamSynchronize(c->stream);
  if (dcurv) (void)hipFree(dcurv);
  if (rc) return rc;
  if (e != hipSuccess) return set_error(c, MVR_E_HIP, "mvr_cloud_estimate_normals copy", e);
  if (e2 != hipSuccess) return set_error(c, MVR_E_HIP, "mvr_cloud_estimate_normals sync", e2);
  for (size_t j = 0; j < all.size(); ++j) c->slots[slots[used[j]]].has_normals = true;
  return MVR_OK;
}

API int mvr_cloud_estimate_normals_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot,
                                      const mvr_normal_params *p, int store_in_slot, float *normals, float *curvature)
{
  if (!ctx || !p || !slot_ok(q_slot) || !slot_ok(surface_slot)) return MVR_E_ARG;
  const bool kmode = p->k != 0, rmode = p->radius != 0.0;
  if (kmode == rmode || p->k < 0 || p->k > MVR_MAX_KNN || !(p->radius >= 0.0) || std::isinf(p->radius)) return MVR_E_ARG;
  for (int j = 0; j < 3; ++j) if (!std::isfinite(p->viewpoint[j])) return MVR_E_ARG;
  if (store_in_slot && indices) return MVR_E_ARG;      // Q6
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[q_slot], &t = c->slots[surface_slot];
  if (int rc = knn_cloud_ok(c, q, "mvr_cloud_estimate_normals_at")) return rc;
  if (int rc = knn_cloud_ok(c, t, "mvr_cloud_estimate_normals_at")) return rc;
  if (int rc = at_indices_ok(c, q, indices, n_indices, "mvr_cloud_estimate_normals_at")) return rc;
  const size_t rows = indices ? n_indices : q.n;
  if (rows == 0) return MVR_OK;
  if (store_in_slot && q_slot == surface_slot) {      // Q8: the slot against itself, into the slot
    float *const cv[1] = {curvature};
    if (int rc = mvr_cloud_estimate_normals(ctx, 1, &q_slot, p, cv)) return rc;
    if (normals) MVR_HIP_TRY(c, hipMemcpy(normals, q.nrm, rows * sizeof(float4), hipMemcpyDeviceToHost));
    return MVR_OK;
  }
  KnnSlot S{};
  if (int rc = fill_target(c, t, S)) return rc;
  AtQueries Q;
  if (int rc = at_queries(c, q, false, indices, n_indices, S, &Q)) return rc;
  S.qs = Q.q; S.q_by_pos = 0u; S.nq = (uint32_t)rows;
  DevBuf out;
  if (out.alloc(rows * (sizeof(float4) + sizeof(float))) != hipSuccess) return set_error(c, MVR_E_NOMEM, "mvr_cloud_estimate_normals_at: out of device memory");
  S.curv = reinterpret_cast<float *>(out.as<float4>() + rows);
  S.nrm = out.as<float4>();
  if (store_in_slot) {
    q.has_normals = false;
    if (int rc = ensure(c, q.nrm, q.nrm_cap, q.n)) return rc;
    S.nrm = q.nrm;
  }
  std::vector<KnnSlot> all{S};
  KnnBatch proto{};
  proto.k = p->k;
  proto.r2 = clamp_r2(p->radius);
  for (int j = 0; j < 3; ++j) proto.vp[j] = p->viewpoint[j];
  if (int rc = run_batches(c, all, proto, kmode ? kmax_bucket(p->k) : 8, kmode ? 1 : 2, p->fma_dist != 0)) return rc;
  if (normals) MVR_HIP_TRY(c, hipMemcpyAsync(normals, S.nrm, rows * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (curvature) MVR_HIP_TRY(c, hipMemcpyAsync(curvature, S.curv, rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (store_in_slot) q.has_normals = true;
  return MVR_OK;
}
