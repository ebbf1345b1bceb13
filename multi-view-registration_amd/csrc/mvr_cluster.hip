// csrc/mvr_cluster.hip -- pcl::EuclideanClusterExtraction and extractEuclideanClusters with normals on the GPU (gfx950); the
// rules E1-E8 are written next to mvr_cloud_euclidean_clusters in mvr_hip.h.
//
// The clusters are the connected components of the link graph (E2, E3) over the active points (E1), so no flood fill is run:
//   1. active flags from the caller's index list (or all ones);
//   2. the link kernel, one thread per query in the order of the cloud's own model grid (ensure_model_grid; knn_query,
//      knn_ball_walk of mvr_knn_walk.h -- the lanes of a wave are spatial neighbours): every neighbour within the tolerance
//      whose original index is BELOW the query's (each pair once) and that passes the link rule is united with the query in
//      the lock-free union-find of mvr_union_find.h, on original indices.  The larger root goes under the smaller, so the root
//      of a finished component is its smallest member.  A thread keeps the last root it found for its query and compares the
//      two roots before it pays for a CAS: most of a wave belongs to one component and most pairs are already joined.  The
//      link rule is a template parameter: plain, or with the normals' dot product (E3);
//   3. pointer jumping, then labels (to their own array), component sizes (a wave's lanes that share a root add once) and
//      the counts of active points and components;
//   4. the components that are clusters (E5) get a 64-bit key (~size << 32 | root), everything else ~0: one radix sort ranks
//      them by size descending, root ascending (E6); a second 64-bit sort of (rank << 32 | index) over the clustered points
//      gives the concatenated member lists, and the places where the rank changes are the offsets (E7);
//   5. counters first, then offsets, lists and labels go home; with a dst slot the points of the first `keep` clusters are
//      selected in ascending index (select_flagged) and gathered (gather_kept).
// Integer atomics only: the result does not depend on the order of the unions, on the grid or on the launch shape.  Scratch
// arrays come out of the context's arena (Ctx::dn_arena).  HBM/latency-bound integer work; nothing here is a GEMM.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_union_find.h"

namespace mvr {
namespace {

constexpr int kClThreads = kKnnThreads;
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;
constexpr unsigned long long kNoKey = ~0ull;
// the device counters, in the order of mvr_cluster_result (one copy fills it), then the size of dst's selection
enum { kCntActive = 0, kCntComponents, kCntClusters, kCntClustered, kCntLargest, kCntTooSmall, kCntTooLarge, kCntKept, kCntWords };

struct ClusterArgs {
  KnnSlot S;                       // the cloud searched against itself (nrm / curv / oidx / od2 unused; blk0 = 0)
  const float4 *nrm;               // NORMALS: the slot's normals, by index
  const uint8_t *active;           // by index (E1)
  uint32_t *parent;                // by index
  float r2;
  double cos_eps;
};

__global__ void __launch_bounds__(kClThreads) cl_iota_kernel(uint32_t *__restrict__ v, size_t n)
{
  const size_t i = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// E3: the f64 dot of the two f32 normals, in this order of operations; a NaN fails the test
__device__ __forceinline__ bool cl_normals_link(const float4 a, const float4 b, const double cos_eps)
{
  const double dot = ((double)a.x * (double)b.x + (double)a.y * (double)b.y) + (double)a.z * (double)b.z;
  return dot > cos_eps;
}

template <bool FMA, bool NORMALS>
__global__ void __launch_bounds__(kClThreads) cl_link_kernel(ClusterArgs a)
{
  float4 q; uint32_t qi;
  if (!knn_query(a.S, &q, &qi)) return;
  if (!a.active[qi]) return;
  float4 nq = make_float4(0.f, 0.f, 0.f, 0.f);
  if (NORMALS) nq = a.nrm[qi];
  uint32_t rq = qi;                // a member of the query's component: the root the last find gave
  // (a non-finite query walks nothing, and against the finite r2 a non-finite neighbour fails the walk's test: E4)
  knn_ball_walk<FMA>(a.S, q, a.r2, [&](const float4 p, const uint32_t j) {
    const uint32_t pi = knn_index_of(a.S, p, j);
    if (pi >= qi || !a.active[pi]) return;          // every pair once, from its larger index
    if (NORMALS && !cl_normals_link(nq, a.nrm[pi], a.cos_eps)) return;
    rq = uf_find(a.parent, rq);
    const uint32_t rp = uf_find(a.parent, pi);
    if (rq == rp) return;                           // joined already: no CAS
    uf_unite(a.parent, rq, rp);
    rq = rq < rp ? rq : rp;                         // a member of the joined component: the next find starts here
  });
}

__global__ void __launch_bounds__(kClThreads) cl_jump_kernel(uint32_t *__restrict__ parent, size_t n)
{
  const size_t i = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i < n) uf_jump(parent, i);
}

// label[i] = the root of an active point (kNoLabel for an inactive one), size[root], the counts of active points and components
__global__ void __launch_bounds__(kClThreads) cl_label_kernel(uint32_t *__restrict__ parent, const uint8_t *__restrict__ active, size_t n,
                                                              uint32_t *__restrict__ label, uint32_t *__restrict__ size, uint32_t *__restrict__ counters)
{
  const size_t i = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  const bool live = i < n && active[i] != 0;
  uint32_t r = 0;
  if (live) {
    r = uf_find(parent, (uint32_t)i);
    // The label goes to its OWN array: other threads' finds are still halving paths through node i, and one of them could
    // store a non-root ancestor into parent[i] after a root written there.  Roots are final here (no unions run).
    label[i] = r;
    if (r == (uint32_t)i) atomicAdd(&counters[kCntComponents], 1u);
  } else if (i < n) {
    label[i] = kNoLabel;
  }
  // the lanes of a wave that share a root add once (most of a wave belongs to the one big component)
  unsigned long long todo = __ballot(live);
  const int lane = threadIdx.x & 63;
  if (lane == 0 && todo) atomicAdd(&counters[kCntActive], (uint32_t)__popcll(todo));
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t rl = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
    const unsigned long long same = __ballot(live && r == rl) & todo;
    if (lane == leader) atomicAdd(&size[rl], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// E5 at the roots: a cluster's key orders by size descending, then root ascending; everything else sorts behind them
__global__ void __launch_bounds__(kClThreads) cl_root_key_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ size, size_t n,
                                                                 uint32_t lo, uint32_t hi, unsigned long long *__restrict__ key,
                                                                 uint32_t *__restrict__ counters)
{
  const size_t i = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i >= n) return;
  unsigned long long k = kNoKey;
  if (label[i] == (uint32_t)i) {
    const uint32_t s = size[i];
    if (s < lo) atomicAdd(&counters[kCntTooSmall], 1u);
    else if (s > hi) atomicAdd(&counters[kCntTooLarge], 1u);
    else {
      k = ((unsigned long long)(0xFFFFFFFFu - s) << 32) | (unsigned long long)i;      // s >= 1: never kNoKey
      atomicAdd(&counters[kCntClusters], 1u);
      atomicAdd(&counters[kCntClustered], s);
      atomicMax(&counters[kCntLargest], s);
    }
  }
  key[i] = k;
}

__global__ void __launch_bounds__(kClThreads) cl_rank_kernel(const unsigned long long *__restrict__ sorted, size_t n, uint32_t *__restrict__ rank)
{
  const size_t r = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (r >= n) return;
  const unsigned long long k = sorted[r];
  if (k != kNoKey) rank[(uint32_t)k] = (uint32_t)r;
}

// per point: its cluster's rank (E7's label), the key of the member lists, and whether dst takes it
__global__ void __launch_bounds__(kClThreads) cl_point_key_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ size,
                                                                  const uint32_t *__restrict__ rank, size_t n, uint32_t lo, uint32_t hi, uint32_t keep,
                                                                  unsigned long long *__restrict__ key, uint32_t *__restrict__ label_out,
                                                                  uint8_t *__restrict__ take)
{
  const size_t i = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t root = label[i];
  uint32_t rk = kNoLabel;
  if (root != kNoLabel) {
    const uint32_t s = size[root];
    if (s >= lo && s <= hi) rk = rank[root];
  }
  key[i] = rk == kNoLabel ? kNoKey : (((unsigned long long)rk << 32) | (unsigned long long)i);
  label_out[i] = rk;
  take[i] = rk < keep ? 1 : 0;          // (kNoLabel is below no keep)
}

// the sorted member keys -> the concatenated lists and the offsets: offset[c] where rank c begins, offset[c + 1] where it ends
__global__ void __launch_bounds__(kClThreads) cl_offsets_kernel(const unsigned long long *__restrict__ sorted, size_t n, uint32_t *__restrict__ cidx,
                                                                uint32_t *__restrict__ offset)
{
  const size_t k = (size_t)blockIdx.x * kClThreads + threadIdx.x;
  if (k >= n) return;
  const unsigned long long key = sorted[k];
  if (key == kNoKey) return;
  const uint32_t c = (uint32_t)(key >> 32);
  cidx[k] = (uint32_t)key;
  if (k == 0 || (uint32_t)(sorted[k - 1] >> 32) != c) offset[c] = (uint32_t)k;
  if (k + 1 == n || sorted[k + 1] == kNoKey) offset[c + 1] = (uint32_t)(k + 1);
}

template <bool FMA>
void launch_link(bool normals, const ClusterArgs &a, hipStream_t st)
{
  const dim3 grid(blocks_for(a.S.nq, kClThreads)), block(kClThreads);
  if (normals) hipLaunchKernelGGL((cl_link_kernel<FMA, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((cl_link_kernel<FMA, false>), grid, block, 0, st, a);
}

int cluster_cloud(Ctx *c, Cloud *dst, Cloud &src, const mvr_cluster_params &p, const uint32_t *index, size_t index_count,
                  mvr_cluster_result *res, size_t *n_out, uint32_t *cluster_offset, size_t offset_cap, uint32_t *cluster_index, uint32_t *label_out)
{
  const size_t n = src.n;
  const bool normals = src.has_normals, use_normals = p.use_normals != 0, fma = p.fma_dist != 0, negative = p.negative != 0;
  if (int rc = knn_cloud_ok(c, src, "euclidean_clusters")) return rc;
  for (size_t k = 0; index && k < index_count; ++k)
    if (index[k] >= n) return set_error(c, MVR_E_ARG, "euclidean_clusters: an index is outside the source");
  mvr_cluster_result R;
  std::memset(&R, 0, sizeof R);
  size_t kept = 0;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "euclidean_clusters reads back");
    const uint32_t lo = std::max(p.min_size, 1u), hi = p.max_size;
    size_t sel_bytes = 0, sort_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)n, 0, 64, c->stream));
    const size_t tmp_bytes = std::max(sel_bytes, sort_bytes);
    Carver plan;
    plan.plan<uint8_t>(n); plan.plan<uint8_t>(n); plan.plan<uint32_t>(index_count);
    for (int k = 0; k < 6; ++k) plan.plan<uint32_t>(n);
    plan.plan<uint32_t>(n + 1); plan.plan<uint32_t>(kCntWords);
    for (int k = 0; k < 3; ++k) plan.plan<unsigned long long>(n);
    plan.plan<float4>(n); plan.plan<char>(tmp_bytes);
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    uint8_t *active = s.take<uint8_t>(n), *take = s.take<uint8_t>(n);
    uint32_t *d_in = s.take<uint32_t>(index_count);
    uint32_t *parent = s.take<uint32_t>(n), *label = s.take<uint32_t>(n), *size = s.take<uint32_t>(n), *rank = s.take<uint32_t>(n),
             *d_label = s.take<uint32_t>(n), *cidx = s.take<uint32_t>(n);
    uint32_t *offset = s.take<uint32_t>(n + 1), *counters = s.take<uint32_t>(kCntWords);
    unsigned long long *key_a = s.take<unsigned long long>(n), *key_b = s.take<unsigned long long>(n), *list = s.take<unsigned long long>(n);
    float4 *stage = s.take<float4>(n);
    char *tmp = s.take<char>(tmp_bytes);
    const dim3 grid(blocks_for(n, kClThreads)), block(kClThreads);

    // 1. E1
    MVR_HIP_TRY(c, hipMemsetAsync(active, (!index || negative) ? 1 : 0, n, c->stream));
    if (index && index_count) {
      MVR_HIP_TRY(c, hipMemcpyAsync(d_in, index, index_count * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      if (int rc = launch_mark(c, d_in, index_count, (uint8_t)(negative ? 0 : 1), active)) return rc;
    }
    // 2. links
    ClusterArgs a{};
    if (int rc = fill_target(c, src, a.S)) return rc;
    fill_queries(src, a.S);
    a.nrm = use_normals ? src.nrm : nullptr; a.active = active; a.parent = parent;
    a.r2 = clamp_r2(p.tolerance); a.cos_eps = use_normals ? std::cos(p.eps_angle) : 0.0;
    hipLaunchKernelGGL(cl_iota_kernel, grid, block, 0, c->stream, parent, n);
    if (fma) launch_link<true>(use_normals, a, c->stream);
    else launch_link<false>(use_normals, a, c->stream);
    MVR_HIP_TRY(c, hipGetLastError());
    // 3. labels and sizes
    MVR_HIP_TRY(c, hipMemsetAsync(size, 0, n * sizeof(uint32_t), c->stream));
    MVR_HIP_TRY(c, hipMemsetAsync(counters, 0, kCntWords * sizeof(uint32_t), c->stream));
    for (int round = 0; round < 16; ++round) hipLaunchKernelGGL(cl_jump_kernel, grid, block, 0, c->stream, parent, n);
    hipLaunchKernelGGL(cl_label_kernel, grid, block, 0, c->stream, parent, active, n, label, size, counters);
    // 4. order
    hipLaunchKernelGGL(cl_root_key_kernel, grid, block, 0, c->stream, label, size, n, lo, hi, key_a, counters);
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, key_a, key_b, (int)n, 0, 64, c->stream));
    hipLaunchKernelGGL(cl_rank_kernel, grid, block, 0, c->stream, key_b, n, rank);
    hipLaunchKernelGGL(cl_point_key_kernel, grid, block, 0, c->stream, label, size, rank, n, lo, hi, dst ? p.keep : 0u, key_a, d_label, take);
    MVR_HIP_TRY(c, hipGetLastError());
    MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, key_a, key_b, (int)n, 0, 64, c->stream));
    hipLaunchKernelGGL(cl_offsets_kernel, grid, block, 0, c->stream, key_b, n, cidx, offset);
    MVR_HIP_TRY(c, hipGetLastError());
    if (dst)
      if (int rc = select_flagged(c, tmp, sel_bytes, take, n, list, counters + kCntKept)) return rc;
    // 5. home: the counters, then what they size
    uint32_t hc[kCntWords];
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(&R, hc, sizeof R);
    kept = dst ? hc[kCntKept] : 0;
    if (cluster_offset && offset_cap && R.n_clusters)
      MVR_HIP_TRY(c, hipMemcpyAsync(cluster_offset, offset, (std::min<size_t>(R.n_clusters, offset_cap - 1) + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (cluster_index && R.n_clustered) MVR_HIP_TRY(c, hipMemcpyAsync(cluster_index, cidx, (size_t)R.n_clustered * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (label_out) MVR_HIP_TRY(c, hipMemcpyAsync(label_out, d_label, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (dst)
      if (int rc = gather_kept(c, *dst, src.pts, normals ? src.nrm : nullptr, list, kept, stage, nullptr)) return rc;
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  }
  if (cluster_offset && offset_cap && !R.n_clusters) cluster_offset[0] = 0;
  if (dst) finish_dst(c, *dst, kept, normals);
  *res = R;
  if (n_out) *n_out = kept;
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API void mvr_cluster_default_params(mvr_cluster_params *p)
{
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->tolerance = 0.0;
  p->min_size = 1;
  p->max_size = 0x7FFFFFFFu;
  p->keep = 1;
}

API int mvr_cloud_euclidean_clusters(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_cluster_params *p, const uint32_t *index, size_t index_count,
                                     mvr_cluster_result *result, size_t *n_out, uint32_t *cluster_offset, size_t offset_cap, uint32_t *cluster_index,
                                     uint32_t *label)
{
  if (!ctx || !p || !result || !slot_ok(src_slot) || !(dst_slot == -1 || slot_ok(dst_slot))) return MVR_E_ARG;
  if (!(std::isfinite(p->tolerance) && p->tolerance > 0.0)) return MVR_E_ARG;
  if (dst_slot >= 0 && p->keep == 0) return MVR_E_ARG;
  if (p->use_normals && !(p->eps_angle > 0.0 && p->eps_angle <= M_PI)) return MVR_E_ARG;
  if (!index && index_count) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  if (p->use_normals && !c->slots[src_slot].has_normals) return MVR_E_ARG;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return cluster_cloud(c, dst_slot < 0 ? nullptr : &c->slots[dst_slot], c->slots[src_slot], *p, index, index_count, result, n_out, cluster_offset,
                       offset_cap, cluster_index, label);
}
