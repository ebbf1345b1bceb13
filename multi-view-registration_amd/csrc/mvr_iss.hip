// csrc/mvr_iss.hip -- pcl::ISSKeypoint3D on the GPU (gfx950); the rules K1-K11 are written next to mvr_cloud_iss_keypoints in
// mvr_hip.h.
//
// One thread per query, in the order of the cloud's model grid (ensure_model_grid; the helpers of mvr_knn_walk.h), so the 64
// lanes of a wave are neighbours on the surface and walk the same cells:
//   0. with a border radius only: the boundary kernel (launch_boundary, mvr_boundary.hip) writes the edge flags of K9 by index
//      and by grid position, and the saliency kernel below is its BORDER instantiation, which first asks whether the ball of
//      the border radius holds an edge point (knn_ball_any over the flags in grid order, read beside the points as sal_grid
//      is); a point that has one is a border point (K10): zeros are written and the scatter walk is skipped (K11).  The
//      kernel is a template of mvr_knn_walk.h; its two BORDER instantiations are compiled in mvr_boundary.hip
//      (launch_iss_saliency_border), so that this file holds the kernels it always held.
//   1. iss_saliency_kernel: the ball walk (knn_ball_walk) at the salient radius adds the f64 second moments of the neighbours
//      about the query point (Moments::add of mvr_plane.h; the first moments and its f64 count are never read here and the
//      compiler drops them) and counts them; the eigenvalues come from the cyclic Jacobi of mvr_plane.h with the eigenvectors
//      left out (scatter_eigenvalues).  The saliency -- the smallest eigenvalue of a point that passes K4, else 0 -- is written
//      at the query's GRID position, so that the second walk reads it beside the point it belongs to, and by index for the host.
//   2. iss_nms_kernel: a point of saliency 0 leaves at once; every other one walks the ball of the non-maximum radius, counts
//      it and looks for a strictly larger saliency in it.  One flag per point, by index.
//   3. the flagged indices, ascending (select_flagged), one small read-back, then the gather of points and normals
//      (gather_kept), as the outlier filters do.
// No atomics and a fixed walk order: bit-identical from run to run on one grid.  Scratch arrays come out of the context's arena
// (Ctx::dn_arena).  Compiled with -ffp-contract=off.
#include <cmath>
#include <cstring>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_plane.h"

namespace mvr {
namespace {

template <bool FMA>
__global__ void __launch_bounds__(kIssThreads) iss_nms_kernel(IssArgs a)
{
  const KnnSlot &S = a.S;
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  const uint32_t pos = blockIdx.x * kIssThreads + threadIdx.x;
  const double s = a.sal_grid[pos];
  uint32_t n = 0;
  bool is_max = false;
  if (s != 0.0) {
    is_max = true;
    knn_ball_walk<FMA>(S, q, a.r2_nms, [&](const float4, const uint32_t j) {
      ++n;
      if (s < a.sal_grid[j]) is_max = false;      // strictly: equal saliencies are both kept (K5)
    });
  }
  a.nms_count[qi] = n;
  a.flag[qi] = (is_max && n >= a.min_neighbors) ? 1 : 0;
}

// dst null: the host arrays only
// b null: no border
int iss_cloud(Ctx *c, Cloud *dst, Cloud &src, const mvr_iss_params &p, const mvr_iss_border_params *b, size_t *n_out, uint32_t *kept_index,
              double *saliency, uint32_t *salient_count, uint32_t *nms_count, uint8_t *edge, uint8_t *border)
{
  const size_t n = src.n;
  const bool normals = src.has_normals;
  size_t kept = 0;
  if (b && !normals && n > 0) return set_error(c, MVR_E_ARG, "iss keypoints: a border radius needs the slot's normals");      // K9
  if (int rc = knn_cloud_ok(c, src, "iss keypoints")) return rc;
  if (n > 0) {
    MVR_MAY_BLOCK(c, "iss keypoints reads back");
    IssArgs a{};
    if (int rc = fill_target(c, src, a.S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
    fill_queries(src, a.S);
    size_t sel_bytes = 0;
    if (int rc = select_flagged(c, nullptr, sel_bytes, nullptr, n, nullptr, nullptr)) return rc;
    Carver plan;
    plan.plan<double>(n); plan.plan<double>(n); plan.plan<uint32_t>(n); plan.plan<uint32_t>(n); plan.plan<uint8_t>(n);
    plan.plan<unsigned long long>(n); plan.plan<uint32_t>(4); plan.plan<float4>(n); plan.plan<uint32_t>(n); plan.plan<char>(sel_bytes);
    if (b) { plan.plan<uint8_t>(n); plan.plan<uint8_t>(n); plan.plan<uint8_t>(n); }
    if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
    Carver s; s.base = c->dn_arena;
    a.sal_grid = s.take<double>(n);
    a.sal = s.take<double>(n);
    a.salient_count = s.take<uint32_t>(n);
    a.nms_count = s.take<uint32_t>(n);
    a.flag = s.take<uint8_t>(n);
    unsigned long long *list = s.take<unsigned long long>(n);
    uint32_t *counters = s.take<uint32_t>(4);
    float4 *out = s.take<float4>(n);
    uint32_t *d_index = s.take<uint32_t>(n);
    char *tmp = s.take<char>(sel_bytes);
    uint8_t *d_edge = nullptr;
    if (b) {
      d_edge = s.take<uint8_t>(n);
      a.edge_grid = s.take<uint8_t>(n);
      a.border = s.take<uint8_t>(n);
      a.r2_border = clamp_r2(b->border_radius);
    }
    a.gamma_21 = p.gamma_21; a.gamma_32 = p.gamma_32;
    a.min_neighbors = (uint32_t)p.min_neighbors;
    a.r2_salient = clamp_r2(p.salient_radius); a.r2_nms = clamp_r2(p.non_max_radius);
    const dim3 grid(blocks_for(n, kIssThreads)), block(kIssThreads);
    if (b) {
      // K9: the edge flags, by index for the host and by grid position for the walk of the border instantiation
      if (int rc = launch_boundary(c, a.S, src.nrm, a.r2_border, (float)b->angle_threshold, a.min_neighbors, p.fma_dist != 0, d_edge,
                                   const_cast<uint8_t *>(a.edge_grid), nullptr, nullptr))
        return rc;
      if (int rc = launch_iss_saliency_border(c, a, p.fma_dist != 0)) return rc;
    } else if (p.fma_dist) hipLaunchKernelGGL((iss_saliency_kernel<true, false>), grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL((iss_saliency_kernel<false, false>), grid, block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
    if (p.fma_dist) hipLaunchKernelGGL(iss_nms_kernel<true>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(iss_nms_kernel<false>, grid, block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
    // the keypoints' indices, ascending; the one read-back of the chain
    uint32_t hc[4] = {0, 0, 0, 0};
    if (int rc = select_flagged(c, tmp, sel_bytes, a.flag, n, list, counters)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (saliency) MVR_HIP_TRY(c, hipMemcpyAsync(saliency, a.sal, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (salient_count) MVR_HIP_TRY(c, hipMemcpyAsync(salient_count, a.salient_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (nms_count) MVR_HIP_TRY(c, hipMemcpyAsync(nms_count, a.nms_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (b && edge) MVR_HIP_TRY(c, hipMemcpyAsync(edge, d_edge, n * sizeof(uint8_t), hipMemcpyDeviceToHost, c->stream));
    if (b && border) MVR_HIP_TRY(c, hipMemcpyAsync(border, a.border, n * sizeof(uint8_t), hipMemcpyDeviceToHost, c->stream));
    if (!b && edge) std::memset(edge, 0, n);          // no border radius: nobody is an edge or a border point
    if (!b && border) std::memset(border, 0, n);
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    kept = hc[0];
    // the output (no destination: the indices alone, the points gathered into the arena and left there)
    if (dst) {
      if (int rc = gather_kept(c, *dst, src.pts, normals ? src.nrm : nullptr, list, kept, out, d_index)) return rc;
    } else if (kept_index) {
      if (int rc = launch_gather(c, src.pts, list, kept, out, d_index)) return rc;
    }
    if (kept_index && kept) MVR_HIP_TRY(c, hipMemcpyAsync(kept_index, d_index, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // kept_index is complete on return, and the arena is free again
  }
  if (dst) finish_dst(c, *dst, kept, normals);
  if (n_out) *n_out = kept;
  return MVR_OK;
}

}  // namespace
}  // namespace mvr

using namespace mvr;

API int mvr_cloud_iss_keypoints_border(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_iss_params *p, const mvr_iss_border_params *b,
                                       size_t *n_out, uint32_t *kept_index, double *saliency, uint32_t *salient_count, uint32_t *nms_count,
                                       uint8_t *edge, uint8_t *border)
{
  if (!ctx || !p || !slot_ok(src_slot) || !(dst_slot == -1 || slot_ok(dst_slot))) return MVR_E_ARG;
  if (!(std::isfinite(p->salient_radius) && p->salient_radius > 0.0) || !(std::isfinite(p->non_max_radius) && p->non_max_radius > 0.0))
    return MVR_E_ARG;
  if (!std::isfinite(p->gamma_21) || !std::isfinite(p->gamma_32) || p->min_neighbors < 0) return MVR_E_ARG;
  if (b && b->border_radius == 0.0) b = nullptr;      // radius 0: no border, whatever the threshold
  if (b && (!(std::isfinite(b->border_radius) && b->border_radius > 0.0) || !boundary_angle_ok(b->angle_threshold))) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return iss_cloud(c, dst_slot < 0 ? nullptr : &c->slots[dst_slot], c->slots[src_slot], *p, b, n_out, kept_index, saliency, salient_count,
                   nms_count, edge, border);
}

API int mvr_cloud_iss_keypoints(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_iss_params *p, size_t *n_out, uint32_t *kept_index,
                                double *saliency, uint32_t *salient_count, uint32_t *nms_count)
{
  return mvr_cloud_iss_keypoints_border(ctx, dst_slot, src_slot, p, nullptr, n_out, kept_index, saliency, salient_count, nms_count, nullptr,
                                        nullptr);
}
