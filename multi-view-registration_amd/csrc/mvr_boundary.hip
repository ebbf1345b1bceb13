// csrc/mvr_boundary.hip -- pcl::BoundaryEstimation (radius search, the cloud its own search surface) on the GPU (gfx950); the
// rules B1-B7 are written next to mvr_cloud_boundary in mvr_hip.h.
//
// One thread per query, in the order of the cloud's model grid (ensure_model_grid; the helpers of mvr_knn_walk.h), so the 64
// lanes of a wave are neighbours on the surface and walk the same cells.  One ball walk (knn_ball_walk) per query; the query's
// normal is read by index and gives the tangent basis (u, v) of B2; every neighbour gives one angle atan2f(v . d, u . d).
//
// PCL sorts the angles of a query.  Their number is unbounded, so nothing is sorted here: the circle is cut into kSectors equal
// sectors -- sector(a) = floor((a + pi) * kSectors / 2 pi), clamped, monotone in a -- and a thread keeps the smallest and the
// largest angle of each.  The sector is a runtime value, and a runtime-indexed private array lives in scratch memory
// (mvr_knn.hip), so the 2 x 16 floats of a thread lie in LDS as [sector][thread], as the histogram of fpfh_spfh_kernel does: lane
// t reads and writes the address sector * 256 + t, which is bank t mod 32 whatever its sector, and the entries are private, so
// plain read-modify-write is enough.  32 KiB per block of 256.  After the walk one pass over the occupied sectors, in ascending
// order, takes the largest of (smallest angle of the next occupied sector - largest angle of this one) and of the wrap-around
// from the last maximum to the first minimum: the gaps of the sorted sequence that lie BETWEEN sectors, computed from the same
// two f32 operands as the sorted differences are.  Two angles of one sector are less than a sector width apart, so every gap
// of at least a sector width lies between sectors: the pass returns max_dif itself whenever that is at least a sector width, and
// something below a sector width otherwise -- and the accepted thresholds start at two sector widths (MVR_BOUNDARY_MIN_ANGLE).
// This file also compiles the BORDER instantiations of the ISS saliency kernel (mvr_knn_walk.h; launch_iss_saliency_border),
// which read the flags written here.
// No atomics and a fixed walk order (the result does not even depend on it: minima and maxima): bit-identical from run to run.
// Compiled with -ffp-contract=off (every f32 operation of the basis and of the projections is rounded as written).
#include <cfloat>
#include <cmath>
#include <cstring>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {
namespace {

constexpr int kBoundaryThreads = kKnnThreads;
constexpr int kSectors = 16;
static_assert(MVR_BOUNDARY_MIN_ANGLE >= 2.0 * (2.0 * M_PI / kSectors) * (1.0 - 1e-12), "the smallest threshold is two sector widths");

struct BoundaryArgs {
  KnnSlot S;                       // the cloud searched against itself (nrm / curv / oidx / od2 unused; blk0 = 0)
  const float4 *src_nrm;           // the slot's normals, by index
  uint8_t *flag, *flag_grid;       // by index / by grid position (either may be null)
  float *gap;                      // max_gap by index (may be null)
  uint32_t *count;                 // by index (may be null)
  float r2, threshold;
  uint32_t min_neighbors;
};

template <bool FMA>
__global__ void __launch_bounds__(kBoundaryThreads) boundary_kernel(BoundaryArgs a)
{
  __shared__ float lo[kSectors * kBoundaryThreads], hi[kSectors * kBoundaryThreads];      // [sector][thread]
  const KnnSlot &S = a.S;
  float4 q; uint32_t qi;
  if (!knn_query(S, &q, &qi)) return;
  const uint32_t tid = threadIdx.x, pos = blockIdx.x * kBoundaryThreads + tid;
  // B2: the tangent basis
  const float4 n = a.src_nrm[qi];
  const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
  const int maxi = az > fmaxf(ax, ay) ? 2 : (ay > ax ? 1 : 0);      // the FIRST index of the largest
  float vx, vy, vz;
  if (maxi == 0) {
    const float inv = 1.0f / sqrtf(n.y * n.y + n.x * n.x);
    vx = -n.y * inv; vy = n.x * inv; vz = 0.f;
  } else if (maxi == 1) {
    const float inv = 1.0f / sqrtf(n.x * n.x + n.y * n.y);
    vx = n.y * inv; vy = -n.x * inv; vz = 0.f;
  } else {
    const float inv = 1.0f / sqrtf(n.x * n.x + n.z * n.z);
    vx = n.z * inv; vy = 0.f; vz = -n.x * inv;
  }
  const float ux = n.y * vz - n.z * vy, uy = n.z * vx - n.x * vz, uz = n.x * vy - n.y * vx;
  const bool basis = finite3(n) && isfinite(ux) && isfinite(uy) && isfinite(uz) && isfinite(vx) && isfinite(vy) && isfinite(vz);
#pragma unroll
  for (int s = 0; s < kSectors; ++s) {
    lo[s * kBoundaryThreads + tid] = INFINITY;
    hi[s * kBoundaryThreads + tid] = -INFINITY;
  }
  uint32_t cnt = 0;      // (a non-finite query walks nothing: B1)
  const float pi = (float)M_PI, per_rad = (float)(kSectors / (2.0 * M_PI));
  knn_ball_walk<FMA>(S, q, a.r2, [&](const float4 p, uint32_t) {
    ++cnt;
    if (!basis) return;
    // B3
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    if (dx == 0.f && dy == 0.f && dz == 0.f) return;
    const float ang = atan2f((vx * dx + vy * dy) + vz * dz, (ux * dx + uy * dy) + uz * dz);
    const int s = (int)fminf(fmaxf(floorf((ang + pi) * per_rad), 0.f), (float)(kSectors - 1));
    const uint32_t at = (uint32_t)s * kBoundaryThreads + tid;
    lo[at] = fminf(lo[at], ang);
    hi[at] = fmaxf(hi[at], ang);
  });
  // B4 over the occupied sectors
  float gap = FLT_MIN, first = 0.f, last = 0.f;
  bool any = false;
#pragma unroll
  for (int s = 0; s < kSectors; ++s) {
    const float l = lo[s * kBoundaryThreads + tid], h = hi[s * kBoundaryThreads + tid];
    if (l <= h) {
      if (any) gap = fmaxf(gap, l - last);
      else first = l;
      last = h;
      any = true;
    }
  }
  if (any) gap = fmaxf(gap, (2.0f * pi - last) + first);
  // B5
  const bool edge = any && cnt >= 3u && cnt >= a.min_neighbors && gap > a.threshold;
  if (a.flag) a.flag[qi] = edge ? 1 : 0;
  if (a.flag_grid) a.flag_grid[pos] = edge ? 1 : 0;
  if (a.gap) a.gap[qi] = any ? gap : 0.f;
  if (a.count) a.count[qi] = cnt;
}

int boundary_cloud(Ctx *c, Cloud &cl, const mvr_boundary_params &p, uint8_t *boundary, float *max_gap, uint32_t *neighbor_count)
{
  const size_t n = cl.n;
  if (!cl.has_normals && n > 0) return set_error(c, MVR_E_ARG, "boundary: the slot has no normals");
  if (int rc = knn_cloud_ok(c, cl, "boundary")) return rc;
  if (n == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "boundary reads back");
  KnnSlot S{};
  if (int rc = fill_target(c, cl, S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
  fill_queries(cl, S);
  Carver plan;
  plan.plan<uint8_t>(n); plan.plan<float>(n); plan.plan<uint32_t>(n);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  uint8_t *flag = s.take<uint8_t>(n);
  float *gap = s.take<float>(n);
  uint32_t *count = s.take<uint32_t>(n);
  if (int rc = launch_boundary(c, S, cl.nrm, clamp_r2(p.radius), (float)p.angle_threshold, (uint32_t)p.min_neighbors, p.fma_dist != 0,
                               flag, nullptr, max_gap ? gap : nullptr, neighbor_count ? count : nullptr))
    return rc;
  if (boundary) MVR_HIP_TRY(c, hipMemcpyAsync(boundary, flag, n * sizeof(uint8_t), hipMemcpyDeviceToHost, c->stream));
  if (max_gap) MVR_HIP_TRY(c, hipMemcpyAsync(max_gap, gap, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (neighbor_count) MVR_HIP_TRY(c, hipMemcpyAsync(neighbor_count, count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  return MVR_OK;
}

}  // namespace

int launch_boundary(Ctx *c, const KnnSlot &S, const float4 *nrm, float r2, float angle_threshold, uint32_t min_neighbors, bool fma,
                    uint8_t *flag, uint8_t *flag_grid, float *max_gap, uint32_t *count)
{
  if (S.nq == 0) return MVR_OK;
  BoundaryArgs a{};
  a.S = S; a.S.blk0 = 0;
  a.src_nrm = nrm;
  a.flag = flag; a.flag_grid = flag_grid; a.gap = max_gap; a.count = count;
  a.r2 = r2; a.threshold = angle_threshold; a.min_neighbors = min_neighbors;
  const dim3 grid(blocks_for(S.nq, kBoundaryThreads)), block(kBoundaryThreads);
  if (fma) hipLaunchKernelGGL(boundary_kernel<true>, grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL(boundary_kernel<false>, grid, block, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

int launch_iss_saliency_border(Ctx *c, const IssArgs &a, bool fma)
{
  const dim3 grid(blocks_for(a.S.nq, kIssThreads)), block(kIssThreads);
  if (fma) hipLaunchKernelGGL((iss_saliency_kernel<true, true>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((iss_saliency_kernel<false, true>), grid, block, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

// B6's range of the angle threshold: [MVR_BOUNDARY_MIN_ANGLE, 2 pi)
bool boundary_angle_ok(double t) { return std::isfinite(t) && t >= MVR_BOUNDARY_MIN_ANGLE && t < 2.0 * M_PI; }

}  // namespace mvr

using namespace mvr;

API int mvr_cloud_boundary(mvr_ctx *ctx, int slot, const mvr_boundary_params *p, uint8_t *boundary, float *max_gap, uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(slot)) return MVR_E_ARG;
  if (!(std::isfinite(p->radius) && p->radius > 0.0) || p->min_neighbors < 0 || !boundary_angle_ok(p->angle_threshold)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return boundary_cloud(c, c->slots[slot], *p, boundary, max_gap, neighbor_count);
}
