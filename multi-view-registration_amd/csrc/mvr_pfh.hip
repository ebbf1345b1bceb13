// csrc/mvr_pfh.hip -- pcl::PFHEstimation (radius or k neighbours, the cloud its own search surface) on the GPU (gfx950); the rules
// P1-P8 are written next to mvr_cloud_pfh in mvr_hip.h.
//
// PFH costs n_i (n_i - 1) / 2 pair features per query, ~ 20 000 at 200 neighbours: one thread per query, the shape of every
// other walk here, would leave the lanes of a wave with neighbourhoods of different sizes and no place for the lists.  So ONE
// WAVE PER QUERY (a block is one wave), the queries in the order of the cloud's grid so that blocks in flight share cells:
//   1. valid_normals_kernel (mvr_pair_features.h): the normals in grid order, w = 1 for a valid point.
//   2. pfh_radius_kernel: the wave walks the ball cooperatively -- the cell rows of knn_ball_cells / knn_row_range, its 64 lanes
//      over 64 consecutive grid positions of a row, a ballot compacting the lanes inside the ball -- and stages each neighbour as
//      two 16-byte records in LDS: the point with w = bits of its index, the normal with w = bits of its d2 (together the key of
//      P3).  Then the pairs (a < b) are dealt over the lanes in row-major order of the triangle -- lane l takes pairs l, l + 64,
//      ... and moves through the triangle by integer steps, no square root -- each lane computing F3 / P4 (the code of
//      mvr_pair_features.h) and adding 1 to a 125-bin u32 histogram in LDS with an integer LDS atomic.  The row is written with
//      the scale of P5.  pfh_knn_kernel stages straight from the k list instead (k <= 64: one entry per lane).
//   3. A query with more than `cap` neighbours (MVR_PFH_STAGE, or the tune key's lower value) only counts them in step 2, adds
//      itself to a list and reserves n_i records of device scratch (integer atomics; the order of the list changes nothing).  The
//      host reads the list's length, the largest n_i (P6) and the record total; pfh_tiled_kernel then takes one listed query per
//      wave: the same walk writes the records to scratch, and the pairs are processed tile against tile -- tile A in LDS, its
//      own pairs, then every later tile B in LDS and all |A| x |B| cross pairs.  Every pair is met once, whichever path.
// The counts are integers: the result does not depend on the order of anything (P8).  8.7 KiB of LDS per staged wave (18 waves
// per compute unit), 16.7 KiB per tiled one.  Compiled with -ffp-contract=off.
#include <cmath>
#include <cstring>

#include "mvr_feature_knn.h"
#include "mvr_internal.h"
#include "mvr_knn_walk.h"
#include "mvr_pair_features.h"

namespace mvr {
namespace {

constexpr int kLanes = 64;                       // a block is one wave
constexpr int kStage = MVR_PFH_STAGE;
constexpr int kDim = MVR_PFH_DIM, kSub = 5;
constexpr uint32_t kMaxNeighbors = 65535u;       // P6
static_assert(kSub * kSub * kSub == kDim, "125 joint bins");
static_assert(MVR_MAX_KNN <= kLanes && MVR_MAX_KNN <= kStage, "a k list is staged one entry per lane");

struct PfhTotals {
  unsigned long long records, pairs;             // scratch records reserved by the listed queries; sum of m_i
  uint32_t listed, max_n;
};

struct PfhArgs {
  KnnSlot S;                       // the surface as target; its own points as queries, or (at) the query array (nrm / curv / oidx / od2 unused)
  const float4 *gn;                // radius mode: normals in the order of S.gt, w = 1 for a valid point, else 0
  int at;                          // the queries are a query array (mvr_cloud_pfh_at): valid iff finite (Q2), rows by w
  const float4 *pts, *nrm;         // k mode: the slot's points and normals by index
  const uint32_t *kidx;            // k mode: [n][k] by index
  const float *kd2;
  int k;
  float r2;
  uint32_t cap;                    // neighbours staged in LDS (<= kStage); also the tile of the tiled path
  float *out;                      // [n][125] by index, or null
  uint32_t *counts;                // [n][125] by index, or null
  uint32_t *ncount;                // n_i by index
  PfhTotals *totals;
  uint32_t *big_pos;               // the listed queries: their position in S.qs ...
  unsigned long long *big_ofs;     // ... and their first record
  float4 *scratch;                 // records: [2 r] point, [2 r + 1] normal
};

// P3 / P4 for one pair of staged records: the member with the later key takes F3's role of "i"
__device__ __forceinline__ void pfh_pair(const float4 pa, const float4 na, const float4 pb, const float4 nb, uint32_t *hist)
{
  const nnkey_t ka = ((nnkey_t)__float_as_uint(na.w) << 32) | __float_as_uint(pa.w);
  const nnkey_t kb = ((nnkey_t)__float_as_uint(nb.w) << 32) | __float_as_uint(pb.w);
  const bool a_later = ka > kb;
  float f1, f2, f3;
  if (!pair_features(a_later ? pa : pb, a_later ? na : nb, a_later ? pb : pa, a_later ? nb : na, &f1, &f2, &f3)) return;
  int b1, b2, b3;
  pair_bins<kSub>(f1, f2, f3, &b1, &b2, &b3);
  atomicAdd(&hist[b1 + kSub * b2 + kSub * kSub * b3], 1u);
}

// every pair (a < b) of n staged records, dealt over the lanes: pair number t of the triangle's rows b = 1, 2, ... (row b holds
// a = 0..b - 1) goes to lane t mod 64
__device__ __forceinline__ void pfh_pairs_within(const float4 *sp, const float4 *sn, const uint32_t n, uint32_t *hist)
{
  uint32_t a = threadIdx.x, b = 1;
  while (b < n && a >= b) { a -= b; ++b; }
  while (b < n) {
    pfh_pair(sp[a], sn[a], sp[b], sn[b], hist);
    a += kLanes;
    while (b < n && a >= b) { a -= b; ++b; }
  }
}

// every pair of one record of tile A and one of tile B
__device__ __forceinline__ void pfh_pairs_cross(const float4 *ap, const float4 *an, const uint32_t na, const float4 *bp, const float4 *bn,
                                                const uint32_t nb, uint32_t *hist)
{
  for (uint32_t t = threadIdx.x; t < na * nb; t += kLanes) {      // (na, nb <= 256)
    const uint32_t a = t % na, b = t / na;
    pfh_pair(ap[a], an[a], bp[b], bn[b], hist);
  }
}

// the cooperative ball walk of one wave around the valid query q: put(slot, point record, normal record) for every valid target
// point with d2 <= r2, slot = 0, 1, ... in walk order; returns their number.  Uniform control flow: every lane of the wave calls
// it with the same arguments.
template <bool FMA, class Put>
__device__ __forceinline__ uint32_t pfh_walk(const KnnSlot &S, const float4 *__restrict__ gn, const float4 q, const float r2, Put &&put)
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
        float d2 = 0.f;
        if (j < e) {
          p = S.gt[j];
          d2 = knn_dist2<FMA>(p, q);
          if (d2 <= r2) { nj = gn[j]; in = nj.w != 0.f; }
        }
        const unsigned long long m = __ballot(in);
        if (in)
          put(n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), make_float4(p.x, p.y, p.z, __uint_as_float(knn_index_of(S, p, j))),
              make_float4(nj.x, nj.y, nj.z, d2));
        n += (uint32_t)__popcll(m);
      }
    }
  return n;
}

// P5: the row of query qi from its histogram; n == 0 (and an invalid query): NaN
__device__ __forceinline__ void pfh_write_row(const PfhArgs &a, const uint32_t qi, const uint32_t n, const bool valid, const uint32_t *hist)
{
  const unsigned long long m = (unsigned long long)n * (unsigned long long)(n > 0u ? n - 1u : 0u) / 2ull;
  const float scale = m > 0ull ? 100.0f / (float)m : 0.f;
  for (uint32_t h = threadIdx.x; h < (uint32_t)kDim; h += kLanes) {
    const uint32_t cnt = valid ? hist[h] : 0u;
    if (a.out) a.out[(size_t)qi * kDim + h] = valid && n > 0u ? (float)cnt * scale : __builtin_nanf("");
    if (a.counts) a.counts[(size_t)qi * kDim + h] = cnt;
  }
}

__device__ __forceinline__ void pfh_clear(uint32_t *hist)
{
  for (uint32_t h = threadIdx.x; h < 128u; h += kLanes) hist[h] = 0u;
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) pfh_radius_kernel(PfhArgs a)
{
  __shared__ float4 sp[kStage], sn[kStage];
  __shared__ uint32_t hist[128];
  const KnnSlot &S = a.S;
  const uint32_t pos = blockIdx.x;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  if (a.at ? !finite3(q) : a.gn[pos].w == 0.f) {      // P1 / Q2 (an invalid query walks nothing)
    pfh_write_row(a, qi, 0u, false, hist);
    if (threadIdx.x == 0) a.ncount[qi] = 0u;
    return;
  }
  pfh_clear(hist);
  const uint32_t cap = a.cap;
  const uint32_t n = pfh_walk<FMA>(S, a.gn, q, a.r2, [&](const uint32_t slot, const float4 p, const float4 nj) {
    if (slot < cap) { sp[slot] = p; sn[slot] = nj; }
  });
  if (threadIdx.x == 0) {
    a.ncount[qi] = n;
    atomicMax(&a.totals->max_n, n);
    atomicAdd(&a.totals->pairs, (unsigned long long)n * (unsigned long long)(n > 0u ? n - 1u : 0u) / 2ull);      // (n == 0: a query off the surface)
    if (n > cap) {                                    // the tiled launch takes it
      const uint32_t at = atomicAdd(&a.totals->listed, 1u);
      a.big_pos[at] = pos;
      a.big_ofs[at] = atomicAdd(&a.totals->records, (unsigned long long)n);
    }
  }
  if (n > cap) return;
  __syncthreads();
  pfh_pairs_within(sp, sn, n, hist);
  __syncthreads();
  pfh_write_row(a, qi, n, true, hist);
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) pfh_tiled_kernel(PfhArgs a)
{
  __shared__ float4 ap[kStage], an[kStage], bp[kStage], bn[kStage];
  __shared__ uint32_t hist[128];
  const KnnSlot &S = a.S;
  const uint32_t pos = a.big_pos[blockIdx.x];
  float4 *rec = a.scratch + 2ull * a.big_ofs[blockIdx.x];
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  pfh_clear(hist);
  const uint32_t reserved = a.ncount[qi];             // what the staged launch counted and reserved: the same walk gives the same n
  const uint32_t n = min(reserved, pfh_walk<FMA>(S, a.gn, q, a.r2, [&](const uint32_t slot, const float4 p, const float4 nj) {
    if (slot < reserved) { rec[2u * slot] = p; rec[2u * slot + 1u] = nj; }
  }));
  __syncthreads();
  const uint32_t tile = a.cap;
  for (uint32_t ta = 0; ta < n; ta += tile) {
    const uint32_t na = min(tile, n - ta);
    for (uint32_t r = threadIdx.x; r < na; r += kLanes) { ap[r] = rec[2u * (ta + r)]; an[r] = rec[2u * (ta + r) + 1u]; }
    __syncthreads();
    pfh_pairs_within(ap, an, na, hist);
    for (uint32_t tb = ta + tile; tb < n; tb += tile) {
      const uint32_t nb = min(tile, n - tb);
      for (uint32_t r = threadIdx.x; r < nb; r += kLanes) { bp[r] = rec[2u * (tb + r)]; bn[r] = rec[2u * (tb + r) + 1u]; }
      __syncthreads();
      pfh_pairs_cross(ap, an, na, bp, bn, nb, hist);
      __syncthreads();
    }
    __syncthreads();
  }
  pfh_write_row(a, qi, n, true, hist);
}

// k mode: block = query INDEX (at: output row, whose list is row qi of the table); lane l stages entry l of the query's list
__global__ void __launch_bounds__(kLanes) pfh_knn_kernel(PfhArgs a)
{
  __shared__ float4 sp[kLanes], sn[kLanes];
  __shared__ uint32_t hist[128];
  const uint32_t qi = blockIdx.x, lane = threadIdx.x;
  if (!a.at && !(finite3(a.pts[qi]) && finite3(a.nrm[qi]))) {  // P1 (at: an invalid query has an empty list, the same row)
    pfh_write_row(a, qi, 0u, false, hist);
    if (lane == 0) a.ncount[qi] = 0u;
    return;
  }
  pfh_clear(hist);
  bool in = false;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f), nj = p;
  uint32_t j = kNone;
  float d2 = 0.f;
  if (lane < (uint32_t)a.k) {
    j = a.kidx[(size_t)qi * a.k + lane];
    if (j != kNone) {
      p = a.pts[j]; nj = a.nrm[j]; d2 = a.kd2[(size_t)qi * a.k + lane];
      in = finite3(nj);                               // P2 (a listed point has finite coordinates: N1)
    }
  }
  const unsigned long long m = __ballot(in);
  const uint32_t n = (uint32_t)__popcll(m);
  if (in) {
    const uint32_t slot = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    sp[slot] = make_float4(p.x, p.y, p.z, __uint_as_float(j));
    sn[slot] = make_float4(nj.x, nj.y, nj.z, d2);
  }
  if (lane == 0) {
    a.ncount[qi] = n;
    atomicAdd(&a.totals->pairs, (unsigned long long)n * (unsigned long long)(n > 0u ? n - 1u : 0u) / 2ull);
  }
  __syncthreads();
  pfh_pairs_within(sp, sn, n, hist);
  __syncthreads();
  pfh_write_row(a, qi, n, true, hist);
}

// qc null: every point of the cloud cl against cl itself (mvr_cloud_pfh).  Else the queries of rules Q1 / Q2 -- the points
// `indices` of qc (null: all of them) -- over the surface cl (mvr_cloud_pfh_at); the refusals of both are the caller's.
int pfh_cloud(Ctx *c, Cloud &cl, const mvr_pfh_params &p, float *pfh, uint32_t *counts, uint32_t *neighbor_count, const Cloud *qc = nullptr,
              const uint32_t *indices = nullptr, size_t n_indices = 0)
{
  const size_t ns = cl.n, n = !qc ? ns : indices ? n_indices : qc->n;      // surface points; queries = output rows
  c->pfh_tiled = c->pfh_pairs = 0;
  if (!cl.has_normals && ns > 0) return set_error(c, MVR_E_ARG, "pfh: the slot has no normals");
  if (int rc = knn_cloud_ok(c, cl, "pfh")) return rc;
  if (n == 0) return MVR_OK;
  MVR_MAY_BLOCK(c, "pfh reads back");
  const bool kmode = p.k > 0, fma = p.fma_dist != 0;
  PfhArgs a{};
  a.at = qc ? 1 : 0;
  DevBuf klist_i, klist_d;
  AtQueries Q;
  KnnSlot self{};                                          // the surface walking itself: the order of gn
  if (kmode && !qc) {
    const size_t m = n * (size_t)p.k;
    if (klist_i.alloc(m * 4) != hipSuccess || klist_d.alloc(m * 4) != hipSuccess) return set_error(c, MVR_E_NOMEM, "pfh: out of device memory");
    if (int rc = knn_self_device(c, cl, p.k, fma, klist_i.as<uint32_t>(), klist_d.as<float>())) return rc;
    a.pts = cl.pts; a.nrm = cl.nrm; a.kidx = klist_i.as<uint32_t>(); a.kd2 = klist_d.as<float>(); a.k = p.k;
  } else {
    if (int rc = fill_target(c, cl, a.S)) return rc;      // (before the arena is carved: the grid build uses the context's buffers)
    fill_queries(cl, a.S);
    self = a.S;
    a.r2 = clamp_r2(p.radius);
    if (qc) {
      if (int rc = at_queries(c, *qc, qc == &cl, indices, n_indices, a.S, &Q)) return rc;
      a.S.qs = Q.q; a.S.q_by_pos = 0u; a.S.nq = (uint32_t)n;
    }
    if (kmode) {                                           // the lists of the queries in the surface, by row
      const size_t m = n * (size_t)p.k;
      if (klist_i.alloc(m * 4) != hipSuccess || klist_d.alloc(m * 4) != hipSuccess) return set_error(c, MVR_E_NOMEM, "pfh: out of device memory");
      a.S.oidx = klist_i.as<uint32_t>(); a.S.od2 = klist_d.as<float>();
      if (int rc = knn_device(c, a.S, p.k, fma)) return rc;
      a.pts = cl.pts; a.nrm = cl.nrm; a.kidx = klist_i.as<uint32_t>(); a.kd2 = klist_d.as<float>(); a.k = p.k;
    }
  }
  const size_t rows = n * (size_t)kDim;
  Carver plan;
  plan.plan<float4>(ns); plan.plan<float>(pfh ? rows : 1); plan.plan<uint32_t>(counts ? rows : 1); plan.plan<uint32_t>(n);
  plan.plan<PfhTotals>(1); plan.plan<uint32_t>(n); plan.plan<unsigned long long>(n);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  float4 *gn = s.take<float4>(ns);
  a.gn = gn;
  a.out = s.take<float>(pfh ? rows : 1);
  a.counts = s.take<uint32_t>(counts ? rows : 1);
  if (!pfh) a.out = nullptr;
  if (!counts) a.counts = nullptr;
  a.ncount = s.take<uint32_t>(n);
  a.totals = s.take<PfhTotals>(1);
  a.big_pos = s.take<uint32_t>(n);
  a.big_ofs = s.take<unsigned long long>(n);
  a.cap = (uint32_t)std::min(std::max(c->pfh_stage, MVR_MAX_KNN), kStage);
  MVR_HIP_TRY(c, hipMemsetAsync(a.totals, 0, sizeof(PfhTotals), c->stream));
  const dim3 grid((unsigned)n), block(kLanes);
  if (kmode) {
    hipLaunchKernelGGL(pfh_knn_kernel, grid, block, 0, c->stream, a);
  } else {
    if (ns > 0) {
      hipLaunchKernelGGL(valid_normals_kernel<kKnnThreads>, dim3(blocks_for(ns, kKnnThreads)), dim3(kKnnThreads), 0, c->stream, self, cl.nrm, gn);
      MVR_HIP_TRY(c, hipGetLastError());
    }
    if (fma) hipLaunchKernelGGL(pfh_radius_kernel<true>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(pfh_radius_kernel<false>, grid, block, 0, c->stream, a);
  }
  MVR_HIP_TRY(c, hipGetLastError());
  PfhTotals tot{};
  MVR_HIP_TRY(c, hipMemcpyAsync(&tot, a.totals, sizeof tot, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (tot.max_n > kMaxNeighbors) return set_error(c, MVR_E_ARG, "pfh: a neighbourhood of more than 65535 points (rule P6)");
  c->pfh_tiled = tot.listed; c->pfh_pairs = tot.pairs;
  DevBuf scratch;
  if (tot.listed) {
    if (scratch.alloc((size_t)tot.records * 2 * sizeof(float4)) != hipSuccess) return set_error(c, MVR_E_NOMEM, "pfh: out of device memory");
    a.scratch = scratch.as<float4>();
    if (fma) hipLaunchKernelGGL(pfh_tiled_kernel<true>, dim3(tot.listed), block, 0, c->stream, a);
    else hipLaunchKernelGGL(pfh_tiled_kernel<false>, dim3(tot.listed), block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
  }
  if (pfh) MVR_HIP_TRY(c, hipMemcpyAsync(pfh, a.out, rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (counts) MVR_HIP_TRY(c, hipMemcpyAsync(counts, a.counts, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (neighbor_count) MVR_HIP_TRY(c, hipMemcpyAsync(neighbor_count, a.ncount, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return, and the arena is free again
  return MVR_OK;
}

}  // namespace

// the matcher's kernels for rows of 125 floats (mvr_feature_knn.h; launched from mvr_feature.hip)
void launch_feature_knn_pfh(hipStream_t st, dim3 grid, const float *q, uint32_t nq, const float *t, uint32_t nt, uint32_t rows_per_split, int k,
                            nnkey_t *part)
{
  launch_feature_knn<kPfhDim>(st, grid, q, nq, t, nt, rows_per_split, k, part);
}

}  // namespace mvr

using namespace mvr;

API int mvr_cloud_pfh(mvr_ctx *ctx, int slot, const mvr_pfh_params *p, float *pfh, uint32_t *counts, uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(slot)) return MVR_E_ARG;
  const bool kmode = p->k != 0, rmode = p->radius != 0.0;
  if (kmode == rmode || p->k < 0 || p->k > MVR_MAX_KNN || !(std::isfinite(p->radius) && p->radius >= 0.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  return pfh_cloud(c, c->slots[slot], *p, pfh, counts, neighbor_count);
}

API int mvr_cloud_pfh_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot, const mvr_pfh_params *p, float *pfh,
                         uint32_t *counts, uint32_t *neighbor_count)
{
  if (!ctx || !p || !slot_ok(q_slot) || !slot_ok(surface_slot)) return MVR_E_ARG;
  const bool kmode = p->k != 0, rmode = p->radius != 0.0;
  if (kmode == rmode || p->k < 0 || p->k > MVR_MAX_KNN || !(std::isfinite(p->radius) && p->radius >= 0.0)) return MVR_E_ARG;
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[q_slot], &t = c->slots[surface_slot];
  if (!indices && q_slot == surface_slot) return pfh_cloud(c, t, *p, pfh, counts, neighbor_count);      // Q8
  if (!t.has_normals && t.n > 0) return set_error(c, MVR_E_ARG, "pfh: the surface slot has no normals");
  if (int rc = knn_cloud_ok(c, q, "pfh")) return rc;
  if (int rc = knn_cloud_ok(c, t, "pfh")) return rc;
  if (int rc = at_indices_ok(c, q, indices, n_indices, "pfh")) return rc;
  return pfh_cloud(c, t, *p, pfh, counts, neighbor_count, &q, indices, n_indices);
}
