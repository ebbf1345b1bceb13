// csrc/mvr_radius.hip -- pcl::search::KdTree::radiusSearch for every point of a slot at once, as CSR lists (gfx950); the rules
// RS1-RS12 are written next to mvr_radius_search in mvr_hip.h.
//
// The ball of every query is the one knn_ball_walk gives every other radius-mode entry of the library (RS1); what is new is the
// variable-length output: count, scan, fill, order.
//   1. radius_count_kernel: one thread per query (the queries in the order of their cloud's grid, as in mvr_knn.hip) walks the
//      ball with a counter and writes, by query index, the row's length n_i and the length it is given in the output,
//      min(n_i, max_nn).  A row longer than the stage adds itself to a list and reserves n_i keys of device scratch (integer
//      atomics; the order of the list changes nothing).
//   2. hipCUB's exclusive sum over the nq + 1 output lengths (the last one 0) gives the 64-bit offsets, offsets[nq] = total.
//      The host reads total, the list's length and the scratch total: the one wait of the call.
//   3. radius_fill_kernel, ONE WAVE PER QUERY (a block is one wave): the wave walks the ball cooperatively -- the cell rows of
//      knn_ball_cells / knn_row_range, its 64 lanes over 64 consecutive grid positions of a row, a ballot compacting the lanes
//      inside the ball -- and stages the 64-bit keys (bits(d2) << 32) | index in LDS.  It orders them there with a bitonic
//      network over the row padded to a power of two (skipped for sorted = 0 without max_nn: the walk order is fixed, RS5) and
//      writes idx / d2 of the row, consecutive lanes to consecutive entries.
//   4. The listed rows: radius_long_kernel, one wave per listed row, the same walk writing the keys to the row's scratch (with
//      sorted = 0 and no max_nn straight to the output, and that is all); hipCUB's segmented radix sort over the listed rows'
//      64-bit keys; radius_long_write_kernel copies the leading min(n_i, max_nn) keys of each sorted row to the output.
// Every row's order is fixed by the total order of the keys, so it does not matter which path it took (RS11).  8 KiB of LDS per
// wave: 20 waves per compute unit.  Compiled with -ffp-contract=off.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {
namespace {

constexpr int kLanes = 64;                       // a block of the fill kernels is one wave
constexpr int kStage = MVR_RADIUS_STAGE;
static_assert((kStage & (kStage - 1)) == 0 && kStage >= kLanes && MVR_MAX_KNN <= kStage, "the bitonic network pads a row to a power of two within the stage");

struct RadiusTotals {
  unsigned long long records;      // scratch keys reserved by the listed rows
  uint32_t listed, pad;
};

struct RadiusArgs {
  KnnSlot S;                       // (nrm / curv / oidx / od2 unused; blk0 = 0)
  float r2;
  uint32_t max_nn, cap;            // cap: entries staged in LDS (<= kStage)
  int order;                       // the rows are ordered (sorted, or max_nn > 0)
  uint32_t *nfull;                 // n_i by query index
  unsigned long long *len;         // [nq + 1] min(n_i, max_nn) by query index, then 0
  const unsigned long long *offsets;
  uint32_t *oidx; float *od2;      // [total]
  RadiusTotals *totals;
  uint32_t *big_pos, *big_qi;      // the listed rows: position in S.qs, query index ...
  unsigned long long *big_beg, *big_end;      // ... and their keys in the scratch
  nnkey_t *scratch;
};

__device__ __forceinline__ uint32_t row_len(const RadiusArgs &a, const uint32_t n) { return a.max_nn && n > a.max_nn ? a.max_nn : n; }

template <bool FMA>
__global__ void __launch_bounds__(kKnnThreads) radius_count_kernel(RadiusArgs a)
{
  float4 q; uint32_t qi;
  if (!knn_query(a.S, &q, &qi)) return;
  uint32_t n = 0;
  knn_ball_walk<FMA>(a.S, q, a.r2, [&](const float4, const uint32_t) { ++n; });
  a.nfull[qi] = n;
  a.len[qi] = row_len(a, n);
  if (qi == 0) a.len[a.S.nq] = 0ull;
  if (n > a.cap) {
    const uint32_t at = atomicAdd(&a.totals->listed, 1u);
    const unsigned long long beg = atomicAdd(&a.totals->records, (unsigned long long)n);
    a.big_pos[at] = blockIdx.x * kKnnThreads + threadIdx.x;
    a.big_qi[at] = qi;
    a.big_beg[at] = beg;
    a.big_end[at] = beg + n;
  }
}

// the cooperative ball walk of one wave around q: put(slot, key) for every target point with d2 <= r2, slot = 0, 1, ... in
// walk order (the order of knn_ball_walk); returns their number.  Uniform control flow: every lane calls it with the same
// arguments.
template <bool FMA, class Put>
__device__ __forceinline__ uint32_t radius_walk(const KnnSlot &S, const float4 q, const float r2, Put &&put)
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
        nnkey_t key = 0ull;
        if (j < e) {
          const float4 p = S.gt[j];
          const float d2 = knn_dist2<FMA>(p, q);
          in = d2 <= r2;
          key = ((nnkey_t)__float_as_uint(d2) << 32) | knn_index_of(S, p, j);
        }
        const unsigned long long m = __ballot(in);
        if (in) put(n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), key);
        n += (uint32_t)__popcll(m);
      }
    }
  return n;
}

__device__ __forceinline__ void write_row(const RadiusArgs &a, const unsigned long long at, const nnkey_t *keys, const uint32_t len)
{
  for (uint32_t r = threadIdx.x; r < len; r += kLanes) {
    const nnkey_t key = keys[r];
    a.oidx[at + r] = (uint32_t)key;
    a.od2[at + r] = __uint_as_float((uint32_t)(key >> 32));
  }
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) radius_fill_kernel(RadiusArgs a)
{
  __shared__ nnkey_t sk[kStage];
  const KnnSlot &S = a.S;
  const uint32_t pos = blockIdx.x;
  const float4 q = S.qs[pos];
  const uint32_t qi = S.q_by_pos ? pos : __float_as_uint(q.w);
  const uint32_t counted = a.nfull[qi];               // what the count launch found: the same ball gives the same n
  if (counted == 0u || counted > a.cap) return;       // (a longer row is listed: radius_long_kernel)
  const uint32_t n = min(counted, radius_walk<FMA>(S, q, a.r2, [&](const uint32_t slot, const nnkey_t key) {
    if (slot < counted) sk[slot] = key;
  }));
  __syncthreads();
  if (a.order) {
    uint32_t m = kLanes;
    while (m < n) m <<= 1;                            // (n <= cap <= kStage, a power of two)
    for (uint32_t i = n + threadIdx.x; i < m; i += kLanes) sk[i] = ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = threadIdx.x; i < m; i += kLanes) {
          const uint32_t o = i ^ j;
          if (o > i) {
            const nnkey_t x = sk[i], y = sk[o];
            if ((x > y) == ((i & k) == 0u)) { sk[i] = y; sk[o] = x; }
          }
        }
        __syncthreads();
      }
  }
  write_row(a, a.offsets[qi], sk, row_len(a, n));
}

template <bool FMA>
__global__ void __launch_bounds__(kLanes) radius_long_kernel(RadiusArgs a)
{
  const KnnSlot &S = a.S;
  const uint32_t pos = a.big_pos[blockIdx.x], qi = a.big_qi[blockIdx.x];
  const float4 q = S.qs[pos];
  const uint32_t reserved = (uint32_t)(a.big_end[blockIdx.x] - a.big_beg[blockIdx.x]);
  if (a.order) {
    nnkey_t *rec = a.scratch + a.big_beg[blockIdx.x];
    radius_walk<FMA>(S, q, a.r2, [&](const uint32_t slot, const nnkey_t key) { if (slot < reserved) rec[slot] = key; });
  } else {                                            // RS5: the walk order, straight to the output (no max_nn: the row has n_i entries)
    const unsigned long long at = a.offsets[qi];
    radius_walk<FMA>(S, q, a.r2, [&](const uint32_t slot, const nnkey_t key) {
      if (slot < reserved) { a.oidx[at + slot] = (uint32_t)key; a.od2[at + slot] = __uint_as_float((uint32_t)(key >> 32)); }
    });
  }
}

__global__ void __launch_bounds__(kLanes) radius_long_write_kernel(RadiusArgs a, const nnkey_t *sorted)
{
  const uint32_t qi = a.big_qi[blockIdx.x];
  const uint32_t n = (uint32_t)(a.big_end[blockIdx.x] - a.big_beg[blockIdx.x]);
  write_row(a, a.offsets[qi], sorted + a.big_beg[blockIdx.x], row_len(a, n));
}

}  // namespace

RadiusLists::~RadiusLists()
{
  if (offsets) (void)hipFree(offsets);
  if (idx) (void)hipFree(idx);
  if (d2) (void)hipFree(d2);
}

int radius_search_device(Ctx *c, Cloud &q, Cloud &t, const mvr_radius_params &p, bool fill, size_t capacity, RadiusLists *out)
{
  const size_t nq = q.n;
  const bool fma = p.fma_dist != 0;
  c->radius_long_rows = 0;
  c->radius_ms[0] = c->radius_ms[1] = c->radius_ms[2] = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  out->nq = nq; out->total = 0; out->counted = false;
  MVR_HIP_TRY(c, hipMalloc(&out->offsets, (nq + 1) * sizeof(unsigned long long)));
  if (nq == 0) {
    MVR_HIP_TRY(c, hipMemsetAsync(out->offsets, 0, sizeof(unsigned long long), c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->counted = true;
    return MVR_OK;
  }
  MVR_MAY_BLOCK(c, "radius search reads back");
  RadiusArgs a{};
  if (int rc = fill_target(c, t, a.S)) return rc;
  if (&q != &t && q.n >= 4) {      // the queries' own grid gives them their walking order
    bool ok = false;
    if (int rc = ensure_model_grid(c, q, &ok)) return rc;
  }
  fill_queries(q, a.S);
  a.r2 = clamp_r2(p.radius);
  a.max_nn = p.max_nn;
  a.order = (p.sorted != 0 || p.max_nn != 0) ? 1 : 0;
  a.cap = (uint32_t)std::min(std::max(c->radius_stage, MVR_MAX_KNN), kStage);
  size_t scan_bytes = 0;
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (int)(nq + 1), c->stream));
  Carver plan;
  plan.plan<uint32_t>(nq); plan.plan<unsigned long long>(nq + 1); plan.plan<RadiusTotals>(1); plan.plan<uint32_t>(nq); plan.plan<uint32_t>(nq);
  plan.plan<unsigned long long>(nq); plan.plan<unsigned long long>(nq); plan.plan<char>(scan_bytes);
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  a.nfull = s.take<uint32_t>(nq);
  a.len = s.take<unsigned long long>(nq + 1);
  a.totals = s.take<RadiusTotals>(1);
  a.big_pos = s.take<uint32_t>(nq);
  a.big_qi = s.take<uint32_t>(nq);
  a.big_beg = s.take<unsigned long long>(nq);
  a.big_end = s.take<unsigned long long>(nq);
  char *scan_tmp = s.take<char>(scan_bytes);
  a.offsets = out->offsets;
  // 1, 2. the lengths and the offsets
  MVR_HIP_TRY(c, hipMemsetAsync(a.totals, 0, sizeof(RadiusTotals), c->stream));
  const dim3 cgrid(blocks_for(nq, kKnnThreads)), cblock(kKnnThreads);
  if (fma) hipLaunchKernelGGL(radius_count_kernel<true>, cgrid, cblock, 0, c->stream, a);
  else hipLaunchKernelGGL(radius_count_kernel<false>, cgrid, cblock, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  MVR_HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, a.len, out->offsets, (int)(nq + 1), c->stream));
  RadiusTotals tot{};
  unsigned long long total = 0;
  MVR_HIP_TRY(c, hipMemcpyAsync(&tot, a.totals, sizeof tot, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipMemcpyAsync(&total, out->offsets + nq, sizeof total, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  out->total = (size_t)total; out->counted = true;
  c->radius_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->radius_long_rows = tot.listed;
  char msg[192];
  if (total > MVR_RADIUS_MAX_TOTAL || (a.order && tot.records > MVR_RADIUS_MAX_TOTAL)) {
    std::snprintf(msg, sizeof msg, "mvr_radius_search: %llu entries (%llu keys of long rows to order) exceed MVR_RADIUS_MAX_TOTAL = %llu (rule RS8)",
                  total, tot.records, (unsigned long long)MVR_RADIUS_MAX_TOTAL);
    return set_error(c, MVR_E_ARG, msg);
  }
  if (!fill) return MVR_OK;
  if (total > capacity) {
    std::snprintf(msg, sizeof msg, "mvr_radius_search: capacity %zu is short of the total %llu (rule RS7)", capacity, total);
    return set_error(c, MVR_E_ARG, msg);
  }
  if (total == 0) return MVR_OK;
  // 3. the staged rows
  MVR_HIP_TRY(c, hipMalloc(&out->idx, (size_t)total * sizeof(uint32_t)));
  MVR_HIP_TRY(c, hipMalloc(&out->d2, (size_t)total * sizeof(float)));
  a.oidx = out->idx; a.od2 = out->d2;
  const dim3 block(kLanes);
  if (fma) hipLaunchKernelGGL(radius_fill_kernel<true>, dim3((unsigned)nq), block, 0, c->stream, a);
  else hipLaunchKernelGGL(radius_fill_kernel<false>, dim3((unsigned)nq), block, 0, c->stream, a);
  MVR_HIP_TRY(c, hipGetLastError());
  // 4. the listed rows
  if (tot.listed) {
    DevBuf keys_a, keys_b, sort_tmp;
    const nnkey_t *sorted = nullptr;
    size_t sort_bytes = 0;
    if (a.order) {
      if (keys_a.alloc((size_t)tot.records * sizeof(nnkey_t)) != hipSuccess || keys_b.alloc((size_t)tot.records * sizeof(nnkey_t)) != hipSuccess)
        return set_error(c, MVR_E_NOMEM, "mvr_radius_search: out of device memory");
      a.scratch = keys_a.as<nnkey_t>();
      sorted = keys_b.as<nnkey_t>();
      MVR_HIP_TRY(c, hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_bytes, a.scratch, keys_b.as<nnkey_t>(), (int)tot.records, (int)tot.listed,
                                                                a.big_beg, a.big_end, 0, 64, c->stream));
      if (sort_tmp.alloc(sort_bytes) != hipSuccess) return set_error(c, MVR_E_NOMEM, "mvr_radius_search: out of device memory");
    }
    if (fma) hipLaunchKernelGGL(radius_long_kernel<true>, dim3(tot.listed), block, 0, c->stream, a);
    else hipLaunchKernelGGL(radius_long_kernel<false>, dim3(tot.listed), block, 0, c->stream, a);
    MVR_HIP_TRY(c, hipGetLastError());
    if (a.order) {
      MVR_HIP_TRY(c, hipcub::DeviceSegmentedRadixSort::SortKeys(sort_tmp.p, sort_bytes, a.scratch, keys_b.as<nnkey_t>(), (int)tot.records, (int)tot.listed,
                                                                a.big_beg, a.big_end, 0, 64, c->stream));
      hipLaunchKernelGGL(radius_long_write_kernel, dim3(tot.listed), block, 0, c->stream, a, sorted);
      MVR_HIP_TRY(c, hipGetLastError());
    }
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the scratch of the listed rows is freed here
  }
  return MVR_OK;
}

}  // namespace mvr

using namespace mvr;

API void mvr_radius_default_params(mvr_radius_params *p)
{
  if (!p) return;
  p->radius = 0.0; p->max_nn = 0u; p->sorted = 1; p->fma_dist = 0;
}

API int mvr_radius_search(mvr_ctx *ctx, int qs, int ts, const mvr_radius_params *p, uint64_t *offsets, uint32_t *idx, float *d2, size_t capacity,
                          size_t *total)
{
  if (!ctx) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  if (!p) return set_error(c, MVR_E_ARG, "mvr_radius_search: no parameters");
  if (!slot_ok(qs) || !slot_ok(ts)) return set_error(c, MVR_E_ARG, "mvr_radius_search: a slot number outside 0..MVR_MAX_SLOTS - 1");
  if (!(std::isfinite(p->radius) && p->radius > 0.0)) return set_error(c, MVR_E_ARG, "mvr_radius_search: the radius must be finite and > 0");
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  Cloud &q = c->slots[qs], &t = c->slots[ts];
  if (int rc = knn_cloud_ok(c, q, "mvr_radius_search")) return rc;
  if (int rc = knn_cloud_ok(c, t, "mvr_radius_search")) return rc;
  const bool fill = idx || d2;
  RadiusLists L;
  const auto t0 = std::chrono::steady_clock::now();
  const auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
  const int rc = radius_search_device(c, q, t, *p, fill, fill ? capacity : SIZE_MAX, &L);
  if (L.counted) {      // (also when the call refused after the count: RS7, RS8)
    if (total) *total = L.total;
    if (offsets) {
      const hipError_t e = hipMemcpyAsync(offsets, L.offsets, (L.nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
      const hipError_t e2 = hipStreamSynchronize(c->stream);
      if (!rc && (e != hipSuccess || e2 != hipSuccess)) return set_error(c, MVR_E_HIP, "mvr_radius_search copy", e != hipSuccess ? e : e2);
    }
  }
  if (rc) return rc;
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the phase clock; the copies below wait for the rows anyway)
  c->radius_ms[1] = ms_since(t0) - c->radius_ms[0];
  const auto t1 = std::chrono::steady_clock::now();
  if (fill && L.total) {
    if (idx) MVR_HIP_TRY(c, hipMemcpyAsync(idx, L.idx, L.total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (d2) MVR_HIP_TRY(c, hipMemcpyAsync(d2, L.d2, L.total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host arrays are complete on return
  c->radius_ms[2] = ms_since(t1);
  return MVR_OK;
}
