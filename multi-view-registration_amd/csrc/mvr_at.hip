// csrc/mvr_at.hip -- the query side of the entries that answer chosen queries over a search surface (mvr_cloud_estimate_normals_at
// in mvr_knn.hip, mvr_cloud_fpfh_at in mvr_fpfh.hip, mvr_cloud_pfh_at in mvr_pfh.hip; rules Q1-Q8 in mvr_hip.h), for gfx950:
//   * at_gather_kernel builds the query array: q[r] = the position of the point that output row r answers, w = bits of r, NaN
//     coordinates for a query that is invalid under Q2 (it walks nothing: every entry gives it the row of an empty
//     neighbourhood), and the sort key of the row, the cell of the SURFACE's grid the query falls in;
//   * one hipCUB pair sort orders the rows by that key, so that the 64 lanes of a wave (one thread per query) or consecutive
//     waves (one wave per query: PFH) walk the same cells of the surface.  Tune key "at_sort" = 0 leaves it out; no result
//     depends on it, every row is written by its own number.  Measured on an MI355X (profiles/feature_at_bench.json), sorted /
//     unsorted, at the ISS keypoints: FPFH 2.5 / 5 mm on a 200k view 2.61 / 3.08 and 8.38 / 12.2 ms, on the 2.4 M object 37.5 / 36.7
//     and 146 / 148 ms; PFH 2.5 mm 0.63 / 0.60 ms on the view, 55.2 / 62.0 ms on the object.  It pays where one thread walks per
//     query and on the large cloud, and costs 5 % where one wave walks a small cloud: it stays on;
//   * at_mark_kernel is the marking walk of the SPFH on demand (see mvr_fpfh.hip).
// A walk's cells and order depend only on the query position and the surface's grid -- not on where the query came from -- which
// is why a query at a surface point gets the bits the whole-cloud calls give that point (Q5).
#include <string>

#include <hipcub/hipcub.hpp>

#include "mvr_internal.h"
#include "mvr_knn_walk.h"

namespace mvr {
namespace {

// the query array of the _at entries before its sort: q[r] = the position of point indices[r] (or r) with w = bits of r, NaN
// coordinates for an invalid query; key[r] = the cell of the surface's grid it falls in, `cells` for an invalid one
__global__ void __launch_bounds__(kKnnThreads) at_gather_kernel(const float4 *__restrict__ pts, const float4 *__restrict__ nrm,
                                                                const uint32_t *__restrict__ indices, const uint32_t rows, const KnnSlot S,
                                                                const uint32_t cells, float4 *__restrict__ q, uint32_t *__restrict__ key)
{
  const uint32_t r = blockIdx.x * kKnnThreads + threadIdx.x;
  if (r >= rows) return;
  const uint32_t i = indices ? indices[r] : r;
  float4 p = pts[i];
  const bool ok = finite3(p) && (!nrm || finite3(nrm[i]));
  if (!ok) p.x = p.y = p.z = __builtin_nanf("");
  q[r] = make_float4(p.x, p.y, p.z, __uint_as_float(r));
  uint32_t c = 0u;
  if (!ok) c = cells;
  else if (S.dir)
    c = (uint32_t)((knn_cell_of(p.z, S.lo[2], S.inv_h, S.dim[2]) * S.dim[1] + knn_cell_of(p.y, S.lo[1], S.inv_h, S.dim[1])) * S.dim[0] +
                   knn_cell_of(p.x, S.lo[0], S.inv_h, S.dim[0]));
  key[r] = c;
}

// the marking walk of the SPFH on demand (mvr_fpfh.hip): n_i of every query of the query array -- its neighbours that are valid in
// gn -- by output row, and need[j] = 1 at the grid position j of each of them: a plain store of one constant (racing stores of
// the same value need no atomic)
template <bool FMA>
__global__ void __launch_bounds__(kKnnThreads) at_mark_kernel(const KnnSlot S, const float4 *__restrict__ gn, const float r2,
                                                              uint32_t *__restrict__ count, uint8_t *__restrict__ need)
{
  const uint32_t pos = blockIdx.x * kKnnThreads + threadIdx.x;
  if (pos >= S.nq) return;
  const float4 q = S.qs[pos];
  uint32_t n = 0;
  knn_ball_walk<FMA>(S, q, r2, [&](const float4, const uint32_t j) {      // (j < S.nt: a position of the surface's grid)
    if (gn[j].w == 0.f) return;
    ++n;
    need[j] = 1;
  });
  count[__float_as_uint(q.w)] = n;
}

}  // namespace

int at_indices_ok(Ctx *c, const Cloud &q, const uint32_t *indices, size_t n_indices, const char *fn)
{
  if (!indices) return MVR_OK;
  for (size_t r = 0; r < n_indices; ++r)
    if (indices[r] >= q.n) return set_error(c, MVR_E_ARG, (std::string(fn) + ": an index beyond the query slot (rule Q1)").c_str());
  return MVR_OK;
}

int at_queries(Ctx *c, const Cloud &q, bool with_normals, const uint32_t *indices, size_t n_indices, const KnnSlot &S, AtQueries *out)
{
  const size_t rows = indices ? n_indices : q.n;
  out->rows = rows;
  if (rows == 0) return MVR_OK;
  if (rows > 0x7FFFFFF0ull) return set_error(c, MVR_E_ARG, "too many queries");
  const uint32_t cells = S.dir ? (uint32_t)S.dim[0] * (uint32_t)S.dim[1] * (uint32_t)S.dim[2] : 1u;
  const bool sort = c->at_sort && S.dir && rows > 1;
  int bits = 1;
  while (bits < 32 && (cells >> bits)) ++bits;      // the keys are 0..cells
  size_t sort_bytes = 0;
  if (sort)
    MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (float4 *)nullptr, (float4 *)nullptr,
                                                      (int)rows, 0, bits, c->stream));
  Carver plan;
  plan.plan<float4>(rows); plan.plan<float4>(sort ? rows : 1); plan.plan<uint32_t>(rows); plan.plan<uint32_t>(sort ? rows : 1);
  plan.plan<uint32_t>(indices ? rows : 1); plan.plan<char>(sort_bytes);
  if (out->buf.alloc(plan.off + 256) != hipSuccess) return set_error(c, MVR_E_NOMEM, "the query array: out of device memory");
  Carver s; s.base = out->buf.as<char>();
  float4 *qa = s.take<float4>(rows), *qb = s.take<float4>(sort ? rows : 1);
  uint32_t *ka = s.take<uint32_t>(rows), *kb = s.take<uint32_t>(sort ? rows : 1), *di = s.take<uint32_t>(indices ? rows : 1);
  char *tmp = s.take<char>(sort_bytes);
  if (indices) MVR_HIP_TRY(c, hipMemcpy(di, indices, rows * sizeof(uint32_t), hipMemcpyHostToDevice));      // (the caller's array is read when this returns)
  hipLaunchKernelGGL(at_gather_kernel, dim3(blocks_for(rows, kKnnThreads)), dim3(kKnnThreads), 0, c->stream, q.pts, with_normals ? q.nrm : nullptr,
                     indices ? di : nullptr, (uint32_t)rows, S, cells, qa, ka);
  MVR_HIP_TRY(c, hipGetLastError());
  if (sort) MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, ka, kb, qa, qb, (int)rows, 0, bits, c->stream));
  out->q = sort ? qb : qa;
  return MVR_OK;
}

int launch_at_mark(Ctx *c, const KnnSlot &S, const float4 *gn, float r2, bool fma, uint32_t *count, uint8_t *need)
{
  if (S.nq == 0) return MVR_OK;
  const dim3 grid(blocks_for(S.nq, kKnnThreads)), block(kKnnThreads);
  if (fma) hipLaunchKernelGGL(at_mark_kernel<true>, grid, block, 0, c->stream, S, gn, r2, count, need);
  else hipLaunchKernelGGL(at_mark_kernel<false>, grid, block, 0, c->stream, S, gn, r2, count, need);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

}  // namespace mvr
