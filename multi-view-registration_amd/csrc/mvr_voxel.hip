// csrc/mvr_voxel.hip -- pcl::VoxelGrid<PointXYZ>::filter on the GPU (mvr_cloud_voxel_grid; the rules are written next to
// its declaration in mvr_hip.h).
//
//   1. bounding box and count of the finite points: the one read-back before the sort -- the host needs the box for
//      PCL's overflow rule and for the number of key bits;
//   2. voxel index of every finite point in PCL's f32 arithmetic, as a 64-bit integer (kept in 32 bits when the largest
//      index fits); a non-finite point gets one past the largest index and sorts behind every voxel;
//   3. one hipCUB pair sort (index, point) over exactly the bits the index needs.  The sort is stable: a voxel's
//      members stay in ascending point order;
//   4. segment heads and an inclusive scan: the voxel number of every sorted position;
//   5. per-voxel f64 sums in a FIXED order (no float atomics: bit-identical from run to run).  The head thread of a
//      voxel of up to kShort points sums them itself, in point order.  A longer voxel is cut into pieces of kPiece
//      sorted positions; one block sums a piece (strided per thread, then a fixed LDS tree) and one thread adds the
//      pieces in order.  A voxel that holds the whole cloud is spread over the GPU instead of serialised in one thread;
//   6. kept voxels (count >= min_points) compacted by a second scan, in ascending index; the voxel map of every point.
// The read-back of the output count (with the voxel map) is the second and last host synchronisation.
// HBM/latency-bound integer work and a sort; nothing here is reshaped into a GEMM.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvr_internal.h"

namespace mvr {
namespace {

constexpr int kVoxThreads = 256;
constexpr int kBoxBlocks = 256;
constexpr uint32_t kShort = 64;       // voxels of up to this many points are summed by their head thread
constexpr uint32_t kPiece = 4096;     // sorted positions one block sums of a longer voxel (16 per thread)
constexpr unsigned kPieceGrid = 2048; // blocks of the piece launch (grid-stride over the pieces)

static_assert(kBoxBlocks <= kVoxThreads, "the final box reduction takes one partial record per thread");

__device__ __forceinline__ void box_reduce(const float lo[3], const float hi[3], uint32_t cnt, float *__restrict__ rec);

// part[block][8]: lo xyz, hi xyz of the finite points, their count (bits), unused
__global__ __launch_bounds__(kVoxThreads) void vox_box_partial_kernel(const float4 *__restrict__ p, size_t n, float *__restrict__ part)
{
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  uint32_t cnt = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float4 v = p[i];
    if (!finite3(v)) continue;
    ++cnt;
    lo[0] = fminf(lo[0], v.x); lo[1] = fminf(lo[1], v.y); lo[2] = fminf(lo[2], v.z);
    hi[0] = fmaxf(hi[0], v.x); hi[1] = fmaxf(hi[1], v.y); hi[2] = fmaxf(hi[2], v.z);
  }
  box_reduce(lo, hi, cnt, part + blockIdx.x * 8);
}

// the block's lo / hi / count -> rec[0..7] (LDS tree)
__device__ __forceinline__ void box_reduce(const float lo[3], const float hi[3], uint32_t cnt, float *__restrict__ rec)
{
  __shared__ float s[6][kVoxThreads];
  __shared__ uint32_t sc[kVoxThreads];
  const int t = threadIdx.x;
  for (int k = 0; k < 3; ++k) { s[k][t] = lo[k]; s[3 + k][t] = hi[k]; }
  sc[t] = cnt;
  __syncthreads();
  for (int o = kVoxThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      for (int k = 0; k < 3; ++k) {
        s[k][t] = fminf(s[k][t], s[k][t + o]);
        s[3 + k][t] = fmaxf(s[3 + k][t], s[3 + k][t + o]);
      }
      sc[t] += sc[t + o];
    }
    __syncthreads();
  }
  if (t < 6) rec[t] = s[t][0];
  if (t == 6) rec[6] = __uint_as_float(sc[0]);
  if (t == 7) rec[7] = 0.f;
}

// one block of kVoxThreads over the (<= kVoxThreads) partial records: a thread per record, then the same tree
__global__ __launch_bounds__(kVoxThreads) void vox_box_final_kernel(const float *__restrict__ part, int blocks, float *__restrict__ out /* 8 */)
{
  const int t = threadIdx.x;
  const bool live = t < blocks;
  float lo[3], hi[3];
  for (int k = 0; k < 3; ++k) { lo[k] = live ? part[t * 8 + k] : INFINITY; hi[k] = live ? part[t * 8 + 3 + k] : -INFINITY; }
  box_reduce(lo, hi, live ? __float_as_uint(part[t * 8 + 6]) : 0u, out);
}

// PCL's voxel arithmetic (voxel_grid.cpp, applyFilter): ijk = floor(p * inv) - (float)min_b in f32, idx in 64 bits
struct VoxGeom {
  float inv[3], minbf[3];
  unsigned long long div0, div01, sentinel;
};

template <class K>
__global__ __launch_bounds__(kVoxThreads) void vox_key_kernel(const float4 *__restrict__ p, size_t n, VoxGeom g, K *__restrict__ key,
                                                               uint32_t *__restrict__ idx)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 v = p[i];
  unsigned long long k = g.sentinel;
  if (finite3(v)) {
    // (f32 products by inv, never contracted: -ffp-contract=off; the difference is a non-negative f32 integer)
    const unsigned long long i0 = (unsigned long long)(floorf(v.x * g.inv[0]) - g.minbf[0]);
    const unsigned long long i1 = (unsigned long long)(floorf(v.y * g.inv[1]) - g.minbf[1]);
    const unsigned long long i2 = (unsigned long long)(floorf(v.z * g.inv[2]) - g.minbf[2]);
    k = i0 + i1 * g.div0 + i2 * g.div01;
  }
  key[i] = (K)k;
  idx[i] = (uint32_t)i;
}

template <class K>
__global__ __launch_bounds__(kVoxThreads) void vox_head_kernel(const K *__restrict__ key, size_t nf, uint32_t *__restrict__ head)
{
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nf) return;
  head[j] = (j == 0 || key[j] != key[j - 1]) ? 1u : 0u;
}

__device__ __forceinline__ float4 vox_centroid(const double *s, uint32_t cnt)
{
  const double c = (double)cnt;
  return make_float4((float)(s[0] / c), (float)(s[1] / c), (float)(s[2] / c), 1.0f);
}

// the f64 sum normalised in f64: a zero sum stays zero, a NaN member gives NaN
__device__ __forceinline__ float4 vox_unit(const double *s)
{
  const double l = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  if (l == 0.0) return make_float4(0.f, 0.f, 0.f, 0.f);
  return make_float4((float)(s[0] / l), (float)(s[1] / l), (float)(s[2] / l), 0.f);
}

struct LongRec { uint32_t head, cnt, base, pieces; };

// One thread per sorted position; the head of a voxel finds its end (gallop, then bisect over the sorted keys), decides
// whether the voxel is kept, and sums it (short) or hands it to the piece launch (long).  keep[] is by position (1 at
// the head of a kept voxel); cent[] / cnrm[] by head position.
template <class K, bool NRM>
__global__ __launch_bounds__(kVoxThreads) void vox_voxel_kernel(const K *__restrict__ key, const uint32_t *__restrict__ sidx, size_t nf,
                                                                 const float4 *__restrict__ pts, const float4 *__restrict__ nrm,
                                                                 uint32_t min_points, uint32_t *__restrict__ keep, float4 *__restrict__ cent,
                                                                 float4 *__restrict__ cnrm, LongRec *__restrict__ longs,
                                                                 uint2 *__restrict__ pieces, uint32_t *__restrict__ counters)
{
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nf) return;
  const K kj = key[j];
  if (j > 0 && key[j - 1] == kj) { keep[j] = 0u; return; }
  size_t lo = j, step = 1;                    // key[lo] == kj
  while (j + step < nf && key[j + step] == kj) { lo = j + step; step <<= 1; }
  size_t hi = j + step < nf ? j + step : nf;  // key[hi] != kj, or hi == nf
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (key[mid] == kj) lo = mid; else hi = mid;
  }
  const uint32_t cnt = (uint32_t)(hi - j);
  const bool kept = cnt >= min_points;
  keep[j] = kept ? 1u : 0u;
  if (!kept) return;
  if (cnt <= kShort) {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t i = sidx[j + k];
      const float4 v = pts[i];
      s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z;
      if (NRM) { const float4 w = nrm[i]; s[3] += (double)w.x; s[4] += (double)w.y; s[5] += (double)w.z; }
    }
    cent[j] = vox_centroid(s, cnt);
    if (NRM) cnrm[j] = vox_unit(s + 3);
    return;
  }
  const uint32_t np = (cnt + kPiece - 1) / kPiece;
  const uint32_t li = atomicAdd(&counters[0], 1u), base = atomicAdd(&counters[1], np);
  LongRec r; r.head = (uint32_t)j; r.cnt = cnt; r.base = base; r.pieces = np;
  longs[li] = r;
  const uint32_t end = (uint32_t)j + cnt;
  for (uint32_t q = 0; q < np; ++q) {
    const uint32_t b = (uint32_t)j + q * kPiece;
    pieces[base + q] = make_uint2(b, end - b > kPiece ? b + kPiece : end);      // sorted positions [b, e)
  }
}

// one block per piece (grid-stride): partial[piece][0..5] = sums of the piece, each thread over positions t, t + 256, ...
// in order, then a fixed LDS tree -- the same bits whichever block takes the piece
template <bool NRM>
__global__ __launch_bounds__(kVoxThreads) void vox_piece_kernel(const uint2 *__restrict__ pieces, const uint32_t *__restrict__ counters,
                                                                 const uint32_t *__restrict__ sidx, const float4 *__restrict__ pts,
                                                                 const float4 *__restrict__ nrm, double *__restrict__ partial)
{
  constexpr int C = NRM ? 6 : 3;
  __shared__ double red[C][kVoxThreads];
  const uint32_t np = counters[1];
  const int t = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < np; q += gridDim.x) {
    const uint2 pc = pieces[q];
    double s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.0;
    for (uint32_t k = pc.x + (uint32_t)t; k < pc.y; k += kVoxThreads) {
      const uint32_t i = sidx[k];
      const float4 v = pts[i];
      s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z;
      if (NRM) { const float4 w = nrm[i]; s[C - 3] += (double)w.x; s[C - 2] += (double)w.y; s[C - 1] += (double)w.z; }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) red[c][t] = s[c];
    __syncthreads();
    for (int o = kVoxThreads / 2; o > 0; o >>= 1) {
      if (t < o)
#pragma unroll
        for (int c = 0; c < C; ++c) red[c][t] += red[c][t + o];
      __syncthreads();
    }
    if (t < C) partial[(size_t)q * 8 + t] = red[t][0];
    __syncthreads();                          // red[] is reused by the block's next piece
  }
}

// one thread per long voxel: its pieces added in order
template <bool NRM>
__global__ __launch_bounds__(kVoxThreads) void vox_long_kernel(const LongRec *__restrict__ longs, const uint32_t *__restrict__ counters,
                                                                const double *__restrict__ partial, float4 *__restrict__ cent,
                                                                float4 *__restrict__ cnrm)
{
  const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= counters[0]) return;
  const LongRec r = longs[li];
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t q = 0; q < r.pieces; ++q)
    for (int c = 0; c < (NRM ? 6 : 3); ++c) s[c] += partial[(size_t)(r.base + q) * 8 + c];
  cent[r.head] = vox_centroid(s, r.cnt);
  if (NRM) cnrm[r.head] = vox_unit(s + 3);
}

// kept voxels to their output positions (kpos = inclusive scan of keep); vmap[voxel] = output position or kNone
template <bool NRM>
__global__ __launch_bounds__(kVoxThreads) void vox_out_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ vid,
                                                               const uint32_t *__restrict__ keep, const uint32_t *__restrict__ kpos, size_t nf,
                                                               const float4 *__restrict__ cent, const float4 *__restrict__ cnrm,
                                                               float4 *__restrict__ out, float4 *__restrict__ onrm, uint32_t *__restrict__ vmap,
                                                               uint32_t *__restrict__ counters)
{
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nf) return;
  if (j == nf - 1) counters[2] = kpos[j];     // the output count
  if (!head[j]) return;
  const uint32_t v = vid[j] - 1u;
  if (keep[j]) {
    const uint32_t o = kpos[j] - 1u;
    out[o] = cent[j];
    if (NRM) onrm[o] = cnrm[j];
    vmap[v] = o;
  } else {
    vmap[v] = kNone;
  }
}

// voxel_of[original index] for every sorted position (non-finite points sit behind position nf)
__global__ __launch_bounds__(kVoxThreads) void vox_map_kernel(const uint32_t *__restrict__ sidx, const uint32_t *__restrict__ vid,
                                                               const uint32_t *__restrict__ vmap, size_t n, size_t nf,
                                                               uint32_t *__restrict__ voxel_of)
{
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  voxel_of[sidx[j]] = j < nf ? vmap[vid[j] - 1u] : kNone;
}

template <class K, bool NRM>
int voxel_pass(Ctx *c, const Cloud &src, size_t nf, const VoxGeom &g, int bits, unsigned min_points, Carver &s, size_t sort_bytes,
               size_t scan_bytes, uint32_t *counters, float4 **out, float4 **onrm, uint32_t **d_voxel_of, bool want_map)
{
  const size_t n = src.n;
  K *key_a = s.take<K>(n), *key_b = s.take<K>(n);
  uint32_t *idx_a = s.take<uint32_t>(n), *idx_b = s.take<uint32_t>(n);
  uint32_t *head = s.take<uint32_t>(nf), *vid = s.take<uint32_t>(nf), *keep = s.take<uint32_t>(nf), *kpos = s.take<uint32_t>(nf),
           *vmap = s.take<uint32_t>(nf);
  float4 *cent = s.take<float4>(nf), *cnrm = NRM ? s.take<float4>(nf) : nullptr;
  *out = s.take<float4>(nf);
  *onrm = NRM ? s.take<float4>(nf) : nullptr;
  const size_t max_long = nf / (kShort + 1) + 1, max_pieces = nf / kPiece + max_long;
  LongRec *longs = s.take<LongRec>(max_long);
  uint2 *pieces = s.take<uint2>(max_pieces);
  double *partial = s.take<double>(max_pieces * 8);
  *d_voxel_of = want_map ? s.take<uint32_t>(n) : nullptr;
  char *tmp = s.take<char>(std::max(sort_bytes, scan_bytes));
  hipLaunchKernelGGL(vox_key_kernel<K>, dim3(blocks_for(n, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, src.pts, n, g, key_a, idx_a);
  MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, key_a, key_b, idx_a, idx_b, n, 0, bits, c->stream));
  hipLaunchKernelGGL(vox_head_kernel<K>, dim3(blocks_for(nf, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, key_b, nf, head);
  size_t b = scan_bytes;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(tmp, b, head, vid, nf, c->stream));
  hipLaunchKernelGGL((vox_voxel_kernel<K, NRM>), dim3(blocks_for(nf, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, key_b, idx_b, nf, src.pts,
                     (const float4 *)src.nrm, (uint32_t)min_points, keep, cent, cnrm, longs, pieces, counters);
  hipLaunchKernelGGL(vox_piece_kernel<NRM>, dim3((unsigned)std::min<size_t>(max_pieces, kPieceGrid)), dim3(kVoxThreads), 0, c->stream,
                     pieces, counters, idx_b, src.pts, (const float4 *)src.nrm, partial);
  hipLaunchKernelGGL(vox_long_kernel<NRM>, dim3(blocks_for(max_long, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, longs, counters, partial, cent, cnrm);
  b = scan_bytes;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(tmp, b, keep, kpos, nf, c->stream));
  hipLaunchKernelGGL(vox_out_kernel<NRM>, dim3(blocks_for(nf, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, head, vid, keep, kpos, nf, cent, cnrm,
                     *out, *onrm, vmap, counters);
  if (want_map)
    hipLaunchKernelGGL(vox_map_kernel, dim3(blocks_for(n, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, idx_b, vid, vmap, n, nf, *d_voxel_of);
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

template <class K>
size_t sort_temp_bytes(Ctx *c, size_t n)
{
  size_t bytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (K *)nullptr, (K *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, n, 0,
                                           (int)(8 * sizeof(K)), c->stream);
  return bytes;
}

}  // namespace

// steps 1-3 of voxel_grid_cloud: the finite box and count (the one read-back before the sort), PCL's overflow rule and the
// geometry of the index.  part / box: 8 * kBoxBlocks and 8 floats of scratch.
static int voxel_lattice(Ctx *c, const Cloud &src, const float inv[3], float *part, float *box, VoxLattice *L)
{
  const size_t n = src.n;
  // 1. finite box + count
  const int bb = (int)std::min<size_t>(kBoxBlocks, blocks_for(n, kVoxThreads));
  hipLaunchKernelGGL(vox_box_partial_kernel, dim3(bb), dim3(kVoxThreads), 0, c->stream, src.pts, n, part);
  hipLaunchKernelGGL(vox_box_final_kernel, dim3(1), dim3(kVoxThreads), 0, c->stream, part, bb, box);
  MVR_HIP_TRY(c, hipGetLastError());
  float hb[8];
  MVR_HIP_TRY(c, hipMemcpyAsync(hb, box, sizeof hb, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint32_t nf32;
  std::memcpy(&nf32, &hb[6], 4);
  L->nf = nf32;
  L->pass = false;
  if (nf32 == 0) return MVR_OK;
  // 2. PCL's overflow rule, in f32 as PCL computes it: (max_p - min_p) * inv per axis, truncated, + 1.  A product that is not
  // below 2^31 (NaN included), or a bound product whose integer does not fit in 62 bits, takes the same exit (no cast overflows)
  bool pass = false;
  long long d[3], min_b[3], max_b[3];
  for (int a = 0; a < 3; ++a) {
    const float range = hb[3 + a] - hb[a], prod = range * inv[a];
    const float lo = hb[a] * inv[a], hi = hb[3 + a] * inv[a];
    if (!(prod < 0x1p31f) || !(std::fabs(lo) < 0x1p62f) || !(std::fabs(hi) < 0x1p62f)) { pass = true; break; }
    d[a] = (long long)prod + 1;
    min_b[a] = (long long)std::floor(lo);
    max_b[a] = (long long)std::floor(hi);
  }
  if (!pass && (d[0] * d[1] > 2147483647ll || d[0] * d[1] * d[2] > 2147483647ll)) pass = true;
  // 3. geometry of the index: div = max_b - min_b + 1; the largest ijk of an axis is the f32 difference of its bounds (a
  // point's difference cannot exceed it: the f32 operations are monotonic).  Two distinct f32 bounds differ by at least half an
  // ulp of the larger, and each bound product is rounded by at most half an ulp, so div[a] stays within a small multiple of
  // d[a] (about 5 d[a] + 3): with d0 d1 d2 <= 2^31 the index needs about 40 bits.  An index that would not fit in 64 bits
  // takes the pass-through exit all the same (the last guard of rule 3 in mvr_hip.h) rather than wrap.
  unsigned __int128 max_key = 0, div[3] = {1, 1, 1}, top[3] = {0, 0, 0};
  if (!pass) {
    for (int a = 0; a < 3; ++a) {
      L->inv[a] = inv[a];
      L->minbf[a] = (float)min_b[a];
      div[a] = (unsigned __int128)(max_b[a] - min_b[a] + 1);
      top[a] = (unsigned __int128)(unsigned long long)((float)max_b[a] - (float)min_b[a]);
    }
    max_key = top[0] + top[1] * div[0] + top[2] * div[0] * div[1];
    if (max_key + 1 >= ((unsigned __int128)1 << 64)) pass = true;
  }
  L->pass = pass;
  if (pass) return MVR_OK;
  for (int a = 0; a < 3; ++a) L->div[a] = (unsigned long long)div[a];
  L->sentinel = (unsigned long long)(max_key + 1);      // non-finite points: behind every voxel
  L->bits = 1;
  while (L->bits < 64 && (L->sentinel >> L->bits) != 0) ++L->bits;
  return MVR_OK;
}

namespace {
VoxGeom geom_of(const VoxLattice &L)
{
  VoxGeom g;
  for (int a = 0; a < 3; ++a) { g.inv[a] = L.inv[a]; g.minbf[a] = L.minbf[a]; }
  g.div0 = L.div[0];
  g.div01 = L.div[0] * L.div[1];
  g.sentinel = L.sentinel;
  return g;
}
}  // namespace

int voxel_grid_cloud(Ctx *c, Cloud &dst, Cloud &src, const float leaf[3], unsigned min_points, size_t *n_out, uint32_t *voxel_of,
                     int *passthrough)
{
  const size_t n = src.n;
  if (n > 0xFFFFFFF0ull) return set_error(c, MVR_E_ARG, "mvr_cloud_voxel_grid: cloud too large for 32-bit indices");
  if (src.pts_stale) return set_error(c, MVR_E_ARG, "mvr_cloud_voxel_grid: the source's points are not current (pipelined run)");
  const bool same = &dst == &src, normals = src.has_normals;
  float inv[3];
  for (int a = 0; a < 3; ++a) inv[a] = 1.0f / leaf[a];
  if (n == 0) {
    finish_dst(c, dst, 0, false);
    if (n_out) *n_out = 0;
    if (passthrough) *passthrough = 0;
    return MVR_OK;
  }
  MVR_MAY_BLOCK(c, "mvr_cloud_voxel_grid reads back");
  // scratch: one grow-only arena per context, shared with mvr_cloud_denoise.  Both run on the context's stream, and this call
  // returns with its copies out of the arena still queued there: a later call that grows the arena synchronises the stream
  // before it frees the old buffer (ensure()), so stream order is what keeps the arena safe -- a user on another stream
  // would have to wait for c->stream first.
  size_t scan_bytes = 0;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, n, c->stream));
  const size_t sort_bytes = std::max(sort_temp_bytes<uint32_t>(c, n), sort_temp_bytes<unsigned long long>(c, n));
  const size_t max_long = n / (kShort + 1) + 1, max_pieces = n / kPiece + max_long;
  Carver plan;
  plan.plan<float>(8 * kBoxBlocks); plan.plan<float>(8); plan.plan<uint32_t>(4);
  plan.plan<unsigned long long>(n); plan.plan<unsigned long long>(n);
  for (int k = 0; k < 8; ++k) plan.plan<uint32_t>(n);
  for (int k = 0; k < 4; ++k) plan.plan<float4>(n);
  plan.plan<LongRec>(max_long); plan.plan<uint2>(max_pieces); plan.plan<double>(max_pieces * 8);
  plan.plan<char>(std::max(sort_bytes, scan_bytes));
  if (int rc = ensure(c, c->dn_arena, c->dn_arena_cap, plan.off + 256)) return rc;
  Carver s; s.base = c->dn_arena;
  float *part = s.take<float>(8 * kBoxBlocks), *box = s.take<float>(8);
  uint32_t *counters = s.take<uint32_t>(4);
  MVR_HIP_TRY(c, hipMemsetAsync(counters, 0, 4 * sizeof(uint32_t), c->stream));
  VoxLattice lat;
  if (int rc = voxel_lattice(c, src, inv, part, box, &lat)) return rc;
  const size_t nf = lat.nf;
  if (nf == 0) {                                        // no finite point: no voxel
    finish_dst(c, dst, 0, false);
    if (voxel_of) std::fill(voxel_of, voxel_of + n, kNone);
    if (n_out) *n_out = 0;
    if (passthrough) *passthrough = 0;
    return MVR_OK;
  }
  const bool pass = lat.pass;
  if (pass) {                                           // a copy of the input: every point, normals included
    if (!same) {
      dst.n = 0;
      if (int rc = cloud_reserve(c, dst, n, false)) return rc;
      MVR_HIP_TRY(c, hipMemcpyAsync(dst.pts, src.pts, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
      if (normals) {
        if (int rc = ensure(c, dst.nrm, dst.nrm_cap, n)) return rc;
        MVR_HIP_TRY(c, hipMemcpyAsync(dst.nrm, src.nrm, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
      }
    }
    finish_dst(c, dst, n, normals);
    if (voxel_of) for (size_t i = 0; i < n; ++i) voxel_of[i] = (uint32_t)i;
    if (n_out) *n_out = n;
    if (passthrough) *passthrough = 1;
    return MVR_OK;
  }
  const VoxGeom g = geom_of(lat);
  const int bits = lat.bits;
  const bool k32 = g.sentinel <= 0xFFFFFFFFull;
  float4 *out = nullptr, *onrm = nullptr;
  uint32_t *d_map = nullptr;
  const bool want_map = voxel_of != nullptr;
  int rc;
  if (k32) rc = normals ? voxel_pass<uint32_t, true>(c, src, nf, g, bits, min_points, s, sort_bytes, scan_bytes, counters, &out, &onrm, &d_map, want_map)
                        : voxel_pass<uint32_t, false>(c, src, nf, g, bits, min_points, s, sort_bytes, scan_bytes, counters, &out, &onrm, &d_map, want_map);
  else rc = normals ? voxel_pass<unsigned long long, true>(c, src, nf, g, bits, min_points, s, sort_bytes, scan_bytes, counters, &out, &onrm, &d_map, want_map)
                    : voxel_pass<unsigned long long, false>(c, src, nf, g, bits, min_points, s, sort_bytes, scan_bytes, counters, &out, &onrm, &d_map, want_map);
  if (rc) return rc;
  uint32_t hc[4];
  MVR_HIP_TRY(c, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, c->stream));
  if (want_map) MVR_HIP_TRY(c, hipMemcpyAsync(voxel_of, d_map, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t kept = hc[2];
  // 4. the kept voxels become dst's points (stream-ordered copies out of the arena)
  if (!same) {
    dst.n = 0;
    if (int rc2 = cloud_reserve(c, dst, kept, false)) return rc2;
  }
  if (kept) {
    MVR_HIP_TRY(c, hipMemcpyAsync(dst.pts, out, kept * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    if (normals) {
      if (int rc2 = ensure(c, dst.nrm, dst.nrm_cap, kept)) return rc2;
      MVR_HIP_TRY(c, hipMemcpyAsync(dst.nrm, onrm, kept * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    }
  }
  finish_dst(c, dst, kept, normals);
  if (n_out) *n_out = kept;
  if (passthrough) *passthrough = 0;
  return MVR_OK;
}

// ---- steps 1-4 alone, for a cubic leaf and always with 64-bit keys (mvr_internal.h)
void voxel_sorted_plan(Ctx *c, size_t n, Carver &plan)
{
  size_t scan_bytes = 0;
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, n, c->stream);
  plan.plan<float>(8 * kBoxBlocks); plan.plan<float>(8);
  plan.plan<unsigned long long>(n); plan.plan<unsigned long long>(n);
  for (int k = 0; k < 4; ++k) plan.plan<uint32_t>(n);
  plan.plan<char>(std::max(sort_temp_bytes<unsigned long long>(c, n), scan_bytes));
}

int voxel_sorted_index(Ctx *c, const Cloud &src, float leaf, Carver &s, VoxLattice *lat, VoxSorted *out)
{
  const size_t n = src.n;
  if (n == 0 || n > 0xFFFFFFF0ull) return set_error(c, MVR_E_ARG, "voxel index: an empty cloud, or one too large for 32-bit indices");
  if (src.pts_stale) return set_error(c, MVR_E_ARG, "voxel index: the cloud's points are not current (pipelined run)");
  const float i1 = 1.0f / leaf, inv[3] = {i1, i1, i1};
  size_t scan_bytes = 0;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, n, c->stream));
  size_t sort_bytes = sort_temp_bytes<unsigned long long>(c, n);
  float *part = s.take<float>(8 * kBoxBlocks), *box = s.take<float>(8);
  unsigned long long *key_a = s.take<unsigned long long>(n), *key_b = s.take<unsigned long long>(n);
  uint32_t *idx_a = s.take<uint32_t>(n), *idx_b = s.take<uint32_t>(n), *head = s.take<uint32_t>(n), *vid = s.take<uint32_t>(n);
  char *tmp = s.take<char>(std::max(sort_bytes, scan_bytes));
  MVR_MAY_BLOCK(c, "the voxel index reads back");
  if (int rc = voxel_lattice(c, src, inv, part, box, lat)) return rc;
  out->key = key_b; out->idx = idx_b; out->head = head; out->vid = vid;
  if (lat->nf == 0 || lat->pass) return MVR_OK;
  const size_t nf = lat->nf;
  hipLaunchKernelGGL(vox_key_kernel<unsigned long long>, dim3(blocks_for(n, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, src.pts, n,
                     geom_of(*lat), key_a, idx_a);
  MVR_HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, key_a, key_b, idx_a, idx_b, n, 0, lat->bits, c->stream));
  hipLaunchKernelGGL(vox_head_kernel<unsigned long long>, dim3(blocks_for(nf, kVoxThreads)), dim3(kVoxThreads), 0, c->stream, key_b, nf, head);
  size_t b = scan_bytes;
  MVR_HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(tmp, b, head, vid, nf, c->stream));
  MVR_HIP_TRY(c, hipGetLastError());
  return MVR_OK;
}

}  // namespace mvr
