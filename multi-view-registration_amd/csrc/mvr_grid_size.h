// csrc/mvr_grid_size.h -- the sizing of a cloud's own grid (ensure_model_grid, mvr_grid.hip): bounding box and point count in;
// origin, cell edge and cells per axis out; and the layout of the device block every grid's arrays are carved out of
// (ensure_grids, ensure_model_grid).  Plain host C++ with no GPU header, so tests/cxx/grid_size_driver.cpp compiles it alone
// under the sanitizers.  Not installed.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace mvr {

constexpr double kModelGridMaxCells = 32.0e6;
constexpr int kModelGridMaxDim = 513;           // the edge is at least 1 / 512 of the longest extent: floor(512) + 1 cells at most
constexpr size_t kModelGridMinPoints = 4, kModelGridMaxPoints = 0x7FFFFFF0ull;

enum ModelGridStatus {
  kModelGridOk = 0,
  kModelGridEmpty,         // lo > hi on an axis: the box of no point at all (a cloud without a finite point)
  kModelGridRefused        // a non-finite corner, a point count out of range, or an edge that f32 cannot hold
};

struct ModelGridSize {
  float lo[3], h, inv_h;
  double h64;              // the edge before its rounding to f32
  int dim[3];
  size_t cells;
};

// bb = {lo xyz, hi xyz} of the FINITE points, n = the cloud's size, cell_points = the tune key seq_cell_points (points per
// cell aimed at, on a surface).  No conversion to int of a value that is not known to lie in [0, 512]: a NaN or an infinity in
// the box is refused before any arithmetic, and the quotient ext / h is bounded by construction and checked all the same.
inline ModelGridStatus model_grid_size(const float bb[6], size_t n, int cell_points, ModelGridSize *out)
{
  for (int j = 0; j < 6; ++j) if (!std::isfinite(bb[j])) return kModelGridRefused;
  for (int j = 0; j < 3; ++j) if (bb[j] > bb[3 + j]) return kModelGridEmpty;
  if (n < kModelGridMinPoints || n > kModelGridMaxPoints) return kModelGridRefused;
  double ext[3];
  for (int j = 0; j < 3; ++j) { out->lo[j] = bb[j]; ext[j] = std::max(1e-6, (double)bb[3 + j] - (double)bb[j]); }
  const double area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2];
  double h = std::sqrt((double)std::max(1, cell_points) * area / (double)n);
  h = std::max(h, std::max(ext[0], std::max(ext[1], ext[2])) / 512.0);
  for (;;) {
    if (!(h > 0.0) || !std::isfinite(h)) return kModelGridRefused;
    double cells = 1.0;
    for (int j = 0; j < 3; ++j) {
      const double q = std::floor(ext[j] / h);
      if (!(q >= 0.0 && q <= (double)(kModelGridMaxDim - 1))) return kModelGridRefused;
      out->dim[j] = (int)q + 1;
      cells *= (double)out->dim[j];
    }
    if (cells <= kModelGridMaxCells) break;
    h *= 1.25;
  }
  // the walks multiply by inv_h and divide by it: both must be ordinary f32 numbers (checked before the conversion)
  if (!(h >= 1.0e-30 && h <= 1.0e30)) return kModelGridRefused;
  out->h64 = h; out->h = (float)h; out->inv_h = (float)(1.0 / h);
  out->cells = (size_t)out->dim[0] * (size_t)out->dim[1] * (size_t)out->dim[2];
  return kModelGridOk;
}

// ---- where the arrays of a grid lie in its ONE device block (CellGrid::block): byte offsets, each a multiple of 256, in
// ascending order, and the block's size.  A scan's grid keeps its cell starts as the dense table or as the compact one
// (directory + records) and carries the maps between grid order and Hilbert order; a cloud's own grid (ensure_model_grid) is
// compact, holds four points more (its walks read four at a time) and has no Hilbert maps.
enum GridBlockForm { kGridBlockDense, kGridBlockCompact, kGridBlockModel };
// the eight entries behind start[cells] (the walk reads four consecutive starts with one load, the staged walk eight with two): all n
constexpr size_t kStartPad = 8;
constexpr size_t kGridBlockNone = ~(size_t)0;      // the form has no such array
struct GridBlockLayout {
  size_t start, dir, recs;       // uint32 [cells + 1 + kStartPad] | [nseg + 2], [32 x (min(n, nseg + 1) + 1)]
  size_t gperm, graw;            // uint32 [n], float4 [n] (model: [n + 4])
  size_t g2h, h2g;               // uint32 [n] each (scan grids)
  size_t dt;                     // uint8 [cells2]: the distance map per 2 x 2 x 2 cells
  size_t total;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline GridBlockLayout grid_block_layout(size_t n, size_t cells, size_t cells2, size_t nseg, GridBlockForm form)
{
  GridBlockLayout l;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
  l.start = l.dir = l.recs = l.g2h = l.h2g = kGridBlockNone;
  if (form == kGridBlockDense) l.start = take((cells + 1 + kStartPad) * 4);
  else { l.dir = take((nseg + 2) * 4); l.recs = take((std::min(n, nseg + 1) + 1) * 32 * 4); }
  l.gperm = take(n * 4);
  l.graw = take((form == kGridBlockModel ? n + 4 : n) * 16);
  if (form != kGridBlockModel) { l.g2h = take(n * 4); l.h2g = take(n * 4); }
  l.dt = take(cells2);
  l.total = at;
  return l;
}

}  // namespace mvr
