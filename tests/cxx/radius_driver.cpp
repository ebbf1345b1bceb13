// tests/cxx/radius_driver.cpp -- drives the C++ layers of the neighbour searches (pcl::search::KdTree in mvr/registration.hpp,
// ScanCloud::radiusSearch in mvr/registrator.hpp) on two small clouds and compares what every overload returns with the lists
// tests/test_gpu_radius_cxx.py computed with tests/radius_ref.py / tests/normals_ref.py and passed in a file; prints the number
// of mismatching rows per check, and the return values, as JSON.
//
// usage: radius_driver <case file>
// the file: u32 nA, nB, n_indices, k, max_nn; f64 radius; f32 A[nA][4], B[nB][4]; i32 indices[n_indices]; then six CSR tables
// (u64 offsets[rows + 1], u32 idx[total], u32 bits of d2[total]):
//   0 radius A in A                 1 radius B[indices] in A, max_nn      2 k-NN B in A (the finite entries)
//   3 radius A in B                 4 k-NN A in A                         5 radius B in A, max_nn
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"

using namespace mvr;

struct Csr {
  std::vector<uint64_t> off;
  std::vector<uint32_t> idx, d2;
  size_t rows() const { return off.size() - 1; }
};

static bool get(FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

static bool read_csr(FILE *f, size_t rows, Csr &c)
{
  c.off.resize(rows + 1);
  if (!get(f, c.off.data(), 8 * (rows + 1))) return false;
  c.idx.resize(c.off[rows]); c.d2.resize(c.off[rows]);
  return get(f, c.idx.data(), 4 * c.idx.size()) && get(f, c.d2.data(), 4 * c.d2.size());
}

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// row r of `want` against one returned list; any_order: as multisets of (d2, index)
static bool row_equal(const Csr &want, size_t r, const std::vector<int> &i, const std::vector<float> &d, bool any_order = false)
{
  const size_t a = want.off[r], m = want.off[r + 1] - a;
  if (i.size() != m || d.size() != m) return false;
  std::vector<uint64_t> x(m), y(m);
  for (size_t e = 0; e < m; ++e) {
    x[e] = ((uint64_t)want.d2[a + e] << 32) | want.idx[a + e];
    y[e] = ((uint64_t)bits(d[e]) << 32) | (uint32_t)i[e];
  }
  if (any_order) { std::sort(x.begin(), x.end()); std::sort(y.begin(), y.end()); }
  return x == y;
}

static size_t mismatches(const Csr &want, const std::vector<std::vector<int> > &vi, const std::vector<std::vector<float> > &vd, bool any_order = false)
{
  if (vi.size() != want.rows() || vd.size() != want.rows()) return want.rows() + 1;
  size_t bad = 0;
  for (size_t r = 0; r < want.rows(); ++r) bad += row_equal(want, r, vi[r], vd[r], any_order) ? 0 : 1;
  return bad;
}

static size_t mismatches(const Csr &want, const NeighborLists &got)
{
  if (got.offsets != want.off || got.indices != want.idx || got.sqr_distances.size() != want.d2.size()) return want.rows() + 1;
  size_t bad = 0;
  for (size_t e = 0; e < want.d2.size(); ++e) bad += bits(got.sqr_distances[e]) == want.d2[e] ? 0 : 1;
  return bad;
}

int main(int argc, char **argv)
{
  if (argc < 2) { std::fprintf(stderr, "usage: %s case-file\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "radius_driver: cannot open %s\n", argv[1]); return 2; }
  uint32_t hdr[5];
  double radius = 0.0;
  if (!get(f, hdr, sizeof hdr) || !get(f, &radius, 8)) return 2;
  const size_t nA = hdr[0], nB = hdr[1], nI = hdr[2];
  const int k = (int)hdr[3];
  const unsigned max_nn = hdr[4];
  pcl::PointCloud<pcl::PointXYZ>::Ptr A(new pcl::PointCloud<pcl::PointXYZ>()), B(new pcl::PointCloud<pcl::PointXYZ>());
  A->resize(nA); B->resize(nB);
  std::vector<int> indices(nI);
  if (!get(f, A->points[0].data, 16 * nA) || !get(f, B->points[0].data, 16 * nB) || !get(f, indices.data(), 4 * nI)) return 2;
  Csr E[6];
  const size_t rows[6] = {nA, nI, nB, nA, nA, nB};
  for (int e = 0; e < 6; ++e)
    if (!read_csr(f, rows[e], E[e])) { std::fprintf(stderr, "radius_driver: short case file (table %d)\n", e); return 2; }
  std::fclose(f);
  try {
    std::printf("{");
    const std::vector<int> all;
    std::vector<std::vector<int> > vi;
    std::vector<std::vector<float> > vd;
    std::vector<int> i1;
    std::vector<float> d1;
    pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
    {   // before setInputCloud: an error, nothing found
      const int r0 = tree->radiusSearch(A->points[0], radius, i1, d1), r1 = tree->nearestKSearch(A->points[0], k, i1, d1);
      tree->radiusSearch(*A, all, radius, vi, vd);
      std::printf("\"no_input\": [%d, %d, %zu, %d], ", r0, r1, vi.size(), (int)(tree->getInputCloud() == nullptr));
    }
    tree->setInputCloud(A);
    std::printf("\"input_is_a\": %d, \"sorted_default\": %d, ", (int)(tree->getInputCloud() == A), (int)tree->getSortedResults());
    // radiusSearch: the batch form over the whole cloud (empty indices), over listed points with max_nn, the three single forms
    tree->radiusSearch(*A, all, radius, vi, vd);
    std::printf("\"radius_batch\": %zu, ", mismatches(E[0], vi, vd));
    tree->radiusSearch(*B, indices, radius, vi, vd, max_nn);
    std::printf("\"radius_batch_indices_max_nn\": %zu, ", mismatches(E[1], vi, vd));
    {
      size_t bad = 0, bad_ret = 0;
      for (size_t j = 0; j < nA; j += 7) {
        int r = tree->radiusSearch((int)j, radius, i1, d1);
        bad += row_equal(E[0], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[0].off[j + 1] - E[0].off[j] ? 0 : 1;
        r = tree->radiusSearch(*A, (int)j, radius, i1, d1);
        bad += row_equal(E[0], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[0].off[j + 1] - E[0].off[j] ? 0 : 1;
        r = tree->radiusSearch(A->points[j], radius, i1, d1);
        bad += row_equal(E[0], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[0].off[j + 1] - E[0].off[j] ? 0 : 1;
      }
      for (size_t j = 0; j < nI; j += 3) {
        const int r = tree->radiusSearch(*B, indices[j], radius, i1, d1, max_nn);
        bad += row_equal(E[1], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[1].off[j + 1] - E[1].off[j] ? 0 : 1;
      }
      std::printf("\"radius_single\": [%zu, %zu], ", bad, bad_ret);
    }
    {   // setSortedResults(false): the same rows as multisets; with max_nn the order of RS3 all the same
      tree->setSortedResults(false);
      tree->radiusSearch(*A, all, radius, vi, vd);
      const size_t sets = mismatches(E[0], vi, vd, true);
      tree->radiusSearch(*B, indices, radius, vi, vd, max_nn);
      std::printf("\"unsorted\": [%zu, %zu, %d], ", sets, mismatches(E[1], vi, vd), (int)tree->getSortedResults());
      tree->setSortedResults(true);
    }
    // nearestKSearch: the batch form, the three single forms, k > MVR_MAX_KNN refused
    tree->nearestKSearch(*B, all, k, vi, vd);
    std::printf("\"knn_batch\": %zu, ", mismatches(E[2], vi, vd));
    {
      size_t bad = 0, bad_ret = 0;
      for (size_t j = 0; j < nB; j += 11) {
        int r = tree->nearestKSearch(B->points[j], k, i1, d1);
        bad += row_equal(E[2], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[2].off[j + 1] - E[2].off[j] ? 0 : 1;
        r = tree->nearestKSearch(*B, (int)j, k, i1, d1);
        bad += row_equal(E[2], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[2].off[j + 1] - E[2].off[j] ? 0 : 1;
      }
      for (size_t j = 0; j < nA; j += 13) {
        const int r = tree->nearestKSearch((int)j, k, i1, d1);
        bad += row_equal(E[4], j, i1, d1) ? 0 : 1; bad_ret += (size_t)r == E[4].off[j + 1] - E[4].off[j] ? 0 : 1;
      }
      std::printf("\"knn_single\": [%zu, %zu], ", bad, bad_ret);
      i1.assign(3, 7); d1.assign(3, 7.f);
      const int big = tree->nearestKSearch(B->points[0], MVR_MAX_KNN + 1, i1, d1);
      const size_t big_left = i1.size() + d1.size();
      tree->nearestKSearch(*B, all, MVR_MAX_KNN + 1, vi, vd);
      const int zero = tree->nearestKSearch(0, 0, i1, d1), outside = tree->radiusSearch((int)nA, radius, i1, d1);
      const int bad_radius = tree->radiusSearch(0, -1.0, i1, d1);
      std::printf("\"refused\": [%d, %zu, %zu, %d, %d, %d], ", big, big_left, vi.size(), zero, outside, bad_radius);
    }
    {   // setInputCloud a second time: the second cloud is the one searched
      tree->setInputCloud(B);
      tree->radiusSearch(*A, all, radius, vi, vd);
      std::printf("\"second_input\": [%zu, %d], ", mismatches(E[3], vi, vd), (int)(tree->getInputCloud() == B));
      pcl::search::KdTree<pcl::PointXYZ> copy(*tree);          // a copy goes on searching the cloud it was copied with
      tree->setInputCloud(A);
      copy.radiusSearch(*A, all, radius, vi, vd);
      const size_t of_copy = mismatches(E[3], vi, vd);
      tree->radiusSearch(*A, all, radius, vi, vd);
      std::printf("\"copy\": [%zu, %zu], ", of_copy, mismatches(E[0], vi, vd));
    }
    {   // a tree handed to a feature class is still ignored by it
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
      pcl::PointCloud<pcl::Normal> normals;
      ne.setInputCloud(B); ne.setSearchMethod(tree); ne.setKSearch(8);
      ne.compute(normals);
      std::printf("\"normals\": %zu, ", normals.size());
    }
    {   // ScanCloud::radiusSearch, a cloud in itself and another cloud's points in it
      ScanCloud a, b;
      a.points = *A; b.points = *B;
      const NeighborLists self = a.radiusSearch(radius), cross = a.radiusSearch(b, radius, max_nn), bad = a.radiusSearch(0.0);
      ScanCloud none;
      const NeighborLists empty = a.radiusSearch(none, radius);
      std::printf("\"scan\": [%zu, %zu, %zu, %zu, %zu, %zu]", mismatches(E[0], self), mismatches(E[5], cross), bad.offsets.size(), bad.rows(),
                  empty.offsets.size(), empty.indices.size());
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "radius_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
