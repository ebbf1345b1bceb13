// tests/cxx/mls_driver.cpp -- drives the C++ layers of the moving-least-squares smoothing (pcl::MovingLeastSquares in
// mvr/registration.hpp, ScanCloud::smooth and the smoothing overload of Registrator::saveRegisteredPoints in
// mvr/registrator.hpp) on synthetic turntable scans and prints what they return as JSON; tests/test_gpu_mls_cxx.py compares
// it with the Python path (Context.mls) on the same scans and on the files written here.
//
// usage: mls_driver <views> <points> <config_id> <folder>      (<folder>/raw, /mls, /mls_vox and /bad must exist)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"

using namespace mvr;

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static void u32s(const char *key, const std::vector<uint32_t> &v, bool last = false)
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%u" : "%u", v[i]);
  std::printf(last ? "]" : "], ");
}

int main(int argc, char **argv)
{
  if (argc < 5) { std::fprintf(stderr, "usage: %s views points config folder\n", argv[0]); return 2; }
  const int V = std::atoi(argv[1]);
  const size_t N = (size_t)std::atol(argv[2]);
  const int config = std::atoi(argv[3]);
  const std::string folder = argv[4];
  try {
    mvr_synth_params sp;
    mvr_synth_default(&sp, V, config);
    TurntableModel model;
    model.views.resize(V);
    for (int v = 0; v < V; ++v) {
      ScanCloud &pc = model.views[v];
      pc.view = v;
      pc.points.resize(N);
      std::vector<float> nrm(4 * N);
      if (mvr_synth_view(&sp, v, N, pc.points.points[0].data, nrm.data()) != MVR_OK) return 3;
      pc.rich.resize(N);
      for (size_t i = 0; i < N; ++i) {      // colours, the analytic normals and (as curvature) the original index ride along
        io::RichPoint &q = pc.rich[i];
        q.x = pc.points.points[i].x; q.y = pc.points.points[i].y; q.z = pc.points.points[i].z;
        q.r = (uint8_t)v; q.g = (uint8_t)(i % 251); q.b = (uint8_t)(255 - v);
        q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2]; q.curvature = (float)i;
      }
    }
    std::printf("{");
    {   // pcl::MovingLeastSquares, PCL's tutorial call for call
      pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(model.views[0].points));
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
      pcl::PointCloud<pcl::PointNormal> out;
      pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> mls;
      std::printf("\"defaults\": [%d, %d], ", mls.getPolynomialOrder(), (int)mls.getPolynomialFit());
      mls.setComputeNormals(true);
      mls.setInputCloud(cloud);
      mls.setPolynomialFit(true);
      mls.setSearchMethod(tree);
      mls.setSearchRadius(1.2);
      std::printf("\"gauss\": %.17g, ", mls.getSqrGaussParam());
      mls.process(out);
      std::vector<uint32_t> xyz, nrm, curv, idx;
      for (size_t i = 0; i < out.size(); ++i) {
        xyz.push_back(bits(out[i].x)); xyz.push_back(bits(out[i].y)); xyz.push_back(bits(out[i].z));
        nrm.push_back(bits(out[i].normal_x)); nrm.push_back(bits(out[i].normal_y)); nrm.push_back(bits(out[i].normal_z));
        curv.push_back(bits(out[i].curvature));
      }
      for (int i : mls.getCorrespondingIndices()->indices) idx.push_back((uint32_t)i);
      u32s("mls_xyz", xyz); u32s("mls_nrm", nrm); u32s("mls_curv", curv); u32s("mls_idx", idx);
      // order 1 into the input cloud itself
      pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointXYZ> plane;
      plane.setInputCloud(cloud); plane.setSearchRadius(1.2); plane.setPolynomialOrder(1);
      plane.process(*cloud);
      xyz.clear();
      for (size_t i = 0; i < cloud->size(); ++i) { xyz.push_back(bits((*cloud)[i].x)); xyz.push_back(bits((*cloud)[i].y)); xyz.push_back(bits((*cloud)[i].z)); }
      u32s("plane_inplace_xyz", xyz);
      // refusals: no input; a radius that was never set
      pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> none, bad;
      none.process(out);
      const size_t n_none = out.size();
      bad.setInputCloud(cloud);
      bad.process(out);
      std::printf("\"none\": %zu, \"bad\": %zu, ", n_none, out.size());
    }
    {   // ScanCloud::smooth: rich records follow through the kept indices
      ScanCloud a = model.views[0], b = model.views[0];
      const size_t da = a.smooth(1.2), db = b.smooth(1.2, 2, true);
      std::vector<uint32_t> ia, xa, nb, cb;
      bool ok = a.rich.size() == a.points.size() && b.rich.size() == b.points.size();
      for (size_t i = 0; i < a.rich.size(); ++i) {
        const io::RichPoint &q = a.rich[i];
        xa.push_back(bits(a.points[i].x)); xa.push_back(bits(a.points[i].y)); xa.push_back(bits(a.points[i].z));
        ok = ok && q.x == a.points[i].x && q.y == a.points[i].y && q.z == a.points[i].z;
        // colour, normal and curvature are those of the original record
        const size_t o = (size_t)q.curvature;
        ia.push_back((uint32_t)o);
        ok = ok && q.g == (uint8_t)(o % 251) && q.normal_x == model.views[0].rich[o].normal_x;
      }
      for (size_t i = 0; i < b.rich.size(); ++i) {
        const io::RichPoint &q = b.rich[i];
        nb.push_back(bits(q.normal_x)); nb.push_back(bits(q.normal_y)); nb.push_back(bits(q.normal_z)); cb.push_back(bits(q.curvature));
        ok = ok && q.x == b.points[i].x && q.z == b.points[i].z;
      }
      u32s("scan_idx", ia); u32s("scan_xyz", xa); u32s("scan_nrm", nb); u32s("scan_curv", cb);
      const size_t before = a.points.size();
      const size_t bad = a.smooth(0.0) + a.smooth(1.0, 3) + a.smooth(-1.0, 2, true);
      std::printf("\"scan_dropped\": [%zu, %zu], \"scan_rich_ok\": %d, \"scan_bad\": %zu, \"scan_after_bad\": %d, ", da, db, (int)ok, bad,
                  (int)(a.points.size() == before));
    }
    {   // the merged object: as the reference writes it, smoothed, and smoothed + downsampled
      Registrator reg(&model);
      double piv[3], ax[3];
      mvr_synth_prior(&sp, piv, ax);
      reg.setPivotPoint(piv[0], piv[1], piv[2]);
      reg.setAxisNormal(ax[0], ax[1], ax[2]);
      for (int v = 0; v < V; ++v) { model.views[v].initRotation(reg); model.views[v].setRegisterState(true); }
      io::RichCloud m;
      const size_t n_raw = reg.saveRegisteredPoints(0, folder + "/raw");
      const size_t n_mls = reg.saveRegisteredPoints(0, folder + "/mls", 2.0, 2, 0.f, &m);
      const size_t n_vox = reg.saveRegisteredPoints(0, folder + "/mls_vox", 2.0, 2, 1.5f);
      // refused parameters write nothing (<folder>/bad stays empty)
      const size_t n_bad = reg.saveRegisteredPoints(0, folder + "/bad", 0.0, 2, 0.f) + reg.saveRegisteredPoints(0, folder + "/bad", 2.0, 3, 0.f) +
                           reg.saveRegisteredPoints(0, folder + "/bad", 2.0, 2, -1.f);
      std::printf("\"merged\": [%zu, %zu, %zu], \"merged_out\": %zu, \"merged_bad\": %zu", n_raw, n_mls, n_vox, m.size(), n_bad);
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "mls_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
