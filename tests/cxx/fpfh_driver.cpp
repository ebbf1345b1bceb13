// tests/cxx/fpfh_driver.cpp -- drives the C++ layers of the FPFH descriptors (pcl::FPFHEstimation in mvr/registration.hpp and
// ScanCloud::computeFPFH in mvr/registrator.hpp) on a synthetic turntable scan and prints what they return as JSON;
// tests/test_gpu_fpfh_cxx.py compares it with the Python path (Context.fpfh) on the same scan.
//
// usage: fpfh_driver <points> <config_id> <normal_radius> <fpfh_radius>
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

template <class F>
static int throws(F f) { try { f(); } catch (const std::invalid_argument &) { return 1; } return 0; }

int main(int argc, char **argv)
{
  if (argc < 5) { std::fprintf(stderr, "usage: %s points config normal_radius fpfh_radius\n", argv[0]); return 2; }
  const size_t N = (size_t)std::atol(argv[1]);
  const int config = std::atoi(argv[2]);
  const double rn = std::atof(argv[3]), rf = std::atof(argv[4]);
  try {
    mvr_synth_params sp;
    mvr_synth_default(&sp, 12, config);
    ScanCloud scan;
    scan.view = 0;
    scan.points.resize(N);
    if (mvr_synth_view(&sp, 0, N, scan.points.points[0].data, nullptr) != MVR_OK) return 3;
    std::printf("{");
    {   // pcl::FPFHEstimation, PCL's tutorial call for call
      pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(scan.points));
      pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>());
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
      ne.setInputCloud(cloud); ne.setSearchMethod(tree); ne.setRadiusSearch(rn);
      ne.compute(*normals);
      pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33> fpfh;
      fpfh.setInputCloud(cloud);
      fpfh.setInputNormals(normals);
      fpfh.setSearchMethod(tree);
      fpfh.setKSearch(0);
      fpfh.setRadiusSearch(rf);
      pcl::PointCloud<pcl::FPFHSignature33>::Ptr out(new pcl::PointCloud<pcl::FPFHSignature33>());
      fpfh.compute(*out);
      std::vector<uint32_t> sig;
      for (size_t i = 0; i < out->size(); ++i)
        for (int k = 0; k < pcl::FPFHSignature33::descriptorSize(); ++k) sig.push_back(bits((*out)[i].histogram[k]));
      u32s("shim", sig);
      std::printf("\"shim_size\": %zu, \"shim_dense\": %d, \"descriptor_size\": %d, ", out->size(), (int)out->is_dense, pcl::FPFHSignature33::descriptorSize());
      // what the class cannot do it refuses
      const int t_k = throws([&] { fpfh.setKSearch(10); }), t_s = throws([&] { fpfh.setSearchSurface(cloud); }),
                t_i = throws([&] { fpfh.setIndices(std::make_shared<const std::vector<int> >(3, 0)); });
      std::printf("\"throws\": [%d, %d, %d], ", t_k, t_s, t_i);
      // refusals of compute: no input; no normals; normals of another size; a radius that was never set
      pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal> none, no_normals, short_normals, no_radius;
      pcl::PointCloud<pcl::FPFHSignature33> o;
      std::vector<size_t> sz;
      o.resize(3); none.compute(o); sz.push_back(o.size());
      no_normals.setInputCloud(cloud); no_normals.setRadiusSearch(rf);
      o.resize(3); no_normals.compute(o); sz.push_back(o.size());
      pcl::PointCloud<pcl::Normal>::Ptr fewer(new pcl::PointCloud<pcl::Normal>(*normals));
      fewer->points.pop_back();
      short_normals.setInputCloud(cloud); short_normals.setInputNormals(fewer); short_normals.setRadiusSearch(rf);
      o.resize(3); short_normals.compute(o); sz.push_back(o.size());
      no_radius.setInputCloud(cloud); no_radius.setInputNormals(normals);
      o.resize(3); no_radius.compute(o); sz.push_back(o.size());
      std::printf("\"refused\": [%zu, %zu, %zu, %zu], ", sz[0], sz[1], sz[2], sz[3]);
    }
    {   // ScanCloud::computeFPFH with the normals of estimateNormals
      std::vector<FPFHSignature33> out(7);
      const bool no_rich = scan.computeFPFH(rf, out);
      const size_t n_no_rich = out.size();
      scan.estimateNormals(0, rn);
      const bool bad = scan.computeFPFH(0.0, out) || scan.computeFPFH(-1.0, out);
      const size_t n_bad = out.size();
      const bool ok = scan.computeFPFH(rf, out);
      std::vector<uint32_t> sig;
      for (size_t i = 0; i < out.size(); ++i)
        for (int k = 0; k < 33; ++k) sig.push_back(bits(out[i].histogram[k]));
      u32s("scan", sig);
      std::printf("\"scan_ok\": %d, \"scan_refused\": [%d, %zu, %d, %zu], \"scan_points\": %zu", (int)ok, (int)no_rich, n_no_rich, (int)bad, n_bad, scan.points.size());
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "fpfh_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
