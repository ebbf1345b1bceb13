// tests/cxx/sac_driver.cpp -- drives the C++ layers of the plane segmentation (pcl::SACSegmentation, pcl::ExtractIndices,
// pcl::ModelCoefficients in mvr/registration.hpp; ScanCloud::segmentPlane / removePlane and Registrator::setPlatterRemoval in
// mvr/registrator.hpp) on a cloud read
// from a file and prints what they return as JSON; tests/test_gpu_sac_cxx.py compares it with the Python path
// (Context.segment_plane, Context.extract_indices) on the same cloud.
//
// usage: sac_driver <cloud.f32> <threshold> <max_iterations> <seed> <axis x> <axis y> <axis z> <eps_angle> <folder>
//        (the file: n x 4 floats, x y z 1; the folder: where saveRegisteredPoints writes)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"

using namespace mvr;

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static bool load(const char *path, std::vector<float> &v)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / 4);
  const bool ok = v.empty() || std::fread(v.data(), 4, v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

template <class V>
static void u32s(const char *key, const V &v)
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%u" : "%u", (unsigned)v[i]);
  std::printf("], ");
}

template <class C>
static void points(const char *key, const C &c)
{
  std::vector<uint32_t> b;
  for (size_t i = 0; i < c.size(); ++i) { b.push_back(bits(c[i].x)); b.push_back(bits(c[i].y)); b.push_back(bits(c[i].z)); }
  u32s(key, b);
}

int main(int argc, char **argv)
{
  if (argc < 10) { std::fprintf(stderr, "usage: %s cloud threshold max_iterations seed ax ay az eps_angle folder\n", argv[0]); return 2; }
  const double threshold = std::atof(argv[2]);
  const int max_iterations = std::atoi(argv[3]);
  const uint64_t seed = std::strtoull(argv[4], nullptr, 10);
  const float axis[3] = {(float)std::atof(argv[5]), (float)std::atof(argv[6]), (float)std::atof(argv[7])};
  const double eps_angle = std::atof(argv[8]);
  try {
    std::vector<float> xyz;
    if (!load(argv[1], xyz)) return 3;
    const size_t n = xyz.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    Cloud::Ptr cloud(new Cloud());
    cloud->resize(n);
    for (size_t i = 0; i < n; ++i) { (*cloud)[i].x = xyz[4 * i]; (*cloud)[i].y = xyz[4 * i + 1]; (*cloud)[i].z = xyz[4 * i + 2]; }
    std::printf("{");
    {   // pcl::SACSegmentation -> pcl::ExtractIndices, PCL's call order
      pcl::ModelCoefficients::Ptr coefficients(new pcl::ModelCoefficients());
      pcl::PointIndices::Ptr inliers(new pcl::PointIndices());
      pcl::SACSegmentation<pcl::PointXYZ> seg;
      std::printf("\"defaults\": [%d, %d, %d], ", seg.getMaxIterations(), (int)seg.getOptimizeCoefficients(), (int)(seg.getProbability() == 0.99));
      seg.setOptimizeCoefficients(true);
      seg.setModelType(pcl::SACMODEL_PLANE);
      seg.setMethodType(pcl::SAC_RANSAC);
      seg.setMaxIterations(max_iterations);
      seg.setDistanceThreshold(threshold);
      seg.setSeed(seed);
      seg.setInputCloud(cloud);
      seg.segment(*inliers, *coefficients);
      u32s("seg_index", inliers->indices);
      std::vector<uint32_t> co;
      for (float v : coefficients->values) co.push_back(bits(v));
      u32s("seg_coefficients", co);
      std::printf("\"seg_iterations\": %d, ", seg.getResult().iterations);
      pcl::ExtractIndices<pcl::PointXYZ> extract;
      Cloud object, plane;
      extract.setInputCloud(cloud);
      extract.setIndices(inliers);
      extract.setNegative(true);
      extract.filter(object);
      points("extract_negative", object);
      extract.setNegative(false);
      extract.filter(plane);
      points("extract_positive", plane);
      // the perpendicular model with the caller's axis
      seg.setModelType(pcl::SACMODEL_PERPENDICULAR_PLANE);
      seg.setAxis(axis);
      seg.setEpsAngle(eps_angle);
      seg.segment(*inliers, *coefficients);
      u32s("perp_index", inliers->indices);
      // an axis that lies in the platter: the platter is no valid model any more, something much smaller is found
      seg.setAxis(axis[1], axis[2], axis[0]);
      seg.segment(*inliers, *coefficients);
      u32s("perp_other_index", inliers->indices);
      // refusals: another method or model throws at the setter; no threshold prints an error and finds nothing
      int thrown = 0;
      try { seg.setMethodType(pcl::SAC_LMEDS); } catch (const mvr::Error &) { ++thrown; }
      try { seg.setModelType(pcl::SACMODEL_SPHERE); } catch (const mvr::Error &) { ++thrown; }
      pcl::SACSegmentation<pcl::PointXYZ> unset;
      unset.setModelType(pcl::SACMODEL_PLANE);
      unset.setInputCloud(cloud);
      inliers->indices.assign(3, 1);
      unset.segment(*inliers, *coefficients);
      pcl::PointIndices::Ptr bad(new pcl::PointIndices());
      bad->indices.push_back((int)n);
      extract.setIndices(bad);
      Cloud refused;
      refused.resize(3);
      extract.filter(refused);
      std::printf("\"refused\": [%d, %zu, %zu], ", thrown, inliers->indices.size(), refused.size());
    }
    {   // ScanCloud::segmentPlane and removePlane
      ScanCloud scan;
      scan.points.resize(n);
      scan.rich.resize(n);
      for (size_t i = 0; i < n; ++i) {
        scan.points.points[i].x = xyz[4 * i]; scan.points.points[i].y = xyz[4 * i + 1]; scan.points.points[i].z = xyz[4 * i + 2];
        scan.rich[i].x = xyz[4 * i]; scan.rich[i].y = xyz[4 * i + 1]; scan.rich[i].z = xyz[4 * i + 2]; scan.rich[i].curvature = (float)i;
      }
      ScanCloud::PlaneParams pp;
      pp.threshold = threshold; pp.max_iterations = max_iterations; pp.seed = seed;
      std::vector<uint32_t> index;
      float co[4];
      const bool ok = scan.segmentPlane(pp, index, co);
      u32s("scan_index", index);
      std::printf("\"scan_ok\": [%d, %d], ", (int)ok, (int)(scan.points.size() == n));
      ScanCloud::PlaneParams bad = pp;
      bad.threshold = 0.0;
      std::vector<uint32_t> none(5);
      const bool refused = scan.segmentPlane(bad, none, co);
      const size_t untouched = scan.removePlane(bad);
      std::printf("\"scan_refused\": [%d, %zu, %zu, %zu], ", (int)refused, none.size(), untouched, scan.points.size());
      const size_t removed = scan.removePlane(pp, co);
      std::printf("\"scan_removed\": %zu, ", removed);
      points("scan_points", scan.points);
      std::vector<uint32_t> follow;
      for (size_t i = 0; i < scan.rich.size(); ++i) follow.push_back((uint32_t)scan.rich[i].curvature);
      u32s("scan_rich_follow", follow);
    }
    {   // Registrator::setPlatterRemoval in front of saveRegisteredPoints: one registered view with the identity pose
      TurntableModel model;
      model.views.resize(1);
      ScanCloud &view = model.views[0];
      view.points.resize(n);
      for (size_t i = 0; i < n; ++i) { view.points.points[i].x = xyz[4 * i]; view.points.points[i].y = xyz[4 * i + 1]; view.points.points[i].z = xyz[4 * i + 2]; }
      view.setRegisterState(true);
      Registrator reg(&model);
      std::printf("\"platter_off_by_default\": %d, ", (int)!reg.getPlatterRemoval());
      reg.setAxisNormal(axis[0], axis[1], axis[2]);
      const std::string folder = argv[9];
      const size_t plain = reg.saveRegisteredPoints(0, folder);
      reg.setPlatterRemoval(threshold, eps_angle, max_iterations, seed);
      io::RichCloud merged, small;
      const size_t written = reg.saveRegisteredPoints(0, folder, &merged), taken = reg.lastPlatterPoints();
      const size_t written_leaf = reg.saveRegisteredPoints(0, folder, 4.0f, &small), taken_leaf = reg.lastPlatterPoints();
      io::RichCloud back;
      const bool read = io::loadPCDFile(folder + "/points.pcd", back);
      // the same by hand: the perpendicular model along the registrator's axis on the same points
      ScanCloud same;
      same.points = view.points;
      ScanCloud::PlaneParams pp;
      pp.threshold = threshold; pp.max_iterations = max_iterations; pp.seed = seed; pp.perpendicular = true; pp.eps_angle = eps_angle;
      for (int k = 0; k < 3; ++k) pp.axis[k] = axis[k];
      const size_t removed = same.removePlane(pp);
      bool equal = merged.size() == same.points.size();
      for (size_t i = 0; equal && i < merged.size(); ++i)
        equal = bits(merged[i].x) == bits(same.points.points[i].x) && bits(merged[i].y) == bits(same.points.points[i].y) && bits(merged[i].z) == bits(same.points.points[i].z);
      reg.setPlatterRemoval(0.0);
      const size_t off_again = reg.saveRegisteredPoints(0, folder);
      std::printf("\"platter\": [%zu, %zu, %zu, %zu, %zu, %d, %zu, %zu, %zu, %d, %zu, %d]", plain, written, taken, removed, merged.size(), (int)equal,
                  written_leaf, taken_leaf, small.size(), (int)read, back.size(), (int)(!reg.getPlatterRemoval() && off_again == plain));
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "sac_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
