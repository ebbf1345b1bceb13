// tests/cxx/iss_driver.cpp -- drives the C++ layers of the ISS keypoints (pcl::ISSKeypoint3D in mvr/registration.hpp,
// ScanCloud::detectKeypoints and ScanCloud::alignPrerejective with use_keypoints in mvr/registrator.hpp) on two clouds read from
// files and prints what they return as JSON; tests/test_gpu_iss_cxx.py compares it with the Python path
// (Context.iss_keypoints, Context.align_prerejective on NaN-masked tables) on the same clouds.
//
// usage: iss_driver <source.f32> <target.f32> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors>
//                   <normal_radius> <fpfh_radius> <iterations> <samples> <randomness> <similarity> <max_dist> <inlier_fraction> <seed>
//        (the files: n x 4 floats, x y z 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"

using namespace mvr;

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

static bool load(const char *path, PCLPointCloud &c)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  c.resize((size_t)bytes / 16);
  const bool ok = c.empty() || std::fread(c.points[0].data, 16, c.size(), f) == c.size();
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

static void pose(const char *key, const float *T)
{
  std::printf("\"%s\": [", key);
  for (int k = 0; k < 16; ++k) std::printf(k ? ",%u" : "%u", bits(T[k]));
  std::printf("], ");
}

int main(int argc, char **argv)
{
  if (argc < 17) { std::fprintf(stderr, "usage: %s source target salient non_max gamma_21 gamma_32 min_neighbors normal_radius fpfh_radius iterations samples randomness similarity max_dist inlier_fraction seed\n", argv[0]); return 2; }
  mvr_iss_params kp = mvr_iss_params();
  kp.salient_radius = std::atof(argv[3]); kp.non_max_radius = std::atof(argv[4]); kp.gamma_21 = std::atof(argv[5]); kp.gamma_32 = std::atof(argv[6]);
  kp.min_neighbors = std::atoi(argv[7]);
  const double rn = std::atof(argv[8]), rf = std::atof(argv[9]);
  const int iters = std::atoi(argv[10]), samples = std::atoi(argv[11]), randomness = std::atoi(argv[12]);
  const double similarity = std::atof(argv[13]), max_dist = std::atof(argv[14]), fraction = std::atof(argv[15]);
  const uint64_t seed = std::strtoull(argv[16], nullptr, 10);
  try {
    ScanCloud src, tgt;
    if (!load(argv[1], src.points) || !load(argv[2], tgt.points)) return 3;
    std::printf("{");
    {   // pcl::ISSKeypoint3D, PCL's call order
      typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
      Cloud::Ptr model(new Cloud(src.points)), keypoints(new Cloud());
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>());
      pcl::ISSKeypoint3D<pcl::PointXYZ, pcl::PointXYZ> iss;
      iss.setSearchMethod(tree);
      iss.setSalientRadius(kp.salient_radius);
      iss.setNonMaxRadius(kp.non_max_radius);
      iss.setThreshold21(kp.gamma_21);
      iss.setThreshold32(kp.gamma_32);
      iss.setMinNeighbors(kp.min_neighbors);
      iss.setNumberOfThreads(4);
      iss.setInputCloud(model);
      iss.compute(*keypoints);
      u32s("shim_index", iss.getKeypointsIndices()->indices);
      std::vector<uint32_t> xyz;
      for (size_t i = 0; i < keypoints->size(); ++i) { xyz.push_back(bits((*keypoints)[i].x)); xyz.push_back(bits((*keypoints)[i].y)); xyz.push_back(bits((*keypoints)[i].z)); }
      u32s("shim_points", xyz);
      // PCL's defaults, then in place: the output is the input cloud itself
      pcl::ISSKeypoint3D<pcl::PointXYZ> plain;
      plain.setSalientRadius(kp.salient_radius); plain.setNonMaxRadius(kp.non_max_radius);
      Cloud::Ptr own(new Cloud(src.points));
      plain.setInputCloud(own);
      plain.compute(*own);
      u32s("default_index", plain.getKeypointsIndices()->indices);
      std::printf("\"in_place_size\": %zu, ", own->size());
      // refusals: no input; no radius; a border radius; a normal radius
      pcl::ISSKeypoint3D<pcl::PointXYZ> none, no_radius, border, normal;
      Cloud o;
      std::vector<size_t> sz;
      o.resize(3); none.compute(o); sz.push_back(o.size());
      no_radius.setInputCloud(model); no_radius.setNonMaxRadius(kp.non_max_radius);
      o.resize(3); no_radius.compute(o); sz.push_back(o.size());
      border.setInputCloud(model); border.setSalientRadius(kp.salient_radius); border.setNonMaxRadius(kp.non_max_radius); border.setBorderRadius(1.0);
      o.resize(3); border.compute(o); sz.push_back(o.size() + border.getKeypointsIndices()->indices.size());
      normal.setInputCloud(model); normal.setSalientRadius(kp.salient_radius); normal.setNonMaxRadius(kp.non_max_radius); normal.setNormalRadius(1.0);
      o.resize(3); normal.compute(o); sz.push_back(o.size() + normal.getKeypointsIndices()->indices.size());
      u32s("refused", sz);
    }
    {   // ScanCloud::detectKeypoints
      std::vector<uint32_t> key(7), bad(7);
      mvr_iss_params off = kp;
      off.salient_radius = 0.0;
      const bool refused = src.detectKeypoints(off, bad);
      const size_t before = src.points.size();
      const bool ok = src.detectKeypoints(kp, key);
      u32s("scan_index", key);
      std::printf("\"scan_ok\": %d, \"scan_refused\": [%d, %zu], \"scan_untouched\": %d, ", (int)ok, (int)refused, bad.size(), (int)(src.points.size() == before));
      std::vector<uint32_t> tkey;
      tgt.detectKeypoints(kp, tkey);
      u32s("target_index", tkey);
    }
    {   // ScanCloud::alignPrerejective on the keypoints, with the normals of estimateNormals
      ScanCloud::PrerejectiveParams p;
      const int off_by_default = p.use_keypoints ? 0 : 1;
      p.feature_radius = rf;
      p.align.max_iterations = iters; p.align.nr_samples = samples; p.align.k = randomness; p.align.similarity = similarity;
      p.align.max_dist = max_dist; p.align.inlier_fraction = fraction; p.align.seed = seed;
      src.estimateNormals(0, rn);
      tgt.estimateNormals(0, rn);
      RowMatrixd start;
      mvr_prerej_result all, res;
      const bool ok_all = src.alignPrerejective(tgt, p, start, &all);
      pose("all_T", all.T);
      p.use_keypoints = true;
      const bool no_radius = src.alignPrerejective(tgt, p, start, &res);      // the detector's radii were never set
      p.keypoints = kp;
      const bool ok = src.alignPrerejective(tgt, p, start, &res);
      pose("key_T", res.T);
      std::printf("\"all_ok\": %d, \"all_inliers\": %u, \"all_best\": %d, \"key_ok\": %d, \"key_refused\": %d, \"key_inliers\": %u, \"key_best\": %d, "
                  "\"key_rejected\": %u, \"key_scored\": %u, \"off_by_default\": %d",
                  (int)ok_all, all.inliers, all.best_iteration, (int)ok, (int)no_radius, res.inliers, res.best_iteration, res.rejected, res.scored, off_by_default);
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "iss_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
