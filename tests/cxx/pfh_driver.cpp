// tests/cxx/pfh_driver.cpp -- drives the C++ layers of the PFH descriptors (pcl::PFHEstimation and
// pcl::SampleConsensusPrerejective<..., PFHSignature125> in mvr/registration.hpp, ScanCloud::computePFH and
// ScanCloud::alignPrerejectivePFH in mvr/registrator.hpp) on a synthetic turntable scan and prints what they return as JSON;
// tests/test_gpu_pfh_cxx.py compares it with the Python path (Context.pfh, Context.align_prerejective) on the same scan.
//
// usage: pfh_driver <points> <config_id> <normal_radius> <pfh_radius> <k> <iterations> <seed> <max_dist>
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

template <class Cloud>
static std::vector<uint32_t> rows(const Cloud &c)
{
  std::vector<uint32_t> sig;
  for (size_t i = 0; i < c.size(); ++i)
    for (int k = 0; k < 125; ++k) sig.push_back(bits(c[i].histogram[k]));
  return sig;
}

template <class F>
static int throws(F f) { try { f(); } catch (const std::invalid_argument &) { return 1; } return 0; }

int main(int argc, char **argv)
{
  if (argc < 9) { std::fprintf(stderr, "usage: %s points config normal_radius pfh_radius k iterations seed max_dist\n", argv[0]); return 2; }
  const size_t N = (size_t)std::atol(argv[1]);
  const int config = std::atoi(argv[2]);
  const double rn = std::atof(argv[3]), rf = std::atof(argv[4]);
  const int k = std::atoi(argv[5]), iterations = std::atoi(argv[6]);
  const uint64_t seed = (uint64_t)std::atoll(argv[7]);
  const double max_dist = std::atof(argv[8]);
  try {
    mvr_synth_params sp;
    mvr_synth_default(&sp, 12, config);
    ScanCloud scan, next;
    scan.view = 0; next.view = 1;
    scan.points.resize(N); next.points.resize(N);
    if (mvr_synth_view(&sp, 0, N, scan.points.points[0].data, nullptr) != MVR_OK) return 3;
    if (mvr_synth_view(&sp, 1, N, next.points.points[0].data, nullptr) != MVR_OK) return 3;
    std::printf("{");
    pcl::PointCloud<pcl::PFHSignature125>::Ptr sfeat(new pcl::PointCloud<pcl::PFHSignature125>()), tfeat(new pcl::PointCloud<pcl::PFHSignature125>());
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(scan.points)), other(new pcl::PointCloud<pcl::PointXYZ>(next.points));
    {   // pcl::PFHEstimation, PCL's tutorial call for call
      pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>()), other_normals(new pcl::PointCloud<pcl::Normal>());
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
      ne.setInputCloud(cloud); ne.setSearchMethod(tree); ne.setRadiusSearch(rn);
      ne.compute(*normals);
      ne.setInputCloud(other);
      ne.compute(*other_normals);
      pcl::PFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::PFHSignature125> pfh;
      pfh.setInputCloud(cloud);
      pfh.setInputNormals(normals);
      pfh.setSearchMethod(tree);
      pfh.setMaximumCacheSize(1000);
      pfh.setUseInternalCache(true);
      pfh.setRadiusSearch(rf);
      pfh.compute(*sfeat);
      u32s("shim", rows(*sfeat));
      std::printf("\"shim_size\": %zu, \"shim_dense\": %d, \"descriptor_size\": %d, \"modes\": [%g, %d, ", sfeat->size(), (int)sfeat->is_dense,
                  pcl::PFHSignature125::descriptorSize(), pfh.getRadiusSearch(), pfh.getKSearch());
      pcl::PointCloud<pcl::PFHSignature125> by_k;
      pfh.setKSearch(k);                                     // the later call decides the mode
      std::printf("%g, %d], ", pfh.getRadiusSearch(), pfh.getKSearch());
      pfh.compute(by_k);
      u32s("shim_k", rows(by_k));
      pfh.setRadiusSearch(rf);
      pfh.setInputCloud(other); pfh.setInputNormals(other_normals);
      pfh.compute(*tfeat);
      const int t_s = throws([&] { pfh.setSearchSurface(cloud); }), t_i = throws([&] { pfh.setIndices(std::make_shared<const std::vector<int> >(3, 0)); });
      std::printf("\"throws\": [%d, %d], ", t_s, t_i);
      // refusals of compute: no input; no normals; normals of another size; neither radius nor k; a k out of range
      pcl::PFHEstimation<pcl::PointXYZ, pcl::Normal> none, no_normals, short_normals, no_mode, bad_k;
      pcl::PointCloud<pcl::PFHSignature125> o;
      std::vector<size_t> sz;
      o.resize(3); none.compute(o); sz.push_back(o.size());
      no_normals.setInputCloud(cloud); no_normals.setRadiusSearch(rf);
      o.resize(3); no_normals.compute(o); sz.push_back(o.size());
      pcl::PointCloud<pcl::Normal>::Ptr fewer(new pcl::PointCloud<pcl::Normal>(*normals));
      fewer->points.pop_back();
      short_normals.setInputCloud(cloud); short_normals.setInputNormals(fewer); short_normals.setRadiusSearch(rf);
      o.resize(3); short_normals.compute(o); sz.push_back(o.size());
      no_mode.setInputCloud(cloud); no_mode.setInputNormals(normals);
      o.resize(3); no_mode.compute(o); sz.push_back(o.size());
      bad_k.setInputCloud(cloud); bad_k.setInputNormals(normals); bad_k.setKSearch(MVR_MAX_KNN + 1);
      o.resize(3); bad_k.compute(o); sz.push_back(o.size());
      std::printf("\"refused\": [%zu, %zu, %zu, %zu, %zu], ", sz[0], sz[1], sz[2], sz[3], sz[4]);
    }
    {   // pcl::SampleConsensusPrerejective on the 125-float signatures, PCL's tutorial call for call
      pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::PFHSignature125> align;
      align.setInputSource(cloud);
      align.setSourceFeatures(sfeat);
      align.setInputTarget(other);
      align.setTargetFeatures(tfeat);
      align.setMaximumIterations(iterations);
      align.setNumberOfSamples(3);
      align.setCorrespondenceRandomness(2);
      align.setSimilarityThreshold(0.8f);
      align.setMaxCorrespondenceDistance(max_dist);
      align.setInlierFraction(0.25f);
      align.setSeed(seed);
      pcl::PointCloud<pcl::PointXYZ> aligned;
      align.align(aligned);
      const mvr_prerej_result &r = align.getResult();
      std::vector<uint32_t> T;
      for (int e = 0; e < 16; ++e) T.push_back(bits(r.T[e]));
      u32s("align_T", T);
      std::printf("\"align\": [%d, %d, %u, %u, %u], \"align_error\": %.17g, \"aligned_size\": %zu, \"inlier_list\": %zu, ", r.converged, r.best_iteration,
                  r.inliers, r.rejected, r.scored, r.error, aligned.size(), align.getInliers().size());
    }
    {   // ScanCloud::computePFH and alignPrerejectivePFH with the normals of estimateNormals
      std::vector<PFHSignature125> out(7);
      const bool no_rich = scan.computePFH(rf, out);
      const size_t n_no_rich = out.size();
      scan.estimateNormals(0, rn);
      next.estimateNormals(0, rn);
      const bool bad = scan.computePFH(0.0, out) || scan.computePFH(-1.0, out);
      const size_t n_bad = out.size();
      const bool ok = scan.computePFH(rf, out);
      std::vector<uint32_t> sig;
      for (size_t i = 0; i < out.size(); ++i)
        for (int b = 0; b < 125; ++b) sig.push_back(bits(out[i].histogram[b]));
      u32s("scan", sig);
      ScanCloud::PrerejectiveParams pp;
      pp.feature_radius = rf;
      pp.align.max_iterations = iterations; pp.align.similarity = (double)0.8f; pp.align.max_dist = max_dist; pp.align.inlier_fraction = (double)0.25f;
      pp.align.seed = seed;
      RowMatrixd pose;
      mvr_prerej_result res;
      const bool aligned = scan.alignPrerejectivePFH(next, pp, pose, &res);
      std::vector<uint32_t> T;
      for (int e = 0; e < 16; ++e) T.push_back(bits(res.T[e]));
      u32s("scan_align_T", T);
      std::printf("\"scan_align\": [%d, %d, %d, %u, %u, %u], ", (int)aligned, res.converged, res.best_iteration, res.inliers, res.rejected, res.scored);
      std::printf("\"scan_ok\": %d, \"scan_refused\": [%d, %zu, %d, %zu], \"scan_points\": %zu", (int)ok, (int)no_rich, n_no_rich, (int)bad, n_bad, scan.points.size());
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "pfh_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
