// tests/cxx/shot_driver.cpp -- drives the C++ layers of the SHOT descriptors (pcl::SHOTLocalReferenceFrameEstimation,
// pcl::SHOTEstimation and pcl::SampleConsensusPrerejective<..., SHOT352> in mvr/registration.hpp, ScanCloud::computeSHOT,
// computeSHOTAt and alignPrerejectiveSHOT in mvr/registrator.hpp) on a synthetic turntable scan and prints what they return as
// JSON; tests/test_gpu_shot_cxx.py compares it with the Python path (Context.shot_lrf, Context.shot, Context.shot_at,
// Context.align_prerejective) on the same scan.
//
// usage: shot_driver <points> <config_id> <normal_radius> <shot_radius> <iterations> <seed> <max_dist>
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

template <class Rows>
static std::vector<uint32_t> frames_of(const Rows &c)
{
  std::vector<uint32_t> sig;
  for (size_t i = 0; i < c.size(); ++i)
    for (int k = 0; k < 9; ++k) sig.push_back(bits(c[i].rf[k]));
  return sig;
}

template <class Rows>
static std::vector<uint32_t> rows(const Rows &c)
{
  std::vector<uint32_t> sig;
  for (size_t i = 0; i < c.size(); ++i)
    for (int k = 0; k < 352; ++k) sig.push_back(bits(c[i].descriptor[k]));
  return sig;
}

static void pose(const char *key, const mvr_prerej_result &r)
{
  std::vector<uint32_t> T;
  for (int e = 0; e < 16; ++e) T.push_back(bits(r.T[e]));
  u32s(key, T);
}

int main(int argc, char **argv)
{
  if (argc < 8) { std::fprintf(stderr, "usage: %s points config normal_radius shot_radius iterations seed max_dist\n", argv[0]); return 2; }
  const size_t N = (size_t)std::atol(argv[1]);
  const int config = std::atoi(argv[2]);
  const double rn = std::atof(argv[3]), rf = std::atof(argv[4]);
  const int iterations = std::atoi(argv[5]);
  const uint64_t seed = (uint64_t)std::atoll(argv[6]);
  const double max_dist = std::atof(argv[7]);
  const std::vector<uint32_t> picks = {5, 3, 3, (uint32_t)(N - 1), 0};
  try {
    mvr_synth_params sp;
    mvr_synth_default(&sp, 12, config);
    ScanCloud scan, next;
    scan.view = 0; next.view = 1;
    scan.points.resize(N); next.points.resize(N);
    if (mvr_synth_view(&sp, 0, N, scan.points.points[0].data, nullptr) != MVR_OK) return 3;
    if (mvr_synth_view(&sp, 1, N, next.points.points[0].data, nullptr) != MVR_OK) return 3;
    std::printf("{");
    pcl::PointCloud<pcl::SHOT352>::Ptr sfeat(new pcl::PointCloud<pcl::SHOT352>()), tfeat(new pcl::PointCloud<pcl::SHOT352>());
    pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>(scan.points)), other(new pcl::PointCloud<pcl::PointXYZ>(next.points));
    {   // pcl::SHOTLocalReferenceFrameEstimation and pcl::SHOTEstimation, PCL's call order
      pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>()), other_normals(new pcl::PointCloud<pcl::Normal>());
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
      ne.setInputCloud(cloud); ne.setSearchMethod(tree); ne.setRadiusSearch(rn);
      ne.compute(*normals);
      ne.setInputCloud(other);
      ne.compute(*other_normals);
      pcl::PointCloud<pcl::ReferenceFrame>::Ptr frames(new pcl::PointCloud<pcl::ReferenceFrame>());
      pcl::SHOTLocalReferenceFrameEstimation<pcl::PointXYZ, pcl::ReferenceFrame> lrf;
      lrf.setInputCloud(cloud); lrf.setSearchMethod(tree); lrf.setRadiusSearch(rf);
      lrf.compute(*frames);
      u32s("lrf", frames_of(*frames));
      pcl::SHOTEstimation<pcl::PointXYZ, pcl::Normal, pcl::SHOT352, pcl::ReferenceFrame> shot;
      shot.setInputCloud(cloud);
      shot.setInputNormals(normals);
      shot.setSearchMethod(tree);
      shot.setRadiusSearch(rf);
      shot.compute(*sfeat);
      u32s("shim", rows(*sfeat));
      u32s("shim_rf", frames_of(*sfeat));
      std::printf("\"shim_size\": %zu, \"shim_dense\": %d, \"descriptor_size\": %d, ", sfeat->size(), (int)sfeat->is_dense, pcl::SHOT352::descriptorSize());
      pcl::PointCloud<pcl::SHOT352> o;
      shot.setInputReferenceFrames(frames);                  // its own frames passed in: the same rows
      shot.compute(o);
      u32s("shim_fed", rows(o));
      shot.setInputReferenceFrames(nullptr);
      shot.setLRFRadius((float)(0.75 * rf));
      shot.compute(o);
      u32s("shim_lrf_radius_rf", frames_of(o));
      shot.setLRFRadius(0.f);
      std::vector<int> ix(picks.begin(), picks.end());
      shot.setIndices(std::make_shared<const std::vector<int> >(ix));
      shot.compute(o);
      u32s("shim_indices", rows(o));
      shot.setIndices(nullptr);
      pcl::PointCloud<pcl::PointXYZ>::Ptr few(new pcl::PointCloud<pcl::PointXYZ>());
      for (uint32_t i : picks) few->push_back(cloud->points[i]);
      shot.setInputCloud(few); shot.setSearchSurface(cloud);   // normals_ belong to the surface
      shot.compute(o);
      u32s("shim_surface", rows(o));
      shot.setSearchSurface(nullptr);
      shot.setInputCloud(other); shot.setInputNormals(other_normals);
      shot.compute(*tfeat);
      // refusals of compute: no input; no normals; no radius
      pcl::SHOTEstimation<pcl::PointXYZ, pcl::Normal> none, no_normals, no_radius;
      std::vector<size_t> sz;
      o.resize(3); none.compute(o); sz.push_back(o.size());
      no_normals.setInputCloud(cloud); no_normals.setRadiusSearch(rf);
      o.resize(3); no_normals.compute(o); sz.push_back(o.size());
      no_radius.setInputCloud(cloud); no_radius.setInputNormals(normals);
      o.resize(3); no_radius.compute(o); sz.push_back(o.size());
      std::printf("\"refused\": [%zu, %zu, %zu], ", sz[0], sz[1], sz[2]);
    }
    {   // pcl::SampleConsensusPrerejective on SHOT352
      pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::SHOT352> align;
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
      pose("align_T", r);
      std::printf("\"align\": [%d, %d, %u, %u, %u], \"aligned_size\": %zu, ", r.converged, r.best_iteration, r.inliers, r.rejected, r.scored, aligned.size());
    }
    {   // ScanCloud::computeSHOT, computeSHOTAt and alignPrerejectiveSHOT with the normals of estimateNormals
      std::vector<SHOT352> out(7), at, over;
      const bool no_rich = scan.computeSHOT(rf, out);
      const size_t n_no_rich = out.size();
      scan.estimateNormals(0, rn);
      next.estimateNormals(0, rn);
      const bool bad = scan.computeSHOT(0.0, out) || scan.computeSHOT(-1.0, out) || scan.computeSHOT(rf, out, -1.0);
      const size_t n_bad = out.size();
      const bool ok = scan.computeSHOT(rf, out);
      u32s("scan", rows(out));
      u32s("scan_rf", frames_of(out));
      const bool ok_at = scan.computeSHOTAt(rf, picks, at);
      u32s("scan_at", rows(at));
      ScanCloud few;
      for (uint32_t i : picks) few.points.push_back(scan.points[i]);
      const bool ok_over = few.computeSHOTAt(scan, rf, over);
      u32s("scan_over", rows(over));
      std::vector<uint32_t> beyond = {0, (uint32_t)N};
      const bool bad_at = scan.computeSHOTAt(rf, beyond, at);
      ScanCloud::PrerejectiveParams pp;
      pp.feature_radius = rf;
      pp.align.max_iterations = iterations; pp.align.similarity = (double)0.8f; pp.align.max_dist = max_dist; pp.align.inlier_fraction = (double)0.25f;
      pp.align.seed = seed;
      RowMatrixd T;
      mvr_prerej_result res;
      const bool aligned = scan.alignPrerejectiveSHOT(next, pp, T, &res);
      pose("scan_align_T", res);
      std::printf("\"scan_align\": [%d, %d, %d, %u, %u, %u], ", (int)aligned, res.converged, res.best_iteration, res.inliers, res.rejected, res.scored);
      pp.use_keypoints = true;
      pp.keypoints.salient_radius = 2.0 * rf; pp.keypoints.non_max_radius = rf;
      std::vector<uint32_t> sk, tk;
      scan.detectKeypoints(pp.keypoints, pp.border, sk);
      next.detectKeypoints(pp.keypoints, pp.border, tk);
      u32s("keys_s", sk); u32s("keys_t", tk);
      const bool kaligned = scan.alignPrerejectiveSHOT(next, pp, T, &res);
      pose("key_align_T", res);
      std::printf("\"key_align\": [%d, %d, %d, %u, %u, %u], ", (int)kaligned, res.converged, res.best_iteration, res.inliers, res.rejected, res.scored);
      std::printf("\"scan_ok\": [%d, %d, %d], \"scan_refused\": [%d, %zu, %d, %zu, %d], \"scan_points\": %zu", (int)ok, (int)ok_at, (int)ok_over, (int)no_rich, n_no_rich,
                  (int)bad, n_bad, (int)bad_at, scan.points.size());
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "shot_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
