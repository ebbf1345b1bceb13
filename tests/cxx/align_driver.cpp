// tests/cxx/align_driver.cpp -- drives the C++ layers of the sample-consensus alignment (pcl::SampleConsensusPrerejective in
// mvr/registration.hpp and ScanCloud::alignPrerejective in mvr/registrator.hpp) on two clouds read from files and prints what
// they return as JSON; tests/test_gpu_align_cxx.py compares it with the Python path (Context.align_prerejective) on the same clouds.
//
// usage: align_driver <source.f32> <target.f32> <normal_radius> <fpfh_radius> <iterations> <samples> <randomness> <similarity>
//                     <max_dist> <inlier_fraction> <seed>          (the files: n x 4 floats, x y z 1)
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

static void pose(const char *key, const float *T)
{
  std::printf("\"%s\": [", key);
  for (int k = 0; k < 16; ++k) std::printf(k ? ",%u" : "%u", bits(T[k]));
  std::printf("], ");
}

int main(int argc, char **argv)
{
  if (argc < 12) { std::fprintf(stderr, "usage: %s source target normal_radius fpfh_radius iterations samples randomness similarity max_dist inlier_fraction seed\n", argv[0]); return 2; }
  const double rn = std::atof(argv[3]), rf = std::atof(argv[4]);
  const int iters = std::atoi(argv[5]), samples = std::atoi(argv[6]), randomness = std::atoi(argv[7]);
  const double similarity = std::atof(argv[8]), max_dist = std::atof(argv[9]), fraction = std::atof(argv[10]);
  const uint64_t seed = std::strtoull(argv[11], nullptr, 10);
  try {
    ScanCloud src, tgt;
    if (!load(argv[1], src.points) || !load(argv[2], tgt.points)) return 3;
    std::printf("{");
    {   // pcl::SampleConsensusPrerejective, PCL's alignment tutorial call for call
      typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
      typedef pcl::PointCloud<pcl::FPFHSignature33> Features;
      Cloud::Ptr object(new Cloud(src.points)), scene(new Cloud(tgt.points)), aligned(new Cloud());
      Features::Ptr feat[2] = {Features::Ptr(new Features()), Features::Ptr(new Features())};
      Cloud::Ptr clouds[2] = {object, scene};
      for (int c = 0; c < 2; ++c) {
        pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>());
        pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
        ne.setInputCloud(clouds[c]); ne.setRadiusSearch(rn);
        ne.compute(*normals);
        pcl::FPFHEstimation<pcl::PointXYZ, pcl::Normal, pcl::FPFHSignature33> fe;
        fe.setInputCloud(clouds[c]); fe.setInputNormals(normals); fe.setRadiusSearch(rf);
        fe.compute(*feat[c]);
      }
      pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::FPFHSignature33> align;
      align.setInputSource(object);
      align.setSourceFeatures(feat[0]);
      align.setInputTarget(scene);
      align.setTargetFeatures(feat[1]);
      align.setMaximumIterations(iters);
      align.setNumberOfSamples(samples);
      align.setCorrespondenceRandomness(randomness);
      align.setSimilarityThreshold((float)similarity);
      align.setMaxCorrespondenceDistance(max_dist);
      align.setInlierFraction((float)fraction);
      align.setSeed(seed);
      align.align(*aligned);
      pose("shim_T", align.getFinalTransformation().data());
      std::printf("\"shim_converged\": %d, \"shim_inliers\": %zu, \"shim_result_inliers\": %u, \"shim_fitness_bits\": %llu, \"shim_aligned\": %zu, ",
                  (int)align.hasConverged(), align.getInliers().size(), align.getResult().inliers,
                  [&] { const double e = align.getFitnessScore(); unsigned long long b; std::memcpy(&b, &e, 8); return b; }(), aligned->size());
      std::printf("\"shim_first\": [%u,%u,%u], ", aligned->empty() ? 0u : bits((*aligned)[0].x), aligned->empty() ? 0u : bits((*aligned)[0].y),
                  aligned->empty() ? 0u : bits((*aligned)[0].z));
      // with the result as the guess nothing is strictly better: the guess comes back
      Cloud again;
      align.align(again, align.getFinalTransformation());
      pose("guess_T", align.getFinalTransformation().data());
      std::printf("\"guess_best\": %d, ", align.getResult().best_iteration);
      // refusals: no features
      pcl::SampleConsensusPrerejective<pcl::PointXYZ, pcl::PointXYZ, pcl::FPFHSignature33> bare;
      bare.setInputSource(object); bare.setInputTarget(scene);
      Cloud o; o.resize(3);
      bare.align(o);
      std::printf("\"refused\": [%zu, %d], ", o.size(), (int)bare.hasConverged());
    }
    {   // ScanCloud::alignPrerejective with the normals of estimateNormals
      ScanCloud::PrerejectiveParams p;
      p.feature_radius = rf;
      p.align.max_iterations = iters; p.align.nr_samples = samples; p.align.k = randomness; p.align.similarity = similarity;
      p.align.max_dist = max_dist; p.align.inlier_fraction = fraction; p.align.seed = seed;
      RowMatrixd start;
      mvr_prerej_result res;
      const bool no_normals = src.alignPrerejective(tgt, p, start, &res);
      src.estimateNormals(0, rn);
      tgt.estimateNormals(0, rn);
      const bool ok = src.alignPrerejective(tgt, p, start, &res);
      pose("scan_T", res.T);
      const Matrix4f back = PclMatrixCaster<RowMatrixd>(start);
      pose("scan_pose", back.data());
      std::printf("\"scan_ok\": %d, \"scan_refused\": %d, \"scan_inliers\": %u, \"scan_best\": %d", (int)ok, (int)no_normals, res.inliers, res.best_iteration);
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "align_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
