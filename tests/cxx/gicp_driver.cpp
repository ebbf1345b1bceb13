// tests/cxx/gicp_driver.cpp -- drives pcl::GeneralizedIterativeClosestPoint of the C++ shim (mvr/registration.hpp) and
// ScanCloud::alignGICP (mvr/registrator.hpp) on clouds read from files and prints what they return as JSON;
// tests/test_gpu_gicp_cxx.py compares it with the Python path (Context.icp_align_gicp) on the same clouds.
//
// usage: gicp_driver <source.f32> <target.f32> <source_normals.f32> <target_normals.f32> <guess.f32> <max_dist>
//        (clouds and normals: n x 4 floats; the guess: 16 floats, column-major)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registration.hpp"
#include "mvr/registrator.hpp"

using namespace mvr;

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

template <class T>
static bool load(const char *path, std::vector<T> &v)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  const bool ok = v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
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

template <class M>
static void matrix(const char *key, const M &T)
{
  std::vector<uint32_t> b;
  for (int k = 0; k < 16; ++k) b.push_back(bits(T.m[k]));
  u32s(key, b);
}

int main(int argc, char **argv)
{
  if (argc < 7) { std::fprintf(stderr, "usage: %s source target source_normals target_normals guess max_dist\n", argv[0]); return 2; }
  const double max_dist = std::atof(argv[6]);
  try {
    std::vector<float> s, t, sn, tn, g;
    if (!load(argv[1], s) || !load(argv[2], t) || !load(argv[3], sn) || !load(argv[4], tn) || !load(argv[5], g) || g.size() != 16) return 3;
    const size_t ns = s.size() / 4, nt = t.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    typedef pcl::PointCloud<pcl::PointNormal> NCloud;
    Cloud::Ptr src(new Cloud()), tgt(new Cloud());
    NCloud::Ptr nsrc(new NCloud()), ntgt(new NCloud());
    src->resize(ns); tgt->resize(nt); nsrc->resize(ns); ntgt->resize(nt);
    for (size_t i = 0; i < ns; ++i) {
      (*src)[i].x = s[4 * i]; (*src)[i].y = s[4 * i + 1]; (*src)[i].z = s[4 * i + 2];
      (*nsrc)[i].x = s[4 * i]; (*nsrc)[i].y = s[4 * i + 1]; (*nsrc)[i].z = s[4 * i + 2];
      (*nsrc)[i].normal_x = sn[4 * i]; (*nsrc)[i].normal_y = sn[4 * i + 1]; (*nsrc)[i].normal_z = sn[4 * i + 2];
    }
    for (size_t i = 0; i < nt; ++i) {
      (*tgt)[i].x = t[4 * i]; (*tgt)[i].y = t[4 * i + 1]; (*tgt)[i].z = t[4 * i + 2];
      (*ntgt)[i].x = t[4 * i]; (*ntgt)[i].y = t[4 * i + 1]; (*ntgt)[i].z = t[4 * i + 2];
      (*ntgt)[i].normal_x = tn[4 * i]; (*ntgt)[i].normal_y = tn[4 * i + 1]; (*ntgt)[i].normal_z = tn[4 * i + 2];
    }
    std::printf("{");
    {   // PointXYZ: the normals are estimated inside, k = the correspondence randomness
      pcl::GeneralizedIterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> gicp;
      std::vector<uint32_t> defaults = {(uint32_t)gicp.getMaximumIterations(), (uint32_t)gicp.getMaximumOptimizerIterations(),
                                        (uint32_t)gicp.getCorrespondenceRandomness(), (uint32_t)(gicp.getRotationEpsilon() == 2e-3),
                                        (uint32_t)(gicp.getTransformationEpsilon() == 5e-4), (uint32_t)(gicp.getMaxCorrespondenceDistance() == 5.0),
                                        (uint32_t)(gicp.getCovarianceEpsilon() == 1e-3), (uint32_t)gicp.getUseReciprocalCorrespondences()};
      u32s("defaults", defaults);
      gicp.setInputSource(src);
      gicp.setInputTarget(tgt);
      gicp.setMaxCorrespondenceDistance(max_dist);
      gicp.setCorrespondenceRandomness(12); gicp.setCorrespondenceRandomness(20);
      gicp.setRotationEpsilon(1e-3); gicp.setRotationEpsilon(2e-3);
      gicp.setMaximumOptimizerIterations(7); gicp.setMaximumOptimizerIterations(20);
      Cloud out;
      gicp.align(out);
      matrix("xyz_T", gicp.getFinalTransformation());
      std::vector<uint32_t> api = {(uint32_t)gicp.hasConverged(), (uint32_t)gicp.getStats().iterations, (uint32_t)gicp.getStats().n_corr,
                                   (uint32_t)out.size(), (uint32_t)gicp.getConvergenceState()};
      u32s("xyz_api", api);
      std::vector<uint32_t> sample;
      for (size_t i = 0; i < out.size(); i += 97) { sample.push_back(bits(out[i].x)); sample.push_back(bits(out[i].z)); }
      u32s("xyz_out", sample);
      const float fit = (float)gicp.getFitnessScore();
      std::vector<uint32_t> fb = {bits(fit)};
      u32s("xyz_fitness", fb);
      // a guess: the align starts from the source under it
      Mat4<float> guess;
      for (int k = 0; k < 16; ++k) guess.m[k] = g[k];
      Cloud out2;
      gicp.align(out2, guess);
      matrix("guess_T", gicp.getFinalTransformation());
      // with a rejector and reciprocal correspondences
      pcl::registration::CorrespondenceRejectorMedianDistance::Ptr med(new pcl::registration::CorrespondenceRejectorMedianDistance());
      med->setMedianFactor(2.0);
      gicp.addCorrespondenceRejector(med);
      gicp.setUseReciprocalCorrespondences(true);
      gicp.align(out2);
      matrix("chain_T", gicp.getFinalTransformation());
      std::vector<uint32_t> mb = {bits((float)med->getMedianDistance())};
      u32s("chain_median", mb);
    }
    {   // PointNormal: the clouds' own normals (the shim's deviation)
      pcl::GeneralizedIterativeClosestPoint<pcl::PointNormal, pcl::PointNormal> gicp;
      gicp.setInputSource(nsrc);
      gicp.setInputTarget(ntgt);
      gicp.setMaxCorrespondenceDistance(max_dist);
      gicp.setCovarianceEpsilon(0.01);
      NCloud out;
      gicp.align(out);
      matrix("normal_T", gicp.getFinalTransformation());
      std::vector<uint32_t> sample;
      for (size_t i = 0; i < out.size(); i += 97) { sample.push_back(bits(out[i].x)); sample.push_back(bits(out[i].normal_x)); sample.push_back(bits(out[i].normal_z)); }
      u32s("normal_out", sample);
    }
    {   // ScanCloud::alignGICP: no rich records, so the normals are estimated
      ScanCloud a, b;
      a.points = *src; b.points = *tgt;
      ScanCloud::GICPParams p;
      p.gicp.max_corr_dist = max_dist;
      RowMatrixd pose;
      mvr_icp_stats st;
      const bool ok = a.alignGICP(b, p, pose, &st);
      std::printf("\"scan_ok\": [%d, %d], \"scan_pose\": [", ok ? 1 : 0, st.iterations);
      for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf((i || j) ? ",%.17g" : "%.17g", pose.m[i][j]);
      std::printf("], ");
    }
    std::printf("\"done\": 1}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "gicp_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
