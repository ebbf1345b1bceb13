// tests/cxx/ndt_driver.cpp -- drives pcl::NormalDistributionsTransform of the C++ shim (mvr/registration.hpp) and
// ScanCloud::alignNDT (mvr/registrator.hpp) on clouds read from files and prints what they return as JSON;
// tests/test_gpu_ndt_cxx.py compares it with the Python path (Context.ndt_align) on the same clouds.
//
// usage: ndt_driver <source.f32> <target.f32> <guess.f32> <resolution> <step_size> <transformation_epsilon>
//        (clouds: n x 4 floats; the guess: 16 floats, column-major)
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
  if (argc < 7) { std::fprintf(stderr, "usage: %s source target guess resolution step_size transformation_epsilon\n", argv[0]); return 2; }
  const double resolution = std::atof(argv[4]), step = std::atof(argv[5]), eps = std::atof(argv[6]);
  try {
    std::vector<float> s, t, g;
    if (!load(argv[1], s) || !load(argv[2], t) || !load(argv[3], g) || g.size() != 16) return 3;
    const size_t ns = s.size() / 4, nt = t.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    Cloud::Ptr src(new Cloud()), tgt(new Cloud());
    src->resize(ns); tgt->resize(nt);
    for (size_t i = 0; i < ns; ++i) { (*src)[i].x = s[4 * i]; (*src)[i].y = s[4 * i + 1]; (*src)[i].z = s[4 * i + 2]; }
    for (size_t i = 0; i < nt; ++i) { (*tgt)[i].x = t[4 * i]; (*tgt)[i].y = t[4 * i + 1]; (*tgt)[i].z = t[4 * i + 2]; }
    std::printf("{");
    {
      pcl::NormalDistributionsTransform<pcl::PointXYZ, pcl::PointXYZ> ndt;
      std::vector<uint32_t> defaults = {(uint32_t)(ndt.getResolution() == 1.0f), (uint32_t)(ndt.getStepSize() == 0.1), (uint32_t)(ndt.getOulierRatio() == 0.55),
                                        (uint32_t)(ndt.getTransformationEpsilon() == 0.1), (uint32_t)ndt.getMaximumIterations(),
                                        (uint32_t)ndt.getMinPointsPerVoxel(), (uint32_t)ndt.hasConverged(), (uint32_t)ndt.getFinalNumIteration()};
      u32s("defaults", defaults);
      ndt.setInputSource(src);
      ndt.setInputTarget(tgt);
      ndt.setResolution(1.5f); ndt.setResolution((float)resolution);
      ndt.setStepSize(0.3); ndt.setStepSize(step);
      ndt.setOulierRatio(0.4); ndt.setOutlierRatio(0.55);
      ndt.setTransformationEpsilon(eps);
      ndt.setMaximumIterations(35);
      std::vector<uint32_t> set = {(uint32_t)(ndt.getResolution() == (float)resolution), (uint32_t)(ndt.getStepSize() == step),
                                   (uint32_t)(ndt.getOutlierRatio() == 0.55 && ndt.getOulierRatio() == 0.55), (uint32_t)(ndt.getInputSource() == src)};
      u32s("setters", set);
      Cloud out;
      ndt.align(out);
      matrix("T", ndt.getFinalTransformation());
      std::vector<uint32_t> api = {(uint32_t)ndt.hasConverged(), (uint32_t)ndt.getFinalNumIteration(), (uint32_t)ndt.getStats().evaluations,
                                   (uint32_t)out.size(), (uint32_t)ndt.getStats().stop};
      u32s("api", api);
      std::printf("\"probability\": %.17g, \"score\": %.17g, \"fitness\": %.17g, ", ndt.getTransformationProbability(), ndt.getStats().score,
                  ndt.getFitnessScore());
      std::vector<uint32_t> sample;
      for (size_t i = 0; i < out.size(); i += 97) { sample.push_back(bits(out[i].x)); sample.push_back(bits(out[i].z)); }
      u32s("out", sample);
      Mat4<float> guess;
      for (int k = 0; k < 16; ++k) guess.m[k] = g[k];
      Cloud out2;
      ndt.align(out2, guess);
      matrix("guess_T", ndt.getFinalTransformation());
      std::vector<uint32_t> api2 = {(uint32_t)ndt.hasConverged(), (uint32_t)ndt.getFinalNumIteration(), (uint32_t)ndt.getStats().evaluations,
                                    (uint32_t)out2.size(), (uint32_t)ndt.getStats().stop};
      u32s("guess_api", api2);
      ndt.setMinPointsPerVoxel(1000000);          // no voxel is a cell: nothing overlaps, the final transformation is the guess
      ndt.align(out2, guess);
      matrix("none_T", ndt.getFinalTransformation());
      std::vector<uint32_t> api3 = {(uint32_t)ndt.hasConverged(), (uint32_t)ndt.getFinalNumIteration(), (uint32_t)ndt.getStats().stop};
      u32s("none_api", api3);
    }
    {   // ScanCloud::alignNDT rotates about the centre of the target's bounding box
      ScanCloud a, b;
      a.points = *src; b.points = *tgt;
      ScanCloud::NDTParams p;
      p.ndt.resolution = resolution; p.ndt.step_size = step; p.ndt.transformation_epsilon = eps;
      RowMatrixd pose;
      mvr_ndt_stats st;
      const bool ok = a.alignNDT(b, p, pose, &st);
      std::printf("\"scan_ok\": [%d, %d, %d], \"scan_pose\": [", ok ? 1 : 0, st.iterations, st.stop);
      for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf((i || j) ? ",%.17g" : "%.17g", pose.m[i][j]);
      std::printf("], ");
    }
    std::printf("\"done\": 1}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "ndt_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
