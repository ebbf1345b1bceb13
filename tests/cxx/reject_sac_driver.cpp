// tests/cxx/reject_sac_driver.cpp -- drives pcl::registration::CorrespondenceRejectorSampleConsensus of the C++ shim
// (mvr/registration.hpp) on clouds read from files, on its own list and inside an IterativeClosestPoint, and prints what it
// returns as JSON; tests/test_gpu_reject_sac_cxx.py compares it with the Python path (Context.reject_sample_consensus,
// Context.icp_align_rejected, Context.last_sample_consensus) on the same clouds.
//
// usage: reject_sac_driver <source.f32> <target.f32> <list.u32> <max_dist> <max_iterations> <threshold> <sac_iterations> <seed>
//        (clouds: n x 4 floats; the list: n x 3 words, query, match, bits of the squared distance)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registration.hpp"

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
static void u32s(const char *key, const V &v, const char *end = ", ")
{
  std::printf("\"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ",%u" : "%u", (unsigned)v[i]);
  std::printf("]%s", end);
}

template <class M>
static void matrix(const char *key, const M &T)
{
  std::vector<uint32_t> b;
  for (int k = 0; k < 16; ++k) b.push_back(bits(T.m[k]));
  u32s(key, b);
}

static void list(const char *key, const pcl::Correspondences &c)
{
  std::vector<uint32_t> b;
  for (const pcl::Correspondence &x : c) { b.push_back((uint32_t)x.index_query); b.push_back((uint32_t)x.index_match); b.push_back(bits(x.distance)); }
  u32s(key, b);
}

typedef pcl::registration::CorrespondenceRejectorSampleConsensus<pcl::PointXYZ> Sac;

static std::vector<uint32_t> record(const mvr_rej_sac_result &r)
{
  return std::vector<uint32_t>{(uint32_t)r.found, r.live, r.valid, r.inliers, r.ransac_inliers, (uint32_t)r.iterations, (uint32_t)r.attempts,
                               (uint32_t)r.best_attempt, (uint32_t)r.refine_rounds};
}

int main(int argc, char **argv)
{
  if (argc < 9) { std::fprintf(stderr, "usage: %s source target list max_dist max_iterations threshold sac_iterations seed\n", argv[0]); return 2; }
  const double max_dist = std::atof(argv[4]), threshold = std::atof(argv[6]);
  const int max_iterations = std::atoi(argv[5]), sac_iterations = std::atoi(argv[7]);
  const uint64_t seed = std::strtoull(argv[8], nullptr, 10);
  try {
    std::vector<float> s, t;
    std::vector<uint32_t> words;
    if (!load(argv[1], s) || !load(argv[2], t) || !load(argv[3], words)) return 3;
    const size_t ns = s.size() / 4, nt = t.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    Cloud::Ptr src(new Cloud()), tgt(new Cloud());
    src->resize(ns); tgt->resize(nt);
    for (size_t i = 0; i < ns; ++i) { (*src)[i].x = s[4 * i]; (*src)[i].y = s[4 * i + 1]; (*src)[i].z = s[4 * i + 2]; }
    for (size_t i = 0; i < nt; ++i) { (*tgt)[i].x = t[4 * i]; (*tgt)[i].y = t[4 * i + 1]; (*tgt)[i].z = t[4 * i + 2]; }
    pcl::CorrespondencesPtr corrs(new pcl::Correspondences());
    for (size_t k = 0; k + 2 < words.size(); k += 3) { float d; std::memcpy(&d, &words[k + 2], 4); corrs->push_back(pcl::Correspondence((int)words[k], (int)words[k + 1], d)); }
    std::printf("{");
    {   // the rejector on its own list, PCL's call order
      Sac sac;
      std::vector<uint32_t> api;
      api.push_back(sac.getInlierThreshold() == 0.05 && sac.getMaximumIterations() == 1000 && !sac.getRefineModel() && !sac.getSaveInliers());      // PCL's defaults
      api.push_back(sac.getBestTransformation().isIdentity());
      sac.setInputSource(src);
      sac.setInputTarget(tgt);
      sac.setInlierThreshold(threshold);
      sac.setMaximumIterations(sac_iterations);
      sac.setRefineModel(true);
      sac.setSaveInliers(true);
      sac.setSeed(seed);
      api.push_back(sac.getInputSource().get() == src.get() && sac.getInputTarget().get() == tgt.get());
      api.push_back(sac.getInlierThreshold() == threshold && sac.getMaximumIterations() == sac_iterations && sac.getRefineModel() && sac.getSaveInliers());
      api.push_back(sac.requiresSourcePoints() && sac.requiresTargetPoints());
      sac.setInputCorrespondences(corrs);
      pcl::Correspondences kept;
      sac.getCorrespondences(kept);
      list("own_kept", kept);
      matrix("own_T", sac.getBestTransformation());
      u32s("own_result", record(sac.getResult()));
      std::vector<int> inl;
      sac.getInliersIndices(inl);
      u32s("own_inliers", inl);
      // the older names, without refinement, through getRemainingCorrespondences
      Sac old;
      old.setInputCloud(src);
      old.setTargetCloud(tgt);
      old.setInlierThreshold(threshold);
      old.setMaximumIterations(sac_iterations);
      old.setSeed(seed);
      kept.clear();
      old.getRemainingCorrespondences(*corrs, kept);
      list("old_kept", kept);
      matrix("old_T", old.getBestTransformation());
      old.getInliersIndices(inl);
      api.push_back(inl.empty());                                       // (setSaveInliers was not called)
      // without clouds: an error line, nothing returned
      Sac none;
      kept.assign(3, pcl::Correspondence());
      none.getRemainingCorrespondences(*corrs, kept);
      api.push_back(kept.empty());
      std::printf("\"name\": \"%s\", ", sac.getClassName().c_str());
      u32s("own_api", api);
    }
    {   // inside an ICP: a stage of the chain; afterwards the rejector knows the last iteration's motion
      pcl::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
      icp.setInputSource(src);
      icp.setInputTarget(tgt);
      icp.setUseReciprocalCorrespondences(true);
      icp.setMaxCorrespondenceDistance(max_dist);
      icp.setMaximumIterations(max_iterations);
      Sac::Ptr sac(new Sac());
      sac->setInlierThreshold(threshold);
      sac->setMaximumIterations(sac_iterations);
      sac->setRefineModel(true);
      sac->setSeed(seed);
      pcl::registration::CorrespondenceRejectorMedianDistance::Ptr med(new pcl::registration::CorrespondenceRejectorMedianDistance());
      med->setMedianFactor(2.0);
      icp.addCorrespondenceRejector(sac);
      icp.addCorrespondenceRejector(med);
      Cloud out;
      icp.align(out);
      matrix("icp_T", icp.getFinalTransformation());
      matrix("icp_best", sac->getBestTransformation());
      u32s("icp_result", record(sac->getResult()));
      std::vector<uint32_t> api;
      api.push_back(icp.hasConverged()); api.push_back((uint32_t)icp.getStats().iterations); api.push_back((uint32_t)icp.getStats().n_corr);
      api.push_back((uint32_t)out.size()); api.push_back(bits((float)med->getMedianDistance()));
      u32s("icp_api", api, "");
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "reject_sac_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
