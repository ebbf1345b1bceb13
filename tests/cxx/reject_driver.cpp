// tests/cxx/reject_driver.cpp -- drives the correspondence rejectors of the C++ shim (pcl::registration::CorrespondenceRejector*
// and IterativeClosestPoint::addCorrespondenceRejector in mvr/registration.hpp) on clouds read from files and prints what they
// return as JSON; tests/test_gpu_reject_cxx.py compares it with the Python path (Context.icp_align_rejected,
// Context.reject_correspondences) on the same clouds.
//
// usage: reject_driver <source.f32> <target.f32> <source_normals.f32> <target_normals.f32> <list.u32> <max_dist> <max_iterations>
//        (clouds and normals: n x 4 floats; the list: n x 3 words, query, match, bits of the squared distance)
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

static void list(const char *key, const pcl::Correspondences &c)
{
  std::vector<uint32_t> b;
  for (const pcl::Correspondence &x : c) { b.push_back((uint32_t)x.index_query); b.push_back((uint32_t)x.index_match); b.push_back(bits(x.distance)); }
  u32s(key, b);
}

int main(int argc, char **argv)
{
  if (argc < 8) { std::fprintf(stderr, "usage: %s source target source_normals target_normals list max_dist max_iterations\n", argv[0]); return 2; }
  const double max_dist = std::atof(argv[6]);
  const int max_iterations = std::atoi(argv[7]);
  try {
    std::vector<float> s, t, sn, tn;
    std::vector<uint32_t> words;
    if (!load(argv[1], s) || !load(argv[2], t) || !load(argv[3], sn) || !load(argv[4], tn) || !load(argv[5], words)) return 3;
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
    {   // an ICP with two rejectors, PCL's call order
      pcl::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
      icp.setInputSource(src);
      icp.setInputTarget(tgt);
      icp.setUseReciprocalCorrespondences(true);
      icp.setMaxCorrespondenceDistance(max_dist);
      icp.setMaximumIterations(max_iterations);
      pcl::registration::CorrespondenceRejectorMedianDistance::Ptr med(new pcl::registration::CorrespondenceRejectorMedianDistance());
      med->setMedianFactor(2.0);
      pcl::registration::CorrespondenceRejectorTrimmed::Ptr trim(new pcl::registration::CorrespondenceRejectorTrimmed());
      trim->setOverlapRatio(0.8f);
      trim->setMinCorrespondences(10);
      pcl::registration::CorrespondenceRejectorDistance::Ptr dist(new pcl::registration::CorrespondenceRejectorDistance());
      dist->setMaximumDistance(1.5f);
      icp.addCorrespondenceRejector(med);
      icp.addCorrespondenceRejector(dist);
      icp.addCorrespondenceRejector(trim);
      const bool removed = icp.removeCorrespondenceRejector(1), not_removed = icp.removeCorrespondenceRejector(7);
      std::vector<uint32_t> api;
      api.push_back(removed); api.push_back(not_removed); api.push_back((uint32_t)icp.getCorrespondenceRejectors().size());
      api.push_back(icp.getCorrespondenceRejectors()[1].get() == trim.get());
      api.push_back(med->getMedianFactor() == 2.0 && trim->getOverlapRatio() == 0.8f && trim->getMinCorrespondences() == 10 && dist->getMaximumDistance() == 1.5f);
      Cloud out;
      icp.align(out);
      matrix("icp_T", icp.getFinalTransformation());
      api.push_back(icp.hasConverged()); api.push_back((uint32_t)icp.getStats().iterations); api.push_back((uint32_t)icp.getStats().n_corr);
      api.push_back((uint32_t)out.size());
      u32s("icp_api", api);
      std::vector<uint32_t> md(1, bits((float)med->getMedianDistance()));
      u32s("icp_median", md);
      std::printf("\"names\": [\"%s\", \"%s\", \"%s\"], ", med->getClassName().c_str(), trim->getClassName().c_str(), dist->getClassName().c_str());
      icp.clearCorrespondenceRejectors();                              // without rejectors: the plain align again
      api.assign(1, (uint32_t)icp.getCorrespondenceRejectors().size());
      icp.align(out);
      matrix("plain_T", icp.getFinalTransformation());
      u32s("cleared", api);
    }
    {   // clouds with normals: the surface-normal rejector reads the normals the ICP holds
      pcl::IterativeClosestPoint<pcl::PointNormal, pcl::PointNormal> icp;
      icp.setInputSource(nsrc);
      icp.setInputTarget(ntgt);
      icp.setMaxCorrespondenceDistance(max_dist);
      icp.setMaximumIterations(max_iterations);
      pcl::registration::CorrespondenceRejectorOneToOne::Ptr oto(new pcl::registration::CorrespondenceRejectorOneToOne());
      pcl::registration::CorrespondenceRejectorSurfaceNormal::Ptr sn_rej(new pcl::registration::CorrespondenceRejectorSurfaceNormal());
      sn_rej->setThreshold(0.9995);
      icp.addCorrespondenceRejector(oto);
      icp.addCorrespondenceRejector(sn_rej);
      NCloud out;
      icp.align(out);
      matrix("normal_T", icp.getFinalTransformation());
      std::vector<uint32_t> b;
      for (size_t i = 0; i < out.size(); i += 97) { b.push_back(bits(out[i].x)); b.push_back(bits(out[i].normal_x)); b.push_back(bits(out[i].normal_z)); }
      u32s("normal_out", b);
      b.assign(1, (uint32_t)icp.getStats().n_corr); b.push_back(sn_rej->getThreshold() == 0.9995);
      u32s("normal_api", b);
    }
    pcl::CorrespondencesPtr corrs(new pcl::Correspondences());
    for (size_t k = 0; k + 2 < words.size(); k += 3) { float d; std::memcpy(&d, &words[k + 2], 4); corrs->push_back(pcl::Correspondence((int)words[k], (int)words[k + 1], d)); }
    {   // a rejector on its own
      pcl::registration::CorrespondenceRejectorMedianDistance med;
      med.setMedianFactor(1.25);
      med.setInputCorrespondences(corrs);
      pcl::Correspondences kept;
      med.getCorrespondences(kept);
      list("median_kept", kept);
      std::vector<uint32_t> md(1, bits((float)med.getMedianDistance()));
      u32s("median_distance", md);
      pcl::registration::CorrespondenceRejectorSurfaceNormal sn_rej;
      sn_rej.initializeDataContainer<pcl::PointXYZ, pcl::PointNormal>();
      sn_rej.setInputSource<pcl::PointXYZ>(src);
      sn_rej.setInputTarget<pcl::PointXYZ>(tgt);
      sn_rej.setInputNormals<pcl::PointXYZ, pcl::PointNormal>(nsrc);
      sn_rej.setTargetNormals<pcl::PointXYZ, pcl::PointNormal>(ntgt);
      sn_rej.setThreshold(0.9995);
      kept.clear();
      sn_rej.getRemainingCorrespondences(*corrs, kept);
      list("normal_kept", kept);
      pcl::registration::CorrespondenceRejectorMedianDistance negative;
      negative.setMedianFactor(-1.0);                                   // refused by the library: an error line, nothing returned
      negative.setInputCorrespondences(corrs);
      kept.assign(3, pcl::Correspondence());
      negative.getCorrespondences(kept);
      std::vector<uint32_t> r(1, (uint32_t)kept.size());
      std::printf("\"refused\": [%u]", r[0]);
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "reject_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
