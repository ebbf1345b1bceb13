// tests/cxx/surface_driver.cpp -- drives the C++ layers of the features over a search surface (pcl::NormalEstimation with
// setSearchSurface / setIndices in mvr/registration.hpp; ScanCloud::computeFPFHAt, computePFHAt, estimateNormalsFrom and
// alignPrerejectivePFH (descriptors at the keypoints) and alignPrerejective with use_keypoints in mvr/registrator.hpp) on two clouds read from files.  Tables go to
// files of raw floats in <outdir>, the rest is printed as JSON; tests/test_gpu_surface_cxx.py compares both with the Python path
// (Context.estimate_normals_at, fpfh_at, pfh_at) on the same clouds.
//
// usage: surface_driver <source.f32> <target.f32> <outdir> <salient_radius> <non_max_radius> <gamma_21> <gamma_32> <min_neighbors>
//                       <normal_radius> <feature_radius> <iterations> <samples> <randomness> <similarity> <max_dist> <inlier_fraction>
//                       <seed> <index_step>          (the files: n x 4 floats, x y z 1)
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

static std::string outdir;

static void save(const char *name, const float *v, size_t count)
{
  FILE *f = std::fopen((outdir + "/" + name + ".f32").c_str(), "wb");
  if (!f || std::fwrite(v, 4, count, f) != count) { std::fprintf(stderr, "surface_driver: cannot write %s\n", name); std::exit(4); }
  std::fclose(f);
}

template <typename FeatureT>
static void save_rows(const char *name, const std::vector<FeatureT> &rows)
{
  static const float none[1] = {0.f};
  save(name, rows.empty() ? none : rows[0].histogram, rows.size() * sizeof(FeatureT) / sizeof(float));
}

static void save_normals(const char *name, const pcl::PointCloud<pcl::Normal> &n)
{
  std::vector<float> v;
  for (size_t i = 0; i < n.size(); ++i) { v.push_back(n[i].normal_x); v.push_back(n[i].normal_y); v.push_back(n[i].normal_z); v.push_back(n[i].curvature); }
  v.push_back(0.f);
  save(name, v.data(), v.size() - 1);
}

static void pose(const char *key, const float *T)
{
  std::printf("\"%s\": [", key);
  for (int k = 0; k < 16; ++k) std::printf(k ? ",%u" : "%u", bits(T[k]));
  std::printf("], ");
}

static bool same(const mvr_prerej_result &a, const mvr_prerej_result &b)
{
  return std::memcmp(a.T, b.T, sizeof a.T) == 0 && a.best_iteration == b.best_iteration && a.inliers == b.inliers && a.converged == b.converged;
}

static bool same_pose(const RowMatrixd &a, const RowMatrixd &b)
{
  const Matrix4f x = PclMatrixCaster<RowMatrixd>(a), y = PclMatrixCaster<RowMatrixd>(b);
  return std::memcmp(x.data(), y.data(), 16 * sizeof(float)) == 0;
}

int main(int argc, char **argv)
{
  if (argc < 19) { std::fprintf(stderr, "usage: %s source target outdir salient non_max gamma_21 gamma_32 min_neighbors normal_radius feature_radius "
                                        "iterations samples randomness similarity max_dist inlier_fraction seed index_step\n", argv[0]); return 2; }
  outdir = argv[3];
  mvr_iss_params kp = mvr_iss_params();
  kp.salient_radius = std::atof(argv[4]); kp.non_max_radius = std::atof(argv[5]); kp.gamma_21 = std::atof(argv[6]); kp.gamma_32 = std::atof(argv[7]);
  kp.min_neighbors = std::atoi(argv[8]);
  const double rn = std::atof(argv[9]), rf = std::atof(argv[10]);
  const size_t step = (size_t)std::atoi(argv[18]);
  try {
    ScanCloud src, tgt;
    if (!load(argv[1], src.points) || !load(argv[2], tgt.points)) return 3;
    std::vector<uint32_t> idx;                          // every step-th point of the source, backwards, the first one twice
    for (size_t i = src.points.size(); i-- > 0;)
      if (i % step == 0) idx.push_back((uint32_t)i);
    if (!idx.empty()) idx.push_back(idx[0]);
    std::printf("{");
    {   // pcl::NormalEstimation: the normals of the target's points from the source as surface; of an index subset of the source
      typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
      Cloud::Ptr object(new Cloud(src.points)), scene(new Cloud(tgt.points));
      pcl::PointCloud<pcl::Normal> n;
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
      ne.setInputCloud(scene); ne.setSearchSurface(object); ne.setRadiusSearch(rn);
      ne.compute(n);
      save_normals("ne_surface", n);
      std::printf("\"ne_surface\": %zu, ", n.size());
      pcl::NormalEstimation<pcl::PointXYZ, pcl::Normal> ni;
      std::shared_ptr<std::vector<int> > ii(new std::vector<int>(idx.begin(), idx.end()));
      ni.setInputCloud(object); ni.setIndices(ii); ni.setKSearch(12);
      ni.compute(n);
      save_normals("ne_indices", n);
      std::printf("\"ne_indices\": %zu, ", n.size());
      ii->push_back((int)object->size());                // an index outside the cloud: refused, output empty
      ni.compute(n);
      std::printf("\"ne_refused\": %zu, ", n.size());
    }
    {   // ScanCloud: descriptors at chosen points; refusals first (no normals yet)
      std::vector<pcl::FPFHSignature33> f;
      std::vector<pcl::PFHSignature125> h;
      const bool no_normals = src.computeFPFHAt(rf, idx, f) || src.computePFHAt(rf, idx, h);
      src.estimateNormals(0, rn);
      tgt.estimateNormals(0, rn);
      const bool bad_radius = src.computeFPFHAt(0.0, idx, f) || src.computePFHAt(-1.0, idx, h);
      std::vector<uint32_t> beyond(idx);
      beyond.push_back((uint32_t)src.points.size());
      const bool bad_index = src.computeFPFHAt(rf, beyond, f) || src.computePFHAt(rf, beyond, h);
      const bool ok = src.computeFPFHAt(rf, idx, f) && src.computePFHAt(rf, idx, h);
      save_rows("fpfh_indices", f);
      save_rows("pfh_indices", h);
      std::printf("\"at_ok\": %d, \"at_refused\": [%d, %d, %d], \"at_rows\": [%zu, %zu], ", (int)ok, (int)no_normals, (int)bad_radius, (int)bad_index, f.size(), h.size());
      ScanCloud bare;                                    // the target's points alone: positions over the source and ITS normals
      bare.points = tgt.points;
      const bool ok2 = bare.computeFPFHAt(src, rf, f) && bare.computePFHAt(src, rf, h);
      save_rows("fpfh_surface", f);
      save_rows("pfh_surface", h);
      std::printf("\"surface_ok\": %d, \"surface_rows\": [%zu, %zu], ", (int)ok2, f.size(), h.size());
      bare.estimateNormalsFrom(src, 0, rn);
      std::vector<float> v;
      for (size_t i = 0; i < bare.rich.size(); ++i) { v.push_back(bare.rich[i].normal_x); v.push_back(bare.rich[i].normal_y); v.push_back(bare.rich[i].normal_z); v.push_back(bare.rich[i].curvature); }
      v.push_back(0.f);
      save("normals_from", v.data(), v.size() - 1);
      std::printf("\"normals_from\": %zu, ", bare.rich.size());
    }
    {   // the coarse alignment on keypoints: descriptors at the keypoints against full tables through the four-argument overload
      ScanCloud::PrerejectiveParams p;
      p.feature_radius = rf;
      p.align.max_iterations = std::atoi(argv[11]); p.align.nr_samples = std::atoi(argv[12]); p.align.k = std::atoi(argv[13]);
      p.align.similarity = std::atof(argv[14]); p.align.max_dist = std::atof(argv[15]); p.align.inlier_fraction = std::atof(argv[16]);
      p.align.seed = std::strtoull(argv[17], nullptr, 10);
      p.keypoints = kp;
      p.use_keypoints = true;
      RowMatrixd a, b;
      mvr_prerej_result at, full;
      const bool ok = src.alignPrerejective(tgt, p, a, &at);
      std::vector<pcl::FPFHSignature33> sf, tf;
      src.computeFPFH(rf, sf); tgt.computeFPFH(rf, tf);
      const bool ok_full = src.alignPrerejective(tgt, p, sf, tf, b, &full);
      pose("fpfh_T", at.T);
      std::printf("\"fpfh_ok\": [%d, %d], \"fpfh_same\": %d, \"fpfh_inliers\": %u, \"fpfh_best\": %d, ", (int)ok, (int)ok_full, (int)(same(at, full) && same_pose(a, b)),
                  at.inliers, at.best_iteration);
      const bool okp = src.alignPrerejectivePFH(tgt, p, a, &at);
      std::vector<pcl::PFHSignature125> sh, th;
      src.computePFH(rf, sh); tgt.computePFH(rf, th);
      const bool okp_full = src.alignPrerejective(tgt, p, sh, th, b, &full);
      pose("pfh_T", at.T);
      std::printf("\"pfh_ok\": [%d, %d], \"pfh_same\": %d, \"pfh_inliers\": %u, \"pfh_best\": %d", (int)okp, (int)okp_full, (int)(same(at, full) && same_pose(a, b)),
                  at.inliers, at.best_iteration);
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "surface_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
