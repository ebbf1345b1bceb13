// tests/cxx/boundary_driver.cpp -- drives the C++ layers of the boundary estimation and of the ISS keypoints with a border
// (pcl::BoundaryEstimation and pcl::ISSKeypoint3D in mvr/registration.hpp, ScanCloud::detectBoundary and
// ScanCloud::detectKeypoints with border parameters in mvr/registrator.hpp) on a cloud and its normals read from files and prints
// what they return as JSON; tests/test_gpu_boundary_cxx.py compares it with the Python path (Context.boundary,
// Context.iss_keypoints) on the same cloud.
//
// usage: boundary_driver <cloud.f32> <normals.f32> <radius> <salient_radius> <non_max_radius> <min_neighbors> <border_radius>
//                        <normal_radius> <angle_threshold>
//        (the files: n x 4 floats, x y z 1 and nx ny nz 0)
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

int main(int argc, char **argv)
{
  if (argc < 10) { std::fprintf(stderr, "usage: %s cloud normals radius salient non_max min_neighbors border_radius normal_radius angle_threshold\n", argv[0]); return 2; }
  const double radius = std::atof(argv[3]);
  mvr_iss_params kp = mvr_iss_params();
  kp.salient_radius = std::atof(argv[4]); kp.non_max_radius = std::atof(argv[5]); kp.gamma_21 = kp.gamma_32 = 0.975; kp.min_neighbors = std::atoi(argv[6]);
  const double border_radius = std::atof(argv[7]), normal_radius = std::atof(argv[8]);
  const float angle = (float)std::atof(argv[9]);
  try {
    std::vector<float> xyz, nrm;
    if (!load(argv[1], xyz) || !load(argv[2], nrm) || xyz.size() != nrm.size()) return 3;
    const size_t n = xyz.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    typedef pcl::PointCloud<pcl::Normal> Normals;
    Cloud::Ptr model(new Cloud());
    Normals::Ptr normals(new Normals());
    model->resize(n); normals->resize(n);
    for (size_t i = 0; i < n; ++i) {
      (*model)[i].x = xyz[4 * i]; (*model)[i].y = xyz[4 * i + 1]; (*model)[i].z = xyz[4 * i + 2];
      (*normals)[i].normal_x = nrm[4 * i]; (*normals)[i].normal_y = nrm[4 * i + 1]; (*normals)[i].normal_z = nrm[4 * i + 2];
    }
    pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>());
    std::printf("{");
    {   // pcl::BoundaryEstimation, PCL's call order
      pcl::PointCloud<pcl::Boundary> out;
      pcl::BoundaryEstimation<pcl::PointXYZ, pcl::Normal, pcl::Boundary> est;
      std::printf("\"default_angle\": %u, ", bits(est.getAngleThreshold()));
      est.setInputCloud(model);
      est.setInputNormals(normals);
      est.setSearchMethod(tree);
      est.setRadiusSearch(radius);
      est.compute(out);
      std::vector<uint32_t> f;
      for (size_t i = 0; i < out.size(); ++i) f.push_back(out[i].boundary_point);
      u32s("be_default", f);
      est.setAngleThreshold(angle);
      est.compute(out);
      f.clear();
      for (size_t i = 0; i < out.size(); ++i) f.push_back(out[i].boundary_point);
      u32s("be_angle", f);
      // refusals: the k-neighbour mode; no normals; no radius
      std::vector<size_t> sz;
      est.setKSearch(10);
      out.resize(3); est.compute(out); sz.push_back(out.size());
      pcl::BoundaryEstimation<pcl::PointXYZ, pcl::Normal> no_normals, no_radius;
      no_normals.setInputCloud(model); no_normals.setRadiusSearch(radius);
      out.resize(3); no_normals.compute(out); sz.push_back(out.size());
      no_radius.setInputCloud(model); no_radius.setInputNormals(normals);
      out.resize(3); no_radius.compute(out); sz.push_back(out.size());
      u32s("be_refused", sz);
    }
    {   // pcl::ISSKeypoint3D with a border: the caller's normals, then a normal radius
      Cloud::Ptr keypoints(new Cloud());
      pcl::ISSKeypoint3D<pcl::PointXYZ, pcl::PointXYZ> iss;
      iss.setSearchMethod(tree);
      iss.setSalientRadius(kp.salient_radius);
      iss.setNonMaxRadius(kp.non_max_radius);
      iss.setMinNeighbors(kp.min_neighbors);
      iss.setNormals(normals);
      iss.setBorderRadius(border_radius);
      iss.setInputCloud(model);
      iss.compute(*keypoints);
      u32s("iss_normals_index", iss.getKeypointsIndices()->indices);
      std::vector<uint32_t> pts;
      for (size_t i = 0; i < keypoints->size(); ++i) { pts.push_back(bits((*keypoints)[i].x)); pts.push_back(bits((*keypoints)[i].y)); pts.push_back(bits((*keypoints)[i].z)); }
      u32s("iss_normals_points", pts);
      iss.setAngleThreshold(angle);
      iss.compute(*keypoints);
      u32s("iss_angle_index", iss.getKeypointsIndices()->indices);
      pcl::ISSKeypoint3D<pcl::PointXYZ> own;      // the defaulted PointOutT and NormalT
      own.setSalientRadius(kp.salient_radius); own.setNonMaxRadius(kp.non_max_radius); own.setMinNeighbors(kp.min_neighbors);
      own.setNormalRadius(normal_radius);
      own.setBorderRadius(border_radius);
      own.setInputCloud(model);
      own.compute(*keypoints);
      u32s("iss_normal_radius_index", own.getKeypointsIndices()->indices);
      // refused: normals of another size
      Normals::Ptr fewer(new Normals());
      fewer->resize(n ? n - 1 : 1);
      iss.setNormals(fewer);
      keypoints->resize(3); iss.compute(*keypoints);
      std::printf("\"iss_refused\": %zu, ", keypoints->size() + iss.getKeypointsIndices()->indices.size());
    }
    {   // ScanCloud::detectBoundary and detectKeypoints with a border, with the normals of estimateNormals
      ScanCloud scan;
      scan.points.resize(n);
      for (size_t i = 0; i < n; ++i) { scan.points.points[i].x = xyz[4 * i]; scan.points.points[i].y = xyz[4 * i + 1]; scan.points.points[i].z = xyz[4 * i + 2]; }
      mvr_iss_border_params b = mvr_iss_border_params();
      b.border_radius = border_radius; b.angle_threshold = 1.57079632679489661923;
      mvr_boundary_params bp = mvr_boundary_params();
      bp.radius = radius; bp.angle_threshold = 1.57079632679489661923;
      std::vector<uint32_t> key(7), plain;
      std::vector<uint8_t> flag(7);
      const bool no_normals = scan.detectKeypoints(kp, b, key), no_normals_b = scan.detectBoundary(bp, flag);
      std::printf("\"scan_refused\": [%d, %zu, %d, %zu], ", (int)no_normals, key.size(), (int)no_normals_b, flag.size());
      scan.estimateNormals(0, normal_radius);
      const size_t before = scan.points.size();
      const bool ok = scan.detectKeypoints(kp, b, key);
      u32s("scan_index", key);
      b.border_radius = 0.0;
      const bool ok0 = scan.detectKeypoints(kp, b, plain);
      u32s("scan_no_border_index", plain);
      scan.detectKeypoints(kp, plain);
      u32s("scan_plain_index", plain);
      const bool okb = scan.detectBoundary(bp, flag);
      u32s("scan_boundary", flag);
      b.border_radius = border_radius; b.angle_threshold = 0.1;
      const bool bad = scan.detectKeypoints(kp, b, plain);
      ScanCloud::PrerejectiveParams pp;
      std::printf("\"scan_ok\": [%d, %d, %d], \"scan_bad_angle\": [%d, %zu], \"scan_untouched\": %d, \"border_off_by_default\": %d",
                  (int)ok, (int)ok0, (int)okb, (int)bad, plain.size(), (int)(scan.points.size() == before), (int)(pp.border.border_radius == 0.0));
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "boundary_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
