// tests/cxx/cluster_driver.cpp -- drives the C++ layers of the Euclidean cluster extraction (pcl::EuclideanClusterExtraction and
// pcl::extractEuclideanClusters in mvr/registration.hpp; ScanCloud::extractClusters / keepLargestClusters and
// Registrator::setObjectIsolation in mvr/registrator.hpp) on a cloud read from a file and prints what they return as JSON;
// tests/test_gpu_cluster_cxx.py compares it with the Python path (Context.euclidean_clusters) on the same cloud.
//
// usage: cluster_driver <cloud.f32> <normals.f32> <tolerance> <min_size> <max_size> <eps_angle> <keep> <folder>
//        (the files: n x 4 floats; the folder: saveRegisteredPoints writes into its subfolders off, direct, on, off_again)
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

// clusters as JSON: a list of index lists
static void lists(const char *key, const std::vector<pcl::PointIndices> &c)
{
  std::printf("\"%s\": [", key);
  for (size_t k = 0; k < c.size(); ++k) {
    std::printf(k ? ",[" : "[");
    for (size_t i = 0; i < c[k].indices.size(); ++i) std::printf(i ? ",%d" : "%d", c[k].indices[i]);
    std::printf("]");
  }
  std::printf("], ");
}

int main(int argc, char **argv)
{
  if (argc < 9) { std::fprintf(stderr, "usage: %s cloud normals tolerance min_size max_size eps_angle keep folder\n", argv[0]); return 2; }
  const double tolerance = std::atof(argv[3]);
  const int min_size = std::atoi(argv[4]), max_size = std::atoi(argv[5]);
  const double eps_angle = std::atof(argv[6]);
  const uint32_t keep = (uint32_t)std::atoi(argv[7]);
  const std::string folder = argv[8];
  try {
    std::vector<float> xyz, nrm;
    if (!load(argv[1], xyz) || !load(argv[2], nrm) || nrm.size() != xyz.size()) return 3;
    const size_t n = xyz.size() / 4;
    typedef pcl::PointCloud<pcl::PointXYZ> Cloud;
    Cloud::Ptr cloud(new Cloud());
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>());
    pcl::PointCloud<pcl::PointNormal>::Ptr both(new pcl::PointCloud<pcl::PointNormal>());
    cloud->resize(n); normals->resize(n); both->resize(n);
    for (size_t i = 0; i < n; ++i) {
      (*cloud)[i].x = xyz[4 * i]; (*cloud)[i].y = xyz[4 * i + 1]; (*cloud)[i].z = xyz[4 * i + 2];
      (*normals)[i].normal_x = nrm[4 * i]; (*normals)[i].normal_y = nrm[4 * i + 1]; (*normals)[i].normal_z = nrm[4 * i + 2];
      (*both)[i].x = xyz[4 * i]; (*both)[i].y = xyz[4 * i + 1]; (*both)[i].z = xyz[4 * i + 2];
      (*both)[i].normal_x = nrm[4 * i]; (*both)[i].normal_y = nrm[4 * i + 1]; (*both)[i].normal_z = nrm[4 * i + 2];
    }
    std::printf("{");
    {   // pcl::EuclideanClusterExtraction, PCL's call order
      pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>());
      tree->setInputCloud(cloud);
      std::vector<pcl::PointIndices> cluster_indices;
      pcl::EuclideanClusterExtraction<pcl::PointXYZ> ec;
      std::printf("\"defaults\": [%d, %d, %d], ", ec.getMinClusterSize(), ec.getMaxClusterSize(), (int)(ec.getClusterTolerance() == 0.0));
      ec.setClusterTolerance(tolerance);
      ec.setMinClusterSize(min_size);
      ec.setMaxClusterSize(max_size);
      ec.setSearchMethod(tree);
      ec.setInputCloud(cloud);
      ec.extract(cluster_indices);
      lists("ece", cluster_indices);
      std::printf("\"ece_result\": [%u, %u, %u], ", ec.getResult().n_components, ec.getResult().too_small, ec.getResult().too_large);
      // setIndices: every third point
      pcl::PointIndices::Ptr third(new pcl::PointIndices());
      for (size_t i = 0; i < n; i += 3) third->indices.push_back((int)i);
      ec.setIndices(third);
      ec.extract(cluster_indices);
      lists("ece_third", cluster_indices);
      // refusals: no tolerance, an index outside the cloud, no input
      pcl::EuclideanClusterExtraction<pcl::PointXYZ> unset;
      unset.setInputCloud(cloud);
      std::vector<pcl::PointIndices> a(2), b(2), c(2);
      unset.extract(a);
      pcl::PointIndices::Ptr bad(new pcl::PointIndices());
      bad->indices.push_back((int)n);
      ec.setIndices(bad);
      ec.extract(b);
      pcl::EuclideanClusterExtraction<pcl::PointXYZ> none;
      none.setClusterTolerance(tolerance);
      none.extract(c);
      std::printf("\"refused\": [%zu, %zu, %zu], ", a.size(), b.size(), c.size());
      // the free function with normals: two clouds, and a PointNormal cloud with its own
      std::vector<pcl::PointIndices> with_normals, own_normals;
      pcl::extractEuclideanClusters(*cloud, *normals, (float)tolerance, tree, with_normals, eps_angle, (unsigned)min_size, (unsigned)max_size);
      lists("normals", with_normals);
      pcl::search::KdTree<pcl::PointNormal>::Ptr tree_n(new pcl::search::KdTree<pcl::PointNormal>());
      pcl::extractEuclideanClusters(*both, (float)tolerance, tree_n, own_normals, eps_angle, (unsigned)min_size, (unsigned)max_size);
      lists("own_normals", own_normals);
      pcl::PointCloud<pcl::Normal> fewer;
      fewer.resize(n ? n - 1 : 1);
      std::vector<pcl::PointIndices> mismatch(2);
      pcl::extractEuclideanClusters(*cloud, fewer, (float)tolerance, tree, mismatch, eps_angle);
      std::printf("\"normals_refused\": %zu, ", mismatch.size());
    }
    ScanCloud::ClusterParams cp;
    cp.tolerance = tolerance; cp.min_size = (uint32_t)min_size; cp.max_size = (uint32_t)max_size;
    auto fill = [&](ScanCloud &scan) {
      scan.points.resize(n);
      scan.rich.resize(n);
      for (size_t i = 0; i < n; ++i) {
        scan.points.points[i].x = xyz[4 * i]; scan.points.points[i].y = xyz[4 * i + 1]; scan.points.points[i].z = xyz[4 * i + 2];
        scan.rich[i].x = xyz[4 * i]; scan.rich[i].y = xyz[4 * i + 1]; scan.rich[i].z = xyz[4 * i + 2]; scan.rich[i].curvature = (float)i;
        scan.rich[i].normal_x = nrm[4 * i]; scan.rich[i].normal_y = nrm[4 * i + 1]; scan.rich[i].normal_z = nrm[4 * i + 2];
      }
    };
    {   // ScanCloud::extractClusters and keepLargestClusters
      ScanCloud scan;
      fill(scan);
      std::vector<std::vector<uint32_t> > clusters;
      const bool ok = scan.extractClusters(cp, clusters);
      std::vector<pcl::PointIndices> as_pi(clusters.size());
      for (size_t k = 0; k < clusters.size(); ++k) as_pi[k].indices.assign(clusters[k].begin(), clusters[k].end());
      lists("scan_clusters", as_pi);
      ScanCloud::ClusterParams with = cp;
      with.eps_angle = eps_angle;
      scan.extractClusters(with, clusters);
      as_pi.assign(clusters.size(), pcl::PointIndices());
      for (size_t k = 0; k < clusters.size(); ++k) as_pi[k].indices.assign(clusters[k].begin(), clusters[k].end());
      lists("scan_clusters_normals", as_pi);
      std::printf("\"scan_ok\": [%d, %d], ", (int)ok, (int)(scan.points.size() == n && scan.rich.size() == n));
      ScanCloud::ClusterParams bad = cp;
      bad.tolerance = 0.0;
      std::vector<std::vector<uint32_t> > none(5);
      const bool refused = scan.extractClusters(bad, none);
      const size_t untouched = scan.keepLargestClusters(bad), zero_keep = scan.keepLargestClusters(cp, 0);
      std::printf("\"scan_refused\": [%d, %zu, %zu, %zu, %zu], ", (int)refused, none.size(), untouched, zero_keep, scan.points.size());
      const size_t dropped = scan.keepLargestClusters(cp, keep);
      std::printf("\"scan_dropped\": %zu, ", dropped);
      std::vector<uint32_t> pts, follow;
      for (size_t i = 0; i < scan.points.size(); ++i) { pts.push_back(bits(scan.points.points[i].x)); pts.push_back(bits(scan.points.points[i].y)); pts.push_back(bits(scan.points.points[i].z)); }
      u32s("scan_points", pts);
      for (size_t i = 0; i < scan.rich.size(); ++i) follow.push_back((uint32_t)scan.rich[i].curvature);
      u32s("scan_rich_follow", follow);
    }
    {   // Registrator::setObjectIsolation in front of saveRegisteredPoints: one registered view with the identity pose
      TurntableModel model;
      model.views.resize(1);
      fill(model.views[0]);
      model.views[0].setRegisterState(true);
      Registrator reg(&model);
      std::printf("\"isolation_off_by_default\": %d, ", (int)!reg.getObjectIsolation());
      io::RichCloud plain_cloud, merged, small;
      const size_t plain = reg.saveRegisteredPoints(0, folder + "/off", &plain_cloud);
      // the same cloud written without the Registrator: the bytes saveRegisteredPoints must produce with the isolation off
      const bool direct = io::savePCDFile(folder + "/direct/points.pcd", plain_cloud, io::PCD_BINARY_COMPRESSED) &&
                          io::savePointsASC(folder + "/direct/points.asc", plain_cloud);
      reg.setObjectIsolation(tolerance, (uint32_t)min_size, keep);
      const size_t written = reg.saveRegisteredPoints(0, folder + "/on", &merged), dropped = reg.lastIsolationDropped();
      const size_t written_leaf = reg.saveRegisteredPoints(0, folder + "/on", 4.0f, &small), dropped_leaf = reg.lastIsolationDropped();
      io::RichCloud back;
      const bool read = io::loadPCDFile(folder + "/on/points.pcd", back);
      ScanCloud same;
      fill(same);
      ScanCloud::ClusterParams ip;
      ip.tolerance = tolerance; ip.min_size = (uint32_t)min_size;
      const size_t by_hand = same.keepLargestClusters(ip, keep);
      bool equal = merged.size() == same.points.size();
      for (size_t i = 0; equal && i < merged.size(); ++i)
        equal = bits(merged[i].x) == bits(same.points.points[i].x) && bits(merged[i].y) == bits(same.points.points[i].y) &&
                bits(merged[i].z) == bits(same.points.points[i].z) && merged[i].curvature == same.rich[i].curvature;
      reg.setObjectIsolation(0.0, 1);
      const size_t off_again = reg.saveRegisteredPoints(0, folder + "/off_again");
      std::printf("\"isolation\": [%zu, %d, %zu, %zu, %zu, %zu, %d, %zu, %zu, %zu, %d, %zu, %d]", plain, (int)direct, written, dropped, by_hand, merged.size(),
                  (int)equal, written_leaf, dropped_leaf, small.size(), (int)read, back.size(),
                  (int)(!reg.getObjectIsolation() && off_again == plain && reg.lastIsolationDropped() == 0));
    }
    std::printf("}\n");
  } catch (const std::exception &e) {
    std::fprintf(stderr, "cluster_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
