// include/mvr/registrator.hpp -- the registration driver on top of the C-ABI: scan objects (raw points + pose +
// the reference's per-view text/PCD files) and a DEVICE-RESIDENT Registrator.
//
// What it stands for in the reference (mvr/src/registrator.cpp, mvr/src/point_cloud.cpp):
//   PointCloud::getTransformedPoints :290-303, initRotation :400-413, open :78-95, save :97-123,
//     load/saveTransformation :305-347, denoise :423-465                     -> ScanCloud
//   Registrator::getRotationMatrix :331-342, load/save (axis.txt) :258-308   -> Registrator (same formats)
//   registrationICP :517-588        -> Registrator::registrationICPDevice   (target grows in a device slot)
//   registrationLUM :611-664        -> Registrator::registrationLUMDevice   (all passes in one native call)
//   automaticRegistration :746-842, :877-990, :1008-1030 -> Registrator::automaticRegistrationDevice (in-place aligns, model grown in a slot)
//   computeError :466-515           -> Registrator::computeErrorDevice      (per-pair count + residual)
//   refineAxis :402-455             -> Registrator::refineAxis              (mvr_refine_axis)
//   saveRegisteredPoints :344-400, registration :719-744                    -> same names
// The Qt/OSG/file-tree plumbing (FileSystemModel, QtConcurrent, draggers, rendering, dialogs) is out of scope:
// `TurntableModel` is an in-memory stand-in for FileSystemModel::getPointCloud(object, view).
// The PCL-named call surface itself is exercised, in the reference's order of calls, by tests/cxx/call_surface.hpp.
#pragma once

#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <utility>
#include <vector>

#include <memory>

#include "io.hpp"
#include "registration.hpp"

namespace mvr {

typedef PointXYZ PCLPoint;                       // mvr/include/types.h:14
typedef PointCloud<PCLPoint> PCLPointCloud;      // mvr/include/types.h:17

class Registrator;

// what ScanCloud::radiusSearch returns: the rows of mvr_radius_search (mvr_hip.h) as CSR -- the neighbours of query i are
// indices[offsets[i] .. offsets[i + 1]) with their squared distances beside them
struct NeighborLists {
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> indices;
  std::vector<float> sqr_distances;
  size_t rows() const { return offsets.empty() ? 0 : offsets.size() - 1; }
};

// One scan: raw points + its pose (osg::Matrix of the reference's
// osg::MatrixTransform base) + the flags the driver consults.
class ScanCloud {
 public:
  PCLPointCloud points;          // what the registration path sees (point_cloud.cpp:297-299 strips the rest)
  io::RichCloud rich;            // the full PointXYZRGBNormal records when the scan came from a PCD file; may be empty
  int view = 0;
  bool shown = true;
  bool registered = false;

  size_t size() const { return points.size(); }
  // a counter the device-resident Registrator watches: bump it (touch) after editing `points` by hand
  unsigned long long revision() const { return revision_; }
  void touch() { ++revision_; }

  // PointCloud::open (point_cloud.cpp:78-95): the PCD file (ascii / binary / binary_compressed), the pose from the
  // transformation.txt beside it, registered = view 0 or a non-identity pose.  false: nothing changed.
  bool open(const std::string &filename)
  {
    io::RichCloud loaded;
    if (!io::loadPCDFile(filename, loaded)) return false;
    rich.swap(loaded);
    io::toXYZ(rich, points);
    filename_ = filename;
    matrix_.makeIdentity();
    loadTransformation(folder() + "/transformation.txt");
    registered = (view == 0) || !matrix_.isIdentity();
    touch();
    return true;
  }
  // PointCloud::save (point_cloud.cpp:97-123): "*.ply" = the XYZ points in the turntable's canonical frame (pivot at
  // the origin, axis along +z; the reference hard-codes its calibration there) as an ASCII PLY; anything else = the
  // rich cloud as binary_compressed PCD.
  bool save(const std::string &filename) const
  {
    if (filename.size() >= 3 && filename.compare(filename.size() - 3, 3, "ply") == 0) {
      const RowMatrixd transformation = RowMatrixd::translate(13.382786, -50.223461, -917.477600) *
                                        RowMatrixd::rotateFromTo(-0.054323, -0.814921, -0.577020, 0.0, 0.0, 1.0);
      PCLPointCloud canon;
      for (size_t i = 0; i < points.size(); ++i) {
        const PCLPoint &p = points.points[i];
        float o[3];
        for (int k = 0; k < 3; ++k)
          o[k] = (float)(transformation(0, k) * p.x + transformation(1, k) * p.y + transformation(2, k) * p.z + transformation(3, k));
        canon.push_back(PCLPoint(o[0], o[1], o[2]));
      }
      return io::savePLYFile(filename, canon);
    }
    if (rich.size() == points.size()) return io::savePCDFile(filename, rich, io::PCD_BINARY_COMPRESSED);
    io::RichCloud plain(points.size());
    for (size_t i = 0; i < points.size(); ++i) { plain[i].x = points.points[i].x; plain[i].y = points.points[i].y; plain[i].z = points.points[i].z; }
    return io::savePCDFile(filename, plain, io::PCD_BINARY_COMPRESSED);
  }
  const std::string &filename() const { return filename_; }
  std::string folder() const { const size_t k = filename_.find_last_of('/'); return k == std::string::npos ? std::string(".") : filename_.substr(0, k); }
  const RowMatrixd &getMatrix() const { return matrix_; }
  void setMatrix(const RowMatrixd &m) { matrix_ = m; }
  bool isShown() const { return shown; }
  bool isRegistered() const { return registered; }
  void setRegisterState(bool r) { registered = r; }
  int getView() const { return view; }

  // point_cloud.cpp:290-303 -- (x,y,z) * M in double, rounded to float.  K1 on the GPU.
  void getTransformedPoints(PCLPointCloud &out) const
  {
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    d.check(mvr_cloud_transform(d.ctx(), s.s, s.s, matrix_.asColumnMajorColumnVector()), "mvr_cloud_transform");
    d.download(s.s, out);
  }
  void initRotation(const Registrator &r);        // point_cloud.cpp:400-413

  // point_cloud.cpp:423-465: drop the connected components (points linked when <= triangle_length apart -- the
  // reference's short Delaunay edges give the same components) with fewer than segment_threshold points; the
  // survivors are stored component after component, as the reference's denoised_cloud.  Returns the noise count.
  // A point with a non-finite x, y or z (a scanner file with is_dense == false) is linked to nothing: a component of its own,
  // kept exactly when segment_threshold <= 1, and no part of the grid's sizing (rules D1-D4 of mvr_cloud_denoise in mvr_hip.h).
  size_t denoise(int segment_threshold, double triangle_length)
  {
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    d.upload(s.s, points);
    size_t kept = 0, comps = 0;
    std::vector<uint32_t> index(before ? before : 1);
    d.check(mvr_cloud_denoise(d.ctx(), s.s, segment_threshold, triangle_length, &kept, &comps, index.data()), "mvr_cloud_denoise");
    d.download(s.s, points);
    if (rich.size() == before) {                   // colours and normals follow their points
      io::RichCloud r(kept);
      for (size_t k = 0; k < kept; ++k) r[k] = rich[index[k]];
      rich.swap(r);
    }
    touch();
    return before - kept;
  }

  // EXTENSION (pcl::NormalEstimation on the raw points, viewpoint at the origin -- the sensor of a raw turntable scan):
  // k nearest neighbours (k > 0) or every point within `radius` (k = 0) per point, on the GPU.  Fills the normals and the
  // curvature of `rich` (made from `points` first when it does not hold one record per point); `points` and the pose stay as
  // they are.  save() and Registrator::saveRegisteredPoints then write these normals.
  void estimateNormals(int k, double radius = 0.0)
  {
    Device &d = Device::instance();
    SlotGuard s;
    const size_t n = points.size();
    if (rich.size() != n) {
      io::RichCloud r(n);
      for (size_t i = 0; i < n; ++i) { r[i].x = points.points[i].x; r[i].y = points.points[i].y; r[i].z = points.points[i].z; }
      rich.swap(r);
    }
    d.upload(s.s, points);
    mvr_normal_params p;
    p.k = k; p.radius = radius; p.fma_dist = 0;
    p.viewpoint[0] = p.viewpoint[1] = p.viewpoint[2] = 0.f;
    std::vector<float> curv(n ? n : 1), nrm(4 * (n ? n : 1));
    float *cp = curv.data();
    d.check(mvr_cloud_estimate_normals(d.ctx(), 1, &s.s, &p, &cp), "mvr_cloud_estimate_normals");
    size_t got = 0;
    if (n) d.check(mvr_cloud_download_normals(d.ctx(), s.s, nrm.data(), n, 16, &got), "mvr_cloud_download_normals");
    for (size_t i = 0; i < n; ++i) {
      rich[i].normal_x = nrm[4 * i]; rich[i].normal_y = nrm[4 * i + 1]; rich[i].normal_z = nrm[4 * i + 2]; rich[i].curvature = curv[i];
    }
  }

  // EXTENSION (pcl::VoxelGrid with a cubic leaf, mvr_cloud_voxel_grid): `points` become the centroids of the occupied
  // voxels, in ascending voxel index; voxels with fewer than min_points points are dropped.  When `rich` holds one record
  // per point it is replaced too: xyz and normals come from the GPU (the rich normals go into the slot first, and the
  // voxel's normal sum is normalised, as PCL >= 1.8); rgb is the per-channel mean truncated to an integer (PCL's
  // AccumulatorRGBA) and curvature the f64 mean rounded to f32, both averaged on the host through the voxel map.  When
  // PCL's integer indices would overflow, nothing changes but PCL's warning.  Returns the number of points removed.
  size_t voxelDownsample(float leaf, unsigned min_points = 0)
  {
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    const bool with_rich = before > 0 && rich.size() == before;
    d.upload(s.s, points);
    if (with_rich) {
      std::vector<float> nrm(4 * before);
      for (size_t i = 0; i < before; ++i) { nrm[4 * i] = rich[i].normal_x; nrm[4 * i + 1] = rich[i].normal_y; nrm[4 * i + 2] = rich[i].normal_z; nrm[4 * i + 3] = 0.f; }
      d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), before, 16), "mvr_cloud_upload_normals");
    }
    const float lf[3] = {leaf, leaf, leaf};
    size_t kept = 0;
    int passthrough = 0;
    std::vector<uint32_t> vox(before ? before : 1);
    d.check(mvr_cloud_voxel_grid(d.ctx(), s.s, s.s, lf, min_points, &kept, vox.data(), &passthrough), "mvr_cloud_voxel_grid");
    if (passthrough) {
      std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
      return 0;
    }
    d.download(s.s, points);
    if (with_rich) {
      std::vector<float> nrm(4 * (kept ? kept : 1));
      size_t got = 0;
      if (kept) d.check(mvr_cloud_download_normals(d.ctx(), s.s, nrm.data(), kept, 16, &got), "mvr_cloud_download_normals");
      std::vector<unsigned long long> rgb(3 * kept, 0ull), cnt(kept, 0ull);
      std::vector<double> curv(kept, 0.0);
      for (size_t i = 0; i < before; ++i) {
        const uint32_t o = vox[i];
        if (o == 0xFFFFFFFFu) continue;
        rgb[3 * o] += rich[i].r; rgb[3 * o + 1] += rich[i].g; rgb[3 * o + 2] += rich[i].b;
        curv[o] += (double)rich[i].curvature;
        ++cnt[o];
      }
      io::RichCloud r(kept);
      for (size_t k = 0; k < kept; ++k) {
        r[k].x = points.points[k].x; r[k].y = points.points[k].y; r[k].z = points.points[k].z;
        r[k].r = (uint8_t)(rgb[3 * k] / cnt[k]); r[k].g = (uint8_t)(rgb[3 * k + 1] / cnt[k]); r[k].b = (uint8_t)(rgb[3 * k + 2] / cnt[k]);
        r[k].normal_x = nrm[4 * k]; r[k].normal_y = nrm[4 * k + 1]; r[k].normal_z = nrm[4 * k + 2];
        r[k].curvature = (float)(curv[k] / (double)cnt[k]);
      }
      rich.swap(r);
    }
    touch();
    return before - kept;
  }

  // EXTENSION (pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval on the raw points, on the GPU): `points` keep the
  // inliers in their original order (rules: mvr_cloud_statistical_outlier_removal / mvr_cloud_radius_outlier_removal in
  // mvr_hip.h); when `rich` holds one record per point, the records follow their points as in denoise().  Parameters outside
  // their range print an error and change nothing.  Returns the number of points removed.
  size_t removeStatisticalOutliers(int mean_k, double stddev_mul)
  {
    if (mean_k < 1 || mean_k > MVR_MAX_KNN || !std::isfinite(stddev_mul)) {
      std::fprintf(stderr, "[ScanCloud::removeStatisticalOutliers] mean_k (%d) must be in 1..%d and the multiplier (%f) finite.\n", mean_k, MVR_MAX_KNN, stddev_mul);
      return 0;
    }
    mvr_sor_params p;
    p.mean_k = mean_k; p.stddev_mul = stddev_mul; p.negative = 0; p.fma_dist = 0;
    return removeOutliers(&p, nullptr);
  }
  size_t removeRadiusOutliers(double radius, int min_neighbors)
  {
    if (!(std::isfinite(radius) && radius > 0.0) || min_neighbors < 0) {
      std::fprintf(stderr, "[ScanCloud::removeRadiusOutliers] The radius (%f) must be finite and > 0, min_neighbors (%d) >= 0.\n", radius, min_neighbors);
      return 0;
    }
    mvr_ror_params p;
    p.radius = radius; p.min_neighbors = min_neighbors; p.negative = 0; p.fma_dist = 0;
    return removeOutliers(nullptr, &p);
  }

  // EXTENSION (pcl::MovingLeastSquares on the raw points, on the GPU; rules: mvr_cloud_mls in mvr_hip.h): every point with at
  // least 3 neighbours within `radius` is moved onto the plane through them and, with order 2 and at least 6 neighbours, onto
  // the weighted quadratic over that plane; the others are dropped.  `points` are replaced; when `rich` holds one record per
  // point, the records follow through the kept indices and take the new coordinates.  With compute_normals the normals
  // (oriented towards the origin, the sensor of a raw scan) and the curvature of `rich` come from the fit too (`rich` is made
  // from `points` first when it does not hold one record per point).  Parameters outside their range print an error and
  // change nothing.  Returns the number of points dropped.
  size_t smooth(double radius, int order = 2, bool compute_normals = false)
  {
    if (!(std::isfinite(radius) && radius > 0.0) || order < 0 || order > 2) {
      std::fprintf(stderr, "[ScanCloud::smooth] The radius (%f) must be finite and > 0, the order (%d) in 0..2.\n", radius, order);
      return 0;
    }
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    if (compute_normals && rich.size() != before) {
      io::RichCloud r(before);
      for (size_t i = 0; i < before; ++i) { r[i].x = points.points[i].x; r[i].y = points.points[i].y; r[i].z = points.points[i].z; }
      rich.swap(r);
    }
    d.upload(s.s, points);
    mvr_mls_params p;
    p.radius = radius; p.order = order; p.sqr_gauss_param = 0.0; p.compute_normals = compute_normals ? 1 : 0; p.orient = 0;
    p.viewpoint[0] = p.viewpoint[1] = p.viewpoint[2] = 0.f; p.fma_dist = 0;
    size_t kept = 0;
    std::vector<uint32_t> index(before ? before : 1);
    std::vector<float> curv(before ? before : 1), nrm(4 * (before ? before : 1));
    d.check(mvr_cloud_mls(d.ctx(), s.s, s.s, &p, &kept, index.data(), curv.data()), "mvr_cloud_mls");
    d.download(s.s, points);
    size_t got = 0;
    if (compute_normals && kept) d.check(mvr_cloud_download_normals(d.ctx(), s.s, nrm.data(), kept, 16, &got), "mvr_cloud_download_normals");
    if (rich.size() == before) {
      io::RichCloud r(kept);
      for (size_t k = 0; k < kept; ++k) {
        r[k] = rich[index[k]];
        r[k].x = points.points[k].x; r[k].y = points.points[k].y; r[k].z = points.points[k].z;
        if (compute_normals) { r[k].normal_x = nrm[4 * k]; r[k].normal_y = nrm[4 * k + 1]; r[k].normal_z = nrm[4 * k + 2]; r[k].curvature = curv[k]; }
      }
      rich.swap(r);
    }
    touch();
    return before - kept;
  }

  // EXTENSION (pcl::SACSegmentation with SAC_RANSAC on the raw points, on the GPU; rules: mvr_cloud_segment_plane in mvr_hip.h):
  // the largest plane of the scan -- the platter or the table the object stands on -- within `threshold`; with an axis the
  // model is SACMODEL_PERPENDICULAR_PLANE (the plane's normal within eps_angle of the axis: a turntable's platter), without
  // one SACMODEL_PLANE.  segmentPlane fills the inliers' indices (ascending) and the four coefficients and changes nothing;
  // removePlane takes the inliers out of `points` (ExtractIndices with setNegative(true)), `rich` following as in denoise(), and
  // returns the number of points removed.  Parameters outside their range print an error and change nothing; so does a scan
  // without a plane (segmentPlane then returns false).
  struct PlaneParams {
    double threshold = 0.5;
    int max_iterations = 1000;
    double probability = 0.99;
    bool optimize = true;
    bool perpendicular = false;            // with it: the axis and the largest angle between it and the plane's normal
    double axis[3] = {0.0, 0.0, 1.0}, eps_angle = 0.1;
    uint64_t seed = 0;
  };
  bool segmentPlane(const PlaneParams &pp, std::vector<uint32_t> &inliers, float coefficients[4], mvr_sac_result *result = nullptr) const
  {
    inliers.clear();
    for (int k = 0; k < 4; ++k) coefficients[k] = 0.f;
    mvr_sac_params p;
    if (!planeParams(pp, false, p)) return false;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    std::vector<uint32_t> index(points.size() ? points.size() : 1);
    mvr_sac_result r;
    d.check(mvr_cloud_segment_plane(d.ctx(), -1, s.s, &p, &r, nullptr, index.data(), nullptr, nullptr, 0), "mvr_cloud_segment_plane");
    if (result) *result = r;
    if (!r.found) return false;
    inliers.assign(index.begin(), index.begin() + (std::ptrdiff_t)r.inliers);
    for (int k = 0; k < 4; ++k) coefficients[k] = r.coefficients[k];
    return true;
  }
  size_t removePlane(const PlaneParams &pp, float coefficients[4] = nullptr)
  {
    mvr_sac_params p;
    if (!planeParams(pp, true, p)) return 0;
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    d.upload(s.s, points);
    std::vector<uint32_t> index(before ? before : 1);
    mvr_sac_result r;
    size_t kept = 0;
    d.check(mvr_cloud_segment_plane(d.ctx(), s.s, s.s, &p, &r, &kept, index.data(), nullptr, nullptr, 0), "mvr_cloud_segment_plane");
    if (coefficients) for (int k = 0; k < 4; ++k) coefficients[k] = r.coefficients[k];
    if (!r.found || r.inliers == 0) return 0;
    d.download(s.s, points);
    if (rich.size() == before) {                   // colours and normals follow their points
      io::RichCloud out(kept);
      size_t k = 0, w = 0;
      for (size_t i = 0; i < before; ++i) {
        if (k < r.inliers && index[k] == i) ++k;
        else out[w++] = rich[i];
      }
      rich.swap(out);
    }
    touch();
    return before - kept;
  }

  // EXTENSION (pcl::EuclideanClusterExtraction on the raw points, on the GPU; rules E1-E8: mvr_cloud_euclidean_clusters in
  // mvr_hip.h): what is left once the platter is out is the object plus whatever stood beside it.  extractClusters fills the
  // clusters' indices -- largest first, members ascending -- and changes nothing; keepLargestClusters keeps the points of the
  // first `keep` clusters in their original order, `rich` following as in removePlane, and returns the number of points it
  // dropped.  With eps_angle > 0 the normals of `rich` must agree too (one record per point, as computeFPFH).  Parameters
  // outside their range print an error and change nothing (extractClusters then returns false).
  struct ClusterParams {
    double tolerance = 2.5;
    uint32_t min_size = 1, max_size = 0x7FFFFFFFu;
    double eps_angle = 0.0;                // > 0: extractEuclideanClusters with the normals of `rich`, in (0, pi]
  };
  bool extractClusters(const ClusterParams &cp, std::vector<std::vector<uint32_t> > &clusters, mvr_cluster_result *result = nullptr) const
  {
    clusters.clear();
    mvr_cluster_params p;
    if (!clusterParams(cp, 1, p)) return false;
    Device &d = Device::instance();
    SlotGuard s;
    const size_t n = points.size();
    uploadForClusters(d, s.s, p);
    std::vector<uint32_t> offset(n + 2), member(n ? n : 1);
    mvr_cluster_result r;
    d.check(mvr_cloud_euclidean_clusters(d.ctx(), -1, s.s, &p, nullptr, 0, &r, nullptr, offset.data(), offset.size(), member.data(), nullptr),
            "mvr_cloud_euclidean_clusters");
    if (result) *result = r;
    clusters.resize(r.n_clusters);
    for (uint32_t c = 0; c < r.n_clusters; ++c) clusters[c].assign(member.begin() + offset[c], member.begin() + offset[c + 1]);
    return true;
  }
  size_t keepLargestClusters(const ClusterParams &cp, uint32_t keep = 1, mvr_cluster_result *result = nullptr)
  {
    mvr_cluster_params p;
    if (!clusterParams(cp, keep, p)) return 0;
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    uploadForClusters(d, s.s, p);
    std::vector<uint32_t> label(before ? before : 1);
    mvr_cluster_result r;
    size_t kept = 0;
    d.check(mvr_cloud_euclidean_clusters(d.ctx(), s.s, s.s, &p, nullptr, 0, &r, &kept, nullptr, 0, nullptr, label.data()), "mvr_cloud_euclidean_clusters");
    if (result) *result = r;
    if (kept == before) return 0;
    d.download(s.s, points);
    if (rich.size() == before) {                   // colours and normals follow their points
      io::RichCloud out(kept);
      size_t w = 0;
      for (size_t i = 0; i < before; ++i)
        if (label[i] < keep) out[w++] = rich[i];
      rich.swap(out);
    }
    touch();
    return before - kept;
  }

  // EXTENSION (pcl::FPFHEstimation on the raw points, on the GPU; rules: mvr_cloud_fpfh in mvr_hip.h): one 33-bin signature per
  // point from every neighbour within `radius`, with the normals of `rich` (estimateNormals, smooth with compute_normals, or
  // a file that carries them).  Without one rich record per point, or with a radius that is not finite and > 0, it prints an
  // error, leaves `out` empty and returns false.  `points`, `rich` and the pose stay as they are.
  bool computeFPFH(double radius, std::vector<FPFHSignature33> &out) const
  {
    out.clear();
    const size_t n = points.size();
    if (rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::computeFPFH] The cloud has no normals (%zu points, %zu records): call estimateNormals first.\n", n, rich.size());
      return false;
    }
    if (!(std::isfinite(radius) && radius > 0.0)) {
      std::fprintf(stderr, "[ScanCloud::computeFPFH] The radius (%f) must be finite and > 0.\n", radius);
      return false;
    }
    out.resize(n);
    if (!n) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    std::vector<float> nrm(4 * n);
    for (size_t i = 0; i < n; ++i) { nrm[4 * i] = rich[i].normal_x; nrm[4 * i + 1] = rich[i].normal_y; nrm[4 * i + 2] = rich[i].normal_z; nrm[4 * i + 3] = 0.f; }
    d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
    mvr_fpfh_params p;
    p.radius = radius; p.fma_dist = 0;
    d.check(mvr_cloud_fpfh(d.ctx(), s.s, &p, out[0].histogram, nullptr, nullptr), "mvr_cloud_fpfh");
    return true;
  }

  // EXTENSION (pcl::PFHEstimation on the raw points, on the GPU; rules: mvr_cloud_pfh in mvr_hip.h): one 125-bin signature per
  // point from every PAIR of its neighbours within `radius`, with the normals of `rich`; refusals as computeFPFH.
  bool computePFH(double radius, std::vector<PFHSignature125> &out) const
  {
    out.clear();
    const size_t n = points.size();
    if (rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::computePFH] The cloud has no normals (%zu points, %zu records): call estimateNormals first.\n", n, rich.size());
      return false;
    }
    if (!(std::isfinite(radius) && radius > 0.0)) {
      std::fprintf(stderr, "[ScanCloud::computePFH] The radius (%f) must be finite and > 0.\n", radius);
      return false;
    }
    out.resize(n);
    if (!n) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    uploadRichNormals(d, s.s);
    mvr_pfh_params p;
    p.radius = radius; p.k = 0; p.fma_dist = 0;
    d.check(mvr_cloud_pfh(d.ctx(), s.s, &p, out[0].histogram, nullptr, nullptr), "mvr_cloud_pfh");
    return true;
  }

  // EXTENSION (setIndices / setSearchSurface of pcl::FPFHEstimation and pcl::PFHEstimation; rules Q1-Q8: mvr_cloud_fpfh_at /
  // mvr_cloud_pfh_at in mvr_hip.h): the descriptors at chosen points only.  With `indices`, `out` holds indices.size() rows, row r
  // the signature of point indices[r] of this cloud, which is its own surface -- bit for bit the row computeFPFH / computePFH
  // give that point.  With `surface`, every raw point of THIS cloud is a query position (it needs no normals) over the points and
  // the normals of `surface`, and `out` holds one row per point of this cloud.  Refusals as computeFPFH, of the surface; an
  // index beyond the cloud prints an error too.
  bool computeFPFHAt(double radius, const std::vector<uint32_t> &indices, std::vector<FPFHSignature33> &out) const
  {
    return featuresAt("computeFPFHAt", radius, nullptr, &indices, out);
  }
  bool computePFHAt(double radius, const std::vector<uint32_t> &indices, std::vector<PFHSignature125> &out) const
  {
    return featuresAt("computePFHAt", radius, nullptr, &indices, out);
  }
  bool computeFPFHAt(const ScanCloud &surface, double radius, std::vector<FPFHSignature33> &out) const
  {
    return surface.featuresAt("computeFPFHAt", radius, this, nullptr, out);
  }
  bool computePFHAt(const ScanCloud &surface, double radius, std::vector<PFHSignature125> &out) const
  {
    return surface.featuresAt("computePFHAt", radius, this, nullptr, out);
  }
  // EXTENSION (pcl::NormalEstimation with setSearchSurface; mvr_cloud_estimate_normals_at): estimateNormals with the neighbours
  // taken from the raw points of `surface` -- the normals of a downsampled cloud from the scan it came from
  void estimateNormalsFrom(const ScanCloud &surface, int k, double radius = 0.0)
  {
    Device &d = Device::instance();
    SlotGuard s, t;
    const size_t n = points.size();
    if (rich.size() != n) {
      io::RichCloud r(n);
      for (size_t i = 0; i < n; ++i) { r[i].x = points.points[i].x; r[i].y = points.points[i].y; r[i].z = points.points[i].z; }
      rich.swap(r);
    }
    d.upload(s.s, points);
    d.upload(t.s, surface.points);
    mvr_normal_params p;
    p.k = k; p.radius = radius; p.fma_dist = 0;
    p.viewpoint[0] = p.viewpoint[1] = p.viewpoint[2] = 0.f;
    std::vector<float> curv(n ? n : 1), nrm(4 * (n ? n : 1));
    d.check(mvr_cloud_estimate_normals_at(d.ctx(), s.s, nullptr, 0, t.s, &p, 0, nrm.data(), curv.data()), "mvr_cloud_estimate_normals_at");
    for (size_t i = 0; i < n; ++i) {
      rich[i].normal_x = nrm[4 * i]; rich[i].normal_y = nrm[4 * i + 1]; rich[i].normal_z = nrm[4 * i + 2]; rich[i].curvature = curv[i];
    }
  }

  // EXTENSION (pcl::search::KdTree::radiusSearch for every point at once, on the GPU; rules RS1-RS11: mvr_radius_search in
  // mvr_hip.h): the neighbours within `radius` of every raw point of this cloud among its own points -- each row starts with the
  // point itself -- or of every raw point of `queries` among the points of this cloud; rows ascending by (distance, index), at
  // most max_nn entries each when max_nn > 0.  A radius that is not finite and > 0 prints an error and returns empty lists.
  NeighborLists radiusSearch(double radius, unsigned int max_nn = 0) const { return radiusSearch(*this, radius, max_nn); }
  NeighborLists radiusSearch(const ScanCloud &queries, double radius, unsigned int max_nn = 0) const
  {
    NeighborLists out;
    if (!(std::isfinite(radius) && radius > 0.0)) {
      std::fprintf(stderr, "[ScanCloud::radiusSearch] The radius (%f) must be finite and > 0.\n", radius);
      return out;
    }
    const size_t n = queries.points.size();
    out.offsets.assign(n + 1, 0);
    if (!n) return out;
    Device &d = Device::instance();
    SlotGuard t;
    d.upload(t.s, points);
    std::unique_ptr<SlotGuard> q;
    if (&queries != this) { q.reset(new SlotGuard()); d.upload(q->s, queries.points); }
    const int qs = q ? q->s : t.s;
    mvr_radius_params p;
    mvr_radius_default_params(&p);
    p.radius = radius; p.max_nn = max_nn;
    size_t total = 0;
    d.check(mvr_radius_search(d.ctx(), qs, t.s, &p, out.offsets.data(), nullptr, nullptr, 0, &total), "mvr_radius_search");
    out.indices.resize(total); out.sqr_distances.resize(total);
    if (total) d.check(mvr_radius_search(d.ctx(), qs, t.s, &p, out.offsets.data(), out.indices.data(), out.sqr_distances.data(), total, &total), "mvr_radius_search");
    return out;
  }

  // EXTENSION (pcl::MarchingCubesHoppe on the raw points, on the GPU; rules M1-M15: mvr_cloud_marching_cubes_hoppe in mvr_hip.h):
  // the triangle mesh of this cloud from the normals of `rich`, which must be oriented (a scan's are: estimateNormals flips
  // them towards the sensor).  voxel_size > 0 (an extension of the extension) replaces res by ceil(extent / voxel_size) + 1 per
  // axis, extent = the finite points' box widened by percentage_extend_grid.  Without one rich record per point, or with a
  // parameter outside rule M12 (a lattice of more than 2^27 vertices included), it prints an error, leaves `mesh` empty and
  // returns false.  `points`, `rich` and the pose stay as they are.
  struct MeshParams {
    int res[3] = {32, 32, 32};
    float iso_level = 0.f, percentage_extend_grid = 0.f, dist_ignore = -1.f;
    bool weld = true;              // one vertex per lattice edge (rule M13); false: PCL's triangle soup
    double voxel_size = 0.0;       // 0: res as given
  };
  bool reconstructMesh(const MeshParams &mp, PolygonMesh &mesh) const
  {
    mesh.cloud.clear();
    mesh.polygons.clear();
    const size_t n = points.size();
    if (rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::reconstructMesh] The cloud has no normals (%zu points, %zu records): call estimateNormals first.\n", n, rich.size());
      return false;
    }
    mvr_mc_params p;
    mvr_mc_default_params(&p);
    for (int k = 0; k < 3; ++k) p.res[k] = mp.res[k];
    p.iso_level = mp.iso_level; p.percentage_extend_grid = mp.percentage_extend_grid; p.dist_ignore = mp.dist_ignore; p.weld = mp.weld ? 1 : 0;
    if (mp.voxel_size != 0.0) {
      if (!(std::isfinite(mp.voxel_size) && mp.voxel_size > 0.0) || !(mp.percentage_extend_grid >= 0.f) || !std::isfinite(mp.percentage_extend_grid)) {
        std::fprintf(stderr, "[ScanCloud::reconstructMesh] The voxel size (%f) must be finite and > 0, the grid extension (%f) finite and >= 0.\n",
                     mp.voxel_size, (double)mp.percentage_extend_grid);
        return false;
      }
      double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
      for (const PCLPoint &q : points.points) {
        if (!(std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z))) continue;
        const double v[3] = {q.x, q.y, q.z};
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], v[k]); hi[k] = std::max(hi[k], v[k]); }
      }
      double cells = 1.0;
      for (int k = 0; k < 3; ++k) {
        const double extent = hi[k] >= lo[k] ? (hi[k] - lo[k]) * (1.0 + (double)mp.percentage_extend_grid) : 0.0;
        const double r = std::ceil(extent / mp.voxel_size) + 1.0;
        cells *= std::max(r, 2.0);
        p.res[k] = (int)std::min(std::max(r, 2.0), 2147483647.0);
      }
      if (cells > (double)MVR_MC_MAX_VERTICES) {
        std::fprintf(stderr, "[ScanCloud::reconstructMesh] A voxel size of %f gives a lattice of %.0f vertices, above the limit of %llu.\n", mp.voxel_size, cells,
                     (unsigned long long)MVR_MC_MAX_VERTICES);
        return false;
      }
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    if (n) uploadRichNormals(d, s.s);
    uint64_t nt = 0, nv = 0;
    size_t cap = std::max<size_t>(1024, 8 * ((size_t)std::max(p.res[0], 0) * std::max(p.res[1], 0) + (size_t)std::max(p.res[1], 0) * std::max(p.res[2], 0) +
                                             (size_t)std::max(p.res[0], 0) * std::max(p.res[2], 0)));
    std::vector<float> xyz;
    std::vector<uint32_t> idx;
    for (;;) {      // a first capacity from the lattice's faces; a surface that needs more says how much (rule M11)
      xyz.resize(cap * 9);
      if (p.weld) idx.resize(cap * 3);
      const int rc = mvr_cloud_marching_cubes_hoppe(d.ctx(), s.s, &p, nullptr, xyz.data(), cap, p.weld ? idx.data() : nullptr, &nt, &nv);
      if (rc == MVR_E_ARG && nt > cap) { cap = (size_t)nt; continue; }
      if (rc == MVR_E_ARG) { std::fprintf(stderr, "[ScanCloud::reconstructMesh] %s\n", mvr_last_error(d.ctx())); return false; }
      d.check(rc, "mvr_cloud_marching_cubes_hoppe");
      break;
    }
    mesh.cloud.resize((size_t)nv);
    for (size_t i = 0; i < (size_t)nv; ++i) mesh.cloud.points[i] = PCLPoint(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    mesh.polygons.resize((size_t)nt);
    for (size_t t = 0; t < (size_t)nt; ++t) {
      mesh.polygons[t].vertices.resize(3);
      for (uint32_t k = 0; k < 3; ++k) mesh.polygons[t].vertices[k] = p.weld ? idx[3 * t + k] : (uint32_t)(3 * t + k);
    }
    return true;
  }

  // EXTENSION (pcl::BoundaryEstimation on the raw points, on the GPU; rules: mvr_cloud_boundary in mvr_hip.h): one flag per point,
  // whether its neighbours within p.radius, projected onto its tangent plane, leave an angular gap above p.angle_threshold,
  // with the normals of `rich` (estimateNormals, smooth with compute_normals, or a file that carries them).  Without one rich
  // record per point, or with a parameter outside its range, it prints an error, leaves `boundary` empty and returns false.
  // `points`, `rich` and the pose stay as they are.
  bool detectBoundary(const mvr_boundary_params &p, std::vector<uint8_t> &boundary) const
  {
    boundary.clear();
    const size_t n = points.size();
    if (rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::detectBoundary] The cloud has no normals (%zu points, %zu records): call estimateNormals first.\n", n, rich.size());
      return false;
    }
    if (!(std::isfinite(p.radius) && p.radius > 0.0) || p.min_neighbors < 0 ||
        !(p.angle_threshold >= MVR_BOUNDARY_MIN_ANGLE && p.angle_threshold < 2.0 * 3.14159265358979323846)) {
      std::fprintf(stderr, "[ScanCloud::detectBoundary] The radius (%f) must be finite and > 0, the angle threshold (%f) in [pi / 4, 2 pi), min_neighbors (%d) >= 0.\n",
                   p.radius, p.angle_threshold, p.min_neighbors);
      return false;
    }
    boundary.resize(n);
    if (!n) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    uploadRichNormals(d, s.s);
    d.check(mvr_cloud_boundary(d.ctx(), s.s, &p, boundary.data(), nullptr, nullptr), "mvr_cloud_boundary");
    return true;
  }

  // EXTENSION (pcl::ISSKeypoint3D on the raw points, on the GPU; rules: mvr_cloud_iss_keypoints in mvr_hip.h): the indices,
  // ascending, of the points whose scatter over salient_radius passes both eigenvalue ratio tests and whose smallest eigenvalue
  // no neighbour within non_max_radius exceeds.  A parameter outside its range prints an error, leaves `indices` empty and
  // returns false.  `points`, `rich` and the pose stay as they are.
  bool detectKeypoints(const mvr_iss_params &p, std::vector<uint32_t> &indices) const
  {
    mvr_iss_border_params none = mvr_iss_border_params();
    return detectKeypoints(p, none, indices);
  }
  // the same with the border handling of the detector (rules K9-K11): with b.border_radius > 0 the points that have a boundary
  // point -- detectBoundary at that radius, b.angle_threshold and p.min_neighbors -- within it are dropped before the saliency
  // test; the normals are those of `rich`, and a cloud without them is refused as in detectBoundary.  A radius of 0: no border.
  bool detectKeypoints(const mvr_iss_params &p, const mvr_iss_border_params &b, std::vector<uint32_t> &indices) const
  {
    indices.clear();
    if (!(std::isfinite(p.salient_radius) && p.salient_radius > 0.0) || !(std::isfinite(p.non_max_radius) && p.non_max_radius > 0.0) ||
        !std::isfinite(p.gamma_21) || !std::isfinite(p.gamma_32) || p.min_neighbors < 0) {
      std::fprintf(stderr, "[ScanCloud::detectKeypoints] The radii (%f, %f) must be finite and > 0, the thresholds (%f, %f) finite, min_neighbors (%d) >= 0.\n",
                   p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors);
      return false;
    }
    const bool border = b.border_radius != 0.0;
    const size_t n = points.size();
    if (border && (!(std::isfinite(b.border_radius) && b.border_radius > 0.0) ||
                   !(b.angle_threshold >= MVR_BOUNDARY_MIN_ANGLE && b.angle_threshold < 2.0 * 3.14159265358979323846))) {
      std::fprintf(stderr, "[ScanCloud::detectKeypoints] The border radius (%f) must be 0 (no border) or finite and > 0, the angle threshold (%f) in [pi / 4, 2 pi).\n",
                   b.border_radius, b.angle_threshold);
      return false;
    }
    if (border && rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::detectKeypoints] A border radius needs normals (%zu points, %zu records): call estimateNormals first.\n", n, rich.size());
      return false;
    }
    if (!n) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    if (border) uploadRichNormals(d, s.s);
    indices.resize(n);
    size_t kept = 0;
    d.check(mvr_cloud_iss_keypoints_border(d.ctx(), -1, s.s, &p, border ? &b : nullptr, &kept, indices.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
            "mvr_cloud_iss_keypoints_border");
    indices.resize(kept);
    return true;
  }

  // EXTENSION (pcl::SampleConsensusPrerejective on the raw points, on the GPU; rules: mvr_align_prerejective in mvr_hip.h): the
  // coarse pose of THIS scan onto `target` for a pair without a turntable prior -- computeFPFH of both scans (both need their
  // normals in `rich`) at feature_radius, then the aligner.  On success `pose` is the scan's pose in the scene's own type:
  // setMatrix(pose * target.getMatrix()) puts the scan where registrationICPDevice can take over.  false (pose untouched): no
  // normals, a bad radius, or the aligner found no pose that reaches inlier_fraction; `result` (optional) says which.
  // With use_keypoints, detectKeypoints(keypoints) runs on both scans first and the descriptor rows of the other points are
  // NaN: such a row is never sampled (A1) and never matched (M3), so the matcher's work drops from n_source x n_target pairs to
  // keypoints x n_target while every pose is still scored over all points of the source.  alignPrerejectivePFH computes its
  // descriptors AT the keypoints only (computePFHAt, into tables of NaN): by rule Q5 the tables are bit for bit those of the full
  // computation with the other rows overwritten, at the cost of the keypoints' neighbourhoods (measured: 0.34 ms against 0.53 ms on
  // the 3k-point recovery pair, 10.2 ms against 138 ms per 200k view at 5 mm; profiles/feature_at_bench.json).  The FPFH overload
  // still computes every row and overwrites: FPFH at the keypoints needs the SPFH of nearly the whole surface and measured SLOWER
  // than the whole-cloud call up to 200k points (3.26 ms against 2.22 ms on that pair), so it was not switched.
  // With a border radius (border.border_radius > 0; off by default) the keypoints are those of the detector's border variant.
  struct PrerejectiveParams {
    double feature_radius = 0.0;
    mvr_prerej_params align;
    mvr_iss_params keypoints;            // salient_radius / non_max_radius must be set when use_keypoints is
    mvr_iss_border_params border;        // border_radius 0: no border handling (the default); angle_threshold pi / 2
    bool use_keypoints = false;
    PrerejectiveParams()
    {
      border = mvr_iss_border_params(); border.angle_threshold = 1.57079632679489661923;
      align = mvr_prerej_params(); align.max_iterations = 10; align.nr_samples = 3; align.k = 2; align.similarity = 0.9; align.inlier_fraction = 0.25;
      keypoints = mvr_iss_params(); keypoints.gamma_21 = keypoints.gamma_32 = 0.975; keypoints.min_neighbors = 5;
    }
  };
  bool alignPrerejective(const ScanCloud &target, const PrerejectiveParams &params, RowMatrixd &pose, mvr_prerej_result *result = nullptr) const
  {
    std::vector<FPFHSignature33> sf, tf;
    if (result) { *result = mvr_prerej_result(); result->best_iteration = -1; result->error = DBL_MAX; }
    if (!computeFPFH(params.feature_radius, sf) || !target.computeFPFH(params.feature_radius, tf)) return false;
    return alignPrerejective(target, params, sf, tf, pose, result);
  }
  // the same from PFH descriptors (computePFH of both scans at feature_radius): 125 floats per row through the same matcher
  // and aligner
  bool alignPrerejectivePFH(const ScanCloud &target, const PrerejectiveParams &params, RowMatrixd &pose, mvr_prerej_result *result = nullptr) const
  {
    std::vector<PFHSignature125> sf, tf;
    if (result) { *result = mvr_prerej_result(); result->best_iteration = -1; result->error = DBL_MAX; }
    if (params.use_keypoints) return alignAtKeypoints("computePFH", target, params, sf, tf, pose, result);
    if (!computePFH(params.feature_radius, sf) || !target.computePFH(params.feature_radius, tf)) return false;
    return alignPrerejective(target, params, sf, tf, pose, result);
  }
  // EXTENSION (pcl::SHOTEstimation on the raw points, on the GPU; rules L1-L7 and H1-H9: mvr_cloud_shot in mvr_hip.h): one SHOT352
  // per point -- 352 unit-norm floats and the local reference frame they were computed in -- with the normals of `rich`;
  // lrf_radius 0: the radius.  Refusals as computeFPFH.  computeSHOTAt: at the points `indices` of this cloud, or at every raw
  // point of this cloud over `surface` and its normals (rules Q1-Q8), bit for bit the rows computeSHOT gives those points.
  bool computeSHOT(double radius, std::vector<SHOT352> &out, double lrf_radius = 0.0) const
  {
    return shotAt("computeSHOT", radius, lrf_radius, nullptr, nullptr, out);
  }
  bool computeSHOTAt(double radius, const std::vector<uint32_t> &indices, std::vector<SHOT352> &out, double lrf_radius = 0.0) const
  {
    return shotAt("computeSHOTAt", radius, lrf_radius, nullptr, &indices, out);
  }
  bool computeSHOTAt(const ScanCloud &surface, double radius, std::vector<SHOT352> &out, double lrf_radius = 0.0) const
  {
    return surface.shotAt("computeSHOTAt", radius, lrf_radius, this, nullptr, out);
  }
  // the coarse alignment from SHOT descriptors (computeSHOT of both scans at feature_radius): 352 floats per row through the
  // same matcher and aligner; with use_keypoints the descriptors are computed AT the ISS keypoints only, as alignPrerejectivePFH
  // does it, into tables that are NaN elsewhere
  bool alignPrerejectiveSHOT(const ScanCloud &target, const PrerejectiveParams &params, RowMatrixd &pose, mvr_prerej_result *result = nullptr) const
  {
    if (result) { *result = mvr_prerej_result(); result->best_iteration = -1; result->error = DBL_MAX; }
    std::vector<float> st, tt;
    if (params.use_keypoints) {
      if (!featureInputsOk("computeSHOT", params.feature_radius) || !target.featureInputsOk("computeSHOT", params.feature_radius)) return false;
      std::vector<uint32_t> sk, tk;
      if (!detectKeypoints(params.keypoints, params.border, sk) || !target.detectKeypoints(params.keypoints, params.border, tk)) return false;
      if (!shotTable(params.feature_radius, &sk, st) || !target.shotTable(params.feature_radius, &tk, tt)) return false;
    } else if (!shotTable(params.feature_radius, nullptr, st) || !target.shotTable(params.feature_radius, nullptr, tt)) {
      return false;
    }
    Device &d = Device::instance();
    SlotGuard s, t;
    d.upload(s.s, points);
    d.upload(t.s, target.points);
    static const float none[MVR_SHOT_DIM] = {0};
    mvr_prerej_result res;
    d.check(mvr_align_prerejective_dim(d.ctx(), s.s, t.s, st.empty() ? none : st.data(), tt.empty() ? none : tt.data(), MVR_SHOT_DIM, &params.align, nullptr,
                                       &res, nullptr), "mvr_align_prerejective_dim");
    if (result) *result = res;
    if (!res.converged) return false;
    pose = PclMatrixCaster<RowMatrixd>(Matrix4f(res.T));
    return true;
  }
  // the SHOT rows of this cloud as the contiguous table the matcher takes, one row of 352 floats per point; with `key` only
  // those rows are computed and the others are NaN
  bool shotTable(double radius, const std::vector<uint32_t> *key, std::vector<float> &table) const
  {
    std::vector<SHOT352> rows;
    if (!shotAt("computeSHOT", radius, 0.0, nullptr, key, rows)) return false;
    table.assign(points.size() * (size_t)MVR_SHOT_DIM, key ? std::numeric_limits<float>::quiet_NaN() : 0.f);
    for (size_t r = 0; r < rows.size(); ++r)
      std::memcpy(table.data() + (size_t)(key ? (*key)[r] : r) * MVR_SHOT_DIM, rows[r].descriptor, sizeof(float) * MVR_SHOT_DIM);
    return true;
  }
  // the SHOT rows of the queries over THIS cloud and its normals: the points `indices` of this cloud, or every raw point of
  // `queries`, or (both null) every point of this cloud
  bool shotAt(const char *fn, double radius, double lrf_radius, const ScanCloud *queries, const std::vector<uint32_t> *indices, std::vector<SHOT352> &out) const
  {
    out.clear();
    if (!featureInputsOk(fn, radius)) return false;
    if (!(std::isfinite(lrf_radius) && lrf_radius >= 0.0)) {
      std::fprintf(stderr, "[ScanCloud::%s] The LRF radius (%f) must be finite and >= 0.\n", fn, lrf_radius);
      return false;
    }
    const size_t n = points.size(), nq = queries ? queries->points.size() : n;
    if (indices)
      for (uint32_t i : *indices)
        if (i >= nq) {
          std::fprintf(stderr, "[ScanCloud::%s] The index %u lies beyond the cloud (%zu points).\n", fn, i, nq);
          return false;
        }
    const size_t rows = indices ? indices->size() : nq;
    out.resize(rows);
    if (!rows) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    if (n) uploadRichNormals(d, s.s);
    std::shared_ptr<SlotGuard> q;
    if (queries && queries != this) { q = std::make_shared<SlotGuard>(); d.upload(q->s, queries->points); }
    mvr_shot_params p;
    p.radius = radius; p.lrf_radius = lrf_radius; p.fma_dist = 0;
    std::vector<float> table(rows * (size_t)MVR_SHOT_DIM), lrf(rows * 9);
    if (q || indices)
      d.check(mvr_cloud_shot_at(d.ctx(), q ? q->s : s.s, indices ? indices->data() : nullptr, rows, s.s, &p, nullptr, table.data(), lrf.data(), nullptr, nullptr),
              "mvr_cloud_shot_at");
    else
      d.check(mvr_cloud_shot(d.ctx(), s.s, &p, nullptr, table.data(), lrf.data(), nullptr, nullptr), "mvr_cloud_shot");
    for (size_t r = 0; r < rows; ++r) {
      std::memcpy(out[r].descriptor, table.data() + r * MVR_SHOT_DIM, sizeof(float) * MVR_SHOT_DIM);
      std::memcpy(out[r].rf, lrf.data() + r * 9, sizeof(float) * 9);
    }
    return true;
  }
  // the aligner on descriptor tables the caller holds, one row per point of this scan (sf) and of `target` (tf), 33 or 125
  // floats per row; with use_keypoints the rows of the other points are overwritten with NaN first
  template <typename FeatureT>
  bool alignPrerejective(const ScanCloud &target, const PrerejectiveParams &params, std::vector<FeatureT> &sf, std::vector<FeatureT> &tf,
                         RowMatrixd &pose, mvr_prerej_result *result = nullptr) const
  {
    static_assert(sizeof(FeatureT) == sizeof(float) * 3 * MVR_FPFH_BINS || sizeof(FeatureT) == sizeof(float) * MVR_PFH_DIM,
                  "a 33-float or a 125-float signature expected");
    if (result) { *result = mvr_prerej_result(); result->best_iteration = -1; result->error = DBL_MAX; }
    if (sf.size() != points.size() || tf.size() != target.points.size()) {
      std::fprintf(stderr, "[ScanCloud::alignPrerejective] One descriptor row per point expected (%zu rows for %zu points, %zu for %zu).\n",
                   sf.size(), points.size(), tf.size(), target.points.size());
      return false;
    }
    if (params.use_keypoints && (!keepKeypointRows(params.keypoints, params.border, sf) || !target.keepKeypointRows(params.keypoints, params.border, tf))) return false;
    Device &d = Device::instance();
    SlotGuard s, t;
    d.upload(s.s, points);
    d.upload(t.s, target.points);
    static const float none[MVR_PFH_DIM] = {0};
    mvr_prerej_result res;
    d.check(mvr_align_prerejective_dim(d.ctx(), s.s, t.s, sf.empty() ? none : sf[0].histogram, tf.empty() ? none : tf[0].histogram,
                                       (int)(sizeof(FeatureT) / sizeof(float)), &params.align, nullptr, &res, nullptr), "mvr_align_prerejective_dim");
    if (result) *result = res;
    if (!res.converged) return false;
    pose = PclMatrixCaster<RowMatrixd>(Matrix4f(res.T));
    return true;
  }
  // EXTENSION (pcl::GeneralizedIterativeClosestPoint on the raw points, on the GPU; rules G1-G10 at mvr_icp_align_gicp in
  // mvr_hip.h): the plane-to-plane refinement of this scan against `target`, both as their `points` lie.  A scan whose `rich`
  // holds one record per point uses those normals (estimateNormals, smooth with compute_normals, or a file that carries them);
  // otherwise the normals of its k_normals nearest neighbours are estimated in the slot.  On true, `pose` takes this scan's
  // points onto the target's (setMatrix(pose * getMatrix()) when both lie under their poses already).  false (pose
  // untouched): too few correspondences, or a singular system; `stats` (optional) says which.  Refused parameters throw.
  struct GICPParams {
    mvr_gicp_params gicp;
    int k_normals = 20;                  // setCorrespondenceRandomness
    GICPParams() { mvr_gicp_default_params(&gicp); }
  };
  bool alignGICP(const ScanCloud &target, const GICPParams &params, RowMatrixd &pose, mvr_icp_stats *stats = nullptr) const
  {
    Device &d = Device::instance();
    SlotGuard s, t;
    uploadWithNormals(d, s.s, params.k_normals);
    target.uploadWithNormals(d, t.s, params.k_normals);
    float T[16];
    mvr_icp_stats st = mvr_icp_stats();
    const int rc = mvr_icp_align_gicp(d.ctx(), s.s, t.s, -1, &params.gicp, nullptr, 0, T, &st, nullptr, 0);
    if (stats) *stats = st;
    if (rc == MVR_E_NOCORR || rc == MVR_E_SINGULAR) return false;
    d.check(rc, "mvr_icp_align_gicp");
    pose = PclMatrixCaster<RowMatrixd>(Matrix4f(T));
    return true;
  }
  // EXTENSION (pcl::NormalDistributionsTransform on the raw points, on the GPU; rules N1-N12 at mvr_ndt_align in mvr_hip.h): this
  // scan against the per-voxel Gaussians of `target`, both as their `points` lie; no correspondence search.  resolution (the
  // voxel edge) and step_size are in the clouds' unit.  The rotation parameters turn about the centre of the target's bounding
  // box, whatever params.ndt.origin says (N4: far from the origin the line search wanders otherwise).  On true, `pose` takes this
  // scan's points onto the target's, wherever the align stopped (`stats`, optional, says where and whether it calls that
  // converged); false (pose untouched): the source overlaps no cell.  Refused parameters throw.
  struct NDTParams {
    mvr_ndt_params ndt;
    NDTParams() { mvr_ndt_default_params(&ndt); }
  };
  bool alignNDT(const ScanCloud &target, double resolution, double step_size, RowMatrixd &pose, mvr_ndt_stats *stats = nullptr) const
  {
    NDTParams params;
    params.ndt.resolution = resolution; params.ndt.step_size = step_size;
    return alignNDT(target, params, pose, stats);
  }
  bool alignNDT(const ScanCloud &target, const NDTParams &params, RowMatrixd &pose, mvr_ndt_stats *stats = nullptr) const
  {
    mvr_ndt_params p = params.ndt;
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (size_t i = 0; i < target.points.size(); ++i) {
      const auto &q = target.points[i];
      const double v[3] = {(double)q.x, (double)q.y, (double)q.z};
      if (!(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))) continue;
      for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], v[a]); hi[a] = std::max(hi[a], v[a]); }
    }
    for (int a = 0; a < 3; ++a) p.origin[a] = lo[a] <= hi[a] ? 0.5 * (lo[a] + hi[a]) : 0.0;
    Device &d = Device::instance();
    SlotGuard s, t;
    d.upload(s.s, points);
    d.upload(t.s, target.points);
    float T[16];
    mvr_ndt_stats st = mvr_ndt_stats();
    const int rc = mvr_ndt_align(d.ctx(), s.s, t.s, -1, &p, nullptr, T, nullptr, &st, nullptr, 0);
    if (stats) *stats = st;
    if (rc == MVR_E_NOCORR) return false;
    d.check(rc, "mvr_ndt_align");
    pose = PclMatrixCaster<RowMatrixd>(Matrix4f(T));
    return true;
  }
  void uploadWithNormals(Device &d, int slot, int k_normals) const
  {
    const size_t n = points.size();
    d.upload(slot, points);
    if (!n) return;
    if (rich.size() == n) {
      std::vector<float> nrm(4 * n);
      for (size_t i = 0; i < n; ++i) { nrm[4 * i] = rich[i].normal_x; nrm[4 * i + 1] = rich[i].normal_y; nrm[4 * i + 2] = rich[i].normal_z; nrm[4 * i + 3] = 0.f; }
      d.check(mvr_cloud_upload_normals(d.ctx(), slot, nrm.data(), n, 16), "mvr_cloud_upload_normals");
    } else {
      mvr_normal_params np = mvr_normal_params();
      np.k = k_normals;
      d.check(mvr_cloud_estimate_normals(d.ctx(), 1, &slot, &np, nullptr), "mvr_cloud_estimate_normals");
    }
  }
  // what computeFPFH / computePFH (`fn`) refuse, with their texts: a cloud without normals, a radius that is not finite and > 0
  bool featureInputsOk(const char *fn, double radius) const
  {
    const size_t n = points.size();
    if (rich.size() != n) {
      std::fprintf(stderr, "[ScanCloud::%s] The cloud has no normals (%zu points, %zu records): call estimateNormals first.\n", fn, n, rich.size());
      return false;
    }
    if (!(std::isfinite(radius) && radius > 0.0)) {
      std::fprintf(stderr, "[ScanCloud::%s] The radius (%f) must be finite and > 0.\n", fn, radius);
      return false;
    }
    return true;
  }
  // the descriptors of the queries over THIS cloud and its normals: the points `indices` of this cloud, or every raw point of
  // `queries`; 33 or 125 floats per row
  template <typename FeatureT>
  bool featuresAt(const char *fn, double radius, const ScanCloud *queries, const std::vector<uint32_t> *indices, std::vector<FeatureT> &out) const
  {
    static_assert(sizeof(FeatureT) == sizeof(float) * 3 * MVR_FPFH_BINS || sizeof(FeatureT) == sizeof(float) * MVR_PFH_DIM,
                  "a 33-float or a 125-float signature expected");
    out.clear();
    if (!featureInputsOk(fn, radius)) return false;
    const size_t n = points.size(), nq = queries ? queries->points.size() : n;
    if (indices)
      for (uint32_t i : *indices)
        if (i >= nq) {
          std::fprintf(stderr, "[ScanCloud::%s] The index %u lies beyond the cloud (%zu points).\n", fn, i, nq);
          return false;
        }
    const size_t rows = indices ? indices->size() : nq;
    out.resize(rows);
    if (!rows) return true;
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, points);
    if (n) uploadRichNormals(d, s.s);
    std::shared_ptr<SlotGuard> q;
    if (queries && queries != this) { q = std::make_shared<SlotGuard>(); d.upload(q->s, queries->points); }
    const int qs = q ? q->s : s.s;
    const uint32_t *ip = indices ? indices->data() : nullptr;
    if (sizeof(FeatureT) == sizeof(float) * MVR_PFH_DIM) {
      mvr_pfh_params p;
      p.radius = radius; p.k = 0; p.fma_dist = 0;
      d.check(mvr_cloud_pfh_at(d.ctx(), qs, ip, rows, s.s, &p, out[0].histogram, nullptr, nullptr), "mvr_cloud_pfh_at");
    } else {
      mvr_fpfh_params p;
      p.radius = radius; p.fma_dist = 0;
      d.check(mvr_cloud_fpfh_at(d.ctx(), qs, ip, rows, s.s, &p, out[0].histogram, nullptr), "mvr_cloud_fpfh_at");
    }
    return true;
  }
  // a descriptor table of this cloud, NaN but for the rows of `key`, which are computed (the table keepKeypointRows leaves)
  template <typename FeatureT>
  bool keypointRows(const char *fn, double radius, const std::vector<uint32_t> &key, std::vector<FeatureT> &feat) const
  {
    std::vector<FeatureT> rows;
    if (!featuresAt(fn, radius, nullptr, &key, rows)) return false;
    FeatureT nan;
    for (float &v : nan.histogram) v = std::numeric_limits<float>::quiet_NaN();
    feat.assign(points.size(), nan);
    for (size_t r = 0; r < key.size(); ++r) feat[key[r]] = rows[r];
    return true;
  }
  // alignPrerejective with use_keypoints and descriptors of its own (`fn`: the call whose refusals come first, as when it ran)
  template <typename FeatureT>
  bool alignAtKeypoints(const char *fn, const ScanCloud &target, const PrerejectiveParams &params, std::vector<FeatureT> &sf, std::vector<FeatureT> &tf,
                        RowMatrixd &pose, mvr_prerej_result *result) const
  {
    if (!featureInputsOk(fn, params.feature_radius) || !target.featureInputsOk(fn, params.feature_radius)) return false;
    std::vector<uint32_t> sk, tk;
    if (!detectKeypoints(params.keypoints, params.border, sk) || !target.detectKeypoints(params.keypoints, params.border, tk)) return false;
    if (!keypointRows(fn, params.feature_radius, sk, sf) || !target.keypointRows(fn, params.feature_radius, tk, tf)) return false;
    PrerejectiveParams rest = params;
    rest.use_keypoints = false;                          // (the tables hold the keypoints' rows alone already)
    return alignPrerejective(target, rest, sf, tf, pose, result);
  }
  // the descriptor rows of the points detectKeypoints does not list become NaN (false: the detector refused its parameters)
  template <typename FeatureT>
  bool keepKeypointRows(const mvr_iss_params &p, std::vector<FeatureT> &feat) const
  {
    mvr_iss_border_params none = mvr_iss_border_params();
    return keepKeypointRows(p, none, feat);
  }
  template <typename FeatureT>
  bool keepKeypointRows(const mvr_iss_params &p, const mvr_iss_border_params &b, std::vector<FeatureT> &feat) const
  {
    std::vector<uint32_t> key;
    if (!detectKeypoints(p, b, key)) return false;
    std::vector<char> keep(feat.size(), 0);
    for (uint32_t i : key) keep[i] = 1;
    for (size_t i = 0; i < feat.size(); ++i)
      if (!keep[i])
        for (float &v : feat[i].histogram) v = std::numeric_limits<float>::quiet_NaN();
    return true;
  }

  // point_cloud.cpp:305-326 / :328-347 -- `transformation.txt`: the column-vector
  // 4x4 printed row by row (matrix(j,i), i outer), "%lf " per element, one row per
  // line.  6 decimals: poses round-trip to 1e-6 only.
  bool loadTransformation(const std::string &filename)
  {
    FILE *file = std::fopen(filename.c_str(), "r");
    if (file == NULL) return false;
    RowMatrixd matrix;
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i)
      for (int j = 0; j < 4 && ok; ++j) {
        double element;
        ok = std::fscanf(file, "%lf", &element) == 1;
        if (ok) matrix(j, i) = element;
      }
    std::fclose(file);
    if (ok) setMatrix(matrix);
    return ok;
  }
  bool saveTransformation(const std::string &filename) const
  {
    FILE *file = std::fopen(filename.c_str(), "w");
    if (file == NULL) return false;
    for (int i = 0; i < 4; ++i) {
      for (int j = 0; j < 4; ++j) std::fprintf(file, "%lf ", matrix_(j, i));
      std::fprintf(file, "\n");
    }
    std::fclose(file);
    return true;
  }

 private:
  // the normals of `rich` (one record per point) into a slot that holds `points`
  void uploadRichNormals(Device &d, int slot) const
  {
    const size_t n = points.size();
    std::vector<float> nrm(4 * n);
    for (size_t i = 0; i < n; ++i) { nrm[4 * i] = rich[i].normal_x; nrm[4 * i + 1] = rich[i].normal_y; nrm[4 * i + 2] = rich[i].normal_z; nrm[4 * i + 3] = 0.f; }
    d.check(mvr_cloud_upload_normals(d.ctx(), slot, nrm.data(), n, 16), "mvr_cloud_upload_normals");
  }

  // PlaneParams -> mvr_sac_params, checked as the C-ABI checks them (P12)
  static bool planeParams(const PlaneParams &pp, bool negative, mvr_sac_params &p)
  {
    p.model = pp.perpendicular ? 1 : 0; p.threshold = pp.threshold; p.max_iterations = pp.max_iterations; p.probability = pp.probability;
    p.optimize = pp.optimize ? 1 : 0; p.eps_angle = pp.eps_angle; p.seed = pp.seed; p.negative = negative ? 1 : 0; p.fma_dist = 0;
    for (int k = 0; k < 3; ++k) p.axis[k] = pp.axis[k];
    const double *a = p.axis;
    const bool axis_ok = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && (a[0] != 0.0 || a[1] != 0.0 || a[2] != 0.0);
    if (!(std::isfinite(p.threshold) && p.threshold > 0.0) || p.max_iterations < 1 || p.max_iterations > (1 << 24) ||
        !(p.probability > 0.0 && p.probability < 1.0) || (p.model == 1 && (!axis_ok || !(p.eps_angle > 0.0 && p.eps_angle <= 1.57079632679489661923)))) {
      std::fprintf(stderr, "[ScanCloud::segmentPlane] The threshold (%f) must be finite and > 0, the iterations (%d) in 1..2^24, the probability (%f) in (0, 1); the perpendicular model needs an axis and an angle (%f) in (0, pi / 2].\n",
                   p.threshold, p.max_iterations, p.probability, p.eps_angle);
      return false;
    }
    return true;
  }

  // ClusterParams -> mvr_cluster_params, checked as the C-ABI checks them (E8); normals need one rich record per point
  bool clusterParams(const ClusterParams &cp, uint32_t keep, mvr_cluster_params &p) const
  {
    p.tolerance = cp.tolerance; p.min_size = cp.min_size; p.max_size = cp.max_size; p.use_normals = cp.eps_angle > 0.0 ? 1 : 0;
    p.eps_angle = cp.eps_angle; p.negative = 0; p.keep = keep; p.fma_dist = 0;
    if (!(std::isfinite(p.tolerance) && p.tolerance > 0.0) || keep == 0 || !(cp.eps_angle >= 0.0 && cp.eps_angle <= 3.14159265358979323846) ||
        (p.use_normals && rich.size() != points.size())) {
      std::fprintf(stderr, "[ScanCloud::extractClusters] The tolerance (%f) must be finite and > 0, keep (%u) >= 1, the angle (%f) 0 (no normals) or in (0, pi] with one rich record per point.\n",
                   p.tolerance, keep, cp.eps_angle);
      return false;
    }
    if (points.size() == 0) p.use_normals = 0;      // (an empty slot has no normals to offer)
    return true;
  }
  void uploadForClusters(Device &d, int slot, const mvr_cluster_params &p) const
  {
    d.upload(slot, points);
    if (p.use_normals) uploadRichNormals(d, slot);
  }

  // one of the two filters (the other pointer null) in place on `points`; `rich` follows through kept_index
  size_t removeOutliers(const mvr_sor_params *sor, const mvr_ror_params *ror)
  {
    Device &d = Device::instance();
    SlotGuard s;
    const size_t before = points.size();
    d.upload(s.s, points);
    size_t kept = 0;
    std::vector<uint32_t> index(before ? before : 1);
    if (sor) d.check(mvr_cloud_statistical_outlier_removal(d.ctx(), s.s, s.s, sor, &kept, index.data(), nullptr, nullptr), "mvr_cloud_statistical_outlier_removal");
    else d.check(mvr_cloud_radius_outlier_removal(d.ctx(), s.s, s.s, ror, &kept, index.data(), nullptr), "mvr_cloud_radius_outlier_removal");
    d.download(s.s, points);
    if (rich.size() == before) {                   // colours and normals follow their points
      io::RichCloud r(kept);
      for (size_t k = 0; k < kept; ++k) r[k] = rich[index[k]];
      rich.swap(r);
    }
    touch();
    return before - kept;
  }

  RowMatrixd matrix_;
  std::string filename_;
  unsigned long long revision_ = 0;
};

// stand-in for FileSystemModel::getPointCloud(object, view): views 0..V-1
struct TurntableModel {
  std::vector<ScanCloud> views;
  ScanCloud &getPointCloud(int /*object*/, int view) { return views.at((size_t)view); }
  int numViews() const { return (int)views.size(); }
};

struct AlignLog { int view; Matrix4f T; int n_corr; double mse; int iterations; double fitness; bool has_fitness; };

// The registration driver of this library: DEVICE-RESIDENT.  The scans of one object are uploaded once and stay in
// device slots for the whole session; a registration pass moves poses (V x 16 doubles) and per-pair sums
// (V x 32 doubles) across the bus, never points.  It covers the non-GUI duties of the reference's class Registrator
// (mvr/include/registrator.h:40-59) -- which pairs are registered in which order with which parameters, and how the
// result is composed into the views' poses -- without its PCL-shaped data flow (a host cloud rebuilt, re-uploaded and
// re-indexed at every align).  (tests/cxx/call_surface.hpp drives the PCL-named shim members in the reference's order of calls.)
class Registrator {
 public:
  explicit Registrator(TurntableModel *model) : model_(model) {}
  virtual ~Registrator() {}

  // pivot / axis are osg::Vec3 (float) in the reference (registrator.h)
  void setPivotPoint(double x, double y, double z) { pivot_[0] = (float)x; pivot_[1] = (float)y; pivot_[2] = (float)z; }
  void setAxisNormal(double x, double y, double z) { axis_[0] = (float)x; axis_[1] = (float)y; axis_[2] = (float)z; }
  const float *getPivotPoint() const { return pivot_; }
  const float *getAxisNormal() const { return axis_; }

  // registrator.cpp:258-274 / :294-308 -- `axis.txt`: pivot "x y z" then axis "nx ny nz", "%f"
  bool load(const std::string &filename)
  {
    FILE *file = std::fopen(filename.c_str(), "r");
    if (file == NULL) return false;
    double x, y, z, nx, ny, nz;
    const bool ok = std::fscanf(file, "%lf %lf %lf", &x, &y, &z) == 3 && std::fscanf(file, "%lf %lf %lf", &nx, &ny, &nz) == 3;
    std::fclose(file);
    if (ok) { setPivotPoint(x, y, z); setAxisNormal(nx, ny, nz); }
    return ok;
  }
  bool save(const std::string &filename) const
  {
    FILE *file = std::fopen(filename.c_str(), "w");
    if (file == NULL) return false;
    std::fprintf(file, "%f %f %f\n", pivot_[0], pivot_[1], pivot_[2]);
    std::fprintf(file, "%f %f %f\n", axis_[0], axis_[1], axis_[2]);
    std::fclose(file);
    return true;
  }

  // registrator.cpp:331-342
  RowMatrixd getRotationMatrix(double angle) const
  {
    RowMatrixd matrix = RowMatrixd::identity();
    matrix = matrix * RowMatrixd::translate(-pivot_[0], -pivot_[1], -pivot_[2]);
    matrix = matrix * RowMatrixd::rotate(angle, axis_[0], axis_[1], axis_[2]);
    matrix = matrix * RowMatrixd::translate(pivot_[0], pivot_[1], pivot_[2]);
    return matrix;
  }

  // point_cloud.cpp:409 generalised from 12 views / 30 degrees
  double viewAngle(int view) const { return mvr_turntable_angle(view, model_->numViews()); }

  // ---- sequential registration against the growing model (what registrationICP computes, registrator.cpp:517-588):
  // views in the order 1, V-1, 2, V-2, ..., V/2 (shown ones only), each aligned to the merged cloud of view 0 and all
  // views before it, `repeat_times` sweeps.  Device form: the target grows IN PLACE in a reserved slot
  // (mvr_cloud_append), a view is posed from its resident raw scan (mvr_cloud_transform), aligned (mvr_icp_align: one
  // 4x4 comes back) and appended; the fitness score of the last view of a sweep is taken as the reference does.
  void registrationICPDevice(int max_iterations, double max_distance, int object, int repeat_times = 1)
  {
    const int V = model_->numViews();
    if (V < 2) return;
    Device &d = Device::instance();
    ensureResident(object);
    std::vector<int> order;
    for (int i = 1; i < V / 2; ++i) for (int v : {i, V - i}) if (model_->getPointCloud(object, v).isShown()) order.push_back(v);
    if (model_->getPointCloud(object, V / 2).isShown() && (order.empty() || order.back() != V / 2) && V / 2 >= 1) order.push_back(V / 2);
    if (order.empty()) return;
    size_t total = model_->getPointCloud(object, 0).size();
    for (int v : order) { model_->getPointCloud(object, v).initRotation(*this); total += model_->getPointCloud(object, v).size(); }
    mvr_icp_params p = mvr_icp_params();
    p.use_reciprocal = 1; p.max_corr_dist = max_distance; p.max_iterations = max_iterations;
    p.transformation_epsilon = 0.000001; p.euclidean_fitness_eps = 64;       // registrator.cpp:558-560
    SlotGuard target, source, moved;
    for (int sweep = 0; sweep < repeat_times; ++sweep) {
      d.check(mvr_cloud_transform(d.ctx(), target.s, raw_[0], model_->getPointCloud(object, 0).getMatrix().asColumnMajorColumnVector()), "mvr_cloud_transform");
      d.check(mvr_cloud_reserve(d.ctx(), target.s, total), "mvr_cloud_reserve");
      for (size_t k = 0; k < order.size(); ++k) {
        ScanCloud &pc = model_->getPointCloud(object, order[k]);
        d.check(mvr_cloud_transform(d.ctx(), source.s, raw_[(size_t)order[k]], pc.getMatrix().asColumnMajorColumnVector()), "mvr_cloud_transform");
        float T[16];
        mvr_icp_stats st = mvr_icp_stats();
        const int rc = mvr_icp_align(d.ctx(), source.s, target.s, moved.s, &p, T, &st);
        if (rc != MVR_OK && rc != MVR_E_NOCORR) d.check(rc, "mvr_icp_align");
        AlignLog entry{pc.getView(), Matrix4f(T), st.n_corr, st.mse, st.iterations, 0.0, false};
        if (k + 1 == order.size()) {
          d.check(mvr_fitness(d.ctx(), source.s, target.s, T, DBL_MAX, 0, &entry.fitness), "mvr_fitness");
          entry.has_fitness = true;
        }
        log.push_back(entry);
        pc.setMatrix(pc.getMatrix() * RowMatrixd(PclMatrixCaster<RowMatrixd>(entry.T)));      // pose <- T_icp o pose
        d.check(mvr_cloud_append(d.ctx(), target.s, moved.s), "mvr_cloud_append");
      }
    }
  }

  // ---- incremental registration (what automaticRegistration computes, registrator.cpp:746-842 with
  // automaticRegistrationICP :877-990 and refineTransformation :1008-1030; intent per SURVEY App. C.1 -- the original
  // indexes its view list out of bounds from the second view on and re-registers the earlier views cumulatively):
  // the views are added one at a time; a new view gets its turntable prior, is posed from its resident raw scan, then
  // advanced IN PLACE by `repeat_times` aligns against everything merged so far (the reference's `icp_.align(*source_)`
  // whose output aliases its input, :920 / :1012 / :1024: every repeat continues from the last, pose <- T_j o pose), and
  // is appended to the model where it stands.  The transformation epsilon is never set in this mode (it stays PCL's 0,
  // App. C.3); the fitness epsilon is the caller's (the dialog's default is 50).  Per repeat one 4x4 crosses the bus.
  // The logged fitness is the TRUE residual of the advanced source against the model (mvr_fitness with the identity),
  // not the reference's double-transformed number (App. C.2).
  void automaticRegistrationDevice(int object, int max_iterations, int repeat_times, double max_distance, double euclidean_fitness_epsilon,
                                   bool log_fitness = false)
  {
    const int V = model_->numViews();
    if (V < 2) return;
    Device &d = Device::instance();
    ensureResident(object);
    size_t total = 0;
    for (int v = 0; v < V; ++v) total += model_->getPointCloud(object, v).size();
    mvr_icp_params p = mvr_icp_params();
    p.use_reciprocal = 1; p.max_corr_dist = max_distance; p.max_iterations = max_iterations;
    p.transformation_epsilon = 0.0; p.euclidean_fitness_eps = euclidean_fitness_epsilon;          // registrator.cpp:901-904
    SlotGuard model, moving;
    d.check(mvr_cloud_transform(d.ctx(), model.s, raw_[0], model_->getPointCloud(object, 0).getMatrix().asColumnMajorColumnVector()), "mvr_cloud_transform");
    d.check(mvr_cloud_reserve(d.ctx(), model.s, total), "mvr_cloud_reserve");
    const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int v = 1; v < V; ++v) {
      ScanCloud &pc = model_->getPointCloud(object, v);
      pc.initRotation(*this);
      pc.setRegisterState(true);
      d.check(mvr_cloud_transform(d.ctx(), moving.s, raw_[(size_t)v], pc.getMatrix().asColumnMajorColumnVector()), "mvr_cloud_transform");
      for (int j = 0; j < repeat_times; ++j) {
        float T[16];
        mvr_icp_stats st = mvr_icp_stats();
        const int rc = mvr_icp_align(d.ctx(), moving.s, model.s, moving.s, &p, T, &st);            // out == in: the source advances in place
        if (rc != MVR_OK && rc != MVR_E_NOCORR) d.check(rc, "mvr_icp_align");
        AlignLog entry{pc.getView(), Matrix4f(T), st.n_corr, st.mse, st.iterations, 0.0, false};
        if (log_fitness) {
          d.check(mvr_fitness(d.ctx(), moving.s, model.s, identity, DBL_MAX, 0, &entry.fitness), "mvr_fitness");
          entry.has_fitness = true;
        }
        log.push_back(entry);
        pc.setMatrix(pc.getMatrix() * RowMatrixd(PclMatrixCaster<RowMatrixd>(entry.T)));
      }
      d.check(mvr_cloud_append(d.ctx(), model.s, moving.s), "mvr_cloud_append");
    }
  }

  // ---- global registration over the ring of views (what registrationLUM computes, registrator.cpp:611-664):
  // max(1, max_iterations / 16) outer passes; a pass = pose all views, reciprocal correspondences + sums of every ring
  // pair (i -> i+1), Lu-Milios relaxation (16 iterations) on the host from those sums, pose_v <- LUM_v o pose_v.
  // One native call (mvr_ring_run) runs ALL the passes.
  void registrationLUMDevice(int max_iterations, double max_distance, int object)
  {
    const int V = model_->numViews();
    if (V < 2) return;
    Device &d = Device::instance();
    ensureResident(object);
    std::vector<int> es((size_t)V), et((size_t)V);
    std::vector<double> poses((size_t)V * 16), rows((size_t)V * 32), pair_n((size_t)V), pair_mse((size_t)V), lum_pose((size_t)V * 6);
    for (int v = 0; v < V; ++v) {
      ScanCloud &pc = model_->getPointCloud(object, v);
      pc.initRotation(*this);
      pc.setRegisterState(true);
      std::memcpy(&poses[(size_t)v * 16], pc.getMatrix().asColumnMajorColumnVector(), 16 * sizeof(double));
      es[(size_t)v] = v; et[(size_t)v] = (v + 1) % V;
    }
    const int lum_iterations = 16, passes = std::max(1, max_iterations / lum_iterations);     // registrator.cpp:623-624
    int iters = 0;
    d.check(mvr_ring_run(d.ctx(), passes, V, posed_.data(), raw_.data(), V, es.data(), et.data(), max_distance, 1, 0, origin_,
                         lum_iterations, poses.data(), lum_pose.data(), nullptr, pair_n.data(), pair_mse.data(), &iters, rows.data(),
                         nullptr), "mvr_ring_run");
    lum_ncorr.clear();
    for (int e = 0; e < V; ++e) lum_ncorr.push_back((int)pair_n[(size_t)e]);
    for (int v = 0; v < V; ++v) {
      RowMatrixd m;
      std::memcpy(&m(0, 0), &poses[(size_t)v * 16], 16 * sizeof(double));
      model_->getPointCloud(object, v).setMatrix(m);
    }
  }

  // ---- residuals over the ring (what computeError gathers, registrator.cpp:466-515): neighbouring shown views
  // (i, i+1) plus (0, V-1); per pair the number of reciprocal correspondences within the threshold and the sum of
  // their squared distances.  All views are posed by one launch, all pairs searched by one launch per stage; only
  // 32 doubles per pair reach the host.
  struct PairResidual { int source, target; size_t n; double sum_d2; };
  std::vector<PairResidual> computeErrorDevice(int object, double distance_threshold)
  {
    const int V = model_->numViews();
    std::vector<PairResidual> out;
    if (V < 2) return out;
    Device &d = Device::instance();
    ensureResident(object);
    std::vector<char> shown((size_t)V, 0);
    std::vector<int> dst, src;
    std::vector<double> T;
    for (int v = 0; v < V; ++v) {
      ScanCloud &pc = model_->getPointCloud(object, v);
      shown[(size_t)v] = v == 0 || pc.isShown();
      if (!shown[(size_t)v]) continue;
      if (v) pc.initRotation(*this);
      dst.push_back(posed_[(size_t)v]); src.push_back(raw_[(size_t)v]);
      T.insert(T.end(), pc.getMatrix().asColumnMajorColumnVector(), pc.getMatrix().asColumnMajorColumnVector() + 16);
    }
    d.check(mvr_cloud_transform_batch(d.ctx(), (int)dst.size(), dst.data(), src.data(), T.data()), "mvr_cloud_transform_batch");
    std::vector<int> ps, pt;
    for (int i = 0; i + 1 < V; ++i) if (shown[(size_t)i] && shown[(size_t)i + 1]) { out.push_back(PairResidual{i, i + 1, 0, 0.0}); }
    if (V > 2 && shown[0] && shown[(size_t)V - 1]) out.push_back(PairResidual{0, V - 1, 0, 0.0});
    for (const PairResidual &r : out) { ps.push_back(posed_[(size_t)r.source]); pt.push_back(posed_[(size_t)r.target]); }
    if (out.empty()) return out;
    std::vector<mvr_pair_moments2_t> m2(out.size());
    d.check(mvr_pair_moments2_batch(d.ctx(), (int)out.size(), ps.data(), pt.data(), distance_threshold, 1, 0, nullptr, nullptr, origin_,
                                    m2.data(), nullptr), "mvr_pair_moments2_batch");
    for (size_t k = 0; k < out.size(); ++k) { out[k].n = (size_t)m2[k].n; out[k].sum_d2 = m2[k].sum_d2; }
    return out;
  }

  // ---- turntable axis and pivot from the registered views' poses (registrator.cpp:402-455): mvr_refine_axis.
  // Returns false (nothing changed) when no view but view 0 is registered or the poses do not determine an axis.
  bool refineAxis(int object)
  {
    const int V = model_->numViews();
    std::vector<double> poses;
    for (int v = 1; v < V; ++v) {
      const ScanCloud &pc = model_->getPointCloud(object, v);
      if (!pc.isRegistered()) continue;
      poses.insert(poses.end(), pc.getMatrix().asColumnMajorColumnVector(), pc.getMatrix().asColumnMajorColumnVector() + 16);
    }
    if (poses.empty()) return false;
    float axis[3], pivot[3];
    if (mvr_refine_axis((int)(poses.size() / 16), poses.data(), pivot_[1], axis, pivot) != MVR_OK) return false;
    for (int k = 0; k < 3; ++k) { axis_[k] = axis[k]; pivot_[k] = pivot[k]; }
    return true;
  }

  // EXTENSION, off by default: every saveRegisteredPoints (and saveRegisteredMesh) below first takes the platter out of the merged cloud -- the plane
  // perpendicular to the turntable axis (getAxisNormal, refined or not) within eps_angle, found by ScanCloud::removePlane with
  // SACMODEL_PERPENDICULAR_PLANE at this distance threshold.  threshold 0 switches it off again.  A merged cloud without such
  // a plane is written as it is.
  void setPlatterRemoval(double threshold, double eps_angle = 0.1, int max_iterations = 1000, uint64_t seed = 0)
  {
    platter_.threshold = threshold; platter_.eps_angle = eps_angle; platter_.max_iterations = max_iterations; platter_.seed = seed;
    platter_.perpendicular = true;
    platter_on_ = threshold != 0.0;
  }
  bool getPlatterRemoval() const { return platter_on_; }
  size_t lastPlatterPoints() const { return platter_removed_; }      // what the last saveRegisteredPoints / saveRegisteredMesh took out

  // EXTENSION, off by default: every saveRegisteredPoints (and saveRegisteredMesh) below keeps only the `keep` largest Euclidean clusters of the merged
  // cloud (ScanCloud::keepLargestClusters: points within `tolerance` of each other, clusters of at least min_size points) --
  // the object without the clamp, the pot rim and the speckle that stood beside it -- right after the platter removal step and
  // before any smoothing or downsampling.  tolerance 0 switches it off again.  A merged cloud without a cluster of min_size
  // points is written empty.
  void setObjectIsolation(double tolerance, uint32_t min_size, uint32_t keep = 1)
  {
    isolation_.tolerance = tolerance; isolation_.min_size = min_size; isolation_keep_ = keep;
    isolation_on_ = tolerance != 0.0;
  }
  bool getObjectIsolation() const { return isolation_on_; }
  size_t lastIsolationDropped() const { return isolation_dropped_; }      // what the last saveRegisteredPoints / saveRegisteredMesh took out

  // ---- the merged object (registrator.cpp:344-400, the step registration() ends with, :719-744): every registered
  // view's points (and normals) moved by its pose -- the normals by the FULL affine including the translation, as
  // the reference does -- concatenated in view order and written as <folder>/points.pcd
  // (binary_compressed) and <folder>/points.asc.  Views that only hold XYZ points contribute zero colour / normals.
  // Returns the number of points written, 0 on failure.
  size_t saveRegisteredPoints(int object, const std::string &folder, io::RichCloud *merged_out = nullptr)
  {
    io::RichCloud merged;
    mergeRegisteredPoints(object, merged);
    isolation_dropped_ = 0;
    if (platter_on_ || isolation_on_) {
      ScanCloud whole;
      whole.rich.swap(merged);
      for (const io::RichPoint &q : whole.rich) whole.points.push_back(PCLPoint(q.x, q.y, q.z));
      removePlatter(whole);
      isolateObject(whole);
      merged.swap(whole.rich);
    }
    const bool ok = io::savePCDFile(folder + "/points.pcd", merged, io::PCD_BINARY_COMPRESSED) && io::savePointsASC(folder + "/points.asc", merged);
    const size_t n = merged.size();
    if (merged_out) merged_out->swap(merged);
    return ok ? n : 0;
  }

  // EXTENSION: the same merged cloud put through ScanCloud::voxelDownsample(leaf_size) before it is written to the same two
  // files -- twelve overlapping turntable views hold mostly duplicated surface.  Its normals are the reference's
  // full-affine-moved normals and are averaged as they are (the voxel's sum, normalised).  merged_out receives the
  // downsampled cloud.  Returns the number of points written, 0 on failure.
  size_t saveRegisteredPoints(int object, const std::string &folder, float leaf_size, io::RichCloud *merged_out = nullptr)
  {
    ScanCloud merged;
    mergeRegisteredPoints(object, merged.rich);
    for (const io::RichPoint &q : merged.rich) merged.points.push_back(PCLPoint(q.x, q.y, q.z));
    removePlatter(merged);
    isolateObject(merged);
    merged.voxelDownsample(leaf_size);
    const bool ok = io::savePCDFile(folder + "/points.pcd", merged.rich, io::PCD_BINARY_COMPRESSED) &&
                    io::savePointsASC(folder + "/points.asc", merged.rich);
    const size_t n = merged.rich.size();
    if (merged_out) merged_out->swap(merged.rich);
    return ok ? n : 0;
  }

  // EXTENSION: the merged cloud smoothed by ScanCloud::smooth(mls_radius, polynomial_order) -- the layers of overlapping views
  // carry their own sensor noise and what registration error is left; a surface fitted through the stack removes the "double
  // walls" -- and then, with leaf_size > 0, put through ScanCloud::voxelDownsample(leaf_size), before it is written to the same
  // two files.  Only the coordinates are smoothed: colours, the full-affine-moved normals and curvature follow their points.
  // merged_out receives the cloud as written.  Returns the number of points written, 0 on failure; parameters outside their
  // range are a failure: an error is printed and nothing is written.
  size_t saveRegisteredPoints(int object, const std::string &folder, double mls_radius, int polynomial_order, float leaf_size /* 0: none */,
                              io::RichCloud *merged_out = nullptr)
  {
    if (!(std::isfinite(mls_radius) && mls_radius > 0.0) || polynomial_order < 0 || polynomial_order > 2 || !(leaf_size >= 0.f) || !std::isfinite(leaf_size)) {
      std::fprintf(stderr, "[Registrator::saveRegisteredPoints] The radius (%f) must be finite and > 0, the order (%d) in 0..2, the leaf size (%f) finite and >= 0.\n",
                   mls_radius, polynomial_order, leaf_size);
      return 0;
    }
    ScanCloud merged;
    mergeRegisteredPoints(object, merged.rich);
    for (const io::RichPoint &q : merged.rich) merged.points.push_back(PCLPoint(q.x, q.y, q.z));
    removePlatter(merged);
    isolateObject(merged);
    merged.smooth(mls_radius, polynomial_order, false);
    if (leaf_size > 0.f) merged.voxelDownsample(leaf_size);
    const bool ok = io::savePCDFile(folder + "/points.pcd", merged.rich, io::PCD_BINARY_COMPRESSED) &&
                    io::savePointsASC(folder + "/points.asc", merged.rich);
    const size_t n = merged.rich.size();
    if (merged_out) merged_out->swap(merged.rich);
    return ok ? n : 0;
  }

  // EXTENSION: the surface of the merged object -- the merged cloud of saveRegisteredPoints, after the same platter removal and
  // isolation steps when they are on, put through ScanCloud::reconstructMesh with its merged (full-affine-moved) normals and
  // written as <folder>/mesh.ply beside points.pcd (io::savePLYFile: ASCII, vertex + face elements).  mesh_out receives the
  // mesh as written.  Returns the number of triangles written.  NOTE: the merged normals are moved by the FULL affine, as the
  // reference moves them (mergeRegisteredPoints): a pose with a translation adds it to the normal and so turns it, and the signed
  // distances of rule M5 are then wrong near that view's points -- the mesh is meaningful for views whose poses are pure rotations
  // (or whose normals are estimated again on the merged cloud).  A merge without normals -- a registered view that holds XYZ
  // points only, or no registered view at all -- writes nothing and returns 0, and so does a refusal of reconstructMesh.
  size_t saveRegisteredMesh(int object, const std::string &folder, const ScanCloud::MeshParams &params, PolygonMesh *mesh_out = nullptr)
  {
    bool normals = false;
    for (int v = 0; v < model_->numViews(); ++v) {
      const ScanCloud &pc = model_->getPointCloud(object, v);
      if (!pc.isRegistered()) continue;
      if (pc.rich.size() != pc.size()) { normals = false; break; }
      normals = normals || pc.size() > 0;
    }
    if (!normals) return 0;
    ScanCloud merged;
    mergeRegisteredPoints(object, merged.rich);
    for (const io::RichPoint &q : merged.rich) merged.points.push_back(PCLPoint(q.x, q.y, q.z));
    removePlatter(merged);
    isolateObject(merged);
    PolygonMesh mesh;
    if (!merged.reconstructMesh(params, mesh)) return 0;
    if (!io::savePLYFile(folder + "/mesh.ply", mesh)) return 0;
    const size_t n = mesh.polygons.size();
    if (mesh_out) { mesh_out->cloud = mesh.cloud; mesh_out->polygons.swap(mesh.polygons); }
    return n;
  }

  // ---- Registrator::registration (registrator.cpp:719-744): denoise every view, give it its prior, mark it
  // registered, save the merged cloud, refine the axis.
  size_t registration(int object, int segment_threshold, double triangle_length, const std::string &folder)
  {
    for (int v = 0; v < model_->numViews(); ++v) {
      ScanCloud &pc = model_->getPointCloud(object, v);
      pc.denoise(segment_threshold, triangle_length);
      pc.initRotation(*this);
      pc.setRegisterState(true);
    }
    const size_t n = saveRegisteredPoints(object, folder);
    refineAxis(object);
    return n;
  }

  // the scans of the model changed on the host (loaded, denoised, edited): upload them again at the next use
  void invalidate() { resident_object_ = -1; }

  std::vector<AlignLog> log;       // one entry per align (what the reference prints / writes to fitness_scores.txt)
  std::vector<int> lum_ncorr;      // correspondences per ring edge of the last global pass

 private:
  // the merged object of saveRegisteredPoints (registrator.cpp:344-400)
  void mergeRegisteredPoints(int object, io::RichCloud &merged)
  {
    const int V = model_->numViews();
    for (int v = 0; v < V; ++v) {
      const ScanCloud &pc = model_->getPointCloud(object, v);
      if (!pc.isRegistered()) continue;
      const RowMatrixd &M = pc.getMatrix();
      auto pre = [&M](float x, float y, float z, float out[3]) {              // osg::Matrixd::preMult(Vec3f): (x, y, z, 1) * M / w
        const double w = 1.0 / (M(0, 3) * x + M(1, 3) * y + M(2, 3) * z + M(3, 3));
        for (int k = 0; k < 3; ++k) out[k] = (float)((M(0, k) * x + M(1, k) * y + M(2, k) * z + M(3, k)) * w);
      };
      for (size_t j = 0; j < pc.size(); ++j) {
        io::RichPoint q = j < pc.rich.size() ? pc.rich[j] : io::RichPoint();
        const PCLPoint &p = pc.points.points[j];
        float o[3];
        pre(p.x, p.y, p.z, o); q.x = o[0]; q.y = o[1]; q.z = o[2];
        pre(q.normal_x, q.normal_y, q.normal_z, o); q.normal_x = o[0]; q.normal_y = o[1]; q.normal_z = o[2];
        merged.push_back(q);
      }
    }
  }

  // setPlatterRemoval's step on a merged cloud (points and rich records, one per point)
  void removePlatter(ScanCloud &merged)
  {
    platter_removed_ = 0;
    if (!platter_on_) return;
    for (int k = 0; k < 3; ++k) platter_.axis[k] = axis_[k];
    platter_removed_ = merged.removePlane(platter_);
  }

  // setObjectIsolation's step on a merged cloud (points and rich records, one per point)
  void isolateObject(ScanCloud &merged)
  {
    isolation_dropped_ = 0;
    if (!isolation_on_) return;
    isolation_dropped_ = merged.keepLargestClusters(isolation_, isolation_keep_);
  }

  // raw scans -> device slots (once per object and per revision of its clouds); posed copies get slots of their own
  void ensureResident(int object)
  {
    const int V = model_->numViews();
    unsigned long long rev = 0;
    for (int v = 0; v < V; ++v) rev += model_->getPointCloud(object, v).revision() + (unsigned long long)model_->getPointCloud(object, v).size() * 1000003ull;
    if (resident_object_ == object && resident_rev_ == rev && (int)raw_.size() == V) return;
    Device &d = Device::instance();
    raw_guard_.clear(); posed_guard_.clear(); raw_.clear(); posed_.clear();
    for (int v = 0; v < V; ++v) {
      raw_guard_.emplace_back(new SlotGuard); posed_guard_.emplace_back(new SlotGuard);
      raw_.push_back(raw_guard_.back()->s); posed_.push_back(posed_guard_.back()->s);
      d.upload(raw_.back(), model_->getPointCloud(object, v).points);
    }
    origin_[0] = origin_[1] = origin_[2] = 0.0;           // moments are taken about a point of the data: small magnitudes
    if (V && !model_->getPointCloud(object, 0).points.empty()) {
      const PCLPoint &p = model_->getPointCloud(object, 0).points.points[0];
      origin_[0] = p.x; origin_[1] = p.y; origin_[2] = p.z;
    }
    resident_object_ = object; resident_rev_ = rev;
  }

  TurntableModel *model_;
  float pivot_[3] = {0, 0, 0};
  float axis_[3] = {0, 0, 1};
  ScanCloud::PlaneParams platter_;      // setPlatterRemoval
  bool platter_on_ = false;
  size_t platter_removed_ = 0;
  ScanCloud::ClusterParams isolation_;  // setObjectIsolation
  uint32_t isolation_keep_ = 1;
  bool isolation_on_ = false;
  size_t isolation_dropped_ = 0;
  int resident_object_ = -1;
  unsigned long long resident_rev_ = 0;
  std::vector<std::unique_ptr<SlotGuard> > raw_guard_, posed_guard_;
  std::vector<int> raw_, posed_;
  double origin_[3] = {0, 0, 0};
};

// point_cloud.cpp:400-413
inline void ScanCloud::initRotation(const Registrator &r)
{
  if (!getMatrix().isIdentity()) return;
  if (view == 0) return;
  setMatrix(r.getRotationMatrix(r.viewAngle(view)));
}

}  // namespace mvr
