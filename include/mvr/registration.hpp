// include/mvr/registration.hpp -- drop-in C++ shim over the C-ABI (mvr_hip.h).
//
// Source-compatible stand-ins for the three PCL classes the reference's
// Registrator drives:
//   pcl::IterativeClosestPoint<PointXYZ,PointXYZ>          mvr/include/registrator.h:91,
//       call sites mvr/src/registrator.cpp:551-576, 768-777, 901-923, 1012-1015, 1024-1025
//   pcl::registration::CorrespondenceEstimation<P,P,float> registrator.cpp:496-502, 644-649
//   pcl::registration::LUM<PointXYZ>                       registrator.cpp:627-658
// Same method names, argument meaning and error behaviour (align never throws
// for bad data: it reports through hasConverged(), as PCL does; HIP/runtime
// failures DO throw mvr::Error -- there is no CPU fallback to hide them).
// All arithmetic runs in libmvr_hip.so on the GPU (+ the tiny host solves).
// Like the reference, drive one object from one thread at a time.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../mvr_hip.h"
#include "types.hpp"

namespace mvr {

// One GPU context per thread, shared by the shim objects of that thread.
class Device {
 public:
  static Device &instance()
  {
    static thread_local Device d;
    return d;
  }
  mvr_ctx *ctx()
  {
    if (!ctx_) check(mvr_ctx_create(&ctx_, device_id()), "mvr_ctx_create (no usable GPU: there is no CPU fallback)");
    return ctx_;
  }
  static int &device_id() { static int id = 0; return id; }
  int acquire()
  {
    for (int s = 0; s < MVR_MAX_SLOTS; ++s) if (!used_[s]) { used_[s] = true; return s; }
    throw Error(MVR_E_NOMEM, "mvr: out of device cloud slots");
  }
  void release(int s) { if (s >= 0 && s < MVR_MAX_SLOTS) { used_[s] = false; if (ctx_) mvr_cloud_clear(ctx_, s); } }
  void check(int rc, const char *what)
  {
    if (rc != MVR_OK) throw Error(rc, std::string(what) + ": " + mvr_strerror(rc) + " (" + (ctx_ ? mvr_last_error(ctx_) : "") + ")");
  }
  template <typename PointT>
  void upload(int slot, const PointCloud<PointT> &c)
  {
    static_assert(sizeof(PointT) == 16, "16-byte XYZ points expected");
    check(mvr_cloud_upload(ctx(), slot, c.empty() ? nullptr : c.points[0].data, c.size(), sizeof(PointT)), "mvr_cloud_upload");
  }
  template <typename PointT>
  void download(int slot, PointCloud<PointT> &c)
  {
    size_t n = 0;
    check(mvr_cloud_size(ctx(), slot, &n), "mvr_cloud_size");
    c.resize(n);
    if (n) check(mvr_cloud_download(ctx(), slot, c.points[0].data, n, sizeof(PointT), &n), "mvr_cloud_download");
  }
  ~Device() { if (ctx_) mvr_ctx_destroy(ctx_); }

 private:
  Device() {}
  mvr_ctx *ctx_ = nullptr;
  bool used_[MVR_MAX_SLOTS] = {false};
};

struct SlotGuard {
  int s;
  SlotGuard() : s(Device::instance().acquire()) {}
  ~SlotGuard() { Device::instance().release(s); }
  SlotGuard(const SlotGuard &) = delete;
  SlotGuard &operator=(const SlotGuard &) = delete;
};

// ---- clouds whose points carry normals (PointNormal): the points go up as 16-byte x, y, z, 1 and the normals beside them
namespace detail {
template <typename P> auto has_normal_test(int) -> decltype((void)std::declval<P>().normal_x, std::true_type());
template <typename P> std::false_type has_normal_test(...);
template <typename P> struct has_normal : decltype(has_normal_test<P>(0)) {};

template <typename PointT>
void upload_cloud(Device &d, int slot, const PointCloud<PointT> &c, std::false_type) { d.upload(slot, c); }
template <typename PointT>
void upload_cloud(Device &d, int slot, const PointCloud<PointT> &c, std::true_type)
{
  const size_t n = c.size();
  std::vector<float> xyz(4 * n), nrm(4 * n);
  for (size_t i = 0; i < n; ++i) {
    const PointT &q = c.points[i];
    xyz[4 * i] = q.x; xyz[4 * i + 1] = q.y; xyz[4 * i + 2] = q.z; xyz[4 * i + 3] = 1.f;
    nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
  }
  d.check(mvr_cloud_upload(d.ctx(), slot, n ? xyz.data() : nullptr, n, 16), "mvr_cloud_upload");
  d.check(mvr_cloud_upload_normals(d.ctx(), slot, n ? nrm.data() : nullptr, n, 16), "mvr_cloud_upload_normals");
}
template <typename PointT>
void upload_cloud(Device &d, int slot, const PointCloud<PointT> &c) { upload_cloud(d, slot, c, has_normal<PointT>()); }

template <typename PointT>
void download_cloud(Device &d, int slot, PointCloud<PointT> &c, std::false_type) { d.download(slot, c); }
// (the cloud keeps whatever else its points hold: the caller sized it from the input)
template <typename PointT>
void download_cloud(Device &d, int slot, PointCloud<PointT> &c, std::true_type)
{
  size_t n = 0, got = 0;
  d.check(mvr_cloud_size(d.ctx(), slot, &n), "mvr_cloud_size");
  c.resize(n);
  if (!n) return;
  std::vector<float> xyz(4 * n), nrm(4 * n, 0.f);
  d.check(mvr_cloud_download(d.ctx(), slot, xyz.data(), n, 16, &got), "mvr_cloud_download");
  d.check(mvr_cloud_download_normals(d.ctx(), slot, nrm.data(), n, 16, &got), "mvr_cloud_download_normals");
  for (size_t i = 0; i < n; ++i) {
    PointT &q = c.points[i];
    q.x = xyz[4 * i]; q.y = xyz[4 * i + 1]; q.z = xyz[4 * i + 2];
    if (got == n) { q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2]; }
  }
}
template <typename PointT>
void download_cloud(Device &d, int slot, PointCloud<PointT> &c) { download_cloud(d, slot, c, has_normal<PointT>()); }
}  // namespace detail

// ---------------------------------------------------------------- correspondence rejectors
// pcl::registration::CorrespondenceRejector and the five rejectors of mvr_hip.h (rules R1-R10 at
// mvr_correspondences_rejected).  A rejector is a parameter record: added to an IterativeClosestPoint
// (addCorrespondenceRejector) it becomes a stage of the chain that mvr_icp_align_rejected runs on the GPU between the search
// and the estimator of every iteration; on its own, with setInputCorrespondences, getCorrespondences runs
// mvr_reject_correspondences on the list.  Survivors come in ascending query index.
namespace registration {

class CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejector> Ptr;
  typedef std::shared_ptr<const CorrespondenceRejector> ConstPtr;
  virtual ~CorrespondenceRejector() {}
  virtual void setInputCorrespondences(const CorrespondencesConstPtr &c) { input_correspondences_ = c; }
  CorrespondencesConstPtr getInputCorrespondences() { return input_correspondences_; }
  void getCorrespondences(Correspondences &out)
  {
    out.clear();
    if (!input_correspondences_ || input_correspondences_->empty()) return;
    getRemainingCorrespondences(*input_correspondences_, out);
  }
  virtual void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining)
  {
    Device &d = Device::instance();
    const size_t n = original.size();
    std::vector<int32_t> q(n), m(n), qo(n), mo(n);
    std::vector<float> dd(n), dout(n);
    size_t ns = 0, nt = 0, kept = 0;
    for (size_t k = 0; k < n; ++k) {
      q[k] = original[k].index_query; m[k] = original[k].index_match; dd[k] = original[k].distance;
      if (q[k] >= 0) ns = std::max(ns, (size_t)q[k] + 1);
      if (m[k] >= 0) nt = std::max(nt, (size_t)m[k] + 1);
    }
    SlotGuard s, t;
    prepareSlots(d, s.s, t.s, ns, nt);
    const mvr_rejector r = stage();
    mvr_rejector_stage st = mvr_rejector_stage();
    remaining.clear();
    const int rc = mvr_reject_correspondences(d.ctx(), s.s, t.s, q.data(), m.data(), dd.data(), n, &r, 1, qo.data(), mo.data(), dout.data(), n, &kept, &st);
    if (rc == MVR_E_ARG) {
      std::fprintf(stderr, "[pcl::registration::%s::getRemainingCorrespondences] %s\n", getClassName().c_str(), mvr_last_error(d.ctx()));
      return;
    }
    d.check(rc, "mvr_reject_correspondences");
    remaining.resize(kept);
    for (size_t k = 0; k < kept; ++k) remaining[k] = Correspondence(qo[k], mo[k], dout[k]);
    noteStage(st);
  }
  const std::string &getClassName() const { return rejection_name_; }
  // ours: the stage of the C-ABI chain this rejector stands for, and what the last run of that stage reported
  virtual mvr_rejector stage() const = 0;
  virtual void noteStage(const mvr_rejector_stage &) {}

 protected:
  // the list's slots: only their sizes matter (R8), so two clouds of zeros large enough for the indices
  virtual void prepareSlots(Device &d, int s, int t, size_t ns, size_t nt)
  {
    std::vector<float> z(4 * std::max(ns, nt), 0.f);
    d.check(mvr_cloud_upload(d.ctx(), s, ns ? z.data() : nullptr, ns, 16), "mvr_cloud_upload");
    d.check(mvr_cloud_upload(d.ctx(), t, nt ? z.data() : nullptr, nt, 16), "mvr_cloud_upload");
  }
  std::string rejection_name_;
  CorrespondencesConstPtr input_correspondences_;
};
typedef CorrespondenceRejector::Ptr CorrespondenceRejectorPtr;

class CorrespondenceRejectorDistance : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorDistance> Ptr;
  CorrespondenceRejectorDistance() { rejection_name_ = "CorrespondenceRejectorDistance"; }
  void setMaximumDistance(float distance) { max_distance_ = distance; }      // (PCL keeps the square; getMaximumDistance returns the root)
  float getMaximumDistance() const { return max_distance_; }
  mvr_rejector stage() const override { return mvr_rejector{MVR_REJ_DISTANCE, (double)max_distance_, 0u}; }

 private:
  float max_distance_ = FLT_MAX;
};

class CorrespondenceRejectorMedianDistance : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorMedianDistance> Ptr;
  CorrespondenceRejectorMedianDistance() { rejection_name_ = "CorrespondenceRejectorMedianDistance"; }
  void setMedianFactor(double factor) { factor_ = factor; }
  double getMedianFactor() const { return factor_; }
  // the median the last run cut at (of the squared distances the correspondences carry, R3's upper median)
  double getMedianDistance() const { return median_distance_; }
  mvr_rejector stage() const override { return mvr_rejector{MVR_REJ_MEDIAN, factor_, 0u}; }
  void noteStage(const mvr_rejector_stage &st) override { median_distance_ = (double)st.threshold; }

 private:
  double factor_ = 1.0, median_distance_ = 0.0;
};

class CorrespondenceRejectorTrimmed : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorTrimmed> Ptr;
  CorrespondenceRejectorTrimmed() { rejection_name_ = "CorrespondenceRejectorTrimmed"; }
  void setOverlapRatio(float ratio) { overlap_ratio_ = std::min(1.0f, std::max(0.0f, ratio)); }
  float getOverlapRatio() const { return overlap_ratio_; }
  void setMinCorrespondences(unsigned int n) { nr_min_correspondences_ = n; }
  unsigned int getMinCorrespondences() const { return nr_min_correspondences_; }
  mvr_rejector stage() const override { return mvr_rejector{MVR_REJ_TRIMMED, (double)overlap_ratio_, (uint32_t)nr_min_correspondences_}; }

 private:
  float overlap_ratio_ = 0.5f;
  unsigned int nr_min_correspondences_ = 0;
};

class CorrespondenceRejectorOneToOne : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorOneToOne> Ptr;
  CorrespondenceRejectorOneToOne() { rejection_name_ = "CorrespondenceRejectorOneToOne"; }
  mvr_rejector stage() const override { return mvr_rejector{MVR_REJ_ONE_TO_ONE, 0.0, 0u}; }
};

// setThreshold takes a cosine, as in PCL.  In an IterativeClosestPoint the normals are those of the clouds the ICP holds
// (PointNormal clouds: align uploads them); the data container calls are accepted, and used when the rejector runs on its own.
class CorrespondenceRejectorSurfaceNormal : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorSurfaceNormal> Ptr;
  CorrespondenceRejectorSurfaceNormal() { rejection_name_ = "CorrespondenceRejectorSurfaceNormal"; }
  void setThreshold(double threshold) { threshold_ = threshold; }
  double getThreshold() const { return threshold_; }
  template <typename PointT, typename NormalT> void initializeDataContainer() {}
  template <typename PointT> void setInputSource(const typename PointCloud<PointT>::ConstPtr &c) { take(src_xyz_, *c); }
  template <typename PointT> void setInputTarget(const typename PointCloud<PointT>::ConstPtr &c) { take(tgt_xyz_, *c); }
  template <typename PointT, typename NormalT> void setInputNormals(const typename PointCloud<NormalT>::ConstPtr &c) { takeNormals(src_nrm_, *c); }
  template <typename PointT, typename NormalT> void setTargetNormals(const typename PointCloud<NormalT>::ConstPtr &c) { takeNormals(tgt_nrm_, *c); }
  mvr_rejector stage() const override { return mvr_rejector{MVR_REJ_SURFACE_NORMAL, threshold_, 0u}; }

 protected:
  void prepareSlots(Device &d, int s, int t, size_t ns, size_t nt) override
  {
    one(d, s, src_xyz_, src_nrm_, ns);
    one(d, t, tgt_xyz_, tgt_nrm_, nt);
  }

 private:
  template <typename C> static void take(std::vector<float> &out, const C &c)
  {
    out.resize(4 * c.size());
    for (size_t i = 0; i < c.size(); ++i) { out[4 * i] = c.points[i].x; out[4 * i + 1] = c.points[i].y; out[4 * i + 2] = c.points[i].z; out[4 * i + 3] = 1.f; }
  }
  template <typename C> static void takeNormals(std::vector<float> &out, const C &c)
  {
    out.resize(4 * c.size());
    for (size_t i = 0; i < c.size(); ++i) { out[4 * i] = c.points[i].normal_x; out[4 * i + 1] = c.points[i].normal_y; out[4 * i + 2] = c.points[i].normal_z; out[4 * i + 3] = 0.f; }
  }
  // the normals decide; points are only there to size the slot (zeros when the caller gave none)
  static void one(Device &d, int slot, const std::vector<float> &xyz, const std::vector<float> &nrm, size_t need)
  {
    const size_t n = std::max(need, nrm.size() / 4);
    std::vector<float> p(4 * n, 0.f);
    if (xyz.size() == 4 * n) p = xyz;
    d.check(mvr_cloud_upload(d.ctx(), slot, n ? p.data() : nullptr, n, 16), "mvr_cloud_upload");
    if (nrm.size() == 4 * n && n) d.check(mvr_cloud_upload_normals(d.ctx(), slot, nrm.data(), n, 16), "mvr_cloud_upload_normals");
  }
  double threshold_ = 1.0;
  std::vector<float> src_xyz_, tgt_xyz_, src_nrm_, tgt_nrm_;
};

// pcl::registration::CorrespondenceRejectorSampleConsensus (rules C1-C12 at mvr_reject_sample_consensus in mvr_hip.h): keeps
// the correspondences that agree with one rigid motion.  On its own list it uploads its clouds and runs the dedicated entry;
// added to an IterativeClosestPoint or a GeneralizedIterativeClosestPoint it is a stage of the chain, which takes the points
// from the clouds the registration holds (the current source of every iteration), and after align getBestTransformation() is
// what mvr_ctx_last_sample_consensus returns.  setSeed is ours: PCL draws with rand().
template <typename PointT>
class CorrespondenceRejectorSampleConsensus : public CorrespondenceRejector {
 public:
  typedef std::shared_ptr<CorrespondenceRejectorSampleConsensus<PointT>> Ptr;
  typedef std::shared_ptr<const CorrespondenceRejectorSampleConsensus<PointT>> ConstPtr;
  typedef typename PointCloud<PointT>::Ptr PointCloudPtr;
  typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  CorrespondenceRejectorSampleConsensus() { rejection_name_ = "CorrespondenceRejectorSampleConsensus"; }

  virtual void setInputSource(const PointCloudConstPtr &cloud) { input_ = cloud; }
  virtual void setInputTarget(const PointCloudConstPtr &cloud) { target_ = cloud; }
  virtual void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; }       // (the older names)
  virtual void setTargetCloud(const PointCloudConstPtr &cloud) { target_ = cloud; }
  PointCloudConstPtr const getInputSource() { return input_; }
  PointCloudConstPtr const getInputTarget() { return target_; }
  void setInlierThreshold(double threshold) { inlier_threshold_ = threshold; }
  double getInlierThreshold() { return inlier_threshold_; }
  void setMaximumIterations(int max_iterations) { max_iterations_ = std::max(max_iterations, 0); }
  int getMaximumIterations() { return max_iterations_; }
  void setRefineModel(const bool refine) { refine_ = refine; }
  bool getRefineModel() const { return refine_; }
  void setSaveInliers(bool s) { save_inliers_ = s; }
  bool getSaveInliers() { return save_inliers_; }
  // positions, in the list the rejector last ran on by itself, of the correspondences it kept (with setSaveInliers)
  void getInliersIndices(std::vector<int> &indices) { indices = inlier_indices_; }
  Mat4<float> getBestTransformation() { return best_transformation_; }
  bool requiresSourcePoints() const { return true; }
  bool requiresTargetPoints() const { return true; }
  void setSeed(uint64_t seed) { seed_ = seed; }
  uint64_t getSeed() const { return seed_; }
  // ours: the whole record of the last run (mvr_rej_sac_result)
  const mvr_rej_sac_result &getResult() const { return result_; }

  mvr_rejector stage() const override
  {
    mvr_rejector r = mvr_rejector{MVR_REJ_SAMPLE_CONSENSUS, inlier_threshold_, 0u};
    r.max_iterations = (uint32_t)max_iterations_; r.refine = refine_ ? 1 : 0; r.seed = seed_;
    return r;
  }
  // (the registration calls this after align: the stage's record says nothing about the motion, the context does)
  void noteStage(const mvr_rejector_stage &) override
  {
    mvr_rej_sac_result res;
    if (mvr_ctx_last_sample_consensus(Device::instance().ctx(), &res) == MVR_OK) take(res);
  }

  void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) override
  {
    remaining.clear();
    inlier_indices_.clear();
    if (!input_ || !target_) {
      std::fprintf(stderr, "[pcl::registration::%s::getRemainingCorrespondences] No input cloud dataset was given!\n", getClassName().c_str());
      return;
    }
    Device &d = Device::instance();
    const size_t n = original.size();
    std::vector<int32_t> q(n), m(n), qo(n), mo(n);
    std::vector<float> dd(n), dout(n);
    for (size_t k = 0; k < n; ++k) { q[k] = original[k].index_query; m[k] = original[k].index_match; dd[k] = original[k].distance; }
    SlotGuard s, t;
    d.upload(s.s, *input_);
    d.upload(t.s, *target_);
    const mvr_rejector r = stage();
    mvr_rej_sac_result res;
    size_t kept = 0;
    const int rc = mvr_reject_sample_consensus(d.ctx(), s.s, t.s, q.data(), m.data(), dd.data(), n, &r, &res, qo.data(), mo.data(), dout.data(), n,
                                               &kept, nullptr, 0);
    if (rc == MVR_E_ARG) {
      std::fprintf(stderr, "[pcl::registration::%s::getRemainingCorrespondences] %s\n", getClassName().c_str(), mvr_last_error(d.ctx()));
      return;
    }
    d.check(rc, "mvr_reject_sample_consensus");
    take(res);
    remaining.resize(kept);
    for (size_t k = 0; k < kept; ++k) remaining[k] = Correspondence(qo[k], mo[k], dout[k]);
    if (save_inliers_) {
      std::vector<int32_t> sorted(qo.begin(), qo.begin() + (std::ptrdiff_t)kept);      // (ascending already: R7)
      for (size_t k = 0; k < n; ++k)
        if (std::binary_search(sorted.begin(), sorted.end(), q[k])) inlier_indices_.push_back((int)k);
    }
  }

 private:
  void take(const mvr_rej_sac_result &res)
  {
    result_ = res;
    for (int k = 0; k < 16; ++k) best_transformation_.m[k] = res.T[k];
  }
  double inlier_threshold_ = 0.05;
  int max_iterations_ = 1000;
  bool refine_ = false, save_inliers_ = false;
  uint64_t seed_ = 0;
  PointCloudConstPtr input_, target_;
  Mat4<float> best_transformation_ = Mat4<float>::Identity();
  mvr_rej_sac_result result_ = mvr_rej_sac_result();
  std::vector<int> inlier_indices_;
};

}  // namespace registration

// ---------------------------------------------------------------- ICP
template <typename PointSource, typename PointTarget, typename Scalar = float>
class IterativeClosestPoint {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef typename PointCloudSource::Ptr PointCloudSourcePtr;
  typedef typename PointCloudTarget::Ptr PointCloudTargetPtr;
  typedef Mat4<Scalar> Matrix4;

  IterativeClosestPoint()
  {
    // PCL defaults
    p_ = mvr_icp_params();     // zero every field, incl. the point_to_plane extension switch
    p_.use_reciprocal = 0; p_.max_corr_dist = std::sqrt(DBL_MAX); p_.max_iterations = 10;
    p_.transformation_epsilon = 0.0; p_.euclidean_fitness_eps = -DBL_MAX; p_.fma_dist = 0;
  }

  void setUseReciprocalCorrespondences(bool b) { p_.use_reciprocal = b ? 1 : 0; }
  bool getUseReciprocalCorrespondences() const { return p_.use_reciprocal != 0; }
  void setMaxCorrespondenceDistance(double d) { p_.max_corr_dist = d; }
  double getMaxCorrespondenceDistance() const { return p_.max_corr_dist; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  int getMaximumIterations() const { return p_.max_iterations; }
  void setTransformationEpsilon(double e) { p_.transformation_epsilon = e; }
  double getTransformationEpsilon() const { return p_.transformation_epsilon; }
  void setEuclideanFitnessEpsilon(double e) { p_.euclidean_fitness_eps = e; }
  double getEuclideanFitnessEpsilon() const { return p_.euclidean_fitness_eps; }
  void setInputSource(const PointCloudSourcePtr &c) { input_ = c; }
  void setInputTarget(const PointCloudTargetPtr &c) { target_ = c; }
  PointCloudSourcePtr const getInputSource() const { return input_; }
  PointCloudTargetPtr const getInputTarget() const { return target_; }

  // the rejector chain (rules R1-R10 in mvr_hip.h): with at least one rejector align runs mvr_icp_align_rejected, the chain in
  // the order of the calls; at most MVR_MAX_REJECTORS of them
  typedef registration::CorrespondenceRejector::Ptr CorrespondenceRejectorPtr;
  void addCorrespondenceRejector(const CorrespondenceRejectorPtr &rejector) { rejectors_.push_back(rejector); }
  std::vector<CorrespondenceRejectorPtr> getCorrespondenceRejectors() { return rejectors_; }
  bool removeCorrespondenceRejector(unsigned int i)
  {
    if (i >= rejectors_.size()) return false;
    rejectors_.erase(rejectors_.begin() + i);
    return true;
  }
  void clearCorrespondenceRejectors() { rejectors_.clear(); }

  // align(output): `output` may be the very cloud handed to setInputSource
  // (registrator.cpp:920 `icp_.align(*source_)`): the input is uploaded first.
  void align(PointCloudSource &output)
  {
    Device &d = Device::instance();
    converged_ = false; final_ = Matrix4::Identity(); stats_ = mvr_icp_stats();
    if (!input_ || !target_) { state_ = MVR_CONV_NO_CORRESPONDENCES; return; }
    // the caller may have mutated either cloud since the last call (:576)
    detail::upload_cloud(d, src_.s, *input_);
    detail::upload_cloud(d, tgt_.s, *target_);
    float T[16];
    int rc;
    if (rejectors_.empty()) rc = mvr_icp_align(d.ctx(), src_.s, tgt_.s, out_.s, &p_, T, &stats_);
    else {
      if (rejectors_.size() > (size_t)MVR_MAX_REJECTORS) throw Error(MVR_E_ARG, "mvr: more than MVR_MAX_REJECTORS correspondence rejectors");
      std::vector<mvr_rejector> chain;
      for (const CorrespondenceRejectorPtr &r : rejectors_) chain.push_back(r->stage());
      std::vector<mvr_icp_iter_trace> trace((size_t)std::max(1, p_.max_iterations));
      rc = mvr_icp_align_rejected(d.ctx(), src_.s, tgt_.s, out_.s, &p_, chain.data(), (int)chain.size(), T, &stats_, trace.data(), (int)trace.size());
      if (rc == MVR_OK || rc == MVR_E_NOCORR) {      // every rejector learns what its stage did in the last iteration
        const size_t last = std::min(trace.size() - 1, (size_t)std::max(0, stats_.iterations - (rc == MVR_OK ? 1 : 0)));
        for (size_t k = 0; k < rejectors_.size(); ++k) rejectors_[k]->noteStage(trace[last].stages[k]);
      }
    }
    if (rc != MVR_OK && rc != MVR_E_NOCORR) d.check(rc, "mvr_icp_align");
    if (rc == MVR_E_NOCORR)
      std::fprintf(stderr, "[mvr::IterativeClosestPoint::computeTransformation] Not enough correspondences found. "
                           "Relax your threshold parameters.\n");
    for (int k = 0; k < 16; ++k) final_.m[k] = (Scalar)T[k];
    converged_ = stats_.converged != 0;
    state_ = stats_.state;
    if (detail::has_normal<PointSource>::value && &output != input_.get()) output = *input_;      // (the fields beside x, y, z and the normal)
    detail::download_cloud(d, out_.s, output);
    aligned_once_ = true;
  }

  Matrix4 getFinalTransformation() const { return final_; }
  bool hasConverged() const { return converged_; }
  int getConvergenceState() const { return state_; }
  const mvr_icp_stats &getStats() const { return stats_; }

  // Registration::getFitnessScore(max_range): uses the input cloud and the
  // target as they were at the last align (the registration's own tree),
  // i.e. the clouds still resident in this object's device slots.
  double getFitnessScore(double max_range = DBL_MAX)
  {
    Device &d = Device::instance();
    if (!aligned_once_) { if (!input_ || !target_) return DBL_MAX; detail::upload_cloud(d, src_.s, *input_); detail::upload_cloud(d, tgt_.s, *target_); }
    else if (input_) detail::upload_cloud(d, src_.s, *input_);       // PCL transforms *input_ as it is NOW (App. C.2)
    float T[16];
    for (int k = 0; k < 16; ++k) T[k] = (float)final_.m[k];
    double score = DBL_MAX;
    d.check(mvr_fitness(d.ctx(), src_.s, tgt_.s, T, max_range, p_.fma_dist, &score), "mvr_fitness");
    return score;
  }

 private:
  mvr_icp_params p_;
  mvr_icp_stats stats_ = mvr_icp_stats();
  PointCloudSourcePtr input_;
  PointCloudTargetPtr target_;
  Matrix4 final_;
  bool converged_ = false, aligned_once_ = false;
  int state_ = MVR_CONV_NOT;
  std::vector<CorrespondenceRejectorPtr> rejectors_;
  SlotGuard src_, tgt_, out_;
};

// ---------------------------------------------------------------- Generalized ICP
// pcl::GeneralizedIterativeClosestPoint over mvr_icp_align_gicp (rules G1-G10 in mvr_hip.h).  The side covariances come from
// normals: a cloud without them (PointXYZ) gets the normals of its k nearest neighbours from mvr_cloud_estimate_normals with
// k = the correspondence randomness (PCL's k-neighbourhood covariance, regularised, is I - (1 - eps) n n^T of exactly that
// normal).  DEVIATION: a cloud that carries normals (PointNormal) uses them as they are; PCL recomputes the covariances from
// the neighbours in every case.  DEVIATION: the inner optimiser is Levenberg-Marquardt on the device, not BFGS (G7).
// setSourceCovariances / setTargetCovariances are not offered.
template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef typename PointCloudSource::Ptr PointCloudSourcePtr;
  typedef typename PointCloudTarget::Ptr PointCloudTargetPtr;
  typedef Mat4<float> Matrix4;
  typedef registration::CorrespondenceRejector::Ptr CorrespondenceRejectorPtr;

  GeneralizedIterativeClosestPoint() { mvr_gicp_default_params(&p_); }      // PCL's defaults

  void setInputSource(const PointCloudSourcePtr &c) { input_ = c; }
  void setInputTarget(const PointCloudTargetPtr &c) { target_ = c; }
  PointCloudSourcePtr const getInputSource() const { return input_; }
  PointCloudTargetPtr const getInputTarget() const { return target_; }
  void setMaxCorrespondenceDistance(double d) { p_.max_corr_dist = d; }
  double getMaxCorrespondenceDistance() const { return p_.max_corr_dist; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  int getMaximumIterations() const { return p_.max_iterations; }
  void setTransformationEpsilon(double e) { p_.transformation_epsilon = e; }
  double getTransformationEpsilon() const { return p_.transformation_epsilon; }
  void setRotationEpsilon(double e) { p_.rotation_epsilon = e; }
  double getRotationEpsilon() const { return p_.rotation_epsilon; }
  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; }
  int getCorrespondenceRandomness() const { return k_correspondences_; }
  void setMaximumOptimizerIterations(int n) { p_.max_inner_iterations = n; }
  int getMaximumOptimizerIterations() const { return p_.max_inner_iterations; }
  void setUseReciprocalCorrespondences(bool b) { p_.use_reciprocal = b ? 1 : 0; }
  bool getUseReciprocalCorrespondences() const { return p_.use_reciprocal != 0; }
  // EXTENSION: gicp_epsilon, the small eigenvalue of the side covariances (a protected constant 0.001 in PCL)
  void setCovarianceEpsilon(double e) { p_.gicp_epsilon = e; }
  double getCovarianceEpsilon() const { return p_.gicp_epsilon; }

  void addCorrespondenceRejector(const CorrespondenceRejectorPtr &rejector) { rejectors_.push_back(rejector); }
  std::vector<CorrespondenceRejectorPtr> getCorrespondenceRejectors() { return rejectors_; }
  bool removeCorrespondenceRejector(unsigned int i)
  {
    if (i >= rejectors_.size()) return false;
    rejectors_.erase(rejectors_.begin() + i);
    return true;
  }
  void clearCorrespondenceRejectors() { rejectors_.clear(); }

  void align(PointCloudSource &output) { align(output, Matrix4::Identity(), false); }
  // the source starts under `guess` (PCL's Registration::align): the result is what the align finds from there, times guess
  void align(PointCloudSource &output, const Matrix4 &guess) { align(output, guess, true); }

  Matrix4 getFinalTransformation() const { return final_; }
  bool hasConverged() const { return converged_; }
  int getConvergenceState() const { return state_; }
  const mvr_icp_stats &getStats() const { return stats_; }

  // as IterativeClosestPoint::getFitnessScore
  double getFitnessScore(double max_range = DBL_MAX)
  {
    Device &d = Device::instance();
    if (!input_ || !target_) return DBL_MAX;
    detail::upload_cloud(d, src_.s, *input_);
    if (!aligned_once_) detail::upload_cloud(d, tgt_.s, *target_);
    double score = DBL_MAX;
    d.check(mvr_fitness(d.ctx(), src_.s, tgt_.s, final_.data(), max_range, p_.fma_dist, &score), "mvr_fitness");
    return score;
  }

 private:
  template <typename P>
  void upload_with_normals(Device &d, int slot, const PointCloud<P> &c)
  {
    detail::upload_cloud(d, slot, c);
    if (!detail::has_normal<P>::value && !c.empty()) {
      mvr_normal_params np = mvr_normal_params();
      np.k = k_correspondences_;
      d.check(mvr_cloud_estimate_normals(d.ctx(), 1, &slot, &np, nullptr), "mvr_cloud_estimate_normals");
    }
  }

  void align(PointCloudSource &output, const Matrix4 &guess, bool with_guess)
  {
    Device &d = Device::instance();
    converged_ = false; final_ = with_guess ? guess : Matrix4::Identity(); stats_ = mvr_icp_stats();
    if (!input_ || !target_) { state_ = MVR_CONV_NO_CORRESPONDENCES; return; }
    if (rejectors_.size() > (size_t)MVR_MAX_REJECTORS) throw Error(MVR_E_ARG, "mvr: more than MVR_MAX_REJECTORS correspondence rejectors");
    upload_with_normals(d, src_.s, *input_);
    upload_with_normals(d, tgt_.s, *target_);
    if (with_guess) d.check(mvr_cloud_transform_f32(d.ctx(), src_.s, src_.s, guess.data()), "mvr_cloud_transform_f32");
    std::vector<mvr_rejector> chain;
    for (const CorrespondenceRejectorPtr &r : rejectors_) chain.push_back(r->stage());
    std::vector<mvr_gicp_iter_trace> trace((size_t)std::max(1, p_.max_iterations));
    float T[16];
    const int rc = mvr_icp_align_gicp(d.ctx(), src_.s, tgt_.s, out_.s, &p_, chain.data(), (int)chain.size(), T, &stats_, trace.data(), (int)trace.size());
    if (rc == MVR_OK || rc == MVR_E_NOCORR) {        // every rejector learns what its stage did in the last iteration
      const size_t last = std::min(trace.size() - 1, (size_t)std::max(0, stats_.iterations - (rc == MVR_OK ? 1 : 0)));
      for (size_t k = 0; k < rejectors_.size(); ++k) rejectors_[k]->noteStage(trace[last].stages[k]);
    }
    if (rc != MVR_OK && rc != MVR_E_NOCORR && rc != MVR_E_SINGULAR) d.check(rc, "mvr_icp_align_gicp");
    if (rc == MVR_E_NOCORR)
      std::fprintf(stderr, "[mvr::GeneralizedIterativeClosestPoint::computeTransformation] Not enough correspondences found. "
                           "Relax your threshold parameters.\n");
    if (with_guess) { float F[16]; mvr_mat4f_mul(T, guess.data(), F); for (int k = 0; k < 16; ++k) final_.m[k] = F[k]; }
    else for (int k = 0; k < 16; ++k) final_.m[k] = T[k];
    converged_ = stats_.converged != 0;
    state_ = stats_.state;
    if (detail::has_normal<PointSource>::value && &output != input_.get()) output = *input_;      // (the fields beside x, y, z and the normal)
    detail::download_cloud(d, out_.s, output);
    aligned_once_ = true;
  }

  mvr_gicp_params p_;
  mvr_icp_stats stats_ = mvr_icp_stats();
  int k_correspondences_ = 20;
  PointCloudSourcePtr input_;
  PointCloudTargetPtr target_;
  Matrix4 final_;
  bool converged_ = false, aligned_once_ = false;
  int state_ = MVR_CONV_NOT;
  std::vector<CorrespondenceRejectorPtr> rejectors_;
  SlotGuard src_, tgt_, out_;
};

// ---------------------------------------------------------------- Normal Distributions Transform
// pcl::NormalDistributionsTransform over mvr_ndt_align (rules N1-N12 in mvr_hip.h), with PCL's names and PCL's defaults --
// which are meant for metres: setResolution and setStepSize take the cloud's unit.  DEVIATIONS (N3, N4, N5, N7-N9): C^-1 from
// the eigen-decomposition instead of a numerical inverse; the guess is applied as a matrix and the pose parametrises the
// increment on top of it; the 27 neighbouring voxels instead of a radius search over all centroids; a backtracking line search
// in the place of More-Thuente; the align may stop on its first iteration.  EXTENSIONS: setMinPointsPerVoxel, setRotationOrigin.
// getSearchMethodTarget is not offered.
template <typename PointSource, typename PointTarget>
class NormalDistributionsTransform {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef typename PointCloudSource::Ptr PointCloudSourcePtr;
  typedef typename PointCloudTarget::Ptr PointCloudTargetPtr;
  typedef Mat4<float> Matrix4;

  NormalDistributionsTransform() { mvr_ndt_default_params(&p_); }      // PCL's defaults

  void setInputSource(const PointCloudSourcePtr &c) { input_ = c; }
  void setInputTarget(const PointCloudTargetPtr &c) { target_ = c; }
  PointCloudSourcePtr const getInputSource() const { return input_; }
  PointCloudTargetPtr const getInputTarget() const { return target_; }
  void setResolution(float r) { p_.resolution = (double)r; }
  float getResolution() const { return (float)p_.resolution; }
  void setStepSize(double s) { p_.step_size = s; }
  double getStepSize() const { return p_.step_size; }
  void setOulierRatio(double r) { p_.outlier_ratio = r; }               // (PCL's spelling)
  double getOulierRatio() const { return p_.outlier_ratio; }
  void setOutlierRatio(double r) { p_.outlier_ratio = r; }              // (newer PCL)
  double getOutlierRatio() const { return p_.outlier_ratio; }
  void setTransformationEpsilon(double e) { p_.transformation_epsilon = e; }
  double getTransformationEpsilon() const { return p_.transformation_epsilon; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  int getMaximumIterations() const { return p_.max_iterations; }
  // EXTENSIONS: VoxelGridCovariance's minimum (6), and the point the rotation parameters turn about (N4; PCL: the origin)
  void setMinPointsPerVoxel(int n) { p_.min_points_per_voxel = n; }
  int getMinPointsPerVoxel() const { return p_.min_points_per_voxel; }
  void setRotationOrigin(double x, double y, double z) { p_.origin[0] = x; p_.origin[1] = y; p_.origin[2] = z; }

  void align(PointCloudSource &output) { align(output, nullptr); }
  // the result is what the align finds on top of `guess`, times guess (N4: the source itself is never moved or re-rounded)
  void align(PointCloudSource &output, const Matrix4 &guess) { align(output, &guess); }

  Matrix4 getFinalTransformation() const { return final_; }
  bool hasConverged() const { return converged_; }
  int getFinalNumIteration() const { return stats_.iterations; }
  double getTransformationProbability() const { return input_ && !input_->empty() ? stats_.score / (double)input_->size() : 0.0; }
  const mvr_ndt_stats &getStats() const { return stats_; }

  // as IterativeClosestPoint::getFitnessScore
  double getFitnessScore(double max_range = DBL_MAX)
  {
    Device &d = Device::instance();
    if (!input_ || !target_) return DBL_MAX;
    detail::upload_cloud(d, src_.s, *input_);
    if (!aligned_once_) detail::upload_cloud(d, tgt_.s, *target_);
    double score = DBL_MAX;
    d.check(mvr_fitness(d.ctx(), src_.s, tgt_.s, final_.data(), max_range, 0, &score), "mvr_fitness");
    return score;
  }

 private:
  void align(PointCloudSource &output, const Matrix4 *guess)
  {
    Device &d = Device::instance();
    converged_ = false; final_ = guess ? *guess : Matrix4::Identity(); stats_ = mvr_ndt_stats();
    if (!input_ || !target_) return;
    detail::upload_cloud(d, src_.s, *input_);
    detail::upload_cloud(d, tgt_.s, *target_);
    double G[16];
    if (guess) for (int k = 0; k < 16; ++k) G[k] = (double)guess->data()[k];
    float T[16];
    const int rc = mvr_ndt_align(d.ctx(), src_.s, tgt_.s, out_.s, &p_, guess ? G : nullptr, T, nullptr, &stats_, nullptr, 0);
    if (rc != MVR_E_NOCORR) d.check(rc, "mvr_ndt_align");
    else std::fprintf(stderr, "[mvr::NormalDistributionsTransform::computeTransformation] The source overlaps no cell of the target.\n");
    for (int k = 0; k < 16; ++k) final_.m[k] = T[k];
    converged_ = stats_.converged != 0;
    detail::download_cloud(d, out_.s, output);
    aligned_once_ = true;
  }

  mvr_ndt_params p_;
  mvr_ndt_stats stats_ = mvr_ndt_stats();
  PointCloudSourcePtr input_;
  PointCloudTargetPtr target_;
  Matrix4 final_;
  bool converged_ = false, aligned_once_ = false;
  SlotGuard src_, tgt_, out_;
};

// ---------------------------------------------------------------- normals
namespace search {
// pcl::search::KdTree: the neighbour search is the library's grid walk on the GPU (mvr_knn, mvr_radius_search in mvr_hip.h), so
// there is no tree to build: setInputCloud stores the pointer, the first search uploads the cloud into a slot of the thread's
// context, and later searches reuse it until the next setInputCloud.  The feature classes that take a tree through
// setSearchMethod go on ignoring it (they upload their own input).  nearestKSearch / radiusSearch have PCL's signatures and
// return the number of neighbours found; the lists are those of mvr_knn (ascending by (d2, index), cut at the last finite
// entry) and of mvr_radius_search (rules RS1-RS5: d2 <= r2, not FLANN's <; with setSortedResults(false) and max_nn = 0 the
// order is unspecified).  The single-point forms upload a one-point query cloud per call: the batch forms are the ones to use.
// A search before setInputCloud, a k outside 1..MVR_MAX_KNN or a radius that is not finite and > 0 prints an error and finds
// nothing (0).
template <typename PointT>
class KdTree {
 public:
  typedef std::shared_ptr<KdTree<PointT> > Ptr;
  typedef std::shared_ptr<const KdTree<PointT> > ConstPtr;
  typedef PointCloud<PointT> Cloud;
  typedef typename Cloud::ConstPtr PointCloudConstPtr;

  explicit KdTree(bool sorted = true) : sorted_(sorted) {}
  void setInputCloud(const PointCloudConstPtr &cloud) { input_ = cloud; slot_.reset(); }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setSortedResults(bool sorted) { sorted_ = sorted; }
  bool getSortedResults() const { return sorted_; }

  int nearestKSearch(const PointT &point, int k, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances) const
  {
    std::vector<std::vector<int> > vi; std::vector<std::vector<float> > vd;
    knn(&point, 1, k, vi, vd);
    return take_first(vi, vd, k_indices, k_sqr_distances);
  }
  int nearestKSearch(const Cloud &cloud, int index, int k, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances) const
  {
    if (!index_ok(cloud, index, "nearestKSearch")) { k_indices.clear(); k_sqr_distances.clear(); return 0; }
    return nearestKSearch(cloud.points[(size_t)index], k, k_indices, k_sqr_distances);
  }
  int nearestKSearch(int index, int k, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances) const
  {
    if (!input_ok("nearestKSearch")) { k_indices.clear(); k_sqr_distances.clear(); return 0; }
    return nearestKSearch(*input_, index, k, k_indices, k_sqr_distances);
  }
  void nearestKSearch(const Cloud &cloud, const std::vector<int> &indices, int k, std::vector<std::vector<int> > &k_indices,
                      std::vector<std::vector<float> > &k_sqr_distances) const
  {
    std::vector<PointT> sel;
    if (!select(cloud, indices, sel, "nearestKSearch")) { k_indices.clear(); k_sqr_distances.clear(); return; }
    knn(indices.empty() ? (cloud.empty() ? nullptr : &cloud.points[0]) : sel.data(), indices.empty() ? cloud.size() : sel.size(), k, k_indices,
        k_sqr_distances);
  }

  int radiusSearch(const PointT &point, double radius, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances, unsigned int max_nn = 0) const
  {
    std::vector<std::vector<int> > vi; std::vector<std::vector<float> > vd;
    radius_rows(&point, 1, radius, max_nn, vi, vd);
    return take_first(vi, vd, k_indices, k_sqr_distances);
  }
  int radiusSearch(const Cloud &cloud, int index, double radius, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances,
                   unsigned int max_nn = 0) const
  {
    if (!index_ok(cloud, index, "radiusSearch")) { k_indices.clear(); k_sqr_distances.clear(); return 0; }
    return radiusSearch(cloud.points[(size_t)index], radius, k_indices, k_sqr_distances, max_nn);
  }
  int radiusSearch(int index, double radius, std::vector<int> &k_indices, std::vector<float> &k_sqr_distances, unsigned int max_nn = 0) const
  {
    if (!input_ok("radiusSearch")) { k_indices.clear(); k_sqr_distances.clear(); return 0; }
    return radiusSearch(*input_, index, radius, k_indices, k_sqr_distances, max_nn);
  }
  void radiusSearch(const Cloud &cloud, const std::vector<int> &indices, double radius, std::vector<std::vector<int> > &k_indices,
                    std::vector<std::vector<float> > &k_sqr_distances, unsigned int max_nn = 0) const
  {
    std::vector<PointT> sel;
    if (!select(cloud, indices, sel, "radiusSearch")) { k_indices.clear(); k_sqr_distances.clear(); return; }
    radius_rows(indices.empty() ? (cloud.empty() ? nullptr : &cloud.points[0]) : sel.data(), indices.empty() ? cloud.size() : sel.size(), radius, max_nn,
                k_indices, k_sqr_distances);
  }

 private:
  static int take_first(std::vector<std::vector<int> > &vi, std::vector<std::vector<float> > &vd, std::vector<int> &i, std::vector<float> &d)
  {
    i.clear(); d.clear();
    if (!vi.empty()) { i.swap(vi[0]); d.swap(vd[0]); }
    return (int)i.size();
  }
  bool input_ok(const char *fn) const
  {
    if (input_) return true;
    std::fprintf(stderr, "[search::KdTree::%s] No input dataset was given (setInputCloud)!\n", fn);
    return false;
  }
  bool index_ok(const Cloud &cloud, int index, const char *fn) const
  {
    if (index >= 0 && (size_t)index < cloud.size()) return true;
    std::fprintf(stderr, "[search::KdTree::%s] The index %d is outside the cloud (%zu points).\n", fn, index, cloud.size());
    return false;
  }
  bool select(const Cloud &cloud, const std::vector<int> &indices, std::vector<PointT> &sel, const char *fn) const
  {
    sel.reserve(indices.size());
    for (size_t i = 0; i < indices.size(); ++i) {
      if (!index_ok(cloud, indices[i], fn)) return false;
      sel.push_back(cloud.points[(size_t)indices[i]]);
    }
    return true;
  }
  // the slot that holds the input cloud, uploaded at the first search after setInputCloud
  int target() const
  {
    if (!slot_) {
      slot_.reset(new SlotGuard());
      Device::instance().upload(slot_->s, *input_);
    }
    return slot_->s;
  }
  static void upload_queries(Device &d, int slot, const PointT *q, size_t n)
  {
    static_assert(sizeof(PointT) == 16, "16-byte XYZ points expected");
    d.check(mvr_cloud_upload(d.ctx(), slot, n ? q->data : nullptr, n, sizeof(PointT)), "mvr_cloud_upload");
  }
  void knn(const PointT *q, size_t n, int k, std::vector<std::vector<int> > &vi, std::vector<std::vector<float> > &vd) const
  {
    vi.clear(); vd.clear();
    if (!input_ok("nearestKSearch")) return;
    if (k < 1 || k > MVR_MAX_KNN) {
      std::fprintf(stderr, "[search::KdTree::nearestKSearch] k = %d is outside 1..%d.\n", k, MVR_MAX_KNN);
      return;
    }
    vi.resize(n); vd.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    const int t = target();
    SlotGuard qs;
    upload_queries(d, qs.s, q, n);
    std::vector<uint32_t> idx(n * (size_t)k);
    std::vector<float> d2(n * (size_t)k);
    d.check(mvr_knn(d.ctx(), qs.s, t, k, 0, idx.data(), d2.data()), "mvr_knn");
    for (size_t i = 0; i < n; ++i) {
      size_t m = 0;
      while (m < (size_t)k && idx[i * k + m] != UINT32_MAX) ++m;
      vi[i].assign(idx.begin() + (ptrdiff_t)(i * k), idx.begin() + (ptrdiff_t)(i * k + m));
      vd[i].assign(d2.begin() + (ptrdiff_t)(i * k), d2.begin() + (ptrdiff_t)(i * k + m));
    }
  }
  void radius_rows(const PointT *q, size_t n, double radius, unsigned int max_nn, std::vector<std::vector<int> > &vi,
                   std::vector<std::vector<float> > &vd) const
  {
    vi.clear(); vd.clear();
    if (!input_ok("radiusSearch")) return;
    if (!(std::isfinite(radius) && radius > 0.0)) {
      std::fprintf(stderr, "[search::KdTree::radiusSearch] The radius (%f) must be finite and > 0.\n", radius);
      return;
    }
    vi.resize(n); vd.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    const int t = target();
    SlotGuard qs;
    upload_queries(d, qs.s, q, n);
    mvr_radius_params p;
    mvr_radius_default_params(&p);
    p.radius = radius; p.max_nn = max_nn; p.sorted = sorted_ ? 1 : 0;
    std::vector<uint64_t> offsets(n + 1);
    size_t total = 0;
    d.check(mvr_radius_search(d.ctx(), qs.s, t, &p, offsets.data(), nullptr, nullptr, 0, &total), "mvr_radius_search");
    std::vector<uint32_t> idx(total ? total : 1);
    std::vector<float> d2(total ? total : 1);
    if (total) d.check(mvr_radius_search(d.ctx(), qs.s, t, &p, offsets.data(), idx.data(), d2.data(), total, &total), "mvr_radius_search");
    for (size_t i = 0; i < n; ++i) {
      vi[i].assign(idx.begin() + (ptrdiff_t)offsets[i], idx.begin() + (ptrdiff_t)offsets[i + 1]);
      vd[i].assign(d2.begin() + (ptrdiff_t)offsets[i], d2.begin() + (ptrdiff_t)offsets[i + 1]);
    }
  }

  bool sorted_;
  PointCloudConstPtr input_;
  mutable std::shared_ptr<SlotGuard> slot_;      // (copies of a tree share the uploaded cloud until one of them gets another)
};
}  // namespace search

// pcl::NormalEstimation<PointInT, PointOutT> (features/normal_3d.h): setKSearch XOR setRadiusSearch, setViewPoint, compute.
// Semantics: mvr_cloud_estimate_normals (mvr_hip.h).  As PCL's Feature::compute, a call with both or neither of k / radius
// set prints an error and leaves `output` empty.  setSearchSurface / setIndices (Feature's own): the neighbours are taken from
// the surface, and `output` holds one normal per index, in the order of the indices, or one per input point -- rules Q1-Q8 of
// mvr_cloud_estimate_normals_at.  An index outside the input cloud prints an error and leaves `output` empty.
template <typename PointInT, typename PointOutT>
class NormalEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setSearchSurface(const PointCloudConstPtr &c) { surface_ = c; }
  PointCloudConstPtr getSearchSurface() const { return surface_; }
  void setIndices(const IndicesConstPtr &i) { indices_ = i; }
  IndicesConstPtr getIndices() const { return indices_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setViewPoint(float vpx, float vpy, float vpz) { vp_[0] = vpx; vp_[1] = vpy; vp_[2] = vpz; }
  void getViewPoint(float &vpx, float &vpy, float &vpz) const { vpx = vp_[0]; vpy = vp_[1]; vpz = vp_[2]; }

  void compute(PointCloudOut &output)
  {
    output.clear();
    if (!input_) { std::fprintf(stderr, "[NormalEstimation::compute] No input dataset was given!\n"); return; }
    if ((k_ != 0) == (radius_ != 0.0)) {
      std::fprintf(stderr, "[NormalEstimation::compute] Set exactly one of setKSearch / setRadiusSearch (k = %d, radius = %f).\n", k_, radius_);
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, *input_);
    mvr_normal_params p;
    p.k = k_; p.radius = radius_; p.fma_dist = 0;
    for (int j = 0; j < 3; ++j) p.viewpoint[j] = vp_[j];
    if (surface_ || indices_) {
      std::vector<uint32_t> idx;
      if (indices_)
        for (int i : *indices_) {
          if (i < 0 || (size_t)i >= input_->size()) { std::fprintf(stderr, "[NormalEstimation::compute] The index %d lies outside the input cloud (%zu points).\n", i, input_->size()); return; }
          idx.push_back((uint32_t)i);
        }
      std::shared_ptr<SlotGuard> t;
      if (surface_ && surface_ != input_) { t = std::make_shared<SlotGuard>(); d.upload(t->s, *surface_); }
      const size_t rows = indices_ ? idx.size() : input_->size();
      std::vector<float> curv(rows ? rows : 1), nrm(4 * (rows ? rows : 1));
      static const uint32_t none[1] = {0};
      d.check(mvr_cloud_estimate_normals_at(d.ctx(), s.s, indices_ ? (idx.empty() ? none : idx.data()) : nullptr, idx.size(), t ? t->s : s.s, &p, 0,
                                            nrm.data(), curv.data()), "mvr_cloud_estimate_normals_at");
      output.resize(rows);
      for (size_t i = 0; i < rows; ++i) {
        PointOutT &o = output.points[i];
        o.normal_x = nrm[4 * i]; o.normal_y = nrm[4 * i + 1]; o.normal_z = nrm[4 * i + 2]; o.curvature = curv[i];
      }
      return;
    }
    const size_t n = input_->size();
    std::vector<float> curv(n ? n : 1), nrm(4 * (n ? n : 1));
    float *cp = curv.data();
    d.check(mvr_cloud_estimate_normals(d.ctx(), 1, &s.s, &p, &cp), "mvr_cloud_estimate_normals");
    size_t got = 0;
    if (n) d.check(mvr_cloud_download_normals(d.ctx(), s.s, nrm.data(), n, 16, &got), "mvr_cloud_download_normals");
    output.resize(n);
    for (size_t i = 0; i < n; ++i) {
      PointOutT &o = output.points[i];
      o.normal_x = nrm[4 * i]; o.normal_y = nrm[4 * i + 1]; o.normal_z = nrm[4 * i + 2]; o.curvature = curv[i];
    }
  }

 private:
  PointCloudConstPtr input_, surface_;
  IndicesConstPtr indices_;
  KdTreePtr tree_;
  int k_ = 0;
  double radius_ = 0.0;
  float vp_[3] = {0.f, 0.f, 0.f};
};

// ---------------------------------------------------------------- voxel grid
// pcl::VoxelGrid<PointT> (filters/voxel_grid.h) for 16-byte XYZ points: setLeafSize, setMinimumPointsNumberPerVoxel,
// filter; downsample_all_data as PCL's default (true).  Semantics: mvr_cloud_voxel_grid (mvr_hip.h).  `output` may be the input
// cloud itself (`vg.setInputCloud(cloud); vg.filter(*cloud);`): the input is on the device before `output` is written, which
// is what PCL's Filter::filter gets by filtering such a call into a temporary.  A missing input or a leaf that is not finite
// and > 0 prints an error and leaves `output` empty (untouched when it is the input); when PCL's integer indices would
// overflow, the output is a copy of the input and PCL's warning is printed.
template <typename PointT>
class VoxelGrid {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz; }
  void setMinimumPointsNumberPerVoxel(unsigned int m) { min_points_ = m; }
  unsigned int getMinimumPointsNumberPerVoxel() const { return min_points_; }

  void filter(PointCloudT &output)
  {
    if (!input_) { std::fprintf(stderr, "[pcl::VoxelGrid::filter] No input dataset given!\n"); output.clear(); return; }
    for (int a = 0; a < 3; ++a)
      if (!(std::isfinite(leaf_[a]) && leaf_[a] > 0.f)) {
        std::fprintf(stderr, "[pcl::VoxelGrid::filter] Leaf size (%f, %f, %f) must be finite and > 0.\n", leaf_[0], leaf_[1], leaf_[2]);
        if (&output != input_.get()) output.clear();
        return;
      }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, *input_);              // first: `output` may alias the input
    size_t n = 0;
    int passthrough = 0;
    d.check(mvr_cloud_voxel_grid(d.ctx(), s.s, s.s, leaf_, min_points_, &n, nullptr, &passthrough), "mvr_cloud_voxel_grid");
    if (passthrough)
      std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
    d.download(s.s, output);
  }

 private:
  PointCloudConstPtr input_;
  float leaf_[3] = {0.f, 0.f, 0.f};
  unsigned int min_points_ = 0;
};

// ---------------------------------------------------------------- outlier removal
// pcl::StatisticalOutlierRemoval<PointT> (filters/statistical_outlier_removal.h) and pcl::RadiusOutlierRemoval<PointT>
// (filters/radius_outlier_removal.h) for 16-byte XYZ points, PCL's member names and defaults (mean_k 1, stddev_mul 0,
// min_neighbors 1).  Semantics: mvr_cloud_statistical_outlier_removal / mvr_cloud_radius_outlier_removal (mvr_hip.h) -- one
// call on the GPU per filter().  `output` may be the input cloud itself, as for VoxelGrid.  filter(indices) gives the indices
// of the output points instead; constructed with extract_removed_indices = true, getRemovedIndices() holds the complement
// after a filter().  A missing input or a parameter outside its range prints an error and leaves the output empty
// (untouched when it is the input).
namespace detail {
// the ascending complement of the ascending list `kept` in 0..n-1
inline void complement_indices(const std::vector<uint32_t> &kept, size_t n_kept, size_t n, std::vector<int> &out)
{
  out.clear();
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    if (k < n_kept && kept[k] == i) ++k;
    else out.push_back((int)i);
  }
}
}  // namespace detail

template <typename PointT>
class StatisticalOutlierRemoval {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  explicit StatisticalOutlierRemoval(bool extract_removed_indices = false) : extract_removed_(extract_removed_indices) {}
  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setMeanK(int k) { mean_k_ = k; }
  int getMeanK() const { return mean_k_; }
  void setStddevMulThresh(double m) { stddev_mul_ = m; }
  double getStddevMulThresh() const { return stddev_mul_; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  IndicesConstPtr getRemovedIndices() const { return removed_; }
  void getRemovedIndices(std::vector<int> &out) const { out = *removed_; }

  void filter(PointCloudT &output) { run(&output, nullptr); }
  void filter(std::vector<int> &indices) { run(nullptr, &indices); }

 private:
  void run(PointCloudT *output, std::vector<int> *indices)
  {
    removed_->clear();
    if (indices) indices->clear();
    if (!input_) { std::fprintf(stderr, "[pcl::StatisticalOutlierRemoval::filter] No input dataset given!\n"); if (output) output->clear(); return; }
    if (mean_k_ < 1 || mean_k_ > MVR_MAX_KNN || !std::isfinite(stddev_mul_)) {
      std::fprintf(stderr, "[pcl::StatisticalOutlierRemoval::filter] mean_k (%d) must be in 1..%d and the multiplier (%f) finite.\n", mean_k_, MVR_MAX_KNN, stddev_mul_);
      if (output && output != input_.get()) output->clear();
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, *input_);              // first: `output` may alias the input
    const size_t n = input_->size();
    std::vector<uint32_t> kept(n ? n : 1);
    size_t n_out = 0;
    mvr_sor_params p;
    p.mean_k = mean_k_; p.stddev_mul = stddev_mul_; p.negative = negative_ ? 1 : 0; p.fma_dist = 0;
    d.check(mvr_cloud_statistical_outlier_removal(d.ctx(), s.s, s.s, &p, &n_out, kept.data(), nullptr, nullptr), "mvr_cloud_statistical_outlier_removal");
    if (extract_removed_) detail::complement_indices(kept, n_out, n, *removed_);
    if (indices) indices->assign(kept.begin(), kept.begin() + (std::ptrdiff_t)n_out);
    if (output) d.download(s.s, *output);
  }

  PointCloudConstPtr input_;
  int mean_k_ = 1;
  double stddev_mul_ = 0.0;
  bool negative_ = false, extract_removed_ = false;
  std::shared_ptr<std::vector<int> > removed_ = std::make_shared<std::vector<int> >();
};

template <typename PointT>
class RadiusOutlierRemoval {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  explicit RadiusOutlierRemoval(bool extract_removed_indices = false) : extract_removed_(extract_removed_indices) {}
  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setMinNeighborsInRadius(int m) { min_neighbors_ = m; }
  int getMinNeighborsInRadius() const { return min_neighbors_; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }
  IndicesConstPtr getRemovedIndices() const { return removed_; }
  void getRemovedIndices(std::vector<int> &out) const { out = *removed_; }

  void filter(PointCloudT &output) { run(&output, nullptr); }
  void filter(std::vector<int> &indices) { run(nullptr, &indices); }

 private:
  void run(PointCloudT *output, std::vector<int> *indices)
  {
    removed_->clear();
    if (indices) indices->clear();
    if (!input_) { std::fprintf(stderr, "[pcl::RadiusOutlierRemoval::filter] No input dataset given!\n"); if (output) output->clear(); return; }
    if (!(std::isfinite(radius_) && radius_ > 0.0) || min_neighbors_ < 0) {
      std::fprintf(stderr, "[pcl::RadiusOutlierRemoval::filter] The radius (%f) must be finite and > 0, min_neighbors (%d) >= 0.\n", radius_, min_neighbors_);
      if (output && output != input_.get()) output->clear();
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, *input_);              // first: `output` may alias the input
    const size_t n = input_->size();
    std::vector<uint32_t> kept(n ? n : 1);
    size_t n_out = 0;
    mvr_ror_params p;
    p.radius = radius_; p.min_neighbors = min_neighbors_; p.negative = negative_ ? 1 : 0; p.fma_dist = 0;
    d.check(mvr_cloud_radius_outlier_removal(d.ctx(), s.s, s.s, &p, &n_out, kept.data(), nullptr), "mvr_cloud_radius_outlier_removal");
    if (extract_removed_) detail::complement_indices(kept, n_out, n, *removed_);
    if (indices) indices->assign(kept.begin(), kept.begin() + (std::ptrdiff_t)n_out);
    if (output) d.download(s.s, *output);
  }

  PointCloudConstPtr input_;
  double radius_ = 0.0;
  int min_neighbors_ = 1;
  bool negative_ = false, extract_removed_ = false;
  std::shared_ptr<std::vector<int> > removed_ = std::make_shared<std::vector<int> >();
};

// ---------------------------------------------------------------- moving least squares
// pcl::MovingLeastSquares<PointInT, PointOutT> (surface/mls.h) with upsampling NONE and the SIMPLE projection, PCL's member
// names and defaults (polynomial order 2, sqr_gauss_param = the squared search radius until setSqrGaussParam is called, no
// normals).  Semantics: mvr_cloud_mls (mvr_hip.h) -- one call on the GPU per process().  PointInT / PointOutT: any point
// whose first three floats are x, y, z (PointXYZ, PointNormal); an output type with normal_x / curvature members receives
// the normals (with setComputeNormals(true); oriented towards the origin, the sensor of a raw scan) and the curvature.
// `output` may be the input cloud itself.  A missing input or a parameter outside its range prints an error and leaves the
// output empty (untouched when it is the input).  Upsampling, the ORTHOGONAL projection, orders above 2 and cached
// polynomials are not offered.
namespace detail {
template <class P>
auto set_normal(P &o, const float *n, float curv, int) -> decltype((void)o.normal_x) { o.normal_x = n[0]; o.normal_y = n[1]; o.normal_z = n[2]; o.curvature = curv; }
template <class P>
void set_normal(P &, const float *, float, long) {}
}  // namespace detail

template <typename PointInT, typename PointOutT>
class MovingLeastSquares {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudInConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;

  void setInputCloud(const PointCloudInConstPtr &c) { input_ = c; }
  PointCloudInConstPtr getInputCloud() const { return input_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setSearchRadius(double r) { radius_ = r; if (!gauss_set_) sqr_gauss_ = r * r; }
  double getSearchRadius() const { return radius_; }
  void setPolynomialOrder(int order) { order_ = order; }
  int getPolynomialOrder() const { return order_; }
  void setPolynomialFit(bool fit) { order_ = fit ? (order_ > 1 ? order_ : 2) : 0; }      // (PCL 1.7's switch: order > 1 is the fit)
  bool getPolynomialFit() const { return order_ > 1; }
  void setSqrGaussParam(double g) { sqr_gauss_ = g; gauss_set_ = true; }
  double getSqrGaussParam() const { return sqr_gauss_; }
  void setComputeNormals(bool c) { compute_normals_ = c; }
  PointIndicesPtr getCorrespondingIndices() const { return corresponding_; }

  void process(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12 && sizeof(PointOutT) >= 12, "points that begin with x, y, z expected");
    corresponding_->indices.clear();
    const bool alias = (const void *)&output == (const void *)input_.get();
    if (!input_) { std::fprintf(stderr, "[pcl::MovingLeastSquares::process] No input dataset given!\n"); output.clear(); return; }
    if (!(std::isfinite(radius_) && radius_ > 0.0) || !(std::isfinite(sqr_gauss_) && sqr_gauss_ > 0.0) || order_ < 0 || order_ > 2) {
      std::fprintf(stderr, "[pcl::MovingLeastSquares::process] The search radius (%f) and the gauss parameter (%f) must be finite and > 0, the polynomial order (%d) in 0..2.\n",
                   radius_, sqr_gauss_, order_);
      if (!alias) output.clear();
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    const size_t n = input_->size();
    // first: `output` may alias the input
    d.check(mvr_cloud_upload(d.ctx(), s.s, n ? input_->points[0].data : nullptr, n, sizeof(PointInT)), "mvr_cloud_upload");
    mvr_mls_params p;
    p.radius = radius_; p.order = order_; p.sqr_gauss_param = sqr_gauss_; p.compute_normals = compute_normals_ ? 1 : 0; p.orient = 0;
    p.viewpoint[0] = p.viewpoint[1] = p.viewpoint[2] = 0.f; p.fma_dist = 0;
    std::vector<uint32_t> kept(n ? n : 1);
    std::vector<float> curv(n ? n : 1);
    size_t m = 0;
    d.check(mvr_cloud_mls(d.ctx(), s.s, s.s, &p, &m, kept.data(), curv.data()), "mvr_cloud_mls");
    std::vector<float> xyz(4 * (m ? m : 1)), nrm(4 * (m ? m : 1), 0.f);
    size_t got = 0;
    if (m) d.check(mvr_cloud_download(d.ctx(), s.s, xyz.data(), m, 16, &got), "mvr_cloud_download");
    if (m && compute_normals_) d.check(mvr_cloud_download_normals(d.ctx(), s.s, nrm.data(), m, 16, &got), "mvr_cloud_download_normals");
    output.clear();
    output.resize(m);
    for (size_t i = 0; i < m; ++i) {
      PointOutT &o = output.points[i];
      o.x = xyz[4 * i]; o.y = xyz[4 * i + 1]; o.z = xyz[4 * i + 2];
      detail::set_normal(o, &nrm[4 * i], curv[i], 0);
    }
    corresponding_->indices.assign(kept.begin(), kept.begin() + (std::ptrdiff_t)m);
  }

 private:
  PointCloudInConstPtr input_;
  KdTreePtr tree_;
  double radius_ = 0.0, sqr_gauss_ = 0.0;
  int order_ = 2;
  bool gauss_set_ = false, compute_normals_ = false;
  PointIndicesPtr corresponding_ = std::make_shared<PointIndices>();
};

// ---------------------------------------------------------------- surface reconstruction
// pcl::MarchingCubesHoppe<PointNT> (surface/marching_cubes_hoppe.h): setInputCloud, setSearchMethod (accepted, unused: the
// search is the library's), setGridResolution, setIsoLevel, setPercentageExtendGrid, setDistanceIgnore, reconstruct.  Semantics:
// mvr_cloud_marching_cubes_hoppe (mvr_hip.h, rules M1-M15) -- one call on the GPU per reconstruct().  PointNT: a point with x, y,
// z and normal_x / y / z (PointNormal).  reconstruct(PolygonMesh &) fills mesh.cloud (DEVIATION: a PointCloud<PointXYZ>, see
// PolygonMesh) and mesh.polygons; reconstruct(points, polygons) gives the vertices as PointNT with zero normals, as PCL leaves
// them.  Without setWeld (EXTENSION, rule M13) polygon t is (3t, 3t + 1, 3t + 2) over a triangle soup, as in PCL.  A missing
// input or a parameter outside rule M12 prints an error and leaves the outputs empty.
template <typename PointNT>
class MarchingCubesHoppe {
 public:
  typedef PointCloud<PointNT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudInConstPtr;
  typedef search::KdTree<PointNT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<MarchingCubesHoppe<PointNT> > Ptr;

  void setInputCloud(const PointCloudInConstPtr &c) { input_ = c; }
  PointCloudInConstPtr getInputCloud() const { return input_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setGridResolution(int res_x, int res_y, int res_z) { p_.res[0] = res_x; p_.res[1] = res_y; p_.res[2] = res_z; }
  void getGridResolution(int &res_x, int &res_y, int &res_z) const { res_x = p_.res[0]; res_y = p_.res[1]; res_z = p_.res[2]; }
  void setIsoLevel(float iso_level) { p_.iso_level = iso_level; }
  float getIsoLevel() const { return p_.iso_level; }
  void setPercentageExtendGrid(float percentage) { p_.percentage_extend_grid = percentage; }
  float getPercentageExtendGrid() const { return p_.percentage_extend_grid; }
  void setDistanceIgnore(float dist_ignore) { p_.dist_ignore = dist_ignore; }
  float getDistanceIgnore() const { return p_.dist_ignore; }
  void setWeld(bool weld) { p_.weld = weld ? 1 : 0; }      // EXTENSION
  bool getWeld() const { return p_.weld != 0; }

  void reconstruct(PolygonMesh &output)
  {
    std::vector<float> xyz;
    run(xyz, output.polygons);
    output.cloud.clear();
    output.cloud.resize(xyz.size() / 3);
    for (size_t i = 0; i < output.cloud.size(); ++i) output.cloud.points[i] = PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  }
  void reconstruct(PointCloud<PointNT> &points, std::vector<Vertices> &polygons)
  {
    std::vector<float> xyz;
    run(xyz, polygons);
    points.clear();
    points.resize(xyz.size() / 3);
    for (size_t i = 0; i < points.size(); ++i) points.points[i] = PointNT(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  }

 private:
  void run(std::vector<float> &xyz, std::vector<Vertices> &polygons)
  {
    static_assert(detail::has_normal<PointNT>::value, "MarchingCubesHoppe needs points that carry normals");
    xyz.clear();
    polygons.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::MarchingCubesHoppe::reconstruct] No input dataset given!\n"); return; }
    Device &d = Device::instance();
    SlotGuard s;
    detail::upload_cloud(d, s.s, *input_);
    // a first capacity from the lattice's faces; a surface that needs more says how much (rule M11) and is asked again
    uint64_t nt = 0, nv = 0;
    size_t cap = 1024;
    if (p_.res[0] >= 2 && p_.res[1] >= 2 && p_.res[2] >= 2)
      cap = std::max<size_t>(cap, 8 * ((size_t)p_.res[0] * p_.res[1] + (size_t)p_.res[1] * p_.res[2] + (size_t)p_.res[0] * p_.res[2]));
    std::vector<uint32_t> idx;
    for (;;) {
      xyz.resize(cap * 9);
      if (p_.weld) idx.resize(cap * 3);
      const int rc = mvr_cloud_marching_cubes_hoppe(d.ctx(), s.s, &p_, nullptr, xyz.data(), cap, p_.weld ? idx.data() : nullptr, &nt, &nv);
      if (rc == MVR_E_ARG && nt > cap) { cap = (size_t)nt; continue; }
      if (rc == MVR_E_ARG) { std::fprintf(stderr, "[pcl::MarchingCubesHoppe::reconstruct] %s\n", mvr_last_error(d.ctx())); xyz.clear(); return; }
      d.check(rc, "mvr_cloud_marching_cubes_hoppe");
      break;
    }
    xyz.resize((size_t)nv * 3);
    polygons.resize((size_t)nt);
    for (size_t t = 0; t < (size_t)nt; ++t) {
      polygons[t].vertices.resize(3);
      for (uint32_t k = 0; k < 3; ++k) polygons[t].vertices[k] = p_.weld ? idx[3 * t + k] : (uint32_t)(3 * t + k);
    }
  }

  static mvr_mc_params defaults() { mvr_mc_params p; mvr_mc_default_params(&p); return p; }
  PointCloudInConstPtr input_;
  KdTreePtr tree_;
  mvr_mc_params p_ = defaults();
};

// ---------------------------------------------------------------- fast point feature histograms
// pcl::FPFHEstimation<PointInT, PointNT, PointOutT> (features/fpfh.h) in radius mode, the input cloud its own search surface:
// setInputCloud, setInputNormals, setSearchMethod, setRadiusSearch, compute.  Semantics: mvr_cloud_fpfh (mvr_hip.h) -- one call
// on the GPU per compute().  PointInT: any point whose first three floats are x, y, z; PointNT: any point with normal_x / y / z
// (Normal, PointNormal).  A point with a non-finite coordinate or normal gets a NaN signature (PCL does the same) and
// is_dense is cleared.  As PCL's Feature::compute, a missing input, missing normals, a normal cloud of another size or a
// radius that is not finite and > 0 prints an error and leaves `output` empty.  What this class cannot do it refuses with an
// exception, not silently: the k-neighbour mode (setKSearch with a non-zero k), setSearchSurface and setIndices.  (The two stay
// refused in this class and in PFHEstimation below: their drivers pin the refusal.  The library itself offers both --
// mvr_cloud_fpfh_at / mvr_cloud_pfh_at -- and ScanCloud::computeFPFHAt / computePFHAt are their C++ form.)
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33>
class FPFHEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointNT> PointCloudN;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setInputNormals(const PointCloudNConstPtr &n) { normals_ = n; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setKSearch(int k) { if (k != 0) throw std::invalid_argument("[pcl::FPFHEstimation::setKSearch] the k-neighbour mode is not offered: use setRadiusSearch"); }
  int getKSearch() const { return 0; }
  void setSearchSurface(const PointCloudConstPtr &) { throw std::invalid_argument("[pcl::FPFHEstimation::setSearchSurface] a separate search surface is not offered: the input cloud is its own surface"); }
  void setIndices(const IndicesConstPtr &) { throw std::invalid_argument("[pcl::FPFHEstimation::setIndices] index subsets are not offered: every point gets a signature"); }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12, "points that begin with x, y, z expected");
    static_assert(sizeof(PointOutT) == sizeof(float) * 3 * MVR_FPFH_BINS, "a 33-float signature expected");
    output.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::FPFHEstimation::compute] No input dataset was given!\n"); return; }
    if (!normals_ || normals_->size() != input_->size()) {
      std::fprintf(stderr, "[pcl::FPFHEstimation::compute] The number of points in the input dataset differs from the number of points in the dataset containing the normals!\n");
      return;
    }
    if (!(std::isfinite(radius_) && radius_ > 0.0)) {
      std::fprintf(stderr, "[pcl::FPFHEstimation::compute] The search radius (%f) must be finite and > 0 (setRadiusSearch).\n", radius_);
      return;
    }
    const size_t n = input_->size();
    output.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    SlotGuard s;
    d.check(mvr_cloud_upload(d.ctx(), s.s, input_->points[0].data, n, sizeof(PointInT)), "mvr_cloud_upload");
    std::vector<float> nrm(4 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointNT &q = normals_->points[i];
      nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
    }
    d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
    mvr_fpfh_params p;
    p.radius = radius_; p.fma_dist = 0;
    d.check(mvr_cloud_fpfh(d.ctx(), s.s, &p, output.points[0].histogram, nullptr, nullptr), "mvr_cloud_fpfh");
    for (size_t i = 0; i < n && output.is_dense; ++i)
      if (std::isnan(output.points[i].histogram[0])) output.is_dense = false;
  }

 private:
  PointCloudConstPtr input_;
  PointCloudNConstPtr normals_;
  KdTreePtr tree_;
  double radius_ = 0.0;
};

// ---------------------------------------------------------------- point feature histograms
// pcl::PFHEstimation<PointInT, PointNT, PointOutT> (features/pfh.h), the input cloud its own search surface: setInputCloud,
// setInputNormals, setSearchMethod, setRadiusSearch or setKSearch (the later call decides the mode, exactly one is in force),
// setMaximumCacheSize / setUseInternalCache (PCL's cache of pair features: accepted, no effect on the result, as in PCL),
// compute.  Semantics: mvr_cloud_pfh (mvr_hip.h) -- one call on the GPU per compute().  Points, normals, NaN signatures,
// is_dense and the error prints are those of FPFHEstimation above; setSearchSurface and setIndices are refused with an exception.
template <typename PointInT, typename PointNT, typename PointOutT = PFHSignature125>
class PFHEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointNT> PointCloudN;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setInputNormals(const PointCloudNConstPtr &n) { normals_ = n; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setRadiusSearch(double r) { radius_ = r; if (r != 0.0) k_ = 0; }
  double getRadiusSearch() const { return radius_; }
  void setKSearch(int k) { k_ = k; if (k != 0) radius_ = 0.0; }
  int getKSearch() const { return k_; }
  void setMaximumCacheSize(unsigned int n) { cache_size_ = n; }
  unsigned int getMaximumCacheSize() const { return cache_size_; }
  void setUseInternalCache(bool on) { use_cache_ = on; }
  bool getUseInternalCache() const { return use_cache_; }
  void setSearchSurface(const PointCloudConstPtr &) { throw std::invalid_argument("[pcl::PFHEstimation::setSearchSurface] a separate search surface is not offered: the input cloud is its own surface"); }
  void setIndices(const IndicesConstPtr &) { throw std::invalid_argument("[pcl::PFHEstimation::setIndices] index subsets are not offered: every point gets a signature"); }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12, "points that begin with x, y, z expected");
    static_assert(sizeof(PointOutT) == sizeof(float) * MVR_PFH_DIM, "a 125-float signature expected");
    output.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::PFHEstimation::compute] No input dataset was given!\n"); return; }
    if (!normals_ || normals_->size() != input_->size()) {
      std::fprintf(stderr, "[pcl::PFHEstimation::compute] The number of points in the input dataset differs from the number of points in the dataset containing the normals!\n");
      return;
    }
    const bool kmode = k_ != 0;
    if (kmode ? (k_ < 1 || k_ > MVR_MAX_KNN) : !(std::isfinite(radius_) && radius_ > 0.0)) {
      std::fprintf(stderr, "[pcl::PFHEstimation::compute] The search radius (%f) must be finite and > 0 (setRadiusSearch), or k (%d) in 1..%d (setKSearch).\n",
                   radius_, k_, MVR_MAX_KNN);
      return;
    }
    const size_t n = input_->size();
    output.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    SlotGuard s;
    d.check(mvr_cloud_upload(d.ctx(), s.s, input_->points[0].data, n, sizeof(PointInT)), "mvr_cloud_upload");
    std::vector<float> nrm(4 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointNT &q = normals_->points[i];
      nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
    }
    d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
    mvr_pfh_params p;
    p.radius = kmode ? 0.0 : radius_; p.k = k_; p.fma_dist = 0;
    d.check(mvr_cloud_pfh(d.ctx(), s.s, &p, output.points[0].histogram, nullptr, nullptr), "mvr_cloud_pfh");
    for (size_t i = 0; i < n && output.is_dense; ++i)
      if (std::isnan(output.points[i].histogram[0])) output.is_dense = false;
  }

 private:
  PointCloudConstPtr input_;
  PointCloudNConstPtr normals_;
  KdTreePtr tree_;
  double radius_ = 0.0;
  int k_ = 0;
  unsigned int cache_size_ = (1u << 31) - 1u;
  bool use_cache_ = false;
};

// ---------------------------------------------------------------- SHOT descriptors
// pcl::SHOTLocalReferenceFrameEstimation<PointInT, PointOutT> (features/shot_lrf.h), the input cloud its own search surface:
// setInputCloud, setSearchMethod, setRadiusSearch, compute.  Semantics: mvr_cloud_shot_lrf (rules L1-L7 in mvr_hip.h); a point
// with fewer than five other points within the radius gets nine NaN, and is_dense says so.
template <typename PointInT, typename PointOutT = ReferenceFrame>
class SHOTLocalReferenceFrameEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12, "points that begin with x, y, z expected");
    static_assert(sizeof(PointOutT) == sizeof(float) * 9, "a frame of nine floats expected");
    output.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::SHOTLocalReferenceFrameEstimation::compute] No input dataset was given!\n"); return; }
    if (!(std::isfinite(radius_) && radius_ > 0.0)) {
      std::fprintf(stderr, "[pcl::SHOTLocalReferenceFrameEstimation::compute] The search radius (%f) must be finite and > 0 (setRadiusSearch).\n", radius_);
      return;
    }
    const size_t n = input_->size();
    output.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    SlotGuard s;
    d.check(mvr_cloud_upload(d.ctx(), s.s, input_->points[0].data, n, sizeof(PointInT)), "mvr_cloud_upload");
    mvr_shot_params p;
    p.radius = radius_; p.lrf_radius = 0.0; p.fma_dist = 0;
    d.check(mvr_cloud_shot_lrf(d.ctx(), s.s, &p, output.points[0].rf, nullptr), "mvr_cloud_shot_lrf");
    for (size_t i = 0; i < n && output.is_dense; ++i)
      if (std::isnan(output.points[i].rf[0])) output.is_dense = false;
  }

 private:
  PointCloudConstPtr input_;
  KdTreePtr tree_;
  double radius_ = 0.0;
};

// pcl::SHOTEstimation<PointInT, PointNT, PointOutT, PointRFT> (features/shot.h): setInputCloud, setInputNormals (the normals of
// the search surface when one is set, as in PCL, else of the input), setSearchSurface, setIndices, setSearchMethod,
// setRadiusSearch, setLRFRadius (0, the default: the search radius), setInputReferenceFrames (one frame per output row; no frame
// is then computed), compute.  Semantics: mvr_cloud_shot / mvr_cloud_shot_at (rules L1-L7, H1-H9 and Q1-Q8 in mvr_hip.h) -- one
// call on the GPU per compute().  With indices the output holds one row per index; every row carries its frame in rf.
template <typename PointInT, typename PointNT, typename PointOutT = SHOT352, typename PointRFT = ReferenceFrame>
class SHOTEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointNT> PointCloudN;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef PointCloud<PointRFT> PointCloudRF;
  typedef typename PointCloudRF::ConstPtr PointCloudRFConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  void setInputNormals(const PointCloudNConstPtr &n) { normals_ = n; }
  void setSearchSurface(const PointCloudConstPtr &c) { surface_ = c; }
  void setIndices(const IndicesConstPtr &i) { indices_ = i; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setLRFRadius(float r) { lrf_radius_ = r; }
  float getLRFRadius() const { return lrf_radius_; }
  void setInputReferenceFrames(const PointCloudRFConstPtr &f) { frames_ = f; }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12, "points that begin with x, y, z expected");
    static_assert(sizeof(PointOutT) == sizeof(float) * (MVR_SHOT_DIM + 9) && sizeof(PointRFT) == sizeof(float) * 9, "SHOT352 and a frame of nine floats expected");
    output.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::SHOTEstimation::compute] No input dataset was given!\n"); return; }
    const PointCloudConstPtr &surface = surface_ ? surface_ : input_;
    if (!normals_ || normals_->size() != surface->size()) {
      std::fprintf(stderr, "[pcl::SHOTEstimation::compute] The number of points in the search surface differs from the number of points in the dataset containing the normals!\n");
      return;
    }
    if (!(std::isfinite(radius_) && radius_ > 0.0) || !(std::isfinite(lrf_radius_) && lrf_radius_ >= 0.f)) {
      std::fprintf(stderr, "[pcl::SHOTEstimation::compute] The search radius (%f) must be finite and > 0 (setRadiusSearch), the LRF radius (%f) finite and >= 0.\n",
                   radius_, (double)lrf_radius_);
      return;
    }
    std::vector<uint32_t> idx;
    if (indices_)
      for (int i : *indices_) {
        if (i < 0 || (size_t)i >= input_->size()) { std::fprintf(stderr, "[pcl::SHOTEstimation::compute] The index %d lies beyond the input cloud.\n", i); return; }
        idx.push_back((uint32_t)i);
      }
    const size_t rows = indices_ ? idx.size() : input_->size();
    if (frames_ && frames_->size() != rows) {
      std::fprintf(stderr, "[pcl::SHOTEstimation::compute] One input reference frame per output row expected (%zu for %zu)!\n", frames_->size(), rows);
      return;
    }
    output.resize(rows);
    if (!rows) return;
    Device &d = Device::instance();
    SlotGuard s;
    const size_t ns = surface->size();
    d.check(mvr_cloud_upload(d.ctx(), s.s, ns ? surface->points[0].data : nullptr, ns, sizeof(PointInT)), "mvr_cloud_upload");
    if (ns) {
      std::vector<float> nrm(4 * ns);
      for (size_t i = 0; i < ns; ++i) {
        const PointNT &q = normals_->points[i];
        nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
      }
      d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), ns, 16), "mvr_cloud_upload_normals");
    }
    std::shared_ptr<SlotGuard> q;
    if (surface_ && surface_ != input_) {
      q = std::make_shared<SlotGuard>();
      d.check(mvr_cloud_upload(d.ctx(), q->s, input_->points[0].data, input_->size(), sizeof(PointInT)), "mvr_cloud_upload");
    }
    mvr_shot_params p;
    p.radius = radius_; p.lrf_radius = (double)lrf_radius_; p.fma_dist = 0;
    std::vector<float> rowsf(rows * (size_t)MVR_SHOT_DIM), lrf(rows * 9);
    const float *fin = frames_ ? frames_->points[0].rf : nullptr;
    if (q || indices_)
      d.check(mvr_cloud_shot_at(d.ctx(), q ? q->s : s.s, indices_ ? idx.data() : nullptr, idx.size(), s.s, &p, fin, rowsf.data(), lrf.data(), nullptr, nullptr),
              "mvr_cloud_shot_at");
    else
      d.check(mvr_cloud_shot(d.ctx(), s.s, &p, fin, rowsf.data(), lrf.data(), nullptr, nullptr), "mvr_cloud_shot");
    for (size_t i = 0; i < rows; ++i) {
      std::memcpy(output.points[i].descriptor, rowsf.data() + i * MVR_SHOT_DIM, sizeof(float) * MVR_SHOT_DIM);
      std::memcpy(output.points[i].rf, lrf.data() + i * 9, sizeof(float) * 9);
      if (std::isnan(output.points[i].descriptor[0])) output.is_dense = false;
    }
  }

 private:
  PointCloudConstPtr input_, surface_;
  PointCloudNConstPtr normals_;
  PointCloudRFConstPtr frames_;
  IndicesConstPtr indices_;
  KdTreePtr tree_;
  double radius_ = 0.0;
  float lrf_radius_ = 0.f;
};

// the rows of a feature cloud as the contiguous table the matcher takes: `dim` floats per row.  A signature that is nothing but
// its histogram is the table already; pcl::SHOT352 carries its frame behind the descriptor and is packed.
template <typename FeatureT> struct FeatureRows {
  enum { dim = sizeof(FeatureT) / sizeof(float) };
  static const float *table(const std::vector<FeatureT> &f, std::vector<float> &) { return f.empty() ? nullptr : f[0].histogram; }
};
template <> struct FeatureRows<SHOT352> {
  enum { dim = MVR_SHOT_DIM };
  static const float *table(const std::vector<SHOT352> &f, std::vector<float> &packed)
  {
    packed.resize(f.size() * (size_t)MVR_SHOT_DIM);
    for (size_t i = 0; i < f.size(); ++i) std::memcpy(packed.data() + i * MVR_SHOT_DIM, f[i].descriptor, sizeof(float) * MVR_SHOT_DIM);
    return f.empty() ? nullptr : packed.data();
  }
};

// ---------------------------------------------------------------- boundary points
// pcl::BoundaryEstimation<PointInT, PointNT, PointOutT> (features/boundary.h) in radius mode, the input cloud its own search
// surface: setInputCloud, setInputNormals, setSearchMethod, setRadiusSearch, setAngleThreshold / getAngleThreshold (PCL's
// default pi / 2), compute.  Semantics: mvr_cloud_boundary (mvr_hip.h) with min_neighbors 0 -- one call on the GPU per compute().
// PointInT: any point whose first three floats are x, y, z; PointNT: any point with normal_x / y / z; PointOutT: any point
// with a boundary_point member.  As PCL's Feature::compute, a missing input, missing normals, a normal cloud of another size,
// a radius that is not finite and > 0 or an angle threshold outside [MVR_BOUNDARY_MIN_ANGLE, 2 pi) prints an error and leaves
// `output` empty, and so does a non-zero setKSearch: the k-neighbour mode is not offered.
template <typename PointInT, typename PointNT, typename PointOutT = Boundary>
class BoundaryEstimation {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudConstPtr;
  typedef PointCloud<PointNT> PointCloudN;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setInputNormals(const PointCloudNConstPtr &n) { normals_ = n; }
  PointCloudNConstPtr getInputNormals() const { return normals_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setRadiusSearch(double r) { radius_ = r; }
  double getRadiusSearch() const { return radius_; }
  void setKSearch(int k) { k_ = k; }
  int getKSearch() const { return k_; }
  void setAngleThreshold(float angle) { angle_threshold_ = angle; }
  float getAngleThreshold() const { return angle_threshold_; }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12, "points that begin with x, y, z expected");
    output.clear();
    if (!input_) { std::fprintf(stderr, "[pcl::BoundaryEstimation::compute] No input dataset was given!\n"); return; }
    if (!normals_ || normals_->size() != input_->size()) {
      std::fprintf(stderr, "[pcl::BoundaryEstimation::compute] The number of points in the input dataset differs from the number of points in the dataset containing the normals!\n");
      return;
    }
    if (k_ != 0) {
      std::fprintf(stderr, "[pcl::BoundaryEstimation::compute] The k-neighbour mode (setKSearch %d) is not offered: use setRadiusSearch.\n", k_);
      return;
    }
    if (!(std::isfinite(radius_) && radius_ > 0.0) || !(angle_threshold_ >= MVR_BOUNDARY_MIN_ANGLE && (double)angle_threshold_ < 2.0 * 3.14159265358979323846)) {
      std::fprintf(stderr, "[pcl::BoundaryEstimation::compute] The search radius (%f) must be finite and > 0 (setRadiusSearch), the angle threshold (%f) in [pi / 4, 2 pi).\n",
                   radius_, (double)angle_threshold_);
      return;
    }
    const size_t n = input_->size();
    output.resize(n);
    if (!n) return;
    Device &d = Device::instance();
    SlotGuard s;
    d.check(mvr_cloud_upload(d.ctx(), s.s, input_->points[0].data, n, sizeof(PointInT)), "mvr_cloud_upload");
    std::vector<float> nrm(4 * n);
    for (size_t i = 0; i < n; ++i) {
      const PointNT &q = normals_->points[i];
      nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
    }
    d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
    mvr_boundary_params p;
    p.radius = radius_; p.angle_threshold = angle_threshold_; p.min_neighbors = 0; p.fma_dist = 0;
    std::vector<uint8_t> flag(n);
    d.check(mvr_cloud_boundary(d.ctx(), s.s, &p, flag.data(), nullptr, nullptr), "mvr_cloud_boundary");
    for (size_t i = 0; i < n; ++i) output.points[i].boundary_point = flag[i];
  }

 private:
  PointCloudConstPtr input_;
  PointCloudNConstPtr normals_;
  KdTreePtr tree_;
  double radius_ = 0.0;
  int k_ = 0;
  float angle_threshold_ = 1.57079632679489661923f;
};

// ---------------------------------------------------------------- intrinsic shape signature keypoints
// pcl::ISSKeypoint3D<PointInT, PointOutT, NormalT> (keypoints/iss_3d.h): setInputCloud, setSearchMethod, setSalientRadius,
// setNonMaxRadius, setThreshold21, setThreshold32, setMinNeighbors, setNumberOfThreads, setBorderRadius, setNormalRadius,
// setNormals, setAngleThreshold, compute, getKeypointsIndices, PCL's defaults (both thresholds 0.975, 5 neighbours, angle
// threshold pi / 2, no border; the radii must be set).  Semantics: mvr_cloud_iss_keypoints_border (mvr_hip.h) -- one call on
// the GPU per compute().  PointInT / PointOutT: any point whose first three floats are x, y, z; NormalT: any point with
// normal_x / y / z.  `output` may be the input cloud itself.  With setBorderRadius > 0 the points that have a boundary point
// within that radius are dropped before the saliency test (rules K9-K11); the normals the boundary test needs are those of
// setNormals, or -- without them, with setNormalRadius > 0 -- those of the library's radius-mode normal estimation at that
// radius (mvr_cloud_estimate_normals; their sign does not matter to the test).  A missing input, a radius that is not finite
// and > 0, a non-finite threshold or a negative neighbour count prints an error and leaves the output empty (untouched when
// it is the input), and so do: a border radius with neither normals nor a normal radius; a normal cloud of another size than
// the input; and a normal radius with a zero border radius (DEVIATION: PCL ignores the radius there) -- computing something
// else in silence would be worse than computing nothing.
template <typename PointInT, typename PointOutT = PointInT, typename NormalT = Normal>
class ISSKeypoint3D {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudInConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef PointCloud<NormalT> PointCloudN;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef search::KdTree<PointInT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;

  void setInputCloud(const PointCloudInConstPtr &c) { input_ = c; }
  PointCloudInConstPtr getInputCloud() const { return input_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setSalientRadius(double r) { p_.salient_radius = r; }
  void setNonMaxRadius(double r) { p_.non_max_radius = r; }
  void setThreshold21(double g) { p_.gamma_21 = g; }
  void setThreshold32(double g) { p_.gamma_32 = g; }
  void setMinNeighbors(int m) { p_.min_neighbors = m; }
  void setNumberOfThreads(unsigned int = 0) {}
  void setBorderRadius(double r) { b_.border_radius = r; }
  void setNormalRadius(double r) { normal_radius_ = r; }
  void setNormals(const PointCloudNConstPtr &normals) { normals_ = normals; }
  void setAngleThreshold(float angle) { b_.angle_threshold = angle; }
  PointIndices::ConstPtr getKeypointsIndices() const { return indices_; }

  void compute(PointCloudOut &output)
  {
    static_assert(sizeof(PointInT) % 4 == 0 && sizeof(PointInT) >= 12 && sizeof(PointOutT) >= 12, "points that begin with x, y, z expected");
    indices_->indices.clear();
    const bool alias = (const void *)&output == (const void *)input_.get();
    if (!input_) { std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] No input dataset given!\n"); output.clear(); return; }
    if ((b_.border_radius != 0.0 && !normals_ && normal_radius_ == 0.0) || (b_.border_radius == 0.0 && normal_radius_ != 0.0)) {
      std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] The border estimation (setBorderRadius %f, setNormalRadius %f) needs a border radius and either setNormals or a normal radius.\n",
                   b_.border_radius, normal_radius_);
      if (!alias) output.clear();
      return;
    }
    const bool border = b_.border_radius != 0.0;
    if (border && normals_ && normals_->size() != input_->size()) {
      std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] The number of points in the input dataset differs from the number of points in the dataset containing the normals!\n");
      if (!alias) output.clear();
      return;
    }
    if (!(std::isfinite(p_.salient_radius) && p_.salient_radius > 0.0) || !(std::isfinite(p_.non_max_radius) && p_.non_max_radius > 0.0) ||
        !std::isfinite(p_.gamma_21) || !std::isfinite(p_.gamma_32) || p_.min_neighbors < 0) {
      std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] The salient radius (%f) and the non maxima radius (%f) must be finite and > 0, the thresholds (%f, %f) finite, the minimum number of neighbors (%d) >= 0.\n",
                   p_.salient_radius, p_.non_max_radius, p_.gamma_21, p_.gamma_32, p_.min_neighbors);
      if (!alias) output.clear();
      return;
    }
    if (border && (!(std::isfinite(b_.border_radius) && b_.border_radius > 0.0) || !(normals_ || (std::isfinite(normal_radius_) && normal_radius_ > 0.0)) ||
                   !(b_.angle_threshold >= MVR_BOUNDARY_MIN_ANGLE && b_.angle_threshold < 2.0 * 3.14159265358979323846))) {
      if (normals_)
        std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] The border radius (%f) must be finite and > 0, the angle threshold (%f) in [pi / 4, 2 pi).\n",
                     b_.border_radius, b_.angle_threshold);
      else
        std::fprintf(stderr, "[pcl::ISSKeypoint3D::compute] The border radius (%f) and, without setNormals, the normal radius (%f) must be finite and > 0, the angle threshold (%f) in [pi / 4, 2 pi).\n",
                     b_.border_radius, normal_radius_, b_.angle_threshold);
      if (!alias) output.clear();
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    const size_t n = input_->size();
    // first: `output` may alias the input
    d.check(mvr_cloud_upload(d.ctx(), s.s, n ? input_->points[0].data : nullptr, n, sizeof(PointInT)), "mvr_cloud_upload");
    if (border && n) {
      if (normals_) {
        std::vector<float> nrm(4 * n);
        for (size_t i = 0; i < n; ++i) {
          const NormalT &q = normals_->points[i];
          nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
        }
        d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
      } else {
        mvr_normal_params np;
        np.k = 0; np.radius = normal_radius_; np.fma_dist = 0;
        np.viewpoint[0] = np.viewpoint[1] = np.viewpoint[2] = 0.f;
        d.check(mvr_cloud_estimate_normals(d.ctx(), 1, &s.s, &np, nullptr), "mvr_cloud_estimate_normals");
      }
    }
    std::vector<uint32_t> kept(n ? n : 1);
    size_t m = 0;
    d.check(mvr_cloud_iss_keypoints_border(d.ctx(), s.s, s.s, &p_, border ? &b_ : nullptr, &m, kept.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
            "mvr_cloud_iss_keypoints_border");
    std::vector<float> xyz(4 * (m ? m : 1));
    size_t got = 0;
    if (m) d.check(mvr_cloud_download(d.ctx(), s.s, xyz.data(), m, 16, &got), "mvr_cloud_download");
    output.clear();
    output.resize(m);
    for (size_t i = 0; i < m; ++i) {
      PointOutT &o = output.points[i];
      o.x = xyz[4 * i]; o.y = xyz[4 * i + 1]; o.z = xyz[4 * i + 2];
    }
    indices_->indices.assign(kept.begin(), kept.begin() + (std::ptrdiff_t)m);
  }

 private:
  PointCloudInConstPtr input_;
  PointCloudNConstPtr normals_;
  KdTreePtr tree_;
  mvr_iss_params p_ = {0.0, 0.0, 0.975, 0.975, 5, 0};
  mvr_iss_border_params b_ = {0.0, 1.57079632679489661923};
  double normal_radius_ = 0.0;
  PointIndicesPtr indices_ = std::make_shared<PointIndices>();
};

// ---------------------------------------------------------------- plane segmentation
// pcl::SACSegmentation<PointT> (segmentation/sac_segmentation.h) for SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE with
// SAC_RANSAC: setInputCloud, setModelType, setMethodType, setDistanceThreshold, setMaxIterations, setProbability,
// setOptimizeCoefficients, setAxis, setEpsAngle, segment, with PCL's defaults (50 iterations, probability 0.99, coefficients
// optimised; the model and the threshold must be set).  Semantics: mvr_cloud_segment_plane (mvr_hip.h) -- one call on the GPU per
// segment().  PCL draws with rand(); here the result is a pure function of the input and of setSeed (ours).  Any other model
// or method throws mvr::Error at the setter: computing something else in silence would be worse.  As PCL, a missing input, a
// parameter outside its range or a cloud without a plane prints an error and leaves indices and coefficients empty.
template <typename PointT>
class SACSegmentation {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;

  explicit SACSegmentation(bool /*random*/ = false) {}
  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setModelType(int model)
  {
    if (model != SACMODEL_PLANE && model != SACMODEL_PERPENDICULAR_PLANE)
      throw Error(MVR_E_ARG, "pcl::SACSegmentation::setModelType: only SACMODEL_PLANE and SACMODEL_PERPENDICULAR_PLANE are offered");
    model_ = model;
  }
  int getModelType() const { return model_; }
  void setMethodType(int method)
  {
    if (method != SAC_RANSAC) throw Error(MVR_E_ARG, "pcl::SACSegmentation::setMethodType: only SAC_RANSAC is offered");
  }
  int getMethodType() const { return SAC_RANSAC; }
  void setDistanceThreshold(double t) { p_.threshold = t; }
  double getDistanceThreshold() const { return p_.threshold; }
  void setMaxIterations(int n) { p_.max_iterations = n; }
  int getMaxIterations() const { return p_.max_iterations; }
  void setProbability(double pr) { p_.probability = pr; }
  double getProbability() const { return p_.probability; }
  void setOptimizeCoefficients(bool o) { p_.optimize = o ? 1 : 0; }
  bool getOptimizeCoefficients() const { return p_.optimize != 0; }
  void setAxis(float x, float y, float z) { p_.axis[0] = x; p_.axis[1] = y; p_.axis[2] = z; }
  template <class V> void setAxis(const V &ax) { setAxis((float)ax[0], (float)ax[1], (float)ax[2]); }      // (an Eigen::Vector3f, an array)
  void setEpsAngle(double ea) { p_.eps_angle = ea; }
  double getEpsAngle() const { return p_.eps_angle; }
  void setSeed(uint64_t seed) { p_.seed = seed; }
  const mvr_sac_result &getResult() const { return result_; }      // ours: iterations, attempts, the RANSAC plane before the refinement

  void segment(PointIndices &inliers, ModelCoefficients &model_coefficients)
  {
    static_assert(sizeof(PointT) % 4 == 0 && sizeof(PointT) >= 12, "points that begin with x, y, z expected");
    inliers.indices.clear();
    model_coefficients.values.clear();
    result_ = mvr_sac_result();
    if (!input_) { std::fprintf(stderr, "[pcl::SACSegmentation::segment] No input dataset given!\n"); return; }
    if (model_ < 0) { std::fprintf(stderr, "[pcl::SACSegmentation::initSACModel] No valid model given!\n"); return; }
    mvr_sac_params p = p_;
    p.model = model_ == SACMODEL_PLANE ? 0 : 1;
    const double *a = p.axis;
    const bool axis_ok = std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && (a[0] != 0.0 || a[1] != 0.0 || a[2] != 0.0);
    if (!(std::isfinite(p.threshold) && p.threshold > 0.0) || p.max_iterations < 1 || p.max_iterations > (1 << 24) ||
        !(p.probability > 0.0 && p.probability < 1.0) || (p.model == 1 && (!axis_ok || !(p.eps_angle > 0.0 && p.eps_angle <= 1.57079632679489661923)))) {
      std::fprintf(stderr, "[pcl::SACSegmentation::segment] The distance threshold (%f) must be finite and > 0, the iterations (%d) in 1..2^24, the probability (%f) in (0, 1); the perpendicular model needs an axis and an angle (%f) in (0, pi / 2].\n",
                   p.threshold, p.max_iterations, p.probability, p.eps_angle);
      return;
    }
    Device &d = Device::instance();
    SlotGuard s;
    const size_t n = input_->size();
    d.check(mvr_cloud_upload(d.ctx(), s.s, n ? input_->points[0].data : nullptr, n, sizeof(PointT)), "mvr_cloud_upload");
    std::vector<uint32_t> index(n ? n : 1);
    d.check(mvr_cloud_segment_plane(d.ctx(), -1, s.s, &p, &result_, nullptr, index.data(), nullptr, nullptr, 0), "mvr_cloud_segment_plane");
    if (!result_.found || result_.inliers == 0) {
      std::fprintf(stderr, "[pcl::SACSegmentation::segment] Error segmenting the model! No solution found.\n");
      return;
    }
    inliers.indices.assign(index.begin(), index.begin() + (std::ptrdiff_t)result_.inliers);
    model_coefficients.values.assign(result_.coefficients, result_.coefficients + 4);
  }

 private:
  PointCloudConstPtr input_;
  int model_ = -1;
  mvr_sac_params p_ = {0, 0.0, 50, 0.99, 1, {0.0, 0.0, 0.0}, 0.0, 0, 0, 0};
  mvr_sac_result result_ = mvr_sac_result();
};

// pcl::ExtractIndices<PointT> (filters/extract_indices.h): setInputCloud, setIndices, setNegative, filter.  One call of
// mvr_cloud_extract_indices per filter(): the listed points -- or with setNegative(true) all the others -- in ascending index.
// `output` may be the input cloud itself.  A missing input or index list, or an index outside the cloud, prints an error and
// leaves the output empty (untouched when it is the input).
template <typename PointT>
class ExtractIndices {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setIndices(const PointIndices::ConstPtr &i) { indices_ = i ? std::make_shared<const std::vector<int> >(i->indices) : IndicesConstPtr(); }
  void setIndices(const PointIndices::Ptr &i) { setIndices(PointIndices::ConstPtr(i)); }
  void setIndices(const IndicesConstPtr &i) { indices_ = i; }
  IndicesConstPtr getIndices() const { return indices_; }
  void setNegative(bool negative) { negative_ = negative; }
  bool getNegative() const { return negative_; }

  void filter(PointCloudT &output)
  {
    static_assert(sizeof(PointT) == 16, "16-byte XYZ points expected");
    const bool alias = (const void *)&output == (const void *)input_.get();
    if (!input_ || !indices_) {
      std::fprintf(stderr, "[pcl::ExtractIndices::filter] No input dataset or no indices given!\n");
      if (!alias) output.clear();
      return;
    }
    const size_t n = input_->size();
    std::vector<uint32_t> index(indices_->size() ? indices_->size() : 1);
    for (size_t k = 0; k < indices_->size(); ++k) {
      const int i = (*indices_)[k];
      if (i < 0 || (size_t)i >= n) {
        std::fprintf(stderr, "[pcl::ExtractIndices::filter] The index %d is outside the input dataset of %zu points!\n", i, n);
        if (!alias) output.clear();
        return;
      }
      index[k] = (uint32_t)i;
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.upload(s.s, *input_);              // first: `output` may alias the input
    size_t m = 0;
    d.check(mvr_cloud_extract_indices(d.ctx(), s.s, s.s, index.data(), indices_->size(), negative_ ? 1 : 0, &m), "mvr_cloud_extract_indices");
    d.download(s.s, output);
  }

 private:
  PointCloudConstPtr input_;
  IndicesConstPtr indices_;
  bool negative_ = false;
};

// ---------------------------------------------------------------- Euclidean cluster extraction
namespace detail {
// one call of mvr_cloud_euclidean_clusters on an uploaded slot -> PCL's vector of PointIndices (largest cluster first, members
// ascending); index null: every point
inline void clusters_of_slot(Device &d, int slot, size_t n, const mvr_cluster_params &p, const std::vector<uint32_t> *index,
                             std::vector<PointIndices> &clusters, mvr_cluster_result &result)
{
  std::vector<uint32_t> offset(n + 2), member(n ? n : 1);
  const uint32_t none = 0;
  const uint32_t *idx = index ? (index->empty() ? &none : index->data()) : nullptr;
  d.check(mvr_cloud_euclidean_clusters(d.ctx(), -1, slot, &p, idx, index ? index->size() : 0, &result, nullptr, offset.data(), offset.size(),
                                       member.data(), nullptr), "mvr_cloud_euclidean_clusters");
  clusters.resize(result.n_clusters);
  for (uint32_t c = 0; c < result.n_clusters; ++c) clusters[c].indices.assign(member.begin() + offset[c], member.begin() + offset[c + 1]);
}
}  // namespace detail

// pcl::EuclideanClusterExtraction<PointT> (segmentation/extract_clusters.h): setClusterTolerance, setMinClusterSize,
// setMaxClusterSize, setSearchMethod (accepted and unused), setInputCloud, setIndices, extract, with PCL's defaults (min 1, max
// INT_MAX; the tolerance must be set).  Semantics: mvr_cloud_euclidean_clusters (mvr_hip.h, rules E1-E8) -- one call on the
// GPU per extract(): the clusters largest first, members in ascending index; two points link at d2 <= tolerance^2 (FLANN's
// radius search is strict).  As PCL, a missing input, a tolerance that is not finite and > 0 or an index outside the cloud
// prints an error and leaves `clusters` empty.
template <typename PointT>
class EuclideanClusterExtraction {
 public:
  typedef PointCloud<PointT> PointCloudT;
  typedef typename PointCloudT::ConstPtr PointCloudConstPtr;
  typedef search::KdTree<PointT> KdTree;
  typedef typename KdTree::Ptr KdTreePtr;
  typedef std::shared_ptr<const std::vector<int> > IndicesConstPtr;

  void setInputCloud(const PointCloudConstPtr &c) { input_ = c; }
  PointCloudConstPtr getInputCloud() const { return input_; }
  void setIndices(const PointIndices::ConstPtr &i) { indices_ = i ? std::make_shared<const std::vector<int> >(i->indices) : IndicesConstPtr(); }
  void setIndices(const PointIndices::Ptr &i) { setIndices(PointIndices::ConstPtr(i)); }
  void setIndices(const IndicesConstPtr &i) { indices_ = i; }
  IndicesConstPtr getIndices() const { return indices_; }
  void setSearchMethod(const KdTreePtr &tree) { tree_ = tree; }
  KdTreePtr getSearchMethod() const { return tree_; }
  void setClusterTolerance(double tolerance) { p_.tolerance = tolerance; }
  double getClusterTolerance() const { return p_.tolerance; }
  void setMinClusterSize(int n) { p_.min_size = n > 0 ? (uint32_t)n : 0u; }
  int getMinClusterSize() const { return (int)p_.min_size; }
  void setMaxClusterSize(int n) { p_.max_size = n > 0 ? (uint32_t)n : 0u; }
  int getMaxClusterSize() const { return (int)p_.max_size; }
  const mvr_cluster_result &getResult() const { return result_; }      // ours: components, the ones too small and too large

  void extract(std::vector<PointIndices> &clusters)
  {
    static_assert(sizeof(PointT) % 4 == 0 && sizeof(PointT) >= 12, "points that begin with x, y, z expected");
    clusters.clear();
    result_ = mvr_cluster_result();
    if (!input_) { std::fprintf(stderr, "[pcl::EuclideanClusterExtraction::extract] No input dataset given!\n"); return; }
    if (!(std::isfinite(p_.tolerance) && p_.tolerance > 0.0)) {
      std::fprintf(stderr, "[pcl::EuclideanClusterExtraction::extract] The cluster tolerance (%f) must be finite and > 0.\n", p_.tolerance);
      return;
    }
    const size_t n = input_->size();
    std::vector<uint32_t> index;
    if (indices_) {
      index.reserve(indices_->size());
      for (const int i : *indices_) {
        if (i < 0 || (size_t)i >= n) {
          std::fprintf(stderr, "[pcl::EuclideanClusterExtraction::extract] The index %d is outside the input dataset of %zu points!\n", i, n);
          return;
        }
        index.push_back((uint32_t)i);
      }
    }
    Device &d = Device::instance();
    SlotGuard s;
    d.check(mvr_cloud_upload(d.ctx(), s.s, n ? input_->points[0].data : nullptr, n, sizeof(PointT)), "mvr_cloud_upload");
    detail::clusters_of_slot(d, s.s, n, p_, indices_ ? &index : nullptr, clusters, result_);
  }

 private:
  PointCloudConstPtr input_;
  IndicesConstPtr indices_;
  KdTreePtr tree_;
  mvr_cluster_params p_ = {0.0, 1u, 0x7FFFFFFFu, 0, 0.0, 0, 1u, 0};
  mvr_cluster_result result_ = mvr_cluster_result();
};

// pcl::extractEuclideanClusters(cloud, normals, tolerance, tree, clusters, eps_angle, min_pts, max_pts)
// (segmentation/extract_clusters.h): two points link when they are within the tolerance AND their normals are less than
// eps_angle apart (rule E3).  The tree is accepted and unused.  As PCL, clouds of different sizes print an error and leave
// `clusters` empty; so do a tolerance or an angle outside their ranges ((0, inf), (0, pi]).
template <typename PointT, typename NormalT>
void extractEuclideanClusters(const PointCloud<PointT> &cloud, const PointCloud<NormalT> &normals, float tolerance,
                              const typename search::KdTree<PointT>::Ptr & /*tree*/, std::vector<PointIndices> &clusters, double eps_angle,
                              unsigned int min_pts_per_cluster = 1, unsigned int max_pts_per_cluster = 0x7FFFFFFFu)
{
  static_assert(sizeof(PointT) % 4 == 0 && sizeof(PointT) >= 12, "points that begin with x, y, z expected");
  clusters.clear();
  const size_t n = cloud.size();
  if (normals.size() != n) {
    std::fprintf(stderr, "[pcl::extractEuclideanClusters] Number of points in the input point cloud (%zu) different than normals (%zu)!\n", n, normals.size());
    return;
  }
  if (!(std::isfinite(tolerance) && tolerance > 0.f) || !(eps_angle > 0.0 && eps_angle <= 3.14159265358979323846)) {
    std::fprintf(stderr, "[pcl::extractEuclideanClusters] The tolerance (%f) must be finite and > 0, the angle (%f) in (0, pi].\n", (double)tolerance, eps_angle);
    return;
  }
  if (!n) return;
  Device &d = Device::instance();
  SlotGuard s;
  std::vector<float> xyz(4 * n), nrm(4 * n);
  for (size_t i = 0; i < n; ++i) {
    const PointT &v = cloud.points[i];
    xyz[4 * i] = v.x; xyz[4 * i + 1] = v.y; xyz[4 * i + 2] = v.z; xyz[4 * i + 3] = 1.f;
  }
  d.check(mvr_cloud_upload(d.ctx(), s.s, xyz.data(), n, 16), "mvr_cloud_upload");
  for (size_t i = 0; i < n; ++i) {
    const NormalT &q = normals.points[i];
    nrm[4 * i] = q.normal_x; nrm[4 * i + 1] = q.normal_y; nrm[4 * i + 2] = q.normal_z; nrm[4 * i + 3] = 0.f;
  }
  d.check(mvr_cloud_upload_normals(d.ctx(), s.s, nrm.data(), n, 16), "mvr_cloud_upload_normals");
  mvr_cluster_params p = {(double)tolerance, min_pts_per_cluster, max_pts_per_cluster, 1, eps_angle, 0, 1u, 0};
  mvr_cluster_result result;
  detail::clusters_of_slot(d, s.s, n, p, nullptr, clusters, result);
}
// a PointNormal cloud carries its own normals
template <typename PointT>
typename std::enable_if<detail::has_normal<PointT>::value>::type
extractEuclideanClusters(const PointCloud<PointT> &cloud, float tolerance, const typename search::KdTree<PointT>::Ptr &tree,
                         std::vector<PointIndices> &clusters, double eps_angle, unsigned int min_pts_per_cluster = 1,
                         unsigned int max_pts_per_cluster = 0x7FFFFFFFu)
{
  extractEuclideanClusters(cloud, cloud, tolerance, tree, clusters, eps_angle, min_pts_per_cluster, max_pts_per_cluster);
}

// ---------------------------------------------------------------- sample-consensus alignment
// pcl::SampleConsensusPrerejective<PointSource, PointTarget, FeatureT> (registration/sample_consensus_prerejective.h):
// setInputSource, setInputTarget, setSourceFeatures, setTargetFeatures, setMaximumIterations, setNumberOfSamples,
// setCorrespondenceRandomness, setSimilarityThreshold, setMaxCorrespondenceDistance, setInlierFraction, align, hasConverged,
// getFinalTransformation, getFitnessScore, getInliers.  Semantics: mvr_align_prerejective_dim (mvr_hip.h) -- one call per align();
// FeatureT is a signature of 33 floats (FPFHSignature33), of 125 (PFHSignature125) or pcl::SHOT352 (352; FeatureRows above).
// PCL draws with rand(); here the result is a pure function of the inputs and of setSeed (ours).  Defaults are PCL's (3
// samples, randomness 2, similarity 0.9, inlier fraction 0); an inlier fraction of 0 -- which the C-ABI refuses -- is sent as
// the smallest positive double, the same test.  As PCL, a missing cloud or feature set, or a feature set of another size than
// its cloud, prints an error and leaves `output` empty and hasConverged() false.  getInliers() lists, ascending, the source
// points within the correspondence distance of the target under the final pose (one call of mvr_nn).
template <typename PointSource, typename PointTarget, typename FeatureT = FPFHSignature33>
class SampleConsensusPrerejective {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef typename PointCloudSource::Ptr PointCloudSourcePtr;
  typedef typename PointCloudTarget::Ptr PointCloudTargetPtr;
  typedef PointCloud<FeatureT> FeatureCloud;
  typedef typename FeatureCloud::ConstPtr FeatureCloudConstPtr;
  typedef Matrix4f Matrix4;

  SampleConsensusPrerejective()
  {
    p_ = mvr_prerej_params();
    p_.max_iterations = 10; p_.nr_samples = 3; p_.k = 2; p_.similarity = 0.9; p_.max_dist = std::sqrt(DBL_MAX); p_.inlier_fraction = 0.0;
  }
  void setInputSource(const PointCloudSourcePtr &c) { input_ = c; }
  void setInputTarget(const PointCloudTargetPtr &c) { target_ = c; }
  void setSourceFeatures(const FeatureCloudConstPtr &f) { sfeat_ = f; }
  void setTargetFeatures(const FeatureCloudConstPtr &f) { tfeat_ = f; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  int getMaximumIterations() const { return p_.max_iterations; }
  void setNumberOfSamples(int n) { p_.nr_samples = n; }
  int getNumberOfSamples() const { return p_.nr_samples; }
  void setCorrespondenceRandomness(int k) { p_.k = k; }
  int getCorrespondenceRandomness() const { return p_.k; }
  void setSimilarityThreshold(float s) { p_.similarity = s; }
  float getSimilarityThreshold() const { return (float)p_.similarity; }
  void setMaxCorrespondenceDistance(double d) { p_.max_dist = d; }
  double getMaxCorrespondenceDistance() const { return p_.max_dist; }
  void setInlierFraction(float f) { p_.inlier_fraction = f; }
  float getInlierFraction() const { return (float)p_.inlier_fraction; }
  void setSeed(uint64_t seed) { p_.seed = seed; }
  uint64_t getSeed() const { return p_.seed; }

  void align(PointCloudSource &output) { align(output, Matrix4::Identity(), false); }
  void align(PointCloudSource &output, const Matrix4 &guess) { align(output, guess, true); }

  bool hasConverged() const { return result_.converged != 0; }
  Matrix4 getFinalTransformation() const { return final_; }
  const mvr_prerej_result &getResult() const { return result_; }
  // the mean squared distance of the inliers of the final pose (PCL's getFitness; DBL_MAX without a pose)
  double getFitnessScore() const { return result_.error; }
  const std::vector<int> &getInliers() const { return inliers_; }

 private:
  void align(PointCloudSource &output, const Matrix4 &guess, bool with_guess)
  {
    static_assert(FeatureRows<FeatureT>::dim == 3 * MVR_FPFH_BINS || FeatureRows<FeatureT>::dim == MVR_PFH_DIM || FeatureRows<FeatureT>::dim == MVR_SHOT_DIM,
                  "a 33-float or a 125-float signature, or SHOT352, expected");
    output.clear(); inliers_.clear();
    result_ = mvr_prerej_result(); result_.best_iteration = -1; result_.error = DBL_MAX;
    final_ = with_guess ? guess : Matrix4::Identity();
    if (!input_ || !target_) { std::fprintf(stderr, "[pcl::SampleConsensusPrerejective::align] No input source or target was given!\n"); return; }
    if (!sfeat_ || !tfeat_ || sfeat_->size() != input_->size() || tfeat_->size() != target_->size()) {
      std::fprintf(stderr, "[pcl::SampleConsensusPrerejective::align] The source and target features must be set, one per point of their cloud!\n");
      return;
    }
    Device &d = Device::instance();
    d.upload(src_.s, *input_);
    d.upload(tgt_.s, *target_);
    mvr_prerej_params p = p_;
    if (p.inlier_fraction == 0.0) p.inlier_fraction = DBL_MIN;
    static const float none[MVR_SHOT_DIM] = {0};
    std::vector<float> spack, tpack;
    const float *sp = FeatureRows<FeatureT>::table(sfeat_->points, spack), *tp = FeatureRows<FeatureT>::table(tfeat_->points, tpack);
    d.check(mvr_align_prerejective_dim(d.ctx(), src_.s, tgt_.s, sp ? sp : none, tp ? tp : none, (int)FeatureRows<FeatureT>::dim, &p,
                                       with_guess ? guess.data() : nullptr, &result_, nullptr),
            "mvr_align_prerejective_dim");
    final_ = Matrix4(result_.T);
    d.check(mvr_cloud_transform_f32(d.ctx(), out_.s, src_.s, result_.T), "mvr_cloud_transform_f32");
    d.download(out_.s, output);
    if (result_.converged && !input_->empty()) {
      std::vector<float> d2(input_->size());
      d.check(mvr_nn(d.ctx(), out_.s, tgt_.s, p.fma_dist, nullptr, d2.data()), "mvr_nn");
      for (size_t i = 0; i < d2.size(); ++i) if ((double)d2[i] < p.max_dist * p.max_dist) inliers_.push_back((int)i);
    }
  }

  mvr_prerej_params p_;
  mvr_prerej_result result_ = mvr_prerej_result();
  PointCloudSourcePtr input_;
  PointCloudTargetPtr target_;
  FeatureCloudConstPtr sfeat_, tfeat_;
  Matrix4 final_;
  std::vector<int> inliers_;
  SlotGuard src_, tgt_, out_;
};

namespace registration {

// ------------------------------------------------- CorrespondenceEstimation
template <typename PointSource, typename PointTarget, typename Scalar = float>
class CorrespondenceEstimation {
 public:
  typedef typename PointCloud<PointSource>::Ptr PointCloudSourcePtr;
  typedef typename PointCloud<PointTarget>::Ptr PointCloudTargetPtr;
  void setInputSource(const PointCloudSourcePtr &c) { input_ = c; }
  void setInputTarget(const PointCloudTargetPtr &c) { target_ = c; }

  void determineReciprocalCorrespondences(Correspondences &out, double max_distance = DBL_MAX) { run(out, max_distance, 1); }
  void determineCorrespondences(Correspondences &out, double max_distance = DBL_MAX) { run(out, max_distance, 0); }

 private:
  void run(Correspondences &out, double max_distance, int reciprocal)
  {
    out.clear();
    if (!input_ || !target_ || input_->empty()) return;
    Device &d = Device::instance();
    d.upload(src_.s, *input_);
    d.upload(tgt_.s, *target_);
    const size_t ns = input_->size();
    std::vector<int32_t> q(ns), m(ns);
    std::vector<float> dd(ns);
    size_t n = 0;
    // sqrt(DBL_MAX)^2 == DBL_MAX: an unbounded search, as PCL's default
    const double md = std::min(max_distance, std::sqrt(DBL_MAX));
    d.check(mvr_correspondences(d.ctx(), src_.s, tgt_.s, md, reciprocal, 0, q.data(), m.data(), dd.data(), ns, &n),
            "mvr_correspondences");
    out.resize(n);
    for (size_t k = 0; k < n; ++k) out[k] = Correspondence(q[k], m[k], dd[k]);
  }
  PointCloudSourcePtr input_;
  PointCloudTargetPtr target_;
  SlotGuard src_, tgt_;
};

// ---------------------------------------------------------------------- LUM
template <typename PointT>
class LUM {
 public:
  typedef PointCloud<PointT> Cloud;
  typedef typename Cloud::Ptr PointCloudPtr;
  typedef size_t Vertex;

  size_t getNumVertices() const { return clouds_.size(); }
  void setMaxIterations(int n) { max_iterations_ = n; }
  int getMaxIterations() const { return max_iterations_; }
  void setConvergenceThreshold(float t) { threshold_ = t; }
  float getConvergenceThreshold() const { return threshold_; }

  Vertex addPointCloud(const PointCloudPtr &cloud, const Vector6f &pose = Vector6f())
  {
    clouds_.push_back(cloud);
    for (int k = 0; k < 6; ++k) poses_.push_back(clouds_.size() == 1 ? 0.0 : (double)pose(k));   // vertex 0 is the reference
    return clouds_.size() - 1;
  }
  PointCloudPtr getPointCloud(Vertex v) const { return v < clouds_.size() ? clouds_[v] : PointCloudPtr(); }
  void setCorrespondences(Vertex s, Vertex t, const CorrespondencesPtr &corrs)
  {
    if (s >= clouds_.size() || t >= clouds_.size() || s == t) {
      std::fprintf(stderr, "[mvr::registration::LUM::setCorrespondences] invalid vertices\n");
      return;
    }
    for (Edge &e : edges_) if (e.s == (int)s && e.t == (int)t) { e.corrs = corrs; return; }
    edges_.push_back(Edge{(int)s, (int)t, corrs});
  }
  CorrespondencesPtr getCorrespondences(Vertex s, Vertex t) const
  {
    for (const Edge &e : edges_) if (e.s == (int)s && e.t == (int)t) return e.corrs;
    return CorrespondencesPtr();
  }
  Vector6f getPose(Vertex v) const { Vector6f p; for (int k = 0; k < 6; ++k) p(k) = (float)poses_[6 * v + k]; return p; }

  // LUM::compute.  One GPU pass per edge reduces its
  // correspondences to raw second moments; the max_iterations_ linearised
  // solves then run on the host from those moments.
  void compute()
  {
    const int n = (int)clouds_.size();
    if (n < 2) { std::fprintf(stderr, "[mvr::registration::LUM::compute] The slam graph needs at least 2 vertices.\n"); return; }
    Device &d = Device::instance();
    std::vector<SlotGuard> slots(n);
    double origin[3] = {0, 0, 0};
    for (int v = 0; v < n; ++v) d.upload(slots[v].s, *clouds_[v]);
    if (!clouds_[0]->empty()) { const PointT &p = clouds_[0]->points[0]; origin[0] = p.x; origin[1] = p.y; origin[2] = p.z; }
    std::vector<mvr_pair_moments2_t> m2(edges_.size());
    std::vector<int> es(edges_.size()), et(edges_.size());
    for (size_t e = 0; e < edges_.size(); ++e) {
      const Correspondences &c = *edges_[e].corrs;
      std::vector<int32_t> q(c.size()), m(c.size());
      for (size_t k = 0; k < c.size(); ++k) { q[k] = c[k].index_query; m[k] = c[k].index_match; }
      es[e] = edges_[e].s; et[e] = edges_[e].t;
      d.check(mvr_pair_moments2_from_corr(d.ctx(), slots[es[e]].s, slots[et[e]].s, q.data(), m.data(), c.size(), origin, &m2[e]),
              "mvr_pair_moments2_from_corr");
    }
    int iters = 0;
    const int rc = mvr_lum_compute(n, (int)edges_.size(), es.data(), et.data(), m2.data(), max_iterations_,
                                   (double)threshold_, poses_.data(), &iters);
    if (rc != MVR_OK) std::fprintf(stderr, "[mvr::registration::LUM::compute] %s\n", mvr_strerror(rc));
  }

  Affine3f getTransformation(Vertex v) const
  {
    double T[16];
    mvr_pose_to_mat4(&poses_[6 * v], T);
    Affine3f a;
    for (int k = 0; k < 16; ++k) a.mat.m[k] = (float)T[k];
    return a;
  }

 private:
  struct Edge { int s, t; CorrespondencesPtr corrs; };
  std::vector<PointCloudPtr> clouds_;
  std::vector<double> poses_;
  std::vector<Edge> edges_;
  int max_iterations_ = 5;      // PCL default; the reference sets 16 (registrator.cpp:623,653)
  float threshold_ = 0.0f;
};

}  // namespace registration
}  // namespace mvr

#ifdef MVR_ALIAS_PCL
namespace pcl = mvr;   // lets `pcl::IterativeClosestPoint<...>` etc. resolve to the shim
#endif
