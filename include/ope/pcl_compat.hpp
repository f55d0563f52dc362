// pcl_compat.hpp — header-only C++ façade over the C ABI (include/ope.h) that re-creates the PCL call
// shapes the reference consumes, so that DetectAndLocalize/src/poseestimator.cpp and
// BuildModel/src/regmeshpcd.cpp can be re-pointed with a namespace alias:
//
//     namespace pcl = ope::compat;          // instead of #include <pcl/...>
//
// Mirrored interfaces (names, argument meaning and error behaviour follow the reference):
//   Registration / IterativeClosestPoint[WithNormals]   vPCL registration_mod.h:151-479, icp_mod.h:165-281
//   registration::CorrespondenceEstimationNormalShooting poseestimator.cpp:242-246
//   registration::CorrespondenceRejectorSurfaceNormal    poseestimator.cpp:264-272
//   registration::CorrespondenceRejectorSelfOccludedNormal vPCL correspondence_rejection_self_occluded_normal.h
//   registration::TransformationEstimationSVD            poseestimator.cpp:306,435
//   registration::TransformationEstimationPointToPlane[LLS] BuildModel regmeshpcd.cpp:162,193; vPCL icp_mod.h:355
//   NormalEstimation / FPFHEstimation / UniformSampling  poseestimator.cpp:121-125,141-156
//   removeNaNFromPointCloud / PassThrough / VoxelGrid    poseestimator.cpp:192-194; BuildModel processingpcd.cpp:8-52
//   SampleConsensusInitialAlignment                      poseestimator.cpp:50-64
//   SampleConsensusPrerejective                          BuildModel poseestimator.cpp:90-108 (commented out there)
//   registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33>
//   registration::CorrespondenceRejectorSampleConsensus  BuildModel poseestimator.cpp:43-60 (commented out there)
//   registration::CorrespondenceRejectorMedianDistance / OneToOne / VarTrimmed   poseestimator.cpp:250-292 (commented out there)
// Point types are layout-compatible PODs (x@0,y@4,z@8; normal@16 in PointXYZRGBNormal; 16-byte aligned).
// Errors never throw on the hot path: like PCL, a failed call logs to stderr and leaves
// hasConverged() == false / the transform at identity (registration_mod.hpp:60-64,73-77).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <memory>
#include <string>
#include <vector>

#include "../ope.h"

namespace ope {
namespace compat {

// ------------------------------------------------------------------------------------------ PODs
struct alignas(16) PointXYZ { float x, y, z, data3 = 1.f; };
struct alignas(16) Normal { float normal_x, normal_y, normal_z, data_n3 = 0.f; float curvature = 0.f, pad_[3] = {0, 0, 0}; };
struct alignas(16) PointXYZRGB { float x, y, z, data3 = 1.f; float rgb = 0.f, pad_[3] = {0, 0, 0}; };
struct alignas(16) PointXYZRGBNormal {
  float x, y, z, data3 = 1.f;
  float normal_x = 0.f, normal_y = 0.f, normal_z = 0.f, data_n3 = 0.f;
  float rgb = 0.f, curvature = 0.f, pad_[2] = {0, 0};
};
struct FPFHSignature33 { float histogram[33]; };
struct VFHSignature308 { float histogram[308]; };
struct Correspondence { int index_query = 0; int index_match = -1; float distance = FLT_MAX; };
typedef std::vector<Correspondence> Correspondences;
static_assert(sizeof(PointXYZ) == 16 && sizeof(Normal) == 32 && sizeof(PointXYZRGB) == 32 &&
              sizeof(PointXYZRGBNormal) == 48 && sizeof(FPFHSignature33) == 132 && sizeof(Correspondence) == 12,
              "PCL layouts");

template <class T> struct point_traits { static constexpr ptrdiff_t normal_offset = -1; static constexpr ptrdiff_t rgb_offset = -1; };
template <> struct point_traits<PointXYZRGB> { static constexpr ptrdiff_t normal_offset = -1; static constexpr ptrdiff_t rgb_offset = 16; };
template <> struct point_traits<PointXYZRGBNormal> { static constexpr ptrdiff_t normal_offset = 16; static constexpr ptrdiff_t rgb_offset = 32; };
template <> struct point_traits<Normal> { static constexpr ptrdiff_t normal_offset = 0; static constexpr ptrdiff_t rgb_offset = -1; };

template <class PointT> struct PointCloud {
  typedef std::shared_ptr<PointCloud<PointT>> Ptr;
  typedef std::shared_ptr<const PointCloud<PointT>> ConstPtr;
  std::vector<PointT> points;
  uint32_t width = 0, height = 1;
  bool is_dense = true;
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void clear() { points.clear(); width = 0; height = 1; }
  void resize(size_t n) { points.resize(n); width = (uint32_t)n; height = 1; }
  void push_back(const PointT &p) { points.push_back(p); width = (uint32_t)points.size(); height = 1; }
  PointT &operator[](size_t i) { return points[i]; }
  const PointT &operator[](size_t i) const { return points[i]; }
};

// Column-major 4x4, the memory layout of Eigen::Matrix4f.
struct Matrix4f {
  float m[16];
  static Matrix4f Identity() { Matrix4f r; std::memset(r.m, 0, sizeof r.m); r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.f; return r; }
  float &operator()(int r, int c) { return m[4 * c + r]; }
  float operator()(int r, int c) const { return m[4 * c + r]; }
  Matrix4f operator*(const Matrix4f &b) const {
    Matrix4f o;
    for (int c = 0; c < 4; ++c)
      for (int r = 0; r < 4; ++r) {
        float a = 0.f;
        for (int k = 0; k < 4; ++k) a += m[4 * k + r] * b.m[4 * c + k];
        o.m[4 * c + r] = a;
      }
    return o;
  }
  bool operator!=(const Matrix4f &b) const { return std::memcmp(m, b.m, sizeof m) != 0; }
  const float *data() const { return m; }
  float *data() { return m; }
};

// ------------------------------------------------------------------------------------------ plumbing
inline ope_ctx *default_context(int device = 0) {
  static ope_ctx *ctx = nullptr;
  if (!ctx && ope_ctx_create(&ctx, device) != OPE_OK) {
    std::fprintf(stderr, "[ope] cannot create a GPU context: %s\n", ope_last_error(nullptr));
    ctx = nullptr;
  }
  return ctx;
}
inline void log_error(const char *where, ope_ctx *ctx) { std::fprintf(stderr, "[ope::%s] %s\n", where, ope_last_error(ctx)); }

struct CloudHandle {
  ope_cloud *h = nullptr;
  ~CloudHandle() { if (h) ope_cloud_free(h); }
};
struct IndexHandle {
  ope_index *h = nullptr;
  ~IndexHandle() { if (h) ope_index_free(h); }
};

template <class PointT> inline std::shared_ptr<CloudHandle> upload(const PointCloud<PointT> &c, bool with_normals) {
  auto r = std::make_shared<CloudHandle>();
  ope_ctx *ctx = default_context();
  if (!ctx) return r;
  const ptrdiff_t noff = with_normals ? point_traits<PointT>::normal_offset : -1;
  if (ope_cloud_upload(ctx, c.points.data(), c.points.size(), sizeof(PointT), 0, noff, &r->h) != OPE_OK) log_error("upload", ctx);
  return r;
}

template <class PointT> inline void transformPointCloud(const PointCloud<PointT> &in, PointCloud<PointT> &out, const Matrix4f &T) {
  if (&in != &out) out = in;
  for (auto &p : out.points) {
    if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z)) continue;
    const float x = p.x, y = p.y, z = p.z;
    p.x = T.m[0] * x + T.m[4] * y + T.m[8] * z + T.m[12];
    p.y = T.m[1] * x + T.m[5] * y + T.m[9] * z + T.m[13];
    p.z = T.m[2] * x + T.m[6] * y + T.m[10] * z + T.m[14];
  }
}

// pcl::transformPointCloudWithNormals: xyz by T, the normal by T's rotation block (what
// IterativeClosestPointWithNormals::transformCloud applies to its working cloud, vPCL impl/icp_mod.hpp:311-318).
template <class PointT> inline void transformPointCloudWithNormals(const PointCloud<PointT> &in, PointCloud<PointT> &out, const Matrix4f &T) {
  static_assert(point_traits<PointT>::normal_offset >= 0, "transformPointCloudWithNormals needs a point type with normals");
  transformPointCloud(in, out, T);
  for (auto &p : out.points) {
    float *n = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(&p) + point_traits<PointT>::normal_offset);
    const float x = n[0], y = n[1], z = n[2];
    n[0] = T.m[0] * x + T.m[4] * y + T.m[8] * z;
    n[1] = T.m[1] * x + T.m[5] * y + T.m[9] * z;
    n[2] = T.m[2] * x + T.m[6] * y + T.m[10] * z;
  }
}

// pcl::ScopeTime: wall-clock of a scope, printed to stderr as "<title> took <ms>ms." when the scope ends.  The reference
// wraps its two stages in ScopeTime t("Initial Alignment") / ("Final Alignment") (poseestimator.cpp:61,349).
class ScopeTime {
 public:
  explicit ScopeTime(const char *title) : title_(title) { clock_gettime(CLOCK_MONOTONIC, &t0_); }
  double getTime() const {
    timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return (t1.tv_sec - t0_.tv_sec) * 1e3 + (t1.tv_nsec - t0_.tv_nsec) * 1e-6;
  }
  ~ScopeTime() { std::fprintf(stderr, "%s took %gms.\n", title_.c_str(), getTime()); }
 private:
  std::string title_;
  timespec t0_;
};

// ------------------------------------------------------------------------------------------ strategies
namespace registration {

// CorrespondenceEstimationBase (vPCL correspondence_estimation_mod.h:286-299).  Inside ICP the estimation is fused into
// the search kernel and the object only selects the mode; called stand-alone (poseestimator.cpp:242-247 does, once, and
// throws the result away) determineCorrespondences runs ONE search pass of the same kernel through the C ABI
// (ope_icp_begin -> ope_icp_accumulate -> ope_icp_correspondences) and returns pcl::Correspondences in query order with
// squared distances.
template <class PointSource, class PointTarget> struct CorrespondenceEstimationBase {
  typedef std::shared_ptr<CorrespondenceEstimationBase> Ptr;
  virtual ~CorrespondenceEstimationBase() {}
  virtual int mode() const { return OPE_CORR_NEAREST; }
  virtual int k() const { return 1; }
  void setInputSource(const typename PointCloud<PointSource>::ConstPtr &c) { input_ = c; }
  void setInputCloud(const typename PointCloud<PointSource>::ConstPtr &c) { input_ = c; }
  void setInputTarget(const typename PointCloud<PointTarget>::ConstPtr &c) { target_ = c; }
  // max_distance: 1-NN keeps d2 <= max_distance^2 (correspondence_estimation_mod.hpp:171); normal shooting compares the
  // SQUARED point-to-line distance with the unsquared max_distance (quirk Q2, ...normal_shooting_weighted.hpp:136)
  virtual void determineCorrespondences(Correspondences &correspondences, double max_distance = std::sqrt(DBL_MAX)) {
    run_pass(correspondences, max_distance, false);
  }
  virtual void determineReciprocalCorrespondences(Correspondences &correspondences, double max_distance = std::sqrt(DBL_MAX)) {
    run_pass(correspondences, max_distance, true);
  }
 protected:
  void run_pass(Correspondences &out, double max_distance, bool reciprocal) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || !target_ || target_->empty()) return;
    const bool nrm = mode() == OPE_CORR_NORMAL_SHOOTING;
    auto src = upload(*input_, nrm), tgt = upload(*target_, false);
    IndexHandle ix;
    if (!src->h || !tgt->h || ope_index_build(ctx, tgt->h, nullptr, &ix.h) != OPE_OK) { log_error("determineCorrespondences", ctx); return; }
    ope_icp_params p;
    ope_icp_default_params(&p);
    p.max_iterations = 1;
    p.max_corr_dist = max_distance;
    p.corr_mode = mode();
    p.k_normal_shooting = k();
    p.use_reciprocal = reciprocal ? 1 : 0;
    std::vector<int32_t> q(input_->size()), m(input_->size());
    std::vector<float> d(input_->size());
    size_t n = 0;
    if (ope_icp_begin(ctx, src->h, ix.h, nullptr, &p) != OPE_OK || ope_icp_accumulate(ctx) != OPE_OK ||
        ope_icp_correspondences(ctx, q.data(), m.data(), d.data(), q.size(), &n) != OPE_OK) {
      log_error("determineCorrespondences", ctx);
      return;
    }
    ope_icp_end(ctx, nullptr, nullptr);
    out.resize(n);
    for (size_t i = 0; i < n; ++i) { out[i].index_query = q[i]; out[i].index_match = m[i]; out[i].distance = d[i]; }
  }
  typename PointCloud<PointSource>::ConstPtr input_;
  typename PointCloud<PointTarget>::ConstPtr target_;
};
template <class S, class T, class Scalar = float> struct CorrespondenceEstimation : CorrespondenceEstimationBase<S, T> {
  typedef std::shared_ptr<CorrespondenceEstimation> Ptr;
};
template <class S, class T, class N, class Scalar = float> struct CorrespondenceEstimationNormalShooting : CorrespondenceEstimationBase<S, T> {
  typedef std::shared_ptr<CorrespondenceEstimationNormalShooting> Ptr;
  int k_ = 10;   // the class default (vPCL correspondence_estimation_normal_shooting_weighted.h:117)
  void setKSearch(int k) { k_ = k; }
  int mode() const override { return OPE_CORR_NORMAL_SHOOTING; }
  int k() const override { return k_; }
  // the source normals travel inside the source point type (PointXYZRGBNormal at poseestimator.cpp:244)
  template <class P> void setSourceNormals(const P &) {}
};

// CorrespondenceRejector (vPCL correspondence_rejection_mod.h:108-110,138-183).  Inside ICP the predicates are fused into
// the search kernel (`apply`); stand-alone, getRemainingCorrespondences evaluates the same predicate for the given
// correspondences on the device (ope_reject_pairs).
struct CorrespondenceRejector {
  typedef std::shared_ptr<CorrespondenceRejector> Ptr;
  virtual ~CorrespondenceRejector() {}
  virtual void apply(ope_icp_params &p) const = 0;
  // The global rejectors (median distance, one to one, var trimmed) decide over all of an iteration's pairs: they are not fused
  // into the search but handed to the context as a list (ope_icp_set_global_rejectors).  global() fills the list entry and says
  // so; took() receives what the last iteration of an align() did with it.
  virtual bool global(ope_global_rejector &) const { return false; }
  virtual void took(const ope_global_rejector_stats &) {}
  virtual void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) = 0;
  void setInputCorrespondences(const std::shared_ptr<const Correspondences> &c) { input_correspondences_ = c; }
  void getCorrespondences(Correspondences &out) {
    out.clear();
    if (input_correspondences_) getRemainingCorrespondences(*input_correspondences_, out);
  }
 protected:
  std::shared_ptr<const Correspondences> input_correspondences_;
  // packed xyz / normal triples of a cloud, pulled out of whatever point type it has
  struct Triples { std::vector<float> v; bool set = false; };
  template <class P> static void take_xyz(const PointCloud<P> &c, Triples &t) {
    t.v.resize(3 * c.size());
    for (size_t i = 0; i < c.size(); ++i) { t.v[3 * i] = c[i].x; t.v[3 * i + 1] = c[i].y; t.v[3 * i + 2] = c[i].z; }
    t.set = true;
  }
  template <class N> static void take_normals(const PointCloud<N> &c, Triples &t) {
    static_assert(point_traits<N>::normal_offset >= 0, "point type carries no normal");
    t.v.resize(3 * c.size());
    for (size_t i = 0; i < c.size(); ++i)
      std::memcpy(&t.v[3 * i], reinterpret_cast<const unsigned char *>(&c[i]) + point_traits<N>::normal_offset, 12);
    t.set = true;
  }
  static void filter(int kind, double thr, const Triples &a, bool a_by_query, const Triples &b, bool b_by_query,
                     const Correspondences &in, Correspondences &out) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || in.empty()) return;
    if (!a.set || !b.set) { std::fprintf(stderr, "[ope::CorrespondenceRejector] input clouds / normals were not set\n"); return; }
    std::vector<float> pa(3 * in.size()), pb(3 * in.size());
    for (size_t i = 0; i < in.size(); ++i) {
      const size_t ia = (size_t)(a_by_query ? in[i].index_query : in[i].index_match), ib = (size_t)(b_by_query ? in[i].index_query : in[i].index_match);
      if (3 * ia + 2 >= a.v.size() || 3 * ib + 2 >= b.v.size()) return;
      std::memcpy(&pa[3 * i], &a.v[3 * ia], 12);
      std::memcpy(&pb[3 * i], &b.v[3 * ib], 12);
    }
    std::vector<unsigned char> keep(in.size());
    if (ope_reject_pairs(ctx, kind, pa.data(), pb.data(), in.size(), thr, keep.data()) != OPE_OK) { log_error("getRemainingCorrespondences", ctx); return; }
    for (size_t i = 0; i < in.size(); ++i)
      if (keep[i]) out.push_back(in[i]);
  }
};
// keep a correspondence if n_src . n_tgt > threshold (score: correspondence_rejection_mod.h:368-376; poseestimator.cpp:264-273)
struct CorrespondenceRejectorSurfaceNormal : CorrespondenceRejector {
  typedef std::shared_ptr<CorrespondenceRejectorSurfaceNormal> Ptr;
  double threshold_ = 1.0;
  void setThreshold(double t) { threshold_ = t; }
  double getThreshold() const { return threshold_; }
  template <class P, class N> void initializeDataContainer() {}
  template <class P> void setInputSource(const typename PointCloud<P>::ConstPtr &) {}
  template <class P> void setInputTarget(const typename PointCloud<P>::ConstPtr &) {}
  template <class P, class N> void setInputNormals(const typename PointCloud<N>::ConstPtr &n) { if (n) take_normals(*n, src_n_); }
  template <class P, class N> void setTargetNormals(const typename PointCloud<N>::ConstPtr &n) { if (n) take_normals(*n, tgt_n_); }
  void apply(ope_icp_params &p) const override { p.use_surface_normal_rej = 1; p.surface_normal_thr = threshold_; }
  void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) override {
    filter(OPE_REJ_SURFACE_NORMAL, threshold_, src_n_, true, tgt_n_, false, original, remaining);
  }
 private:
  Triples src_n_, tgt_n_;
};
// keep a correspondence if n_src . (-p_src / |p_src|) > threshold (vPCL correspondence_rejection_mod.h:382-391,
// impl/correspondence_rejection_self_occluded_normal.cpp:43-64); opt-in, see SURVEY Q3
struct CorrespondenceRejectorSelfOccludedNormal : CorrespondenceRejector {
  typedef std::shared_ptr<CorrespondenceRejectorSelfOccludedNormal> Ptr;
  double threshold_ = 1.0;
  void setThreshold(double t) { threshold_ = t; }
  double getThreshold() const { return threshold_; }
  template <class P, class N> void initializeDataContainer() {}
  template <class P> void setInputSource(const typename PointCloud<P>::ConstPtr &c) { if (c) take_xyz(*c, src_p_); }
  template <class P, class N> void setInputNormals(const typename PointCloud<N>::ConstPtr &n) { if (n) take_normals(*n, src_n_); }
  void apply(ope_icp_params &p) const override { p.use_self_occluded_rej = 1; p.self_occluded_thr = threshold_; }
  void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) override {
    filter(OPE_REJ_SELF_OCCLUDED, threshold_, src_n_, true, src_p_, true, original, remaining);
  }
 private:
  Triples src_n_, src_p_;
};

// The three rejectors of estimateFinePose's list that need every pair of an iteration (poseestimator.cpp:250-292, blocks 3.1, 3.2
// and 3.5, commented out there), without a data container as that block uses them: `distance` is what the estimation wrote.
// Stand-alone they run ope_reject_correspondences; added to an ICP they become the context's list for that align(), in the order
// added.  The remaining correspondences stay in the order given (PCL's one-to-one returns them in match order).
struct CorrespondenceRejectorGlobal : CorrespondenceRejector {
  void apply(ope_icp_params &) const override {}
  void took(const ope_global_rejector_stats &st) override { stats_ = st; }
  void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) override {
    remaining.clear();
    ope_ctx *ctx = default_context();
    ope_global_rejector r;
    if (!ctx || !global(r)) return;
    std::vector<int32_t> q(original.size()), m(original.size());
    std::vector<float> d(original.size());
    for (size_t i = 0; i < original.size(); ++i) { q[i] = original[i].index_query; m[i] = original[i].index_match; d[i] = original[i].distance; }
    std::vector<unsigned char> keep(original.size());
    if (ope_reject_correspondences(ctx, &r, q.data(), m.data(), d.data(), original.size(), keep.data(), &stats_) != OPE_OK) {
      log_error("getRemainingCorrespondences", ctx);
      return;
    }
    for (size_t i = 0; i < original.size(); ++i)
      if (keep[i]) remaining.push_back(original[i]);
  }
  const ope_global_rejector_stats &getStats() const { return stats_; }   // not PCL's: pairs in and out, threshold, ratio
 protected:
  ope_global_rejector_stats stats_{};
};
struct CorrespondenceRejectorMedianDistance : CorrespondenceRejectorGlobal {
  typedef std::shared_ptr<CorrespondenceRejectorMedianDistance> Ptr;
  void setMedianFactor(double f) { factor_ = f; }
  double getMedianFactor() const { return factor_; }
  double getMedianDistance() const { return stats_.threshold; }
  bool global(ope_global_rejector &r) const override {
    ope_global_rejector_defaults(OPE_GREJ_MEDIAN_DISTANCE, &r);
    r.factor = factor_;
    return true;
  }
 private:
  double factor_ = 1.0;
};
struct CorrespondenceRejectorOneToOne : CorrespondenceRejectorGlobal {
  typedef std::shared_ptr<CorrespondenceRejectorOneToOne> Ptr;
  bool global(ope_global_rejector &r) const override {
    ope_global_rejector_defaults(OPE_GREJ_ONE_TO_ONE, &r);
    return true;
  }
};
struct CorrespondenceRejectorVarTrimmed : CorrespondenceRejectorGlobal {
  typedef std::shared_ptr<CorrespondenceRejectorVarTrimmed> Ptr;
  void setMinRatio(double r) { min_ratio_ = r; }
  double getMinRatio() const { return min_ratio_; }
  void setMaxRatio(double r) { max_ratio_ = r; }
  double getMaxRatio() const { return max_ratio_; }
  double getTrimmedDistance() const { return stats_.threshold; }
  double getTrimFactor() const { return stats_.ratio; }
  bool global(ope_global_rejector &r) const override {
    ope_global_rejector_defaults(OPE_GREJ_VAR_TRIMMED, &r);
    r.min_ratio = min_ratio_;
    r.max_ratio = max_ratio_;
    return true;
  }
 private:
  double min_ratio_ = 0.05, max_ratio_ = 0.95;
};

template <class S, class T, class Scalar = float> struct TransformationEstimationSVD {
  typedef std::shared_ptr<TransformationEstimationSVD> Ptr;
  static constexpr int ope_estimator = OPE_EST_SVD;
  void estimateRigidTransformation(const PointCloud<S> &src, const PointCloud<T> &tgt, const Correspondences &corrs,
                                   Matrix4f &out) const {
    out = Matrix4f::Identity();
    ope_ctx *ctx = default_context();
    if (!ctx || corrs.empty()) return;
    std::vector<float> a(3 * corrs.size()), b(3 * corrs.size());
    for (size_t i = 0; i < corrs.size(); ++i) {
      const S &s = src.points[corrs[i].index_query];
      const T &t = tgt.points[corrs[i].index_match];
      a[3 * i] = s.x; a[3 * i + 1] = s.y; a[3 * i + 2] = s.z;
      b[3 * i] = t.x; b[3 * i + 1] = t.y; b[3 * i + 2] = t.z;
    }
    if (ope_rigid_transform_svd(ctx, a.data(), b.data(), corrs.size(), out.m) != OPE_OK) log_error("TransformationEstimationSVD", ctx);
  }
};

// CorrespondenceEstimation over FPFH rows (BuildModel poseestimator.cpp:43-47, commented out there): every source row is matched to
// the target row with the smallest squared L2 distance, lowest index on a tie (ope_feature_correspondences); `distance` is that
// squared distance.  Rows without a finite distance give no correspondence.  max_distance keeps distance <= max_distance^2, as the
// point version does.  Reciprocal matches are not built.
template <class Scalar> struct CorrespondenceEstimation<FPFHSignature33, FPFHSignature33, Scalar> {
  typedef std::shared_ptr<CorrespondenceEstimation> Ptr;
  void setInputSource(const typename PointCloud<FPFHSignature33>::ConstPtr &c) { input_ = c; }
  void setInputCloud(const typename PointCloud<FPFHSignature33>::ConstPtr &c) { input_ = c; }
  void setInputTarget(const typename PointCloud<FPFHSignature33>::ConstPtr &c) { target_ = c; }
  void determineCorrespondences(Correspondences &out, double max_distance = std::sqrt(DBL_MAX)) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || !target_ || input_->empty() || target_->empty()) return;
    std::vector<int32_t> q(input_->size()), m(input_->size());
    std::vector<float> d(input_->size());
    size_t n = 0;
    if (ope_feature_correspondences(ctx, &input_->points[0].histogram[0], input_->size(), &target_->points[0].histogram[0], target_->size(),
                                    q.data(), m.data(), d.data(), &n) != OPE_OK) { log_error("determineCorrespondences", ctx); return; }
    const double max_d2 = max_distance * max_distance;
    for (size_t i = 0; i < n; ++i) {
      if ((double)d[i] > max_d2) continue;
      Correspondence c;
      c.index_query = q[i]; c.index_match = m[i]; c.distance = d[i];
      out.push_back(c);
    }
  }
 private:
  typename PointCloud<FPFHSignature33>::ConstPtr input_, target_;
};

// CorrespondenceRejectorSampleConsensus (BuildModel poseestimator.cpp:49-60; DetectAndLocalize :275-281, both commented out there) on
// ope_corr_sac: RANSAC over SampleConsensusModelRegistration, the class defaults PCL's (threshold 0.05, 1000 iterations).
// getBestTransformation() is the winning hypothesis, the identity when no model was found (then every correspondence remains).
// Stand-alone only: inside an ICP loop apply() selects nothing (ICP's fused search has no such stage); refineModel is not built.
// Two correspondences with one index_query are refused (PCL's index map would silently keep the last): nothing remains.
template <class PointT> struct CorrespondenceRejectorSampleConsensus : CorrespondenceRejector {
  typedef std::shared_ptr<CorrespondenceRejectorSampleConsensus> Ptr;
  CorrespondenceRejectorSampleConsensus() { ope_corr_sac_default_params(&p_); }
  void setInputSource(const typename PointCloud<PointT>::ConstPtr &c) { src_ = c; }
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { src_ = c; }
  void setInputTarget(const typename PointCloud<PointT>::ConstPtr &c) { tgt_ = c; }
  void setInlierThreshold(double t) { p_.inlier_threshold = t; }
  double getInlierThreshold() const { return p_.inlier_threshold; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  int getMaximumIterations() const { return p_.max_iterations; }
  void setSeed(uint64_t s) { p_.seed = s; }   // PCL's engine starts from 12345 unless asked for a random seed: made explicit here
  Matrix4f getBestTransformation() const { return best_; }
  bool foundModel() const { return found_; }                 // not PCL's: whether RANSAC came back with a model
  int getNumberOfIterations() const { return iterations_; }  // not PCL's: RandomSampleConsensus::iterations_
  void apply(ope_icp_params &) const override {}
  void getRemainingCorrespondences(const Correspondences &original, Correspondences &remaining) override {
    remaining.clear();
    best_ = Matrix4f::Identity();
    found_ = false;
    iterations_ = 0;
    ope_ctx *ctx = default_context();
    if (!ctx || !src_ || !tgt_) { std::fprintf(stderr, "[ope::CorrespondenceRejectorSampleConsensus] input clouds were not set\n"); return; }
    if (original.empty()) return;
    auto ds = upload(*src_, false), dt = upload(*tgt_, false);
    if (!ds->h || !dt->h) return;
    std::vector<int32_t> q(original.size()), m(original.size()), pos(original.size());
    for (size_t i = 0; i < original.size(); ++i) { q[i] = original[i].index_query; m[i] = original[i].index_match; }
    ope_corr_sac_result r;
    if (ope_corr_sac(ctx, ds->h, dt->h, q.data(), m.data(), q.size(), &p_, nullptr, 0, &r, pos.data()) != OPE_OK) {
      log_error("CorrespondenceRejectorSampleConsensus", ctx);
      return;
    }
    std::memcpy(best_.m, r.T_best, sizeof best_.m);
    found_ = r.found != 0;
    iterations_ = r.iterations;
    remaining.reserve((size_t)r.inliers);
    for (int32_t i = 0; i < r.inliers; ++i) remaining.push_back(original[(size_t)pos[(size_t)i]]);
  }
 private:
  typename PointCloud<PointT>::ConstPtr src_, tgt_;
  ope_corr_sac_params p_;
  Matrix4f best_ = Matrix4f::Identity();
  bool found_ = false;
  int iterations_ = 0;
};

// Selected by type in setTransformationEstimation: the 6x6 normal equations of the linearised point-to-plane
// error (the IterativeClosestPointWithNormals default, vPCL icp_mod.h:355).
template <class S, class T, class Scalar = float> struct TransformationEstimationPointToPlaneLLS {
  typedef std::shared_ptr<TransformationEstimationPointToPlaneLLS> Ptr;
  static constexpr int ope_estimator = OPE_EST_POINT_TO_PLANE_LLS;
};
// PCL's class of this name minimises the same error with Levenberg-Marquardt over (t, quaternion)
// (BuildModel regmeshpcd.cpp:162,193): OPE_EST_POINT_TO_PLANE_LM, csrc/lm.hip.
template <class S, class T, class Scalar = float> struct TransformationEstimationPointToPlane {
  typedef std::shared_ptr<TransformationEstimationPointToPlane> Ptr;
  static constexpr int ope_estimator = OPE_EST_POINT_TO_PLANE_LM;
};

// DefaultConvergenceCriteria knobs the reference can reach through getConvergeCriteria()
struct DefaultConvergenceCriteria {
  enum ConvergenceState {
    CONVERGENCE_CRITERIA_NOT_CONVERGED, CONVERGENCE_CRITERIA_ITERATIONS, CONVERGENCE_CRITERIA_TRANSFORM,
    CONVERGENCE_CRITERIA_ABS_MSE, CONVERGENCE_CRITERIA_REL_MSE, CONVERGENCE_CRITERIA_NO_CORRESPONDENCES
  };
  double mse_threshold_absolute_ = 1e-12;
  bool failure_after_max_iter_ = false;
  ConvergenceState state_ = CONVERGENCE_CRITERIA_NOT_CONVERGED;
  void setAbsoluteMSE(double v) { mse_threshold_absolute_ = v; }
  double getAbsoluteMSE() const { return mse_threshold_absolute_; }
  void setFailureAfterMaximumIterations(bool v) { failure_after_max_iter_ = v; }
  ConvergenceState getConvergenceState() const { return state_; }
};

}  // namespace registration

// ------------------------------------------------------------------------------------------ ICP
template <class PointSource, class PointTarget, class Scalar = float> class IterativeClosestPoint {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef Matrix4f Matrix4;

  IterativeClosestPoint() { ope_icp_default_params(&params_); criteria_ = std::make_shared<registration::DefaultConvergenceCriteria>(); }
  virtual ~IterativeClosestPoint() {}

  void setInputSource(const typename PointCloudSource::ConstPtr &cloud) { input_ = cloud; src_dev_.reset(); correspondences_.clear(); }
  typename PointCloudSource::ConstPtr const getInputSource() const { return input_; }
  typename PointCloudTarget::ConstPtr const getInputTarget() const { return target_; }
  void setInputCloud(const typename PointCloudSource::ConstPtr &cloud) { setInputSource(cloud); }
  void setInputTarget(const typename PointCloudTarget::ConstPtr &cloud) {
    if (!cloud || cloud->points.empty()) {  // registration_mod.hpp:60-64
      std::fprintf(stderr, "[ope::IterativeClosestPoint::setInputTarget] Invalid or empty point cloud dataset given!\n");
      return;
    }
    target_ = cloud;
    tgt_dev_.reset(); tgt_index_.reset();
  }
  void setMaximumIterations(int n) { params_.max_iterations = n; }
  void setTransformationEpsilon(double e) { params_.transformation_epsilon = e; }
  void setEuclideanFitnessEpsilon(double e) { params_.euclidean_fitness_epsilon = e; }
  void setMaxCorrespondenceDistance(double d) { params_.max_corr_dist = d; }
  void setRANSACOutlierRejectionThreshold(double) {}  // accepted and unused, as in the reference (poseestimator.cpp:319)
  void setUseReciprocalCorrespondences(bool b) { params_.use_reciprocal = b ? 1 : 0; }
  typedef registration::CorrespondenceEstimationBase<PointSource, PointTarget> CorrespondenceEstimation;
  void setCorrespondenceEstimation(const std::shared_ptr<CorrespondenceEstimation> &ce) { corr_est_ = ce; }
  void addCorrespondenceRejector(const registration::CorrespondenceRejector::Ptr &r) { rejectors_.push_back(r); }
  template <class TE> void setTransformationEstimation(const std::shared_ptr<TE> &) { params_.estimator = TE::ope_estimator; }
  std::shared_ptr<registration::DefaultConvergenceCriteria> getConvergeCriteria() { return criteria_; }
  // vPCL icp_mod.h:268-281 — the reference's injection of given pairs into every iteration (unused by its own programs).
  // The pointer is kept, as in the reference; the pairs are read at align().  The reference's correspondence estimation also
  // writes each pair's `distance` field back through the pointer, every iteration (correspondence_estimation_mod.hpp:150-161):
  // align() leaves the last iteration's values there, which is what a caller of the reference finds after align().
  void setFixedCorrespondences(Correspondences *correspondences) { corres_fixed_ = correspondences; }
  Correspondences getFixedCorrespondences() { return *corres_fixed_; }
  void clearCorrespondences() { if (corres_fixed_) corres_fixed_->clear(); }

  void align(PointCloudSource &output) { align(output, Matrix4f::Identity()); }
  void align(PointCloudSource &output, const Matrix4f &guess) {
    converged_ = false;
    final_ = Matrix4f::Identity();
    last_incremental_ = Matrix4f::Identity();
    nr_iterations_ = 0;
    n_corr_ = 0;
    correspondences_.clear();
    ope_ctx *ctx = default_context();
    if (!ctx) return;
    if (!target_) {  // registration_mod.hpp:73-77
      std::fprintf(stderr, "[ope::IterativeClosestPoint::compute] No input target dataset was given!\n");
      return;
    }
    if (!input_) return;
    ope_icp_params p = params_;
    p.corr_mode = corr_est_ ? corr_est_->mode() : OPE_CORR_NEAREST;
    if (corr_est_) p.k_normal_shooting = corr_est_->k();
    p.use_surface_normal_rej = p.use_self_occluded_rej = 0;
    // the global rejectors become the context's list for this run, in the order added; a pointwise rejector behind one of them
    // cannot be honoured (the pointwise ones are fused into the search, which runs first)
    std::vector<ope_global_rejector> glist;
    std::vector<registration::CorrespondenceRejector *> gown;
    for (auto &r : rejectors_) {
      ope_global_rejector g;
      if (r->global(g)) { glist.push_back(g); gown.push_back(r.get()); continue; }
      if (!glist.empty()) {
        std::fprintf(stderr, "[ope::IterativeClosestPoint::align] a pointwise correspondence rejector was added after a global one: "
                             "pointwise rejectors are fused into the search and cannot run behind it; not aligning\n");
        return;
      }
      r->apply(p);
    }
    p.mse_threshold_absolute = criteria_->mse_threshold_absolute_;
    p.failure_after_max_iter = criteria_->failure_after_max_iter_ ? 1 : 0;
    const bool nrm = p.corr_mode == OPE_CORR_NORMAL_SHOOTING || p.use_surface_normal_rej || p.use_self_occluded_rej ||
                     p.estimator == OPE_EST_POINT_TO_PLANE_LLS || p.estimator == OPE_EST_POINT_TO_PLANE_LM;
    // uploads are cached between align() calls on the same clouds; a cache made without normals is of no use once a
    // rejector, normal shooting or the point-to-plane estimator has been added
    if (nrm && !uploaded_with_normals_) { src_dev_.reset(); tgt_dev_.reset(); tgt_index_.reset(); }
    if (!src_dev_) src_dev_ = upload(*input_, nrm);
    if (!tgt_index_) {
      uploaded_with_normals_ = nrm;
      tgt_dev_ = upload(*target_, nrm);
      tgt_index_ = std::make_shared<IndexHandle>();
      if (tgt_dev_->h && ope_index_build(ctx, tgt_dev_->h, nullptr, &tgt_index_->h) != OPE_OK) log_error("align", ctx);
    }
    if (!src_dev_->h || !tgt_index_->h) return;
    // icp_mod.hpp:150-151: the given pairs, if any, go to the correspondence estimation of THIS run (the context is shared
    // between objects: they are cleared again below)
    std::vector<int32_t> fq, fm;
    {
      if (corres_fixed_)
        for (const Correspondence &c : *corres_fixed_) { fq.push_back(c.index_query); fm.push_back(c.index_match); }
      if (ope_icp_set_fixed_correspondences(ctx, src_dev_->h, tgt_dev_->h, fq.data(), fm.data(), fq.size()) != OPE_OK) {
        log_error("align (fixed correspondences)", ctx);
        return;
      }
    }
    if (ope_icp_set_global_rejectors(ctx, glist.data(), glist.size()) != OPE_OK) {
      log_error("align (global rejectors)", ctx);
      (void)ope_icp_set_fixed_correspondences(ctx, nullptr, nullptr, nullptr, nullptr, 0);
      return;
    }
    ope_icp_result res;
    const int rc_run = ope_icp_run(ctx, src_dev_->h, tgt_index_->h, guess.m, &p, final_.m, &res);
    if (!glist.empty()) {   // the context is shared between objects: the list is this run's only
      for (size_t k = 0; rc_run == OPE_OK && k < gown.size(); ++k) {
        ope_global_rejector_stats st;
        if (ope_icp_global_rejector_stats(ctx, k, &st) == OPE_OK) gown[k]->took(st);
      }
      (void)ope_icp_set_global_rejectors(ctx, nullptr, 0);
    }
    std::vector<int32_t> fixed_listed, fixed_appended;
    if (corres_fixed_ && !corres_fixed_->empty()) {
      std::vector<float> fd(fq.size());
      fixed_listed.resize(fq.size());
      fixed_appended.resize(fq.size());
      size_t nf = 0;
      if (rc_run == OPE_OK && ope_icp_fixed_correspondences(ctx, fd.data(), fixed_listed.data(), fixed_appended.data(), fd.size(), &nf) == OPE_OK &&
          nf == corres_fixed_->size())
        for (size_t f = 0; f < nf; ++f) (*corres_fixed_)[f].distance = fd[f];
      else
        fixed_listed.clear(), fixed_appended.clear();
      (void)ope_icp_set_fixed_correspondences(ctx, nullptr, nullptr, nullptr, nullptr, 0);
    }
    if (rc_run != OPE_OK) {
      log_error("align", ctx);
      final_ = Matrix4f::Identity();
      return;
    }
    converged_ = res.converged != 0;
    nr_iterations_ = res.iterations;
    n_corr_ = res.n_corr;
    criteria_->state_ = (registration::DefaultConvergenceCriteria::ConvergenceState)res.state;
    if (ope_icp_last_incremental(ctx, last_incremental_.m) != OPE_OK) last_incremental_ = Matrix4f::Identity();
    // correspondences_ is a member of the reference's object too (icp_mod.h:249-260 reads it): fetched now, while the
    // context still holds THIS object's run
    {
      std::vector<int32_t> q(input_->size()), m(input_->size());
      std::vector<float> d(input_->size());
      size_t n = 0;
      if (ope_icp_correspondences(ctx, q.data(), m.data(), d.data(), q.size(), &n) == OPE_OK) {
        // the reference's list: given pairs that the estimation listed (through every rejector), the searched pairs, the given
        // pairs once more where the first rejector alone lets them through (icp_mod.hpp:210-224)
        for (size_t f = 0; f < fixed_listed.size(); ++f)
          if (fixed_listed[f]) correspondences_.push_back((*corres_fixed_)[f]);
        const size_t at = correspondences_.size();
        correspondences_.resize(at + n);
        for (size_t i = 0; i < n; ++i) { correspondences_[at + i].index_query = q[i]; correspondences_[at + i].index_match = m[i]; correspondences_[at + i].distance = d[i]; }
        for (size_t f = 0; f < fixed_appended.size(); ++f)
          if (fixed_appended[f]) correspondences_.push_back((*corres_fixed_)[f]);
      }
    }
    transformOutput(output);  // icp_mod.hpp:269-271
  }

  Matrix4f getFinalTransformation() const { return final_; }
  Matrix4f getLastIncrementalTransformation() const { return last_incremental_; }   // transformation_, registration_mod.h
  bool hasConverged() const { return converged_; }
  int getNumberOfIterations() const { return nr_iterations_; }
  double getFitnessScore(double max_range = DBL_MAX) {
    ope_ctx *ctx = default_context();
    double score = DBL_MAX;
    if (ctx && src_dev_ && tgt_index_ && src_dev_->h && tgt_index_->h &&
        ope_fitness(ctx, src_dev_->h, tgt_index_->h, final_.m, max_range, &score, nullptr, nullptr) != OPE_OK)
      log_error("getFitnessScore", ctx);
    return score;
  }
  // icp_mod.h:249-260
  double getAlignStrength() const {
    const double denom = (double)((input_ ? input_->size() : 0) + (target_ ? target_->size() : 0));
    return denom > 0 ? (double)n_corr_ / denom : 0.0;
  }
  // pcl::Correspondences of the last iteration (post-rejection), query order
  Correspondences getCorrespondences() const { return correspondences_; }

 protected:
  // Registration::transformCloud of the final result: xyz only here, xyz + normals in IterativeClosestPointWithNormals
  virtual void transformOutput(PointCloudSource &output) const { transformPointCloud(*input_, output, final_); }
  typename PointCloudSource::ConstPtr input_;
  typename PointCloudTarget::ConstPtr target_;
  bool uploaded_with_normals_ = false;
  Matrix4f last_incremental_ = Matrix4f::Identity();
  Correspondences correspondences_;
  Correspondences *corres_fixed_ = nullptr;   // icp_mod.h:326
  std::shared_ptr<CloudHandle> src_dev_, tgt_dev_;
  std::shared_ptr<IndexHandle> tgt_index_;
  ope_icp_params params_;
  std::shared_ptr<CorrespondenceEstimation> corr_est_;
  std::vector<registration::CorrespondenceRejector::Ptr> rejectors_;
  std::shared_ptr<registration::DefaultConvergenceCriteria> criteria_;
  Matrix4f final_ = Matrix4f::Identity();
  bool converged_ = false;
  int nr_iterations_ = 0;
  int64_t n_corr_ = 0;
};

// Transforms the normals too (vPCL impl/icp_mod.hpp:311-318; the kernels always do) and starts from the point-to-plane
// LLS estimator (icp_mod.h:355).
template <class S, class T, class Scalar = float> class IterativeClosestPointWithNormals : public IterativeClosestPoint<S, T, Scalar> {
 public:
  IterativeClosestPointWithNormals() { this->params_.estimator = OPE_EST_POINT_TO_PLANE_LLS; }
 protected:
  void transformOutput(PointCloud<S> &output) const override { transformPointCloudWithNormals(*this->input_, output, this->final_); }
};

// ------------------------------------------------------------------------------------------ features
namespace search { template <class P> struct KdTree { typedef std::shared_ptr<KdTree> Ptr; explicit KdTree(bool = true) {} }; }

template <class PointInT, class PointOutT = Normal> class NormalEstimation {
 public:
  void setInputCloud(const typename PointCloud<PointInT>::ConstPtr &c) { input_ = c; }
  template <class Tree> void setSearchMethod(const Tree &) {}  // the GPU index replaces the kd-tree
  void setKSearch(int k) { k_ = k; }
  void setViewPoint(float x, float y, float z) { vp_[0] = x; vp_[1] = y; vp_[2] = z; }
  // pcl::Feature::setSearchSurface: neighbourhoods are taken from `surface` instead of the input cloud
  void setSearchSurface(const typename PointCloud<PointInT>::ConstPtr &surface) { surface_ = surface; }
  void compute(PointCloud<PointOutT> &out) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    const size_t n = input_->size();
    std::vector<float> nrm(3 * n), curv(n);
    int rc;
    if (surface_ && surface_ != input_) {
      auto sdev = upload(*surface_, false);
      IndexHandle six;
      rc = sdev->h ? ope_index_build(ctx, sdev->h, nullptr, &six.h) : OPE_EINVAL;
      if (rc == OPE_OK) rc = ope_normals_from(ctx, dev->h, six.h, k_, vp_, nrm.data(), curv.data());
    } else {
      rc = ope_normals(ctx, dev->h, k_, vp_, nrm.data(), curv.data());
    }
    if (rc != OPE_OK) { log_error("NormalEstimation", ctx); return; }
    out.resize(n);
    out.is_dense = true;
    for (size_t i = 0; i < n; ++i) {
      out.points[i].normal_x = nrm[3 * i]; out.points[i].normal_y = nrm[3 * i + 1]; out.points[i].normal_z = nrm[3 * i + 2];
      out.points[i].curvature = curv[i];
      if (!std::isfinite(nrm[3 * i])) out.is_dense = false;
    }
  }
 private:
  typename PointCloud<PointInT>::ConstPtr input_, surface_;
  int k_ = 0;
  float vp_[3] = {0, 0, 0};
};

template <class PointInT, class PointNT = Normal, class PointOutT = FPFHSignature33> class FPFHEstimation {
 public:
  void setInputCloud(const typename PointCloud<PointInT>::ConstPtr &c) { input_ = c; }
  void setInputNormals(const typename PointCloud<PointNT>::ConstPtr &n) { normals_ = n; }
  void setRadiusSearch(double r) { radius_ = r; }
  template <class Tree> void setSearchMethod(const Tree &) {}
  void compute(PointCloud<PointOutT> &out) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || !normals_ || normals_->size() != input_->size()) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    const size_t n = input_->size();
    std::vector<float> nrm(3 * n);
    for (size_t i = 0; i < n; ++i) {
      nrm[3 * i] = normals_->points[i].normal_x; nrm[3 * i + 1] = normals_->points[i].normal_y; nrm[3 * i + 2] = normals_->points[i].normal_z;
    }
    out.resize(n);
    if (ope_cloud_set_normals(ctx, dev->h, nrm.data()) != OPE_OK ||
        ope_fpfh(ctx, dev->h, (float)radius_, &out.points[0].histogram[0]) != OPE_OK) {
      log_error("FPFHEstimation", ctx);
      out.clear();
    }
  }
 private:
  typename PointCloud<PointInT>::ConstPtr input_;
  typename PointCloud<PointNT>::ConstPtr normals_;
  double radius_ = 0;
};

template <class PointInT> class UniformSampling {
 public:
  void setInputCloud(const typename PointCloud<PointInT>::ConstPtr &c) { input_ = c; }
  void setRadiusSearch(double leaf) { leaf_ = leaf; }
  void compute(PointCloud<int> &out) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    std::vector<int32_t> idx(input_->size());
    size_t n = 0;
    if (ope_uniform_sampling(ctx, dev->h, (float)leaf_, idx.data(), &n) != OPE_OK) { log_error("UniformSampling", ctx); return; }
    out.points.assign(idx.begin(), idx.begin() + n);
    out.width = (uint32_t)n;
  }
 private:
  typename PointCloud<PointInT>::ConstPtr input_;
  double leaf_ = 0.01;
};

template <class P> inline void copyPointCloud(const PointCloud<P> &in, const std::vector<int> &indices, PointCloud<P> &out) {
  out.clear();
  out.points.reserve(indices.size());
  for (int i : indices) out.points.push_back(in.points[i]);
  out.width = (uint32_t)out.points.size();
}

// ------------------------------------------------------------------------------------------ filters
// pcl::removeNaNFromPointCloud (poseestimator.cpp:192-194); `index` maps output positions to input positions.
template <class P> inline void removeNaNFromPointCloud(const PointCloud<P> &in, PointCloud<P> &out, std::vector<int> &index) {
  index.clear();
  ope_ctx *ctx = default_context();
  auto dev = ctx ? upload(in, false) : std::shared_ptr<CloudHandle>();
  std::vector<int32_t> idx(in.size() + 1);
  size_t n = 0;
  if (!dev || !dev->h || ope_remove_nan(ctx, dev->h, idx.data(), &n) != OPE_OK) {
    if (ctx && dev && dev->h) log_error("removeNaNFromPointCloud", ctx);
    n = 0;
  }
  index.assign(idx.begin(), idx.begin() + n);
  PointCloud<P> tmp;
  tmp.points.reserve(n);
  for (size_t i = 0; i < n; ++i) tmp.points.push_back(in.points[index[i]]);
  tmp.width = (uint32_t)n;
  out = std::move(tmp);  // `in` and `out` may be the same object, as at poseestimator.cpp:193
  out.is_dense = true;
}

// pcl::PassThrough (processingpcd.cpp:13-33): one field per object, inclusive limits.
template <class PointT> class PassThrough {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setFilterFieldName(const std::string &f) { field_ = f; }
  void setFilterLimits(float lo, float hi) { lo_ = lo; hi_ = hi; }
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    std::vector<int> idx;
    filter(idx);
    tmp.points.reserve(idx.size());
    for (int i : idx) tmp.points.push_back(input_->points[i]);
    tmp.width = (uint32_t)idx.size();
    out = std::move(tmp);
  }
  // the indices of the survivors (segmentationregiongrow.cpp:95)
  void filter(std::vector<int> &indices) {
    indices.clear();
    ope_ctx *ctx = default_context();
    if (ctx && input_ && !input_->empty()) {
      float lo[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX}, hi[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
      const int d = field_ == "x" ? 0 : field_ == "y" ? 1 : field_ == "z" ? 2 : -1;
      if (d >= 0) { lo[d] = lo_; hi[d] = hi_; }   // an unknown / empty field name only drops non-finite points
      auto dev = upload(*input_, false);
      std::vector<int32_t> idx(input_->size());
      size_t n = 0;
      if (dev->h && ope_pass_through(ctx, dev->h, lo, hi, idx.data(), &n) != OPE_OK) { log_error("PassThrough", ctx); n = 0; }
      indices.assign(idx.begin(), idx.begin() + n);
    }
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  std::string field_;
  float lo_ = -FLT_MAX, hi_ = FLT_MAX;
};

// pcl::VoxelGrid (processingpcd.cpp:44-59): centroids in ascending voxel index; point types with a colour get the
// channel-wise mean of their voxel's colours (PCL's downsample_all_data_ default), other fields are default-initialised.
template <class PointT> class VoxelGrid {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx; leaf_[1] = ly; leaf_[2] = lz; }
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    ope_ctx *ctx = default_context();
    if (ctx && input_ && !input_->empty()) {
      auto dev = upload(*input_, false);
      std::vector<float> xyz(3 * input_->size());
      std::vector<uint32_t> rgb_in, rgb_out;
      constexpr ptrdiff_t rgb_off = point_traits<PointT>::rgb_offset;
      if (rgb_off >= 0) {
        rgb_in.resize(input_->size());
        rgb_out.resize(input_->size());
        for (size_t i = 0; i < input_->size(); ++i)
          std::memcpy(&rgb_in[i], reinterpret_cast<const unsigned char *>(&input_->points[i]) + rgb_off, 4);
      }
      size_t n = 0;
      const int rc = !dev->h ? OPE_EINVAL
                     : rgb_off >= 0 ? ope_voxel_grid_rgb(ctx, dev->h, leaf_, rgb_in.data(), xyz.data(), rgb_out.data(), &n)
                                    : ope_voxel_grid(ctx, dev->h, leaf_, xyz.data(), &n);
      if (rc == OPE_ERANGE) {  // voxel_grid.hpp: warn and hand the input back
        std::fprintf(stderr, "[ope::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
        out = *input_;
        return;
      }
      if (rc != OPE_OK) { log_error("VoxelGrid", ctx); n = 0; }
      tmp.points.resize(n);
      for (size_t i = 0; i < n; ++i) {
        tmp.points[i].x = xyz[3 * i]; tmp.points[i].y = xyz[3 * i + 1]; tmp.points[i].z = xyz[3 * i + 2];
        if (rgb_off >= 0) std::memcpy(reinterpret_cast<unsigned char *>(&tmp.points[i]) + rgb_off, &rgb_out[i], 4);
      }
      tmp.width = (uint32_t)n;
    }
    out = std::move(tmp);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  float leaf_[3] = {0.01f, 0.01f, 0.01f};
};

// pcl::StatisticalOutlierRemoval (ProcessingPcd::getOutlierRemove, DetectAndLocalize processingpcd.cpp:62-77)
template <class PointT> class StatisticalOutlierRemoval {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setMeanK(int k) { mean_k_ = k; }
  void setStddevMulThresh(double m) { mul_ = m; }
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    ope_ctx *ctx = default_context();
    if (ctx && input_ && !input_->empty()) {
      auto dev = upload(*input_, false);
      std::vector<int32_t> idx(input_->size());
      size_t n = 0;
      if (dev->h && ope_statistical_outlier_removal(ctx, dev->h, mean_k_, mul_, idx.data(), &n, nullptr) != OPE_OK) { log_error("StatisticalOutlierRemoval", ctx); n = 0; }
      tmp.points.reserve(n);
      for (size_t i = 0; i < n; ++i) tmp.points.push_back(input_->points[idx[i]]);
      tmp.width = (uint32_t)n;
    }
    out = std::move(tmp);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  int mean_k_ = 1;      // PCL's defaults
  double mul_ = 0.0;
};

// pcl::ConditionalRemoval over a ConditionAnd of PackedRGBComparison, as far as ProcessingPcd::getFilterRgb uses them
// (BuildModel processingpcd.cpp:112-141): GT and LT on the channels "r", "g", "b".  The conjunction is an open interval per
// channel, which is what ope_color_filter takes.
namespace ComparisonOps { enum CompareOp { GT, LT }; }

template <class PointT> class PackedRGBComparison {
 public:
  typedef std::shared_ptr<PackedRGBComparison> Ptr;
  // PCL compares the channel, a uint8 widened to double, with compare_val
  PackedRGBComparison(const std::string &component_name, ComparisonOps::CompareOp op, double compare_val)
      : channel_(component_name == "r" ? 0 : component_name == "g" ? 1 : component_name == "b" ? 2 : -1), op_(op), val_(compare_val) {
    if (channel_ < 0) std::fprintf(stderr, "[ope::PackedRGBComparison] unrecognized component name '%s'\n", component_name.c_str());
  }
  bool isCapable() const { return channel_ >= 0; }
  int channel_;
  ComparisonOps::CompareOp op_;
  double val_;
};

template <class PointT> class ConditionAnd {
 public:
  typedef std::shared_ptr<ConditionAnd> Ptr;
  void addComparison(const typename PackedRGBComparison<PointT>::Ptr &c) {
    if (!c || !c->isCapable()) { capable_ = false; return; }
    // an integer channel: c > v iff c > floor(v), c < v iff c < ceil(v); limits beyond a byte decide nothing
    const double v = c->val_ != c->val_ ? (c->op_ == ComparisonOps::GT ? 256.0 : -1.0) : std::fmin(std::fmax(c->val_, -1.0), 256.0);
    if (c->op_ == ComparisonOps::GT) lo_[c->channel_] = std::max(lo_[c->channel_], (int32_t)std::floor(v));
    else hi_[c->channel_] = std::min(hi_[c->channel_], (int32_t)std::ceil(v));
  }
  bool isCapable() const { return capable_; }
  int32_t lo_[3] = {-1, -1, -1}, hi_[3] = {256, 256, 256};
 private:
  bool capable_ = true;
};

template <class PointT> class ConditionalRemoval {
  static_assert(point_traits<PointT>::rgb_offset >= 0, "PackedRGBComparison needs a point type with a colour");
 public:
  explicit ConditionalRemoval(const typename ConditionAnd<PointT>::Ptr &condition) : condition_(condition) {}
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setKeepOrganized(bool keep) { keep_organized_ = keep; }
  // keep organized: the input's size, width and height; a failing point keeps its other fields and gets x = y = z = NaN
  // (PCL's user_filter_value_), and is_dense goes false when any point failed.  Otherwise the finite passing points, in order.
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    ope_ctx *ctx = default_context();
    if (ctx && input_ && condition_ && condition_->isCapable() && !input_->empty()) {
      const size_t n_in = input_->size();
      std::vector<uint32_t> rgb(n_in);
      for (size_t i = 0; i < n_in; ++i)
        std::memcpy(&rgb[i], reinterpret_cast<const unsigned char *>(&input_->points[i]) + point_traits<PointT>::rgb_offset, 4);
      auto dev = upload(*input_, false);
      std::vector<int32_t> idx(n_in);
      size_t n = 0;
      if (!dev->h || ope_cloud_set_rgb(ctx, dev->h, rgb.data()) != OPE_OK ||
          ope_color_filter(ctx, dev->h, condition_->lo_, condition_->hi_, idx.data(), &n) != OPE_OK) {
        log_error("ConditionalRemoval", ctx);
        n = 0;
      }
      if (keep_organized_) {
        tmp = *input_;
        size_t next = 0;
        for (size_t i = 0; i < n_in; ++i) {
          if (next < n && (size_t)idx[next] == i) { ++next; continue; }
          tmp.points[i].x = tmp.points[i].y = tmp.points[i].z = NAN;
        }
        if (n < n_in) tmp.is_dense = false;
      } else {
        tmp.points.reserve(n);
        for (size_t i = 0; i < n; ++i) {
          const PointT &p = input_->points[idx[i]];
          if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) tmp.points.push_back(p);
        }
        tmp.width = (uint32_t)tmp.points.size();
      }
    }
    out = std::move(tmp);
  }
 private:
  typename ConditionAnd<PointT>::Ptr condition_;
  typename PointCloud<PointT>::ConstPtr input_;
  bool keep_organized_ = false;
};

struct PointIndices {
  typedef std::shared_ptr<PointIndices> Ptr;
  typedef std::shared_ptr<const PointIndices> ConstPtr;
  std::vector<int> indices;
};

// pcl::MovingLeastSquares.  Upsampling NONE (ProcessingPcd::getSmooth, BuildModel/src/processingpcd.cpp:80-108): ope_mls_smooth,
// orders 0 to 2.  Upsampling VOXEL_GRID_DILATION (RegMeshPcd::generateMesh, regmeshpcd.cpp:275-292): ope_mls_upsample, orders 0 to 4.
// The output point takes the new xyz; its normal and curvature fields (if OutT has them) are written only when
// setComputeNormals(true), as in PCL; every other field OutT shares with InT (here: rgb) is copied from the input point
// (copyMissingFields).  getCorrespondingIndices: the input index of each output point (when upsampling, the nearest input point).
template <class InT, class OutT> class MovingLeastSquares {
 public:
  enum UpsamplingMethod { NONE, VOXEL_GRID_DILATION };
  MovingLeastSquares() { ope_mls_default_params(&p_); }
  void setInputCloud(const typename PointCloud<InT>::ConstPtr &c) { input_ = c; }
  void setComputeNormals(bool on) { p_.compute_normals = on ? 1 : 0; }
  void setPolynomialFit(bool on) { p_.polynomial_fit = on ? 1 : 0; }
  void setPolynomialOrder(int order) { p_.order = order; }
  template <class Tree> void setSearchMethod(const Tree &) {}   // accepted, unused: the device walks its own tree
  void setSearchRadius(double r) { p_.radius = r; p_.sqr_gauss_param = r * r; }
  void setSqrGaussParam(double g) { p_.sqr_gauss_param = g; }
  void setUpsamplingMethod(UpsamplingMethod m) { method_ = m; }
  void setDilationVoxelSize(float v) { voxel_size_ = v; }
  void setDilationIterations(int n) { dilation_iterations_ = n; }
  PointIndices::Ptr getCorrespondingIndices() const { return corresponding_; }
  void process(PointCloud<OutT> &out) {
    PointCloud<OutT> tmp;
    corresponding_ = std::make_shared<PointIndices>();
    ope_ctx *ctx = default_context();
    if (ctx && input_ && !input_->empty()) {
      auto dev = upload(*input_, false);
      size_t cap = method_ == NONE ? input_->size() : std::max<size_t>(8 * input_->size(), (size_t)1 << 16);   // upsampling: a guess, the call says what it needs
      std::vector<float> xyz(3 * cap), nrm(3 * cap), curv(cap);
      std::vector<int32_t> idx(cap);
      size_t n = 0;
      int rc = OPE_OK;
      if (dev->h && method_ == NONE) {
        rc = ope_mls_smooth(ctx, dev->h, &p_, xyz.data(), nrm.data(), curv.data(), idx.data(), &n);
      } else if (dev->h) {
        ope_mls_upsample_params u;
        ope_mls_upsample_default_params(&u);
        u.radius = p_.radius; u.polynomial_fit = p_.polynomial_fit; u.order = p_.order; u.sqr_gauss_param = p_.sqr_gauss_param;
        u.compute_normals = p_.compute_normals; u.voxel_size = voxel_size_; u.dilation_iterations = dilation_iterations_;
        rc = ope_mls_upsample(ctx, dev->h, &u, xyz.data(), nrm.data(), curv.data(), idx.data(), cap, &n);
        if (rc == OPE_EINVAL && n > cap) {
          cap = n;
          xyz.resize(3 * cap); nrm.resize(3 * cap); curv.resize(cap); idx.resize(cap);
          rc = ope_mls_upsample(ctx, dev->h, &u, xyz.data(), nrm.data(), curv.data(), idx.data(), cap, &n);
        }
      }
      if (rc != OPE_OK) { log_error("MovingLeastSquares", ctx); n = 0; }
      tmp.points.resize(n);
      corresponding_->indices.assign(idx.begin(), idx.begin() + n);
      constexpr ptrdiff_t rgb_in = point_traits<InT>::rgb_offset, rgb_out = point_traits<OutT>::rgb_offset, n_out = point_traits<OutT>::normal_offset;
      for (size_t i = 0; i < n; ++i) {
        OutT &o = tmp.points[i];
        o.x = xyz[3 * i]; o.y = xyz[3 * i + 1]; o.z = xyz[3 * i + 2];
        if (rgb_in >= 0 && rgb_out >= 0)
          std::memcpy(reinterpret_cast<unsigned char *>(&o) + rgb_out, reinterpret_cast<const unsigned char *>(&input_->points[idx[i]]) + rgb_in, 4);
        if (n_out >= 0 && p_.compute_normals) {
          std::memcpy(reinterpret_cast<unsigned char *>(&o) + n_out, &nrm[3 * i], 12);
          set_curvature(o, curv[i]);
        }
      }
      tmp.width = (uint32_t)n;
    }
    out = std::move(tmp);
  }
 private:
  static void set_curvature(PointXYZRGBNormal &o, float c) { o.curvature = c; }
  static void set_curvature(Normal &o, float c) { o.curvature = c; }
  template <class T> static void set_curvature(T &, float) {}
  typename PointCloud<InT>::ConstPtr input_;
  ope_mls_params p_;
  UpsamplingMethod method_ = NONE;
  float voxel_size_ = 1.0f;        // PCL's defaults
  int dilation_iterations_ = 0;
  PointIndices::Ptr corresponding_;
};

// pcl::copyPointCloud between point types: the fields both have (xyz; rgb when both carry it)
template <class A, class B> inline void copyPointCloud(const PointCloud<A> &in, PointCloud<B> &out) {
  PointCloud<B> tmp;
  tmp.points.resize(in.size());
  constexpr ptrdiff_t ra = point_traits<A>::rgb_offset, rb = point_traits<B>::rgb_offset;
  for (size_t i = 0; i < in.size(); ++i) {
    tmp.points[i].x = in.points[i].x; tmp.points[i].y = in.points[i].y; tmp.points[i].z = in.points[i].z;
    if (ra >= 0 && rb >= 0)
      std::memcpy(reinterpret_cast<unsigned char *>(&tmp.points[i]) + rb, reinterpret_cast<const unsigned char *>(&in.points[i]) + ra, 4);
  }
  tmp.width = in.width; tmp.height = in.height; tmp.is_dense = in.is_dense;
  out = std::move(tmp);
}

// ObjectSegmentationPlane::getClusters (objectsegmentationplane.cpp:79-93): the clusters of ope_euclidean_clusters, each as
// ORIGINAL indices ascending, by size descending then smallest index (PCL's order; see ope.h for the one documented difference)
template <class PointT> class EuclideanClusterExtraction {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  template <class Tree> void setSearchMethod(const Tree &) {}   // accepted, unused: the device builds its own grid
  void setClusterTolerance(double t) { p_.tolerance = t; }
  void setMinClusterSize(int n) { p_.min_size = n; }
  void setMaxClusterSize(int n) { p_.max_size = n; }
  void extract(std::vector<PointIndices> &clusters) {
    clusters.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || input_->empty()) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    const size_t n = input_->size();
    std::vector<int32_t> idx(n), off(n + 1);
    size_t k = 0;
    if (ope_euclidean_clusters(ctx, dev->h, &p_, n, &k, idx.data(), off.data(), nullptr) != OPE_OK) { log_error("EuclideanClusterExtraction", ctx); return; }
    clusters.resize(k);
    for (size_t c = 0; c < k; ++c) clusters[c].indices.assign(idx.begin() + off[c], idx.begin() + off[c + 1]);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  ope_cluster_params p_{0.0, 1, 0x7fffffff};   // PCL's defaults: no tolerance set (extract refuses), min 1, max INT_MAX
};

// pcl::RegionGrowing over normals (ope_region_grow), with the setters SegmentationRegionGrow::getSegmentRegGrow calls
// (segmentationregiongrow.cpp:28-39).  Smooth mode, the residual test off: PCL's defaults, which the reference leaves alone.
// extract on a cloud with a curvature above the threshold logs ope_region_grow's refusal and returns no clusters.
template <class PointT, class NormalT = Normal> class RegionGrowing {
 public:
  RegionGrowing() { p_.number_of_neighbours = 30; p_.normals_k = 30; p_.smoothness_threshold = 30.0 / 180.0 * M_PI; p_.curvature_threshold = 0.05;
                    p_.min_size = 1; p_.max_size = 0x7fffffff; }   // PCL's defaults
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setInputNormals(const typename PointCloud<NormalT>::ConstPtr &n) { normals_ = n; }
  template <class Tree> void setSearchMethod(const Tree &) {}   // accepted, unused: the device walks its own tree
  void setNumberOfNeighbours(unsigned int k) { p_.number_of_neighbours = (int32_t)k; }
  void setSmoothnessThreshold(float t) { p_.smoothness_threshold = t; }
  void setCurvatureThreshold(float c) { p_.curvature_threshold = c; }
  void setMinClusterSize(int n) { p_.min_size = n; }
  void setMaxClusterSize(int n) { p_.max_size = n; }
  void extract(std::vector<PointIndices> &clusters) {
    clusters.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || input_->empty() || !normals_ || normals_->size() != input_->size()) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    const size_t n = input_->size();
    std::vector<float> nrm(3 * n), curv(n);
    for (size_t i = 0; i < n; ++i) {
      const NormalT &q = normals_->points[i];
      nrm[3 * i] = q.normal_x; nrm[3 * i + 1] = q.normal_y; nrm[3 * i + 2] = q.normal_z;
      curv[i] = q.curvature;
    }
    std::vector<int32_t> idx(n), off(n + 1);
    size_t k = 0;
    if (ope_region_grow(ctx, dev->h, &p_, nrm.data(), curv.data(), n, &k, idx.data(), off.data(), nullptr) != OPE_OK) { log_error("RegionGrowing", ctx); return; }
    clusters.resize(k);
    for (size_t c = 0; c < k; ++c) clusters[c].indices.assign(idx.begin() + off[c], idx.begin() + off[c + 1]);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  typename PointCloud<NormalT>::ConstPtr normals_;
  ope_region_params p_;
};

// pcl::RegionGrowingRGB (ope_region_grow_rgb), with the setters SegmentationRegionGrow::getSegmentRegGrowRgb calls
// (segmentationregiongrow.cpp:97-106).  The point type carries the colours.  With setIndices the call runs on the selected points
// alone, as PCL's indexed search sees only those, and the clusters come back as indices into the input cloud.
typedef std::shared_ptr<std::vector<int>> IndicesPtr;
template <class PointT, class NormalT = Normal> class RegionGrowingRGB {
  static_assert(point_traits<PointT>::rgb_offset >= 0, "RegionGrowingRGB needs a point type with a colour");
 public:
  RegionGrowingRGB() { ope_region_rgb_default_params(&p_); }   // what the reference sets (:100-103), until a setter changes it
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setIndices(const IndicesPtr &indices) { indices_ = indices; }
  template <class Tree> void setSearchMethod(const Tree &) {}   // accepted, unused: the device walks its own tree
  void setDistanceThreshold(float t) { p_.distance_threshold = t; }
  void setPointColorThreshold(float t) { p_.point_color_threshold = t; }
  void setRegionColorThreshold(float t) { p_.region_color_threshold = t; }
  void setMinClusterSize(int n) { p_.min_size = n; }
  void setMaxClusterSize(int n) { p_.max_size = n; }
  void setNumberOfRegionNeighbours(unsigned int k) { p_.region_neighbour_number = (int32_t)k; }
  void extract(std::vector<PointIndices> &clusters) {
    clusters.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || input_->empty()) return;
    const size_t n_in = input_->size();
    std::vector<uint32_t> rgb(n_in);
    for (size_t i = 0; i < n_in; ++i)
      std::memcpy(&rgb[i], reinterpret_cast<const unsigned char *>(&input_->points[i]) + point_traits<PointT>::rgb_offset, 4);
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    if (ope_cloud_set_rgb(ctx, dev->h, rgb.data()) != OPE_OK) { log_error("RegionGrowingRGB", ctx); return; }
    CloudHandle sub;
    const ope_cloud *cloud = dev->h;
    size_t n = n_in;
    if (indices_) {
      std::vector<int32_t> sel(indices_->begin(), indices_->end());
      for (int32_t i : sel)
        if (i < 0 || (size_t)i >= n_in) { std::fprintf(stderr, "[ope::RegionGrowingRGB] an index lies outside the input cloud\n"); return; }
      if (sel.empty()) return;
      if (ope_cloud_select(ctx, dev->h, sel.data(), sel.size(), &sub.h) != OPE_OK) { log_error("RegionGrowingRGB", ctx); return; }
      cloud = sub.h;
      n = sel.size();
    }
    std::vector<int32_t> idx(n), off(n + 1);
    size_t k = 0;
    if (ope_region_grow_rgb(ctx, cloud, &p_, n, &k, idx.data(), off.data(), nullptr) != OPE_OK) { log_error("RegionGrowingRGB", ctx); return; }
    clusters.resize(k);
    for (size_t c = 0; c < k; ++c) {
      clusters[c].indices.assign(idx.begin() + off[c], idx.begin() + off[c + 1]);
      if (indices_)
        for (int &i : clusters[c].indices) i = (*indices_)[(size_t)i];
    }
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  IndicesPtr indices_;
  ope_region_rgb_params p_;
};

// pcl::VFHEstimation with the call shapes ObjectDetection::getVfhFeature uses (objectdetection.cpp:24-27) and PCL's given centroid /
// normal: one signature per cloud (ope_vfh_batch of one cluster).  The bin layout and normalisation are PCL's defaults; the
// setters that would change them (setNormalizeBins, setNormalizeDistance, setFillSizeComponent) do not exist here.
template <class PointInT, class PointNT = Normal, class PointOutT = VFHSignature308> class VFHEstimation {
 public:
  VFHEstimation() { ope_vfh_default_params(&p_); }
  void setInputCloud(const typename PointCloud<PointInT>::ConstPtr &c) { input_ = c; }
  void setInputNormals(const typename PointCloud<PointNT>::ConstPtr &n) { normals_ = n; }
  template <class Tree> void setSearchMethod(const Tree &) {}   // accepted, unused: VFH takes the whole cloud
  void setViewPoint(float x, float y, float z) { p_.viewpoint[0] = x; p_.viewpoint[1] = y; p_.viewpoint[2] = z; }
  void setUseGivenCentroid(bool use) { p_.use_given_centroid = use ? 1 : 0; }
  void setUseGivenNormal(bool use) { p_.use_given_normal = use ? 1 : 0; }
  template <class V3> void setCentroidToUse(const V3 &c) { p_.centroid[0] = c.v[0]; p_.centroid[1] = c.v[1]; p_.centroid[2] = c.v[2]; }
  template <class V3> void setNormalToUse(const V3 &n) { p_.normal[0] = n.v[0]; p_.normal[1] = n.v[1]; p_.normal[2] = n.v[2]; }
  void compute(PointCloud<PointOutT> &out) {
    out.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || !normals_ || normals_->size() != input_->size()) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    const size_t n = input_->size();
    std::vector<float> nrm(3 * n + 3);
    for (size_t i = 0; i < n; ++i) {
      const PointNT &q = normals_->points[i];
      nrm[3 * i] = q.normal_x; nrm[3 * i + 1] = q.normal_y; nrm[3 * i + 2] = q.normal_z;
    }
    ope_cloud *cl = dev->h;
    PointOutT sig;
    if (ope_cloud_set_normals(ctx, cl, nrm.data()) != OPE_OK || ope_vfh_batch(ctx, 1, &cl, &p_, sig.histogram, nullptr, nullptr) != OPE_OK) {
      log_error("VFHEstimation", ctx);
      return;
    }
    out.push_back(sig);   // "We only output _1_ signature"
  }
 private:
  typename PointCloud<PointInT>::ConstPtr input_;
  typename PointCloud<PointNT>::ConstPtr normals_;
  ope_vfh_params p_;
};

// ------------------------------------------------------------------------------------------ table-top segmentation
// The classes ObjectSegmentationPlane uses (objectsegmentationplane.cpp:36-71, 95-107, 169-214), with its call shapes.
struct ModelCoefficients {
  typedef std::shared_ptr<ModelCoefficients> Ptr;
  typedef std::shared_ptr<const ModelCoefficients> ConstPtr;
  std::vector<float> values;
};
enum SacModel { SACMODEL_PLANE = 0 };
enum SacMethod { SAC_RANSAC = 0 };
struct Vector3f {   // what setAxis takes; SACMODEL_PLANE never reads it
  float v[3];
  Vector3f(float x = 0.f, float y = 0.f, float z = 0.f) : v{x, y, z} {}
};

// pcl::SACSegmentation, SACMODEL_PLANE + SAC_RANSAC only (ope_plane_segment).  An empty `values` means no model, as in PCL.
template <class PointT> class SACSegmentation {
 public:
  SACSegmentation() { ope_plane_default_params(&p_); p_.optimize_coefficients = 0; }   // PCL's default: optimize_coefficients_ (true) is set by the caller at :39
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setModelType(int m) { model_ = m; }
  void setMethodType(int m) { method_ = m; }
  void setOptimizeCoefficients(bool on) { p_.optimize_coefficients = on ? 1 : 0; }
  void setDistanceThreshold(double t) { p_.distance_threshold = t; }
  void setMaxIterations(int n) { p_.max_iterations = n; }
  void setProbability(double pr) { p_.probability = pr; }
  void setAxis(const Vector3f &) {}      // no effect on SACMODEL_PLANE
  void setEpsAngle(double) {}            // no effect on SACMODEL_PLANE
  void setSeed(uint64_t s) { p_.seed = s; }
  void segment(PointIndices &inliers, ModelCoefficients &coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || model_ != SACMODEL_PLANE || method_ != SAC_RANSAC) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    std::vector<int32_t> idx(input_->size() + 1);
    float c[4];
    size_t n = 0;
    if (ope_plane_segment(ctx, dev->h, &p_, nullptr, 0, c, idx.data(), &n, nullptr, nullptr) != OPE_OK) { log_error("SACSegmentation", ctx); return; }
    ope_plane_stats st;
    if (ope_plane_last_stats(ctx, &st) != OPE_OK || !st.found) return;
    coefficients.values.assign(c, c + 4);
    inliers.indices.assign(idx.begin(), idx.begin() + n);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  ope_plane_params p_;
  int model_ = -1, method_ = SAC_RANSAC;
};

// pcl::ExtractIndices: the listed points in list order, or (negative) the others in input order.  Host-side: nothing is computed.
template <class PointT> class ExtractIndices {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setIndices(const PointIndices::ConstPtr &i) { indices_ = i; }
  void setNegative(bool n) { negative_ = n; }
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    if (input_ && indices_) {
      if (!negative_) {
        for (int i : indices_->indices) tmp.points.push_back(input_->points[i]);
      } else {
        std::vector<char> listed(input_->size(), 0);
        for (int i : indices_->indices) listed[i] = 1;
        for (size_t i = 0; i < input_->size(); ++i)
          if (!listed[i]) tmp.points.push_back(input_->points[i]);
      }
    }
    tmp.width = (uint32_t)tmp.points.size();
    tmp.is_dense = input_ ? input_->is_dense : true;
    out = std::move(tmp);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  PointIndices::ConstPtr indices_;
  bool negative_ = false;
};

// pcl::ProjectInliers with SACMODEL_PLANE (SampleConsensusModelPlane::projectPoints, copy_all_data false): the listed points
// projected, in list order, other fields copied.  Float arithmetic in the order DESIGN 4.11 fixes: n' = n / sqrt((a a + b b) + c c),
// dist = ((a' x + b' y) + c' z) + d, p - n' dist.  A handful of float operations per point: on the host.
template <class PointT> class ProjectInliers {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setModelType(int m) { model_ = m; }
  void setIndices(const PointIndices::ConstPtr &i) { indices_ = i; }
  void setModelCoefficients(const ModelCoefficients::ConstPtr &m) { coeff_ = m; }
  void filter(PointCloud<PointT> &out) {
    PointCloud<PointT> tmp;
    if (input_ && coeff_ && coeff_->values.size() == 4 && model_ == SACMODEL_PLANE) {
      const float a = coeff_->values[0], b = coeff_->values[1], c = coeff_->values[2], d = coeff_->values[3];
      volatile float aa = a * a, bb = b * b, cc = c * c;   // (volatile: every product rounded on its own, no contraction into the sums)
      volatile float s1 = aa + bb;
      const float len = std::sqrt(s1 + cc);
      const float ua = a / len, ub = b / len, uc = c / len;
      const size_t m = indices_ ? indices_->indices.size() : input_->size();
      tmp.points.reserve(m);
      for (size_t j = 0; j < m; ++j) {
        PointT p = input_->points[indices_ ? (size_t)indices_->indices[j] : j];
        volatile float t0 = ua * p.x, t1 = ub * p.y, t2 = uc * p.z;
        volatile float dist = t0 + t1; dist = dist + t2; dist = dist + d;
        volatile float mx = ua * dist, my = ub * dist, mz = uc * dist;
        p.x = p.x - mx; p.y = p.y - my; p.z = p.z - mz;
        tmp.points.push_back(p);
      }
    }
    tmp.width = (uint32_t)tmp.points.size();
    out = std::move(tmp);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_;
  PointIndices::ConstPtr indices_;
  ModelCoefficients::ConstPtr coeff_;
  int model_ = -1;
};

// pcl::getMinMax3D: componentwise extremes; points with a non-finite coordinate are skipped unless the cloud is dense
template <class PointT> inline void getMinMax3D(const PointCloud<PointT> &cloud, PointT &min_pt, PointT &max_pt) {
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (const PointT &p : cloud.points) {
    if (!cloud.is_dense && !(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) continue;
    const float v[3] = {p.x, p.y, p.z};
    for (int d = 0; d < 3; ++d) { if (v[d] < lo[d]) lo[d] = v[d]; if (v[d] > hi[d]) hi[d] = v[d]; }
  }
  min_pt.x = lo[0]; min_pt.y = lo[1]; min_pt.z = lo[2];
  max_pt.x = hi[0]; max_pt.y = hi[1]; max_pt.z = hi[2];
}

// pcl::ExtractPolygonalPrismData (ope_prism_extract): height limits 0 .. FLT_MAX and the viewpoint at the origin by default
template <class PointT> class ExtractPolygonalPrismData {
 public:
  void setInputCloud(const typename PointCloud<PointT>::ConstPtr &c) { input_ = c; }
  void setInputPlanarHull(const typename PointCloud<PointT>::ConstPtr &h) { hull_ = h; }
  void setHeightLimits(double lo, double hi) { lo_ = lo; hi_ = hi; }
  void segment(PointIndices &output) {
    output.indices.clear();
    ope_ctx *ctx = default_context();
    if (!ctx || !input_ || !hull_ || hull_->size() < 3) return;
    auto dev = upload(*input_, false);
    if (!dev->h) return;
    std::vector<float> hull(3 * hull_->size());
    for (size_t v = 0; v < hull_->size(); ++v) { hull[3 * v] = hull_->points[v].x; hull[3 * v + 1] = hull_->points[v].y; hull[3 * v + 2] = hull_->points[v].z; }
    std::vector<int32_t> idx(input_->size() + 1);
    size_t n = 0;
    if (ope_prism_extract(ctx, dev->h, hull.data(), hull_->size(), lo_, hi_, idx.data(), &n, nullptr, nullptr) != OPE_OK) { log_error("ExtractPolygonalPrismData", ctx); return; }
    output.indices.assign(idx.begin(), idx.begin() + n);
  }
 private:
  typename PointCloud<PointT>::ConstPtr input_, hull_;
  double lo_ = 0.0, hi_ = FLT_MAX;
};

template <class PointSource, class PointTarget, class FeatureT> class SampleConsensusInitialAlignment {
 public:
  SampleConsensusInitialAlignment() { ope_sacia_default_params(&p_); p_.max_iterations = 10; p_.nr_samples = 3; p_.k_correspondences = 10; p_.min_sample_dist = 0.f; p_.max_corr_dist = std::sqrt(DBL_MAX); }
  void setInputSource(const typename PointCloud<PointSource>::ConstPtr &c) { src_ = c; }
  void setInputTarget(const typename PointCloud<PointTarget>::ConstPtr &c) { tgt_ = c; }
  void setSourceFeatures(const typename PointCloud<FeatureT>::ConstPtr &f) { sf_ = f; }
  void setTargetFeatures(const typename PointCloud<FeatureT>::ConstPtr &f) { tf_ = f; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  void setNumberOfSamples(int n) { p_.nr_samples = n; }
  void setCorrespondenceRandomness(int k) { p_.k_correspondences = k; }
  void setMaxCorrespondenceDistance(double d) { p_.max_corr_dist = d; }
  void setMinSampleDistance(float d) { p_.min_sample_dist = d; }
  void setSeed(uint64_t s) { p_.seed = s; }  // PCL draws from unseeded rand(): made explicit here
  void align(PointCloud<PointSource> &output) {
    final_ = Matrix4f::Identity();
    converged_ = false;
    ope_ctx *ctx = default_context();
    if (!ctx || !src_ || !tgt_ || !sf_ || !tf_ || sf_->size() != src_->size() || tf_->size() != tgt_->size()) return;
    auto ds = upload(*src_, false), dt = upload(*tgt_, false);
    IndexHandle ix;
    if (!ds->h || !dt->h || ope_index_build(ctx, dt->h, nullptr, &ix.h) != OPE_OK) return;
    double err = 0;
    int32_t best = -1;
    if (ope_sacia(ctx, ds->h, &sf_->points[0].histogram[0], dt->h, ix.h, &tf_->points[0].histogram[0], &p_, nullptr,
                  final_.m, &err, &best) != OPE_OK) { log_error("SampleConsensusInitialAlignment", ctx); return; }
    converged_ = best >= 0;
    error_ = err;
    transformPointCloud(*src_, output, final_);
  }
  Matrix4f getFinalTransformation() const { return final_; }
  bool hasConverged() const { return converged_; }
  double getLowestError() const { return error_; }
 private:
  typename PointCloud<PointSource>::ConstPtr src_;
  typename PointCloud<PointTarget>::ConstPtr tgt_;
  typename PointCloud<FeatureT>::ConstPtr sf_, tf_;
  ope_sacia_params p_;
  Matrix4f final_ = Matrix4f::Identity();
  bool converged_ = false;
  double error_ = 0;
};

// pcl::SampleConsensusPrerejective with the calls of the reference's commented block (BuildModel poseestimator.cpp:92-108), on
// ope_prerejective.  The class defaults are PCL's (3 samples, correspondence randomness 2, similarity 0.9, inlier fraction 0,
// Registration's 10 iterations and unbounded distance).  getFitnessScore() is the winner's mean squared inlier distance.
template <class PointSource, class PointTarget, class FeatureT> class SampleConsensusPrerejective {
 public:
  SampleConsensusPrerejective() {
    ope_prerejective_default_params(&p_);
    p_.max_iterations = 10; p_.nr_samples = 3; p_.k_correspondences = 2; p_.similarity_threshold = 0.9f; p_.inlier_fraction = 0.f;
    p_.max_corr_dist = std::sqrt(DBL_MAX);
  }
  void setInputSource(const typename PointCloud<PointSource>::ConstPtr &c) { src_ = c; }
  void setInputTarget(const typename PointCloud<PointTarget>::ConstPtr &c) { tgt_ = c; }
  void setSourceFeatures(const typename PointCloud<FeatureT>::ConstPtr &f) { sf_ = f; }
  void setTargetFeatures(const typename PointCloud<FeatureT>::ConstPtr &f) { tf_ = f; }
  void setMaximumIterations(int n) { p_.max_iterations = n; }
  void setNumberOfSamples(int n) { p_.nr_samples = n; }
  void setCorrespondenceRandomness(int k) { p_.k_correspondences = k; }
  void setSimilarityThreshold(float s) { p_.similarity_threshold = s; }
  void setMaxCorrespondenceDistance(double d) { p_.max_corr_dist = d; }
  void setInlierFraction(float f) { p_.inlier_fraction = f; }
  void setSeed(uint64_t s) { p_.seed = s; }  // PCL draws from unseeded rand(): made explicit here
  void align(PointCloud<PointSource> &output) {
    final_ = Matrix4f::Identity();
    converged_ = false;
    inliers_.clear();
    error_ = FLT_MAX;
    best_ = -1;
    ope_ctx *ctx = default_context();
    if (!ctx || !src_ || !tgt_ || !sf_ || !tf_ || sf_->size() != src_->size() || tf_->size() != tgt_->size()) return;
    if (src_->empty() || tgt_->empty()) return;   // nothing to align (and no first feature row to point at)
    auto ds = upload(*src_, false), dt = upload(*tgt_, false);
    IndexHandle ix;
    if (!ds->h || !dt->h || ope_index_build(ctx, dt->h, nullptr, &ix.h) != OPE_OK) return;
    ope_prerejective_result r;
    std::vector<int32_t> idx(src_->size() + 1);
    if (ope_prerejective(ctx, ds->h, &sf_->points[0].histogram[0], dt->h, ix.h, &tf_->points[0].histogram[0], &p_, nullptr, &r,
                         idx.data()) != OPE_OK) { log_error("SampleConsensusPrerejective", ctx); return; }
    std::memcpy(final_.m, r.T, sizeof final_.m);
    converged_ = r.converged != 0;
    error_ = r.error;
    best_ = r.best_iteration;
    if (converged_) inliers_.assign(idx.begin(), idx.begin() + r.inliers);
    transformPointCloud(*src_, output, final_);
  }
  Matrix4f getFinalTransformation() const { return final_; }
  bool hasConverged() const { return converged_; }
  const std::vector<int> &getInliers() const { return inliers_; }
  double getFitnessScore() const { return error_; }
  int getBestIteration() const { return best_; }   // not PCL's: the winning iteration, -1 for none
 private:
  typename PointCloud<PointSource>::ConstPtr src_;
  typename PointCloud<PointTarget>::ConstPtr tgt_;
  typename PointCloud<FeatureT>::ConstPtr sf_, tf_;
  ope_prerejective_params p_;
  Matrix4f final_ = Matrix4f::Identity();
  bool converged_ = false;
  std::vector<int> inliers_;
  double error_ = FLT_MAX;
  int best_ = -1;
};

}  // namespace compat
}  // namespace ope
