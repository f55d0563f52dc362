// object_detection.hpp — the reference's ObjectDetection (BuildModel/src/objectdetection.cpp, include/objectdetection.h) on the
// device:
//
//     ope::ObjectDetection det;
//     det.loadTrainData("TrainData");                       // training_data.list + training_data.f32
//     std::string name;
//     bool found = det.getObjectName(cluster, name);        // one cluster, the reference's call
//     det.getObjectNames(deviceClusters, names);            // every cluster of a frame in one ope_vfh_recognise
//
// getVfhFeature (:9-29): NormalEstimation with k = 30, then pcl::VFHEstimation; here one ope_vfh_batch that estimates the normals.
// getObjectName (:150-193): the 15 nearest trained signatures by chi-square distance, threshold 120, the name up to the first '_'.
// The table on disk: the reference writes training_data.list (one name per line), training_data.h5 (HDF5) and FLANN's kdtree.idx.
// Here the list is the same file and the signatures lie beside it in training_data.f32: m x 308 little-endian floats, row i the
// signature of line i, nothing else.  There is no tree file: the search is exact (ope.h, ope_vfh_match).
// loadHist / loadFeatureModels read one-point "vfh" PCD files in the reference; here getkdTreeRepresentation takes the signatures
// and names directly (addModel) and writes the table.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "pcl_compat.hpp"

namespace ope {

typedef std::pair<std::string, std::vector<float>> vfhModel;

class ObjectDetection {
 public:
  typedef compat::PointXYZRGB PointTDet;
  typedef compat::PointCloud<PointTDet> Cloud;
  typedef compat::PointCloud<compat::VFHSignature308> VfhCloud;

  ObjectDetection() { ope_vfh_default_params(&params_); }
  ~ObjectDetection() { if (db_) ope_vfh_db_free(db_); }
  ObjectDetection(const ObjectDetection &) = delete;
  ObjectDetection &operator=(const ObjectDetection &) = delete;

  int k = 15;             // :156
  double thresh = 120;    // :157
  ope_vfh_params &params() { return params_; }
  const std::vector<vfhModel> &getModels() const { return models_; }
  // the 1-NN distance the last getObjectName printed (the reference's "The distance of 1-NN is"), i.e. neighbour [1]'s
  float lastDistance() const { return lastDistance_; }

  // :9-29
  void getVfhFeature(Cloud::Ptr p_cloud, VfhCloud::Ptr &p_cloudVfh) {
    p_cloudVfh = VfhCloud::Ptr(new VfhCloud);
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !p_cloud) return;
    auto dev = compat::upload(*p_cloud, false);
    if (!dev->h) return;
    ope_cloud *cl = dev->h;
    compat::VFHSignature308 sig;
    if (ope_vfh_batch(ctx, 1, &cl, &params_, sig.histogram, nullptr, nullptr) != OPE_OK) { compat::log_error("getVfhFeature", ctx); return; }
    p_cloudVfh->push_back(sig);
  }

  // one more trained signature (what loadHist appends to `models`)
  void addModel(const std::string &name, const float *histogram308) {
    models_.push_back(vfhModel(name, std::vector<float>(histogram308, histogram308 + 308)));
  }

  // :32-76, the training stage: the models added so far (addModel) are written as training_data.list / training_data.f32 under
  // `dir` and become the table in use.
  bool getkdTreeRepresentation(const std::string &dir) {
    if (models_.empty()) return false;
    std::ofstream fs((dir + "/training_data.list").c_str());
    std::ofstream fb((dir + "/training_data.f32").c_str(), std::ios::binary);
    if (!fs || !fb) return false;
    for (const vfhModel &m : models_) {
      fs << m.first << "\n";
      fb.write(reinterpret_cast<const char *>(m.second.data()), 308 * sizeof(float));
    }
    return fs.good() && fb.good() && buildTable();
  }

  // :232-264
  bool loadTrainData(const std::string &dir = "../3DModel/TrainData") {
    models_.clear();
    if (!loadFileList(models_, dir + "/training_data.list")) {
      std::fprintf(stderr, "Could not find training data models files %s!\n", (dir + "/training_data.list").c_str());
      return false;
    }
    std::ifstream fb((dir + "/training_data.f32").c_str(), std::ios::binary);
    for (vfhModel &m : models_) {
      m.second.resize(308);
      if (!fb.read(reinterpret_cast<char *>(m.second.data()), 308 * sizeof(float))) {
        std::fprintf(stderr, "training_data.f32 holds fewer rows than training_data.list has names\n");
        models_.clear();
        return false;
      }
    }
    return buildTable();
  }

  // :270-289
  bool loadFileList(std::vector<vfhModel> &models, const std::string &filename) {
    std::ifstream fs(filename.c_str());
    if (!fs.is_open() || fs.fail()) return false;
    std::string line;
    while (std::getline(fs, line)) {
      if (line.empty()) continue;
      vfhModel m;
      m.first = line;
      models.push_back(m);
    }
    return true;
  }

  // :150-193
  bool getObjectName(Cloud::Ptr p_cloud, std::string &p_objName) {
    p_objName = "ObjectNotFound";
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !db_ || !p_cloud) return false;
    auto dev = compat::upload(*p_cloud, false);
    if (!dev->h) return false;
    std::vector<const compat::CloudHandle *> one(1, dev.get());
    std::vector<std::string> names;
    std::vector<float> dist;
    if (!recognise(one, names, dist)) return false;
    p_objName = names[0];
    return names[0] != "ObjectNotFound";
  }

  // Every cluster of a frame in one ope_vfh_recognise; names[i] as getObjectName gives it ("ObjectNotFound" at or above the
  // threshold); distances (optional): the distance getObjectName compares, per cluster.
  bool getObjectNames(const std::vector<std::shared_ptr<compat::CloudHandle>> &clusters, std::vector<std::string> &names,
                      std::vector<float> *distances = nullptr) {
    std::vector<const compat::CloudHandle *> cl;
    for (const auto &c : clusters) cl.push_back(c.get());
    std::vector<float> dist;
    const bool ok = recognise(cl, names, dist);
    if (distances) *distances = dist;
    return ok;
  }
  // the same for clusters on the host (any point type with x, y, z): uploaded first
  template <class PointT> bool getObjectNames(const std::vector<std::shared_ptr<compat::PointCloud<PointT>>> &clusters,
                                              std::vector<std::string> &names, std::vector<float> *distances = nullptr) {
    std::vector<std::shared_ptr<compat::CloudHandle>> dev;
    for (const auto &c : clusters) {
      dev.push_back(c ? compat::upload(*c, false) : std::make_shared<compat::CloudHandle>());
      if (!dev.back()->h) { names.clear(); return false; }
    }
    return getObjectNames(dev, names, distances);
  }

 private:
  bool buildTable() {
    ope_ctx *ctx = compat::default_context();
    if (!ctx) return false;
    if (db_) { ope_vfh_db_free(db_); db_ = nullptr; }
    std::vector<float> rows;
    for (const vfhModel &m : models_) rows.insert(rows.end(), m.second.begin(), m.second.end());
    if (ope_vfh_db_create(ctx, rows.data(), models_.size(), &db_) != OPE_OK) { compat::log_error("loadTrainData", ctx); return false; }
    return true;
  }

  bool recognise(const std::vector<const compat::CloudHandle *> &clusters, std::vector<std::string> &names, std::vector<float> &dist) {
    names.clear();
    dist.clear();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !db_ || clusters.empty()) return false;
    std::vector<ope_cloud *> hs;
    for (const compat::CloudHandle *c : clusters) hs.push_back(c ? c->h : nullptr);
    const size_t n = hs.size();
    std::vector<int32_t> idx(n * (size_t)k);
    std::vector<float> d(n * (size_t)k);
    if (ope_vfh_recognise(ctx, db_, n, hs.data(), &params_, k, nullptr, idx.data(), d.data()) != OPE_OK) {
      compat::log_error("getObjectName", ctx);
      return false;
    }
    for (size_t i = 0; i < n; ++i) {
      // The reference reads k_distances[0][1] and k_indices[0][1] (:179-184): the SECOND nearest row, although its message and
      // comment speak of the first neighbour.  Kept: a table of one row names nothing.
      const int32_t row = k > 1 ? idx[i * (size_t)k + 1] : -1;
      const float dd = k > 1 ? d[i * (size_t)k + 1] : HUGE_VALF;
      lastDistance_ = dd;
      dist.push_back(dd);
      if (row >= 0 && dd < thresh) {
        const std::string &full = models_[(size_t)row].first;
        names.push_back(full.substr(0, full.find('_')));   // boost::split(..., "_") then fieldString.at(0)
      } else {
        names.push_back("ObjectNotFound");
      }
    }
    return true;
  }

  ope_vfh_params params_;
  std::vector<vfhModel> models_;
  ope_vfh_db *db_ = nullptr;
  float lastDistance_ = HUGE_VALF;
};

}  // namespace ope
