// data_grabber.hpp — DetectAndLocalize's DataGrabber (datagrabber.cpp) over the façade:
//
//     ope::DataGrabber dataGrabber(euclidSensor, kinectSensor, astraSensor);          // rosinterface.cpp:70
//     cloudTarget = dataGrabber.rgbd2Pcl(imageDepth);                                 // :422
//
// rgbd2Pcl keeps the reference's signature with ope::DepthImage in place of cv::Mat (OpenCV is not assumed) and returns the host
// cloud the reference builds, by the reference's own loop on the host (convertHost below): no device, no context.
// rgbd2PclDevice is the form the per-frame path wants: the conversion runs on the device (ope_depth_to_cloud), already cropped to the workspace
// (getPassThrough, rosinterface.cpp:212), and goes straight into ObjectSegmentationPlane::getSegmentedObjectsOnPlane.
// The intrinsics are the reference's, with its quirk: cx / fx act on the image ROW and cy / fy on the COLUMN (include/ope.h,
// ope_depth_params).  With several sensors flagged the last of euclid, kinect, astra wins, as the chain of ifs in depthToMeter
// (:126-165) leaves it; with none the reference reads uninitialised values and this class refuses the frame.
#pragma once

#include <cstring>
#include <memory>
#include <vector>

#include "depth_io.hpp"
#include "pcl_compat.hpp"

namespace ope {

class DataGrabber {
 public:
  typedef compat::PointXYZRGB PointT;
  typedef compat::PointCloud<PointT> Cloud;

  DataGrabber(bool p_euclidSensor, bool p_kinectSensor, bool p_astraSensor) {
    if (p_euclidSensor) valid_ = ope_depth_sensor_params(OPE_SENSOR_EUCLID, &params_) == OPE_OK;
    if (p_kinectSensor) valid_ = ope_depth_sensor_params(OPE_SENSOR_KINECT, &params_) == OPE_OK;
    if (p_astraSensor) valid_ = ope_depth_sensor_params(OPE_SENSOR_ASTRA, &params_) == OPE_OK;
  }
  // a calibrated sensor: the caller's own values
  explicit DataGrabber(const ope_depth_params &params) : params_(params), valid_(true) {}
  const ope_depth_params &params() const { return params_; }

  // datagrabber.cpp:65-118: white points (:102-106), height / width the image's, kept after the erase (:69-70,114), is_dense (:71)
  Cloud::Ptr rgbd2Pcl(const DepthImage &p_imageDepth) {
    Cloud::Ptr cloud(new Cloud);
    if (!convertHost(p_imageDepth, *cloud, nullptr)) return cloud;
    const uint32_t rgb = ((uint32_t)255 << 16 | (uint32_t)255 << 8 | (uint32_t)255);
    for (auto &p : cloud->points) std::memcpy(&p.rgb, &rgb, 4);
    return cloud;
  }

  // :9-62: the colour of each point from the BGR image (3 bytes per pixel, rows of p_rgbStep bytes) through the pixel indices
  // (the ones ope_depth_to_cloud's out_pixel gives for the device frame)
  Cloud::Ptr rgbd2Pcl(const unsigned char *p_imageBgr, size_t p_rgbStep, const DepthImage &p_imageDepth) {
    Cloud::Ptr cloud(new Cloud);
    std::vector<int32_t> pixel;
    if (!p_imageBgr || !convertHost(p_imageDepth, *cloud, &pixel)) return cloud;
    for (size_t k = 0; k < cloud->points.size(); ++k) {
      const size_t i = (size_t)pixel[k] / p_imageDepth.cols, j = (size_t)pixel[k] % p_imageDepth.cols;
      const unsigned char *bgr = p_imageBgr + i * p_rgbStep + 3 * j;
      const uint32_t rgb = ((uint32_t)bgr[2] << 16 | (uint32_t)bgr[1] << 8 | (uint32_t)bgr[0]);   // :46-49
      std::memcpy(&cloud->points[k].rgb, &rgb, 4);
    }
    return cloud;
  }

  // BuildModel datagrabber.cpp:9-64, the reference's own signature with the images in place of its cv::Mat: the loop on the host
  Cloud::Ptr rgbd2Pcl(const ColorImage &p_imageRgb, const DepthImage &p_imageDepth) {
    if (p_imageRgb.rows != p_imageDepth.rows || p_imageRgb.cols != p_imageDepth.cols) {
      std::fprintf(stderr, "[ope::DataGrabber] the colour image is not of the depth image's size\n");
      return Cloud::Ptr(new Cloud);
    }
    return rgbd2Pcl(p_imageRgb.data.data(), p_imageRgb.step, p_imageDepth);
  }

  // The coloured frame as a device cloud (ope_depth_to_cloud_rgb), cropped to lo .. hi (both null: no crop): the points carry
  // their colours on the device, through the segmentation and the registration behind it.  An empty handle on failure.
  std::shared_ptr<compat::CloudHandle> rgbd2PclDevice(const ColorImage &p_imageRgb, const DepthImage &p_imageDepth, const float *lo = nullptr,
                                                      const float *hi = nullptr) {
    auto r = std::make_shared<compat::CloudHandle>();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !valid_ || p_imageDepth.empty() || p_imageRgb.rows != p_imageDepth.rows || p_imageRgb.cols != p_imageDepth.cols) {
      if (ctx && !valid_) std::fprintf(stderr, "[ope::DataGrabber] no sensor was selected\n");
      else if (ctx && !p_imageDepth.empty()) std::fprintf(stderr, "[ope::DataGrabber] the colour image is not of the depth image's size\n");
      return r;
    }
    if (ope_depth_to_cloud_rgb(ctx, p_imageDepth.data.data(), p_imageDepth.rows, p_imageDepth.cols, p_imageDepth.step, p_imageRgb.data.data(),
                               p_imageRgb.step, &params_, lo, hi, &r->h, nullptr, nullptr) != OPE_OK)
      compat::log_error("DataGrabber::rgbd2Pcl", ctx);
    return r;
  }

  // The frame as a device cloud, cropped to lo .. hi (both null: no crop); an empty handle on failure.  pixel (optional): the
  // pixel index row * cols + col of every point.
  std::shared_ptr<compat::CloudHandle> rgbd2PclDevice(const DepthImage &p_imageDepth, const float *lo = nullptr, const float *hi = nullptr,
                                                      std::vector<int32_t> *pixel = nullptr) {
    auto r = std::make_shared<compat::CloudHandle>();
    ope_ctx *ctx = compat::default_context();
    if (!ctx || !valid_ || p_imageDepth.empty()) {
      if (ctx && !valid_) std::fprintf(stderr, "[ope::DataGrabber] no sensor was selected\n");
      return r;
    }
    size_t n = 0;
    if (pixel) pixel->resize(p_imageDepth.rows * p_imageDepth.cols);
    if (ope_depth_to_cloud(ctx, p_imageDepth.data.data(), p_imageDepth.rows, p_imageDepth.cols, p_imageDepth.step, &params_, lo, hi, &r->h,
                           pixel ? pixel->data() : nullptr, &n) != OPE_OK) {
      compat::log_error("DataGrabber::rgbd2Pcl", ctx);
      n = 0;
    }
    if (pixel) pixel->resize(n);
    return r;
  }

 private:
  // rgbd2Pcl's loop (:77-110) with depthToMeter (:121-174) on the host: columns outer, rows inner, all float, one operation per
  // statement.  (No product here feeds a sum, so there is nothing a compiler could contract into a fused multiply-add.)  The
  // points carry no colour yet; pixel (optional): row * cols + col of every point.
  bool convertHost(const DepthImage &img, Cloud &cloud, std::vector<int32_t> *pixel) const {
    cloud.height = (uint32_t)img.rows;   // :69-70, kept after the erase (:114)
    cloud.width = (uint32_t)img.cols;
    cloud.is_dense = true;               // :71
    if (img.empty()) return false;
    if (!valid_) { std::fprintf(stderr, "[ope::DataGrabber] no sensor was selected\n"); return false; }
    for (size_t j = 0; j < img.cols; ++j) {
      const float colOff = (float)j - params_.c_col;
      for (size_t i = 0; i < img.rows; ++i) {
        const uint16_t d = img.at(i, j);
        const float Z = (float)d / params_.scale;
        if (d == 0 || (double)Z > params_.z_max) continue;   // :90 with :127,142,155
        const float rowOff = (float)i - params_.c_row;
        const float rowZ = rowOff * Z;
        const float colZ = colOff * Z;
        PointT p;
        p.y = rowZ / params_.f_row;   // the row is p_FeatX, and X goes into .y (:86,98)
        p.x = colZ / params_.f_col;
        p.z = Z;
        cloud.points.push_back(p);
        if (pixel) pixel->push_back((int32_t)(i * img.cols + j));
      }
    }
    return true;
  }

  ope_depth_params params_{};
  bool valid_ = false;
};

}  // namespace ope
