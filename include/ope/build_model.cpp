// build_model.cpp — config C5 from files, BuildModel's own sequence (BuildModel/src/main.cpp:113-153 load the frames,
// :207 registerPointClouds, :221 savePCDFile of the aligned cloud) with pcl:: replaced by the façade:
//
//   build_model <out.pcd> <corrRejThresh> <maxIter> <frame0.pcd> <frame1.pcd> [...]
//
// and from the sensor's images, BuildModel's whole sequence (rgbd2Pcl(rgb, depth) of datagrabber.cpp:9-64 in front of
// main.cpp:171-198: getPassThrough, getSegmentedObjectsOnPlane, cluster 0), every step on the device:
//
//   build_model --scan <kinect|astra|euclid> --limits x0 x1 y0 y1 z0 z1 <out.pcd> <corrRejThresh> <maxIter> <depth0.pgm> <rgb0.ppm> [...]
//
// `--smooth R` anywhere on a --scan line (opt-in) applies getSmooth with radius R to the finished, device-resident model before its
// download, the line the reference keeps at regmeshpcd.cpp:264-266.  Without --scan the model is a host cloud: --smooth is a usage
// error there (status 2).
//
// `--mesh-cloud OUT.pcd` anywhere on either line (opt-in) also runs the head of generateMesh on the aligned cloud, as main.cpp:227-235
// does after saving it (copyPointCloud to PointXYZ, then regmeshpcd.cpp:275-303: MLS upsampling, normals k = 20), and writes the cloud
// the triangulation would get, `FIELDS x y z rgb normal_x normal_y normal_z curvature`, to OUT.pcd.
//
// Depth images are 16-bit binary PGM, colour images 8-bit binary PPM (depth_io.hpp).  A frame without a supporting plane or
// without a cluster ends the program with a message and status 5 (the reference's cloudClusterVector.at(0) throws).
// Prints one `pair <k> iterations <n> converged <0|1> fitness <f> T <16 floats, column-major>` line per registration.
// Status: 2 usage, 3 a file that does not load, 4 the model could not be written, 5 a frame without plane or cluster, 6 a
// device failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "data_grabber.hpp"
#include "object_segmentation_plane.hpp"
#include "pcd_io.hpp"
#include "reg_mesh_pcd.hpp"

namespace pcl = ope::compat;

static int usage(const char *prog) {
  std::fprintf(stderr,
               "usage: %s <out.pcd> <corrRejThresh> <maxIter> <frame0.pcd> <frame1.pcd> [...]\n"
               "       %s --scan <kinect|astra|euclid> --limits x0 x1 y0 y1 z0 z1 <out.pcd> <corrRejThresh> <maxIter> <depth0.pgm> <rgb0.ppm> "
               "[<depth1.pgm> <rgb1.ppm> ...]\n"
               "       --smooth R anywhere on a --scan line: smooth the finished model (moving least squares, radius R) before it is written\n"
               "       --mesh-cloud OUT.pcd anywhere: also write the upsampled cloud with normals that generateMesh hands to the triangulation\n",
               prog, prog);
  return 2;
}

static void print_pairs(const ope::RegMeshPcd &reg) {
  for (size_t k = 0; k < reg.pairs().size(); ++k) {
    const auto &p = reg.pairs()[k];
    std::printf("pair %zu iterations %d converged %d fitness %.12g T", k, p.iterations, (int)p.converged, p.fitness);
    for (int i = 0; i < 16; ++i) std::printf(" %.9g", (double)p.T.m[i]);
    std::printf("\n");
  }
}

// main.cpp:227-235 up to the triangulation: the aligned cloud as PointXYZ, generateMesh's upsampling and normals, saved to `path`
template <class CloudT> static int write_mesh_cloud(ope::RegMeshPcd &reg, const CloudT &aligned, const std::string &path) {
  if (path.empty()) return 0;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloudAlignedXYZ(new pcl::PointCloud<pcl::PointXYZ>);
  pcl::copyPointCloud(aligned, *cloudAlignedXYZ);                               // :232
  auto cloudWithNormals = reg.generateMeshCloud(cloudAlignedXYZ);               // :233 -> regmeshpcd.cpp:275-303
  if (cloudWithNormals->empty()) return 6;
  if (pcl::io::savePCDFile(path, *cloudWithNormals, true) != 0) return 4;
  std::printf("Saved %zu upsampled points with normals to %s.\n", cloudWithNormals->size(), path.c_str());
  return 0;
}

// build_model --scan: argv[2] the sensor, argv[3] "--limits", argv[4..9] the box, argv[10..12] out / thresh / iterations, then the pairs
static int scan_main(int argc, char **argv, float smooth, const std::string &mesh_cloud) {
  if (argc < 15 || (argc - 13) % 2 != 0 || std::strcmp(argv[3], "--limits") != 0) return usage(argv[0]);
  const std::string sensor = argv[2];
  if (sensor != "kinect" && sensor != "astra" && sensor != "euclid") return usage(argv[0]);
  float lo[3], hi[3];
  for (int d = 0; d < 3; ++d) {
    char *end = nullptr;
    lo[d] = std::strtof(argv[4 + 2 * d], &end);
    if (end == argv[4 + 2 * d] || *end) return usage(argv[0]);
    hi[d] = std::strtof(argv[5 + 2 * d], &end);
    if (end == argv[5 + 2 * d] || *end) return usage(argv[0]);
  }
  const std::string out_path = argv[10];
  const float corrRejThresh = (float)std::atof(argv[11]);
  const int maxIter = std::atoi(argv[12]);
  ope::DataGrabber dataGrabber(sensor == "euclid", sensor == "kinect", sensor == "astra");
  ope::ObjectSegmentationPlane objSegPlane;
  std::vector<std::shared_ptr<pcl::CloudHandle>> cloudVectorSeg;
  for (int i = 13; i + 1 < argc; i += 2) {
    ope::DepthImage imageDepth;
    ope::ColorImage imageRgb;
    if (ope::io::loadPGM(argv[i], imageDepth) != 0 || ope::io::loadPPM(argv[i + 1], imageRgb) != 0) return 3;
    auto frame = dataGrabber.rgbd2PclDevice(imageRgb, imageDepth, lo, hi);   // rgbd2Pcl + getPassThrough (main.cpp:180)
    if (!frame->h) return 6;
    std::printf("%zu\n", ope_cloud_size(frame->h));                          // :177
    const bool isPlane = objSegPlane.segmentOnDevice(*frame);               // :181, no host clouds
    if (objSegPlane.deviceFailed()) return 6;
    if (!isPlane) { std::fprintf(stderr, "build_model: no supporting plane in %s\n", argv[i]); return 5; }
    if (objSegPlane.deviceClusters().empty()) { std::fprintf(stderr, "build_model: no cluster on the plane in %s\n", argv[i]); return 5; }
    cloudVectorSeg.push_back(objSegPlane.deviceClusters()[0]);              // :182
  }
  std::printf("Finished segmentation of %zu point clouds!\n", cloudVectorSeg.size());
  ope::RegMeshPcd regMeshPcd;
  regMeshPcd.setSmoothRadius(smooth);
  auto cloudAligned = regMeshPcd.registerPointClouds(cloudVectorSeg, 0.005f, corrRejThresh, maxIter);   // :207
  if (cloudAligned->empty()) return 6;
  print_pairs(regMeshPcd);
  if (pcl::io::savePCDFile(out_path, *cloudAligned, true) != 0) return 4;   // :221
  std::printf("Saved %zu data points to %s.\n", cloudAligned->size(), out_path.c_str());
  return write_mesh_cloud(regMeshPcd, *cloudAligned, mesh_cloud);
}

int main(int argc, char **argv) {
  std::string mesh_cloud;   // --mesh-cloud OUT.pcd, taken out of the line
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--mesh-cloud") == 0) {
      if (i + 1 >= argc || !argv[i + 1][0]) return usage(argv[0]);
      mesh_cloud = argv[i + 1];
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2;
      break;
    }
  float smooth = 0.f;   // --smooth R, taken out of the line
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--smooth") == 0) {
      char *end = nullptr;
      if (i + 1 >= argc) return usage(argv[0]);
      smooth = std::strtof(argv[i + 1], &end);
      if (end == argv[i + 1] || *end || !(smooth > 0.f)) return usage(argv[0]);
      for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
      argc -= 2;
      break;
    }
  if (argc > 1 && std::strcmp(argv[1], "--scan") == 0) return scan_main(argc, argv, smooth, mesh_cloud);
  if (smooth > 0.f) return usage(argv[0]);
  if (argc < 6) return usage(argv[0]);
  const std::string out_path = argv[1];
  const float corrRejThresh = (float)std::atof(argv[2]);
  const int maxIter = std::atoi(argv[3]);
  typedef ope::RegMeshPcd::PointTReg PointTReg;
  std::vector<pcl::PointCloud<PointTReg>::Ptr> cloudVector;
  for (int i = 4; i < argc; ++i) {
    pcl::PointCloud<PointTReg>::Ptr c(new pcl::PointCloud<PointTReg>);
    if (pcl::io::loadPCDFile(argv[i], *c) != 0) return 3;
    cloudVector.push_back(c);
  }
  ope::RegMeshPcd regMeshPcd;
  pcl::PointCloud<PointTReg>::Ptr cloudAligned = regMeshPcd.registerPointClouds(cloudVector, 0.005f, corrRejThresh, maxIter);   // main.cpp:207
  print_pairs(regMeshPcd);
  if (pcl::io::savePCDFile(out_path, *cloudAligned, true) != 0) return 4;   // main.cpp:221
  std::printf("Saved %zu data points to %s.\n", cloudAligned->size(), out_path.c_str());
  return write_mesh_cloud(regMeshPcd, *cloudAligned, mesh_cloud);
}
