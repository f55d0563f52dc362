// processing_pcd.hpp — ope::ProcessingPcd, the reference's helper class for clouds before and after registration
// (BuildModel/src/processingpcd.cpp, DetectAndLocalize/src/processingpcd.cpp), each method a few lines over the façade of
// pcl_compat.hpp, exactly as the reference writes them over PCL:
//   getPassThrough    :8-41    pcl::PassThrough on z, then y, then x            (ope_pass_through)
//   getDownSampled    :45-59   pcl::VoxelGrid with a cubic leaf                  (ope_voxel_grid / ope_voxel_grid_rgb)
//   getOutlierRemove  :62-78   pcl::StatisticalOutlierRemoval, meanK 30          (ope_statistical_outlier_removal)
//   getSmooth         :81-108  pcl::MovingLeastSquares, polynomial fit, no normals (ope_mls_smooth)
// getFilterRgb (:112-) is not built: the colour filter has no device entry point yet.
#pragma once

#include "pcl_compat.hpp"

namespace ope {

typedef compat::PointXYZRGB PointTProc;

class ProcessingPcd {
 public:
  typedef compat::PointCloud<PointTProc> Cloud;

  Cloud::Ptr getPassThrough(Cloud::Ptr p_cloud, float p_minX, float p_maxX, float p_minY, float p_maxY, float p_minZ, float p_maxZ) {
    Cloud::Ptr cloudFilteredZ(new Cloud), cloudFilteredZY(new Cloud), cloudFilteredZYX(new Cloud);
    compat::PassThrough<PointTProc> passThrough;
    passThrough.setInputCloud(p_cloud);
    passThrough.setFilterFieldName("z");
    passThrough.setFilterLimits(p_minZ, p_maxZ);
    passThrough.filter(*cloudFilteredZ);
    passThrough.setInputCloud(cloudFilteredZ);
    passThrough.setFilterFieldName("y");
    passThrough.setFilterLimits(p_minY, p_maxY);
    passThrough.filter(*cloudFilteredZY);
    passThrough.setInputCloud(cloudFilteredZY);
    passThrough.setFilterFieldName("x");
    passThrough.setFilterLimits(p_minX, p_maxX);
    passThrough.filter(*cloudFilteredZYX);
    return cloudFilteredZYX;
  }

  Cloud::Ptr getDownSampled(Cloud::Ptr p_cloud, float p_leafSize) {
    Cloud::Ptr cloudDownSampled(new Cloud);
    compat::VoxelGrid<PointTProc> voxGrid;
    voxGrid.setInputCloud(p_cloud);
    voxGrid.setLeafSize(p_leafSize, p_leafSize, p_leafSize);
    voxGrid.filter(*cloudDownSampled);
    return cloudDownSampled;
  }

  Cloud::Ptr getOutlierRemove(Cloud::Ptr p_cloud, float p_threshold) {
    Cloud::Ptr cloudSor(new Cloud);
    compat::StatisticalOutlierRemoval<PointTProc> sor;
    sor.setInputCloud(p_cloud);
    sor.setMeanK(30);
    sor.setStddevMulThresh(p_threshold);
    sor.filter(*cloudSor);
    return cloudSor;
  }

  Cloud::Ptr getSmooth(Cloud::Ptr p_cloud, float p_searchRadius) {
    Cloud::Ptr cloudSmooth(new Cloud);
    compat::search::KdTree<PointTProc>::Ptr kdtree(new compat::search::KdTree<PointTProc>);
    compat::PointCloud<compat::PointXYZRGBNormal> cloudNormal;   // (mls outputs a cloud with normals)
    compat::MovingLeastSquares<PointTProc, compat::PointXYZRGBNormal> mls;
    mls.setInputCloud(p_cloud);
    mls.setComputeNormals(false);
    mls.setPolynomialFit(true);
    mls.setSearchMethod(kdtree);
    mls.setSearchRadius(p_searchRadius);
    mls.process(cloudNormal);
    compat::copyPointCloud(cloudNormal, *cloudSmooth);
    return cloudSmooth;
  }
};

}  // namespace ope
