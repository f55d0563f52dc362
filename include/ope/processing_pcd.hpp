// processing_pcd.hpp — ope::ProcessingPcd, the reference's helper class for clouds before and after registration
// (BuildModel/src/processingpcd.cpp, DetectAndLocalize/src/processingpcd.cpp), each method a few lines over the façade of
// pcl_compat.hpp, exactly as the reference writes them over PCL:
//   getPassThrough    :8-41    pcl::PassThrough on z, then y, then x            (ope_pass_through)
//   getDownSampled    :45-59   pcl::VoxelGrid with a cubic leaf                  (ope_voxel_grid / ope_voxel_grid_rgb)
//   getOutlierRemove  :62-78   pcl::StatisticalOutlierRemoval, meanK 30          (ope_statistical_outlier_removal)
//   getSmooth         :81-108  pcl::MovingLeastSquares, polynomial fit, no normals (ope_mls_smooth)
//   getFilterRgb      :112-141 pcl::ConditionalRemoval over PackedRGBComparison, organized (ope_color_filter)
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

  // min < channel < max for r, g and b (strict); the output keeps the input's size, width and height, a failing point its colour
  // with x = y = z = NaN
  Cloud::Ptr getFilterRgb(Cloud::Ptr p_cloud, int p_minR, int p_maxR, int p_minG, int p_maxG, int p_minB, int p_maxB) {
    Cloud::Ptr cloudFiltered(new Cloud);
    typedef compat::PackedRGBComparison<PointTProc> Comparison;
    compat::ConditionAnd<PointTProc>::Ptr colorCond(new compat::ConditionAnd<PointTProc>());
    colorCond->addComparison(Comparison::Ptr(new Comparison("r", compat::ComparisonOps::LT, p_maxR)));
    colorCond->addComparison(Comparison::Ptr(new Comparison("r", compat::ComparisonOps::GT, p_minR)));
    colorCond->addComparison(Comparison::Ptr(new Comparison("g", compat::ComparisonOps::LT, p_maxG)));
    colorCond->addComparison(Comparison::Ptr(new Comparison("g", compat::ComparisonOps::GT, p_minG)));
    colorCond->addComparison(Comparison::Ptr(new Comparison("b", compat::ComparisonOps::LT, p_maxB)));
    colorCond->addComparison(Comparison::Ptr(new Comparison("b", compat::ComparisonOps::GT, p_minB)));
    compat::ConditionalRemoval<PointTProc> condRem(colorCond);
    condRem.setInputCloud(p_cloud);
    condRem.setKeepOrganized(true);
    condRem.filter(*cloudFiltered);
    return cloudFiltered;
  }
};

}  // namespace ope
