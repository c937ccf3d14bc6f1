/*
 * Declaration-only stand-in for <pcl/common/transforms.h>. TEST INFRASTRUCTURE ONLY (see ../point_cloud.h).
 * pcl::transformPointCloud is DECLARED here and nothing more, so the reference's translation units cannot inline or contract
 * it under their own flags. The one definition is ours: ../../pcl_transform_standin.cpp, PCL 1.8's expression restated,
 * parity with PCL unpinned.
 */
#ifndef PCS_REF_STANDIN_PCL_TRANSFORMS_H
#define PCS_REF_STANDIN_PCL_TRANSFORMS_H
#include <pcl/point_cloud.h>

namespace pcl {

template <class PointT>
void transformPointCloud(const PointCloud<PointT>& cloud_in, PointCloud<PointT>& cloud_out, const Eigen::Matrix4f& transform);

}  // namespace pcl
#endif
