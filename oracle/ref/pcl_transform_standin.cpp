/*
 * pcl_transform_standin.cpp — the ONE definition the compiled centre programs need from PCL. TEST INFRASTRUCTURE ONLY.
 *
 * RESTATED, UNPINNED: PCL is third-party and absent from the reference checkout. This is PCL 1.8's
 * pcl::transformPointCloud (common/impl/transforms.hpp) restated from its published source: per row r,
 *     ((m(r,0) * x + m(r,1) * y) + m(r,2) * z) + m(r,3)
 * in float, and where the cloud is not dense a point with a non-finite coordinate is left as it is.
 * Built on its own with -O2 -ffp-contract=off (../Makefile), so that neither translation unit's flags (-mfma for the client)
 * contract it. Reached only through the harness's update_and_send; for the order-independent matrices of
 * tests/ref_centre_cases.py its association does not matter.
 */
#include <cmath>

#include <pcl/common/transforms.h>

namespace pcl {

template <class PointT>
void transformPointCloud(const PointCloud<PointT>& cloud_in, PointCloud<PointT>& cloud_out, const Eigen::Matrix4f& transform)
{
    if (&cloud_in != &cloud_out) {
        cloud_out.points = cloud_in.points;
        cloud_out.width = cloud_in.width;
        cloud_out.height = cloud_in.height;
        cloud_out.is_dense = cloud_in.is_dense;
    }
    const float* m = transform.m;
    for (std::size_t i = 0; i < cloud_out.points.size(); i++) {
        const float x = cloud_in.points[i].x, y = cloud_in.points[i].y, z = cloud_in.points[i].z;
        if (!cloud_in.is_dense && (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)))
            continue;
        cloud_out.points[i].x = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        cloud_out.points[i].y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        cloud_out.points[i].z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    }
}

template void transformPointCloud<PointXYZRGB>(const PointCloud<PointXYZRGB>&, PointCloud<PointXYZRGB>&, const Eigen::Matrix4f&);
template void transformPointCloud<PointXYZ>(const PointCloud<PointXYZ>&, PointCloud<PointXYZ>&, const Eigen::Matrix4f&);

}  // namespace pcl
