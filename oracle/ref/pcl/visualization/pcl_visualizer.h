/*
 * Declaration-only stand-in for <pcl/visualization/pcl_visualizer.h>. TEST INFRASTRUCTURE ONLY (see ../point_cloud.h).
 * A visualiser whose methods do nothing: the reference constructs one at load time and touches it only under `-v`,
 * which the harness never sets.
 */
#ifndef PCS_REF_STANDIN_PCL_VISUALIZER_H
#define PCS_REF_STANDIN_PCL_VISUALIZER_H
#include <string>

#include <pcl/point_cloud.h>

namespace pcl {
namespace visualization {

enum { PCL_VISUALIZER_POINT_SIZE };

template <class PointT>
struct PointCloudColorHandlerRGBField {
    explicit PointCloudColorHandlerRGBField(const typename pcl::PointCloud<PointT>::Ptr&) {}
};

template <class PointT>
struct PointCloudColorHandlerCustom {
    PointCloudColorHandlerCustom(const typename pcl::PointCloud<PointT>::Ptr&, double, double, double) {}
};

struct PCLVisualizer {
    explicit PCLVisualizer(const std::string&) {}
    void setBackgroundColor(double, double, double, int = 0) {}
    template <class CloudPtr, class Handler> bool addPointCloud(const CloudPtr&, const Handler&, const std::string&) { return true; }
    template <class CloudPtr> bool updatePointCloud(const CloudPtr&, const std::string&) { return true; }
    bool setPointCloudRenderingProperties(int, double, const std::string&) { return true; }
    void spinOnce(int = 1) {}
    bool wasStopped() const { return true; }
};

}  // namespace visualization
}  // namespace pcl
#endif
