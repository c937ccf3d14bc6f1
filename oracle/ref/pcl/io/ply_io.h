/*
 * Declaration-only stand-in for <pcl/io/ply_io.h>. TEST INFRASTRUCTURE ONLY (see ../point_cloud.h).
 * The reference saves .ply files only under `-s`, which the harness never sets: this writes nothing.
 */
#ifndef PCS_REF_STANDIN_PCL_PLY_IO_H
#define PCS_REF_STANDIN_PCL_PLY_IO_H
#include <string>

#include <pcl/point_cloud.h>

namespace pcl {
namespace io {

template <class PointT>
int savePLYFileBinary(const std::string&, const pcl::PointCloud<PointT>&) { return 0; }

}  // namespace io
}  // namespace pcl
#endif
