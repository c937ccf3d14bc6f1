/*
 * Declaration-only stand-in for <pcl/filters/voxel_grid.h>. TEST INFRASTRUCTURE ONLY (see ../point_cloud.h).
 * The reference's centre programs include this header and use nothing from it.
 */
#ifndef PCS_REF_STANDIN_PCL_VOXEL_GRID_H
#define PCS_REF_STANDIN_PCL_VOXEL_GRID_H
#include <pcl/point_cloud.h>
#endif
