/*
 * Declaration-only stand-in for <pcl/point_cloud.h> (and the slice of Eigen the reference reaches through it).
 * TEST INFRASTRUCTURE ONLY, in the spirit of ../librealsense2/rs.hpp.
 *
 * It exists so that the reference's two centre translation units (pcs-multicamera-optimized.cpp, pcs-multicamera-client.cpp)
 * can be compiled, unmodified, into oracle/_ref/libpcs_ref_centre_{opt,client}.so (see ../../Makefile, target `ref`) and their
 * decode / encode / stitch functions driven with caller-owned arrays. It names the types those files mention and nothing else:
 * plain structs, a std::vector of points, std::shared_ptr as Ptr, clear and operator+= as containers.
 * There is NO arithmetic on coordinates here; every number in a record comes from the reference's text, except the affine of
 * pcl::transformPointCloud, which is third-party and restated in ../pcl_transform_standin.cpp ("restated, unpinned").
 *
 * Eigen::Matrix4f lives here because the reference includes no Eigen header itself (PCL's headers bring it in).
 */
#ifndef PCS_REF_STANDIN_PCL_POINT_CLOUD_H
#define PCS_REF_STANDIN_PCL_POINT_CLOUD_H
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace Eigen {

/* row-major storage: m[4 * row + col]; `mat << a, b, c, ...` fills it in reading order, as Eigen's comma initialiser does */
struct Matrix4f {
    float m[16];
    struct CommaInit {
        Matrix4f* to;
        int at;
        CommaInit& operator,(float v) { if (at < 16) to->m[at++] = v; return *this; }
    };
    CommaInit operator<<(float v) { m[0] = v; CommaInit c = { this, 1 }; return c; }
    float operator()(int r, int c) const { return m[4 * r + c]; }
};

template <class T>
struct aligned_allocator {
    typedef T value_type;
    aligned_allocator() {}
    template <class U> aligned_allocator(const aligned_allocator<U>&) {}
    T* allocate(std::size_t n) { return static_cast<T*>(::operator new(n * sizeof(T))); }
    void deallocate(T* p, std::size_t) { ::operator delete(p); }
    template <class U> bool operator==(const aligned_allocator<U>&) const { return true; }
    template <class U> bool operator!=(const aligned_allocator<U>&) const { return false; }
};

}  // namespace Eigen

namespace pcl {

struct PointXYZ { float x, y, z; };
struct PointXYZRGB { float x, y, z; uint8_t r, g, b; };

template <class PointT>
struct PointCloud {
    typedef std::shared_ptr<PointCloud<PointT> > Ptr;
    typedef std::shared_ptr<const PointCloud<PointT> > ConstPtr;

    std::vector<PointT> points;
    uint32_t width = 0;       /* unsigned, as in PCL: the reference compares an int with it */
    uint32_t height = 0;
    bool is_dense = true;

    void clear() { points.clear(); width = 0; height = 0; }
    std::size_t size() const { return points.size(); }

    /* concatenation as PCL 1.8 does it: the points appended, the result one row wide */
    PointCloud& operator+=(const PointCloud& rhs)
    {
        points.insert(points.end(), rhs.points.begin(), rhs.points.end());
        width = static_cast<uint32_t>(points.size());
        height = 1;
        is_dense = is_dense && rhs.is_dense;
        return *this;
    }
};

}  // namespace pcl
#endif
