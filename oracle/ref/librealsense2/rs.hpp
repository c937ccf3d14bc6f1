/*
 * Declaration-only stand-in for <librealsense2/rs.hpp>. TEST INFRASTRUCTURE ONLY.
 *
 * It exists so that the reference's camera translation unit can be compiled, unmodified, into
 * oracle/_ref/libpcs_ref.so (see ../Makefile, target `ref`) and its pack functions driven with
 * caller-owned arrays. It names the rs2:: types that file mentions and
 * nothing else: plain-data structs, accessors that hand back what the caller stored, and empty
 * pipeline / device types for the parts of main() that are compiled but never run.
 * There is no arithmetic here; every number in a packed record comes from the reference's text.
 */
#ifndef PCS_REF_STANDIN_RS_HPP
#define PCS_REF_STANDIN_RS_HPP
#include <cstddef>
#include <cstdint>

enum { RS2_OPTION_EMITTER_ENABLED, RS2_CAMERA_INFO_NAME, RS2_CAMERA_INFO_FIRMWARE_VERSION };

namespace rs2 {

struct vertex { float x, y, z; };
struct texture_coordinate { float u, v; };

struct video_frame {
    const void* data = nullptr;
    int w = 0, h = 0, bpp = 0, stride = 0;
    const void* get_data() const { return data; }
    int get_width() const { return w; }
    int get_height() const { return h; }
    int get_bytes_per_pixel() const { return bpp; }
    int get_stride_in_bytes() const { return stride; }
};

struct depth_frame : video_frame {
    depth_frame() {}
    depth_frame(const video_frame& f) : video_frame(f) {}
};

struct points {
    const vertex* v = nullptr;
    const texture_coordinate* t = nullptr;
    size_t n = 0;
    const vertex* get_vertices() const { return v; }
    const texture_coordinate* get_texture_coordinates() const { return t; }
    size_t size() const { return n; }
};

struct pointcloud {
    points calculate(const depth_frame&) { return points(); }
    void map_to(const video_frame&) {}
};

struct depth_sensor {
    bool supports(int) const { return false; }
    void set_option(int, float) {}
};

struct device {
    template <class T> T first() const { return T(); }
    const char* get_info(int) const { return ""; }
};

struct pipeline_profile { device get_device() const { return device(); } };
struct config { void enable_device_from_file(const char*) {} };

struct frameset {
    unsigned long long get_frame_number() const { return 0; }
    video_frame get_color_frame() const { return video_frame(); }
    depth_frame get_depth_frame() const { return depth_frame(); }
};

struct pipeline {
    pipeline_profile start() { return pipeline_profile(); }
    pipeline_profile start(const config&) { return pipeline_profile(); }
    frameset wait_for_frames() { return frameset(); }
    bool poll_for_frames(frameset*) { return false; }
    void stop() {}
    pipeline_profile get_active_profile() const { return pipeline_profile(); }
};

}  // namespace rs2
#endif
