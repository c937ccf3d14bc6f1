"""ctypes mirrors of the PODs in include/pcs_hip.h, plus the reference's calibration constants.

Field order follows include/pcs_hip.h exactly (which in turn follows rs2_intrinsics /
rs2_extrinsics so a librealsense binding can memcpy).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

POINT_SHORTS = 5          # src/pcs-camera-optimized.cpp:581-585 — x y z (R|G<<8) B
POINT_BYTES = 10
HEADER_SHORTS = 2         # src/pcs-camera-optimized.cpp:690 — payload at buffer + 2 shorts
REF_BUF_SIZE = 5_000_000  # src/pcs-camera-optimized.cpp:27
MAX_STREAMS = 64

FLAG_CUTOFF = 0x1
FLAG_CUTOFF_COMPAT = 0x2
FLAG_DROP_INVALID = 0x4
FLAG_FORCE_IEEE = 0x8
FLAG_TEXCOORD_HALF_PIXEL = 0x10     # u = (px + 0.5)/W as older librealsense releases
FLAG_SCALAR_ARITH = 0x20            # the reference's default (no -m) arithmetic, copyPointCloudXYZRGBToBuffer, bit for bit

OUTLIER_RADIUS_MIN, OUTLIER_RADIUS_MAX = 1, 1000          # pcs_radius_outlier*: radius_mm
OUTLIER_NEIGHBORS_MIN, OUTLIER_NEIGHBORS_MAX = 1, 255     # ... min_neighbors
OUTLIER_LAUNCHES = 10                                     # intervals one call adds to kernel_times_ms under kernel_timing

STAT_K_MIN, STAT_K_MAX = 1, 64                            # pcs_stat_outlier*: mean_k
STAT_MUL_MILLI_MAX = 10000                                # ... std_mul_milli, 0..
STAT_DIST_MIN, STAT_DIST_MAX = 1, 1000                    # ... max_dist_mm
STAT_OUTLIER_LAUNCHES = 14                                # kernel_times_ms intervals of one call with a statistics block (13 without)
STAT_OUTLIER_STAGES = ("clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "knn", "sums", "threshold", "flag",
                       "tile count", "tile scan", "emit", "finish")
STAT_STATS_FIELDS = ("considered", "dense", "s1", "s2_lo", "s2_hi", "threshold", "kept", "reserved")

CLUSTER_TOLERANCE_MIN, CLUSTER_TOLERANCE_MAX = 1, 1000    # pcs_cluster_*: tolerance_mm
CLUSTER_LAUNCHES = 14                                     # kernel_times_ms intervals of one cluster_filter call with a statistics block (13 without)
CLUSTER_STAGES = ("clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "init", "union", "roots", "flag", "tile count",
                  "tile scan", "emit", "stats")
CLUSTER_LABEL_LAUNCHES = 11                               # ... of one cluster_labels call
CLUSTER_LABEL_STAGES = CLUSTER_STAGES[:9] + ("label roots", "labels")
CLUSTER_STATS_FIELDS = ("considered", "clusters", "kept_clusters", "largest", "kept")      # three reserved words behind them
CLUSTER_OBJECTS_MAX = 65536                               # pcs_cluster_objects_*: max_objects
CLUSTER_OBJECT_STAGES = CLUSTER_STAGES[:9] + ("record roots", "firsts", "first scan", "slots", "accumulate", "finish")
CLUSTER_OBJECT_LAUNCHES = 15                              # kernel_times_ms intervals of one cluster_objects call without the filtered output
CLUSTER_OBJECT_OUT_STAGES = CLUSTER_STAGES[:13] + CLUSTER_OBJECT_STAGES[9:]
CLUSTER_OBJECT_OUT_LAUNCHES = 19                          # ... with the filtered output (20 with a statistics block, behind "emit")
CLUSTER_OBJECT_FIELDS = ("label", "size", "lo", "hi", "sum_xyz", "sum_rgb")

PLANE_DISTANCE_MIN, PLANE_DISTANCE_MAX = 1, 1000          # pcs_plane_*: distance_mm
PLANE_ITERATIONS_MAX, PLANE_MAX_PLANES = 4096, 8
PLANE_MODE_REMOVE, PLANE_MODE_KEEP = 0, 1
PLANE_STATS_FIELDS = ("considered", "planes", "inliers_total", "kept", "largest_plane", "degenerate_hypotheses")    # two reserved words behind them
PLANE_MODEL_FIELDS = ("nx", "ny", "nz", "off", "threshold", "inliers")
BACKGROUND_MODE_REMOVE, BACKGROUND_MODE_KEEP = 0, 1
BACKGROUND_FRAMES_MAX = 65535
BACKGROUND_STATS_FIELDS = ("considered", "kept", "background", "cells", "frames", "min_seen", "overflow")    # one reserved word behind them
BACKGROUND_SUBTRACT_LAUNCHES = ("flag", "tile count", "tile scan", "emit", "stats")     # in kernel_times_ms order; "stats" only with a block
TRACK_STATS_FIELDS = ("considered", "voted", "objects", "continued", "born", "lost", "overflow", "frames")
TRACK_UPDATE_LAUNCHES = ("records", "choose", "claim", "assign")     # in kernel_times_ms order: every update, every form
TRACK_MIN_VOTES_MAX = 1 << 30
OBJECT_BOXES_LAUNCHES = ("clear", "moments", "axes", "extents")      # in kernel_times_ms order: every call, every form
TRACK_FIRST_ID_MAX = 1 << 62
PLAN_STATS_FIELDS = ("considered", "in_band", "mapped", "occupied", "fullest")
PLAN_VIEW_LAUNCHES = ("clear", "accumulate", "resolve")              # in kernel_times_ms order: every call, every form
PLAN_SIDE_MAX = 4096
PLAN_CELLS_MAX = 1 << 22


def plane_stages(max_planes: int, labels: bool = False) -> tuple:
    """The launches of one plane_segment (8 max_planes + 1) or plane_labels (8 max_planes - 2) call, in kernel_times_ms order."""
    out = ["init"]
    for r in range(max_planes):
        out += ["hypotheses", "score", "select", "mark"]
        if r + 1 < max_planes:
            out += ["tile count", "tile scan", "emit", "origins"]
    out.append("finish")
    return tuple(out if labels else out + ["out tile count", "out tile scan", "out emit"])


ALIGN_DIST_MIN, ALIGN_DIST_MAX = 1, 1000                  # pcs_align_*: max_dist_mm
ALIGN_ITERATIONS_MAX = 100
ALIGN_STOP_ITERATIONS, ALIGN_STOP_CONVERGED, ALIGN_STOP_REFUSED = 0, 1, 2
ALIGN_INDEX_LAUNCHES = 6                                  # kernel_times_ms intervals: the target's index, once per call
ALIGN_SUMS_LAUNCHES = 8                                   # ... one align_sums call (index, match, reduce)
ALIGN_ITERATION_LAUNCHES = 3                              # ... one iteration of the loop (transform, match, reduce)
ALIGN_PLANE_INDEX_LAUNCHES = 15                           # ... the plane loop, once per call: the target's normals (8), its index, the scatter
ALIGN_PLANE_SUMS_LAUNCHES = 9                             # ... one align_plane_sums call (index, scatter, match, reduce)
ALIGN_PLANE_ITERATION_LAUNCHES = 3                        # ... one iteration of the plane loop (transform, match, reduce)
ALIGN_PLANE_USED_MIN = 6                                  # pcs_align_plane_solve refuses below it
NORMAL_RADIUS_MIN, NORMAL_RADIUS_MAX = 1, 1000            # pcs_estimate_normals*: radius_mm
NORMAL_NEIGHBORS_MIN, NORMAL_NEIGHBORS_MAX = 3, 32767     # ... min_neighbors
NORMAL_FLATNESS_MAX = 1000                                # ... flatness (0 = off)
NORMAL_SHORTS, NORMAL_BYTES = 4, 8                        # a record's normal: nx, ny, nz (x 16384), the neighbour count
NORMAL_LAUNCHES = 8                                       # kernel_times_ms intervals of one estimate_normals call (index, estimate, gather)

DISTORTION_NONE = 0
DISTORTION_MODIFIED_BROWN_CONRADY = 1
DISTORTION_INVERSE_BROWN_CONRADY = 2
DISTORTION_FTHETA = 3
DISTORTION_BROWN_CONRADY = 4

STATUS_NAMES = {
    0: "PCS_OK", -1: "PCS_ERR_INVALID_ARG", -2: "PCS_ERR_NO_DEVICE", -3: "PCS_ERR_HIP",
    -4: "PCS_ERR_UNSUPPORTED", -5: "PCS_ERR_CAPACITY", -6: "PCS_ERR_NOMEM",
}


class Intrinsics(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("ppx", C.c_float), ("ppy", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float),
                ("model", C.c_int32), ("coeffs", C.c_float * 5)]


class Extrinsics(C.Structure):
    _fields_ = [("rotation", C.c_float * 9), ("translation", C.c_float * 3)]


class StreamConfig(C.Structure):
    _fields_ = [("depth", Intrinsics), ("color", Intrinsics),
                ("depth_to_color", Extrinsics),
                ("depth_scale", C.c_float),
                ("color_bpp", C.c_int32), ("color_stride", C.c_int32),
                ("cam_to_world", C.c_float * 16)]

    @property
    def n_points(self) -> int:
        return int(self.depth.width) * int(self.depth.height)

    @property
    def color_bytes(self) -> int:
        return int(self.color_stride) * int(self.color.height)


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_streams", C.c_int32),
                ("streams", C.POINTER(StreamConfig)),
                ("flags", C.c_uint32), ("downsample", C.c_int32)]


class CloudDesc(C.Structure):
    """pcs_cloud_desc: one camera's rs2::points arrays (device pointers) for the batched a2 twin."""
    _fields_ = [("stream", C.c_int32), ("n_points", C.c_int32),
                ("vertices", C.c_void_p), ("texcoords", C.c_void_p),
                ("color", C.c_void_p), ("pc_buffer", C.c_void_p)]


class PayloadDesc(C.Structure):
    """pcs_payload_desc: one camera's packed records (device pointer) and the 4x4 the centre moves them by."""
    _fields_ = [("d_payload", C.c_void_p), ("n_points", C.c_int32), ("transform", C.c_float * 16)]


class DepthFilterConfig(C.Structure):
    """pcs_depth_filter_config: the depth pre-filter's stages and the temporal stage's parameters (librealsense's defaults)."""
    _fields_ = [("temporal", C.c_int32), ("alpha", C.c_float), ("delta", C.c_int32),
                ("persistence", C.c_int32), ("hole_fill", C.c_int32)]


class SpatialFilterConfig(C.Structure):
    """pcs_spatial_filter_config: the spatial filter's parameters; they travel with every call (nothing is set in the context)."""
    _fields_ = [("alpha", C.c_float), ("delta", C.c_int32), ("iterations", C.c_int32), ("hole_radius", C.c_int32)]


class CompressedInfo(C.Structure):
    """pcs_compressed_info: what the validator reads from a "PCZ1" container's header."""
    _fields_ = [("n_points", C.c_uint32), ("n_blocks", C.c_uint32), ("total_bytes", C.c_uint32), ("data_offset", C.c_uint32)]


class NormalParams(C.Structure):
    """pcs_normal_params."""
    _fields_ = [("radius_mm", C.c_int32), ("min_neighbors", C.c_int32), ("flatness", C.c_int32), ("use_viewpoint", C.c_int32),
                ("viewpoint_mm", C.c_int32 * 3), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, radius_mm: int, min_neighbors: int, flatness: int = 0, viewpoint_mm=None, reserved: int = 0) -> "NormalParams":
        vp = (0, 0, 0) if viewpoint_mm is None else tuple(int(v) for v in viewpoint_mm)
        return cls(int(radius_mm), int(min_neighbors), int(flatness), int(viewpoint_mm is not None), (C.c_int32 * 3)(*vp), int(reserved))


class StatOutlierParams(C.Structure):
    """pcs_stat_outlier_params."""
    _fields_ = [("mean_k", C.c_int32), ("std_mul_milli", C.c_int32), ("max_dist_mm", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, mean_k: int, std_mul_milli: int, max_dist_mm: int, reserved: int = 0) -> "StatOutlierParams":
        return cls(int(mean_k), int(std_mul_milli), int(max_dist_mm), int(reserved))


class StatOutlierStatsC(C.Structure):
    """struct pcs_stat_outlier_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in STAT_STATS_FIELDS]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in STAT_STATS_FIELDS}


class ClusterParams(C.Structure):
    """pcs_cluster_params."""
    _fields_ = [("tolerance_mm", C.c_int32), ("min_size", C.c_int32), ("max_size", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, tolerance_mm: int, min_size: int, max_size: int = 0, reserved: int = 0) -> "ClusterParams":
        return cls(int(tolerance_mm), int(min_size), int(max_size), int(reserved))


class ClusterStatsC(C.Structure):
    """struct pcs_cluster_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in CLUSTER_STATS_FIELDS] + [("reserved", C.c_int64 * 3)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in CLUSTER_STATS_FIELDS}


class ClusterObject(C.Structure):
    """pcs_cluster_object: 80 bytes, 8-byte aligned."""
    _fields_ = [("label", C.c_int32), ("size", C.c_int32), ("lo", C.c_int16 * 3), ("hi", C.c_int16 * 3), ("reserved0", C.c_int32),
                ("sum_xyz", C.c_int64 * 3), ("sum_rgb", C.c_int64 * 3), ("reserved1", C.c_int64)]


# the same layout for numpy: a table is np.ndarray of this dtype
CLUSTER_OBJECT_DTYPE = np.dtype({"names": ["label", "size", "lo", "hi", "reserved0", "sum_xyz", "sum_rgb", "reserved1"],
                                 "formats": ["<i4", "<i4", ("<i2", 3), ("<i2", 3), "<i4", ("<i8", 3), ("<i8", 3), "<i8"],
                                 "offsets": [0, 4, 8, 14, 20, 24, 48, 72], "itemsize": 80})


class ClusterObjectsOut(C.Structure):
    """pcs_cluster_objects_out: a host struct of device pointers."""
    _fields_ = [("objects", C.c_void_p), ("max_objects", C.c_int32), ("reserved", C.c_int32), ("n_objects", C.c_void_p),
                ("object_of", C.c_void_p), ("out", C.c_void_p), ("out_shorts", C.c_size_t), ("out_points", C.c_void_p),
                ("stats", C.c_void_p)]

    @classmethod
    def make(cls, objects: int = 0, max_objects: int = 0, n_objects: int = 0, object_of: int = 0, out: int = 0, out_shorts: int = 0,
             out_points: int = 0, stats: int = 0, reserved: int = 0) -> "ClusterObjectsOut":
        return cls(objects or None, int(max_objects), int(reserved), n_objects or None, object_of or None, out or None, int(out_shorts),
                   out_points or None, stats or None)


class PlaneParams(C.Structure):
    """pcs_plane_params: eight 32-bit words."""
    _fields_ = [("distance_mm", C.c_int32), ("iterations", C.c_int32), ("min_inliers", C.c_int32), ("max_planes", C.c_int32),
                ("seed", C.c_uint32), ("mode", C.c_int32), ("reserved", C.c_int32 * 2)]

    @classmethod
    def make(cls, distance_mm: int, iterations: int, min_inliers: int = 3, max_planes: int = 1, seed: int = 1, mode: int = 0,
             reserved=(0, 0)) -> "PlaneParams":
        return cls(int(distance_mm), int(iterations), int(min_inliers), int(max_planes), int(seed) & 0xFFFFFFFF, int(mode),
                   (C.c_int32 * 2)(int(reserved[0]), int(reserved[1])))


class PlaneModel(C.Structure):
    """pcs_plane_model: 64 bytes."""
    _fields_ = [(name, C.c_int64) for name in PLANE_MODEL_FIELDS] + [("sample", C.c_int32 * 3), ("hypothesis", C.c_int32)]

    def as_dict(self) -> dict:
        d = {name: int(getattr(self, name)) for name in PLANE_MODEL_FIELDS}
        d["sample"] = tuple(int(v) for v in self.sample)
        d["hypothesis"] = int(self.hypothesis)
        return d


class PlaneStats(C.Structure):
    """struct pcs_plane_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in PLANE_STATS_FIELDS] + [("reserved", C.c_int64 * 2)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in PLANE_STATS_FIELDS}


class BackgroundParams(C.Structure):
    """pcs_background_params: four 32-bit words."""
    _fields_ = [("min_seen", C.c_int32), ("dilate", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, min_seen: int, dilate: int = 1, mode: int = 0, reserved: int = 0) -> "BackgroundParams":
        return cls(int(min_seen), int(dilate), int(mode), int(reserved))


class BackgroundInfo(C.Structure):
    """struct pcs_background_info: six 32-bit words."""
    _fields_ = [("cell_mm", C.c_int32), ("max_cells", C.c_int32), ("cells", C.c_uint32), ("frames", C.c_uint32), ("overflow", C.c_int32),
                ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in ("cell_mm", "max_cells", "cells", "frames", "overflow")}


class BackgroundStats(C.Structure):
    """struct pcs_background_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in BACKGROUND_STATS_FIELDS] + [("reserved", C.c_int64)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in BACKGROUND_STATS_FIELDS}


class TrackParams(C.Structure):
    """pcs_track_params: four 32-bit words."""
    _fields_ = [("min_votes", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def make(cls, min_votes: int = 1, reserved=(0, 0, 0)) -> "TrackParams":
        return cls(int(min_votes), (C.c_int32 * 3)(*(int(v) for v in reserved)))


class Track(C.Structure):
    """pcs_track: 24 bytes."""
    _fields_ = [("id", C.c_int64), ("age", C.c_int32), ("prev", C.c_int32), ("votes", C.c_int32), ("reserved", C.c_int32)]


TRACK_DTYPE = np.dtype([("id", "<i8"), ("age", "<i4"), ("prev", "<i4"), ("votes", "<i4"), ("reserved", "<i4")])
assert TRACK_DTYPE.itemsize == C.sizeof(Track) == 24


class ObjectBox(C.Structure):
    """pcs_object_box: 128 bytes."""
    _fields_ = [("count", C.c_int64), ("sum_xyz", C.c_int64 * 3), ("m2", C.c_int64 * 6), ("axis", (C.c_int16 * 3) * 3), ("rank", C.c_int16),
                ("ext_lo", C.c_int32 * 3), ("ext_hi", C.c_int32 * 3), ("reserved", C.c_int32)]


OBJECT_BOX_DTYPE = np.dtype({"names": ["count", "sum_xyz", "m2", "axis", "rank", "ext_lo", "ext_hi", "reserved"],
                             "formats": ["<i8", ("<i8", 3), ("<i8", 6), ("<i2", (3, 3)), "<i2", ("<i4", 3), ("<i4", 3), "<i4"],
                             "offsets": [0, 8, 32, 80, 98, 100, 112, 124], "itemsize": 128})
assert OBJECT_BOX_DTYPE.itemsize == C.sizeof(ObjectBox) == 128
assert all(OBJECT_BOX_DTYPE.fields[name][1] == getattr(ObjectBox, name).offset for name in OBJECT_BOX_DTYPE.names)


class PlanParams(C.Structure):
    """pcs_plan_params: twelve int32 words."""
    _fields_ = [("up_axis", C.c_int32), ("up_sign", C.c_int32), ("cell_mm", C.c_int32), ("origin_u", C.c_int32), ("origin_v", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("band_lo", C.c_int32), ("band_hi", C.c_int32), ("reserved", C.c_int32 * 3)]

    @classmethod
    def make(cls, up_axis: int, up_sign: int, cell_mm: int, width: int, height: int, origin_u=None, origin_v=None, band_lo: int = -32768,
             band_hi: int = 32767, reserved=(0, 0, 0)) -> "PlanParams":
        """Without an origin the map is centred on 0: -(width * cell_mm) // 2 per axis (the CLI's rule)."""
        u0 = -((int(width) * int(cell_mm)) // 2) if origin_u is None else int(origin_u)
        v0 = -((int(height) * int(cell_mm)) // 2) if origin_v is None else int(origin_v)
        return cls(int(up_axis), int(up_sign), int(cell_mm), u0, v0, int(width), int(height), int(band_lo), int(band_hi),
                   (C.c_int32 * 3)(*(int(r) for r in reserved)))


class PlanStats(C.Structure):
    """struct pcs_plan_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in PLAN_STATS_FIELDS] + [("reserved", C.c_int64 * 3)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in PLAN_STATS_FIELDS}


class PlanMaps(C.Structure):
    """pcs_plan_maps: a host struct of five pointers (device pointers for the device forms), all required."""
    _fields_ = [("count", C.c_void_p), ("top", C.c_void_p), ("bottom", C.c_void_p), ("rgb", C.c_void_p), ("stats", C.c_void_p)]

    @classmethod
    def make(cls, count: int = 0, top: int = 0, bottom: int = 0, rgb: int = 0, stats: int = 0) -> "PlanMaps":
        return cls(count or None, top or None, bottom or None, rgb or None, stats or None)


assert C.sizeof(PlanParams) == 48 and C.sizeof(PlanStats) == 64 and C.sizeof(PlanMaps) == 5 * C.sizeof(C.c_void_p)


class TrackStats(C.Structure):
    """struct pcs_track_stats: eight int64."""
    _fields_ = [(name, C.c_int64) for name in TRACK_STATS_FIELDS]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in TRACK_STATS_FIELDS}


class TrackerInfo(C.Structure):
    """struct pcs_tracker_info: 40 bytes."""
    _fields_ = [("cell_mm", C.c_int32), ("max_cells", C.c_int32), ("max_objects", C.c_int32), ("objects", C.c_int32),
                ("frames", C.c_int64), ("next_id", C.c_int64), ("overflow", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name in ("cell_mm", "max_cells", "max_objects", "objects", "frames", "next_id", "overflow")}


class AlignSumsC(C.Structure):
    """struct pcs_align_sums: eighteen int64."""
    _fields_ = [("considered", C.c_int64), ("matched", C.c_int64), ("sp", C.c_int64 * 3), ("sq", C.c_int64 * 3),
                ("spq", C.c_int64 * 9), ("sd2", C.c_int64)]


class AlignParams(C.Structure):
    """pcs_align_params."""
    _fields_ = [("max_dist_mm", C.c_int32), ("iterations", C.c_int32), ("source_stride", C.c_int32), ("reserved", C.c_int32),
                ("eps_rot_rad", C.c_double), ("eps_trans_mm", C.c_double)]


class AlignReportC(C.Structure):
    """pcs_align_report."""
    _fields_ = [("iterations", C.c_int32), ("stop_reason", C.c_int32),
                ("first_matched", C.c_int64), ("first_considered", C.c_int64),
                ("last_matched", C.c_int64), ("last_considered", C.c_int64),
                ("first_rms_mm", C.c_double), ("last_rms_mm", C.c_double),
                ("trace_capacity", C.c_int32), ("trace_count", C.c_int32),
                ("trace_transforms", C.c_void_p), ("trace_sums", C.c_void_p)]


class AlignPlaneSumsC(C.Structure):
    """struct pcs_align_plane_sums: sixty int64."""
    _fields_ = [("considered", C.c_int64), ("matched", C.c_int64), ("used", C.c_int64), ("ata_lo", C.c_int64 * 21),
                ("ata_hi", C.c_int64 * 21), ("atb_lo", C.c_int64 * 6), ("atb_hi", C.c_int64 * 6), ("sb2_lo", C.c_int64),
                ("sb2_hi", C.c_int64), ("sd2", C.c_int64)]


class AlignPlaneParams(C.Structure):
    """pcs_align_plane_params."""
    _fields_ = [("max_dist_mm", C.c_int32), ("iterations", C.c_int32), ("source_stride", C.c_int32), ("reserved", C.c_int32),
                ("eps_rot_rad", C.c_double), ("eps_trans_mm", C.c_double), ("normals", NormalParams)]


class AlignPlaneReportC(C.Structure):
    """pcs_align_plane_report."""
    _fields_ = [("iterations", C.c_int32), ("stop_reason", C.c_int32),
                ("first_matched", C.c_int64), ("first_used", C.c_int64), ("first_considered", C.c_int64),
                ("last_matched", C.c_int64), ("last_used", C.c_int64), ("last_considered", C.c_int64),
                ("first_rms_mm", C.c_double), ("last_rms_mm", C.c_double),
                ("trace_capacity", C.c_int32), ("trace_count", C.c_int32),
                ("trace_transforms", C.c_void_p), ("trace_sums", C.c_void_p)]


@dataclass(frozen=True)
class AlignPlaneSums:
    """The point-to-plane sums of one correspondence step: the sixty int64 words as the library wrote them (Python integers), the
    halves of every product kept apart; ata / atb / sb2 recombine them (hi 2^32 + lo: exact)."""
    words: Tuple[int, ...]

    considered = property(lambda self: self.words[0])
    matched = property(lambda self: self.words[1])
    used = property(lambda self: self.words[2])
    sd2 = property(lambda self: self.words[59])

    def as_array(self) -> np.ndarray:
        """The sixty int64 words in struct order."""
        return np.array(self.words, dtype=np.int64)

    @classmethod
    def from_array(cls, a) -> "AlignPlaneSums":
        v = tuple(int(x) for x in np.asarray(a).reshape(-1))
        if len(v) != 60:
            raise ValueError("point-to-plane sums are 60 integers")
        return cls(v)

    @property
    def ata(self) -> List[int]:
        """The upper triangle of A^T A, row-major, 21 exact integers."""
        return [(self.words[24 + k] << 32) + self.words[3 + k] for k in range(21)]

    @property
    def atb(self) -> List[int]:
        return [(self.words[51 + k] << 32) + self.words[45 + k] for k in range(6)]

    @property
    def sb2(self) -> int:
        return (self.words[58] << 32) + self.words[57]

    def to_c(self) -> AlignPlaneSumsC:
        c = AlignPlaneSumsC()
        C.memmove(C.addressof(c), self.as_array().ctypes.data, C.sizeof(c))
        return c


@dataclass
class AlignPlaneReport:
    """What pcs_align_payloads_plane_device reports: AlignReport's fields with `used` beside `matched`, the trace's sums as
    AlignPlaneSums."""
    iterations: int
    stop_reason: int
    status: int
    detail: str
    first_matched: int
    first_used: int
    first_considered: int
    last_matched: int
    last_used: int
    last_considered: int
    first_rms_mm: float
    last_rms_mm: float
    trace_transforms: np.ndarray = field(default_factory=lambda: np.zeros((0, 4, 4), np.float32))
    trace_sums: List[AlignPlaneSums] = field(default_factory=list)


@dataclass(frozen=True)
class AlignSums:
    """The alignment sums of one correspondence step (Python integers: exact)."""
    considered: int
    matched: int
    sp: Tuple[int, int, int]
    sq: Tuple[int, int, int]
    spq: Tuple[int, ...]          # spq[3a+b] = sum of p_a q_b
    sd2: int

    def as_array(self) -> np.ndarray:
        """The eighteen int64 words in struct order."""
        return np.array([self.considered, self.matched, *self.sp, *self.sq, *self.spq, self.sd2], dtype=np.int64)

    @classmethod
    def from_array(cls, a) -> "AlignSums":
        v = [int(x) for x in np.asarray(a).reshape(-1)]
        if len(v) != 18:
            raise ValueError("alignment sums are 18 integers")
        return cls(v[0], v[1], tuple(v[2:5]), tuple(v[5:8]), tuple(v[8:17]), v[17])

    def to_c(self) -> AlignSumsC:
        c = AlignSumsC()
        c.considered, c.matched, c.sd2 = self.considered, self.matched, self.sd2
        for k in range(3):
            c.sp[k], c.sq[k] = self.sp[k], self.sq[k]
        for k in range(9):
            c.spq[k] = self.spq[k]
        return c


@dataclass
class AlignReport:
    """What pcs_align_payloads_device reports: the iterations run, the first and the last of them, why it stopped, the status the
    call returned (0, or PCS_ERR_UNSUPPORTED when a solve refused) and the trace: F_k [n, 4, 4] float32 and S_k of every recorded
    iteration."""
    iterations: int
    stop_reason: int
    status: int
    detail: str
    first_matched: int
    first_considered: int
    last_matched: int
    last_considered: int
    first_rms_mm: float
    last_rms_mm: float
    trace_transforms: np.ndarray = field(default_factory=lambda: np.zeros((0, 4, 4), np.float32))
    trace_sums: List[AlignSums] = field(default_factory=list)


# --- the reference's surveyed extrinsics (data, not code) -------------------------------------
# src/pcs-camera-optimized.cpp:64-67
TF_MAT = np.array([
    -0.99977970,  0.00926272,  0.01883480,  0.00000000,
    -0.01638983,  0.21604544, -0.97624574,  3.41600000,
    -0.01311186, -0.97633937, -0.21584603,  1.80200000,
     0.00000000,  0.00000000,  0.00000000,  1.00000000], dtype=np.float32)

# src/pcs-multicamera-optimized.cpp:417-455 — transform[0..7]
TRANSFORMS = np.array([
    [-0.69888007, -0.32213748,  0.63858757, -2.22900000,
     -0.71520905,  0.32290986, -0.61984291,  2.91800000,
     -0.00653159, -0.88991947, -0.45607091,  0.36400000,
      0.0, 0.0, 0.0, 1.0],
    [-0.96127595,  0.09045863, -0.26031862,  0.31700000,
      0.27558764,  0.31552831, -0.90801615,  2.83300000,
      0.00000000, -0.94459469, -0.32823906,  0.38100000,
      0.0, 0.0, 0.0, 1.0],
    [-0.63305575,  0.28270490, -0.72063747,  2.80300000,
      0.77409926,  0.22724638, -0.59087175,  2.05500000,
     -0.00328008, -0.93189968, -0.36270128,  0.42100000,
      0.0, 0.0, 0.0, 1.0],
    [ 0.17021299,  0.28598815, -0.94299433,  2.51000000,
      0.98527137, -0.03349883,  0.16768470, -0.27300000,
      0.01636663, -0.95764743, -0.28747787,  0.35900000,
      0.0, 0.0, 0.0, 1.0],
    [ 0.72625904,  0.26139935, -0.63578155,  1.90900000,
      0.68735231, -0.26305364,  0.67701520, -2.81700000,
      0.00972668, -0.92869433, -0.37071853,  0.37900000,
      0.0, 0.0, 0.0, 1.0],
    [ 0.98744750,  0.00686296,  0.15779838, -0.57400000,
     -0.14665062, -0.33120318,  0.93209337, -2.69700000,
      0.05866025, -0.94353450, -0.32603930,  0.30900000,
      0.0, 0.0, 0.0, 1.0],
    [ 0.67295609,  0.40193638,  0.62094867, -2.97300000,
     -0.35777412, -0.55787451,  0.74884826, -0.41700000,
      0.64740079, -0.72610136, -0.23162261,  0.43400000,
      0.0, 0.0, 0.0, 1.0],
    [ 0.08929624, -0.21535297,  0.97244500, -2.95700000,
     -0.67610010, -0.73004840, -0.09958907, -0.33900000,
      0.73137872, -0.64857723, -0.21079074,  0.33800000,
      0.0, 0.0, 0.0, 1.0],
], dtype=np.float32)


def make_intrinsics(width: int, height: int, fx: float, fy: float, ppx: float, ppy: float,
                    model: int = DISTORTION_NONE, coeffs: Optional[Sequence[float]] = None) -> Intrinsics:
    it = Intrinsics()
    it.width, it.height = int(width), int(height)
    it.fx, it.fy, it.ppx, it.ppy = float(fx), float(fy), float(ppx), float(ppy)
    it.model = int(model)
    cs = list(coeffs) if coeffs is not None else [0.0] * 5
    if len(cs) != 5:
        raise ValueError("coeffs must have 5 entries (k1 k2 p1 p2 k3)")
    for k in range(5):
        it.coeffs[k] = float(cs[k])
    return it


def make_stream_config(depth: Intrinsics, color: Optional[Intrinsics] = None, *,
                       cam_to_world: Optional[Iterable[float]] = None,
                       rotation: Optional[Iterable[float]] = None,
                       translation: Iterable[float] = (0.015, 0.0, 0.0),
                       depth_scale: float = 0.001,
                       color_bpp: int = 3, color_stride: Optional[int] = None) -> StreamConfig:
    """Build one camera stream's configuration.

    Defaults follow SURVEY.md §8(d): colour at the depth resolution, depth->colour R = I,
    t = (0.015, 0, 0) m, depth scale 0.001, RGB8 with stride = 3*W, extrinsic = tf_mat.
    """
    sc = StreamConfig()
    sc.depth = depth
    sc.color = color if color is not None else depth
    rot = list(rotation) if rotation is not None else [1, 0, 0, 0, 1, 0, 0, 0, 1]
    tr = list(translation)
    if len(rot) != 9 or len(tr) != 3:
        raise ValueError("rotation needs 9 (column-major) and translation 3 entries")
    for k in range(9):
        sc.depth_to_color.rotation[k] = float(rot[k])
    for k in range(3):
        sc.depth_to_color.translation[k] = float(tr[k])
    sc.depth_scale = float(depth_scale)
    sc.color_bpp = int(color_bpp)
    sc.color_stride = int(color_stride) if color_stride is not None else int(color_bpp) * int(sc.color.width)
    m = np.asarray(TF_MAT if cam_to_world is None else cam_to_world, dtype=np.float32).reshape(-1)
    if m.size != 16:
        raise ValueError("cam_to_world must have 16 entries (row-major 4x4)")
    for k in range(16):
        sc.cam_to_world[k] = float(m[k])
    return sc


def decimated_stream_config(cfg: StreamConfig, scale: int) -> StreamConfig:
    """pcs_decimated_stream_config: the stream a raster decimated by `scale` (1..8) belongs to — smaller depth raster, focal lengths
    and principal point moved so that every decimated pixel deprojects along the centre of its source block; everything else, the
    colour camera included, is copied. The C function does the arithmetic (no device is touched); ValueError on what it refuses."""
    from . import lib as _libmod               # (lib imports this module)
    lib = _libmod.load()
    out = StreamConfig()
    rc = lib.pcs_decimated_stream_config(C.byref(cfg), int(scale), C.byref(out))
    if rc != 0:
        raise ValueError(f"{STATUS_NAMES.get(rc, rc)}: {(lib.pcs_last_error(None) or b'').decode()}")
    return out


def stream_array(configs: Sequence[StreamConfig]):
    arr = (StreamConfig * len(configs))()
    for i, c in enumerate(configs):
        C.memmove(C.byref(arr, i * C.sizeof(StreamConfig)), C.byref(c), C.sizeof(StreamConfig))
    return arr
