"""Host-side mirror of the reference's operator surface, over the C ABI (include/pcs_hip.h).

Reference seam (src/pcs-camera-optimized.cpp):
    copyPointCloudXYZRGBToBufferSIMD(pts, color, pc_buffer)  :363  -> PcsContext.copy_pointcloud_xyzrgb_to_buffer
    sendXYZRGBPointcloud(pts, color, buffer)                 :669  -> PcsContext.send_xyzrgb_pointcloud
    rs2::pointcloud::calculate / map_to                      :288  -> PcsContext.deproject
    (edge + central collapsed)                                      -> PcsContext.process_frames
and src/pcs-multicamera-client.cpp: sendStitchToUnity :373   -> PcsContext.stitch_device

Everything here is plumbing: argument marshalling and error mapping. The arithmetic lives in the
HIP kernels (csrc/pcs_kernels.hip); there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import lib as _libmod
from .types import (BackgroundInfo, BackgroundParams, BackgroundStats, AlignParams, AlignPlaneParams, AlignPlaneReport, AlignPlaneReportC, AlignPlaneSums, AlignPlaneSumsC, AlignReport, AlignReportC, AlignSums, AlignSumsC, CloudDesc, CLUSTER_OBJECT_DTYPE, ClusterObject, ClusterObjectsOut, ClusterParams, ClusterStatsC, CompressedInfo, Config, DepthFilterConfig, NormalParams, NORMAL_SHORTS, OBJECT_BOX_DTYPE, ObjectBox, PlanMaps, PlanParams, PlanStats, PlaneModel, PlaneParams, PlaneStats, SpatialFilterConfig, StatOutlierParams, StatOutlierStatsC, StreamConfig, STATUS_NAMES, Track, TRACK_DTYPE, TrackParams, TrackStats, TrackerInfo, POINT_SHORTS, POINT_BYTES, HEADER_SHORTS,
                    REF_BUF_SIZE, stream_array)


class PcsError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"{name}: {detail}" if detail else name)


def device_count() -> int:
    return int(_libmod.load().pcs_device_count())


def _ptr(a: np.ndarray) -> int:
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("array must be C-contiguous")
    return a.ctypes.data


def compressed_bound(n_points: int) -> int:
    """pcs_compressed_bound: the largest "PCZ1" container of n_points records (16 + 660 ceil(n / 64))."""
    return int(_libmod.load().pcs_compressed_bound(int(n_points)))


def compressed_info(container) -> CompressedInfo:
    """pcs_compressed_info: validate a container (bytes or a uint8 array) on the host — no context, no GPU. Raises PcsError
    (PCS_ERR_INVALID_ARG) whose text names the first violation."""
    lib = _libmod.load()
    buf = np.ascontiguousarray(np.frombuffer(container, np.uint8) if isinstance(container, (bytes, bytearray)) else container)
    info = CompressedInfo()
    rc = lib.pcs_compressed_info(buf.ctypes.data if buf.nbytes else None, buf.nbytes, C.byref(info))
    if rc != 0:
        d = lib.pcs_last_error(None)
        raise PcsError(rc, d.decode() if d else "")
    return info


def _as_bytes_array(container) -> np.ndarray:
    return np.ascontiguousarray(np.frombuffer(container, np.uint8) if isinstance(container, (bytes, bytearray, memoryview)) else container)


def background_export_bound(max_cells: int) -> int:
    """pcs_background_export_bound: the largest "PCB1" container of a model of max_cells cells (32 + 12 max_cells)."""
    return int(_libmod.load().pcs_background_export_bound(int(max_cells)))


def background_validate(container) -> dict:
    """pcs_background_validate: validate a "PCB1" container (bytes or a uint8 array) on the host — no context, no GPU. Returns
    cell_mm, cells and frames; raises PcsError (PCS_ERR_INVALID_ARG) whose text names the first violation."""
    lib = _libmod.load()
    buf = _as_bytes_array(container)
    info = BackgroundInfo()
    rc = lib.pcs_background_validate(buf.ctypes.data if buf.nbytes else None, buf.nbytes, C.byref(info))
    if rc != 0:
        d = lib.pcs_last_error(None)
        raise PcsError(rc, d.decode() if d else "")
    return info.as_dict()


class Background:
    """A background model on a context's device (pcs_background_*): learn frame-sets into it, subtract it from others. Created by
    PcsContext.background_create / background_import; close() it (or leave a `with` block) before the context closes, which frees
    what is left."""

    def __init__(self, ctx: "PcsContext", handle: int):
        self._ctx = ctx
        self._h = handle

    @property
    def handle(self) -> int:
        return self._h or 0

    def close(self) -> None:
        if self._h and self._ctx._h:
            self._ctx._check(self._ctx._lib.pcs_background_destroy(self._ctx._h, self._h))
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call(self, fn, *args) -> None:
        self._ctx._check(fn(self._ctx._h, self._h, *args))

    def reset(self) -> None:
        self._call(self._ctx._lib.pcs_background_reset)

    def info(self) -> dict:
        """cell_mm, max_cells, cells, frames, overflow — synchronous."""
        info = BackgroundInfo()
        self._call(self._ctx._lib.pcs_background_info, C.byref(info))
        return info.as_dict()

    def learn(self, payload: np.ndarray) -> None:
        """Packed records (int16 [n,5]) as one frame-set (pcs_background_learn: host array, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        self._call(self._ctx._lib.pcs_background_learn, _ptr(p) if p.shape[0] else None, p.shape[0])

    def learn_device(self, d_payload: int, n_points: int) -> None:
        self._call(self._ctx._lib.pcs_background_learn_device, d_payload or None, int(n_points))

    def learn_device_counted(self, d_payload: int, d_n_points: int, max_points: int) -> None:
        self._call(self._ctx._lib.pcs_background_learn_device_counted, d_payload or None, d_n_points or None, int(max_points))

    def subtract(self, payload: np.ndarray, min_seen: int, dilate: int = 1, mode: int = 0):
        """Packed records (int16 [n,5]) -> (the records that are not background (mode 0) or are (mode 1), input order; the statistics
        block as a dict) (pcs_background_subtract: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        stats = BackgroundStats()
        params = BackgroundParams.make(min_seen, dilate, mode)
        self._call(self._ctx._lib.pcs_background_subtract, _ptr(p), p.shape[0], C.byref(params), _ptr(out), p.shape[0] * POINT_SHORTS,
                   C.byref(cnt), C.byref(stats))
        return out[:cnt.value].copy(), stats.as_dict()

    def subtract_device(self, d_payload: int, n_points: int, params: BackgroundParams, d_out: int, out_shorts: int, d_out_points: int,
                        d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints; *d_out_points (int32, required) receives the kept count, d_stats (eight int64,
        optional) the statistics block. params may be None (refused). See pcs_background_subtract_device."""
        self._call(self._ctx._lib.pcs_background_subtract_device, d_payload or None, int(n_points),
                   C.byref(params) if params is not None else None, d_out or None, out_shorts, d_out_points or None, d_stats or None)

    def subtract_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: BackgroundParams, d_out: int,
                                out_shorts: int, d_out_points: int, d_stats: int = 0) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run."""
        self._call(self._ctx._lib.pcs_background_subtract_device_counted, d_payload or None, d_n_points or None, int(max_points),
                   C.byref(params) if params is not None else None, d_out or None, out_shorts, d_out_points or None, d_stats or None)

    def export(self) -> bytes:
        """The canonical "PCB1" container (pcs_background_export): synchronous. PcsError (PCS_ERR_CAPACITY) for an overflowed model."""
        buf = np.zeros(background_export_bound(self.info()["max_cells"]), np.uint8)
        n = C.c_size_t(0)
        self._call(self._ctx._lib.pcs_background_export, _ptr(buf), buf.nbytes, C.byref(n))
        return buf[:n.value].tobytes()


class Tracker:
    """An object tracker on a context's device (pcs_tracker_*): persistent identities for the objects of cluster_objects across
    frame-sets. Created by PcsContext.tracker_create; destroy() it (or leave a `with` block) before the context closes, which frees
    what is left."""

    def __init__(self, ctx: "PcsContext", handle: int):
        self._ctx = ctx
        self._h = handle

    @property
    def handle(self) -> int:
        return self._h or 0

    def destroy(self) -> None:
        if self._h and self._ctx._h:
            self._ctx._check(self._ctx._lib.pcs_tracker_destroy(self._ctx._h, self._h))
        self._h = None

    close = destroy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def _call(self, fn, *args) -> None:
        self._ctx._check(fn(self._ctx._h, self._h, *args))

    def reset(self, first_id: int = 1) -> None:
        self._call(self._ctx._lib.pcs_tracker_reset, int(first_id))

    def info(self) -> dict:
        """cell_mm, max_cells, max_objects, objects, frames, next_id, overflow — synchronous."""
        info = TrackerInfo()
        self._call(self._ctx._lib.pcs_tracker_info, C.byref(info))
        return info.as_dict()

    def update(self, payload: np.ndarray, object_of: np.ndarray, n_objects: int, max_objects: int, min_votes: int = 1):
        """Packed records (int16 [n,5]), their object_of (int32 [n]) and the object count -> (tracks as a TRACK_DTYPE array of
        min(n_objects, max_objects) entries, the statistics block as a dict) (pcs_tracker_update: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        o = np.ascontiguousarray(object_of, np.int32).reshape(-1)
        if o.shape[0] != p.shape[0]:
            raise ValueError("object_of must hold one int32 per record")
        tracks = np.zeros(max(int(max_objects), 1), TRACK_DTYPE)
        stats = TrackStats()
        params = TrackParams.make(min_votes)
        self._call(self._ctx._lib.pcs_tracker_update, _ptr(p) if p.shape[0] else None, p.shape[0], _ptr(o) if o.shape[0] else None,
                   int(n_objects), int(max_objects), C.byref(params), C.cast(_ptr(tracks), C.POINTER(Track)), C.byref(stats))
        return tracks[:min(max(int(n_objects), 0), int(max_objects))].copy(), stats.as_dict()

    def update_device(self, d_payload: int, n_points: int, d_object_of: int, d_n_objects: int, max_objects: int, params: TrackParams,
                      d_tracks: int, d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints: what cluster_objects_device left (payload, object_of, *n_objects, its max_objects) ->
        d_tracks (max_objects entries of 24 bytes), d_stats (eight int64, optional). params may be None (refused)."""
        self._call(self._ctx._lib.pcs_tracker_update_device, d_payload or None, int(n_points), d_object_of or None, d_n_objects or None,
                   int(max_objects), C.byref(params) if params is not None else None, d_tracks or None, d_stats or None)

    def update_device_counted(self, d_payload: int, d_n_points: int, max_points: int, d_object_of: int, d_n_objects: int, max_objects: int,
                              params: TrackParams, d_tracks: int, d_stats: int = 0) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run."""
        self._call(self._ctx._lib.pcs_tracker_update_device_counted, d_payload or None, d_n_points or None, int(max_points),
                   d_object_of or None, d_n_objects or None, int(max_objects), C.byref(params) if params is not None else None,
                   d_tracks or None, d_stats or None)


def plane_from_points(p0, p1, p2, distance_mm: int) -> dict:
    """pcs_plane_from_points: the plane model through three records (x, y, z in int16 millimetres) at distance_mm, as a hypothesis
    that drew them builds it — no context, no GPU. Raises PcsError (PCS_ERR_INVALID_ARG) for a degenerate triple or a distance
    outside 1..1000."""
    lib = _libmod.load()
    pts = [np.ascontiguousarray(np.asarray(p, np.int64)[:3].astype(np.int16)) for p in (p0, p1, p2)]
    model = PlaneModel()
    rc = lib.pcs_plane_from_points(_ptr(pts[0]), _ptr(pts[1]), _ptr(pts[2]), int(distance_mm), C.byref(model))
    if rc != 0:
        raise PcsError(rc, "pcs_plane_from_points: a degenerate triple or distance_mm outside 1..1000")
    return model.as_dict()


def _sums_from_c(c: AlignSumsC) -> AlignSums:
    return AlignSums(int(c.considered), int(c.matched), tuple(int(v) for v in c.sp), tuple(int(v) for v in c.sq),
                     tuple(int(v) for v in c.spq), int(c.sd2))


def align_solve(sums: AlignSums) -> Tuple[np.ndarray, float]:
    """pcs_align_solve: the rigid fit of one set of alignment sums on the host — no context, no GPU. Returns (delta, rms_mm):
    delta a float64 [4, 4] in metres that moves the source onto the target. Raises PcsError (PCS_ERR_UNSUPPORTED) with fewer than
    three matches or a degenerate (collinear, coincident) configuration."""
    lib = _libmod.load()
    c = sums.to_c()
    delta = (C.c_double * 16)()
    rms = C.c_double(0)
    rc = lib.pcs_align_solve(C.byref(c), delta, C.byref(rms))
    if rc != 0:
        d = lib.pcs_last_error(None)
        raise PcsError(rc, d.decode() if d else "")
    return np.array(delta[:], np.float64).reshape(4, 4), float(rms.value)


def _plane_sums_from_c(c: AlignPlaneSumsC) -> AlignPlaneSums:
    return AlignPlaneSums.from_array(np.frombuffer(bytes(c), np.int64))


def align_plane_solve(sums: AlignPlaneSums) -> Tuple[np.ndarray, float]:
    """pcs_align_plane_solve: the point-to-plane step of one set of plane sums on the host — no context, no GPU. Returns
    (delta, rms_mm): delta a float64 [4, 4] in metres that moves the source towards the target's planes, rms_mm the distance to
    them. Raises PcsError (PCS_ERR_UNSUPPORTED) with fewer than six used pairs or normals that do not determine the pose."""
    lib = _libmod.load()
    c = sums.to_c()
    delta = (C.c_double * 16)()
    rms = C.c_double(0)
    rc = lib.pcs_align_plane_solve(C.byref(c), delta, C.byref(rms))
    if rc != 0:
        d = lib.pcs_last_error(None)
        raise PcsError(rc, d.decode() if d else "")
    return np.array(delta[:], np.float64).reshape(4, 4), float(rms.value)


class PcsContext:
    """One context per host thread; owns device constants, staging buffers and a HIP stream."""

    def __init__(self, streams: Sequence[StreamConfig], device: int = 0, flags: int = 0, downsample: int = 1):
        self._lib = _libmod.load()
        self._h = C.c_void_p()
        self.streams = list(streams)
        self.n_streams = len(self.streams)
        self.flags = int(flags)
        self.downsample = int(downsample)
        self.device = int(device)
        self._arr = stream_array(self.streams) if self.streams else None
        cfg = Config()
        cfg.device = device
        cfg.n_streams = self.n_streams
        cfg.streams = C.cast(self._arr, C.POINTER(StreamConfig)) if self._arr is not None else None
        cfg.flags = self.flags
        cfg.downsample = self.downsample
        rc = self._lib.pcs_create(C.byref(self._h), C.byref(cfg))
        if rc != 0:
            detail = self._lib.pcs_last_error(None)
            self._h = C.c_void_p()
            raise PcsError(rc, detail.decode() if detail else "")

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            for p in getattr(self, "_pinned", []):
                self._lib.pcs_host_free(self._h, p)
            self._pinned = []
            self._lib.pcs_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> None:
        if rc != 0:
            d = self._lib.pcs_last_error(self._h)
            raise PcsError(rc, d.decode() if d else "")

    # -- queries -----------------------------------------------------------------------------
    def stream_points(self, stream: int) -> int:
        return int(self._lib.pcs_stream_points(self._h, stream))

    def stream_math(self, stream: int) -> int:
        """0 = IEEE expansion, 1 = certified reduced-instruction arithmetic, 2 = + identity-R shortcut."""
        return int(self._lib.pcs_stream_math(self._h, stream))

    def stream_color_row_const(self, stream: int) -> bool:
        """The stream's colour row is certified independent of depth (pcs_stream_color_row_const)."""
        return bool(self._lib.pcs_stream_color_row_const(self._h, stream))

    @property
    def max_payload_shorts(self) -> int:
        return int(self._lib.pcs_max_payload_shorts(self._h))

    def set_cam_to_world(self, stream: int, m16) -> None:
        m = np.ascontiguousarray(m16, np.float32).reshape(16)
        self._check(self._lib.pcs_set_cam_to_world(self._h, stream, m.ctypes.data_as(C.POINTER(C.c_float))))

    # -- crop box ------------------------------------------------------------------------------
    def set_crop_box_mm(self, lo, hi) -> None:
        """pcs_set_crop_box_mm: keep the points whose record lies inside lo <= (x, y, z) <= hi, int16 millimetres in the world frame
        (after the int16 wrap; see the header). set_crop_box_mm(None, None) clears the box."""
        if lo is None and hi is None:
            self._check(self._lib.pcs_set_crop_box_mm(self._h, None, None))
            return
        def three(v):
            if v is None:
                return None
            a = [int(x) for x in v]
            if len(a) != 3 or any(x < -32768 or x > 32767 for x in a):
                raise ValueError("a crop box bound is three int16 values (x, y, z in millimetres)")
            return (C.c_int16 * 3)(*a)
        self._check(self._lib.pcs_set_crop_box_mm(self._h, three(lo), three(hi)))

    def crop_box_mm(self):
        """((lo_x, lo_y, lo_z), (hi_x, hi_y, hi_z)) of the box that is set, or None."""
        lo, hi = (C.c_int16 * 3)(), (C.c_int16 * 3)()
        rc = self._lib.pcs_get_crop_box_mm(self._h, lo, hi)
        if rc < 0:
            self._check(rc)
        return (tuple(int(x) for x in lo), tuple(int(x) for x in hi)) if rc == 1 else None

    def crop_payloads_device(self, d_cam_payload: Sequence[int], cam_points: Sequence[int], downsample: int,
                             d_stitched_payload: int, stitched_shorts: int, d_counts: int) -> None:
        """pcs_crop_payloads_device: the context's crop box over packed per-camera payloads (device pointers), cameras in index order,
        every downsample-th kept record written; d_counts receives len(cams) + 1 int32 on the device. Asynchronous."""
        n = len(d_cam_payload)
        ptrs = (C.c_void_p * max(n, 1))(*d_cam_payload)
        cnts = (C.c_int * max(n, 1))(*cam_points)
        self._check(self._lib.pcs_crop_payloads_device(self._h, ptrs, cnts, n, int(downsample), d_stitched_payload or None,
                                                       stitched_shorts, d_counts or None))

    # -- depth pre-filter ----------------------------------------------------------------------
    def set_depth_filter(self, cfg=True, *, temporal: bool = True, alpha: float = 0.4, delta: int = 20, persistence: int = 3,
                         hole_fill: int = 0) -> None:
        """pcs_set_depth_filter: temporal smoothing and / or fill-from-left on the Z16 rasters, upstream of every other call (the
        definition: DESIGN.md section 3). Keywords default to librealsense's; a DepthFilterConfig may be passed instead;
        set_depth_filter(None) clears the filter and frees its state. Setting a filter (again) resets the state."""
        if cfg is None:
            self._check(self._lib.pcs_set_depth_filter(self._h, None))
            return
        if not isinstance(cfg, DepthFilterConfig):
            cfg = DepthFilterConfig(int(temporal), float(alpha), int(delta), int(persistence), int(hole_fill))
        self._check(self._lib.pcs_set_depth_filter(self._h, C.byref(cfg)))

    def depth_filter(self) -> Optional[DepthFilterConfig]:
        """The filter that is set (a DepthFilterConfig), or None."""
        out = DepthFilterConfig()
        rc = self._lib.pcs_get_depth_filter(self._h, C.byref(out))
        if rc < 0:
            self._check(rc)
        return out if rc == 1 else None

    def reset_depth_filter(self) -> None:
        """Zero the temporal state of every stream (a recording looped, the scene was cut)."""
        self._check(self._lib.pcs_reset_depth_filter(self._h))

    def filter_depth_device(self, d_in: Sequence[int], d_out: Sequence[int], d_tile_kept: int = 0) -> None:
        """pcs_filter_depth_device on device pointers (ints), asynchronous; d_out[s] may equal d_in[s]. Every call advances the
        state by one frame. d_tile_kept (optional): stream_tile_base(n_streams) uint32 for process_frames_device_counted."""
        if len(d_in) != self.n_streams or len(d_out) != self.n_streams:
            raise ValueError("need one input and one output pointer per stream")
        ip = (C.c_void_p * self.n_streams)(*d_in)
        op = (C.c_void_p * self.n_streams)(*d_out)
        self._check(self._lib.pcs_filter_depth_device(self._h, ip, op, d_tile_kept or None))

    def filter_depth(self, depth: Sequence[np.ndarray]) -> List[np.ndarray]:
        """pcs_filter_depth: one frame-set of Z16 rasters through the filter (upload, launch, download); returns new arrays of
        the inputs' shapes."""
        if len(depth) != self.n_streams:
            raise ValueError("need one depth raster per stream")
        d = [np.ascontiguousarray(x, np.uint16) for x in depth]
        for s in range(self.n_streams):
            if d[s].size != self.streams[s].n_points:
                raise ValueError(f"stream {s}: depth raster has {d[s].size} pixels, expected {self.streams[s].n_points}")
        out = [np.empty_like(x) for x in d]
        ip = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in d])
        op = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in out])
        self._check(self._lib.pcs_filter_depth(self._h, ip, op))
        return out

    # -- depth decimation ----------------------------------------------------------------------
    def _src_sizes(self, src_shapes):
        if len(src_shapes) != self.n_streams:
            raise ValueError("need one source (height, width) per stream")
        ws = (C.c_int32 * self.n_streams)(*[int(w) for _, w in src_shapes])
        hs = (C.c_int32 * self.n_streams)(*[int(h) for h, _ in src_shapes])
        return ws, hs

    def decimate_depth_device(self, scale: int, src_shapes: Sequence[Tuple[int, int]], d_in: Sequence[int], d_out: Sequence[int]) -> None:
        """pcs_decimate_depth_device on device pointers (ints), asynchronous and stateless: every scale x scale block of source
        raster s (src_shapes[s] = (height, width)) to one pixel of d_out[s], which has this context's depth size — the context was
        created from types.decimated_stream_config(cfg, scale). The definition: DESIGN.md section 3."""
        if len(d_in) != self.n_streams or len(d_out) != self.n_streams:
            raise ValueError("need one input and one output pointer per stream")
        ws, hs = self._src_sizes(src_shapes)
        ip = (C.c_void_p * self.n_streams)(*d_in)
        op = (C.c_void_p * self.n_streams)(*d_out)
        self._check(self._lib.pcs_decimate_depth_device(self._h, int(scale), ws, hs, ip, op))

    def decimate_depth(self, scale: int, depth: Sequence[np.ndarray]) -> List[np.ndarray]:
        """pcs_decimate_depth: one frame-set of full-size Z16 rasters (2-D arrays) through the decimation (upload, launch,
        download); returns new arrays of this context's depth sizes."""
        if len(depth) != self.n_streams:
            raise ValueError("need one depth raster per stream")
        d = [np.ascontiguousarray(x, np.uint16) for x in depth]
        if any(x.ndim != 2 for x in d):
            raise ValueError("the source rasters must be 2-D (height, width) arrays")
        ws, hs = self._src_sizes([x.shape for x in d])
        out = [np.empty((int(st.depth.height), int(st.depth.width)), np.uint16) for st in self.streams]
        ip = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in d])
        op = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in out])
        self._check(self._lib.pcs_decimate_depth(self._h, int(scale), ws, hs, ip, op))
        return out

    # -- spatial filter ------------------------------------------------------------------------
    def spatial_filter_depth_device(self, d_in: Sequence[int], d_out: Sequence[int], *, alpha: float = 0.5, delta: int = 20,
                                    iterations: int = 2, hole_radius: int = 0) -> None:
        """pcs_spatial_filter_depth_device on device pointers (ints), asynchronous and stateless: the edge-preserving recurrence
        along every row and every column of every stream, `iterations` times (2 x iterations launches); d_out[s] may equal d_in[s].
        The rasters have this context's depth sizes. The definition: DESIGN.md section 3."""
        if len(d_in) != self.n_streams or len(d_out) != self.n_streams:
            raise ValueError("need one input and one output pointer per stream")
        cfg = SpatialFilterConfig(float(alpha), int(delta), int(iterations), int(hole_radius))
        ip = (C.c_void_p * self.n_streams)(*d_in)
        op = (C.c_void_p * self.n_streams)(*d_out)
        self._check(self._lib.pcs_spatial_filter_depth_device(self._h, C.byref(cfg), ip, op))

    def spatial_filter_depth(self, depth: Sequence[np.ndarray], *, alpha: float = 0.5, delta: int = 20, iterations: int = 2,
                             hole_radius: int = 0) -> List[np.ndarray]:
        """pcs_spatial_filter_depth: one frame-set of Z16 rasters through the spatial filter (upload, launches, download); returns
        new arrays of the inputs' shapes."""
        if len(depth) != self.n_streams:
            raise ValueError("need one depth raster per stream")
        d = [np.ascontiguousarray(x, np.uint16) for x in depth]
        for s in range(self.n_streams):
            if d[s].size != self.streams[s].n_points:
                raise ValueError(f"stream {s}: depth raster has {d[s].size} pixels, expected {self.streams[s].n_points}")
        cfg = SpatialFilterConfig(float(alpha), int(delta), int(iterations), int(hole_radius))
        out = [np.empty_like(x) for x in d]
        ip = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in d])
        op = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in out])
        self._check(self._lib.pcs_spatial_filter_depth(self._h, C.byref(cfg), ip, op))
        return out

    # -- a2 twin -----------------------------------------------------------------------------
    def copy_pointcloud_xyzrgb_to_buffer(self, stream: int, vertices, texcoords, color,
                                         pc_buffer: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """copyPointCloudXYZRGBToBufferSIMD (:363-616): returns (payload int16[count,5], count)."""
        vtx = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        tex = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 2)
        col = np.ascontiguousarray(color, np.uint8).reshape(-1)
        n = vtx.shape[0]
        if tex.shape[0] != n:
            raise ValueError("vertices and texcoords disagree on the point count")
        if col.size < self.streams[stream].color_bytes:
            raise ValueError("colour raster smaller than stride*height")
        out = pc_buffer if pc_buffer is not None else np.zeros((max(n, 1), POINT_SHORTS), np.int16)
        if out.dtype != np.int16 or not out.flags["C_CONTIGUOUS"] or out.size < n * POINT_SHORTS:
            # the C entry point mirrors the reference and has no capacity argument: check here
            raise ValueError(f"pc_buffer must be a C-contiguous int16 array of at least {n * POINT_SHORTS} elements")
        cnt = C.c_int(0)
        self._check(self._lib.pcs_copy_pointcloud_xyzrgb_to_buffer(
            self._h, stream, _ptr(vtx), _ptr(tex), n, _ptr(col), _ptr(out), C.byref(cnt)))
        return (out.reshape(-1, POINT_SHORTS)[:cnt.value] if pc_buffer is None else out), cnt.value

    # -- a1 twin -----------------------------------------------------------------------------
    def send_xyzrgb_pointcloud(self, stream: int, vertices, texcoords, color, buffer: np.ndarray,
                               write_header: bool = True) -> int:
        """sendXYZRGBPointcloud (:669-723) minus the socket; returns the payload size in bytes."""
        vtx = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        tex = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 2)
        col = np.ascontiguousarray(color, np.uint8).reshape(-1)
        if buffer.dtype != np.int16 or not buffer.flags["C_CONTIGUOUS"]:
            raise ValueError("buffer must be a contiguous int16 array (the reference's short* buffer)")
        size = C.c_int(0)
        self._check(self._lib.pcs_send_xyzrgb_pointcloud(
            self._h, stream, _ptr(vtx), _ptr(tex), vtx.shape[0], _ptr(col), _ptr(buffer), buffer.size,
            int(write_header), C.byref(size)))
        return size.value

    # -- fused ---------------------------------------------------------------------------------
    def process_frames(self, depth: Sequence[np.ndarray], color: Sequence[np.ndarray],
                       write_header: bool = True, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, List[int], int]:
        """Deproject + transform + pack every stream; returns (stitched int16 buffer incl. 2 header
        shorts, per-stream point counts, payload bytes). Pass `out` (allocated once, reused) in a frame loop:
        a fresh 74 MB buffer per call costs more in first-touch page faults than the whole GPU round trip."""
        if len(depth) != self.n_streams or len(color) != self.n_streams:
            raise ValueError("need one depth and one colour raster per stream")
        d = [np.ascontiguousarray(x, np.uint16).reshape(-1) for x in depth]
        c = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in color]
        for s in range(self.n_streams):
            if d[s].size != self.streams[s].n_points:
                raise ValueError(f"stream {s}: depth raster has {d[s].size} pixels, expected {self.streams[s].n_points}")
            if c[s].size < self.streams[s].color_bytes:
                raise ValueError(f"stream {s}: colour raster smaller than stride*height")
        dp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in d])
        cp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in c])
        buf = out if out is not None else np.zeros(HEADER_SHORTS + self.max_payload_shorts, np.int16)
        if buf.dtype != np.int16 or not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous int16 array")
        counts = (C.c_int * self.n_streams)()
        size = C.c_int(0)
        self._check(self._lib.pcs_process_frames(self._h, dp, cp, _ptr(buf), buf.size, int(write_header),
                                                 counts, C.byref(size)))
        return buf, [int(x) for x in counts], size.value

    def process_frames_compressed(self, depth: Sequence[np.ndarray], color: Sequence[np.ndarray],
                                  write_header: bool = True, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, List[int], int]:
        """process_frames with the payload compressed on the device ("PCZ1", pcs_process_frames_compressed): returns (uint8 buffer:
        int32 container bytes, then the container at byte 4; per-stream point counts; container bytes)."""
        if len(depth) != self.n_streams or len(color) != self.n_streams:
            raise ValueError("need one depth and one colour raster per stream")
        d = [np.ascontiguousarray(x, np.uint16).reshape(-1) for x in depth]
        c = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in color]
        for s in range(self.n_streams):
            if d[s].size != self.streams[s].n_points or c[s].size < self.streams[s].color_bytes:
                raise ValueError(f"stream {s}: raster size mismatch")
        dp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in d])
        cp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in c])
        buf = out if out is not None else np.zeros(4 + compressed_bound(self.max_payload_shorts // POINT_SHORTS), np.uint8)
        if buf.dtype != np.uint8 or not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous uint8 array")
        counts = (C.c_int * self.n_streams)()
        size = C.c_int(0)
        self._check(self._lib.pcs_process_frames_compressed(self._h, dp, cp, _ptr(buf), buf.size, int(write_header),
                                                            counts, C.byref(size)))
        return buf, [int(x) for x in counts], size.value

    # -- payload codec ("PCZ1") ------------------------------------------------------------------
    def compress_payload_device(self, d_payload: int, n_points: int, d_out: int, out_capacity: int, d_out_bytes: int = 0) -> None:
        """Asynchronous; see pcs_compress_payload_device. Device pointers as ints."""
        self._check(self._lib.pcs_compress_payload_device(self._h, d_payload or None, n_points, d_out, out_capacity, d_out_bytes or None))

    def decompress_payload_device(self, d_in: int, in_bytes: int, n_points: int, d_payload: int, payload_shorts: int) -> None:
        """Asynchronous; the caller vouches for the container (compressed_info accepted it). See pcs_decompress_payload_device."""
        self._check(self._lib.pcs_decompress_payload_device(self._h, d_in, in_bytes, n_points, d_payload or None, payload_shorts))

    def decompress_payload(self, container, d_payload: int, payload_shorts: int) -> int:
        """Validate a container held in host memory, upload it and decode it into d_payload; returns the record count."""
        buf = np.ascontiguousarray(np.frombuffer(container, np.uint8) if isinstance(container, (bytes, bytearray)) else container)
        n = C.c_int(0)
        self._check(self._lib.pcs_decompress_payload(self._h, _ptr(buf), buf.nbytes, d_payload or None, payload_shorts, C.byref(n)))
        return n.value

    def submit_frames(self, depth: Sequence[np.ndarray], color: Sequence[np.ndarray]) -> int:
        """Queue one frame-set (uploads + kernel) and return its ticket; see pcs_submit_frames. The arrays must be
        C-contiguous uint16 / uint8 already (no conversion copy is made) and stay alive until collect_frames."""
        if len(depth) != self.n_streams or len(color) != self.n_streams:
            raise ValueError("need one depth and one colour raster per stream")
        for s in range(self.n_streams):
            d, c = depth[s], color[s]
            if d.dtype != np.uint16 or c.dtype != np.uint8 or not d.flags["C_CONTIGUOUS"] or not c.flags["C_CONTIGUOUS"]:
                raise ValueError("submit_frames wants contiguous uint16 depth and uint8 colour arrays")
            if d.size != self.streams[s].n_points or c.size < self.streams[s].color_bytes:
                raise ValueError(f"stream {s}: raster size mismatch")
        dp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in depth])
        cp = (C.c_void_p * self.n_streams)(*[_ptr(x) for x in color])
        t = C.c_int(-1)
        self._check(self._lib.pcs_submit_frames(self._h, dp, cp, C.byref(t)))
        self._inflight = getattr(self, "_inflight", {})
        self._inflight[t.value] = (depth, color)          # keep the rasters alive
        return t.value

    def collect_frames(self, ticket: int, out: Optional[np.ndarray] = None,
                       write_header: bool = True) -> Tuple[np.ndarray, List[int], int]:
        buf = out if out is not None else np.zeros(HEADER_SHORTS + self.max_payload_shorts, np.int16)
        if buf.dtype != np.int16 or not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous int16 array")
        counts = (C.c_int * self.n_streams)()
        size = C.c_int(0)
        try:
            self._check(self._lib.pcs_collect_frames(self._h, int(ticket), _ptr(buf), buf.size, int(write_header),
                                                     counts, C.byref(size)))
        finally:
            getattr(self, "_inflight", {}).pop(ticket, None)
        return buf, [int(x) for x in counts], size.value

    def process_frames_device(self, d_depth: Sequence[int], d_color: Sequence[int], d_payload: int,
                              payload_shorts: int, d_counts: int = 0) -> None:
        """Asynchronous launch on device pointers (ints). See pcs_process_frames_device."""
        dp = (C.c_void_p * self.n_streams)(*d_depth)
        cp = (C.c_void_p * self.n_streams)(*d_color)
        self._check(self._lib.pcs_process_frames_device(self._h, dp, cp, d_payload, payload_shorts,
                                                        d_counts or None))

    def stream_tile_base(self, stream: int) -> int:
        """Index of the stream's first tile in a per-tile array (stream == n_streams: the number of tiles in all)."""
        return int(self._lib.pcs_stream_tile_base(self._h, stream))

    def process_frames_device_counted(self, d_depth: Sequence[int], d_color: Sequence[int], d_tile_kept: int, d_payload: int,
                                      payload_shorts: int, d_counts: int = 0) -> None:
        """pcs_process_frames_device with the per-tile kept counts handed in by the producer (no count pass)."""
        dp = (C.c_void_p * self.n_streams)(*d_depth)
        cp = (C.c_void_p * self.n_streams)(*d_color)
        self._check(self._lib.pcs_process_frames_device_counted(self._h, dp, cp, d_tile_kept, d_payload, payload_shorts,
                                                                d_counts or None))

    def process_frames_device_batch(self, d_depth: Sequence[Sequence[int]], d_color: Sequence[Sequence[int]],
                                    d_payload: Sequence[int], payload_shorts: int,
                                    d_counts: Optional[Sequence[int]] = None) -> None:
        """K frame-sets per call (pcs_process_frames_device_batch): d_depth[k][s], d_color[k][s], d_payload[k]."""
        k = len(d_payload)
        if len(d_depth) != k or len(d_color) != k:
            raise ValueError("need one raster list per frame-set")
        flat_d = [p for row in d_depth for p in row]
        flat_c = [p for row in d_color for p in row]
        if len(flat_d) != k * self.n_streams or len(flat_c) != k * self.n_streams:
            raise ValueError("every frame-set needs one depth and one colour pointer per stream")
        dp = (C.c_void_p * len(flat_d))(*flat_d)
        cp = (C.c_void_p * len(flat_c))(*flat_c)
        pp = (C.c_void_p * k)(*d_payload)
        cc = (C.c_void_p * k)(*d_counts) if d_counts is not None else None
        self._check(self._lib.pcs_process_frames_device_batch(self._h, k, dp, cp, pp, payload_shorts, cc))

    def copy_pointcloud_xyzrgb_to_buffer_device(self, stream: int, d_vertices: int, d_texcoords: int, n_points: int,
                                                d_color: int, d_pc_buffer: int, d_out_points: int = 0) -> None:
        """The a2 twin on device pointers (ints), asynchronous on the context's stream; d_out_points (optional) receives one int."""
        self._check(self._lib.pcs_copy_pointcloud_xyzrgb_to_buffer_device(
            self._h, int(stream), d_vertices or None, d_texcoords or None, int(n_points), d_color or None, d_pc_buffer or None,
            d_out_points or None))

    def copy_pointclouds_xyzrgb_to_buffer_device(self, clouds: Sequence[Tuple[int, int, int, int, int, int]],
                                                 d_out_points: int = 0) -> None:
        """Batched a2 twin on device pointers: clouds = [(stream, n_points, d_vertices, d_texcoords, d_color, d_out)]."""
        arr = (CloudDesc * max(len(clouds), 1))()
        for i, (stream, n, v, t, col, out) in enumerate(clouds):
            arr[i].stream, arr[i].n_points = int(stream), int(n)
            arr[i].vertices, arr[i].texcoords, arr[i].color, arr[i].pc_buffer = v or None, t or None, col or None, out or None
        self._check(self._lib.pcs_copy_pointclouds_xyzrgb_to_buffer_device(self._h, len(clouds), arr, d_out_points or None))

    def deproject(self, stream: int, depth) -> Tuple[np.ndarray, np.ndarray]:
        d = np.ascontiguousarray(depth, np.uint16).reshape(-1)
        n = self.streams[stream].n_points
        if d.size != n:
            raise ValueError("depth raster size mismatch")
        vtx = np.empty((n, 3), np.float32)
        tex = np.empty((n, 2), np.float32)
        self._check(self._lib.pcs_deproject(self._h, stream, _ptr(d), _ptr(vtx), _ptr(tex)))
        return vtx, tex

    # -- a7 ------------------------------------------------------------------------------------
    def stitch_device(self, d_cam_payload: Sequence[int], cam_points: Sequence[int], downsample: int,
                      d_stitched_payload: int, stitched_shorts: int) -> int:
        n = len(d_cam_payload)
        ptrs = (C.c_void_p * n)(*d_cam_payload)
        cnts = (C.c_int * n)(*cam_points)
        total = C.c_int(0)
        self._check(self._lib.pcs_stitch_device(self._h, ptrs, cnts, n, downsample, d_stitched_payload,
                                                stitched_shorts, C.byref(total)))
        return total.value

    def transform_payloads_device(self, d_cam_payload: Sequence[int], cam_points: Sequence[int], transforms, downsample: int,
                                  d_stitched_payload: int, stitched_shorts: int):
        """pcs_transform_payloads_device: what the reference's pcs-multicamera-optimized does to every camera's payload before it
        concatenates them (decode, pcl::transformPointCloud(transform[i]), re-encode; src/pcs-multicamera-optimized.cpp:226-265,
        289). Returns (points per camera, total points)."""
        from .types import PayloadDesc
        n = len(d_cam_payload)
        descs = (PayloadDesc * max(n, 1))()
        for i in range(n):
            descs[i].d_payload = d_cam_payload[i]
            descs[i].n_points = int(cam_points[i])
            m = np.asarray(transforms[i], np.float32).reshape(-1)
            if m.size != 16:
                raise ValueError("a transform is 16 floats, row-major 4x4")
            for k in range(16):
                descs[i].transform[k] = float(m[k])
        per = (C.c_int * max(n, 1))()
        total = C.c_int(0)
        self._check(self._lib.pcs_transform_payloads_device(self._h, n, descs, int(downsample), d_stitched_payload, stitched_shorts,
                                                            per, C.byref(total)))
        return [int(per[i]) for i in range(n)], total.value

    def set_voxel_tail(self, tail: int) -> None:
        """0 = by the leaf (default), 1 = bucket tail, 2 = LSD sort + segmented mean, 3 = LSD latched after a flagged call
        (what a caller of the device forms sets when it reads a voxel count of -1, before it runs the call again); see
        pcs_set_voxel_tail."""
        self._check(self._lib.pcs_set_voxel_tail(self._h, int(tail)))

    def voxel_tail_reruns(self) -> int:
        """How often the LSD tail was latched on this context after a flagged bucket-tail call (pcs_voxel_tail_reruns)."""
        return int(self._lib.pcs_voxel_tail_reruns(self._h))

    def inject_voxel_stall(self, launches: int) -> None:
        """Fault injection: the next `launches` bucket-tail launches of this process end flagged (pcs_inject_voxel_stall)."""
        self._check(self._lib.pcs_inject_voxel_stall(int(launches)))

    # -- voxel grid (defined by this build; see include/pcs_hip.h) --------------------------------
    def voxel_grid(self, payload: np.ndarray, leaf_mm: int) -> np.ndarray:
        """Voxel-grid downsample of packed records (int16 [n,5]) -> int16 [n_voxels,5]."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        self._check(self._lib.pcs_voxel_grid(self._h, _ptr(p), p.shape[0], int(leaf_mm), _ptr(out), out.size, C.byref(cnt)))
        return out[:cnt.value].copy()

    def voxel_grid_device(self, d_payload: int, n_points: int, leaf_mm: int, d_out: int, out_shorts: int,
                          d_out_points: int = 0) -> None:
        self._check(self._lib.pcs_voxel_grid_device(self._h, d_payload, n_points, int(leaf_mm), d_out, out_shorts,
                                                    d_out_points or None))

    def voxel_grid_device_counted(self, d_payload: int, d_n_points: int, max_points: int, leaf_mm: int, d_out: int,
                                  out_shorts: int, d_out_points: int = 0) -> None:
        """The point count is read from device memory (d_n_points) when the kernels run: no host round trip after a
        compaction launch. See pcs_voxel_grid_device_counted."""
        self._check(self._lib.pcs_voxel_grid_device_counted(self._h, d_payload, d_n_points, int(max_points), int(leaf_mm),
                                                            d_out, out_shorts, d_out_points or None))

    # -- radius outlier removal (defined by this build; see include/pcs_hip.h) ---------------------
    def radius_outlier(self, payload: np.ndarray, radius_mm: int, min_neighbors: int) -> np.ndarray:
        """Packed records (int16 [n,5]) -> the records with at least min_neighbors others within radius_mm, input order
        (pcs_radius_outlier: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        self._check(self._lib.pcs_radius_outlier(self._h, _ptr(p), p.shape[0], int(radius_mm), int(min_neighbors), _ptr(out),
                                                 p.shape[0] * POINT_SHORTS, C.byref(cnt)))
        return out[:cnt.value].copy()

    def radius_outlier_device(self, d_payload: int, n_points: int, radius_mm: int, min_neighbors: int, d_out: int, out_shorts: int,
                              d_out_points: int) -> None:
        """Asynchronous; device pointers as ints; *d_out_points (int32, required) receives the kept count. See
        pcs_radius_outlier_device."""
        self._check(self._lib.pcs_radius_outlier_device(self._h, d_payload or None, int(n_points), int(radius_mm), int(min_neighbors),
                                                        d_out or None, out_shorts, d_out_points or None))

    def radius_outlier_device_counted(self, d_payload: int, d_n_points: int, max_points: int, radius_mm: int, min_neighbors: int,
                                      d_out: int, out_shorts: int, d_out_points: int) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_radius_outlier_device_counted."""
        self._check(self._lib.pcs_radius_outlier_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                                int(radius_mm), int(min_neighbors), d_out or None, out_shorts,
                                                                d_out_points or None))

    # -- statistical outlier removal (defined by this build; see include/pcs_hip.h) ----------------
    def stat_outlier(self, payload: np.ndarray, mean_k: int, std_mul_milli: int, max_dist_mm: int):
        """Packed records (int16 [n,5]) -> (the records whose summed distance to their mean_k nearest neighbours within
        max_dist_mm is at most mean + std_mul_milli / 1000 deviations of the cloud's, input order; the statistics block as a
        dict) (pcs_stat_outlier: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        stats = StatOutlierStatsC()
        params = StatOutlierParams.make(mean_k, std_mul_milli, max_dist_mm)
        self._check(self._lib.pcs_stat_outlier(self._h, _ptr(p), p.shape[0], C.byref(params), _ptr(out), p.shape[0] * POINT_SHORTS,
                                               C.byref(cnt), C.byref(stats)))
        return out[:cnt.value].copy(), stats.as_dict()

    def stat_outlier_device(self, d_payload: int, n_points: int, params: StatOutlierParams, d_out: int, out_shorts: int,
                            d_out_points: int, d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints; *d_out_points (int32, required) receives the kept count, d_stats (eight int64,
        optional) the statistics block. params may be None (refused). See pcs_stat_outlier_device."""
        self._check(self._lib.pcs_stat_outlier_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                      d_out or None, out_shorts, d_out_points or None, d_stats or None))

    def stat_outlier_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: StatOutlierParams, d_out: int,
                                    out_shorts: int, d_out_points: int, d_stats: int = 0) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_stat_outlier_device_counted."""
        self._check(self._lib.pcs_stat_outlier_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                              C.byref(params) if params is not None else None, d_out or None, out_shorts,
                                                              d_out_points or None, d_stats or None))

    # -- Euclidean clusters (defined by this build; see include/pcs_hip.h) --------------------------
    def cluster_filter(self, payload: np.ndarray, tolerance_mm: int, min_size: int, max_size: int = 0):
        """Packed records (int16 [n,5]) -> (the records of the clusters — connected components of "within tolerance_mm of each
        other" — that hold min_size..max_size records (max_size 0: no upper bound), input order; the statistics block as a dict)
        (pcs_cluster_filter: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        stats = ClusterStatsC()
        params = ClusterParams.make(tolerance_mm, min_size, max_size)
        self._check(self._lib.pcs_cluster_filter(self._h, _ptr(p), p.shape[0], C.byref(params), _ptr(out), p.shape[0] * POINT_SHORTS,
                                                 C.byref(cnt), C.byref(stats)))
        return out[:cnt.value].copy(), stats.as_dict()

    def cluster_filter_device(self, d_payload: int, n_points: int, params: ClusterParams, d_out: int, out_shorts: int,
                              d_out_points: int, d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints; *d_out_points (int32, required) receives the kept count, d_stats (eight int64,
        optional) the statistics block. params may be None (refused). See pcs_cluster_filter_device."""
        self._check(self._lib.pcs_cluster_filter_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                        d_out or None, out_shorts, d_out_points or None, d_stats or None))

    def cluster_filter_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: ClusterParams, d_out: int,
                                      out_shorts: int, d_out_points: int, d_stats: int = 0) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_cluster_filter_device_counted."""
        self._check(self._lib.pcs_cluster_filter_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                                C.byref(params) if params is not None else None, d_out or None, out_shorts,
                                                                d_out_points or None, d_stats or None))

    def cluster_labels(self, payload: np.ndarray, tolerance_mm: int):
        """Packed records (int16 [n,5]) -> (labels int32 [n]: the smallest input index in every record's cluster; sizes int32 [n]:
        its cluster's record count; the number of clusters) (pcs_cluster_labels: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        n = p.shape[0]
        labels = np.zeros(max(n, 1), np.int32)
        sizes = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(-1)
        self._check(self._lib.pcs_cluster_labels(self._h, _ptr(p) if n else None, n, int(tolerance_mm), _ptr(labels), _ptr(sizes),
                                                 C.byref(cnt)))
        return labels[:n].copy(), sizes[:n].copy(), int(cnt.value)

    def cluster_labels_device(self, d_payload: int, n_points: int, tolerance_mm: int, d_labels: int, d_sizes: int,
                              d_n_clusters: int) -> None:
        """Asynchronous; device pointers as ints; d_labels receives n_points int32, d_sizes (optional, 0 for none) the same shape,
        *d_n_clusters (int32, required) the number of clusters. See pcs_cluster_labels_device."""
        self._check(self._lib.pcs_cluster_labels_device(self._h, d_payload or None, int(n_points), int(tolerance_mm), d_labels or None,
                                                        d_sizes or None, d_n_clusters or None))

    def cluster_objects(self, payload: np.ndarray, tolerance_mm: int, min_size: int, max_size: int = 0, max_objects: int = 1024):
        """Packed records (int16 [n,5]) -> (the object table: a structured array (types.CLUSTER_OBJECT_DTYPE) of the first
        min(n_objects, max_objects) clusters that hold min_size..max_size records, by ascending label, with their box and integer
        sums; n_objects, the full count; object_of int32 [n]: every record's object, -1 for none)
        (pcs_cluster_objects: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        n = p.shape[0]
        table = np.zeros(max(int(max_objects), 1), CLUSTER_OBJECT_DTYPE)
        object_of = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(-1)
        params = ClusterParams.make(tolerance_mm, min_size, max_size)
        self._check(self._lib.pcs_cluster_objects(self._h, _ptr(p) if n else None, n, C.byref(params),
                                                  C.cast(table.ctypes.data, C.POINTER(ClusterObject)) if max_objects else None,
                                                  int(max_objects), C.byref(cnt), _ptr(object_of)))
        return table[:min(int(cnt.value), int(max_objects))].copy(), int(cnt.value), object_of[:n].copy()

    def cluster_objects_device(self, d_payload: int, n_points: int, params: ClusterParams, out: ClusterObjectsOut) -> None:
        """Asynchronous; `out` (types.ClusterObjectsOut) holds the device pointers: the table and *n_objects, optionally object_of,
        the filtered payload with its count, and the statistics block. params and out may be None (refused). See
        pcs_cluster_objects_device."""
        self._check(self._lib.pcs_cluster_objects_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                         C.byref(out) if out is not None else None))

    def cluster_objects_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: ClusterParams,
                                       out: ClusterObjectsOut) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_cluster_objects_device_counted."""
        self._check(self._lib.pcs_cluster_objects_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                                 C.byref(params) if params is not None else None,
                                                                 C.byref(out) if out is not None else None))

    # -- object boxes (defined by this build; see include/pcs_hip.h) ---------------------------------
    def object_boxes(self, payload: np.ndarray, object_of: np.ndarray, n_objects: int, max_objects: int = 1024) -> np.ndarray:
        """Packed records (int16 [n,5]), their object_of (int32 [n]) and the object count -> the boxes: a structured array
        (types.OBJECT_BOX_DTYPE) of min(n_objects, max_objects) entries with the count, the first and second moments, three axes,
        the rank and the extents along the axes (pcs_object_boxes: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        o = np.ascontiguousarray(object_of, np.int32).reshape(-1)
        if o.shape[0] != p.shape[0]:
            raise ValueError(f"object_of has {o.shape[0]} entries for {p.shape[0]} records")
        boxes = np.zeros(max(int(max_objects), 1), OBJECT_BOX_DTYPE)
        self._check(self._lib.pcs_object_boxes(self._h, _ptr(p) if p.shape[0] else None, p.shape[0], _ptr(o) if o.shape[0] else None,
                                               int(n_objects), int(max_objects), C.cast(_ptr(boxes), C.POINTER(ObjectBox))))
        return boxes[:min(max(int(n_objects), 0), int(max_objects))].copy()

    def object_boxes_device(self, d_payload: int, n_points: int, d_object_of: int, d_n_objects: int, max_objects: int, d_boxes: int) -> None:
        """Asynchronous; device pointers as ints: the payload, object_of (int32 per record), *d_n_objects (int32), d_boxes
        (max_objects entries of 128 bytes). See pcs_object_boxes_device."""
        self._check(self._lib.pcs_object_boxes_device(self._h, d_payload or None, int(n_points), d_object_of or None, d_n_objects or None,
                                                      int(max_objects), d_boxes or None))

    def object_boxes_device_counted(self, d_payload: int, d_n_points: int, max_points: int, d_object_of: int, d_n_objects: int,
                                    max_objects: int, d_boxes: int) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_object_boxes_device_counted."""
        self._check(self._lib.pcs_object_boxes_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                              d_object_of or None, d_n_objects or None, int(max_objects), d_boxes or None))

    # -- plan-view maps (defined by this build; see include/pcs_hip.h) --------------------------------
    def plan_view(self, payload: np.ndarray, params: PlanParams):
        """Packed records (int16 [n,5]) -> (count uint32 [H,W], top int16 [H,W], bottom int16 [H,W], rgb uint8 [H,W,3], stats dict):
        the plan-view maps of pcs_plan_view (host arrays, staged, synchronous). Row cv, column cu."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        h, w = max(int(params.height), 1), max(int(params.width), 1)
        count, top, bottom = np.zeros((h, w), np.uint32), np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        rgb, stats = np.zeros((h, w, 3), np.uint8), PlanStats()
        maps = PlanMaps(_ptr(count), _ptr(top), _ptr(bottom), _ptr(rgb), C.addressof(stats))
        self._check(self._lib.pcs_plan_view(self._h, _ptr(p) if p.shape[0] else None, p.shape[0], C.byref(params), C.byref(maps)))
        return count, top, bottom, rgb, stats.as_dict()

    def plan_view_device(self, d_payload: int, n_points: int, params: PlanParams, maps: PlanMaps) -> None:
        """Asynchronous; device pointers as ints inside `maps` (types.PlanMaps.make): count (uint32 per cell), top, bottom (int16),
        rgb (3 bytes), stats (64 bytes). See pcs_plan_view_device."""
        self._check(self._lib.pcs_plan_view_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                   C.byref(maps) if maps is not None else None))

    def plan_view_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: PlanParams, maps: PlanMaps) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_plan_view_device_counted."""
        self._check(self._lib.pcs_plan_view_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                           C.byref(params) if params is not None else None,
                                                           C.byref(maps) if maps is not None else None))

    # -- background model and subtraction (defined by this build; see include/pcs_hip.h) ------------
    def background_create(self, cell_mm: int, max_cells: int) -> Background:
        """An empty background model on this context's device (pcs_background_create)."""
        h = C.c_void_p()
        self._check(self._lib.pcs_background_create(self._h, int(cell_mm), int(max_cells), C.byref(h)))
        return Background(self, h.value)

    def tracker_create(self, cell_mm: int, max_cells: int, max_objects: int) -> Tracker:
        """A fresh object tracker on this context's device (pcs_tracker_create)."""
        h = C.c_void_p()
        self._check(self._lib.pcs_tracker_create(self._h, int(cell_mm), int(max_cells), int(max_objects), C.byref(h)))
        return Tracker(self, h.value)

    def background_import(self, container, max_cells: int) -> Background:
        """A model from a "PCB1" container (bytes or a uint8 array), validated first (pcs_background_import)."""
        buf = _as_bytes_array(container)
        h = C.c_void_p()
        self._check(self._lib.pcs_background_import(self._h, buf.ctypes.data if buf.nbytes else None, buf.nbytes, int(max_cells), C.byref(h)))
        return Background(self, h.value)

    # -- plane segmentation (defined by this build; see include/pcs_hip.h) --------------------------
    def plane_segment(self, payload: np.ndarray, params: PlaneParams):
        """Packed records (int16 [n,5]) -> (the records in no accepted plane (params.mode 0) or in one (mode 1), input order; the
        accepted planes' models as dicts; the statistics block as a dict) (pcs_plane_segment: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), POINT_SHORTS), np.int16)
        cnt = C.c_int(0)
        models = (PlaneModel * max(int(params.max_planes), 1))()
        stats = PlaneStats()
        self._check(self._lib.pcs_plane_segment(self._h, _ptr(p), p.shape[0], C.byref(params), _ptr(out), p.shape[0] * POINT_SHORTS,
                                                C.byref(cnt), models, C.byref(stats)))
        return out[:cnt.value].copy(), [m.as_dict() for m in models], stats.as_dict()

    def plane_segment_device(self, d_payload: int, n_points: int, params: PlaneParams, d_out: int, out_shorts: int, d_out_points: int,
                             d_models: int = 0, d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints; *d_out_points (int32, required) receives the kept count, d_models (max_planes
        blocks of 64 bytes, optional) the models, d_stats (eight int64, optional) the statistics block. params may be None (refused).
        See pcs_plane_segment_device."""
        self._check(self._lib.pcs_plane_segment_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                       d_out or None, out_shorts, d_out_points or None, d_models or None, d_stats or None))

    def plane_segment_device_counted(self, d_payload: int, d_n_points: int, max_points: int, params: PlaneParams, d_out: int,
                                     out_shorts: int, d_out_points: int, d_models: int = 0, d_stats: int = 0) -> None:
        """The record count is read from device memory (d_n_points, clamped to 0..max_points) when the kernels run. See
        pcs_plane_segment_device_counted."""
        self._check(self._lib.pcs_plane_segment_device_counted(self._h, d_payload or None, d_n_points or None, int(max_points),
                                                               C.byref(params) if params is not None else None, d_out or None, out_shorts,
                                                               d_out_points or None, d_models or None, d_stats or None))

    def plane_labels(self, payload: np.ndarray, params: PlaneParams):
        """Packed records (int16 [n,5]) -> (labels int32 [n]: the accepted plane a record is an inlier of, -1 for none; the number of
        accepted planes; the models as dicts; the statistics block as a dict) (pcs_plane_labels: host arrays, staged, synchronous)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        n = p.shape[0]
        labels = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(-1)
        models = (PlaneModel * max(int(params.max_planes), 1))()
        stats = PlaneStats()
        self._check(self._lib.pcs_plane_labels(self._h, _ptr(p) if n else None, n, C.byref(params), _ptr(labels), C.byref(cnt), models,
                                               C.byref(stats)))
        return labels[:n].copy(), int(cnt.value), [m.as_dict() for m in models], stats.as_dict()

    def plane_labels_device(self, d_payload: int, n_points: int, params: PlaneParams, d_labels: int, d_n_planes: int, d_models: int = 0,
                            d_stats: int = 0) -> None:
        """Asynchronous; device pointers as ints; d_labels receives n_points int32, *d_n_planes (int32, required) the number of
        accepted planes. See pcs_plane_labels_device."""
        self._check(self._lib.pcs_plane_labels_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                      d_labels or None, d_n_planes or None, d_models or None, d_stats or None))

    def plane_count_inliers_device(self, d_payload: int, n_points: int, models, d_counts: int) -> None:
        """models: a sequence of PlaneModel (host) — nx, ny, nz, off and threshold are read; d_counts receives one int64 per model:
        the records with |N . p - off| <= threshold. See pcs_plane_count_inliers_device."""
        arr = (PlaneModel * max(len(models), 1))(*models)
        self._check(self._lib.pcs_plane_count_inliers_device(self._h, d_payload or None, int(n_points), arr, len(models), d_counts or None))

    # -- surface normals (defined by this build; see include/pcs_hip.h) -----------------------------
    def estimate_normals(self, payload: np.ndarray, radius_mm: int, min_neighbors: int, flatness: int = 0, viewpoint_mm=None,
                         want_valid: bool = False):
        """Packed records (int16 [n,5]) -> int16 [n,4]: every record's unit normal times 16384 and its neighbour count, four zeros
        where it has none (pcs_estimate_normals: host arrays, staged, synchronous). viewpoint_mm: the point valid normals are
        turned towards (None: the component of largest magnitude is positive). With want_valid: (normals, valid count)."""
        p = np.ascontiguousarray(payload, np.int16).reshape(-1, POINT_SHORTS)
        out = np.zeros((max(p.shape[0], 1), NORMAL_SHORTS), np.int16)
        params = NormalParams.make(radius_mm, min_neighbors, flatness, viewpoint_mm)
        cnt = C.c_int(-1)
        self._check(self._lib.pcs_estimate_normals(self._h, _ptr(p) if p.shape[0] else None, p.shape[0], C.byref(params),
                                                   _ptr(out) if p.shape[0] else None, C.byref(cnt)))
        out = out[:p.shape[0]].copy()
        return (out, int(cnt.value)) if want_valid else out

    def estimate_normals_device(self, d_payload: int, n_points: int, params: NormalParams, d_normals: int, d_valid: int = 0) -> None:
        """Asynchronous; device pointers as ints; d_normals receives 4 n_points int16, *d_valid (optional, int32) the number of
        valid records. params: NormalParams.make(radius_mm, min_neighbors, flatness, viewpoint_mm). See
        pcs_estimate_normals_device."""
        self._check(self._lib.pcs_estimate_normals_device(self._h, d_payload or None, int(n_points), C.byref(params) if params is not None else None,
                                                          d_normals or None, d_valid or None))

    # -- extrinsics refinement (defined by this build; see include/pcs_hip.h) ----------------------
    def align_sums(self, source: np.ndarray, target: np.ndarray, max_dist_mm: int, want_dist2: bool = False):
        """Packed records (int16 [n,5]) of two overlapping payloads -> the alignment sums of the source against the target
        (pcs_align_sums: host arrays, staged, synchronous). With want_dist2: (sums, dist2), dist2 a uint32 array with every source
        record's squared distance to its match, 0xFFFFFFFF when it has none."""
        s = np.ascontiguousarray(source, np.int16).reshape(-1, POINT_SHORTS)
        t = np.ascontiguousarray(target, np.int16).reshape(-1, POINT_SHORTS)
        out = AlignSumsC()
        dist2 = np.zeros(max(s.shape[0], 1), np.uint32) if want_dist2 else None
        self._check(self._lib.pcs_align_sums(self._h, _ptr(s) if s.shape[0] else None, s.shape[0], _ptr(t) if t.shape[0] else None,
                                             t.shape[0], int(max_dist_mm), C.byref(out), _ptr(dist2) if want_dist2 else None))
        sums = _sums_from_c(out)
        return (sums, dist2[:s.shape[0]].copy()) if want_dist2 else sums

    def align_sums_device(self, d_source: int, n_source: int, d_target: int, n_target: int, max_dist_mm: int, d_sums: int,
                          d_dist2: int = 0) -> None:
        """Asynchronous; device pointers as ints; *d_sums receives eighteen int64, d_dist2 (optional) n_source uint32. See
        pcs_align_sums_device."""
        self._check(self._lib.pcs_align_sums_device(self._h, d_source or None, int(n_source), d_target or None, int(n_target),
                                                    int(max_dist_mm), d_sums or None, d_dist2 or None))

    def align_payloads_device(self, d_source: int, n_source: int, d_target: int, n_target: int, *, max_dist_mm: int,
                              iterations: int = 20, source_stride: int = 1, eps_rot_rad: float = 0.0, eps_trans_mm: float = 0.0,
                              init=None, trace: int = 0) -> Tuple[np.ndarray, AlignReport]:
        """pcs_align_payloads_device: the ICP loop over two device payloads. Returns (matrix, report): the refined float32 [4, 4]
        in metres that moves the source onto the target, starting from `init` (identity when None), and an AlignReport. A loop
        whose solve refused does not raise: report.status is PCS_ERR_UNSUPPORTED, report.stop_reason ALIGN_STOP_REFUSED and the
        matrix the last good one. trace: how many iterations' F_k and S_k to record."""
        m0 = np.ascontiguousarray(np.eye(4, dtype=np.float32) if init is None else np.asarray(init, np.float32)).reshape(-1)
        if m0.size != 16:
            raise ValueError("init is 16 floats, row-major 4x4")
        params = AlignParams(int(max_dist_mm), int(iterations), int(source_stride), 0, float(eps_rot_rad), float(eps_trans_mm))
        out = np.zeros(16, np.float32)
        ntr = max(int(trace), 0)
        tf = np.zeros((max(ntr, 1), 16), np.float32)
        ts = (AlignSumsC * max(ntr, 1))()
        rep = AlignReportC()
        rep.trace_capacity = ntr
        rep.trace_transforms = tf.ctypes.data if ntr else None
        rep.trace_sums = C.addressof(ts) if ntr else None
        rc = self._lib.pcs_align_payloads_device(self._h, d_source or None, int(n_source), d_target or None, int(n_target),
                                                 C.byref(params), m0.ctypes.data_as(C.POINTER(C.c_float)),
                                                 out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(rep))
        detail = ""
        if rc != 0:
            d = self._lib.pcs_last_error(self._h)
            detail = d.decode() if d else ""
            if not (rc == -4 and rep.stop_reason == 2 and rep.iterations > 0):      # anything but a refused solve
                raise PcsError(rc, detail)
        n = int(rep.trace_count)
        report = AlignReport(int(rep.iterations), int(rep.stop_reason), int(rc), detail, int(rep.first_matched), int(rep.first_considered),
                             int(rep.last_matched), int(rep.last_considered), float(rep.first_rms_mm), float(rep.last_rms_mm),
                             tf[:n].reshape(n, 4, 4).copy(), [_sums_from_c(ts[k]) for k in range(n)])
        return out.reshape(4, 4), report

    def align_payloads(self, source: np.ndarray, target: np.ndarray, **kw) -> Tuple[np.ndarray, AlignReport]:
        """Host-array convenience over align_payloads_device: uploads both payloads (int16 [n,5]), runs the loop, frees them."""
        s = np.ascontiguousarray(source, np.int16).reshape(-1, POINT_SHORTS)
        t = np.ascontiguousarray(target, np.int16).reshape(-1, POINT_SHORTS)
        d_s = self.device_malloc(max(s.nbytes, 16))
        d_t = self.device_malloc(max(t.nbytes, 16))
        try:
            if s.nbytes:
                self.memcpy_h2d(d_s, s)
            if t.nbytes:
                self.memcpy_h2d(d_t, t)
            return self.align_payloads_device(d_s, s.shape[0], d_t, t.shape[0], **kw)
        finally:
            self.device_free(d_s)
            self.device_free(d_t)

    # -- extrinsics refinement, point to plane (defined by this build; see include/pcs_hip.h) -------
    def align_plane_sums(self, source: np.ndarray, target: np.ndarray, target_normals: np.ndarray, max_dist_mm: int,
                         want_dist2: bool = False):
        """Packed records (int16 [n,5]) of two overlapping payloads and the target's normals (int16 [m,4], what estimate_normals
        returns) -> the point-to-plane sums of the source against the target (pcs_align_plane_sums: host arrays, staged,
        synchronous). With want_dist2: (sums, dist2) as align_sums."""
        s = np.ascontiguousarray(source, np.int16).reshape(-1, POINT_SHORTS)
        t = np.ascontiguousarray(target, np.int16).reshape(-1, POINT_SHORTS)
        nrm = np.ascontiguousarray(target_normals, np.int16).reshape(-1, NORMAL_SHORTS)
        if nrm.shape[0] != t.shape[0]:
            raise ValueError("target_normals needs one row of four shorts per target record")
        if nrm.shape[0] and nrm.ctypes.data % 8:
            buf = np.empty(nrm.size + 4, np.int16)                     # (a view at an odd offset: copy to an 8-byte aligned place)
            off = (-buf.ctypes.data % 8) // 2
            buf[off:off + nrm.size] = nrm.reshape(-1)
            nrm = buf[off:off + nrm.size].reshape(-1, NORMAL_SHORTS)
        out = AlignPlaneSumsC()
        dist2 = np.zeros(max(s.shape[0], 1), np.uint32) if want_dist2 else None
        self._check(self._lib.pcs_align_plane_sums(self._h, _ptr(s) if s.shape[0] else None, s.shape[0], _ptr(t) if t.shape[0] else None,
                                                   t.shape[0], nrm.ctypes.data if t.shape[0] else None, int(max_dist_mm), C.byref(out),
                                                   _ptr(dist2) if want_dist2 else None))
        sums = _plane_sums_from_c(out)
        return (sums, dist2[:s.shape[0]].copy()) if want_dist2 else sums

    def align_plane_sums_device(self, d_source: int, n_source: int, d_target: int, n_target: int, d_target_normals: int, max_dist_mm: int,
                                d_sums: int, d_dist2: int = 0) -> None:
        """Asynchronous; device pointers as ints; d_target_normals 4 n_target int16 (8-byte aligned); *d_sums receives sixty
        int64, d_dist2 (optional) n_source uint32. See pcs_align_plane_sums_device."""
        self._check(self._lib.pcs_align_plane_sums_device(self._h, d_source or None, int(n_source), d_target or None, int(n_target),
                                                          d_target_normals or None, int(max_dist_mm), d_sums or None, d_dist2 or None))

    def align_payloads_plane_device(self, d_source: int, n_source: int, d_target: int, n_target: int, *, max_dist_mm: int,
                                    normals: NormalParams, iterations: int = 6, source_stride: int = 1, eps_rot_rad: float = 0.0,
                                    eps_trans_mm: float = 0.0, init=None, trace: int = 0) -> Tuple[np.ndarray, AlignPlaneReport]:
        """pcs_align_payloads_plane_device: the point-to-plane loop over two device payloads; `normals` (NormalParams.make(...))
        says how the target's normals are estimated. Returns (matrix, report) as align_payloads_device; a loop whose solve refused
        does not raise."""
        m0 = np.ascontiguousarray(np.eye(4, dtype=np.float32) if init is None else np.asarray(init, np.float32)).reshape(-1)
        if m0.size != 16:
            raise ValueError("init is 16 floats, row-major 4x4")
        params = AlignPlaneParams(int(max_dist_mm), int(iterations), int(source_stride), 0, float(eps_rot_rad), float(eps_trans_mm), normals)
        out = np.zeros(16, np.float32)
        ntr = max(int(trace), 0)
        tf = np.zeros((max(ntr, 1), 16), np.float32)
        ts = (AlignPlaneSumsC * max(ntr, 1))()
        rep = AlignPlaneReportC()
        rep.trace_capacity = ntr
        rep.trace_transforms = tf.ctypes.data if ntr else None
        rep.trace_sums = C.addressof(ts) if ntr else None
        rc = self._lib.pcs_align_payloads_plane_device(self._h, d_source or None, int(n_source), d_target or None, int(n_target),
                                                       C.byref(params), m0.ctypes.data_as(C.POINTER(C.c_float)),
                                                       out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(rep))
        detail = ""
        if rc != 0:
            d = self._lib.pcs_last_error(self._h)
            detail = d.decode() if d else ""
            if not (rc == -4 and rep.stop_reason == 2 and rep.iterations > 0):      # anything but a refused solve
                raise PcsError(rc, detail)
        n = int(rep.trace_count)
        report = AlignPlaneReport(int(rep.iterations), int(rep.stop_reason), int(rc), detail, int(rep.first_matched), int(rep.first_used),
                                  int(rep.first_considered), int(rep.last_matched), int(rep.last_used), int(rep.last_considered),
                                  float(rep.first_rms_mm), float(rep.last_rms_mm), tf[:n].reshape(n, 4, 4).copy(),
                                  [_plane_sums_from_c(ts[k]) for k in range(n)])
        return out.reshape(4, 4), report

    def align_payloads_plane(self, source: np.ndarray, target: np.ndarray, **kw) -> Tuple[np.ndarray, AlignPlaneReport]:
        """Host-array convenience over align_payloads_plane_device: uploads both payloads (int16 [n,5]), runs the loop, frees them."""
        s = np.ascontiguousarray(source, np.int16).reshape(-1, POINT_SHORTS)
        t = np.ascontiguousarray(target, np.int16).reshape(-1, POINT_SHORTS)
        d_s = self.device_malloc(max(s.nbytes, 16))
        d_t = self.device_malloc(max(t.nbytes, 16))
        try:
            if s.nbytes:
                self.memcpy_h2d(d_s, s)
            if t.nbytes:
                self.memcpy_h2d(d_t, t)
            return self.align_payloads_plane_device(d_s, s.shape[0], d_t, t.shape[0], **kw)
        finally:
            self.device_free(d_s)
            self.device_free(d_t)

    def process_frames_voxel_device(self, d_depth: Sequence[int], d_color: Sequence[int], leaf_mm: int, d_out: int,
                                    out_shorts: int, d_out_points: int = 0) -> None:
        """Rasters -> voxel grid without the stitched cloud (pcs_process_frames_voxel_device)."""
        if len(d_depth) != self.n_streams or len(d_color) != self.n_streams:
            raise ValueError("need one depth and one colour pointer per stream")
        dp = (C.c_void_p * self.n_streams)(*d_depth)
        cp = (C.c_void_p * self.n_streams)(*d_color)
        self._check(self._lib.pcs_process_frames_voxel_device(self._h, dp, cp, int(leaf_mm), d_out, out_shorts,
                                                              d_out_points or None))

    def process_frames_voxel_partials_device(self, d_depth: Sequence[int], d_color: Sequence[int], leaf_mm: int,
                                             d_keys: int, d_partials: int, capacity: int, d_n_partials: int) -> None:
        """Rasters -> voxel partials (raw keys + sums) in caller arrays: what a rank contributes to a multi-GPU voxel grid
        (pcs_process_frames_voxel_partials_device)."""
        if len(d_depth) != self.n_streams or len(d_color) != self.n_streams:
            raise ValueError("need one depth and one colour pointer per stream")
        dp = (C.c_void_p * self.n_streams)(*d_depth)
        cp = (C.c_void_p * self.n_streams)(*d_color)
        self._check(self._lib.pcs_process_frames_voxel_partials_device(self._h, dp, cp, int(leaf_mm), d_keys, d_partials,
                                                                       int(capacity), d_n_partials))

    def voxel_grid_from_partials_device(self, d_keys: int, d_partials: int, n_partials: int, leaf_mm: int, d_out: int,
                                        out_shorts: int, d_out_points: int = 0, d_n_partials: int = 0) -> None:
        """Concatenated partials of any number of ranks -> the voxel grid (pcs_voxel_grid_from_partials_device)."""
        self._check(self._lib.pcs_voxel_grid_from_partials_device(self._h, d_keys, d_partials, int(n_partials),
                                                                  d_n_partials or None, int(leaf_mm), d_out, out_shorts,
                                                                  d_out_points or None))

    # -- voxel sink: several contexts of one device pre-aggregate into this context's workspace (pcs_voxel_sink_*) -----------------
    def voxel_sink_begin(self, capacity_points: int, leaf_mm: int):
        """Open a sink on this context's stream for `capacity_points` pixels in all; returns the opaque sink (a ctypes buffer) the
        other two calls take. The caller orders the streams (pcs_hip.h)."""
        sink = (C.c_uint64 * 24)()
        self._check(self._lib.pcs_voxel_sink_begin(self._h, int(capacity_points), int(leaf_mm), C.addressof(sink)))
        return sink

    def process_frames_voxel_into_sink_device(self, d_depth: Sequence[int], d_color: Sequence[int], sink) -> None:
        """This context's rasters under its flags -> partials in the sink's workspace, on this context's stream."""
        if len(d_depth) != self.n_streams or len(d_color) != self.n_streams:
            raise ValueError("need one depth and one colour pointer per stream")
        dp = (C.c_void_p * self.n_streams)(*d_depth)
        cp = (C.c_void_p * self.n_streams)(*d_color)
        self._check(self._lib.pcs_process_frames_voxel_into_sink_device(self._h, dp, cp, C.addressof(sink)))

    def voxel_sink_finish(self, sink, d_out: int, out_shorts: int, d_out_points: int = 0) -> None:
        """The tail over everything the sink received, on this context's stream (pcs_voxel_sink_finish)."""
        self._check(self._lib.pcs_voxel_sink_finish(self._h, C.addressof(sink), d_out, out_shorts, d_out_points or None))

    # -- plumbing ------------------------------------------------------------------------------
    def set_stream(self, hip_stream: int) -> None:
        self._check(self._lib.pcs_set_stream(self._h, hip_stream or None))

    def use_stream_beside(self, other: "PcsContext") -> bool:
        """Replace this context's own stream by one that is seen to run beside `other`'s (pcs_use_stream_beside): what two contexts
        used in turn need to overlap. True when such a stream was found."""
        rc = self._lib.pcs_use_stream_beside(self._h, other._h)
        if rc < 0:
            self._check(rc)
        return rc == 1

    def get_stream(self) -> int:
        return int(self._lib.pcs_get_stream(self._h) or 0)

    def synchronize(self) -> None:
        self._check(self._lib.pcs_synchronize(self._h))

    def timer_begin(self) -> None:
        self._check(self._lib.pcs_timer_begin(self._h))

    def timer_end(self) -> None:
        self._check(self._lib.pcs_timer_end(self._h))

    def timer_elapsed_ms(self) -> float:
        ms = C.c_float(0)
        self._check(self._lib.pcs_timer_elapsed_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def kernel_timing(self, enable: bool) -> None:
        self._check(self._lib.pcs_kernel_timing(self._h, int(enable)))

    def kernel_times_ms(self, capacity: int = 65536) -> np.ndarray:
        arr = (C.c_float * capacity)()
        n = C.c_int(0)
        self._check(self._lib.pcs_kernel_times_ms(self._h, arr, capacity, C.byref(n)))
        return np.array(arr[:min(n.value, capacity)], dtype=np.float32)

    def host_array(self, shape, dtype) -> np.ndarray:
        """A numpy array in page-locked host memory (freed with the context). Use it for the rasters and the
        stitched buffer handed to process_frames so the PCIe copies run at link speed."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        self._check(self._lib.pcs_host_malloc(self._h, C.byref(p), max(n, 16)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        buf = (C.c_uint8 * max(n, 16)).from_address(p.value)
        return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def host_register(self, a: np.ndarray) -> None:
        """Page-lock an array the caller owns (pcs_host_register); the host entry points then run zero copy on it."""
        self._check(self._lib.pcs_host_register(self._h, _ptr(a), a.nbytes))

    def host_unregister(self, a: np.ndarray) -> None:
        self._check(self._lib.pcs_host_unregister(self._h, _ptr(a)))

    def device_malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.pcs_device_malloc(self._h, C.byref(p), nbytes))
        return int(p.value)

    def device_free(self, d_ptr: int) -> None:
        self._check(self._lib.pcs_device_free(self._h, d_ptr))

    def memcpy_h2d(self, d_dst: int, src: np.ndarray) -> None:
        src = np.ascontiguousarray(src)
        self._check(self._lib.pcs_memcpy_h2d(self._h, d_dst, _ptr(src), src.nbytes))

    def memcpy_d2h(self, dst: np.ndarray, d_src: int) -> None:
        self._check(self._lib.pcs_memcpy_d2h(self._h, _ptr(dst), d_src, dst.nbytes))
