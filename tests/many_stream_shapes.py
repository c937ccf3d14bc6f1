"""The shape tables of the many-stream filter tests (tests/test_filters_many_streams.py on the GPU, tests/test_many_stream_shapes_cpu.py
without one) and the rasters both run on. The three depth stages of csrc/pcs_kernels_filter.hip put every stream of a context into
one launch (blockIdx.y, up to PCS_MAX_STREAMS = 64) and every stream may have its own size, so one 64-stream context sweeps every row
width and column height the kernels switch code path on:

  NARROW   64 streams, every width 1..64 and every height 1..64 once: fewer than 8 full chunks of a row, every W % 8, the one short
           chunk of a ragged row, columns shorter than 2 kSpatialColAhead, 1 to 7 trailing outputs of a decimated row.
  WIDE     64 streams, widths and heights 65..128: both main loops of the spatial sweeps, a second 64-lane block of the row and of
           the column kernel, every remainder mod 8 on top of 8 or more full chunks, heights on either side of 96.
  MIXED17  one stream more than a stitch launch takes (kLaunchStreams = 16); a 2056-pixel row sets the workgroup size for narrow
           neighbours, and the last stream's tiles lie behind the first stitch launch.

Not a test module."""
import numpy as np

import np_spatial_filter as SP
from pointcloud_stitching_amd import synthetic as S

PCS_MAX_STREAMS = 64          # include/pcs_hip.h
LAUNCH_STREAMS = 16           # kLaunchStreams, csrc/pcs_device.h

NARROW = [(s + 1, 1 + (37 * s) % 64) for s in range(64)]                     # (w, h)
WIDE = [(65 + s, 65 + (37 * s) % 64) for s in range(64)]
MIXED17 = [(2056, 3), (1, 7), (9, 1), (64, 48), (100, 37), (1280, 2)] + [(68, 48) if k % 2 == 0 else (160, 96) for k in range(11)]
TABLES = {"NARROW": NARROW, "WIDE": WIDE, "MIXED17": MIXED17}
SEEDS = {"NARROW": 1000, "WIDE": 2000, "MIXED17": 3000}


def configs(table):
    """One synthetic stream per (w, h); the colour raster is 64 x 48 whatever the depth size."""
    return [S.synth_stream_config(w, h, s, color_size=(64, 48)) for s, (w, h) in enumerate(table)]


def spatial_rasters(name, frame=0):
    """Stream s of table `name`: np_spatial_filter.scene at its size (blends, ties, edges, zero bands)."""
    return [SP.scene(w, h, SEEDS[name] + 100 * frame + s) for s, (w, h) in enumerate(TABLES[name])]


def source_shapes(name, n):
    """(h, w) of the decimation sources at scale n, the table's shapes being the DECIMATED sizes: stream s is s % n columns and
    (s // 2) % n rows larger than n times its output, so sources are and are not multiples of the scale, and of 8."""
    return [(n * h + (s // 2) % n, n * w + s % n) for s, (w, h) in enumerate(TABLES[name])]


def decimation_sources(name, n, frame=0):
    """The scene at the source size, overlaid with two hash patterns of invalid pixels: one pixel in three, and one n x n block in
    seven as a whole (at n = 8 a block of 64 is never empty by the first pattern alone)."""
    out = []
    for s, (h, w) in enumerate(source_shapes(name, n)):
        d = SP.scene(w, h, SEEDS[name] + 100 * frame + 10 * n + s)
        r, c = np.mgrid[0:h, 0:w].astype(np.uint32)
        d[S.hash32(r * np.uint32(w) + c + np.uint32(5 + s)) % 3 == 0] = 0
        d[S.hash32((r // n) * np.uint32(65537) + c // n + np.uint32(77 * n + s)) % 7 == 0] = 0
        out.append(d)
    return out


def temporal_frames(name, n_frames=6):
    """frames[k][s]: the scene of stream s with a new noise seed per frame (neighbouring frames agree within any delta >= 13), a
    quarter of the pixels invalid by a hash that changes with the frame (the persistence rule has histories to decide on), and in
    frame 3 a band of rows divided by 4 (a disagreement with the history)."""
    frames = []
    for k in range(n_frames):
        per_stream = []
        for s, (w, h) in enumerate(TABLES[name]):
            d = SP.scene(w, h, SEEDS[name] + 100 * k + s)
            idx = np.arange(w * h, dtype=np.uint32).reshape(h, w)
            d[S.hash32(idx + np.uint32(1009 * k + 31 * s)) % 4 == 0] = 0
            if k == 3:
                d[h // 5:max(2 * h // 5, h // 5 + 1)] //= 4
            per_stream.append(d)
        frames.append(per_stream)
    return frames
