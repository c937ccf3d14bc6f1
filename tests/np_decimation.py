"""numpy restatement of the depth decimation ("Depth decimation"), written from that text and from nothing
else: `decimate` (every n x n block to the lower median of its non-zero values for n = 2, 3, to their truncated mean for n >= 4)
and `decimated_config` (the stream a decimated raster belongs to, each quantity in double and rounded to float once). The GPU
kernel (csrc/pcs_kernels_filter.hip) and pcs_decimated_stream_config are held to this bit for bit.

Not a test module: the decimation tests import it."""
import ctypes as C

import numpy as np

from pointcloud_stitching_amd.types import StreamConfig


def decimate(raster, n):
    """Wd = W // n, Hd = H // n; source columns >= n Wd and rows >= n Hd are not looked at; the output is not padded."""
    d = np.asarray(raster, np.uint16)
    if d.ndim != 2 or not 2 <= n <= 8:
        raise ValueError("a 2-D raster and a scale in 2..8")
    hd, wd = d.shape[0] // n, d.shape[1] // n
    blocks = d[:n * hd, :n * wd].astype(np.int64).reshape(hd, n, wd, n).transpose(0, 2, 1, 3).reshape(hd, wd, n * n)
    k = (blocks != 0).sum(axis=-1)
    if n <= 3:
        ordered = np.sort(np.where(blocks != 0, blocks, 1 << 20), axis=-1)          # the valid ones ascending, the rest behind them
        pick = np.take_along_axis(ordered, (np.maximum(k - 1, 0) >> 1)[..., None], axis=-1)[..., 0]
    else:
        pick = blocks.sum(axis=-1) // np.maximum(k, 1)
    return np.where(k > 0, pick, 0).astype(np.uint16)


def decimated_config(cfg, n):
    """fx' = (float)((double)fx / n), ppx' = (float)(((double)ppx - (n - 1) / 2.0) / n), fy' and ppy' likewise, width' = W // n,
    height' = H // n; everything else is copied. n = 1 is the identity."""
    if not 1 <= n <= 8 or cfg.depth.width // n == 0 or cfg.depth.height // n == 0:
        raise ValueError("scale outside 1..8, or no pixel left")
    out = StreamConfig()
    C.memmove(C.byref(out), C.byref(cfg), C.sizeof(StreamConfig))
    if n == 1:
        return out
    f64, f32 = np.float64, np.float32
    out.depth.width, out.depth.height = cfg.depth.width // n, cfg.depth.height // n
    out.depth.fx = float(f32(f64(f32(cfg.depth.fx)) / f64(n)))
    out.depth.fy = float(f32(f64(f32(cfg.depth.fy)) / f64(n)))
    out.depth.ppx = float(f32((f64(f32(cfg.depth.ppx)) - f64(n - 1) / f64(2.0)) / f64(n)))
    out.depth.ppy = float(f32((f64(f32(cfg.depth.ppy)) - f64(n - 1) / f64(2.0)) / f64(n)))
    return out
