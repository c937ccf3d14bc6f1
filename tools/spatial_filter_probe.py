#!/usr/bin/env python3
"""GPU box: what does the spatial filter (pcs_spatial_filter_depth_device) cost on 8 x 1280x720, alone and inside the chain?

Method of DESIGN.md section 7, of tools/depth_filter_probe.py and of tools/decimate_probe.py: device-resident synthetic frame-sets
in a ring whose depth rasters alone are more than twice the 256 MiB Infinity Cache, one launch counter through warm-up and the
timed calls, so every call reads cold inputs from HBM (the filter has no state; its outputs rotate through four sets). Every call is
bracketed by its own hipEvent pair: median and minimum of 200 calls after 20 warm-ups.

The whole call at 1, 2 (the default) and 5 iterations, out of place; beside each figure the dependent steps of its chain (a call is
iterations x (2 W + 2 H) steps, one lane per line) and the resulting time per step. The timing does not depend on the data: the step
has no branch in it. Then, in the same process and alternating, `decimate 2 + spatial + filter + process_frames_device` beside the
same chain without the spatial call. There is no pass / fail bar on these times.

The row launch and the column launch of one iteration each on its own are not separable with events from outside the library (a
call enqueues both); take them from the kernel trace of a run of its own,
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/spatial_filter_probe.py 50 5 spatial
where they are pcs_spatial_rows_kernel and pcs_spatial_cols_kernel.

    python tools/spatial_filter_probe.py [calls = 200] [warm-ups = 20] [all | spatial (the filter's own legs only)]
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloud_stitching_amd import synthetic as Syn
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import decimated_stream_config

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 20
SPATIAL_ONLY = len(sys.argv) > 3 and sys.argv[3] == "spatial"
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
N_SEEDS = 4                     # distinct frames in the ring (their copies differ in address, which is what the caches see)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("spatial_filter_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    full_cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n = W * H
    set_bytes = S * n * 2
    R = -(-2 * INFINITY_CACHE_BYTES // set_bytes) + 2
    seeds = [[torch.from_numpy(Syn.synth_depth(W, H, s, seed=Syn.SEED + k).reshape(-1).view(np.int16).copy()).to(dev) for s in range(S)]
             for k in range(N_SEEDS)]
    ring = [[seeds[k % N_SEEDS][s].clone() for s in range(S)] for k in range(R)]
    in_ptrs = [[t.data_ptr() for t in fs] for fs in ring]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    print(f"{S} x {W}x{H}: ring of {R} frame-sets of depth ({R * set_bytes / 1e6:.0f} MB), {CALLS} calls after {WARM} warm-ups", flush=True)

    k = [0]

    def timed(name, call, steps=0):
        """`call(i)` CALLS times after WARM warm-ups, each between its own pair of events; i counts every call of the process."""
        def one():
            i = k[0]
            k[0] += 1
            call(i)
        for _ in range(WARM):
            one()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in ev:
            a.record(stream)
            one()
            b.record(stream)
        stream.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        med, lo = statistics.median(us), min(us)
        line = f"{name:66s} per call: median {med:8.2f} us  min {lo:8.2f} us"
        if steps:
            line += f" | {steps} dependent steps: {med / steps * 1e3:6.1f} ns per step (median) {lo / steps * 1e3:6.1f} (min)"
        print(line, flush=True)
        return med, lo

    full = PcsContext(full_cfgs)
    full.set_stream(stream.cuda_stream)
    outs = [[torch.empty(n, dtype=torch.int16, device=dev) for _ in range(S)] for _ in range(4)]
    out_ptrs = [[t.data_ptr() for t in fs] for fs in outs]
    for it in (1, 2, 5):
        def spatial(i, it=it):
            full.spatial_filter_depth_device(in_ptrs[i % R], out_ptrs[i % 4], iterations=it)
        timed(f"spatial filter, {it} iteration(s), {W}x{H}, {2 * it} launches", spatial, it * (2 * W + 2 * H))

    def spatial_fill(i):
        full.spatial_filter_depth_device(in_ptrs[i % R], out_ptrs[i % 4], iterations=2, hole_radius=2)
    timed(f"spatial filter, 2 iterations, hole_radius 2", spatial_fill, 2 * (2 * W + 2 * H))
    full.close()
    if SPATIAL_ONLY:
        return

    scale = 2
    wd, hd = W // scale, H // scale
    ctx = PcsContext([decimated_stream_config(c, scale) for c in full_cfgs])
    ctx.set_stream(stream.cuda_stream)
    ctx.set_depth_filter(temporal=True, hole_fill=1)
    col = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    cb = full_cfgs[0].color_bytes
    RC = -(-2 * INFINITY_CACHE_BYTES // (S * cb)) + 2
    col_ring = [[c.clone() for c in col] for _ in range(RC)]
    col_ptrs = [[t.data_ptr() for t in fs] for fs in col_ring]
    pay = [torch.empty(S * wd * hd * 5 + 8, dtype=torch.int16, device=dev) for _ in range(4)]
    dec = [[torch.empty(wd * hd, dtype=torch.int16, device=dev) for _ in range(S)] for _ in range(4)]
    dec_ptrs = [[t.data_ptr() for t in fs] for fs in dec]
    src_shapes = [(H, W)] * S

    def chain(i, with_spatial):
        d = dec_ptrs[i % 4]
        ctx.decimate_depth_device(scale, src_shapes, in_ptrs[i % R], d)
        if with_spatial:
            ctx.spatial_filter_depth_device(d, d)
        ctx.filter_depth_device(d, d)
        ctx.process_frames_device(d, col_ptrs[i % RC], pay[i % 4].data_ptr(), S * wd * hd * 5)

    timed(f"spatial filter, 2 iterations, {wd}x{hd} (after decimate 2), in place", lambda i: ctx.spatial_filter_depth_device(dec_ptrs[i % 4], dec_ptrs[i % 4]),
          2 * (2 * wd + 2 * hd))
    res = {"with": [], "without": []}
    for rnd in range(2):               # alternate the two, twice: whatever else the box does falls on both
        res["with"].append(timed(f"decimate 2 + spatial + filter + process_frames_device #{rnd}", lambda i: chain(i, True)))
        res["without"].append(timed(f"decimate 2 + filter + process_frames_device #{rnd}", lambda i: chain(i, False)))
    a, b = min(r[0] for r in res["with"]), min(r[0] for r in res["without"])
    print(f"chain with the spatial filter {a:.2f} us against {b:.2f} us without (median per call, best of 2): {a - b:+.2f} us", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
