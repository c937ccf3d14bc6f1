#!/usr/bin/env python3
"""GPU box: what does the depth decimation (pcs_decimate_depth_device) cost on 8 x 1280x720, and what does the stitch behind it save?

Method of DESIGN.md section 7 and of tools/depth_filter_probe.py: device-resident synthetic frame-sets in a ring whose depth
rasters alone are more than twice the 256 MiB Infinity Cache, one launch counter through warm-up and the timed calls, so every call
reads cold sources from HBM (the decimation has no state; its outputs rotate through four sets). Every call is bracketed by its own
hipEvent pair: median and minimum of 200 calls after 20 warm-ups.

Per scale (2, 3, 4, 8): the decimation alone, with the bytes it moves (2 W H in + 2 Wd Hd out per stream) and their share of
8 TB/s; then, in the same process and alternating, `decimate + pcs_process_frames_device` on the decimated context beside
`pcs_process_frames_device` on the full-size context (colour rasters from a ring of their own, cold too). There is no pass / fail
bar on these times.

    python tools/decimate_probe.py [calls = 200] [warm-ups = 20] [all | decimate (the decimation's own legs only)]
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
DECIMATE_ONLY = len(sys.argv) > 3 and sys.argv[3] == "decimate"
S, W, H = 8, 1280, 720
SCALES = (2, 3, 4, 8)
INFINITY_CACHE_BYTES = 256 << 20
PEAK_GBS = 8000.0
N_SEEDS = 4                     # distinct frames in the ring (their copies differ in address, which is what the caches see)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("decimate_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    full_cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n = W * H
    set_bytes = S * n * 2
    R = -(-2 * INFINITY_CACHE_BYTES // set_bytes) + 2
    seeds = [[torch.from_numpy(Syn.synth_depth(W, H, s, seed=Syn.SEED + k).reshape(-1).view(np.int16).copy()).to(dev) for s in range(S)]
             for k in range(N_SEEDS)]
    ring = [[seeds[k % N_SEEDS][s].clone() for s in range(S)] for k in range(R)]
    in_ptrs = [[t.data_ptr() for t in fs] for fs in ring]
    col = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    cb = full_cfgs[0].color_bytes
    RC = -(-2 * INFINITY_CACHE_BYTES // (S * cb)) + 2
    col_ring = [[c.clone() for c in col] for _ in range(RC)]
    col_ptrs = [[t.data_ptr() for t in fs] for fs in col_ring]
    pay = [torch.empty(S * n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(4)]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    print(f"{S} x {W}x{H}: ring of {R} frame-sets of depth ({R * set_bytes / 1e6:.0f} MB) and {RC} of colour ({RC * S * cb / 1e6:.0f} MB), "
          f"{CALLS} calls after {WARM} warm-ups", flush=True)

    k = [0]

    def timed(name, call, mb=0.0):
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
        line = f"{name:58s} per call: median {med:7.2f} us  min {lo:7.2f} us"
        if mb:
            line += f" | {mb:5.2f} MB: {mb / med * 1e3 / PEAK_GBS * 100:5.1f} % (median) {mb / lo * 1e3 / PEAK_GBS * 100:5.1f} % (min) of 8 TB/s"
        print(line, flush=True)
        return med, lo

    full = PcsContext(full_cfgs)
    full.set_stream(stream.cuda_stream)

    def stitch_full(i):
        full.process_frames_device(in_ptrs[i % R], col_ptrs[i % RC], pay[i % 4].data_ptr(), S * n * 5)

    src_shapes = [(H, W)] * S
    for scale in SCALES:
        wd, hd = W // scale, H // scale
        ctx = PcsContext([decimated_stream_config(c, scale) for c in full_cfgs])
        ctx.set_stream(stream.cuda_stream)
        outs = [[torch.empty(wd * hd, dtype=torch.int16, device=dev) for _ in range(S)] for _ in range(4)]
        out_ptrs = [[t.data_ptr() for t in fs] for fs in outs]
        mb = S * (2 * n + 2 * wd * hd) / 1e6

        def decimate(i):
            ctx.decimate_depth_device(scale, src_shapes, in_ptrs[i % R], out_ptrs[i % 4])

        def chain(i):
            decimate(i)
            ctx.process_frames_device(out_ptrs[i % 4], col_ptrs[i % RC], pay[i % 4].data_ptr(), S * wd * hd * 5)

        timed(f"scale {scale}: decimate -> {wd}x{hd}", decimate, mb)
        if DECIMATE_ONLY:
            ctx.close()
            continue
        res = {"chain": [], "full": []}
        for rnd in range(2):               # alternate the two, twice: whatever else the box does falls on both
            res["chain"].append(timed(f"scale {scale}: decimate + process_frames_device (decimated) #{rnd}", chain))
            res["full"].append(timed(f"         process_frames_device (full size) #{rnd}", stitch_full))
        a, b = min(r[0] for r in res["chain"]), min(r[0] for r in res["full"])
        print(f"scale {scale}: decimated chain {a:.2f} us against the full-size stitch {b:.2f} us (median per call, best of 2): {b - a:+.2f} us", flush=True)
        ctx.close()
    full.close()


if __name__ == "__main__":
    main()
