#!/usr/bin/env python3
"""GPU box: what do learning a background model (pcs_background_learn_device) and subtracting it (pcs_background_subtract_device) cost
on the stitched payload of 8 x 1280x720 and of 16 x 1920x1080, and where does the time go?

The payload is the synthetic frames' with invalid depth dropped (PCS_FLAG_DROP_INVALID). The model (cell_mm 40) is learned from 30
frame-sets of that scene, each with its own depth noise of +-2 mm (added on the device); min_seen is 15, half of them. The payloads that
are subtracted hold a stated share of FOREGROUND: records drawn uniformly from the scene's bounding box, mixed in at random positions
in place of scene records. Method of DESIGN.md section 7 and of tools/outlier_probe.py: device-resident payloads in a ring of more
than twice the 256 MiB Infinity Cache, so every call reads its payload cold from HBM. Printed:

  the learn launch's time (pcs_kernel_timing), median over the 30 frame-sets, and the model's cells and table size;
  at dilate 0 and 1 and at 10, 50 and 90 % foreground: the kept share, the time of each of the call's five launches (median), the whole
  call (one event pair per call, kernel timing off; median and minimum) and the byte floor: 10 B read per record plus 10 B written per
  kept record, at 8 TB/s. A hash probe is not bounded by it; it is printed for scale.

There is no pass / fail bar on these figures.

    python tools/background_probe.py [calls = 30] [warm-ups = 5]
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
from pointcloud_stitching_amd.types import BACKGROUND_SUBTRACT_LAUNCHES, BackgroundParams, FLAG_DROP_INVALID

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 5
SIZES = ((8, 1280, 720), (16, 1920, 1080))
INFINITY_CACHE_BYTES = 256 << 20
PEAK_GBS = 8000.0
CELL_MM, MAX_CELLS, FRAME_SETS, MIN_SEEN = 40, 4194304, 30, 15
FOREGROUND_PERCENT = (10, 50, 90)


def probe(S, W, H, dev, stream):
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n_max = S * W * H
    ctx = PcsContext(cfgs, flags=FLAG_DROP_INVALID)
    ctx.set_stream(stream.cuda_stream)
    clean = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).astype(np.int32)).to(dev) for s in range(S)]
    d_color = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    pay = torch.empty(n_max * 5, dtype=torch.int16, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241020)

    def frame_set(noise):
        depth = [torch.where(c > 0, c + (torch.randint(-2, 3, c.shape, device=dev, generator=gen, dtype=torch.int32) if noise else 0), c)
                 .to(torch.int16) for c in clean]          # (a Z16 raster's bits; depths stay far below 32768)
        stream.synchronize()
        ctx.process_frames_device([t.data_ptr() for t in depth], [t.data_ptr() for t in d_color], pay.data_ptr(), n_max * 5, counts.data_ptr())
        ctx.synchronize()
        return int(counts[S].item())

    bg = ctx.background_create(CELL_MM, MAX_CELLS)
    ctx.kernel_timing(True)
    learn_us = []
    for k in range(FRAME_SETS):
        frame_set(noise=True)
        ctx.kernel_times_ms()
        bg.learn_device_counted(pay.data_ptr(), counts.data_ptr() + 4 * S, n_max)
        learn_us.append(float(ctx.kernel_times_ms()[0]) * 1e3)
    ctx.kernel_timing(False)
    info = bg.info()
    n = frame_set(noise=False)
    scene = pay[:n * 5].cpu().numpy().reshape(-1, 5)
    raw = 10 * n
    print(f"{S} x {W}x{H}, invalid depth dropped: {n} records, {raw / 1e6:.1f} MB; model of {FRAME_SETS} frame-sets at cell_mm {CELL_MM}: "
          f"{info['cells']} cells of max_cells {MAX_CELLS} (table {32 * MAX_CELLS / 1e6:.0f} MB), overflow {info['overflow']}", flush=True)
    print(f"    learn (counted form, one launch): median {statistics.median(learn_us):.1f} us, min {min(learn_us):.1f} us per frame-set", flush=True)

    rng = np.random.default_rng(20241020)
    lo, hi = scene[:, :3].min(axis=0).astype(np.int64), scene[:, :3].max(axis=0).astype(np.int64)
    R = -(-2 * INFINITY_CACHE_BYTES // raw) + 2
    outs = [torch.empty(n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(3)]
    kept_word = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    for percent in FOREGROUND_PERCENT:
        cloud = scene.copy()
        fg = rng.choice(n, n * percent // 100, replace=False)
        cloud[fg, :3] = rng.integers(lo, hi + 1, (fg.shape[0], 3))
        ring = [torch.from_numpy(cloud.reshape(-1)).to(dev) for _ in range(R)]
        for dilate in (0, 1):
            P = BackgroundParams.make(MIN_SEEN, dilate)
            k = [0]

            def call(with_stats=True):
                i = k[0]
                k[0] += 1
                bg.subtract_device(ring[i % R].data_ptr(), n, P, outs[i % 3].data_ptr(), n * 5, kept_word.data_ptr(),
                                   stats.data_ptr() if with_stats else 0)

            call()
            ctx.synchronize()
            kept = int(kept_word.item())
            again = outs[(k[0] - 1) % 3][:kept * 5].clone()
            call()
            ctx.synchronize()
            assert kept == int(kept_word.item()) and torch.equal(again, outs[(k[0] - 1) % 3][:kept * 5]), "two runs differ"
            floor_mb = (raw + 10 * kept) / 1e6
            for _ in range(WARM):
                call()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
            for a, b in ev:
                a.record(stream)
                call(with_stats=False)
                b.record(stream)
            stream.synchronize()
            us = [a.elapsed_time(b) * 1e3 for a, b in ev]
            ctx.kernel_timing(True)
            for _ in range(CALLS):
                call()
            per = ctx.kernel_times_ms().reshape(CALLS, len(BACKGROUND_SUBTRACT_LAUNCHES)) * 1e3
            ctx.kernel_timing(False)
            med = np.median(per, axis=0)
            print(f"[foreground {percent:2d} %, dilate {dilate}] kept {kept} of {n} = {100.0 * kept / n:6.2f} % | whole call (no block): median "
                  f"{statistics.median(us):8.1f} us  min {min(us):8.1f} us | floor {floor_mb:6.1f} MB = {floor_mb / PEAK_GBS * 1e3:5.1f} us at 8 TB/s",
                  flush=True)
            print("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(BACKGROUND_SUBTRACT_LAUNCHES, med))
                  + f" | sum {med.sum():.1f}", flush=True)
        del ring
    bg.close()
    ctx.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("background_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    print(f"{CALLS} calls after {WARM} warm-ups per line", flush=True)
    for S, W, H in SIZES:
        probe(S, W, H, dev, stream)


if __name__ == "__main__":
    main()
