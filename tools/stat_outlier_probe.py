#!/usr/bin/env python3
"""GPU box: what does statistical outlier removal (pcs_stat_outlier_device) cost on the stitched payload of 8 x 1280x720, and where
does the time go? The cloud, the ring and the method are tools/outlier_probe.py's, so that the two filters' figures for one index
edge (max_dist_mm here, radius_mm there) stand side by side when both probes run in one session.

The payload is the synthetic frames' with invalid depth dropped (PCS_FLAG_DROP_INVALID: the filter knows nothing of invalid depth),
plus a stated share of records scattered uniformly over the payload's bounding box, mixed in at random positions. Method of
DESIGN.md section 7 and of tools/codec_probe.py: device-resident payloads in a ring of more than twice the 256 MiB Infinity Cache, so
every call reads its payload cold from HBM. For a small grid of (mean_k, std_mul_milli, max_dist_mm), mean_k in {8, 16, 50}:

  the kept share, the dense count and the threshold;
  the time of each of the call's fourteen launches (pcs_kernel_timing: one event pair per launch), median of the timed calls;
  the index build (launches 0 to 5, the radius filter's own) and the knn launch stated apart;
  the time of the whole call (one event pair per call, kernel timing off), median and minimum;
  the byte floor: 10 B read per record plus 10 B written per kept record, at 8 TB/s. A gather is not bounded by it; it is printed for scale.

There is no pass / fail bar on these figures.

    python tools/stat_outlier_probe.py [calls = 10] [warm-ups = 2] [scatter share in percent = 2]
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
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, STAT_OUTLIER_LAUNCHES, STAT_OUTLIER_STAGES, STAT_STATS_FIELDS, StatOutlierParams

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 2
SCATTER_PERCENT = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
PEAK_GBS = 8000.0
GRID = ((8, 1000, 20), (16, 1000, 20), (8, 1000, 40), (16, 1000, 40), (50, 1000, 40))
LAUNCHES = STAT_OUTLIER_STAGES
assert len(LAUNCHES) == STAT_OUTLIER_LAUNCHES


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stat_outlier_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n_max = S * W * H
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = PcsContext(cfgs, flags=FLAG_DROP_INVALID)
    ctx.set_stream(stream.cuda_stream)

    d_depth = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).view(np.int16).copy()).to(dev) for s in range(S)]
    d_color = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    pay = torch.empty(n_max * 5, dtype=torch.int16, device=dev)
    ctx.process_frames_device([t.data_ptr() for t in d_depth], [t.data_ptr() for t in d_color], pay.data_ptr(), n_max * 5, counts.data_ptr())
    ctx.synchronize()
    n_scene = int(counts[S].item())
    scene = pay[:n_scene * 5].cpu().numpy().reshape(-1, 5)
    rng = np.random.default_rng(20241019)
    n_scatter = int(round(n_scene * SCATTER_PERCENT / 100.0))
    lo, hi = scene[:, :3].min(axis=0).astype(np.int64), scene[:, :3].max(axis=0).astype(np.int64)
    scatter = np.empty((n_scatter, 5), np.int16)
    scatter[:, :3] = rng.integers(lo, hi + 1, (n_scatter, 3))
    scatter[:, 3:] = rng.integers(0, 256, (n_scatter, 2))
    n = n_scene + n_scatter
    is_scatter = np.zeros(n, bool)
    is_scatter[rng.choice(n, n_scatter, replace=False)] = True
    cloud = np.empty((n, 5), np.int16)
    cloud[is_scatter], cloud[~is_scatter] = scatter, scene
    raw = 10 * n
    R = -(-2 * INFINITY_CACHE_BYTES // raw) + 2
    ring = [torch.from_numpy(cloud.reshape(-1)).to(dev) for _ in range(R)]
    outs = [torch.empty(n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(3)]
    kept_word = torch.zeros(1, dtype=torch.int32, device=dev)
    block = torch.zeros(8, dtype=torch.int64, device=dev)
    print(f"{S} x {W}x{H}, invalid depth dropped: {n_scene} records + {n_scatter} scattered ({SCATTER_PERCENT:g} %) over the bounding box "
          f"{lo.tolist()} .. {hi.tolist()} mm = {n} records, {raw / 1e6:.1f} MB; ring of {R} payloads ({R * raw / 1e6:.0f} MB); "
          f"{CALLS} calls after {WARM} warm-ups", flush=True)

    k = [0]

    def call():
        i = k[0]
        k[0] += 1
        ctx.stat_outlier_device(ring[i % R].data_ptr(), n, params, outs[i % 3].data_ptr(), n * 5, kept_word.data_ptr(), block.data_ptr())

    for mean_k, mul, dist in GRID:
        params = StatOutlierParams.make(mean_k, mul, dist)
        call()
        ctx.synchronize()
        kept = int(kept_word.item())
        stats = dict(zip(STAT_STATS_FIELDS, block.tolist()))
        again = outs[(k[0] - 1) % 3][:kept * 5].clone()
        call()
        ctx.synchronize()
        assert kept == int(kept_word.item()) and torch.equal(again, outs[(k[0] - 1) % 3][:kept * 5]), "two runs differ"
        assert stats == dict(zip(STAT_STATS_FIELDS, block.tolist())) and stats["kept"] == kept and stats["considered"] == n
        floor_mb = (raw + 10 * kept) / 1e6
        for _ in range(WARM):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in ev:
            a.record(stream)
            call()
            b.record(stream)
        stream.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        ctx.kernel_timing(True)
        for _ in range(CALLS):
            call()
        per = ctx.kernel_times_ms().reshape(CALLS, STAT_OUTLIER_LAUNCHES) * 1e3
        ctx.kernel_timing(False)
        med = np.median(per, axis=0)
        print(f"[k {mean_k:2d}, mul {mul} / 1000, max_dist {dist:3d} mm] kept {kept} of {n} = {100.0 * kept / n:6.2f} % (dense {stats['dense']}, "
              f"threshold {stats['threshold']} = {stats['threshold'] / 256.0 / mean_k:.2f} mm per neighbour) | whole call: median {statistics.median(us):8.1f} us  "
              f"min {min(us):8.1f} us | floor {floor_mb:6.1f} MB = {floor_mb / PEAK_GBS * 1e3:5.1f} us at 8 TB/s", flush=True)
        print("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(LAUNCHES, med))
              + f" | sum {med.sum():.1f}", flush=True)
        print(f"    index build (launches 0 to 5): {med[:6].sum():.1f} us | knn: {med[6]:.1f} us | everything behind it: {med[7:].sum():.1f} us", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
