#!/usr/bin/env python3
"""GPU box: what does plane segmentation (pcs_plane_segment_device) cost on the stitched payload of 8 x 1280x720, and where does the
time go? The cloud, the ring and the method are tools/cluster_probe.py's: the synthetic frames' payload with invalid depth dropped
plus a stated share of records scattered over its bounding box, device-resident in a ring of more than twice the 256 MiB Infinity
Cache, so every call reads its payload cold from HBM. For iterations in {64, 256, 1024}, at distance_mm
DISTANCE and max_planes PLANES:

  the planes accepted and their inliers, the kept share;
  the time of each of the call's 8 max_planes + 1 launches (pcs_kernel_timing: one event pair per launch), median of the timed calls;
  the score launches stated apart: iterations x m inlier tests each, tests per second;
  the yardstick: the mark launch of the same round reads every record of the same cloud once (and writes a label for the inliers):
  score / mark says how many cloud reads a round's scoring is worth;
  the time of the whole call (one event pair per call, kernel timing off), median and minimum.

There is no pass / fail bar on these figures. Everything printed is also written to the output file.

    python tools/plane_probe.py [output = profiles/plane_probe.txt] [calls = 5] [warm-ups = 1] [scatter share in percent = 2]
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
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID, PLANE_STATS_FIELDS, PlaneParams, plane_stages

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plane_probe.txt")
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 1
SCATTER_PERCENT = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
ITERATIONS = (64, 256, 1024)
DISTANCE, MIN_INLIERS, PLANES, SEED = 20, 10000, 2, 1


def main():
    if not torch.cuda.is_available():
        raise SystemExit("plane_probe needs the GPU: there is nothing to time without one")
    out_file = open(OUT, "w")

    def say(text):
        print(text, flush=True)
        out_file.write(text + "\n")
        out_file.flush()

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
    models = torch.zeros(8 * PLANES, dtype=torch.int64, device=dev)
    stages = plane_stages(PLANES)
    say("# python tools/plane_probe.py")
    say(f"{S} x {W}x{H}, invalid depth dropped: {n_scene} records + {n_scatter} scattered ({SCATTER_PERCENT:g} %) over the bounding box "
        f"{lo.tolist()} .. {hi.tolist()} mm = {n} records, {raw / 1e6:.1f} MB; ring of {R} payloads ({R * raw / 1e6:.0f} MB); "
        f"{CALLS} calls after {WARM} warm-ups; distance {DISTANCE} mm, min_inliers {MIN_INLIERS}, max_planes {PLANES}, seed {SEED}")

    k = [0]

    def timed(call, launches):
        """(whole-call microseconds per call, per-launch medians in microseconds)"""
        for _ in range(WARM):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in ev:
            a.record(stream)
            call()
            b.record(stream)
        stream.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        ctx.kernel_times_ms()
        ctx.kernel_timing(True)
        for _ in range(CALLS):
            call()
        per = ctx.kernel_times_ms().reshape(CALLS, launches) * 1e3
        ctx.kernel_timing(False)
        return us, np.median(per, axis=0)

    for iterations in ITERATIONS:
        params = PlaneParams.make(DISTANCE, iterations, MIN_INLIERS, PLANES, SEED, 0)

        def call():
            i = k[0]
            k[0] += 1
            ctx.plane_segment_device(ring[i % R].data_ptr(), n, params, outs[i % 3].data_ptr(), n * 5, kept_word.data_ptr(), models.data_ptr(),
                                     block.data_ptr())

        call()
        ctx.synchronize()
        kept = int(kept_word.item())
        stats = dict(zip(PLANE_STATS_FIELDS, block.tolist()))
        found = models.clone()
        again = outs[(k[0] - 1) % 3][:kept * 5].clone()
        call()
        ctx.synchronize()
        assert kept == int(kept_word.item()) and torch.equal(again, outs[(k[0] - 1) % 3][:kept * 5]) and torch.equal(found, models), "two runs differ"
        assert stats == dict(zip(PLANE_STATS_FIELDS, block.tolist())) and stats["kept"] == kept and stats["considered"] == n
        inl = [int(found[8 * r + 5].item()) for r in range(stats["planes"])]
        m = [n] + [n - sum(inl[:r + 1]) for r in range(len(inl))]            # the clouds the rounds scored

        us, med = timed(call, len(stages))
        say(f"[iterations {iterations:4d}] kept {kept} of {n} = {100.0 * kept / n:6.2f} % ({stats['planes']} planes, inliers {inl}, "
            f"{stats['degenerate_hypotheses']} degenerate hypotheses) | whole call: median {statistics.median(us):9.1f} us  min {min(us):9.1f} us")
        say("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(stages, med)) + f" | sum {med.sum():.1f}")
        scores = [i for i, name in enumerate(stages) if name == "score"]
        marks = [i for i, name in enumerate(stages) if name == "mark"]
        for r, (i, j) in enumerate(zip(scores, marks)):
            if r >= len(m):
                break
            tests = iterations * m[r]
            say(f"    round {r}: m {m[r]}: score {med[i]:.1f} us = {tests / med[i] / 1e3:.1f} G tests/s; mark (one read of the cloud, "
                f"{10 * m[r] / 1e6:.1f} MB: {10 * m[r] / med[j] / 1e3:.0f} GB/s) {med[j]:.1f} us | score / mark = {med[i] / med[j]:.1f}")
    ctx.close()
    out_file.close()


if __name__ == "__main__":
    main()
