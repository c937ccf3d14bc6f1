#!/usr/bin/env python3
"""GPU box: what do the alignment sums (pcs_align_sums_device) and the ICP loop (pcs_align_payloads_device) cost at working size, and
where does the time go?

The target is the stitched payload of S synthetic 1280x720 cameras with invalid depth dropped (PCS_FLAG_DROP_INVALID: the match knows
nothing of invalid depth), S = 1 and 8; the source is camera 0's payload seen through a small offset (2 degrees, 15 mm:
pcs_transform_payloads_device), the situation the loop is for. For max_dist 20 and 60 mm and source stride 1 and 4:

  the matched share and the rms of the first correspondence step;
  the time of each launch of one sums call (pcs_kernel_timing: one event pair per launch), median of the timed calls: the six launches
  of the target's index, match, reduce;
  the loop's period: (time of a call with ITER iterations - time of a call with 1 iteration) / (ITER - 1), whole calls timed on the host
  around a synchronous call — it holds the 144-byte copy and the host solve — and the per-launch times of its three launches;
  the byte floor of one step: 10 B read per source record considered, the index build's traffic over the target (10 B read twice,
  8 B written per record, 12 B per slot touched), and at least 8 B per candidate visited — the candidates are not counted here, so the
  floor printed is the first two terms at 8 TB/s, for scale: a gather is not bounded by it.

There is no pass / fail bar on these figures.

    python tools/align_probe.py [calls = 20] [warm-ups = 3] [loop iterations = 10]
"""
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloud_stitching_amd import synthetic as Syn
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import ALIGN_INDEX_LAUNCHES, ALIGN_ITERATION_LAUNCHES, ALIGN_SUMS_LAUNCHES, FLAG_DROP_INVALID

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ITER = int(sys.argv[3]) if len(sys.argv) > 3 else 10
W, H = 1280, 720
PEAK_GBS = 8000.0
LAUNCHES = ("clear", "insert", "cell sums", "cell scan", "cell starts", "scatter", "match", "reduce")
assert len(LAUNCHES) == ALIGN_SUMS_LAUNCHES


def offset_matrix():
    a = np.array([0.3, -0.5, 0.81])
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(2.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
    T[:3, 3] = (0.009, -0.008, 0.009)
    return T.astype(np.float32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("align_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    for S in (1, 8):
        cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
        n_max = S * W * H
        ctx = PcsContext(cfgs, flags=FLAG_DROP_INVALID)
        ctx.set_stream(stream.cuda_stream)
        d_depth = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).view(np.int16).copy()).to(dev) for s in range(S)]
        d_color = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
        counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        target = torch.empty(n_max * 5, dtype=torch.int16, device=dev)
        ctx.process_frames_device([t.data_ptr() for t in d_depth], [t.data_ptr() for t in d_color], target.data_ptr(), n_max * 5, counts.data_ptr())
        ctx.synchronize()
        per_cam = counts.cpu().numpy()
        n_target, n_cam0 = int(per_cam[S]), int(per_cam[0])
        source = torch.empty(n_cam0 * 5 + 8, dtype=torch.int16, device=dev)
        ctx.transform_payloads_device([target.data_ptr()], [n_cam0], [offset_matrix()], 1, source.data_ptr(), n_cam0 * 5)
        sums = torch.zeros(18, dtype=torch.int64, device=dev)
        print(f"target: {S} x {W}x{H}, invalid depth dropped = {n_target} records; source: camera 0 through 2 degrees / 15 mm = {n_cam0} records; "
              f"{CALLS} calls after {WARM} warm-ups, loops of {ITER} iterations", flush=True)
        for max_dist in (20, 60):
            for stride in (1, 4):
                n_source = n_cam0 // stride
                # the sums call takes a payload, not a stride: every stride-th record, copied once
                src = source[:n_cam0 * 5].view(-1, 5)[::stride][:n_source].contiguous().view(-1) if stride > 1 else source

                def call():
                    ctx.align_sums_device(src.data_ptr(), n_source, target.data_ptr(), n_target, max_dist, sums.data_ptr())

                call()
                ctx.synchronize()
                first = sums.cpu().numpy().copy()
                call()
                ctx.synchronize()
                assert (first == sums.cpu().numpy()).all(), "two runs differ"
                matched = int(first[1])
                rms = math.sqrt(first[17] / matched) if matched else 0.0
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
                per = ctx.kernel_times_ms().reshape(CALLS, ALIGN_SUMS_LAUNCHES) * 1e3
                med = np.median(per, axis=0)

                # the loop (kernel timing still on: index once, then transform / match / reduce per iteration)
                def loop(iters):
                    t0 = time.perf_counter()
                    _, rep = ctx.align_payloads_device(source.data_ptr(), n_cam0, target.data_ptr(), n_target, max_dist_mm=max_dist,
                                                       iterations=iters, source_stride=stride)
                    return (time.perf_counter() - t0) * 1e6, rep

                ctx.kernel_timing(False)
                loop(2)
                t_one = statistics.median(loop(1)[0] for _ in range(5))
                t_many = statistics.median(loop(ITER)[0] for _ in range(5))
                ctx.kernel_timing(True)
                ctx.kernel_times_ms()
                _, rep = loop(ITER)
                lp = ctx.kernel_times_ms() * 1e3
                ctx.kernel_timing(False)
                assert lp.shape[0] == ALIGN_INDEX_LAUNCHES + ALIGN_ITERATION_LAUNCHES * rep.iterations
                it = np.median(lp[ALIGN_INDEX_LAUNCHES:].reshape(rep.iterations, ALIGN_ITERATION_LAUNCHES), axis=0)
                floor_mb = (10 * n_source + (10 + 10 + 8) * n_target) / 1e6
                print(f"[max_dist {max_dist:3d} mm, stride {stride}] {n_source} source records, matched {matched} = {100.0 * matched / max(n_source, 1):5.1f} %, "
                      f"rms {rms:.2f} mm | sums call: median {statistics.median(us):8.1f} us  min {min(us):8.1f} us | "
                      f"floor {floor_mb:6.1f} MB = {floor_mb / PEAK_GBS * 1e3:5.1f} us at 8 TB/s", flush=True)
                print("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(LAUNCHES, med)) + f" | sum {med.sum():.1f}", flush=True)
                print(f"    loop: {rep.iterations} iterations, matched {rep.first_matched} -> {rep.last_matched}, rms {rep.first_rms_mm:.2f} -> "
                      f"{rep.last_rms_mm:.2f} mm | period {(t_many - t_one) / max(ITER - 1, 1):8.1f} us per iteration (host clock), one-iteration call "
                      f"{t_one:8.1f} us | per launch (median us): transform {it[0]:.1f}, match {it[1]:.1f}, reduce {it[2]:.1f}", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
