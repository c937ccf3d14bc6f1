#!/usr/bin/env python3
"""GPU box: what does Euclidean cluster extraction (pcs_cluster_filter_device, pcs_cluster_labels_device) cost on the stitched payload
of 8 x 1280x720, and where does the time go? The cloud, the ring and the method are tools/stat_outlier_probe.py's, and the yardstick
is that filter: its knn launch does the same 27-cell walk over the same index (cell edge = max_dist_mm = tolerance_mm) plus a list,
the union launch the walk plus the union-find. Both run here, in one session, on one cloud.

The payload is the synthetic frames' with invalid depth dropped (PCS_FLAG_DROP_INVALID: the filter knows nothing of invalid depth),
plus a stated share of records scattered uniformly over the payload's bounding box, mixed in at random positions. Method of
DESIGN.md section 7: device-resident payloads in a ring of more than twice the 256 MiB Infinity Cache, so every call reads its
payload cold from HBM. For tolerance_mm in {10, 20, 40}:

  the clusters, the largest, the kept share at min_size MIN_SIZE;
  the time of each of the filter's fourteen launches (pcs_kernel_timing: one event pair per launch), median of the timed calls;
  the index build (launches 0 to 5), the union launch and the rest stated apart;
  the time of the whole call (one event pair per call, kernel timing off), median and minimum;
  the labels form's eleven launches;
  the yardstick: pcs_stat_outlier_device with mean_k 8, std_mul_milli 1000, max_dist_mm = the tolerance: its knn launch and whole call.

There is no pass / fail bar on these figures. Everything printed is also written to the output file.

    python tools/cluster_probe.py [output = profiles/cluster_probe.txt] [calls = 10] [warm-ups = 2] [scatter share in percent = 2]
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
from pointcloud_stitching_amd.types import (CLUSTER_LABEL_LAUNCHES, CLUSTER_LABEL_STAGES, CLUSTER_LAUNCHES, CLUSTER_STAGES, CLUSTER_STATS_FIELDS,
                                            FLAG_DROP_INVALID, STAT_OUTLIER_LAUNCHES, STAT_OUTLIER_STAGES, ClusterParams, StatOutlierParams)

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cluster_probe.txt")
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 2
SCATTER_PERCENT = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
TOLERANCES = (10, 20, 40)
MIN_SIZE = 100
YARDSTICK_K = 8
assert len(CLUSTER_STAGES) == CLUSTER_LAUNCHES and len(CLUSTER_LABEL_STAGES) == CLUSTER_LABEL_LAUNCHES


def main():
    if not torch.cuda.is_available():
        raise SystemExit("cluster_probe needs the GPU: there is nothing to time without one")
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
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    say("# python tools/cluster_probe.py")
    say(f"{S} x {W}x{H}, invalid depth dropped: {n_scene} records + {n_scatter} scattered ({SCATTER_PERCENT:g} %) over the bounding box "
        f"{lo.tolist()} .. {hi.tolist()} mm = {n} records, {raw / 1e6:.1f} MB; ring of {R} payloads ({R * raw / 1e6:.0f} MB); "
        f"{CALLS} calls after {WARM} warm-ups")

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

    for tol in TOLERANCES:
        params = ClusterParams.make(tol, MIN_SIZE, 0)

        def call_filter():
            i = k[0]
            k[0] += 1
            ctx.cluster_filter_device(ring[i % R].data_ptr(), n, params, outs[i % 3].data_ptr(), n * 5, kept_word.data_ptr(), block.data_ptr())

        def call_labels():
            i = k[0]
            k[0] += 1
            ctx.cluster_labels_device(ring[i % R].data_ptr(), n, tol, labels.data_ptr(), sizes.data_ptr(), kept_word.data_ptr())

        yard = StatOutlierParams.make(YARDSTICK_K, 1000, tol)

        def call_yardstick():
            i = k[0]
            k[0] += 1
            ctx.stat_outlier_device(ring[i % R].data_ptr(), n, yard, outs[i % 3].data_ptr(), n * 5, kept_word.data_ptr(), block.data_ptr())

        call_filter()
        ctx.synchronize()
        kept = int(kept_word.item())
        stats = dict(zip(CLUSTER_STATS_FIELDS, block.tolist()))
        again = outs[(k[0] - 1) % 3][:kept * 5].clone()
        call_filter()
        ctx.synchronize()
        assert kept == int(kept_word.item()) and torch.equal(again, outs[(k[0] - 1) % 3][:kept * 5]), "two runs differ"
        assert stats == dict(zip(CLUSTER_STATS_FIELDS, block.tolist())) and stats["kept"] == kept and stats["considered"] == n
        call_labels()
        ctx.synchronize()
        first = labels.clone()
        assert int(kept_word.item()) == stats["clusters"] and int(sizes.max().item()) == stats["largest"]
        assert int((sizes >= MIN_SIZE).sum().item()) == kept and bool((labels <= torch.arange(n, device=dev, dtype=torch.int32)).all().item())
        call_labels()
        ctx.synchronize()
        assert torch.equal(first, labels), "two runs label differently"

        us, med = timed(call_filter, CLUSTER_LAUNCHES)
        say(f"[tolerance {tol:3d} mm, min_size {MIN_SIZE}] kept {kept} of {n} = {100.0 * kept / n:6.2f} % ({stats['clusters']} clusters, "
            f"{stats['kept_clusters']} kept, largest {stats['largest']}) | whole call: median {statistics.median(us):8.1f} us  min {min(us):8.1f} us")
        say("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(CLUSTER_STAGES, med)) + f" | sum {med.sum():.1f}")
        say(f"    index build (launches 0 to 5): {med[:6].sum():.1f} us | union: {med[7]:.1f} us | init, roots, flag: {med[6] + med[8] + med[9]:.1f} us | "
            f"compaction and stats: {med[10:].sum():.1f} us")
        union_us = med[7]
        us, med = timed(call_labels, CLUSTER_LABEL_LAUNCHES)
        say(f"    labels form: whole call median {statistics.median(us):8.1f} us | per launch (median us): "
            + ", ".join(f"{name} {v:.1f}" for name, v in zip(CLUSTER_LABEL_STAGES, med)))
        us, med = timed(call_yardstick, STAT_OUTLIER_LAUNCHES)
        knn_us = med[STAT_OUTLIER_STAGES.index("knn")]
        say(f"    yardstick, pcs_stat_outlier_device k {YARDSTICK_K}, max_dist {tol} mm, same cloud and cell edge: knn {knn_us:.1f} us, whole call median "
            f"{statistics.median(us):8.1f} us | union / knn = {union_us / knn_us:.2f}")
    ctx.close()
    out_file.close()


if __name__ == "__main__":
    main()
