#!/usr/bin/env python3
"""GPU box: what do the object boxes (pcs_object_boxes_device) cost on the stitched payload of 8 x 1280x720, behind the objects call
whose object_of and count they read? The cloud, the ring and the method are tools/objects_probe.py's: the synthetic frames' payload
with invalid depth dropped plus a stated share of scattered records, a ring of device-resident payloads of more than twice the 256 MiB
Infinity Cache, so every call reads its payload cold from HBM. For tolerance_mm in {10, 20, 40}, min_size MIN_SIZE, max_objects
MAX_OBJECTS:

  the objects, the written entries, the entries of rank 3; count and sum_xyz against the object table's size and sums (exact); two
  runs byte for byte;
  the whole boxes call, one event pair per call, median and minimum; each of its launches through pcs_kernel_timing, median of the
  timed calls;
  the yardsticks, same session, same cloud: the objects call's `accumulate` launch (one grouped pass over the same records): the
  moments launch and the extents launch as ratios of it; and the whole pcs_cluster_objects_device call the boxes call follows: the
  boxes call as a share of it.

There is no pass / fail bar on these figures. Everything printed is also written to the output file.

    python tools/boxes_probe.py [output = profiles/boxes_probe.txt] [calls = 10] [warm-ups = 2] [scatter share in percent = 2]
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
from pointcloud_stitching_amd.types import (CLUSTER_OBJECT_DTYPE, CLUSTER_OBJECT_LAUNCHES, CLUSTER_OBJECT_STAGES, FLAG_DROP_INVALID, OBJECT_BOX_DTYPE,
                                            OBJECT_BOXES_LAUNCHES, ClusterObjectsOut, ClusterParams)

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "boxes_probe.txt")
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 2
SCATTER_PERCENT = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
TOLERANCES = (10, 20, 40)
MIN_SIZE = 100
MAX_OBJECTS = 1024
assert len(CLUSTER_OBJECT_STAGES) == CLUSTER_OBJECT_LAUNCHES and "accumulate" in CLUSTER_OBJECT_STAGES


def main():
    if not torch.cuda.is_available():
        raise SystemExit("boxes_probe needs the GPU: there is nothing to time without one")
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
    words = torch.zeros(16, dtype=torch.int32, device=dev)          # [4] n_objects
    object_of = torch.zeros(n, dtype=torch.int32, device=dev)
    table = torch.zeros(MAX_OBJECTS * 80, dtype=torch.uint8, device=dev)
    boxes = torch.zeros(MAX_OBJECTS * 128, dtype=torch.uint8, device=dev)
    d_nobj = words.data_ptr() + 16
    say("# python tools/boxes_probe.py")
    say(f"{S} x {W}x{H}, invalid depth dropped: {n_scene} records + {n_scatter} scattered ({SCATTER_PERCENT:g} %) over the bounding box "
        f"{lo.tolist()} .. {hi.tolist()} mm = {n} records, {raw / 1e6:.1f} MB; ring of {R} payloads ({R * raw / 1e6:.0f} MB); "
        f"{CALLS} calls after {WARM} warm-ups; min_size {MIN_SIZE}, max_objects {MAX_OBJECTS}")

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

        def call_objects():
            i = k[0]
            k[0] += 1
            ctx.cluster_objects_device(ring[i % R].data_ptr(), n, params, ClusterObjectsOut.make(
                objects=table.data_ptr(), max_objects=MAX_OBJECTS, n_objects=d_nobj, object_of=object_of.data_ptr()))

        def call_boxes():      # (every payload of the ring is the same cloud: object_of fits them all)
            i = k[0]
            k[0] += 1
            ctx.object_boxes_device(ring[i % R].data_ptr(), n, object_of.data_ptr(), d_nobj, MAX_OBJECTS, boxes.data_ptr())

        call_objects()
        call_boxes()
        ctx.synchronize()
        n_objects = int(words[4].item())
        written = min(n_objects, MAX_OBJECTS)
        first = boxes[:128 * written].clone()
        call_boxes()
        ctx.synchronize()
        assert torch.equal(first, boxes[:128 * written]), "two runs differ"
        got = first.cpu().numpy().view(OBJECT_BOX_DTYPE)
        tab = table[:80 * written].cpu().numpy().view(CLUSTER_OBJECT_DTYPE)
        assert got["count"].tolist() == tab["size"].tolist() and got["sum_xyz"].tolist() == tab["sum_xyz"].tolist(), "the sums differ from the table's"
        members = int((object_of.cpu().numpy().astype(np.int64) < written).sum() - (object_of < 0).sum().item())

        us_box, med_box = timed(call_boxes, len(OBJECT_BOXES_LAUNCHES))
        us_obj, med_obj = timed(call_objects, CLUSTER_OBJECT_LAUNCHES)
        m_box, m_obj = statistics.median(us_box), statistics.median(us_obj)
        acc = med_obj[CLUSTER_OBJECT_STAGES.index("accumulate")]
        launch = dict(zip(OBJECT_BOXES_LAUNCHES, med_box))
        say(f"[tolerance {tol:3d} mm] {n_objects} objects ({written} written), {int((got['rank'] == 3).sum())} of rank 3, largest "
            f"{int(got['count'].max(initial=0))}, {members} of {n} records in a written object")
        say(f"    boxes call: median {m_box:8.1f} us  min {min(us_box):8.1f} us")
        say("    per launch (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in launch.items()) + f" | sum {med_box.sum():.1f}")
        say(f"    yardstick, the objects call's accumulate launch: {acc:.1f} us | moments / accumulate = {launch['moments'] / acc:.2f}, "
            f"extents / accumulate = {launch['extents'] / acc:.2f}")
        say(f"    yardstick, pcs_cluster_objects_device (no filtered output): median {m_obj:8.1f} us  min {min(us_obj):8.1f} us | "
            f"boxes / objects = {m_box / m_obj:.3f}")
    ctx.close()
    out_file.close()


if __name__ == "__main__":
    main()
