#!/usr/bin/env python3
"""GPU box: what do the plan-view maps (pcs_plan_view_device) cost on the stitched payload of 8 x 1280x720? The cloud, the ring and the
method are tools/boxes_probe.py's: the synthetic frames' payload with invalid depth dropped plus a stated share of scattered records,
a ring of device-resident payloads of more than twice the 256 MiB Infinity Cache, so every call reads its payload cold from HBM.
Seen along +z over a map that covers -4100 .. 4100 mm on both axes, for cell_mm in {10, 20, 50}:

  the statistics block; the count raster's sum against `mapped`; two runs byte for byte;
  the whole call, one event pair per call, median and minimum; each of its launches through pcs_kernel_timing, median of the timed
  calls; the accumulate launch in nanoseconds per record;
  a "wall" cloud: WALL_RECORDS records in ONE cell (heights spread over 2 m), same map: the same figures, and its accumulate launch
  per record against the probe cloud's;
  the yardsticks, same session, same cloud, two launches that make one grouped pass over the same records: the object table's
  `accumulate` launch and the boxes' `moments` launch at tolerances 10 mm (hundreds of objects) and 20 mm (one).

There is no pass / fail bar on these figures. Everything printed is also written to the output file.

    python tools/plan_probe.py [output = profiles/plan_probe.txt] [calls = 10] [warm-ups = 2] [scatter share in percent = 2]
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
from pointcloud_stitching_amd.types import (CLUSTER_OBJECT_LAUNCHES, CLUSTER_OBJECT_STAGES, FLAG_DROP_INVALID, OBJECT_BOXES_LAUNCHES, PLAN_STATS_FIELDS,
                                            PLAN_VIEW_LAUNCHES, ClusterObjectsOut, ClusterParams, PlanMaps, PlanParams)

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plan_probe.txt")
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 2
SCATTER_PERCENT = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
CELLS_MM = (10, 20, 50)
HALF_MM = 4100
WALL_RECORDS = 1 << 20
YARDSTICK_TOLERANCES = (10, 20)
MIN_SIZE = 100
MAX_OBJECTS = 1024


def main():
    if not torch.cuda.is_available():
        raise SystemExit("plan_probe needs the GPU: there is nothing to time without one")
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
    wall = np.empty((WALL_RECORDS, 5), np.int16)
    wall[:, 0], wall[:, 1] = 1003, -1507
    wall[:, 2] = rng.integers(-1000, 1000, WALL_RECORDS)
    wall[:, 3:] = rng.integers(0, 256, (WALL_RECORDS, 2))
    R_wall = -(-2 * INFINITY_CACHE_BYTES // (10 * WALL_RECORDS)) + 2
    wall_ring = [torch.from_numpy(wall.reshape(-1)).to(dev) for _ in range(R_wall)]
    say("# python tools/plan_probe.py")
    say(f"{S} x {W}x{H}, invalid depth dropped: {n_scene} records + {n_scatter} scattered ({SCATTER_PERCENT:g} %) over the bounding box "
        f"{lo.tolist()} .. {hi.tolist()} mm = {n} records, {raw / 1e6:.1f} MB; ring of {R} payloads ({R * raw / 1e6:.0f} MB); "
        f"wall: {WALL_RECORDS} records in one cell, ring of {R_wall}; {CALLS} calls after {WARM} warm-ups; up +z, the map "
        f"{-HALF_MM} .. {HALF_MM} mm on x and y")

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

    for cell in CELLS_MM:
        side = 2 * HALF_MM // cell
        cells = side * side
        params = PlanParams.make(2, 1, cell, side, side, -HALF_MM, -HALF_MM)
        d_count = torch.zeros(cells, dtype=torch.int32, device=dev)
        d_top, d_bottom = torch.zeros(cells, dtype=torch.int16, device=dev), torch.zeros(cells, dtype=torch.int16, device=dev)
        d_rgb, d_stats = torch.zeros(3 * cells, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.int64, device=dev)
        maps = PlanMaps.make(d_count.data_ptr(), d_top.data_ptr(), d_bottom.data_ptr(), d_rgb.data_ptr(), d_stats.data_ptr())
        probe_ns = None
        for name, payloads, records in (("probe cloud", ring, n), ("wall", wall_ring, WALL_RECORDS)):
            def call_plan():
                i = k[0]
                k[0] += 1
                ctx.plan_view_device(payloads[i % len(payloads)].data_ptr(), records, params, maps)

            call_plan()
            ctx.synchronize()
            first = [t.clone() for t in (d_count, d_top, d_bottom, d_rgb, d_stats)]
            call_plan()
            ctx.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(first, (d_count, d_top, d_bottom, d_rgb, d_stats))), "two runs differ"
            stats = dict(zip(PLAN_STATS_FIELDS, first[4].cpu().tolist()))
            assert int(first[0].to(torch.int64).sum().item()) == stats["mapped"] and stats["considered"] == records, "the count raster and the block disagree"
            us, med = timed(call_plan, len(PLAN_VIEW_LAUNCHES))
            launch = dict(zip(PLAN_VIEW_LAUNCHES, med))
            ns = 1e3 * launch["accumulate"] / records
            say(f"[cell {cell:2d} mm, {side} x {side} = {cells} cells, {name}] " + ", ".join(f"{f} {stats[f]}" for f in PLAN_STATS_FIELDS))
            say(f"    plan view call: median {statistics.median(us):8.1f} us  min {min(us):8.1f} us")
            say("    per launch (median us): " + ", ".join(f"{nm} {v:.1f}" for nm, v in launch.items()) + f" | sum {med.sum():.1f}")
            if probe_ns is None:
                probe_ns = ns
                say(f"    accumulate: {ns:.4f} ns per record")
            else:
                say(f"    accumulate: {ns:.4f} ns per record = {ns / probe_ns:.2f} x the probe cloud's")

    words = torch.zeros(16, dtype=torch.int32, device=dev)          # [4] n_objects
    object_of = torch.zeros(n, dtype=torch.int32, device=dev)
    table = torch.zeros(MAX_OBJECTS * 80, dtype=torch.uint8, device=dev)
    boxes = torch.zeros(MAX_OBJECTS * 128, dtype=torch.uint8, device=dev)
    d_nobj = words.data_ptr() + 16
    for tol in YARDSTICK_TOLERANCES:
        cparams = ClusterParams.make(tol, MIN_SIZE, 0)

        def call_objects():
            i = k[0]
            k[0] += 1
            ctx.cluster_objects_device(ring[i % R].data_ptr(), n, cparams, ClusterObjectsOut.make(
                objects=table.data_ptr(), max_objects=MAX_OBJECTS, n_objects=d_nobj, object_of=object_of.data_ptr()))

        def call_boxes():
            i = k[0]
            k[0] += 1
            ctx.object_boxes_device(ring[i % R].data_ptr(), n, object_of.data_ptr(), d_nobj, MAX_OBJECTS, boxes.data_ptr())

        call_objects()
        ctx.synchronize()
        n_objects = int(words[4].item())
        _, med_box = timed(call_boxes, len(OBJECT_BOXES_LAUNCHES))
        _, med_obj = timed(call_objects, CLUSTER_OBJECT_LAUNCHES)
        say(f"[yardsticks, tolerance {tol} mm, {n_objects} objects, the same {n} records] the object table's accumulate launch "
            f"{med_obj[CLUSTER_OBJECT_STAGES.index('accumulate')]:.1f} us, the boxes' moments launch {med_box[OBJECT_BOXES_LAUNCHES.index('moments')]:.1f} us")
    ctx.close()
    out_file.close()


if __name__ == "__main__":
    main()
