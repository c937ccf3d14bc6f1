#!/usr/bin/env python3
"""GPU box: what does the object table (pcs_cluster_objects_device) cost on the stitched payload of 8 x 1280x720, beside the cluster
filter it rides on and beside today's only other route to the same table? The cloud, the ring and the method are
tools/cluster_probe.py's: the synthetic frames' payload with invalid depth dropped plus a stated share of scattered records, a ring
of device-resident payloads of more than twice the 256 MiB Infinity Cache, so every call reads its payload cold from HBM.
For tolerance_mm in {10, 20, 40}, min_size MIN_SIZE, max_objects MAX_OBJECTS:

  the objects, the written entries, the largest object; the table against a numpy grouping of the labels form's output (exact);
  the whole objects call with the filtered output (and statistics block) and without, one event pair per call, median and minimum;
  each launch of both through pcs_kernel_timing, median of the timed calls; the new launches' sum;
  accumulate against the same call's record roots launch — both one pass over the records with grouped atomics;
  the yardsticks, same session, same cloud: pcs_cluster_filter_device (the objects call with `out` does that work plus the new
  launches: the difference is the price of the table), and pcs_cluster_labels_device + a device-to-host copy of labels and sizes +
  the numpy grouping (wall clock of the host part, once).

There is no pass / fail bar on these figures. Everything printed is also written to the output file.

    python tools/objects_probe.py [output = profiles/objects_probe.txt] [calls = 10] [warm-ups = 2] [scatter share in percent = 2]
"""
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
from pointcloud_stitching_amd.types import (CLUSTER_LABEL_LAUNCHES, CLUSTER_LAUNCHES, CLUSTER_OBJECT_DTYPE, CLUSTER_OBJECT_LAUNCHES,
                                            CLUSTER_OBJECT_OUT_LAUNCHES, CLUSTER_OBJECT_OUT_STAGES, CLUSTER_OBJECT_STAGES, CLUSTER_STAGES,
                                            CLUSTER_STATS_FIELDS, FLAG_DROP_INVALID, ClusterObjectsOut, ClusterParams)

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "objects_probe.txt")
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 2
SCATTER_PERCENT = float(sys.argv[4]) if len(sys.argv) > 4 else 2.0
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
TOLERANCES = (10, 20, 40)
MIN_SIZE = 100
MAX_OBJECTS = 1024
OUT_STAGES = CLUSTER_OBJECT_OUT_STAGES[:13] + ("stats",) + CLUSTER_OBJECT_OUT_STAGES[13:]      # with a statistics block
assert len(CLUSTER_OBJECT_STAGES) == CLUSTER_OBJECT_LAUNCHES and len(OUT_STAGES) == CLUSTER_OBJECT_OUT_LAUNCHES + 1


def group(cloud, labels, sizes):
    """The table from per-record labels and sizes, in numpy: today's route on the host."""
    keep = sizes >= MIN_SIZE
    lab = labels[keep]
    firsts, inverse = np.unique(lab, return_inverse=True)
    rec = cloud[keep]
    xyz = rec[:, :3].astype(np.int64)
    s3, s4 = rec[:, 3].astype(np.int64) & 0xFFFF, rec[:, 4].astype(np.int64) & 0xFFFF
    rgb = np.stack([s3 & 0xFF, s3 >> 8, s4 & 0xFF], axis=1)
    table = np.zeros(firsts.shape[0], CLUSTER_OBJECT_DTYPE)
    table["label"] = firsts
    table["size"] = np.bincount(inverse, minlength=firsts.shape[0])
    if firsts.shape[0]:          # exact int64 per object: the members side by side, one reduceat per column group
        order = np.argsort(inverse, kind="stable")
        starts = np.searchsorted(inverse[order], np.arange(firsts.shape[0]))
        table["lo"] = np.minimum.reduceat(xyz[order], starts, axis=0)
        table["hi"] = np.maximum.reduceat(xyz[order], starts, axis=0)
        table["sum_xyz"] = np.add.reduceat(xyz[order], starts, axis=0)
        table["sum_rgb"] = np.add.reduceat(rgb[order], starts, axis=0)
    return table


def main():
    if not torch.cuda.is_available():
        raise SystemExit("objects_probe needs the GPU: there is nothing to time without one")
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
    words = torch.zeros(16, dtype=torch.int32, device=dev)          # [0] the kept count, [4] n_objects, [8] the labels form's count
    block = torch.zeros(8, dtype=torch.int64, device=dev)
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    object_of = torch.zeros(n, dtype=torch.int32, device=dev)
    table = torch.zeros(MAX_OBJECTS * 80, dtype=torch.uint8, device=dev)
    d_kept, d_nobj, d_ncl = words.data_ptr(), words.data_ptr() + 16, words.data_ptr() + 32
    say("# python tools/objects_probe.py")
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

        def call_objects_out():
            i = k[0]
            k[0] += 1
            ctx.cluster_objects_device(ring[i % R].data_ptr(), n, params, ClusterObjectsOut.make(
                objects=table.data_ptr(), max_objects=MAX_OBJECTS, n_objects=d_nobj, object_of=object_of.data_ptr(), out=outs[i % 3].data_ptr(),
                out_shorts=n * 5, out_points=d_kept, stats=block.data_ptr()))

        def call_objects():
            i = k[0]
            k[0] += 1
            ctx.cluster_objects_device(ring[i % R].data_ptr(), n, params, ClusterObjectsOut.make(
                objects=table.data_ptr(), max_objects=MAX_OBJECTS, n_objects=d_nobj, object_of=object_of.data_ptr()))

        def call_filter():
            i = k[0]
            k[0] += 1
            ctx.cluster_filter_device(ring[i % R].data_ptr(), n, params, outs[i % 3].data_ptr(), n * 5, d_kept, block.data_ptr())

        def call_labels():
            i = k[0]
            k[0] += 1
            ctx.cluster_labels_device(ring[i % R].data_ptr(), n, tol, labels.data_ptr(), sizes.data_ptr(), d_ncl)

        # the table twice, with and without the filtered output: the same bytes; then against the numpy grouping of the labels form
        call_objects_out()
        ctx.synchronize()
        n_objects, kept = int(words[4].item()), int(words[0].item())
        stats = dict(zip(CLUSTER_STATS_FIELDS, block.tolist()))
        written = min(n_objects, MAX_OBJECTS)
        first_table, first_of = table[:80 * written].clone(), object_of.clone()
        call_objects()
        ctx.synchronize()
        assert int(words[4].item()) == n_objects == stats["kept_clusters"] and stats["kept"] == kept
        assert torch.equal(first_table, table[:80 * written]) and torch.equal(first_of, object_of), "two runs differ"
        call_labels()
        ctx.synchronize()
        t0 = time.perf_counter()
        h_labels, h_sizes = labels.cpu().numpy(), sizes.cpu().numpy()
        t1 = time.perf_counter()
        want = group(cloud, h_labels, h_sizes)
        t2 = time.perf_counter()
        got = first_table.cpu().numpy().view(CLUSTER_OBJECT_DTYPE)
        assert want.shape[0] == n_objects and got.tobytes() == want[:written].tobytes(), "the table differs from the numpy grouping"
        assert int((first_of >= 0).sum().item()) == kept

        us_out, med_out = timed(call_objects_out, len(OUT_STAGES))
        us_obj, med_obj = timed(call_objects, CLUSTER_OBJECT_LAUNCHES)
        us_fil, med_fil = timed(call_filter, CLUSTER_LAUNCHES)
        us_lab, _ = timed(call_labels, CLUSTER_LABEL_LAUNCHES)
        m_out, m_obj, m_fil, m_lab = (statistics.median(u) for u in (us_out, us_obj, us_fil, us_lab))
        new = med_out[len(CLUSTER_STAGES):]
        say(f"[tolerance {tol:3d} mm] {n_objects} objects ({written} written), largest {int(got['size'].max(initial=0))}, kept {kept} of {n} records "
            f"({stats['clusters']} clusters)")
        say(f"    objects call with out and stats: median {m_out:8.1f} us  min {min(us_out):8.1f} us | without out: median {m_obj:8.1f} us  "
            f"min {min(us_obj):8.1f} us")
        say("    per launch, with out (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(OUT_STAGES, med_out)) + f" | sum {med_out.sum():.1f}")
        say("    per launch, without out (median us): " + ", ".join(f"{name} {v:.1f}" for name, v in zip(CLUSTER_OBJECT_STAGES, med_obj))
            + f" | sum {med_obj.sum():.1f}")
        say(f"    the six new launches: {new.sum():.1f} us | accumulate {new[4]:.1f} us / record roots {new[0]:.1f} us = {new[4] / new[0]:.2f}")
        say(f"    yardstick, pcs_cluster_filter_device: median {m_fil:8.1f} us  min {min(us_fil):8.1f} us (launch sum {med_fil.sum():.1f}) | "
            f"objects with out / filter = {m_out / m_fil:.3f}, the table costs {m_out - m_fil:.1f} us")
        say(f"    yardstick, today's route: pcs_cluster_labels_device median {m_lab:8.1f} us + copy of labels and sizes to the host "
            f"{(t1 - t0) * 1e6:.0f} us + numpy grouping {(t2 - t1) * 1e6:.0f} us = {m_lab + (t2 - t0) * 1e6:.0f} us | "
            f"/ objects call without out = {(m_lab + (t2 - t0) * 1e6) / m_obj:.1f}")
    ctx.close()
    out_file.close()


if __name__ == "__main__":
    main()
