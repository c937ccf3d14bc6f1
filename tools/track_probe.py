#!/usr/bin/env python3
"""GPU box: what does one object-tracker update (pcs_tracker_update_device) cost on the stitched payload of 8 x 1280x720, launch by
launch, and how does its record pass stand against the background model's `flag` launch on the same cloud?

The payload is the synthetic frames' with invalid depth dropped (PCS_FLAG_DROP_INVALID). object_of is made on the host: the records'
500 mm blocks, numbered by first record as pcs_cluster_objects_device numbers its objects, so a few hundred spatially coherent objects
whose members are mostly neighbours in record order, as a cluster's are. Two sizes: the WORKING size (every record takes part) and a
FOREGROUND-ONLY size (the records of every tenth object, compacted: what is left behind -X). Two frame-sets alternate, the second
moved by 20 mm, so that every update votes against a full previous map. Method of DESIGN.md section 7 and tools/background_probe.py:
device-resident payloads in a ring of more than twice the 256 MiB Infinity Cache, so every call reads its payload cold from HBM.

Printed per size: records, objects, the cells of the map, the time of each of the update's four launches (pcs_kernel_timing, median
and minimum) and the whole call (one event pair per call, kernel timing off); beside them the YARDSTICK from the same run: the `flag`
launch of pcs_background_subtract_device with dilate 0 over the same cloud against a model learned from it (both do one probe
sequence per record), and the learn launch (one find-or-claim per record, as the record pass's second half).

There is no pass / fail bar on these figures.

    python tools/track_probe.py [calls = 30] [warm-ups = 5]
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
from pointcloud_stitching_amd.types import BACKGROUND_SUBTRACT_LAUNCHES, BackgroundParams, FLAG_DROP_INVALID, TRACK_UPDATE_LAUNCHES, TrackParams

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 5
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
CELL_MM, MAX_CELLS, MAX_OBJECTS, BLOCK_MM, MOVE_MM = 100, 4194304, 65536, 500, 20


def objects_of(scene):
    """object_of and the object count: the 500 mm block of every record, numbered by first record."""
    b = scene[:, :3].astype(np.int64) // BLOCK_MM + 100
    key = b[:, 0] | b[:, 1] << 10 | b[:, 2] << 20
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(uniq.shape[0], np.int64)
    rank[np.argsort(first)] = np.arange(uniq.shape[0])
    return rank[inv].astype(np.int32), int(uniq.shape[0])


def timed(ctx, stream, call, launches):
    """(whole-call microseconds with timing off, per-launch microseconds [CALLS, launches])"""
    for _ in range(WARM):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    stream.synchronize()
    whole = [a.elapsed_time(b) * 1e3 for a, b in ev]
    ctx.synchronize()
    ctx.kernel_timing(True)
    ctx.kernel_times_ms()
    for _ in range(CALLS):
        call()
    per = ctx.kernel_times_ms().reshape(CALLS, launches) * 1e3
    ctx.kernel_timing(False)
    return whole, per


def probe(ctx, stream, dev, name, scene):
    n = scene.shape[0]
    obj, m = objects_of(scene)
    moved = scene.copy()
    moved[:, 0] += MOVE_MM
    raw = 10 * n
    R = 2 * (-(-INFINITY_CACHE_BYTES // raw) + 1)                     # even: the two frame-sets alternate through the ring
    ring = [torch.from_numpy((scene if i % 2 == 0 else moved).reshape(-1)).to(dev) for i in range(R)]
    d_obj = torch.from_numpy(obj).to(dev)
    d_m = torch.tensor([m], dtype=torch.int32, device=dev)
    tracks = torch.zeros(3 * MAX_OBJECTS, dtype=torch.int64, device=dev)
    stats = torch.zeros(8, dtype=torch.int64, device=dev)
    P = TrackParams.make(1)
    k = [0]
    with ctx.tracker_create(CELL_MM, MAX_CELLS, MAX_OBJECTS) as tr:
        def update():
            tr.update_device(ring[k[0] % R].data_ptr(), n, d_obj.data_ptr(), d_m.data_ptr(), MAX_OBJECTS, P, tracks.data_ptr(), stats.data_ptr())
            k[0] += 1

        update(); update()
        ctx.synchronize()
        first = (tracks[:3 * m].clone(), stats.clone())
        tr.reset(1)
        k[0] = 0
        update(); update()
        ctx.synchronize()
        assert torch.equal(first[0], tracks[:3 * m]) and torch.equal(first[1], stats), "two runs differ"
        st = stats.cpu().tolist()
        whole, per = timed(ctx, stream, update, len(TRACK_UPDATE_LAUNCHES))
        info = tr.info()
    print(f"[{name}] {n} records ({raw / 1e6:.1f} MB), {m} objects, cell_mm {CELL_MM}, max_cells {MAX_CELLS} (tables {36 * 2 * MAX_CELLS / 1e6:.0f} MB); "
          f"second update: voted {st[1]} of {st[0]}, continued {st[3]}, born {st[4]}, overflow {info['overflow']}", flush=True)
    print(f"    update, whole call: median {statistics.median(whole):8.1f} us  min {min(whole):8.1f} us", flush=True)
    print("    per launch (median / min us): " + ", ".join(f"{nm} {np.median(per[:, i]):.1f} / {per[:, i].min():.1f}"
                                                           for i, nm in enumerate(TRACK_UPDATE_LAUNCHES)), flush=True)
    # the yardstick, same run, same cloud: background learn and the flag launch of subtract with dilate 0
    out = torch.empty(n * 5 + 8, dtype=torch.int16, device=dev)
    kept = torch.zeros(1, dtype=torch.int32, device=dev)
    with ctx.background_create(CELL_MM, MAX_CELLS) as bg:
        bg.learn_device(ring[0].data_ptr(), n)
        B = BackgroundParams.make(1, 0)

        def subtract():
            bg.subtract_device(ring[k[0] % R].data_ptr(), n, B, out.data_ptr(), n * 5, kept.data_ptr(), stats.data_ptr())
            k[0] += 1
        _, per_bg = timed(ctx, stream, subtract, len(BACKGROUND_SUBTRACT_LAUNCHES))
        cells = bg.info()["cells"]
        with ctx.background_create(CELL_MM, MAX_CELLS) as fresh:
            def learn():
                fresh.learn_device(ring[k[0] % R].data_ptr(), n)
                k[0] += 1
            for _ in range(min(WARM, 3)):
                learn()
            ctx.synchronize()
            ctx.kernel_timing(True)
            ctx.kernel_times_ms()
            for _ in range(CALLS):
                learn()
            per_learn = ctx.kernel_times_ms() * 1e3
            ctx.kernel_timing(False)
    flag = per_bg[:, 0]
    rec = per[:, 0]
    print(f"    yardstick: background flag (dilate 0, {cells} cells) median {np.median(flag):.1f} / min {flag.min():.1f} us; learn median "
          f"{np.median(per_learn):.1f} / min {per_learn.min():.1f} us | record pass / flag = {np.median(rec) / np.median(flag):.2f}, "
          f"record pass / (flag + learn) = {np.median(rec) / (np.median(flag) + np.median(per_learn)):.2f}", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("track_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    print(f"{CALLS} calls after {WARM} warm-ups per line", flush=True)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n_max = S * W * H
    ctx = PcsContext(cfgs, flags=FLAG_DROP_INVALID)
    ctx.set_stream(stream.cuda_stream)
    depth = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).astype(np.int16)).to(dev) for s in range(S)]
    color = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    pay = torch.empty(n_max * 5, dtype=torch.int16, device=dev)
    ctx.process_frames_device([t.data_ptr() for t in depth], [t.data_ptr() for t in color], pay.data_ptr(), n_max * 5, counts.data_ptr())
    ctx.synchronize()
    n = int(counts[S].item())
    scene = pay[:n * 5].cpu().numpy().reshape(-1, 5)
    del pay, depth, color
    probe(ctx, stream, dev, "working size", scene)
    obj, _ = objects_of(scene)
    probe(ctx, stream, dev, "foreground only", np.ascontiguousarray(scene[obj % 10 == 0]))
    ctx.close()


if __name__ == "__main__":
    main()
