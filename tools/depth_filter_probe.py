#!/usr/bin/env python3
"""GPU box: what does the depth pre-filter (pcs_filter_depth_device) cost on 8 x 1280x720, and does it earn the counted stitch's saving?

Method of DESIGN.md section 7: device-resident synthetic frame-sets in a ring whose depth rasters alone are more than twice the
256 MiB Infinity Cache, one launch counter through warm-up and the timed calls, so every call reads cold inputs from HBM. The
temporal state is part of the traffic (6 of the 10 B/pixel), and one context's 22 MB of it would simply stay in the Infinity Cache
from call to call: the stateful legs therefore rotate through a ring of contexts (one state each, 2 x the cache in all). One extra
leg keeps to one context and says so — that is a frame loop with nothing between two filter calls.

Every call is bracketed by its own hipEvent pair (200 calls after 20 warm-ups: median and minimum), and the same calls are timed
once more back to back inside one pcs_timer_* window (per call = window / calls; launch gaps hide behind the previous call).
Legs: both stages; temporal alone; holes alone; both stages + tile counts. Then, on a PCS_FLAG_DROP_INVALID context, the pair
filter + pcs_process_frames_device_counted (counts from the filter) against filter + pcs_process_frames_device (its own count pass).
Bytes: 10 B/pixel with the temporal stage (2 in + 2 out + 4 state value + 2 history), 4 B/pixel for holes alone; % of 8 TB/s.

    python tools/depth_filter_probe.py [calls = 200] [warm-ups = 20] [all | filter (the filter's own legs only)]
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
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 20
FILTER_ONLY = len(sys.argv) > 3 and sys.argv[3] == "filter"
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
PEAK_GBS = 8000.0
N_SEEDS = 4                     # distinct frames in the ring (their copies differ in address, which is what the caches see)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("depth_filter_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n = W * H
    set_bytes = S * n * 2
    R = -(-2 * INFINITY_CACHE_BYTES // set_bytes) + 2
    NC = -(-2 * INFINITY_CACHE_BYTES // (S * n * 3)) + 1
    seeds = [[torch.from_numpy(Syn.synth_depth(W, H, s, seed=Syn.SEED + k).reshape(-1).view(np.int16).copy()).to(dev) for s in range(S)]
             for k in range(N_SEEDS)]
    ring = [[seeds[k % N_SEEDS][s].clone() for s in range(S)] for k in range(R)]
    outs = [[torch.empty(n, dtype=torch.int16, device=dev) for _ in range(S)] for _ in range(4)]
    in_ptrs = [[t.data_ptr() for t in fs] for fs in ring]
    out_ptrs = [[t.data_ptr() for t in fs] for fs in outs]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    print(f"{S} x {W}x{H}: ring of {R} frame-sets of depth ({R * set_bytes / 1e6:.0f} MB, {(R - 1) * set_bytes / 1e6:.0f} MB between re-reads), "
          f"{NC} contexts per stateful leg ({NC * S * n * 3 / 1e6:.0f} MB of state), {CALLS} calls after {WARM} warm-ups", flush=True)

    def make(n_ctx, flags=0):
        ctxs = []
        for _ in range(n_ctx):
            c = PcsContext(cfgs, flags=flags)
            c.set_stream(stream.cuda_stream)
            ctxs.append(c)
        return ctxs

    k = [0]

    def timed(name, ctxs, bytes_per_pixel, call):
        """`call(ctx, d_in, d_out)` CALLS times after WARM warm-ups: per-call event pairs, then one back-to-back window."""
        def one():
            i = k[0]
            k[0] += 1
            call(ctxs[i % len(ctxs)], in_ptrs[i % R], out_ptrs[i % 4])
        for _ in range(max(WARM, len(ctxs))):
            one()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in ev:
            a.record(stream)
            one()
            b.record(stream)
        stream.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        ctxs[0].timer_begin()
        for _ in range(CALLS):
            one()
        ctxs[0].timer_end()
        window = ctxs[0].timer_elapsed_ms() / CALLS * 1e3
        med, lo = statistics.median(us), min(us)
        line = f"{name:44s} per call: median {med:7.2f} us  min {lo:7.2f} us | back to back {window:7.2f} us"
        if bytes_per_pixel:
            mb = S * n * bytes_per_pixel / 1e6
            line += f" | {mb:5.1f} MB: {mb / med * 1e3 / PEAK_GBS * 100:5.1f} % (median) {mb / window * 1e3 / PEAK_GBS * 100:5.1f} % (back to back) of 8 TB/s"
        print(line, flush=True)
        return med, lo, window

    def filt(counts):
        return lambda c, i, o: c.filter_depth_device(i, o, counts)

    n_tiles = S * ((n + 2047) // 2048)
    d_kept = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
    legs = [("both stages", NC, dict(temporal=True, hole_fill=1), 10, 0),
            ("temporal alone", NC, dict(temporal=True, hole_fill=0), 10, 0),
            ("holes alone", 1, dict(temporal=False, hole_fill=1), 4, 0),
            ("both stages + tile counts", NC, dict(temporal=True, hole_fill=1), 10, d_kept.data_ptr()),
            ("both stages, ONE context (state stays cached)", 1, dict(temporal=True, hole_fill=1), 10, 0)]
    pool = make(NC)
    for name, n_ctx, kw, bpp, counts in legs:
        for c in pool:
            c.set_depth_filter(None)                 # (one leg's state at a time)
        for c in pool[:n_ctx]:
            c.set_depth_filter(**kw)
        timed(name, pool[:n_ctx], bpp, filt(counts))
    for c in pool:
        c.close()

    if FILTER_ONLY:
        return
    # the filter as the producer of the counted stitch
    col = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    cb = cfgs[0].color_bytes
    RC = -(-2 * INFINITY_CACHE_BYTES // (S * cb)) + 2
    col_ring = [[c.clone() for c in col] for _ in range(RC)]
    col_ptrs = [[t.data_ptr() for t in fs] for fs in col_ring]
    pay = [torch.empty(S * n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(4)]
    ctx = make(1, flags=FLAG_DROP_INVALID)[0]
    ctx.set_depth_filter(temporal=True, hole_fill=0)       # (no fill: holes stay, so the stitch has something to drop)
    kc = [0]

    def chain(counted):
        def call(c, i, o):
            j = kc[0]
            kc[0] += 1
            if counted:
                c.filter_depth_device(i, o, d_kept.data_ptr())
                c.process_frames_device_counted(o, col_ptrs[j % RC], d_kept.data_ptr(), pay[j % 4].data_ptr(), S * n * 5)
            else:
                c.filter_depth_device(i, o)
                c.process_frames_device(o, col_ptrs[j % RC], pay[j % 4].data_ptr(), S * n * 5)
        return call

    res = {}
    for rnd in range(2):                   # alternate the two, twice: whatever else the box does falls on both
        for name, counted in (("filter + process_frames_device (own count pass)", False), ("filter(counts) + process_frames_device_counted", True)):
            res.setdefault(name, []).append(timed(f"{name} #{rnd}", [ctx], 0, chain(counted)))
    a, b = res["filter + process_frames_device (own count pass)"], res["filter(counts) + process_frames_device_counted"]
    for what, idx in (("median per call", 0), ("back to back", 2)):
        x, y = min(r[idx] for r in a), min(r[idx] for r in b)
        print(f"counted path saves ({what}, best of 2): {x - y:+.2f} us  ({x:.2f} -> {y:.2f})", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
