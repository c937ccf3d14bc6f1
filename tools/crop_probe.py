#!/usr/bin/env python3
"""GPU box: what does a world-frame crop box (pcs_set_crop_box_mm) cost, and what does it save, beside the chains that exist?

pcs_process_frames_device on 8 x 1280x720 device-resident synthetic frame-sets, timed with the library's own timer (pcs_timer_*:
a hipEvent pair on the context's stream around K back-to-back calls). The frame-sets live in a ring whose input rasters alone
are more than twice the 256 MiB Infinity Cache, as bench.py sizes its own, so every call reads cold inputs from HBM. Four
contexts over the same ring and output buffers take turns, `rounds` windows each, so that whatever else the box is doing falls on
all of them alike:
    no flag               the dense launch (every record written)
    DROP_INVALID          count (Z16 words alone) + scan + emit
    box                   boxed count (deprojects) + scan + boxed emit
    DROP_INVALID + box    the same with both predicates
The box keeps about 15 % of the records of this scene; the share each leg really keeps is read back from its device counts and
printed. Prints every window, then median, minimum, maximum and spread (max - min) per leg, and the distance from the
DROP_INVALID chain in units of that chain's own spread.

    python tools/crop_probe.py [calls per window = 2000] [rounds = 7]
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

K = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
BOX = ((-1170, 0, -1170), (1170, 2070, 335))         # 15 % of this scene's records (12.9 % at +-1100, 18.9 % at +-1300: the CPU oracle)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("crop_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n, cb = W * H, cfgs[0].color_bytes
    in_bytes = S * (n * 2 + cb)
    R = max(4, -(-2 * INFINITY_CACHE_BYTES // in_bytes) + 2)
    dep0 = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).view(np.uint8)).to(dev) for s in range(S)]
    col0 = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    sets = [(dep0, col0)] + [([d.clone() for d in dep0], [c.clone() for c in col0]) for _ in range(R - 1)]
    outs = [torch.empty(S * n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(4)]
    counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    legs = {"no flag": (0, False), "drop": (FLAG_DROP_INVALID, False), "box": (0, True), "drop + box": (FLAG_DROP_INVALID, True)}
    ctxs = {}
    for name, (flags, boxed) in legs.items():
        ctxs[name] = PcsContext(cfgs, flags=flags)
        ctxs[name].set_stream(stream.cuda_stream)
        if boxed:
            ctxs[name].set_crop_box_mm(*BOX)
    print(f"{S} x {W}x{H}, ring of {R} frame-sets ({R * in_bytes / 1e6:.0f} MB of inputs, {(R - 1) * in_bytes / 1e6:.0f} MB between "
          f"re-reads), {K} calls per window, {ROUNDS} rounds; box {BOX}; arithmetic policy {ctxs['box'].stream_math(0)}", flush=True)
    k = [0]
    ptrs = [([t.data_ptr() for t in d], [t.data_ptr() for t in c]) for d, c in sets]      # (the enqueue must stay well under a call)
    optr = [o.data_ptr() for o in outs]

    def launch(ctx, d_counts=0):
        d, c = ptrs[k[0] % R]
        o = optr[k[0] % 4]
        k[0] += 1
        ctx.process_frames_device(d, c, o, S * n * 5, d_counts)

    for name, ctx in ctxs.items():          # every shape the timed windows use, warm; and what each leg keeps
        for _ in range(100):
            launch(ctx)
        launch(ctx, counts.data_ptr())
        ctx.synchronize()
        kept = int(counts.cpu()[S])
        print(f"{name:10s} keeps {kept} of {S * n} records = {kept / (S * n):.4f}", flush=True)
    torch.cuda.synchronize()
    us = {name: [] for name in legs}
    for r in range(ROUNDS):
        for name, ctx in ctxs.items():
            ctx.timer_begin()
            for _ in range(K):
                launch(ctx)
            ctx.timer_end()
            t = ctx.timer_elapsed_ms() / K * 1e3
            us[name].append(t)
            print(f"round {r} {name:10s} {t:7.3f} us / call", flush=True)
    base = us["drop"]
    spread = max(base) - min(base)
    for name, v in us.items():
        med = statistics.median(v)
        line = f"{name:10s} median {med:7.3f} us  min {min(v):7.3f}  max {max(v):7.3f}  spread {max(v) - min(v):6.3f}"
        if name != "drop":
            d = med - statistics.median(base)
            line += f"  vs drop {d:+.3f} us = {d / spread if spread > 0 else float('inf'):+.1f} x the drop chain's spread"
        print(line, flush=True)
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
