#!/usr/bin/env python3
"""GPU box: what does the reference's default (no -m) arithmetic cost beside its -m arithmetic?

pcs_process_frames_device on 8 x 1280x720 device-resident synthetic frame-sets, timed with the library's own timer (pcs_timer_*:
a hipEvent pair on the context's stream around K back-to-back launches). The frame-sets live in a ring whose input rasters alone
are more than twice the 256 MiB Infinity Cache, as bench.py sizes its own, so every launch reads cold inputs from HBM. Four
contexts over the same ring and output buffers — no flag (-m; and -m without its row-constant tile), FLAG_SCALAR_ARITH, FLAG_SCALAR_ARITH |
FLAG_CUTOFF — take turns,
`rounds` windows each, so that whatever else the box is doing falls on all of them alike. Prints every window, then median, minimum,
maximum and spread (max - min) per leg, and the scalar legs' distance from -m in units of -m's own spread.

    python tools/scalar_probe.py [launches per window = 4000] [rounds = 7]

PCS_LIB_PATH selects a variant build of the library (pcs_kernels.hip: -DPCS_SCALAR_FP64=1 is the FP64 form of the conversion).
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
from pointcloud_stitching_amd.types import FLAG_CUTOFF, FLAG_SCALAR_ARITH

K = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20


def main():
    if not torch.cuda.is_available():
        raise SystemExit("scalar_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n, cb = W * H, cfgs[0].color_bytes
    in_bytes = S * (n * 2 + cb)
    R = max(4, -(-2 * INFINITY_CACHE_BYTES // in_bytes) + 2)
    dep0 = [torch.from_numpy(Syn.synth_depth(W, H, s).reshape(-1).view(np.uint8)).to(dev) for s in range(S)]
    col0 = [torch.from_numpy(Syn.synth_color(W, H, s)).to(dev) for s in range(S)]
    sets = [(dep0, col0)] + [([d.clone() for d in dep0], [c.clone() for c in col0]) for _ in range(R - 1)]
    outs = [torch.empty(S * n * 5 + 8, dtype=torch.int16, device=dev) for _ in range(4)]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    # "-m general": the -m arithmetic through the tile the scalar legs use (PCS_ROW_CONST=0 at create: no row-constant tile), so that
    # the arithmetic's cost can be told from the cost of not having the row-constant tile's colour window
    legs = {"-m": 0, "-m general": 0, "scalar": FLAG_SCALAR_ARITH, "scalar -c": FLAG_SCALAR_ARITH | FLAG_CUTOFF}
    ctxs = {}
    for name, flags in legs.items():
        if name == "-m general":
            os.environ["PCS_ROW_CONST"] = "0"
        ctxs[name] = PcsContext(cfgs, flags=flags)
        os.environ.pop("PCS_ROW_CONST", None)
        ctxs[name].set_stream(stream.cuda_stream)
    print(f"library {os.environ.get('PCS_LIB_PATH', 'in-tree')}; {S} x {W}x{H}, ring of {R} frame-sets ({R * in_bytes / 1e6:.0f} MB of "
          f"inputs, {(R - 1) * in_bytes / 1e6:.0f} MB between re-reads), {K} launches per window, {ROUNDS} rounds; "
          f"arithmetic policy {ctxs['-m'].stream_math(0)}, row-constant {ctxs['-m'].stream_color_row_const(0)}", flush=True)
    k = [0]
    ptrs = [([t.data_ptr() for t in d], [t.data_ptr() for t in c]) for d, c in sets]      # (the enqueue must stay well under a launch)
    optr = [o.data_ptr() for o in outs]

    def launch(ctx):
        d, c = ptrs[k[0] % R]
        o = optr[k[0] % 4]
        k[0] += 1
        ctx.process_frames_device(d, c, o, S * n * 5)

    for ctx in ctxs.values():               # every shape the timed windows use, warm
        for _ in range(200):
            launch(ctx)
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
            print(f"round {r} {name:10s} {t:7.3f} us / launch", flush=True)
    base = us["-m"]
    spread_m = max(base) - min(base)
    for name, v in us.items():
        med = statistics.median(v)
        line = (f"{name:10s} median {med:7.3f} us  min {min(v):7.3f}  max {max(v):7.3f}  spread {max(v) - min(v):6.3f}  "
                f"{S * n * 15 / (med * 1e-6) / 8e12:.4f} of 8 TB/s at 15 B/point")
        if name != "-m":
            d = med - statistics.median(base)
            line += f"  vs -m {d:+.3f} us = {d / spread_m if spread_m > 0 else float('inf'):+.1f} x the -m spread"
        print(line, flush=True)
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
