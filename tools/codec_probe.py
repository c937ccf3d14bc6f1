#!/usr/bin/env python3
"""GPU box: what does the PCZ1 payload codec (pcs_compress_payload_device / pcs_decompress_payload_device) cost on the stitched payload
of 8 x 1280x720, what does it save in bytes, and does the host-pointer call get faster when only the container crosses the link?

Method of DESIGN.md section 7 and of tools/decimate_probe.py: device-resident payloads (and containers) in rings of more than twice
the 256 MiB Infinity Cache, one call counter through warm-up and the timed calls, so every call reads cold data from HBM. Every call
is bracketed by its own hipEvent pair: median and minimum of 200 calls after 20 warm-ups. Legs:

  encode (three launches) and decode (one), dense and with PCS_FLAG_DROP_INVALID (-i), with the byte floor: 20 B per record read
      (the encoder reads the payload twice) plus the container written / the container read plus 10 B per record written;
  container bytes over raw bytes, for the synthetic scene (colour is noise) and for a smooth-colour variant of it;
  pcs_process_frames_compressed against pcs_process_frames on the same context, page-locked host buffers, alternating in one process
      (wall clock per call: these are synchronous host calls).

There is no pass / fail bar on these figures.

    python tools/codec_probe.py [calls = 200] [warm-ups = 20]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloud_stitching_amd import api, synthetic as Syn
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import FLAG_DROP_INVALID

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 20
S, W, H = 8, 1280, 720
INFINITY_CACHE_BYTES = 256 << 20
PEAK_GBS = 8000.0
N_SEEDS = 3                     # distinct frame-sets (their copies in a ring differ in address, which is what the caches see)


def smooth_color(w, h, s):
    """A colour raster whose neighbouring pixels are close: two gradients and a slow wave (the synthetic generator's is noise)."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3), np.uint8)
    img[..., 0] = (x * 255 // (w - 1) + 7 * s) & 255
    img[..., 1] = (y * 255 // (h - 1)) & 255
    img[..., 2] = (128 + 100 * np.sin((x + 2 * y) / 97.0 + s)).astype(np.uint8)
    return img.reshape(-1)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("codec_probe needs the GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    cfgs = [Syn.synth_stream_config(W, H, s) for s in range(S)]
    n_max = S * W * H
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    k = [0]

    def timed(name, call, mb=0.0):
        def one():
            i = k[0]
            k[0] += 1
            call(i)
        for _ in range(WARM):
            one()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
        for a, b in ev:
            a.record(stream)
            one()
            b.record(stream)
        stream.synchronize()
        us = [a.elapsed_time(b) * 1e3 for a, b in ev]
        med, lo = statistics.median(us), min(us)
        line = f"{name:46s} per call: median {med:8.2f} us  min {lo:8.2f} us"
        if mb:
            line += f" | floor {mb:6.1f} MB: {mb / med * 1e3 / PEAK_GBS * 100:5.1f} % (median) of 8 TB/s, {mb / PEAK_GBS * 1e3:5.1f} us at peak"
        print(line, flush=True)
        return med, lo

    depth = [[Syn.synth_depth(W, H, s, seed=Syn.SEED + f) for s in range(S)] for f in range(N_SEEDS)]
    colors = {"synthetic scene": [Syn.synth_color(W, H, s) for s in range(S)], "smooth colour": [smooth_color(W, H, s) for s in range(S)]}
    d_depth = [[torch.from_numpy(d.reshape(-1).view(np.int16).copy()).to(dev) for d in fs] for fs in depth]
    bound = api.compressed_bound(n_max)
    print(f"{S} x {W}x{H}: {n_max} records, {n_max * 10 / 1e6:.1f} MB raw, {CALLS} calls after {WARM} warm-ups", flush=True)

    for flags, tag in ((0, "dense"), (FLAG_DROP_INVALID, "-i")):
        ctx = PcsContext(cfgs, flags=flags)
        ctx.set_stream(stream.cuda_stream)
        counts = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        size_word = torch.zeros(1, dtype=torch.int32, device=dev)
        for cname, col in colors.items():
            d_col = [torch.from_numpy(c).to(dev) for c in col]
            pays, ns = [], []
            for f in range(N_SEEDS):
                p = torch.empty(n_max * 5 + 8, dtype=torch.int16, device=dev)
                ctx.process_frames_device([t.data_ptr() for t in d_depth[f]], [t.data_ptr() for t in d_col], p.data_ptr(), n_max * 5, counts.data_ptr())
                ctx.synchronize()
                pays.append(p)
                ns.append(int(counts[S].item()))
            # ratios: one container per distinct frame-set
            cont = torch.empty(bound + 64, dtype=torch.uint8, device=dev)
            sizes = []
            for f in range(N_SEEDS):
                ctx.compress_payload_device(pays[f].data_ptr(), ns[f], cont.data_ptr(), bound, size_word.data_ptr())
                ctx.synchronize()
                sizes.append(int(size_word.item()))
            raw = [10 * n for n in ns]
            print(f"[{tag}, {cname}] records {ns}, container bytes {sizes}: container / raw = "
                  + ", ".join(f"{c / r:.4f}" for c, r in zip(sizes, raw)) + f" (mean {sum(sizes) / sum(raw):.4f})", flush=True)
            if cname != "synthetic scene":
                continue
            # timing: rings of payloads and of containers, cold
            R = -(-2 * INFINITY_CACHE_BYTES // raw[0]) + 2
            ring = [pays[r % N_SEEDS].clone() for r in range(R)]
            RC = -(-2 * INFINITY_CACHE_BYTES // sizes[0]) + 2
            outs = [torch.empty(bound + 64, dtype=torch.uint8, device=dev) for _ in range(3)]
            conts = []
            for r in range(RC):
                c = torch.empty(sizes[r % N_SEEDS] + 64, dtype=torch.uint8, device=dev)
                ctx.compress_payload_device(pays[r % N_SEEDS].data_ptr(), ns[r % N_SEEDS], outs[0].data_ptr(), bound, 0)
                ctx.synchronize()
                c[:sizes[r % N_SEEDS]] = outs[0][:sizes[r % N_SEEDS]]
                conts.append(c)
            back = [torch.empty(n_max * 5 + 8, dtype=torch.int16, device=dev) for _ in range(3)]
            print(f"[{tag}] rings: {R} payloads ({R * raw[0] / 1e6:.0f} MB), {RC} containers ({RC * sizes[0] / 1e6:.0f} MB)", flush=True)

            def encode(i):
                ctx.compress_payload_device(ring[i % R].data_ptr(), ns[i % R % N_SEEDS], outs[i % 3].data_ptr(), bound, 0)

            def decode(i):
                f = i % RC % N_SEEDS
                ctx.decompress_payload_device(conts[i % RC].data_ptr(), sizes[f], ns[f], back[i % 3].data_ptr(), n_max * 5)

            timed(f"[{tag}] encode (count + offsets + emit)", encode, (2 * raw[0] + sizes[0]) / 1e6)
            timed(f"[{tag}] decode", decode, (raw[0] + sizes[0]) / 1e6)
            f0 = 0
            decode(0)
            ctx.synchronize()
            assert torch.equal(back[0][:ns[f0] * 5], pays[f0][:ns[f0] * 5]), "round trip"
            del ring, conts, outs, back

        # the host-pointer calls, page-locked buffers, alternating
        hd = [ctx.host_array(W * H, np.uint16) for _ in range(S)]
        hc = [ctx.host_array(cfgs[s].color_bytes, np.uint8) for s in range(S)]
        for s in range(S):
            hd[s][:] = depth[0][s].reshape(-1)
            hc[s][:] = colors["synthetic scene"][s][:hc[s].size]
        out = ctx.host_array(2 + n_max * 5, np.int16)
        zout = ctx.host_array(4 + bound, np.uint8)

        def wall(name, call):
            for _ in range(WARM):
                call()
            ms = []
            for _ in range(CALLS):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            print(f"{name:46s} per call: median {statistics.median(ms):7.3f} ms  min {min(ms):7.3f} ms", flush=True)
            return statistics.median(ms)

        res = {"z": [], "raw": []}
        for rnd in range(2):
            res["z"].append(wall(f"[{tag}] pcs_process_frames_compressed #{rnd}", lambda: ctx.process_frames_compressed(hd, hc, out=zout)))
            res["raw"].append(wall(f"[{tag}] pcs_process_frames #{rnd}", lambda: ctx.process_frames(hd, hc, out=out)))
        print(f"[{tag}] host-pointer call: compressed {min(res['z']):.3f} ms against {min(res['raw']):.3f} ms (median per call, best of 2)", flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
