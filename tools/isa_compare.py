#!/usr/bin/env python3
"""Compare two gfx950 assembly listings kernel by kernel.

    hipcc <the Makefile's flags> -S --cuda-device-only pcs_kernels.hip -o a.s      (once per tree)
    python tools/isa_compare.py parent.s new.s

For every kernel of the first listing: its instruction stream and its .amdhsa_ block (VGPR / SGPR / LDS / scratch figures) in the
second, byte for byte. Kernels only the second has are listed with their figures. Exit status 1 if any kernel of the first moved.
"""
import re
import sys


def kernels(path):
    """{kernel: instruction lines}, {kernel: .amdhsa_ lines}. Local labels carry the function's ordinal in the file (.LBB12_3), which
    moves when a kernel is added in front: the ordinal and the comments are dropped."""
    body, meta, cur, blk = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, blk = m.group(1), None
            body[cur] = []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".amdhsa_kernel"):
            blk = meta[cur] = []
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif blk is not None:
            blk.append(t)
        elif not t.startswith((".section", ".p2align")):
            t = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).split()      # (comments name loop headers by that ordinal too)
            if t:
                body[cur].append(" ".join(t))
    return {k: v for k, v in body.items() if k in meta}, meta


def figures(blk):
    want = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")
    return {w: l.split()[-1] for l in blk for w in want if l.startswith(".amdhsa_" + w)}


def main():
    (b0, m0), (b1, m1) = kernels(sys.argv[1]), kernels(sys.argv[2])
    moved = 0
    for k in sorted(m0):
        same = k in m1 and b0.get(k) == b1.get(k) and m0[k] == m1[k]
        moved += not same
        if not same:
            print("MOVED  ", k)
    print(f"{len(m0)} kernels in {sys.argv[1]}: {len(m0) - moved} identical (instructions and .amdhsa block), {moved} moved")
    for k in sorted(set(m1) - set(m0)):
        print("NEW    ", k, figures(m1[k]))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
