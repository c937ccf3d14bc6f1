#!/usr/bin/env python3
"""Regenerates tests/golden/ref_pin/: what the COMPILED REFERENCE (oracle/_ref/libpcs_ref.so, see oracle/ref_pin.py) writes for
the inputs of tests/ref_pin_cases.py. Needs the reference checkout; run from the repo root after __graft_entry__.build():

    python tests/golden/make_ref_pin_golden.py

manifest.json holds, per case: its parameters, the SHA-256 of its inputs, and per reading of the reference (`-m -t1` dense,
`-c -m -t1`, non-`-m` dense) the record count, the returned size, the SHA-256 of the records and, for the two `-m` readings, of
the whole buffer a1 leaves behind. <case>.bin holds the records themselves (little-endian int16, dense then cut then scalar) for
the small cases. Nothing here comes from oracle/pcs_oracle.c except the fused cases' deprojection, which the reference does not
contain (it is librealsense's); those cases pin the pack half of the fused path only.

build_fixtures() returns {file name: bytes} without touching the tree; tests/test_reference_pin.py calls it to check that the
committed files are what the reference produces today.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_pin_cases as RC                             # noqa: E402
from oracle import pcs_oracle as O                     # noqa: E402
from oracle import ref_pin as R                        # noqa: E402

PREFILL = 0x5A5A


def _reading(sc, V, T, col, mode, threads=1):
    """One reading of the reference on one input -> (records, size, whole buffer)."""
    buf, size = R.send(V, T, col, sc.color.width, sc.color.height, sc.color_bpp, sc.color_stride, list(sc.cam_to_world),
                       simd=(mode != "scalar"), cutoff=(mode == "cut"), threads=threads, prefill=PREFILL)
    assert size % 10 == 0
    rec = buf[2:2 + size // 2].reshape(-1, 5).copy()
    want = RC.expected_buffer(rec, PREFILL, R.buf_size(), buf.nbytes)
    assert np.array_equal(buf, want), "a1 wrote outside the cleared prefix and its records"
    return rec, size, buf


def build_fixtures():
    files = {}
    man = {"_about": "Outputs of the compiled reference (src/pcs-camera-optimized.cpp) on the inputs of tests/ref_pin_cases.py. "
                     "Written by tests/golden/make_ref_pin_golden.py; data only.",
           "reference_build": R.compiler(), "buf_size": R.buf_size(), "prefill": PREFILL,
           "undefined_behaviour_note": "short(float) of NaN, infinities and values outside int's range is formally undefined; the "
                                       "cases marked as_compiled hold what this compile does (cvttss2si: 0x80000000, low half kept).",
           "scalar_reading_note": "the non -m loop is plain C++ float arithmetic, so its bytes depend on the compiler's contraction "
                                  "choices: every 'scalar' reading is as compiled with reference_build (g++ fuses u*w + .5f, and "
                                  "m0*x and m2*z into the sums, keeping m1*y and the translation as rounded steps).",
           "cases": {}, "fused": {}, "misreadings": {}}
    small = {}
    for name, (w, h, bpp, pad, mat, kind, full) in RC.CASES.items():
        sc, V, T, col = RC.build_case(name)
        n = V.shape[0]
        entry = {"width": w, "height": h, "bpp": bpp, "stride": sc.color_stride, "matrix": mat, "kind": kind, "points": n,
                 "inputs_sha256": RC.inputs_sha256(sc, V, T, col), "buffer_bytes": R.buffer_bytes(n), "readings": {}}
        if kind == "special":
            b = R.compiler()
            entry["as_compiled"] = f"as compiled with {b['compiler']}, {b['flags']}"
        blobs = []
        recs = {}
        for mode in RC.MODES:
            rec, size, buf = _reading(sc, V, T, col, mode)
            recs[mode] = rec
            e = {"count": int(rec.shape[0]), "size": int(size), "sha256": RC.sha256(rec)}
            if mode != "scalar":
                e["buffer_sha256"] = RC.sha256(buf)
            if mode == "dense":
                # the dense `-m` output does not depend on the thread count
                rec4, size4, _ = _reading(sc, V, T, col, mode, threads=4)
                assert size4 == size and np.array_equal(rec4, rec), f"{name}: -t4 differs from -t1"
                e["t4_equals_t1"] = True
            entry["readings"][mode] = e
            blobs.append(rec.astype("<i2").tobytes())
        if kind == "kat":
            with open(os.path.join(HERE, "kat_appendix_b.json")) as f:
                k = json.load(f)
            B = np.array([[int(x, 16) for x in v["bytes"].split()] for v in k["vectors"]], np.uint8)
            assert np.array_equal(recs["dense"].view(np.uint8).reshape(-1, 10), B), "kat_appendix_b.json is not what the reference gives"
            entry["equals_kat_appendix_b_json"] = True
        if full:
            entry["records_file"] = name + ".bin"
            files[name + ".bin"] = b"".join(blobs)
            small[name] = (sc, V, T, col, recs["dense"], recs["cut"])
        man["cases"][name] = entry

    # the unmodified restatement reproduces the reference on the stored cases; every misreading must not
    assert RC.count_variant(None, small) == 0 and RC.count_variant("cut:none", small) == 0
    for variant in RC.DENSE_VARIANTS + RC.CUT_VARIANTS:
        changed = RC.count_variant(variant, small)
        assert changed > 0, f"the case set cannot tell '{variant}' from the reference: add inputs"
        man["misreadings"][variant] = {"records_changed": changed, "of": "cut" if variant in RC.CUT_VARIANTS else "dense"}

    for name, (ns, w, h, tweak, full) in RC.FUSED.items():
        cfgs, depth, color = RC.build_fused(name)
        vt = [O.deproject(sc, d) for sc, d in zip(cfgs, depth)]
        entry = {"streams": ns, "width": w, "height": h, "tweak": tweak,
                 "deprojected_sha256": RC.sha256(np.concatenate([np.concatenate([v.reshape(-1), t.reshape(-1)]) for v, t in vt])),
                 "readings": {}}
        blobs = []
        for mode in RC.FUSED_MODES:
            parts = [R.pack_config(sc, v, t, c, cutoff=(mode == "cut")) for sc, (v, t), c in zip(cfgs, vt, color)]
            rec = np.concatenate(parts)
            entry["readings"][mode] = {"counts": [int(p.shape[0]) for p in parts], "sha256": RC.sha256(rec)}
            blobs.append(rec.astype("<i2").tobytes())
        if full:
            entry["records_file"] = name + ".bin"
            files[name + ".bin"] = b"".join(blobs)
        man["fused"][name] = entry
    files["manifest.json"] = (json.dumps(man, indent=1, sort_keys=True) + "\n").encode()
    return files


def main():
    if not R.available():
        sys.exit("oracle/_ref/libpcs_ref.so is missing: run __graft_entry__.build() where the reference checkout exists")
    os.makedirs(RC.PIN_DIR, exist_ok=True)
    files = build_fixtures()
    for name, data in files.items():
        with open(os.path.join(RC.PIN_DIR, name), "wb") as f:
            f.write(data)
    print("wrote", len(files), "files,", sum(len(d) for d in files.values()), "bytes, to", RC.PIN_DIR)


if __name__ == "__main__":
    main()
