#!/usr/bin/env python3
"""Regenerates tests/golden/ref_centre/: what the COMPILED REFERENCE's centre programs (oracle/_ref/libpcs_ref_centre_{opt,client}.so,
see oracle/ref_centre.py) write for the inputs of tests/ref_centre_cases.py. Needs the reference checkout; run from the repo root
after __graft_entry__.build():

    python tests/golden/make_ref_centre_golden.py

Transform cases (pcs-multicamera-optimized). The expected records are  encode_ref(affine_np(decode_ref(payload, stride))):  both ends
are the live reference's convertBufferToPointCloudXYZRGB and convertPointCloudXYZRGBToBuffer, the middle is the numpy restatement of
PCL 1.8's affine. For every case the generator also runs update_and_send (updateCloudXYZRGB, +=, send_stitchedXYZRGB over
socketpairs) and requires the same bytes behind the header it checks, so the stand-in transform and the numpy one agree and the
count, the payload offset and the header are the reference's. The decode and encode of the client program (built with -mavx -mfma)
must give the same bits as the optimized program's.

Matrices come in two classes (manifest: matrices/<name>/affine). For an "order-independent" matrix the generator evaluates the affine
under three orders and asserts identical bits: those cases are pinned end to end by reference-compiled code and assume nothing about
PCL. The others are flagged "PCL 1.8 order restated, unpinned".

Stitch cases (pcs-multicamera-client) are the bytes of sendStitchToUnity.

build_fixtures() returns {file name: bytes} without touching the tree; tests/test_reference_pin_centre.py calls it to check that
the committed files are what the reference produces today.
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

import np_restatement as NP                            # noqa: E402
import ref_centre_cases as CC                          # noqa: E402
import ref_pin_cases as RP                             # noqa: E402
from oracle import ref_centre as R                     # noqa: E402


def expected_transform(p, m16, d):
    """encode_ref(affine_np(decode_ref)) with both compiled programs required to agree on both ends."""
    xyz, rgb = R.decode(p, d, "opt")
    xyz_c, rgb_c = R.decode(p, d, "client")
    assert CC.same_bits(xyz, xyz_c) and np.array_equal(rgb, rgb_c), "decode: -mavx -mfma changes the client program's bits"
    w = NP.affine_np(xyz, m16)
    rec = R.encode(w, rgb, "opt")
    assert np.array_equal(rec, R.encode(w, rgb, "client")), "encode: -mavx -mfma changes the client program's bits"
    return rec, xyz


def build_fixtures():
    files = {}
    man = {"_about": "Outputs of the compiled reference's centre programs (src/pcs-multicamera-optimized.cpp, "
                     "src/pcs-multicamera-client.cpp) on the inputs of tests/ref_centre_cases.py. Written by "
                     "tests/golden/make_ref_centre_golden.py; data only.",
           "reference_build": {"opt": R.compiler("opt"), "client": R.compiler("client")},
           "pinned": "decode (convertBufferToPointCloudXYZRGB), encode (convertPointCloudXYZRGBToBuffer), the stride rules, the "
                     "counts and the framing (header, payload offset) of both programs",
           "unpinned": "the association inside pcl::transformPointCloud (third-party): PCL 1.8's ((m0*x + m1*y) + m2*z) + m3 is "
                       "restated. It does not matter for the order-independent matrices. Also not discriminated: FLOOR for the "
                       "transform program at n % d != 0; the live reference cannot be driven there (its loop writes past its "
                       "vector), so that count stays read from src/pcs-multicamera-optimized.cpp:230, :253.",
           "undefined_behaviour_note": "short(float) of NaN, infinities and values outside int's range is formally undefined; the "
                                       "matrices perm_3e6, perm_inf, perm_nan and wild hold what this compile does (cvttss2si: "
                                       "0x80000000, low half kept).",
           "payloads": {}, "matrices": {}, "transform": {}, "stitch": {}, "misreadings": {}}

    pay = {}
    for name, (n, t_strides, s_strides) in CC.PAYLOADS.items():
        pay[name] = CC.payload(name)
        assert pay[name].shape == (n, 5)
        man["payloads"][name] = {"records": n, "inputs_sha256": RP.sha256(pay[name]), "transform_strides": list(t_strides),
                                 "stitch_strides": list(s_strides)}

    # ---- matrices: class, bytes, and for the order-independent class the proof on this case set's own decoded points
    probe = np.concatenate([R.decode(pay[c], 1)[0] for c in CC.TRANSFORM_CASES])
    for mname, (cls, m) in CC.MATRICES.items():
        e = {"affine": cls, "sha256": RP.sha256(m), "values": [repr(float(v)) for v in m]}
        if cls == CC.ORDER_INDEPENDENT:
            orders = CC.affine_orders(probe, m)
            assert CC.same_bits(orders[0], orders[1]) and CC.same_bits(orders[0], orders[2]), f"{mname} is not order-independent"
            e["affine_order_independent"] = True
            e["orders_compared"] = ["PCL 1.8", "PCL 1.8 FMA-contracted", "right to left"]
            e["points_compared"] = int(probe.shape[0])
        man["matrices"][mname] = e

    # ---- transform cases
    recs = {}
    for case, mname, d in CC.transform_keys():
        m = CC.matrix(mname)
        rec, _ = expected_transform(pay[case], m, d)
        sent = R.update_and_send(pay[case], m, d)
        size, sent_rec = R.split_frame(sent)
        assert size == rec.nbytes == 10 * (pay[case].shape[0] // d) and len(sent) == 4 + size, (case, mname, d)
        assert np.array_equal(sent_rec, rec), f"{case}/{mname}/d{d}: update_and_send's bytes are not encode(affine_np(decode))"
        recs[(case, mname, d)] = rec
        man["transform"].setdefault(case, {}).setdefault(mname, {})[str(d)] = {
            "count": int(rec.shape[0]), "header": int(size), "sha256": RP.sha256(rec)}
    for fname, pairs in CC.STORED_TRANSFORM.items():
        files[fname] = b"".join(recs[(c, m, d)].astype("<i2").tobytes() for c, m in pairs for d in CC.PAYLOADS[c][1])
        for c, m in pairs:
            man["transform"][c][m]["records_file"] = fname

    # ---- stitch cases
    srecs = {}
    for case, d in CC.stitch_keys():
        sent = R.stitch(pay[case], d)
        size, rec = R.split_frame(sent)
        assert len(sent) == 4 + size and size == rec.nbytes
        srecs[(case, d)] = rec
        man["stitch"].setdefault(case, {})[str(d)] = {"count": int(rec.shape[0]), "header": int(size), "sha256": RP.sha256(rec)}
    files[CC.STORED_STITCH_FILE] = b"".join(srecs[k].astype("<i2").tobytes() for k in CC.stitch_keys())
    man["stitch_records_file"] = CC.STORED_STITCH_FILE

    # ---- the case set tells every misreading from the reference (counted over the records stored in full)
    stored = [(c, m, d) for pairs in CC.STORED_TRANSFORM.values() for c, m in pairs for d in CC.PAYLOADS[c][1]]
    def changed_t(variant):
        return sum(RP.records_changed(CC.transform_variant_np(pay[c], CC.matrix(m), d, variant), recs[(c, m, d)]) for c, m, d in stored)
    def changed_s(variant):
        return sum(RP.records_changed(CC.stitch_variant_np(pay[c], d, variant), srecs[(c, d)]) for c, d in CC.stitch_keys())
    assert changed_t(None) == 0 and changed_s(None) == 0
    for v in CC.TRANSFORM_VARIANTS + CC.STITCH_VARIANTS:
        n = changed_s(v) if v in CC.STITCH_VARIANTS else changed_t(v)
        assert n > 0, f"the case set cannot tell '{v}' from the reference: add inputs"
        man["misreadings"][v] = {"records_changed": n, "of": "stitch" if v in CC.STITCH_VARIANTS else "transform"}

    # ---- recount: a decode -> encode round trip of every int16 value, compiled reference against each arithmetic misreading
    allv = np.arange(-32768, 32768, dtype=np.int16)
    p = np.zeros((65536, 5), np.int16)
    p[:, 0] = allv
    xyz, rgb = R.decode(p, 1)
    live = R.encode(xyz, rgb)[:, 0]
    ident = CC.matrix("identity")
    assert np.array_equal(live, CC.transform_variant_np(p, ident, 1)[:, 0])
    counts = {v: int((CC.transform_variant_np(p, ident, 1, v)[:, 0] != live).sum())
              for v in CC.ROUNDTRIP_VARIANTS}
    assert counts == CC.roundtrip_int16_counts()
    man["roundtrip_int16"] = {"values": 65536, "round_trip_is_identity_on": int((live == allv).sum()),
                              "values_a_misreading_gets_wrong": counts}
    files["manifest.json"] = (json.dumps(man, indent=1, sort_keys=True) + "\n").encode()
    return files


def main():
    if not R.centre_available():
        sys.exit("oracle/_ref/libpcs_ref_centre_*.so are missing: run __graft_entry__.build() where the reference checkout exists")
    os.makedirs(CC.CENTRE_DIR, exist_ok=True)
    files = build_fixtures()
    for name, data in files.items():
        with open(os.path.join(CC.CENTRE_DIR, name), "wb") as f:
            f.write(data)
    print("wrote", len(files), "files,", sum(len(d) for d in files.values()), "bytes, to", CC.CENTRE_DIR)


if __name__ == "__main__":
    main()
