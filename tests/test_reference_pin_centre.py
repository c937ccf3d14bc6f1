"""The centre-side payload kernels held to bytes that the COMPILED REFERENCE's centre programs produced (tests/golden/ref_centre/,
tests/golden/make_ref_centre_golden.py). The companion of test_reference_pin.py, which does the same for the camera program.

The reference's pcs-multicamera-optimized.cpp and pcs-multicamera-client.cpp are compiled, unmodified and with each target's own
flags, against declaration-only PCL stand-ins (oracle/ref/pcl/, oracle/ref/ref_centre_harness.cpp, oracle/ref_centre.py). They
wrote the fixtures; the restatements (oracle/pcs_oracle.c, tests/np_restatement.py) and the HIP kernels behind
pcs_transform_payloads_device and pcs_stitch_device must reproduce them bit for bit. No tolerance anywhere.

Pinned by reference-produced bytes: convertBufferToPointCloudXYZRGB ((float)short / CONV_RATE with a float CONV_RATE, the colour
bytes, i % downsample == 0, the size / downsample width), convertPointCloudXYZRGBToBuffer (static_cast<short>(x * CONV_RATE),
R + (G << 8) with a negative G short, B with its high byte dropped), updateCloudXYZRGB / send_stitchedXYZRGB (the record count of a
frame, the payload offset, the header) and sendStitchToUnity (the `j += 5 * downsample` loop: CEIL(n / d) records, the header).

NOT pinned: the association inside pcl::transformPointCloud. PCL is third-party; PCL 1.8's ((m0*x + m1*y) + m2*z) + m3 is restated
(oracle/ref/pcl_transform_standin.cpp, np_restatement.affine_np). For the matrices the manifest calls "order-independent" (one
entry of +-1 per row plus a translation) the affine is a single rounding under every association, with or without FMA, so those
cases are pinned end to end and assume nothing about PCL; the others are flagged "PCL 1.8 order restated, unpinned".
NOT discriminated either: FLOOR(n / d) for the transform program at n % d != 0. The live reference cannot be driven there (its
decode loop writes one element past its vector, undefined behaviour), so that count stays read from
src/pcs-multicamera-optimized.cpp:230, :253 and is checked against the restatement only (test_gpu_parity.py).

Tiers, as in test_reference_pin.py. CPU tests run everywhere; those that call the live reference need
oracle/_ref/libpcs_ref_centre_{opt,client}.so, which build() makes where the reference checkout exists. GPU tests (marked gpu)
compare against the fixtures always, and against the live libraries when they travelled with the tree.
"""
import importlib.util
import json
import os
import socket
import struct
import subprocess
import threading

import numpy as np
import pytest

import np_restatement as NP
import ref_centre_cases as CC
import ref_pin_cases as RP
import test_wire as W
from oracle import ref_centre as R
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext

NO_LIVE = ("oracle/_ref/libpcs_ref_centre_*.so are not here and there is no reference checkout to build them from: "
           "the comparison with the live reference cannot run (the fixture comparison does)")

with open(CC.MANIFEST) as _f:
    MAN = json.load(_f)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
_payloads = {}


def payload(name):
    """The case's records, rebuilt from integers, checked against the digest taken when the fixture was written."""
    if name not in _payloads:
        p = CC.payload(name)
        assert RP.sha256(p) == MAN["payloads"][name]["inputs_sha256"], \
            f"{name}: the input generator has drifted from the one the fixtures were made with (not a kernel bug)"
        p.setflags(write=False)
        _payloads[name] = p
    return _payloads[name]


def _load(fname):
    return np.fromfile(os.path.join(CC.CENTRE_DIR, fname), dtype="<i2").astype(np.int16)


_stored = {}


def stored_records():
    """{(case, matrix, stride) or (case, stride): int16[count, 5]} for everything the fixtures store in full."""
    if not _stored:
        for fname, pairs in CC.STORED_TRANSFORM.items():
            raw, at = _load(fname), 0
            for c, m in pairs:
                assert MAN["transform"][c][m]["records_file"] == fname
                for d in CC.PAYLOADS[c][1]:
                    cnt = MAN["transform"][c][m][str(d)]["count"]
                    _stored[(c, m, d)] = raw[at:at + 5 * cnt].reshape(-1, 5)
                    at += 5 * cnt
            assert at == raw.size, fname
        raw, at = _load(MAN["stitch_records_file"]), 0
        for c, d in CC.stitch_keys():
            cnt = MAN["stitch"][c][str(d)]["count"]
            _stored[(c, d)] = raw[at:at + 5 * cnt].reshape(-1, 5)
            at += 5 * cnt
        assert at == raw.size
    return _stored


def first_diff(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{bad.size} of {want.shape[0]} records differ; first at {i}: got {got[i]} want {want[i]}"


def assert_is_reference(got, key, what, live=None, where=None):
    """got == the reference's records for key = (case, matrix, stride) or (case, stride): record by record where the fixture (or
    the live reference's output) has them, count and SHA-256 always. Where a case is held by digest only, a mismatch is located
    against `where()` (the oracle's records)."""
    got = np.ascontiguousarray(got, np.int16).reshape(-1, 5)
    e = MAN["transform"][key[0]][key[1]][str(key[2])] if len(key) == 3 else MAN["stitch"][key[0]][str(key[1])]
    want = live if live is not None else stored_records().get(key)
    if want is not None:
        d = first_diff(got, want)
        assert d is None, f"{what} vs reference, {key}: {d}"
    assert got.shape[0] == e["count"], f"{what}, {key}: {got.shape[0]} records, the reference wrote {e['count']}"
    assert e["header"] == 10 * e["count"]
    if RP.sha256(got) != e["sha256"]:
        hint = first_diff(got, where()) if where is not None else "digest only: case not stored in full"
        pytest.fail(f"{what}, {key}: records differ from the reference's; against the oracle: {hint}")


def need_live():
    if not R.centre_available():
        pytest.skip(NO_LIVE)


def live_transform(case, mname, d):
    """encode_ref(affine_np(decode_ref(payload, stride))): both ends the live reference, the middle PCL 1.8 restated."""
    xyz, rgb = R.decode(payload(case), d)
    return R.encode(NP.affine_np(xyz, CC.matrix(mname)), rgb)


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 1: the fixtures are the reference's
# ---------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_ref_centre_golden", os.path.join(RP.GOLD, "make_ref_centre_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_centre_fixtures_are_what_the_compiled_reference_writes():
    """Regenerate every fixture with the live centre programs and compare with the committed files byte for byte. Where the reference
    checkout exists but oracle/_ref/ was not built this FAILS; it skips only where neither exists."""
    if not R.centre_available():
        if R.reference_present():
            pytest.fail("the reference checkout is here but oracle/_ref/libpcs_ref_centre_*.so are not: run __graft_entry__.build()")
        pytest.skip(NO_LIVE)
    files = _generator().build_fixtures()
    on_disk = sorted(os.listdir(CC.CENTRE_DIR))
    assert on_disk == sorted(files), f"tests/golden/ref_centre holds {on_disk}, the generator writes {sorted(files)}"
    for name, data in sorted(files.items()):
        assert len(data) <= 100_000 or name == "manifest.json", f"{name}: {len(data)} bytes"
        with open(os.path.join(CC.CENTRE_DIR, name), "rb") as f:
            have = f.read()
        if have != data and name == "manifest.json":
            a, b = json.loads(have), json.loads(data)
            keys = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            pytest.fail(f"manifest.json differs from what the reference gives now in {keys}; built with {b['reference_build']}, "
                        f"fixtures made with {a['reference_build']}")
        assert have == data, f"{name} is not what the compiled reference writes"


def test_centre_fixture_inputs_have_not_drifted():
    """Every payload and every matrix still hashes to what the fixtures were made from; the manifest names each matrix's class."""
    for name in CC.PAYLOADS:
        payload(name)
    assert sorted(MAN["matrices"]) == sorted(CC.MATRICES)
    for mname, (cls, m) in CC.MATRICES.items():
        e = MAN["matrices"][mname]
        assert RP.sha256(m) == e["sha256"] and e["affine"] == cls, mname
        assert e.get("affine_order_independent", False) == (cls == CC.ORDER_INDEPENDENT)
    for c in CC.TRANSFORM_CASES:
        assert sorted(MAN["transform"][c]) == sorted(CC.MATRICES)
        for m in CC.MATRICES:
            assert {k for k in MAN["transform"][c][m] if k != "records_file"} == {str(d) for d in CC.PAYLOADS[c][1]}
    assert {(c, int(d)) for c in MAN["stitch"] for d in MAN["stitch"][c]} == set(CC.stitch_keys())
    builds = MAN["reference_build"]
    assert "-mfma" not in builds["opt"]["flags"] and "-mavx -mfma" in builds["client"]["flags"]


def test_order_independent_matrices_are_order_independent():
    """The claim the end-to-end pin rests on, re-evaluated here without the reference: for every matrix of that class, PCL's order,
    the FMA-contracted order and right to left give the same float bits on every decoded point of the case set; a restated-class
    matrix does not (so the check can fail)."""
    pts = np.concatenate([NP.decode_payload_np(payload(c), 1)[0] for c in CC.TRANSFORM_CASES])
    for mname in CC.ORDER_INDEPENDENT_NAMES:
        o = CC.affine_orders(pts, CC.matrix(mname))
        assert CC.same_bits(o[0], o[1]) and CC.same_bits(o[0], o[2]), mname
    o = CC.affine_orders(pts, CC.matrix("transform6"))
    assert not CC.same_bits(o[0], o[1]) and not CC.same_bits(o[0], o[2])


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 2: the restatements are pinned (fixtures only: always runs)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.TRANSFORM_CASES)
def test_oracle_transform_payload_is_the_reference(oracle, case):
    p = payload(case)
    for mname in CC.MATRICES:
        for d in CC.PAYLOADS[case][1]:
            assert_is_reference(oracle.transform_payload(p, CC.matrix(mname), d), (case, mname, d), "oracle.transform_payload")


@pytest.mark.parametrize("case", CC.TRANSFORM_CASES)
def test_np_restatement_transform_is_the_reference(case):
    p = payload(case)
    for mname in CC.MATRICES:
        for d in CC.PAYLOADS[case][1]:
            assert_is_reference(NP.transform_payload_np(p, CC.matrix(mname), d), (case, mname, d), "np_restatement.transform_payload_np")


def test_oracle_stitch_is_the_reference(oracle):
    for case, d in CC.stitch_keys():
        p = payload(case)
        assert_is_reference(oracle.stitch([p], d), (case, d), "oracle.stitch")
        assert_is_reference(CC.stitch_np(p, d), (case, d), "stitch_np")
        assert MAN["stitch"][case][str(d)]["count"] == -(-p.shape[0] // d)                      # CEIL, client :388
    sizes = ("tiles_4133", "tiny_0", "tiny_1", "tiny_7")                 # several cameras = one call per camera, joined
    for d in (1, 2, 7):
        want = np.concatenate([stored_records()[(c, d)] for c in sizes])
        d_ = first_diff(oracle.stitch([payload(c) for c in sizes], d), want)
        assert d_ is None, f"oracle.stitch of four cameras, stride {d}: {d_}"


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 3: the case set can tell a misreading from the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_centre_case_set_discriminates_every_misreading():
    """The numpy restatement with ONE thing read differently must change at least one STORED record, and as many as the generator
    counted; read correctly it changes none. Transform program: multiply by 0.001f, a double CONV_RATE, round to nearest, saturate,
    keep B's high byte, sign-extend G (see ref_centre_cases.transform_variant_np for where that can show), i % d == d - 1. Stitch
    program: FLOOR instead of CEIL, the stride counted in shorts instead of records.

    NOT discriminated: FLOOR against CEIL for the TRANSFORM program at n % d != 0. The compiled reference cannot be driven there
    (undefined behaviour in its decode loop), so no fixture has such a case; the count stays read from
    src/pcs-multicamera-optimized.cpp:230, :253.

    Also recounted, over all 65 536 int16 values of a decode -> encode round trip: how many values each arithmetic misreading gets
    wrong (740 for a multiplication by the reciprocal, 1 140 for double arithmetic throughout)."""
    st = stored_records()
    tkeys = [k for k in st if len(k) == 3]
    skeys = [k for k in st if len(k) == 2]
    assert sorted(MAN["misreadings"]) == sorted(CC.TRANSFORM_VARIANTS + CC.STITCH_VARIANTS)

    def changed(variant):
        if variant in CC.STITCH_VARIANTS:
            return sum(RP.records_changed(CC.stitch_variant_np(payload(c), d, variant), st[(c, d)]) for c, d in skeys)
        return sum(RP.records_changed(CC.transform_variant_np(payload(c), CC.matrix(m), d, variant), st[(c, m, d)]) for c, m, d in tkeys)

    assert changed(None) == 0
    assert sum(RP.records_changed(CC.stitch_variant_np(payload(c), d), st[(c, d)]) for c, d in skeys) == 0
    for variant in CC.TRANSFORM_VARIANTS + CC.STITCH_VARIANTS:
        n = changed(variant)
        print(f"{variant}: {n} records changed")
        assert n > 0, f"the case set cannot tell '{variant}' from the reference"
        assert n == MAN["misreadings"][variant]["records_changed"], variant
    counts = CC.roundtrip_int16_counts()
    print("round trip of every int16 value:", counts)
    assert counts == MAN["roundtrip_int16"]["values_a_misreading_gets_wrong"] and all(v > 0 for v in counts.values())


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 4: live sweep
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_case(k):
    """Payload and matrix k of the sweep, from the counter hash: full-range records, a count with many divisors, matrices of both
    classes (a signed permutation with a random translation; a random 3x4)."""
    n = (5040, 2520, 720, 10080, 1, 0, 27720)[k % 7]
    key = 0x0CE27E00 + 1009 * k
    p = CC._shorts(5 * n, key).reshape(n, 5)
    t = ((RP.uniform(3, key + 1) - 0.5) * (80.0 if k % 2 else 8.0)).astype(np.float32)
    if k % 2:
        perm = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)][(k // 2) % 6]
        sign = [1 - 2 * ((k >> (3 + a)) & 1) for a in range(3)]
        m = np.zeros(16, np.float32)
        for r in range(3):
            m[4 * r + perm[r]] = sign[r]
            m[4 * r + 3] = t[r]
        m[15] = 1
    else:
        m = np.eye(4, dtype=np.float32).reshape(-1)
        m[:12] = ((RP.uniform(12, key + 2) - 0.5) * 2.0).astype(np.float32)
        m[3:12:4] = t
    strides = [d for d in (1, 2, 3, 5, 7, 8) if n % d == 0]
    return p, m, strides, bool(k % 2)


def test_live_sweep_centre_programs(oracle):
    """About 20 more payloads and matrices of both classes against the live reference: decode and encode of the optimized program
    equal those of the client program bit for bit (-mavx -mfma changes nothing in these functions); oracle.transform_payload equals
    encode_ref(affine_np(decode_ref)) and what update_and_send serves; for the order-independent matrices every evaluation order
    gives the same records; oracle.stitch equals sendStitchToUnity at strides with and without a remainder; encode of special
    floats (NaN, infinities, beyond 2^31, the int16 edges) is the same in both programs and in the numpy restatement; the harness
    refuses n % d != 0."""
    need_live()
    total = 0
    for k in range(21):
        p, m, strides, indep = _sweep_case(k)
        for d in strides:
            xyz, rgb = R.decode(p, d, "opt")
            xyz_c, rgb_c = R.decode(p, d, "client")
            assert CC.same_bits(xyz, xyz_c) and np.array_equal(rgb, rgb_c), f"sweep {k} d{d}: decode differs between the programs"
            xn, rn = NP.decode_payload_np(p, d)
            assert CC.same_bits(xyz, xn) and np.array_equal(rgb, rn), f"sweep {k} d{d}: decode_payload_np"
            orders = CC.affine_orders(xyz, m)
            if indep:
                assert CC.same_bits(orders[0], orders[1]) and CC.same_bits(orders[0], orders[2])
            want = R.encode(orders[0], rgb, "opt")
            assert np.array_equal(want, R.encode(orders[0], rgb, "client")), f"sweep {k} d{d}: encode differs between the programs"
            diff = first_diff(oracle.transform_payload(p, m, d), want)
            assert diff is None, f"sweep {k} d{d} oracle.transform_payload: {diff}"
            size, served = R.split_frame(R.update_and_send(p, m, d))
            assert size == want.nbytes and first_diff(served, want) is None, f"sweep {k} d{d}: update_and_send"
            total += want.shape[0]
        for d in (1, 2, 3, 11, 4999):
            size, served = R.split_frame(R.stitch(p, d))
            diff = first_diff(oracle.stitch([p], d), served)
            assert diff is None and size == served.nbytes, f"sweep {k} stitch d{d}: {diff}"
            total += served.shape[0]
    sp = np.array([np.nan, np.inf, -np.inf, 3e6, -3e6, 2.2e9, 1e30, 32.767, -32.768, 32.7675, 65.536, -0.0, 2147483.5, -2147483.75],
                  np.float32)
    xyz = np.stack([sp, np.roll(sp, 1), np.roll(sp, 2)], -1)
    rgb = (np.arange(3 * sp.size) * 37 % 256).astype(np.uint8).reshape(-1, 3)
    e = R.encode(xyz, rgb, "opt")
    assert np.array_equal(e, R.encode(xyz, rgb, "client")) and np.array_equal(e, NP.encode_payload_np(xyz, rgb))
    with pytest.raises(ValueError):
        R.decode(payload("tiny_7"), 2)
    with pytest.raises(ValueError):
        R.update_and_send(payload("tiny_7"), CC.matrix("identity"), 2)
    print(f"{total} records compared with the live centre programs")
    assert total > 200_000


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------
IN_PHASES = (0, 4, 2, 10)            # byte offsets of a camera's payload inside a 16-byte line
OUT_PHASES = (0, 4, 10)
ALL_STRIDES = sorted({d for c in CC.TRANSFORM_CASES for d in CC.PAYLOADS[c][1]})


def _ctx():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48)
    return PcsContext(cfgs)


@pytest.mark.gpu
@pytest.mark.parametrize("against", ["fixture", "live"])
@pytest.mark.parametrize("stride", ALL_STRIDES)
def test_transform_payloads_device_is_the_reference(oracle, stride, against):
    """pcs_transform_payloads_device on every case and matrix that the stride divides, all in ONE call (15 to 90 cameras; a launch
    holds 16, so all strides but 3 take several), camera i's payload at byte phase IN_PHASES[i % 4] of a 16-byte line (each case meets every phase, its 15 matrices
    rotating through them), the output at phases 0, 4 (the wire's buffer + 2 shorts) and 10. At stride 1 the full, aligned tile
    path, the staged ragged / unaligned one; at the others the strided gather."""
    cams = [(c, m) for c in CC.TRANSFORM_CASES if stride in CC.PAYLOADS[c][1] for m in CC.MATRICES]
    assert len(cams) >= len(CC.MATRICES)
    if against == "live":
        need_live()
    lives = [live_transform(c, m, stride) if against == "live" else None for c, m in cams]
    counts = [MAN["transform"][c][m][str(stride)]["count"] for c, m in cams]
    total_want = sum(counts)
    with _ctx() as ctx:
        dptr, bases = [], []
        try:
            for i, (c, m) in enumerate(cams):
                p = payload(c)
                bases.append(ctx.device_malloc(max(p.nbytes, 16) + 64))
                dptr.append(bases[-1] + IN_PHASES[i % len(IN_PHASES)])
                if p.size:
                    ctx.memcpy_h2d(dptr[-1], p)
            out = ctx.device_malloc(total_want * 10 + 64)
            bases.append(out)
            mats = [CC.matrix(m) for _, m in cams]
            for out_phase in OUT_PHASES:
                per, total = ctx.transform_payloads_device(dptr, [payload(c).shape[0] for c, _ in cams], mats, stride,
                                                           out + out_phase, total_want * 5)
                ctx.synchronize()
                assert per == counts and total == total_want
                got = np.empty((total_want, 5), np.int16)
                ctx.memcpy_d2h(got, out + out_phase)
                at = 0
                for (c, m), cnt, live in zip(cams, counts, lives):
                    assert_is_reference(got[at:at + cnt], (c, m, stride), f"pcs_transform_payloads_device (out phase {out_phase})", live=live,
                                        where=lambda c=c, m=m: oracle.transform_payload(payload(c), CC.matrix(m), stride))
                    at += cnt
        finally:
            for b in bases:
                ctx.device_free(b)


@pytest.mark.gpu
def test_transform_payloads_device_twenty_cameras_and_in_place(oracle):
    """Exactly 20 cameras in one call (two launches of 16 and 4), mixed sizes at stride 1; then one camera transformed in place."""
    pairs = [(c, m) for c in ("tiles_4200", "tiny_7", "colour_bits", "tiny_0", "tiny_1") for m in
             ("perm_wrap", "identity", "transform3", "wild")]
    assert len(pairs) == 20
    with _ctx() as ctx:
        bases = []
        try:
            dptr = []
            for i, (c, m) in enumerate(pairs):
                p = payload(c)
                bases.append(ctx.device_malloc(max(p.nbytes, 16) + 64))
                dptr.append(bases[-1] + IN_PHASES[(i + 1) % len(IN_PHASES)])
                if p.size:
                    ctx.memcpy_h2d(dptr[-1], p)
            counts = [payload(c).shape[0] for c, _ in pairs]
            out = ctx.device_malloc(sum(counts) * 10 + 64)
            bases.append(out)
            per, total = ctx.transform_payloads_device(dptr, counts, [CC.matrix(m) for _, m in pairs], 1, out + 4, sum(counts) * 5)
            ctx.synchronize()
            assert per == counts and total == sum(counts)
            got = np.empty((total, 5), np.int16)
            ctx.memcpy_d2h(got, out + 4)
            at = 0
            for (c, m), cnt in zip(pairs, counts):
                assert_is_reference(got[at:at + cnt], (c, m, 1), "pcs_transform_payloads_device (20 cameras)",
                                    where=lambda c=c, m=m: oracle.transform_payload(payload(c), CC.matrix(m), 1))
                at += cnt
            for c, m in (("sweep_int16", "perm_wrap"), ("tiles_4200", "transform6")):       # in place: output = input
                p = payload(c)
                buf = ctx.device_malloc(p.nbytes + 64)
                bases.append(buf)
                ctx.memcpy_h2d(buf, p)
                per, total = ctx.transform_payloads_device([buf], [p.shape[0]], [CC.matrix(m)], 1, buf, p.size)
                ctx.synchronize()
                got = np.empty_like(p)
                ctx.memcpy_d2h(got, buf)
                assert_is_reference(got, (c, m, 1), "pcs_transform_payloads_device (in place)",
                                    where=lambda c=c, m=m: oracle.transform_payload(payload(c), CC.matrix(m), 1))
        finally:
            for b in bases:
                ctx.device_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("against", ["fixture", "live"])
def test_stitch_device_is_the_reference(oracle, against):
    """pcs_stitch_device on every stitch case and stride, into an aligned buffer and into one at +4 bytes (the reference's
    stitched_buf + 2 shorts); then four cameras of 4133, 0, 1 and 7 records in one call against the reference's per-camera frames
    joined in camera order."""
    if against == "live":
        need_live()

    def want_of(c, d):
        return R.split_frame(R.stitch(payload(c), d))[1] if against == "live" else None

    with _ctx() as ctx:
        dev = {}
        try:
            for c in CC.STITCH_CASES:
                p = payload(c)
                dev[c] = ctx.device_malloc(max(p.nbytes, 16))
                if p.size:
                    ctx.memcpy_h2d(dev[c], p)
            out = ctx.device_malloc(sum(payload(c).nbytes for c in CC.STITCH_CASES) + 64)
            dev["out"] = out
            for c, d in CC.stitch_keys():
                cnt = MAN["stitch"][c][str(d)]["count"]
                for skew in (0, 4):
                    total = ctx.stitch_device([dev[c]], [payload(c).shape[0]], d, out + skew, max(cnt, 1) * 5)
                    ctx.synchronize()
                    assert total == cnt
                    got = np.empty((cnt, 5), np.int16)
                    if cnt:
                        ctx.memcpy_d2h(got, out + skew)
                    assert_is_reference(got, (c, d), f"pcs_stitch_device (+{skew} B)", live=want_of(c, d))
            four = ("tiles_4133", "tiny_0", "tiny_1", "tiny_7")
            for d in (1, 2, 7):
                counts = [MAN["stitch"][c][str(d)]["count"] for c in four]
                total = ctx.stitch_device([dev[c] for c in four], [payload(c).shape[0] for c in four], d, out + 4, sum(counts) * 5)
                ctx.synchronize()
                assert total == sum(counts)
                got = np.empty((total, 5), np.int16)
                ctx.memcpy_d2h(got, out + 4)
                at = 0
                for c, cnt in zip(four, counts):
                    assert_is_reference(got[at:at + cnt], (c, d), f"pcs_stitch_device (four cameras, stride {d})", live=want_of(c, d))
                    at += cnt
        finally:
            for b in dev.values():
                ctx.device_free(b)


@pytest.mark.gpu
@W.retry_server_start
def test_central_cli_serves_the_bytes_update_and_send_wrote(tmp_path):
    """`pcs-multicamera-optimized -c <one camera> -T <an order-independent matrix> -d 3`: what the consumer receives, header included,
    is what the compiled reference's updateCloudXYZRGB / += / send_stitchedXYZRGB served for the same frame (the fixture's header and
    records; the live library's bytes too where it travelled with the tree). The camera is played by this test: it answers one 'Z'
    pull with the frame, as the edge program does."""
    subprocess.run(["make", "-C", W.CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    case, mname, d = "tiles_4200", "perm_wrap", 3
    p = payload(case)
    e = MAN["transform"][case][mname][str(d)]
    want = struct.pack("<i", e["header"]) + stored_records()[(case, mname, d)].astype("<i2").tobytes()
    tf = tmp_path / "transforms.txt"
    tf.write_text(" ".join(repr(float(v)) for v in CC.matrix(mname)) + "\n")
    frame = R.wire_frame(p).tobytes()
    cam = socket.socket()
    cam.bind(("127.0.0.1", 0))
    cam.listen(1)
    cam.settimeout(120)
    p3 = W.free_port()
    served = []

    def camera():
        try:
            conn, _ = cam.accept()
            conn.settimeout(120)
            if conn.recv(1) == b"Z":
                conn.sendall(frame)
                served.append(True)
                while conn.recv(64):          # the next pull, then the central's close
                    pass
            conn.close()
        except OSError:
            pass

    th = threading.Thread(target=camera, daemon=True)
    th.start()
    central = subprocess.Popen([W.CENTRAL, "-c", f"127.0.0.1:{cam.getsockname()[1]}", "-d", str(d), "-p", str(p3), "-r", "1",
                                "-T", str(tf)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        consumer = W.connect(p3, procs=[central])
        consumer.sendall(b"Z")
        got = W.read_n(consumer, len(want))
        consumer.close()
        _, err = central.communicate(timeout=60)
        assert central.returncode == 0, err
    finally:
        if central.poll() is None:
            central.kill()
        cam.close()
        th.join(timeout=10)
    assert served == [True]
    assert got[:4] == want[:4], f"header {got[:4].hex()} vs the reference's {want[:4].hex()}"
    assert got == want, first_diff(np.frombuffer(got[4:], "<i2").reshape(-1, 5), np.frombuffer(want[4:], "<i2").reshape(-1, 5))
    if R.centre_available():
        assert got == R.update_and_send(p, CC.matrix(mname), d)
