"""The pack path held to bytes that the COMPILED REFERENCE produced (tests/golden/ref_pin/, tests/golden/make_ref_pin_golden.py).

Everything else in this suite compares a HIP kernel with oracle/, a restatement of the reference written by this project. Here the
chain is closed: the reference's own translation unit, compiled with its own flags (oracle/ref/, oracle/ref_pin.py), wrote the
fixtures; the restatements (oracle/pcs_oracle.c, the AVX2 baseline, tests/np_restatement.py) and the HIP kernels must reproduce
them bit for bit. No tolerance anywhere.

Pinned by reference-produced bytes: a1 sendXYZRGBPointcloud (buffer layout), a2 copyPointCloudXYZRGBToBufferSIMD (`-m`, dense and
`-c` with its reversed-mask order), a3 copyPointCloudXYZRGBToBuffer (non-`-m`, dense).
NOT pinned here: a5 deprojection (librealsense's arithmetic), the voxel grid, and the central programs, which
test_reference_pin_centre.py pins (decode, encode, stride and framing; the association inside PCL's transform stays restated).

Tiers. CPU tests run everywhere; those that call the live reference need oracle/_ref/libpcs_ref.so, which build() makes where the
reference checkout exists. GPU tests (marked gpu) compare against the fixtures always, and against the live library when it
travelled with the tree.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import ref_pin_cases as RC
from np_restatement import cutoff_keep_np, pack_np
from oracle import ref_pin as R
from pointcloud_stitching_amd.api import PcsContext
from pointcloud_stitching_amd.types import (FLAG_CUTOFF, FLAG_CUTOFF_COMPAT, FLAG_FORCE_IEEE, REF_BUF_SIZE, make_intrinsics,
                                            make_stream_config)

CUT = FLAG_CUTOFF | FLAG_CUTOFF_COMPAT
NO_LIVE = ("oracle/_ref/libpcs_ref.so is not here and there is no reference checkout to build it from: "
           "the comparison with the live reference cannot run (the fixture comparison does)")

with open(RC.MANIFEST) as _f:
    MAN = json.load(_f)
PREFILL = MAN["prefill"]
ALL_CASES = list(RC.CASES)
FULL_CASES = [c for c in ALL_CASES if RC.CASES[c][6]]


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
_inputs_cache = {}


def case_inputs(name):
    """The case's inputs, rebuilt from integers, checked against the digest taken when the fixture was written."""
    if name not in _inputs_cache:
        sc, V, T, col = RC.build_case(name)
        assert RC.inputs_sha256(sc, V, T, col) == MAN["cases"][name]["inputs_sha256"], \
            f"{name}: the input generator has drifted from the one the fixtures were made with (not a kernel bug)"
        if len(_inputs_cache) > 4:
            _inputs_cache.clear()
        _inputs_cache[name] = (sc, V, T, col)
    return _inputs_cache[name]


def fixture_records(name, section="cases"):
    """mode -> int16[count, 5] for a case stored in full, else None."""
    e = MAN[section][name]
    if "records_file" not in e:
        return None
    raw = np.fromfile(os.path.join(RC.PIN_DIR, e["records_file"]), dtype="<i2").astype(np.int16)
    out, at = {}, 0
    for mode in (RC.MODES if section == "cases" else RC.FUSED_MODES):
        r = e["readings"][mode]
        cnt = r["count"] if section == "cases" else sum(r["counts"])
        out[mode] = raw[at:at + 5 * cnt].reshape(-1, 5)
        at += 5 * cnt
    assert at == raw.size
    return out


def first_diff(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{bad.size} of {want.shape[0]} records differ; first at {i}: got {got[i]} want {want[i]}"


def assert_is_reference(got, name, mode, what, section="cases", live=None):
    """got == the reference's records for (case, mode): count and SHA-256 always, record by record where the fixture (or the live
    reference's output) has them."""
    got = np.ascontiguousarray(got, np.int16).reshape(-1, 5)
    r = MAN[section][name]["readings"][mode]
    want = live
    if want is None:
        full = fixture_records(name, section)
        want = full[mode] if full else None
    if want is not None:
        d = first_diff(got, want)
        assert d is None, f"{what} vs reference, {name}/{mode}: {d}"
    count = r["count"] if section == "cases" else sum(r["counts"])
    assert got.shape[0] == count, f"{what}, {name}/{mode}: {got.shape[0]} records, the reference wrote {count}"
    assert RC.sha256(got) == r["sha256"], f"{what}, {name}/{mode}: records differ from the reference's (digest only: case not stored in full)"


def need_live():
    if not R.available():
        pytest.skip(NO_LIVE)


def live_records(name, mode):
    sc, V, T, col = case_inputs(name)
    return R.pack_config(sc, V, T, col, simd=(mode != "scalar"), cutoff=(mode == "cut"))


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 1: the fixtures are the reference's
# ---------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_ref_pin_golden", os.path.join(RC.GOLD, "make_ref_pin_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixtures_are_what_the_compiled_reference_writes():
    """Regenerate every fixture with the live reference and compare with the committed files byte for byte. Where the reference
    checkout exists but oracle/_ref/ was not built this FAILS; it skips only where neither exists."""
    if not R.available():
        if R.reference_present():
            pytest.fail("the reference checkout is here but oracle/_ref/libpcs_ref.so is not: run __graft_entry__.build()")
        pytest.skip(NO_LIVE)
    files = _generator().build_fixtures()
    on_disk = sorted(os.listdir(RC.PIN_DIR))
    assert on_disk == sorted(files), f"tests/golden/ref_pin holds {on_disk}, the generator writes {sorted(files)}"
    for name, data in sorted(files.items()):
        with open(os.path.join(RC.PIN_DIR, name), "rb") as f:
            have = f.read()
        if have != data and name == "manifest.json":
            a, b = json.loads(have), json.loads(data)
            keys = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            sub = [f"{k}/{c}" for k in keys if isinstance(a.get(k), dict) and isinstance(b.get(k), dict)
                   for c in sorted(set(a[k]) | set(b[k])) if a[k].get(c) != b[k].get(c)]
            pytest.fail(f"manifest.json differs from what the reference gives now in {keys} {sub[:12]}; built with "
                        f"{b['reference_build']}, fixtures made with {a['reference_build']}")
        assert have == data, f"{name} is not what the compiled reference writes"


def test_fixture_inputs_have_not_drifted(oracle):
    """Every case's inputs, and the fused cases' deprojected points, still hash to what the fixtures were made from."""
    for name in ALL_CASES:
        _inputs_cache.clear()
        case_inputs(name)
    for name, e in MAN["fused"].items():
        cfgs, depth, color = RC.build_fused(name)
        vt = [oracle.deproject(sc, d) for sc, d in zip(cfgs, depth)]
        sha = RC.sha256(np.concatenate([np.concatenate([v.reshape(-1), t.reshape(-1)]) for v, t in vt]))
        assert sha == e["deprojected_sha256"], f"{name}: the restated deprojection or the frame generator has drifted"


def test_kat_appendix_b_is_regenerated_not_only_transcribed():
    """The eight hand-transcribed vectors of kat_appendix_b.json equal the fixture the compiled reference wrote for them."""
    with open(os.path.join(RC.GOLD, "kat_appendix_b.json")) as f:
        k = json.load(f)
    B = np.array([[int(x, 16) for x in v["bytes"].split()] for v in k["vectors"]], np.uint8)
    rec = fixture_records("kat_appendix_b")
    assert np.array_equal(np.ascontiguousarray(rec["dense"]).view(np.uint8).reshape(-1, 10), B)
    assert MAN["cases"]["kat_appendix_b"]["equals_kat_appendix_b_json"] is True
    # the scalar_variant_note of that file: row 0's y is 3415 on the non -m path
    assert rec["scalar"][0, 1] == 3415 and rec["dense"][0, 1] == 3416


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 2: the restatements are pinned (fixtures only: always runs)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_pack_is_the_reference(oracle, name):
    sc, V, T, col = case_inputs(name)
    assert_is_reference(oracle.pack(sc, V, T, col), name, "dense", "oracle.pack")
    assert_is_reference(oracle.pack(sc, V, T, col, flags=CUT), name, "cut", "oracle.pack(-c compat)")


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_pack_simd_omp_is_the_reference(oracle, name, threads):
    if not oracle.lib().pcs_oracle_simd_available():
        pytest.fail("the AVX2+FMA baseline cannot run on this CPU")
    sc, V, T, col = case_inputs(name)
    assert_is_reference(oracle.pack_simd_omp(sc, V, T, col, threads), name, "dense", f"oracle.pack_simd_omp(t={threads})")
    assert MAN["cases"][name]["readings"]["dense"]["t4_equals_t1"] is True      # the reference's own -t4 gave the same bytes


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_pack_scalar_variant_is_the_reference(oracle, name):
    sc, V, T, col = case_inputs(name)
    assert_is_reference(oracle.pack_scalar_variant(sc, V, T, col), name, "scalar", "oracle.pack_scalar_variant")


@pytest.mark.parametrize("name", ALL_CASES)
def test_np_restatement_is_the_reference(name):
    sc, V, T, col = case_inputs(name)
    assert_is_reference(pack_np(sc, V, T, col), name, "dense", "np_restatement.pack_np")
    keep = cutoff_keep_np(V, compat=True)
    assert_is_reference(pack_np(sc, V[keep], T[keep], col), name, "cut", "np_restatement cutoff_keep_np + pack_np")


@pytest.mark.parametrize("mode", ["dense", "cut"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_send_whole_buffer_is_the_reference(oracle, name, mode):
    """a1 on its whole buffer: the 4-byte header slot, the records from short 2 on, the returned size, the cleared BUF_SIZE-byte
    prefix and the untouched bytes beyond it (the reference clears under every mode, -c included)."""
    sc, V, T, col = case_inputs(name)
    e = MAN["cases"][name]
    r = e["readings"][mode]
    assert MAN["buf_size"] == REF_BUF_SIZE
    shorts = (e["buffer_bytes"] + 1) // 2
    flags = CUT if mode == "cut" else 0
    buf, size = oracle.send_xyzrgb_pointcloud(sc, V, T, col, flags=flags, buffer_shorts=shorts, write_header=False, prefill=PREFILL)
    assert size == r["size"] == 10 * r["count"]
    full = fixture_records(name)
    if full:
        want = RC.expected_buffer(full[mode], PREFILL, MAN["buf_size"], e["buffer_bytes"])
        bad = np.nonzero(buf != want)[0]
        assert bad.size == 0, f"{bad.size} shorts differ, first at {bad[:8]}"
    assert RC.sha256(buf) == r["buffer_sha256"]
    # the reference writes the header only when it sends: header on = the same buffer with the size in its first four bytes
    buf2, size2 = oracle.send_xyzrgb_pointcloud(sc, V, T, col, flags=flags, buffer_shorts=shorts, write_header=True, prefill=PREFILL)
    assert size2 == size and buf2[:2].tobytes() == int(size).to_bytes(4, "little", signed=True)
    assert np.array_equal(buf2[2:], buf[2:]) and not buf[:2].any()


@pytest.mark.parametrize("mode", list(RC.FUSED_MODES))
@pytest.mark.parametrize("name", list(RC.FUSED))
def test_oracle_process_frames_pack_half_is_the_reference(oracle, name, mode):
    """oracle.process_frames = its own deprojection, then a pack that must be the reference's. Deprojection is NOT pinned here."""
    cfgs, depth, color = RC.build_fused(name)
    got, counts = oracle.process_frames(cfgs, depth, color, flags=CUT if mode == "cut" else 0)
    assert counts == MAN["fused"][name]["readings"][mode]["counts"]
    assert_is_reference(got, name, mode, "oracle.process_frames", section="fused")


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 3: the case set can tell a misreading from the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_case_set_discriminates_every_misreading():
    """np_restatement's arithmetic with ONE thing read differently must change at least one record of the stored cases, and as many
    as the generator counted; read correctly it changes none. (Records are compared position by position, so one record more or
    less under -c counts every record after it.)"""
    small = {}
    for name in FULL_CASES:
        sc, V, T, col = RC.build_case(name)
        assert RC.inputs_sha256(sc, V, T, col) == MAN["cases"][name]["inputs_sha256"], f"{name}: input generator drift"
        rec = fixture_records(name)
        small[name] = (sc, V, T, col, rec["dense"], rec["cut"])
    assert RC.count_variant(None, small) == 0
    assert RC.count_variant("cut:none", small) == 0
    assert sorted(MAN["misreadings"]) == sorted(RC.DENSE_VARIANTS + RC.CUT_VARIANTS)
    for variant in RC.DENSE_VARIANTS + RC.CUT_VARIANTS:
        changed = RC.count_variant(variant, small)
        print(f"{variant}: {changed} records changed")
        assert changed > 0, f"the case set cannot tell '{variant}' from the reference"
        assert changed == MAN["misreadings"][variant]["records_changed"], variant


# ---------------------------------------------------------------------------------------------------------------------
# CPU tier 4: live sweep
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_case(k):
    """Geometry k of the sweep: a raster size, a pixel format, a random 3x4 matrix and points, all from the counter hash."""
    sizes = [(8, 4), (64, 48), (321, 243), (640, 480), (1280, 720), (848, 480), (37, 5), (640, 360), (424, 240), (1, 7)]
    w, h = sizes[k % len(sizes)]
    bpp = 3 + (k // 3) % 2
    pad = (0, 20, 64)[k % 3]
    key = 0x51ED0000 + 977 * k
    m = np.eye(4, dtype=np.float32).reshape(-1)
    m[:12] = ((RC.uniform(12, key) - 0.5) * 2.0).astype(np.float32)
    m[3:12:4] = ((RC.uniform(3, key + 1) - 0.5) * (80.0 if k % 2 else 8.0)).astype(np.float32)
    it = make_intrinsics(w, h, 1, 1, 0, 0)
    stride = w * bpp + pad
    sc = make_stream_config(it, it, cam_to_world=m, color_bpp=bpp, color_stride=stride)
    n = w * h
    V = np.stack([(RC.uniform(n, key + 2 + a) - 0.5) * s for a, s in enumerate((6.0, 4.0, 8.0))], -1).astype(np.float32)
    V[(RC.uniform(n, key + 5) < 0.1)] = 0
    V[: n // 8] *= np.float32(30)
    b = n // 16
    V[n // 2:n // 2 + b, 2] = np.float32(1.5)                    # points exactly on the -c bounds
    V[n // 2 + b:n // 2 + 2 * b, 0] = np.float32(2.0)
    V[n // 2 + 2 * b:n // 2 + 3 * b, 0] = np.float32(-2.0)
    V[n // 2 + b:n // 2 + 3 * b, 2] = np.float32(0.75)
    T = np.stack([RC.uniform(n, key + 6 + a) * 1.4 - 0.2 for a in range(2)], -1).astype(np.float32)
    col = RC.S.synth_color(w, h, stream=k, bpp=bpp, stride=stride)
    return sc, V, T, col


def test_live_sweep_oracle_equals_the_compiled_reference(oracle):
    """About 20 more geometries and matrices, a few million points: oracle.pack == the live reference, dense and -c; the scalar
    variant == the non -m path; dense -t4 == -t1. Point counts that are not a multiple of 4 go through ref_pin.pack's padding."""
    need_live()
    total = 0
    for k in range(20):
        sc, V, T, col = _sweep_case(k)
        n = V.shape[0]
        want = R.pack_config(sc, V, T, col)
        d = first_diff(oracle.pack(sc, V, T, col), want)
        assert d is None, f"sweep {k} dense: {d}"
        assert np.array_equal(R.pack_config(sc, V, T, col, threads=4), want), f"sweep {k}: -t4 differs from -t1"
        d = first_diff(oracle.pack_scalar_variant(sc, V, T, col), R.pack_config(sc, V, T, col, simd=False))
        assert d is None, f"sweep {k} non -m: {d}"
        total += 2 * n
        if n % 4 == 0:
            d = first_diff(oracle.pack(sc, V, T, col, flags=CUT), R.pack_config(sc, V, T, col, cutoff=True))
            assert d is None, f"sweep {k} -c: {d}"
            total += n
        else:
            with pytest.raises(ValueError):
                R.pack_config(sc, V, T, col, cutoff=True)
    print(f"{total} points compared with the live reference")
    assert total > 3_000_000


# ---------------------------------------------------------------------------------------------------------------------
# GPU tier
# ---------------------------------------------------------------------------------------------------------------------
def _upload(ctx, arrays):
    ptrs = [ctx.device_malloc(max(a.nbytes, 16)) for a in arrays]
    for p, a in zip(ptrs, arrays):
        ctx.memcpy_h2d(p, np.ascontiguousarray(a))
    return ptrs


def _a2_host(ctx, sc, V, T, col):
    out, cnt = ctx.copy_pointcloud_xyzrgb_to_buffer(0, V, T, col)
    assert cnt == out.shape[0]
    return [out]


def _a2_device(ctx, sc, V, T, col):
    """pcs_copy_pointcloud_xyzrgb_to_buffer_device into a 16-byte aligned buffer and into one at +4 bytes, the reference's
    buffer + 2 shorts (another store path)."""
    n = V.shape[0]
    dv, dt, dcol = _upload(ctx, [V, T, col])
    outs = [ctx.device_malloc(n * 10 + 64) for _ in range(2)]
    d_cnt = ctx.device_malloc(8)
    res = []
    try:
        for i, skew in enumerate((0, 4)):
            ctx.copy_pointcloud_xyzrgb_to_buffer_device(0, dv, dt, n, dcol, outs[i] + skew, d_cnt + 4 * i)
        ctx.synchronize()
        cnt = np.empty(2, np.int32)
        ctx.memcpy_d2h(cnt, d_cnt)
        for i, skew in enumerate((0, 4)):
            assert 0 <= cnt[i] <= n
            got = np.empty(int(cnt[i]) * 5, np.int16)
            if got.size:
                ctx.memcpy_d2h(got, outs[i] + skew)
            res.append(got.reshape(-1, 5))
    finally:
        for p in [dv, dt, dcol, d_cnt] + outs:
            ctx.device_free(p)
    return res


def _a2_batched(ctx, sc, V, T, col):
    """pcs_copy_pointclouds_xyzrgb_to_buffer_device: the cloud three times in one call, the third at the +4 byte skew."""
    n = V.shape[0]
    dv, dt, dcol = _upload(ctx, [V, T, col])
    outs = [ctx.device_malloc(n * 10 + 64) for _ in range(3)]
    skews = (0, 0, 4)
    d_cnt = ctx.device_malloc(12)
    res = []
    try:
        ctx.copy_pointclouds_xyzrgb_to_buffer_device([(0, n, dv, dt, dcol, outs[i] + skews[i]) for i in range(3)], d_cnt)
        ctx.synchronize()
        cnt = np.empty(3, np.int32)
        ctx.memcpy_d2h(cnt, d_cnt)
        for i in range(3):
            assert 0 <= cnt[i] <= n
            got = np.empty(int(cnt[i]) * 5, np.int16)
            if got.size:
                ctx.memcpy_d2h(got, outs[i] + skews[i])
            res.append(got.reshape(-1, 5))
    finally:
        for p in [dv, dt, dcol, d_cnt] + outs:
            ctx.device_free(p)
    return res


A2_FORMS = {"host": _a2_host, "device": _a2_device, "batched": _a2_batched}


@pytest.mark.gpu
@pytest.mark.parametrize("against", ["fixture", "live"])
@pytest.mark.parametrize("form", list(A2_FORMS))
@pytest.mark.parametrize("mode", ["dense", "cut"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_a2_twin_is_the_reference(name, mode, form, against):
    """copy_pointcloud_xyzrgb_to_buffer (host, _device, batched _device) on every fixture case, dense and FLAG_CUTOFF |
    FLAG_CUTOFF_COMPAT: the padded and RGBA rasters, the wrapping matrices, and the special values (NaN, infinities, beyond 2^31:
    the lazy-convert redo path of v_cvt_i32_f32, see test_gpu_parity.test_lazy_convert_redo_path)."""
    live = None
    if against == "live":
        need_live()
        live = live_records(name, mode)
    sc, V, T, col = case_inputs(name)
    with PcsContext([sc], flags=CUT if mode == "cut" else 0) as ctx:
        results = A2_FORMS[form](ctx, sc, V, T, col)
    for i, got in enumerate(results):
        assert_is_reference(got, name, mode, f"a2 twin ({form} #{i})", live=live)


@pytest.mark.gpu
@pytest.mark.parametrize("against", ["fixture", "live"])
@pytest.mark.parametrize("mode", ["dense", "cut"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_a1_send_whole_buffer_is_the_reference(name, mode, against):
    """send_xyzrgb_pointcloud's whole buffer against the reference's: header slot, records, returned size, cleared prefix, untouched
    tail."""
    sc, V, T, col = case_inputs(name)
    e = MAN["cases"][name]
    r = e["readings"][mode]
    want = None
    if against == "live":
        need_live()
        want, wsize = R.send(V, T, col, sc.color.width, sc.color.height, sc.color_bpp, sc.color_stride, list(sc.cam_to_world),
                             cutoff=(mode == "cut"), prefill=PREFILL)
        assert wsize == r["size"]
    else:
        full = fixture_records(name)
        if full:
            want = RC.expected_buffer(full[mode], PREFILL, MAN["buf_size"], e["buffer_bytes"])
    buf = np.full((e["buffer_bytes"] + 1) // 2, PREFILL, np.uint16).view(np.int16)
    with PcsContext([sc], flags=CUT if mode == "cut" else 0) as ctx:
        size = ctx.send_xyzrgb_pointcloud(0, V, T, col, buf, write_header=False)
        assert size == r["size"]
        if want is not None:
            bad = np.nonzero(buf != want)[0]
            assert bad.size == 0, f"{bad.size} shorts differ from the reference's buffer, first at {bad[:8]}"
        assert RC.sha256(buf) == r["buffer_sha256"]
        keep = buf.copy()
        buf.view(np.uint16)[:] = PREFILL                      # the same call again, header on
        size2 = ctx.send_xyzrgb_pointcloud(0, V, T, col, buf, write_header=True)
    assert size2 == size and buf[:2].tobytes() == int(size).to_bytes(4, "little", signed=True)
    assert np.array_equal(buf[2:], keep[2:]) and not keep[:2].any()


def _fused_host(ctx, depth, color, n_sh):
    buf, counts, size = ctx.process_frames(depth, color, write_header=True)
    assert size == 10 * sum(counts) and buf[:2].tobytes() == int(size).to_bytes(4, "little", signed=True)
    return buf[2:2 + 5 * sum(counts)].reshape(-1, 5), counts


def _fused_device(ctx, depth, color, n_sh):
    """pcs_process_frames_device on 256-byte aligned rasters and payload (what the dense row-constant kernel wants)."""
    ptrs = _upload(ctx, list(depth) + list(color))
    dd, dc = ptrs[:len(depth)], ptrs[len(depth):]
    out = ctx.device_malloc(n_sh * 2 + 64)
    d_cnt = ctx.device_malloc(4 * (len(depth) + 1))        # per-stream counts, then their total
    try:
        ctx.process_frames_device(dd, dc, out, n_sh, d_cnt)
        ctx.synchronize()
        cnt = np.empty(len(depth) + 1, np.int32)
        ctx.memcpy_d2h(cnt, d_cnt)
        counts = [int(x) for x in cnt[:-1]]
        assert cnt[-1] == sum(counts) and all(c >= 0 for c in counts) and sum(counts) * 5 <= n_sh
        got = np.empty(sum(counts) * 5, np.int16)
        if got.size:
            ctx.memcpy_d2h(got, out)
        return got.reshape(-1, 5), counts
    finally:
        for p in ptrs + [out, d_cnt]:
            ctx.device_free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("against", ["fixture", "live"])
@pytest.mark.parametrize("api", ["host", "device"])
@pytest.mark.parametrize("policy", ["certified", "ieee"])
@pytest.mark.parametrize("mode", list(RC.FUSED_MODES))
@pytest.mark.parametrize("name", list(RC.FUSED))
def test_fused_pack_half_is_the_reference(oracle, name, mode, policy, api, against):
    """process_frames / process_frames_device against the REFERENCE's pack applied, stream by stream in camera order, to the points
    oracle.deproject gives: 1x64x48, 3x640x480, 8x1280x720 with each stream's own cam_to_world, and a pair whose second stream
    (t_y != 0) the row-constant certificate must refuse; certified fast math and FLAG_FORCE_IEEE; dense and -c compat.

    Deprojection itself stays pinned to the restatement only (it is librealsense's arithmetic, not the reference's). What this adds
    is that the transform, convert, colour-gather and compaction half of every fused kernel is held by reference bytes."""
    cfgs, depth, color = RC.build_fused(name)
    e = MAN["fused"][name]
    live = None
    if against == "live":
        need_live()
        vt = [oracle.deproject(sc, d) for sc, d in zip(cfgs, depth)]
        live = np.concatenate([R.pack_config(sc, v, t, c, cutoff=(mode == "cut")) for sc, (v, t), c in zip(cfgs, vt, color)])
    flags = (CUT if mode == "cut" else 0) | (FLAG_FORCE_IEEE if policy == "ieee" else 0)
    with PcsContext(cfgs, flags=flags) as ctx:
        math = [ctx.stream_math(s) for s in range(len(cfgs))]
        rowc = [ctx.stream_color_row_const(s) for s in range(len(cfgs))]
        if policy == "ieee":
            assert math == [0] * len(cfgs), math
        else:
            assert all(m > 0 for m in math), math                       # the synthetic rig certifies
            # CertRowConst: R = I and t_y = t_z = 0 certify; the tweaked stream must be refused
            assert rowc == ([True, False] if e["tweak"] == "ty" else [True] * len(cfgs)), rowc
        got, counts = (_fused_host if api == "host" else _fused_device)(ctx, depth, color, ctx.max_payload_shorts)
    assert counts == e["readings"][mode]["counts"]
    if live is None and "records_file" not in e and RC.sha256(got) != e["readings"][mode]["sha256"]:
        want, _ = oracle.process_frames(cfgs, depth, color, flags=CUT if mode == "cut" else 0)    # only to say where
        pytest.fail(f"{name}/{mode}: not the reference's records; against the oracle: {first_diff(got, want)}")
    assert_is_reference(got, name, mode, f"fused ({api}, {policy})", section="fused", live=live)
