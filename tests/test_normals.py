"""Surface normals on the GPU (pcs_estimate_normals_device, pcs_estimate_normals) against the restatement of DESIGN.md section 3
(tests/np_normals.py: brute-force neighbourhoods, the exact covariance in Python integers, numpy's eigh) over the clouds of
tests/plane_cases.py — validity equal and every short within one unit after aligning signs, the neighbour counts equal — with 0xA5
guard bytes in front of and behind d_normals and d_valid; the sign rules on the scene; equal records, two runs, two payload orders,
every 2-byte phase of the payload, the host form, a small call in a large call's workspace, one timing interval per launch, and
every refusal."""
import functools

import numpy as np
import pytest

import np_normals as NN
import plane_cases as PC
from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.api import PcsContext, PcsError
from pointcloud_stitching_amd.types import NORMAL_LAUNCHES, NormalParams

pytestmark = pytest.mark.gpu

GUARD = 64
N_MAX = 6161 + 64
CASES = {c[0]: c for c in PC.normal_cases()}
INVALID = -1


class Arena:
    """Device buffers shared by the tests of this module: a payload at any 2-byte phase, d_normals and d_valid between guard bytes."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.payload = ctx.device_malloc(64 + 10 * N_MAX + 64)
        self.normals = ctx.device_malloc(GUARD + 8 * N_MAX + GUARD)
        self.valid = ctx.device_malloc(GUARD + 4 + GUARD)
        assert all(p % 16 == 0 for p in (self.payload, self.normals, self.valid))

    def free(self):
        for p in (self.payload, self.normals, self.valid):
            self.ctx.device_free(p)

    def upload(self, payload, phase=4):
        if payload.shape[0]:
            self.ctx.memcpy_h2d(self.payload + phase, np.ascontiguousarray(payload))
        return self.payload + phase

    def paint(self, n):
        self.ctx.memcpy_h2d(self.normals, np.full(GUARD + 8 * n + GUARD, 0xA5, np.uint8))
        self.ctx.memcpy_h2d(self.valid, np.full(GUARD + 4 + GUARD, 0xA5, np.uint8))

    def read(self, n):
        """(normals bytes, valid bytes) with the guards checked."""
        a, b = np.empty(GUARD + 8 * n + GUARD, np.uint8), np.empty(GUARD + 4 + GUARD, np.uint8)
        self.ctx.memcpy_d2h(a, self.normals)
        self.ctx.memcpy_d2h(b, self.valid)
        assert (a[:GUARD] == 0xA5).all() and (a[GUARD + 8 * n:] == 0xA5).all(), "bytes around d_normals were written"
        assert (b[:GUARD] == 0xA5).all() and (b[GUARD + 4:] == 0xA5).all(), "bytes around d_valid were written"
        return a[GUARD:GUARD + 8 * n].copy(), b[GUARD:GUARD + 4].copy()

    def run(self, payload, params, viewpoint=None, phase=4, valid=True):
        """-> int16 [n, 4]; the valid count is checked against the shorts."""
        n = payload.shape[0]
        d_p = self.upload(payload, phase)
        self.paint(n)
        self.ctx.estimate_normals_device(d_p if n else 0, n, NormalParams.make(*params, viewpoint_mm=viewpoint), self.normals + GUARD if n else 0,
                                         self.valid + GUARD if valid else 0)
        self.ctx.synchronize()
        a, b = self.read(n)
        got = a.view(np.int16).reshape(n, 4)
        if valid:
            assert int(b.view(np.int32)[0]) == int((got[:, 3] != 0).sum())
        else:
            assert (b == 0xA5).all(), "d_valid was not given and was written"
        return got


@pytest.fixture(scope="module")
def ctx():
    cfgs, _, _ = S.synth_frame_set(1, 64, 48, single=True)
    with PcsContext(cfgs) as c:
        yield c


@pytest.fixture(scope="module")
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.free()


@functools.lru_cache(maxsize=None)
def reference(name, viewpoint=None):
    _, payload, (radius, min_nb, flat) = CASES[name]
    return NN.normals_np(payload, radius, min_nb, flat, viewpoint)


@pytest.mark.parametrize("name", list(CASES))
def test_device_form_matches_the_restatement(arena, name):
    _, payload, params = CASES[name]
    for phase in (4, 0):                                   # buffer + 2 shorts; 16-byte aligned
        got = arena.run(payload, params, phase=phase)
        compared = NN.compare(got, reference(name), name)
    print(f"{name}: n {payload.shape[0]}, valid {int((got[:, 3] != 0).sum())}, compared {compared}")
    again = arena.run(payload, params, valid=False)
    assert again.tobytes() == got.tobytes()


def test_an_empty_payload_launches_nothing_and_writes_a_zero_count(arena):
    ctx = arena.ctx
    ctx.kernel_timing(True)
    try:
        ctx.kernel_times_ms()
        got = arena.run(CASES["size63"][1][:0], (50, 5, 0))
        assert got.shape == (0, 4)
        assert ctx.kernel_times_ms().shape[0] == 0
    finally:
        ctx.kernel_timing(False)


def test_the_sign_rules_on_the_scene(arena):
    _, payload, params = CASES["scene"]
    q = payload[:, :3].astype(np.int64)
    got = arena.run(payload, params, viewpoint=PC.SCENE_CENTRE)
    ok = got[:, 3] != 0
    assert ok.sum() > 1000
    towards = (got[ok, :3].astype(np.int64) * (np.asarray(PC.SCENE_CENTRE) - q[ok])).sum(axis=1)
    assert (towards > 0).all()
    NN.compare(got, reference("scene", PC.SCENE_CENTRE), "scene towards its centre")
    # without a viewpoint: the component of largest magnitude is positive, checked where it leads by more than 2
    for name in ("scene", "tilted", "size6161"):
        _, payload, params = CASES[name]
        got = arena.run(payload, params)
        g = got[got[:, 3] != 0, :3].astype(np.int64)
        a = np.sort(np.abs(g), axis=1)
        clear = a[:, 2] - a[:, 1] > 2
        lead = g[np.arange(g.shape[0]), np.abs(g).argmax(axis=1)]
        assert clear.sum() > 0 and (lead[clear] > 0).all(), name


def test_equal_records_two_runs_and_two_orders(arena):
    for name in ("size2049", "scene"):
        _, payload, params = CASES[name]
        doubled = np.concatenate([payload, payload[::3]])
        n = payload.shape[0]
        got = arena.run(doubled, params)
        assert (got[n:] == got[:n:3]).all(), name                     # equal records get equal shorts
        assert arena.run(doubled, params).tobytes() == got.tobytes(), name
        order = np.random.default_rng(4).permutation(doubled.shape[0])
        again = arena.run(np.ascontiguousarray(doubled[order]), params)
        assert (again == got[order]).all(), name


def test_every_phase_of_the_payload(arena):
    _, payload, params = CASES["size257"]
    want = arena.run(payload, params)
    assert (want[:, 3] != 0).any()
    for phase in range(0, 16, 2):
        assert arena.run(payload, params, phase=phase).tobytes() == want.tobytes(), phase


def test_host_form_agrees_with_the_device_form(arena):
    for name in ("size2049", "size1", "line", "grid_y", "int16_low_end"):
        _, payload, params = CASES[name]
        want = arena.run(payload, params)
        got, valid = arena.ctx.estimate_normals(payload, *params, want_valid=True)
        assert got.tobytes() == want.tobytes() and valid == int((want[:, 3] != 0).sum()), name
    _, payload, params = CASES["scene"]
    want = arena.run(payload, params, viewpoint=PC.SCENE_CENTRE)
    assert arena.ctx.estimate_normals(payload, *params, viewpoint_mm=PC.SCENE_CENTRE).tobytes() == want.tobytes()
    got, valid = arena.ctx.estimate_normals(payload[:0], *params, want_valid=True)
    assert got.shape == (0, 4) and valid == 0


def test_small_call_after_a_large_one(arena):
    """The workspace a large call left behind is larger than the small call's carve: every piece still lies where its reader looks."""
    _, payload, params = CASES["size6161"]
    NN.compare(arena.run(payload, params), reference("size6161"), "size6161")
    for name in ("size65", "grid_x", "size2049"):
        _, payload, params = CASES[name]
        NN.compare(arena.run(payload, params), reference(name), name)


def test_one_timing_interval_per_launch(arena):
    ctx = arena.ctx
    ctx.kernel_timing(True)
    try:
        ctx.kernel_times_ms()
        for name in ("size257", "size1"):
            _, payload, params = CASES[name]
            arena.run(payload, params)
            ms = ctx.kernel_times_ms()
            assert ms.shape[0] == NORMAL_LAUNCHES and (ms >= 0).all(), (name, ms)
    finally:
        ctx.kernel_timing(False)


def test_every_refusal_leaves_the_outputs_untouched(arena):
    ctx = arena.ctx
    _, payload, params = CASES["size257"]
    n = payload.shape[0]
    d_p = arena.upload(payload)
    d_n, d_v = arena.normals + GUARD, arena.valid + GUARD
    ok = NormalParams.make(*params)
    too_many = (2 ** 31 - 1) // 10 + 1

    def with_(**kw):
        base = dict(radius_mm=params[0], min_neighbors=params[1], flatness=params[2])
        base.update(kw)
        return NormalParams.make(**base)
    odd_viewpoint = NormalParams.make(*params)
    odd_viewpoint.use_viewpoint = 2
    bad = [
        ((d_p, n, with_(radius_mm=0), d_n, d_v), "radius_mm"),
        ((d_p, n, with_(radius_mm=1001), d_n, d_v), "radius_mm"),
        ((d_p, n, with_(min_neighbors=2), d_n, d_v), "min_neighbors"),
        ((d_p, n, with_(min_neighbors=32768), d_n, d_v), "min_neighbors"),
        ((d_p, n, with_(flatness=-1), d_n, d_v), "flatness"),
        ((d_p, n, with_(flatness=1001), d_n, d_v), "flatness"),
        ((d_p, n, with_(reserved=1), d_n, d_v), "reserved"),
        ((d_p, n, odd_viewpoint, d_n, d_v), "use_viewpoint"),
        ((d_p, n, None, d_n, d_v), "params is NULL"),
        ((d_p, -1, ok, d_n, d_v), "n_points"),
        ((d_p, too_many, ok, d_n, d_v), "n_points"),
        ((0, n, ok, d_n, d_v), "d_payload is NULL"),
        ((d_p, n, ok, 0, d_v), "d_normals is NULL"),
        ((d_p + 1, n, ok, d_n, d_v), "d_payload is not 2-byte aligned"),
        ((d_p, n, ok, d_n + 4, d_v), "d_normals is not 8-byte aligned"),
        ((d_p, n, ok, d_n + 2, d_v), "d_normals is not 8-byte aligned"),
        ((d_p, n, ok, d_n, d_v + 2), "d_valid is not 4-byte aligned"),
        ((d_p, n, ok, d_p + 4, d_v), "d_normals overlaps d_payload"),
        ((d_p, n, ok, d_p + 10 * n // 8 * 8 - 4, d_v), "d_normals overlaps d_payload"),
        ((d_p, n, ok, d_n, d_p + 12), "d_valid overlaps"),
        ((d_p, n, ok, d_n, d_n + 8 * n - 4), "d_valid overlaps"),
    ]
    before = np.empty(10 * n, np.uint8)
    ctx.memcpy_d2h(before, d_p)
    for args, text in bad:
        arena.paint(n)
        with pytest.raises(PcsError) as e:
            ctx.estimate_normals_device(*args)
        assert e.value.status == INVALID and text in str(e.value), (text, str(e.value))
        ctx.synchronize()
        a, b = arena.read(n)
        assert (a == 0xA5).all() and (b == 0xA5).all(), text
    after = np.empty(10 * n, np.uint8)
    ctx.memcpy_d2h(after, d_p)
    assert (after == before).all()
    with pytest.raises(PcsError) as e:
        ctx.estimate_normals(payload, 0, 5)
    assert e.value.status == INVALID and "radius_mm" in str(e.value)
