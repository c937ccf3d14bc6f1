"""The case table of the lens-distortion tests (tests/test_distortion_cpu.py, tests/test_distortion.py): plain data and builders over
make_intrinsics / make_stream_config. Every case carries its undistorted twin (the same rig with PCS_DISTORTION_NONE), so a test can
show that the case tells a lens from no lens. Nothing here touches a device; the device helpers at the end take a context."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.types import (FLAG_TEXCOORD_HALF_PIXEL, HEADER_SHORTS, TRANSFORMS, StreamConfig,
                                            make_intrinsics, make_stream_config)

TILE = 2048                                             # points per tile of the fused kernels
D_COEFFS = [0.08, -0.03, 0.001, -0.002, 0.01]           # the depth and colour sets of test_gpu_parity.distorted_config
C_COEFFS = [-0.05, 0.06, 0.0005, -0.0007, -0.02]
D_STRONG = [-0.3, 0.08, 0.002, -0.003, -0.01]           # barrel on the depth side, pincushion on the colour side; finite everywhere
C_STRONG = [0.3, -0.05, -0.002, 0.001, 0.01]
# one coefficient alone, large enough to move a twentieth of the records (asserted on the CPU; tangential terms of a real D400 are
# a tenth of these, which would move too few records to see a lost coefficient)
D_SINGLE = [0.08, 0.2, 0.01, 0.01, 0.3]
C_SINGLE = [-0.05, 0.1, 0.01, 0.01, -0.1]
T_D2C = (0.0147, 0.0003, -0.0002)


def _rodrigues(axis, ang):
    ax = np.asarray(axis, float)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rm = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    return list(Rm.T.reshape(-1))                        # column-major


ROTATIONS = {
    "ident": [1, 0, 0, 0, 1, 0, 0, 0, 1],                # colour-only distortion: certified with the identity shortcut
    "rot": _rodrigues((0.3, 1.0, 0.2), 0.015),           # ... certified without it
    "roll": [np.cos(0.02), np.sin(0.02), 0, -np.sin(0.02), np.cos(0.02), 0, 0, 0, 1],      # distorted_config's
}


def rig(w, h, cw, ch, dmodel=0, dk=None, cmodel=0, ck=None, rot="roll", bpp=3, stride=None, world=3, f_share=0.7,
        c_f_share=0.72, depth_scale=0.001) -> StreamConfig:
    """distorted_config's geometry (test_gpu_parity.py) with the models, the coefficients, the rotation and the lens as arguments."""
    di = make_intrinsics(w, h, f_share * w, (f_share + 0.01) * w, w / 2 + 1.3, h / 2 - 2.2, model=dmodel, coeffs=dk)
    ci = make_intrinsics(cw, ch, c_f_share * cw, c_f_share * cw, cw / 2 - 3.1, ch / 2 + 1.7, model=cmodel, coeffs=ck)
    return make_stream_config(di, ci, cam_to_world=TRANSFORMS[world], rotation=ROTATIONS[rot], translation=T_D2C,
                              depth_scale=depth_scale, color_bpp=bpp, color_stride=stride)


def zero_tile_depth(w, h, stream):
    d = S.synth_depth(w, h, stream).copy()
    d.reshape(-1)[TILE:2 * TILE] = 0                     # the whole second tile
    return d


def random_depth(w, h, stream):
    d = S.synth_depth(w, h, stream, mode="random").copy()
    d.reshape(-1)[[3, 11, w + 5, w * h - 1]] = [0, 1, 65535, 65535]
    return d


TINY_DEPTH = np.array([[0, 1500, 65535, 1, 2000, 2500, 900, 3000]], np.uint16)       # (the synthetic scene's hole covers all of 8 x 1)


@dataclass
class Case:
    name: str
    sc: StreamConfig
    twin: StreamConfig                                   # the same rig without a lens
    depth: np.ndarray
    color: np.ndarray
    ddist: bool
    cdist: bool
    rot: str
    min_changed: float = 0.25                            # share of the valid records that must differ from the twin's
    identity: bool = False                               # a model with all-zero coefficients: the twin's bits
    single: Optional[tuple] = None                       # ("depth" | "colour", slot) for the one-coefficient cases
    conditions: bool = True                              # the inside / changed conditions apply (not to 8 x 1: eight pixels)
    _memo: dict = field(default_factory=dict, repr=False)


def _case(name, shape=(104, 40), cshape=(136, 72), dmodel=0, dk=None, cmodel=0, ck=None, rot="roll", bpp=3, stride=None,
          raster="scene", stream=2, **kw):
    w, h = shape
    cw, ch = cshape
    sc = rig(w, h, cw, ch, dmodel, dk, cmodel, ck, rot, bpp, stride)
    twin = rig(w, h, cw, ch, 0, None, 0, None, rot, bpp, stride)
    depth = {"scene": lambda: S.synth_depth(w, h, stream), "random": lambda: random_depth(w, h, stream),
             "zero_tile": lambda: zero_tile_depth(w, h, stream), "tiny": lambda: TINY_DEPTH.copy()}[raster]()
    color = S.synth_color(cw, ch, stream, bpp=bpp, stride=sc.color_stride)
    nz = lambda k: k is not None and any(float(x) != 0.0 for x in k)
    return Case(name, sc, twin, depth, color, bool(dmodel) and nz(dk), bool(cmodel) and nz(ck), rot, **kw)


def _one_hot(values, slot):
    return [values[k] if k == slot else 0.0 for k in range(5)]


def build_cases():
    c = []
    for rot in ("roll", "ident", "rot"):                 # the four model combinations under every depth->colour rotation
        c.append(_case(f"depth_only_{rot}", dmodel=2, dk=D_COEFFS, rot=rot))
        c.append(_case(f"colour1_{rot}", cmodel=1, ck=C_COEFFS, rot=rot))
        c.append(_case(f"colour2_{rot}", cmodel=2, ck=C_COEFFS, rot=rot))
        c.append(_case(f"both_{rot}", dmodel=2, dk=D_COEFFS, cmodel=1, ck=C_COEFFS, rot=rot))
    for k in range(5):                                   # one coefficient alone: the split coefficient quads, slot by slot
        c.append(_case(f"depth_k{k}_alone", dmodel=2, dk=_one_hot(D_SINGLE, k), min_changed=0.05, single=("depth", k)))
    for k in range(5):
        c.append(_case(f"colour_k{k}_alone", cmodel=1 + k % 2, ck=_one_hot(C_SINGLE, k), rot="ident", min_changed=0.05,
                       single=("colour", k)))
    for m in (1, 2, 3, 4):                               # a model without coefficients is no lens
        c.append(_case(f"depth_model{m}_zero", dmodel=m, dk=[0.0] * 5, identity=True))
        c.append(_case(f"colour_model{m}_zero", cmodel=m, ck=[0.0, -0.0, 0.0, 0.0, -0.0], identity=True))
    c.append(_case("strong", dmodel=2, dk=D_STRONG, cmodel=2, ck=C_STRONG))
    # shapes: W % 8 != 0 (per-pixel path, two tiles), eight pixels, four bytes per colour pixel in a padded row, colour raster = depth's
    c.append(_case("both_ragged", shape=(100, 37), dmodel=2, dk=D_COEFFS, cmodel=1, ck=C_COEFFS))
    c.append(_case("both_tiny", shape=(8, 1), dmodel=2, dk=D_STRONG, cmodel=2, ck=C_STRONG, raster="tiny", conditions=False))
    c.append(_case("both_rgba_padded", dmodel=2, dk=D_COEFFS, cmodel=2, ck=C_COEFFS, bpp=4, stride=136 * 4 + 12))
    c.append(_case("both_same_raster", cshape=(104, 40), dmodel=2, dk=D_COEFFS, cmodel=1, ck=C_COEFFS))
    # depth rasters: every Z16 value incl. 0, 1 and 65 535; a whole tile of zeros
    c.append(_case("both_random", dmodel=2, dk=D_COEFFS, cmodel=1, ck=C_COEFFS, raster="random"))
    c.append(_case("both_zero_tile", dmodel=2, dk=D_COEFFS, cmodel=1, ck=C_COEFFS, raster="zero_tile"))
    c.append(_case("depth_only_ragged_random", shape=(100, 37), dmodel=2, dk=D_COEFFS, raster="random"))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
# `-c` where the cut depends on the lens: fx = 0.3 W puts |x| = z |mx| beyond 2 m inside the 1.5 m range, and the depth scale
# puts about half of the scene beyond 1.5 m. The narrow twin (fx = 0.4 W: 1.5 max|mx| < 2) is a stream whose count pass could
# take the verdict from the Z16 word alone if it had no lens; with this lens the corner rays leave |x| <= 2, so it may not.
# ---------------------------------------------------------------------------------------------------------------------
CUT_SCALE = 0.0006
CUT_COEFFS = [0.12, 0.02, 0.002, -0.002, 0.0]


def _cut_case(name, f_share):
    w, h, cw, ch = 104, 40, 136, 72
    sc = rig(w, h, cw, ch, 2, CUT_COEFFS, 0, None, "roll", f_share=f_share, c_f_share=f_share, depth_scale=CUT_SCALE)
    twin = rig(w, h, cw, ch, 0, None, 0, None, "roll", f_share=f_share, c_f_share=f_share, depth_scale=CUT_SCALE)
    depth = S.synth_depth(w, 4 * h, 5)[:h].copy()        # the rows above the scene's solid hole: every tile holds valid pixels
    return Case(name, sc, twin, depth, S.synth_color(cw, ch, 5), True, False, "roll", min_changed=0.25)


CUT_WIDE = _cut_case("cut_wide", 0.3)
CUT_NARROW = _cut_case("cut_narrow", 0.4)


# ---------------------------------------------------------------------------------------------------------------------
# frame-sets
# ---------------------------------------------------------------------------------------------------------------------
def _stream(shape, cshape, stream, raster="scene", **kw):
    c = _case(f"s{stream}", shape=shape, cshape=cshape, stream=stream, raster=raster, **kw)
    return c.sc, c.depth, c.color


def mixed_frame_set(ragged=False, order=(0, 1, 2, 3)):
    """[depth-only, colour model 2, no lens, both], every stream another raster shape and another colour raster; `order` permutes it.
    Aligned: every width and point count a multiple of 8 (the dense launch). Ragged: the last stream is 100 x 37 (the general path)."""
    streams = [
        _stream((104, 40), (136, 72), 0, dmodel=2, dk=D_COEFFS, rot="roll"),
        _stream((64, 24), (100, 75), 1, cmodel=2, ck=C_COEFFS, rot="ident", bpp=4, stride=100 * 4 + 12),
        _stream((128, 16), (128, 16), 2, rot="ident"),                                       # exactly one tile
        _stream((100, 37) if ragged else (72, 56), (136, 72), 3, raster="random" if ragged else "scene",
                dmodel=2, dk=D_STRONG, cmodel=1, ck=C_COEFFS, rot="rot"),
    ]
    for i, (sc, _, _) in enumerate(streams):             # every stream its own extrinsic
        for k in range(16):
            sc.cam_to_world[k] = float(TRANSFORMS[(2 * i + 1) % 8][k])
    streams = [streams[i] for i in order]
    return [s[0] for s in streams], [s[1] for s in streams], [s[2] for s in streams]


def cut_frame_set():
    """The mixed frame-set with part of every scene inside 1.5 m, then the wide-lens `-c` case and its narrow twin."""
    cfgs, depth, color = mixed_frame_set()
    depth = [d.copy() for d in depth]
    for d in depth:
        d[d.shape[0] // 4:d.shape[0] // 2, :] //= 4
    for c in (CUT_WIDE, CUT_NARROW):
        cfgs.append(c.sc); depth.append(c.depth); color.append(c.color)
    return cfgs, depth, color


# ---------------------------------------------------------------------------------------------------------------------
# CPU helpers shared by both tiers
# ---------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, np.float32).view(np.uint32)
    nan_a = (a & 0x7FFFFFFF) > 0x7F800000
    nan_b = (b & 0x7FFFFFFF) > 0x7F800000
    return a.shape == b.shape and bool(((a == b) | (nan_a & nan_b)).all())


def records_differ(a, b):
    a, b = np.asarray(a).reshape(-1, 5), np.asarray(b).reshape(-1, 5)
    assert a.shape == b.shape
    return (a != b).any(axis=1)


def oracle_deproject(oracle, case, flags=0):
    key = ("deproject", flags & FLAG_TEXCOORD_HALF_PIXEL)
    if key not in case._memo:
        case._memo[key] = oracle.deproject(case.sc, case.depth, flags & FLAG_TEXCOORD_HALF_PIXEL)
    return case._memo[key]


def oracle_records(oracle, case, twin=False):
    """The dense packed records of the case (or of its twin), computed once."""
    key = ("records", twin)
    if key not in case._memo:
        case._memo[key] = oracle.process_frames([case.twin if twin else case.sc], [case.depth], [case.color])[0]
    return case._memo[key]


def first_diff(got, want):
    got, want = np.asarray(got).reshape(-1, 5), np.asarray(want).reshape(-1, 5)
    if got.shape != want.shape:
        return f"shape {got.shape} vs {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return None
    return f"{bad.size} of {want.shape[0]} records differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def assert_same(got, want, what=""):
    d = first_diff(got, want)
    assert d is None, f"{what}: {d}" if what else d


# ---------------------------------------------------------------------------------------------------------------------
# device helpers (a context is handed in; nothing here imports the library)
# ---------------------------------------------------------------------------------------------------------------------
def host_run(ctx, depth, color):
    buf, counts, size = ctx.process_frames(depth, color, write_header=True)
    assert size == 10 * sum(counts)
    assert int.from_bytes(buf[:2].tobytes(), "little", signed=True) == size
    return buf[HEADER_SHORTS:HEADER_SHORTS + 5 * sum(counts)].reshape(-1, 5), counts


class Dev:
    """A frame-set's rasters on the device (the depth rasters `depth_skew` bytes off their allocation), a payload and a counts buffer."""

    def __init__(self, ctx, depth, color, depth_skew=0):
        self.ctx = ctx
        n = len(depth)
        self._d = [ctx.device_malloc(np.asarray(d).nbytes + 32) for d in depth]
        self.dd = [p + depth_skew for p in self._d]
        self.dc = [ctx.device_malloc(max(np.asarray(c).nbytes, 16)) for c in color]
        for p, a in zip(self.dd + self.dc, list(depth) + list(color)):
            ctx.memcpy_h2d(p, np.ascontiguousarray(a))
        self.shorts = ctx.max_payload_shorts
        self.out = ctx.device_malloc(self.shorts * 2 + 64)
        self.cnt = ctx.device_malloc(4 * (n + 1))
        self.n = n

    def run(self, skew=0):
        self.ctx.process_frames_device(self.dd, self.dc, self.out + skew, self.shorts, self.cnt)

    def result(self, skew=0):
        self.ctx.synchronize()
        c = np.empty(self.n + 1, np.int32)
        self.ctx.memcpy_d2h(c, self.cnt)
        assert int(c[-1]) == int(c[:-1].sum())
        got = np.empty(5 * int(c[-1]), np.int16)
        if got.size:
            self.ctx.memcpy_d2h(got, self.out + skew)
        return got.reshape(-1, 5), [int(x) for x in c[:-1]]

    def free(self):
        for p in self._d + self.dc + [self.out, self.cnt]:
            self.ctx.device_free(p)
