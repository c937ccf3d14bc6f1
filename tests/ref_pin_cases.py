"""The case set of tests/golden/ref_pin/ (test infrastructure): inputs rebuilt from integers, and the misreadings of the
reference that the case set must be able to tell from the right reading.

Shared by tests/golden/make_ref_pin_golden.py, which runs the compiled reference (oracle/ref_pin.py) on these inputs and
writes the fixtures, and by tests/test_reference_pin.py, which rebuilds the same inputs where the reference does not exist.
Everything here is integer hashing (synthetic.hash32) followed by exact float conversions: no numpy.random, no libm.
"""
import hashlib
import json
import os

import numpy as np

from pointcloud_stitching_amd import synthetic as S
from pointcloud_stitching_amd.types import (TF_MAT, TRANSFORMS, make_intrinsics, make_stream_config)

import np_restatement as NP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIN_DIR = os.path.join(GOLD, "ref_pin")
MANIFEST = os.path.join(PIN_DIR, "manifest.json")

# name -> (colour width, height, bytes per pixel, row padding in bytes, matrix, kind, stored in full)
CASES = {
    "kat_appendix_b": (8, 4, 3, 0, "tf_mat", "kat", True),
    "g8x4":           (8, 4, 3, 0, "tf_mat", "geometry", True),
    "g64x48":         (64, 48, 3, 0, "tf_mat", "geometry", True),
    "g64x48_rgba":    (64, 48, 4, 0, "tf_mat", "geometry", True),
    "g68x48_padded":  (68, 48, 3, 20, "tf_mat", "geometry", True),
    "special_values": (64, 48, 3, 0, "tf_mat", "special", True),
    "identity_32x24": (32, 24, 3, 0, "identity", "geometry", True),
    "wrap_32x24":     (32, 24, 3, 0, "transform6_far", "geometry", True),
    "g640x480":       (640, 480, 3, 0, "tf_mat", "geometry", False),
    "g848x480":       (848, 480, 3, 0, "tf_mat", "geometry", False),
    "g1280x720":      (1280, 720, 3, 0, "tf_mat", "geometry", False),
}
# the reference's three readings of one input: `-m -t1` dense, `-c -m -t1`, and the non-`-m` loop (dense)
MODES = ("dense", "cut", "scalar")

SPECIALS = [float("nan"), float("inf"), float("-inf"), 3e6, -3e6, 2.2e9, 1e30, 32.767, -32.768, 32.7675, 65.536]


def matrix(name):
    if name == "tf_mat":
        return TF_MAT.copy()
    if name == "identity":
        return np.eye(4, dtype=np.float32).reshape(-1)
    if name == "transform6_far":
        # the surveyed transform[6] (the one with no zero in its rotation), moved far enough that every world coordinate
        # leaves int16's +-32.767 m: each short is the low half of a wider integer
        m = TRANSFORMS[6].copy()
        m[3], m[7], m[11] = np.float32(-41.973), np.float32(36.417), np.float32(-70.434)
        return m
    raise KeyError(name)


def uniform(n, key):
    """n doubles k / 2^24, k uniform over 0 .. 2^24 - 1, from the project's counter hash."""
    i = np.arange(n, dtype=np.uint32)
    h = S.hash32(i * np.uint32(2654435761) + np.uint32(key & 0xFFFFFFFF))
    return (h >> np.uint32(8)).astype(np.float64) / 16777216.0


def case_key(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def build_case(name):
    """-> (StreamConfig, vertices float32[n,3], texcoords float32[n,2], colour uint8[stride*h])."""
    w, h, bpp, pad, mat, kind, _ = CASES[name]
    stride = w * bpp + pad
    it = make_intrinsics(w, h, 1, 1, 0, 0)
    sc = make_stream_config(it, it, cam_to_world=matrix(mat), color_bpp=bpp, color_stride=stride)
    n = w * h
    key = case_key(name)
    if kind == "kat":
        with open(os.path.join(GOLD, "kat_appendix_b.json")) as f:
            k = json.load(f)
        V = np.array([v["vertex"] for v in k["vectors"]], np.float32)
        T = np.array([v["uv"] for v in k["vectors"]], np.float32)
        return sc, V, T, ((7 * np.arange(96) + 3) & 0xFF).astype(np.uint8)
    col = S.synth_color(w, h, stream=key % 251, bpp=bpp, stride=stride)
    # camera-frame points over x +-3 m, y +-2 m, z +-4 m: both sides of every `-c` bound, and of zero
    V = np.stack([(uniform(n, key + 1 + a) - 0.5) * s for a, s in enumerate((6.0, 4.0, 8.0))], -1).astype(np.float32)
    T = np.stack([uniform(n, key + 11 + a) * 1.4 - 0.2 for a in range(2)], -1).astype(np.float32)
    if kind == "special":
        sp = np.array(SPECIALS, np.float32)
        for a in range(3):
            V[a * sp.size:(a + 1) * sp.size, a] = sp
        T[:sp.size, 0] = sp
        T[sp.size:2 * sp.size, 1] = sp
        return sc, V, T, col
    V[(S.hash32(np.arange(n, dtype=np.uint32) + np.uint32(key)) % np.uint32(10)) == 0] = 0      # holes: 10 % zero vertices
    k = n // 8
    V[:k] *= np.float32(30)                                     # up to 90 .. 120 m: int16 wraps
    b = max(n // 16, 1)
    V[k:k + b, 2] = np.float32(1.5)                             # exactly on each `-c` bound
    V[k + b:k + 2 * b, 0] = np.float32(2.0)
    V[k + 2 * b:k + 3 * b, 0] = np.float32(-2.0)
    V[k + 2 * b:k + 3 * b, 2] = np.abs(V[k + 2 * b:k + 3 * b, 2]) * np.float32(0.25) + np.float32(0.125)   # and inside the z range
    V[k + b:k + 2 * b, 2] = np.abs(V[k + b:k + 2 * b, 2]) * np.float32(0.25) + np.float32(0.125)
    e = np.array([0, 1, -0.0, 0.5, (w - 0.5) / w, 0.49999997 / w, 1.4999999 / w, 0.5 / w, 1.5 / w], np.float32)
    e = e[:max(min(e.size, n // 2), 1)]
    T[n - e.size:, 0] = e                                       # pixel edges: x.4999 / x.5 and the raster's ends
    T[n - 2 * e.size:n - e.size, 1] = e
    return sc, V, T, col


def inputs_sha256(sc, V, T, col):
    h = hashlib.sha256()
    for a in (np.array(list(sc.cam_to_world), np.float32), V, T, col):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.array([sc.color.width, sc.color.height, sc.color_bpp, sc.color_stride], np.int32).tobytes())
    return h.hexdigest()


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def expected_buffer(records, prefill, buf_size, n_bytes):
    """What a1 leaves in a buffer of n_bytes prefilled with `prefill` shorts: BUF_SIZE bytes cleared, the records from byte 4 on
    (the 4-byte header slot stays clear: the reference fills it only when it sends), the rest untouched."""
    buf = np.full((n_bytes + 1) // 2, prefill, np.uint16).view(np.int16)
    buf[:min(buf_size // 2, buf.size)] = 0
    buf[2:2 + records.size] = records.reshape(-1)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# fused cases: depth rasters -> (the restatement's deprojection) -> the reference's pack, stream by stream
# ---------------------------------------------------------------------------------------------------------------------
# name -> (streams, width, height, tweak, stored in full)
FUSED = {
    "f1x64x48":           (1, 64, 48, None, True),
    "f3x640x480":         (3, 640, 480, None, False),
    "f8x1280x720":        (8, 1280, 720, None, False),
    "f2x640x480_ty":      (2, 640, 480, "ty", False),       # stream 1: t_y != 0, not row-constant
}
FUSED_MODES = ("dense", "cut")


def build_fused(name):
    """-> (configs, depth rasters, colour rasters): synthetic.synth_frame_set, stream s with the surveyed transform[s]."""
    n, w, h, tweak, _ = FUSED[name]
    cfgs, depth, color = S.synth_frame_set(n, w, h)
    if tweak == "ty":
        cfgs[1].depth_to_color.translation[1] = 0.0002
    return cfgs, depth, color


# ---------------------------------------------------------------------------------------------------------------------
# misreadings: each is np_restatement's arithmetic with one thing read differently
# ---------------------------------------------------------------------------------------------------------------------
DENSE_VARIANTS = ("mul_then_add", "fma_order_zyx", "fma_order_translation_last", "double_x1000", "round_to_nearest",
                  "saturate", "texcoord_without_half", "clamp_to_w_h", "stride_is_w_bpp", "g_b_swapped")
CUT_VARIANTS = ("mask_not_reversed", "z_hi_lt", "x_hi_lt", "x_lo_ge", "z_lo_ge")


def pack_variant_np(sc, V, T, color, variant=None):
    """np_restatement.pack_np with one misreading (None: none; then it equals pack_np)."""
    f32 = np.float32
    V = np.asarray(V, f32); T = np.asarray(T, f32)
    M = np.array(list(sc.cam_to_world), f32)
    W, H, bpp, stride = sc.color.width, sc.color.height, sc.color_bpp, sc.color_stride
    color = np.asarray(color, np.uint8).astype(np.int64)
    if variant == "stride_is_w_bpp":
        stride = W * bpp
    half = f32(0.0 if variant == "texcoord_without_half" else 0.5)
    hi_x, hi_y = (W, H) if variant == "clamp_to_w_h" else (W - 1, H - 1)
    if variant == "clamp_to_w_h":          # pixels one past the raster: give them bytes that are not the raster's
        color = np.concatenate([color, np.full(2 * sc.color_stride + 8, 0xA5, np.int64)])
    xi = np.clip(NP.cvtt(NP.fma32(T[:, 0], f32(W), half)), 0, hi_x)
    yi = np.clip(NP.cvtt(NP.fma32(T[:, 1], f32(H), half)), 0, hi_y)
    idx = xi * bpp + yi * stride
    out = np.zeros((V.shape[0], 5), np.int16)
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    with np.errstate(all="ignore"):
        for r in range(3):
            m0, m1, m2, t = M[4 * r:4 * r + 4]
            if variant == "mul_then_add":
                a = ((x * m0).astype(f32) + t).astype(f32)
                a = (a + (y * m1).astype(f32)).astype(f32)
                a = (a + (z * m2).astype(f32)).astype(f32)
            elif variant == "fma_order_zyx":
                a = NP.fma32(x, m0, NP.fma32(y, m1, NP.fma32(z, m2, t)))
            elif variant == "fma_order_translation_last":
                a = (NP.fma32(z, m2, NP.fma32(y, m1, (x * m0).astype(f32))) + t).astype(f32)
            else:
                a = NP.fma32(z, m2, NP.fma32(y, m1, NP.fma32(x, m0, t)))
            if variant == "double_x1000":
                s = a.astype(np.float64) * 1000.0
                ok = (s >= -2147483648.0) & (s < 2147483648.0)
                q = np.where(ok, np.trunc(np.where(ok, s, 0)).astype(np.int64), -2**31)
            else:
                a = (a * f32(1000.0)).astype(f32)
                if variant == "round_to_nearest":
                    ok = (a >= f32(-2147483648.0)) & (a < f32(2147483648.0))
                    q = np.where(ok, np.rint(np.where(ok, a, 0)).astype(np.int64), -2**31)
                else:
                    q = NP.cvtt(a)
            if variant == "saturate":
                q = np.clip(q, -32768, 32767)
            out[:, r] = (q & 0xFFFF).astype(np.uint16).view(np.int16)
    c0, c1, c2 = color[idx], color[idx + 1], color[idx + 2]
    if variant == "g_b_swapped":
        c1, c2 = c2, c1
    out[:, 3] = (c0 | (c1 << 8)).astype(np.uint16).view(np.int16)
    out[:, 4] = c2.astype(np.int16)
    return out


def keep_variant_np(V, variant=None):
    """np_restatement.cutoff_keep_np(compat) with one misreading of the `-c` test."""
    f32 = np.float32
    V = np.asarray(V, f32)
    if variant is None or variant == "mask_not_reversed":
        return NP.cutoff_keep_np(V, compat=variant is None)
    z, x = V[:, 2], V[:, 0]
    with np.errstate(all="ignore"):
        z_lo = (z >= f32(0)) if variant == "z_lo_ge" else (z > f32(0))
        z_hi = (z < f32(1.5)) if variant == "z_hi_lt" else (z <= f32(1.5))
        x_lo = (x >= f32(-2)) if variant == "x_lo_ge" else (x > f32(-2))
        x_hi = (x < f32(2)) if variant == "x_hi_lt" else (x <= f32(2))
    ok = z_lo & z_hi & x_lo & x_hi
    g = (ok.size // 4) * 4
    return np.concatenate([ok[:g].reshape(-1, 4)[:, ::-1].reshape(-1), ok[g:]])


def records_changed(got, want):
    """Records that differ between two record lists, position by position; a missing record counts as changed."""
    n = min(got.shape[0], want.shape[0])
    return int((got[:n] != want[:n]).any(axis=1).sum()) + max(got.shape[0], want.shape[0]) - n


def count_variant(variant, cases):
    """How many records of the case set `variant` changes. cases: name -> (sc, V, T, col, want_dense, want_cut).
    None = the dense reading unmodified, "cut:none" = the `-c` reading unmodified (both must give 0)."""
    total = 0
    for name, (sc, V, T, col, want_dense, want_cut) in cases.items():
        if variant is None or variant in DENSE_VARIANTS:
            total += records_changed(pack_variant_np(sc, V, T, col, variant), want_dense)
        elif V.shape[0] % 4 == 0:
            keep = keep_variant_np(V, None if variant == "cut:none" else variant)
            total += records_changed(pack_variant_np(sc, V[keep], T[keep], col), want_cut)
    return total
