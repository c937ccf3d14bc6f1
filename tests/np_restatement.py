"""A second, independent restatement of the hot-path arithmetic in numpy (test infrastructure).

Its purpose is to cross-check oracle/pcs_oracle.c: two restatements written separately, in
different languages, that must agree bit for bit. float32 FMA does not exist in numpy, so it is
emulated exactly: the product of two float32 is exact in float64; the sum with the addend is
rounded to ODD in float64 (via TwoSum), and rounding that to float32 is then correctly rounded.
"""
import numpy as np


def fma32(a, b, c):
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = a * b                      # exact: 24 + 24 bits
        s = p + c
        # TwoSum error term
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s) & np.isfinite(e) & (e != 0)
        bits = s.view(np.int64).copy()
        even = (bits & 1) == 0
        # round to odd: if inexact and the float64 result is even, move one ulp toward the true value
        toward_up = (e > 0)
        pos = s > 0
        step = np.where(toward_up == pos, 1, -1)
        adj = fin & even
        bits = np.where(adj, bits + step, bits)
        s_odd = bits.view(np.float64)
        # s == 0 with e != 0 cannot happen for inexact sums of this magnitude; keep s as is otherwise
        return np.where(adj, s_odd, s).astype(np.float32)


def cvtt(f):
    f = np.asarray(f, np.float32)
    with np.errstate(all="ignore"):
        ok = (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
        return np.where(ok, np.trunc(np.where(ok, f, 0)).astype(np.int64), -2**31)


def pack_np(sc, V, T, color):
    V = np.asarray(V, np.float32); T = np.asarray(T, np.float32)
    M = np.array(list(sc.cam_to_world), np.float32)
    W, H = sc.color.width, sc.color.height
    xi = np.clip(cvtt(fma32(T[:, 0], np.float32(W), np.float32(0.5))), 0, W - 1)
    yi = np.clip(cvtt(fma32(T[:, 1], np.float32(H), np.float32(0.5))), 0, H - 1)
    idx = xi * sc.color_bpp + yi * sc.color_stride
    out = np.zeros((V.shape[0], 5), np.int16)
    for r in range(3):
        a = fma32(V[:, 0], M[4 * r], M[4 * r + 3])
        a = fma32(V[:, 1], M[4 * r + 1], a)
        a = fma32(V[:, 2], M[4 * r + 2], a)
        with np.errstate(all="ignore"):
            a = (a * np.float32(1000.0)).astype(np.float32)
        out[:, r] = (cvtt(a) & 0xFFFF).astype(np.uint16).view(np.int16)
    color = np.asarray(color, np.uint8).astype(np.int64)
    out[:, 3] = (color[idx] | (color[idx + 1] << 8)).astype(np.uint16).view(np.int16)
    out[:, 4] = color[idx + 2].astype(np.int16)
    return out


def cutoff_keep_np(V, compat=True):
    """The `-c` predicate on camera-frame z and x: 0 < z <= 1.5 and -2 < x <= 2 (NaN fails every comparison). With compat, as the
    `-m` path applies it: inside each aligned group of four, point k is kept or dropped by the verdict on point 3 - k."""
    V = np.asarray(V, np.float32)
    with np.errstate(all="ignore"):
        ok = (V[:, 2] > np.float32(0)) & (V[:, 2] <= np.float32(1.5)) & (V[:, 0] > np.float32(-2)) & (V[:, 0] <= np.float32(2))
    if compat:
        g = (ok.size // 4) * 4
        ok = np.concatenate([ok[:g].reshape(-1, 4)[:, ::-1].reshape(-1), ok[g:]])
    return ok


MISREADINGS = ("swap_k2_k3", "opencv_order", "no_factor_2", "other_axis", "colour_no_prescale", "colour_r2_after",
               "depth_modified_form", "radial_division", "depth_after_z")


def distortion_active(intr):
    """A model with all-zero coefficients is inactive (-0.0 is zero, a NaN is not)."""
    return int(intr.model) != 0 and any(np.float32(k) != np.float32(0) for k in intr.coeffs)


def _deproject(T, sc, depth, half_pixel, misreading):
    """DESIGN.md section 3 in the number type T, every operation one numpy operation on T, in the stated association. With T = float32
    each of them is rounded once: the exact emulation of a build with no contraction. With T = float64 it is the plain model.
    `misreading` (one of MISREADINGS, test use only) swaps in one plausible wrong reading of the published formula."""
    assert misreading is None or misreading in MISREADINGS
    mis = lambda name: misreading == name
    di, ci = sc.depth, sc.color
    W, H = di.width, di.height
    one, two = T(1), T(2)

    def coeffs(intr):
        k = [T(np.float32(c)) for c in intr.coeffs]
        if mis("swap_k2_k3"):
            k[2], k[3] = k[3], k[2]
        if mis("opencv_order"):              # read as k1 k2 k3 p1 p2
            k = [k[0], k[1], k[3], k[4], k[2]]
        return k

    def radial(k, r2):                       # 1 + k0*r2 + (k1*r2)*r2 + ((k4*r2)*r2)*r2, left to right
        return ((one + k[0] * r2) + (k[1] * r2) * r2) + ((k[4] * r2) * r2) * r2

    def tangential(a, kA, kB, x, y, r2, axis, other):        # a + ((2*kA)*x)*y + kB*(r2 + (2*axis)*axis)
        if mis("other_axis"):
            axis = other
        first = (kA * x) * y if mis("no_factor_2") else ((two * kA) * x) * y
        return (a + first) + kB * (r2 + (two * axis) * axis)

    def scaled(a, f):
        return a / f if mis("radial_division") else a * f

    def modified_form(k, x, y, r2_after=False):              # the colour branch: scale by f first, keep the r2 of the unscaled point
        r2 = x * x + y * y
        f = radial(k, r2)
        x, y = scaled(x, f), scaled(y, f)
        if r2_after:
            r2 = x * x + y * y
        return tangential(x, k[2], k[3], x, y, r2, x, y), tangential(y, k[3], k[2], x, y, r2, y, x)

    def inverse_form(k, x, y):                               # the depth branch: tangential terms of the unscaled point
        r2 = x * x + y * y
        f = radial(k, r2)
        return (tangential(scaled(x, f), k[2], k[3], x, y, r2, x, y),
                tangential(scaled(y, f), k[3], k[2], x, y, r2, y, x))

    d = np.asarray(depth, np.uint16).reshape(H, W)
    with np.errstate(all="ignore"):
        z = T(np.float32(sc.depth_scale)) * d.astype(T)
        mx = np.broadcast_to(((np.arange(W).astype(T) - T(di.ppx)) / T(di.fx))[None, :], (H, W))
        my = np.broadcast_to(((np.arange(H).astype(T) - T(di.ppy)) / T(di.fy))[:, None], (H, W))
        ddist = distortion_active(di)
        if ddist and not mis("depth_after_z"):
            mx, my = (modified_form if mis("depth_modified_form") else inverse_form)(coeffs(di), mx, my)
        X = z * mx; Y = z * my; Z = z
        if ddist and mis("depth_after_z"):
            X, Y = inverse_form(coeffs(di), X, Y)
        R = [T(np.float32(x)) for x in sc.depth_to_color.rotation]; t = [T(np.float32(x)) for x in sc.depth_to_color.translation]
        def row(i):
            return ((R[i] * X + R[i + 3] * Y) + R[i + 6] * Z) + t[i]
        P0, P1, P2 = row(0), row(1), row(2)
        x = P0 / P2; y = P1 / P2
        if distortion_active(ci):
            if mis("colour_no_prescale"):
                x, y = inverse_form(coeffs(ci), x, y)
            else:
                x, y = modified_form(coeffs(ci), x, y, r2_after=mis("colour_r2_after"))
        px = x * T(ci.fx) + T(ci.ppx)
        py = y * T(ci.fy) + T(ci.ppy)
        if half_pixel:                      # PCS_FLAG_TEXCOORD_HALF_PIXEL: older librealsense pixel_to_texcoord
            px = px + T(0.5); py = py + T(0.5)
        u = px / T(ci.width); v = py / T(ci.height)
    valid = Z != 0
    u = np.where(valid, u, T(0)); v = np.where(valid, v, T(0))
    vtx = np.stack([X, Y, Z], -1).reshape(-1, 3)
    tex = np.stack([u, v], -1).reshape(-1, 2)
    assert vtx.dtype == T and tex.dtype == T
    return vtx, tex


def deproject_np(sc, depth, half_pixel=False, misreading=None):
    """a5 in float32, one rounding per operation, with both Brown-Conrady branches: must equal the C oracle bit for bit."""
    return _deproject(np.float32, sc, depth, half_pixel, misreading)


def deproject_f64(sc, depth, half_pixel=False, misreading=None):
    """The same mathematics on the same (float32-valued) parameters, everything in double: what the oracle's rounding is measured
    against. Not a bit-exact anything."""
    return _deproject(np.float64, sc, depth, half_pixel, misreading)


def decode_payload_np(payload, downsample=1):
    """convertBufferToPointCloudXYZRGB (src/pcs-multicamera-optimized.cpp:226-248) -> (xyz float32[w, 3], rgb uint8[w, 3]):
    every record with i % downsample == 0, at most size / downsample of them (:230), (float)short / 1000.0f, R and G the two
    bytes of short 3, B the low byte of short 4."""
    f32 = np.float32
    d = max(int(downsample), 1)
    p = np.asarray(payload, np.int16).reshape(-1, 5)
    p = p[::d][:p.shape[0] // d]          # the cloud's width is size / downsample, rounded down (:230)
    with np.errstate(all="ignore"):
        xyz = (p[:, :3].astype(f32) / f32(1000.0)).astype(f32)
    c = p[:, 3].view(np.uint16)
    rgb = np.stack([c & 0xFF, c >> 8, p[:, 4].view(np.uint16) & 0xFF], -1).astype(np.uint8)
    return xyz, rgb


def affine_np(xyz, m16):
    """pcl::transformPointCloud as PCL 1.8 evaluates it (:289; third-party, restated, unpinned): ((m0*x + m1*y) + m2*z) + m3 with
    every product and sum rounded to float32. (PCL leaves a point with a non-finite coordinate alone when the cloud is not dense;
    decoded coordinates are always finite.)"""
    f32 = np.float32
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    M = np.asarray(m16, f32).reshape(-1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for r in range(3):
            a = (M[4 * r] * x).astype(f32)
            a = (a + (M[4 * r + 1] * y).astype(f32)).astype(f32)
            a = (a + (M[4 * r + 2] * z).astype(f32)).astype(f32)
            out[:, r] = (a + M[4 * r + 3]).astype(f32)
    return out


def encode_payload_np(xyz, rgb):
    """convertPointCloudXYZRGBToBuffer (:251-265): static_cast<short>(coordinate * 1000.0f) = truncation, low 16 bits;
    R + (G << 8) in short 3; B, high byte clear, in short 4."""
    f32 = np.float32
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64)
    out = np.empty((xyz.shape[0], 5), np.int16)
    with np.errstate(all="ignore"):
        a = (xyz * f32(1000.0)).astype(f32)
    out[:, :3] = (cvtt(a) & 0xFFFF).astype(np.uint16).view(np.int16)
    out[:, 3] = ((rgb[:, 0] + (rgb[:, 1] << 8)) & 0xFFFF).astype(np.uint16).view(np.int16)
    out[:, 4] = rgb[:, 2].astype(np.int16)
    return out


def transform_payload_np(payload, m16, downsample=1):
    """The centre's decode / affine / re-encode (src/pcs-multicamera-optimized.cpp:226-265, 289) in numpy float32: division by
    1000.0f, ((m0*x + m1*y) + m2*z) + m3 with every product and sum rounded to float32, * 1000.0f, truncation, low 16 bits."""
    xyz, rgb = decode_payload_np(payload, downsample)
    return encode_payload_np(affine_np(xyz, m16), rgb)
