"""The plan-view maps restated (DESIGN.md section 3 "Plan-view maps"): numpy in int64 — floor division, np.maximum.at on the keys,
bincount — and a second statement as a plain Python loop for small inputs. Neither shares a line with the kernels or with
csrc/pcs_plan_math.h; the tests hold both of those to this file byte for byte.

A parameter set is a dict: up_axis, up_sign, cell_mm, origin_u, origin_v, width, height, band_lo, band_hi."""
import numpy as np

STATS_FIELDS = ("considered", "in_band", "mapped", "occupied", "fullest")
SIDE_MAX = 4096
CELLS_MAX = 1 << 22
UP_NAMES = {"+x": (0, 1), "-x": (0, -1), "+y": (1, 1), "-y": (1, -1), "+z": (2, 1), "-z": (2, -1)}


def params(up="+z", cell_mm=10, width=64, height=64, origin=None, band=None):
    """The CLI's defaults: without an origin the map is centred on 0, without a band it is the whole int16 range."""
    a, s = UP_NAMES[up]
    u0, v0 = (-((width * cell_mm) // 2), -((height * cell_mm) // 2)) if origin is None else origin
    lo, hi = (-32768, 32767) if band is None else band
    return dict(up_axis=a, up_sign=s, cell_mm=cell_mm, origin_u=u0, origin_v=v0, width=width, height=height, band_lo=lo, band_hi=hi)


def cells_np(rec, P):
    """-> (in_band bool [n], cell int64 [n], -1 off the map or out of band)."""
    rec = np.asarray(rec, np.int16).reshape(-1, 5).astype(np.int64)
    a = P["up_axis"]
    up, pu, pv = rec[:, a], rec[:, (a + 1) % 3], rec[:, (a + 2) % 3]
    in_band = (up >= P["band_lo"]) & (up <= P["band_hi"])
    cu = np.floor_divide(pu - P["origin_u"], P["cell_mm"])
    cv = np.floor_divide(pv - P["origin_v"], P["cell_mm"])
    on = in_band & (cu >= 0) & (cu < P["width"]) & (cv >= 0) & (cv < P["height"])
    return in_band, np.where(on, cv * P["width"] + cu, -1)


def keys_np(rec, P):
    """The two 64-bit keys of every record, as uint64: (h + 32768) << 32 | (0xFFFFFFFF - i) and (32768 - h) << 32 | (0xFFFFFFFF - i)."""
    rec = np.asarray(rec, np.int16).reshape(-1, 5).astype(np.int64)
    h = P["up_sign"] * rec[:, P["up_axis"]]
    low = 0xFFFFFFFF - np.arange(rec.shape[0], dtype=np.int64)
    return (((h + 32768) << 32) | low).astype(np.uint64), (((32768 - h) << 32) | low).astype(np.uint64)


def plan_np(rec, P):
    """-> (count uint32 [H,W], top int16 [H,W], bottom int16 [H,W], rgb uint8 [H,W,3], stats dict)."""
    rec = np.asarray(rec, np.int16).reshape(-1, 5)
    W, H = P["width"], P["height"]
    n, cells = rec.shape[0], W * H
    in_band, cell = cells_np(rec, P)
    on = cell >= 0
    idx = np.flatnonzero(on)
    count = np.bincount(cell[idx], minlength=cells).astype(np.int64)
    kt, kb = keys_np(rec, P)
    best_t, best_b = np.zeros(cells, np.uint64), np.zeros(cells, np.uint64)
    np.maximum.at(best_t, cell[idx], kt[idx])
    np.maximum.at(best_b, cell[idx], kb[idx])
    occupied = count > 0
    it = (0xFFFFFFFF - (best_t & np.uint64(0xFFFFFFFF)).astype(np.int64))[occupied]
    ib = (0xFFFFFFFF - (best_b & np.uint64(0xFFFFFFFF)).astype(np.int64))[occupied]
    top, bottom, rgb = np.zeros(cells, np.int16), np.zeros(cells, np.int16), np.zeros((cells, 3), np.uint8)
    a = P["up_axis"]
    top[occupied] = rec[it, a]
    bottom[occupied] = rec[ib, a]
    col = rec[it, 3].view(np.uint16).astype(np.int64)
    rgb[occupied, 0] = col & 0xFF
    rgb[occupied, 1] = col >> 8
    rgb[occupied, 2] = rec[it, 4].view(np.uint16).astype(np.int64) & 0xFF
    stats = dict(considered=n, in_band=int(in_band.sum()), mapped=int(on.sum()), occupied=int(occupied.sum()),
                 fullest=int(count.max()) if cells else 0)
    return count.astype(np.uint32).reshape(H, W), top.reshape(H, W), bottom.reshape(H, W), rgb.reshape(H, W, 3), stats


def plan_loop(rec, P):
    """The same from the definition's sentences, one record at a time in Python integers (small inputs)."""
    rec = np.asarray(rec, np.int16).reshape(-1, 5)
    W, H, c, a, s = P["width"], P["height"], P["cell_mm"], P["up_axis"], P["up_sign"]
    count = [[0] * W for _ in range(H)]
    best = [[None] * W for _ in range(H)]          # (h of the top, its index, h of the bottom, its index)
    in_band = mapped = 0
    for i, r in enumerate(rec.tolist()):
        p = r[:3]
        if not P["band_lo"] <= p[a] <= P["band_hi"]:
            continue
        in_band += 1
        cu, cv = (p[(a + 1) % 3] - P["origin_u"]) // c, (p[(a + 2) % 3] - P["origin_v"]) // c
        if not (0 <= cu < W and 0 <= cv < H):
            continue
        mapped += 1
        h = s * p[a]
        count[cv][cu] += 1
        b = best[cv][cu]
        if b is None:
            best[cv][cu] = (h, i, h, i)
        else:                                       # records arrive by ascending i: a tie keeps the earlier one
            best[cv][cu] = (h, i, b[2], b[3]) if h > b[0] else (b[0], b[1], h, i) if h < b[2] else b
    top, bottom, rgb = np.zeros((H, W), np.int16), np.zeros((H, W), np.int16), np.zeros((H, W, 3), np.uint8)
    for cv in range(H):
        for cu in range(W):
            b = best[cv][cu]
            if b is None:
                continue
            top[cv, cu], bottom[cv, cu] = rec[b[1], a], rec[b[3], a]
            rg = int(rec[b[1], 3]) & 0xFFFF
            rgb[cv, cu] = (rg & 0xFF, rg >> 8, int(rec[b[1], 4]) & 0xFF)
    flat = [v for row in count for v in row]
    stats = dict(considered=rec.shape[0], in_band=in_band, mapped=mapped, occupied=sum(v > 0 for v in flat), fullest=max(flat))
    return np.array(count, np.uint32).reshape(H, W), top, bottom, rgb, stats


def compare(got, want, where=""):
    """got / want: (count, top, bottom, rgb, stats dict); every raster byte for byte, every statistics word."""
    for name, g, w in zip(("count", "top", "bottom", "rgb"), got[:4], want[:4]):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (where, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            first = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{where}: {name} differs in {bad.shape[0]} places, first at {first}: got {g[first]}, want {w[first]}")
    assert {k: int(got[4][k]) for k in STATS_FIELDS} == {k: int(want[4][k]) for k in STATS_FIELDS}, (where, got[4], want[4])


# ---- the CLI's three files ------------------------------------------------------------------------------
def netpbm_bytes(count, top, rgb, P):
    """(<prefix>.rgb.ppm, <prefix>.top.pgm, <prefix>.count.pgm) as bytes: file row r is cv = r, column cu, no flip; the two grey
    maps 16-bit big-endian with maxval 65535; top.pgm 0 for an empty cell, else clamp(h + 32768, 1, 65535), h = up_sign * top."""
    H, W = count.shape
    head = lambda magic, maxval: f"{magic}\n{W} {H}\n{maxval}\n".encode()
    h = P["up_sign"] * top.astype(np.int64)
    grey = np.where(count > 0, np.clip(h + 32768, 1, 65535), 0)
    sat = np.minimum(count.astype(np.int64), 65535)
    return (head("P6", 255) + rgb.astype(np.uint8).tobytes(), head("P5", 65535) + grey.astype(">u2").tobytes(),
            head("P5", 65535) + sat.astype(">u2").tobytes())
