"""Named inputs for the plan-view maps: each the smallest that can break one thing (DESIGN.md section 3 lists them). A case is
(rec int16 [n,5], parameter dict of tests/np_plan_view.py). Shared by the CPU and the GPU tests, built once, never changed."""
from collections import namedtuple

import numpy as np

import np_plan_view as NP

Case = namedtuple("Case", "rec P")

TILE = 8192            # records per workgroup of the accumulate launch
TABLE_SLOTS = 1024     # slots of its LDS table


def records(xyz, seed=0):
    """xyz [n,3] -> records with colours that tell the indices apart: R, G, B from a seeded generator, never all zero."""
    xyz = np.asarray(xyz, np.int64).reshape(-1, 3)
    n = xyz.shape[0]
    rng = np.random.default_rng(1000 + seed)
    rec = np.zeros((n, 5), np.int16)
    rec[:, :3] = xyz.astype(np.int16)
    r, g, b = rng.integers(1, 256, n), rng.integers(0, 256, n), rng.integers(0, 256, n)
    rec[:, 3] = (r | (g << 8)).astype(np.uint16).view(np.int16)
    rec[:, 4] = b.astype(np.int16)
    return rec


def cloud(n, seed, lo=-400, hi=400):
    return records(np.random.default_rng(seed).integers(lo, hi, (n, 3)), seed)


def raster_order(n, seed, width=160, pitch=3):
    """What a camera leaves: consecutive records a few millimetres apart along x, rows along y, a height that varies slowly."""
    i = np.arange(n)
    rng = np.random.default_rng(seed)
    x = (i % width) * pitch - width * pitch // 2
    y = (i // width) * pitch - 200
    z = (50 * np.sin(i / 37.0)).astype(np.int64) + rng.integers(-2, 3, n)
    return records(np.stack([x, y, z], axis=1), seed)


def _build():
    c = {}
    P = NP.params
    c["empty"] = Case(np.zeros((0, 5), np.int16), P(width=8, height=8))
    c["one_record"] = Case(records([[5, -7, 123]]), P(width=8, height=8))
    for n in (63, 64, 65, 255, 256, 257, 2047, 2049, TILE - 1, TILE, TILE + 1):
        c[f"n_{n}"] = Case(cloud(n, n), P(cell_mm=10, width=80, height=80))
    # all six up choices on one cloud; -32768 along every axis so that `-` meets h = 32768
    xyz = np.random.default_rng(7).integers(-300, 300, (700, 3))
    xyz[::50] = -32768
    xyz[5::50, 0] = -32768
    xyz[6::50, 1] = -32768
    xyz[7::50, 2] = -32768
    xyz[8::50, 2] = 32767
    six = records(xyz, 7)
    for up in NP.UP_NAMES:
        c[f"up_{up}"] = Case(six, P(up=up, cell_mm=20, width=40, height=40))
        c[f"up_{up}_corner"] = Case(six, P(up=up, cell_mm=7, width=30, height=30, origin=(-32768, -32768)))
    # cell borders: differences k c - 1, k c, -1, 0, W c - 1, W c on both map axes
    for cell in (1, 2, 3, 7, 10, 1000, 32767):
        W, H = 5, 4
        u0, v0 = (-32768, -32768) if cell >= 1000 else (-17, 23)
        du = [-1, 0, cell - 1, cell, 2 * cell - 1, 2 * cell, W * cell - 1, W * cell, 3 * cell]
        dv = [-1, 0, cell - 1, cell, H * cell - 1, H * cell, 2 * cell]
        pts = [[u0 + a, v0 + b, (a * 7 + b * 3) % 100 - 50] for a in du for b in dv]
        pts = [p for p in pts if -32768 <= p[0] <= 32767 and -32768 <= p[1] <= 32767]
        c[f"borders_c{cell}"] = Case(records(pts, cell), P(cell_mm=cell, width=W, height=H, origin=(u0, v0)))
    ext = [[x, y, z] for x in (-32768, -32767, 0, 32766, 32767) for y in (-32768, 0, 32767) for z in (-32768, -1, 32767)]
    c["origin_low"] = Case(records(ext, 1), P(cell_mm=16, width=4096, height=64, origin=(-32768, -32768)))
    c["origin_high"] = Case(records(ext, 2), P(cell_mm=1, width=3, height=3, origin=(32767, 32767)))
    c["origin_mixed"] = Case(records(ext, 3), P(cell_mm=32767, width=2, height=3, origin=(-32768, 32767)))
    # the band: ends inclusive, one value, nothing
    col = records([[0, 0, z] for z in range(-5, 6)] + [[15, 0, z] for z in (-3, 3, 4)], 4)
    c["band_ends"] = Case(col, P(width=4, height=4, band=(-3, 3)))
    c["band_one_value"] = Case(col, P(width=4, height=4, band=(3, 3)))
    c["band_excludes_all"] = Case(col, P(width=4, height=4, band=(100, 200)))
    c["band_along_x"] = Case(six, P(up="-x", cell_mm=20, width=40, height=40, band=(-100, 50)))
    # grids
    wide = cloud(3000, 11, -3000, 3000)
    c["grid_1x1"] = Case(wide, P(cell_mm=500, width=1, height=1))
    rng = np.random.default_rng(13)
    strip = np.stack([rng.integers(-4200, 4200, 3000), rng.integers(-3, 3, 3000), rng.integers(-50, 50, 3000)], axis=1)
    c["grid_wmax_x1"] = Case(records(strip, 13), P(cell_mm=2, width=NP.SIDE_MAX, height=1))
    c["grid_1x_hmax"] = Case(records(strip[:, [1, 0, 2]], 14), P(cell_mm=2, width=1, height=NP.SIDE_MAX))
    c["grid_37x29"] = Case(wide, P(cell_mm=100, width=37, height=29))
    # 65 536 records in one cell, equal height, distinct colours: the lowest index wins rgb
    wall = np.zeros((65536, 5), np.int16)
    wall[:, :3] = (3, 4, 77)
    i = np.arange(65536)
    wall[:, 3] = ((i & 0xFF) | (((i >> 8) & 0xFF) << 8)).astype(np.uint16).view(np.int16)
    wall[:, 4] = ((i * 7 + 1) & 0xFF).astype(np.int16)
    c["wall_equal"] = Case(wall, P(width=16, height=16))
    ends = wall.copy()
    ends[-1, 2] = 78
    ends[0, 2] = 76
    c["wall_ends"] = Case(ends, P(width=16, height=16))
    # one wave: 64 distinct cells / two cells in turn
    lane = np.arange(64)
    c["wave_64_cells"] = Case(records(np.stack([lane * 10 - 320, np.zeros(64, np.int64), lane % 5], axis=1), 5), P(width=64, height=4))
    c["wave_two_cells"] = Case(records(np.stack([(lane % 2) * 10, np.zeros(64, np.int64), lane % 3], axis=1), 6), P(width=8, height=4))
    c["two_cells_4096"] = Case(records(np.stack([(np.arange(4096) % 2) * 10, np.zeros(4096, np.int64), np.arange(4096) % 9 - 4], axis=1), 8),
                               P(width=8, height=4))
    # more distinct cells in one tile than the table has slots: every record of two tiles in a cell of its own
    k = np.arange(2 * TILE)
    c["table_overflow"] = Case(records(np.stack([(k % 128) * 2 - 128, (k // 128) * 2 - 128, k % 11], axis=1), 9), P(cell_mm=2, width=128, height=128))
    c["raster_order"] = Case(raster_order(6000, 10), P(cell_mm=10, width=64, height=64))
    return c


CASES = _build()
SMALL = sorted(name for name, case in CASES.items() if case.rec.shape[0] <= 300 and case.P["width"] * case.P["height"] <= 4096)


def working_size():
    """2^20 - 100 000 random records over a 400 x 400 map and a 100 000-record column in one cell (2^20 records in all)."""
    rng = np.random.default_rng(20)
    n = (1 << 20) - 100000
    xyz = np.concatenate([np.stack([rng.integers(-2200, 2200, n), rng.integers(-2200, 2200, n), rng.integers(-500, 2500, n)], axis=1),
                          np.stack([np.full(100000, 1003), np.full(100000, -1507), rng.integers(0, 40, 100000)], axis=1)])
    order = rng.permutation(n + 50000)                     # half of the column stays in one run, half is scattered over the cloud
    xyz[:n + 50000] = xyz[:n + 50000][order]
    return Case(records(xyz, 20), NP.params(cell_mm=10, width=400, height=400))
