"""numpy restatement of the spatial filter ("Spatial filter"), written from that text and from nothing else,
in two forms: `line_pass_loop` / `spatial_filter_loop`, the plain per-pixel loop the text describes, and `spatial_filter`, the same
recurrence vectorised ACROSS lines (every row, or every column, advances one pixel at a time together), which also returns a census
of how often each branch of the step fired. The GPU kernels (csrc/pcs_kernels_filter.hip) are held to this bit for bit.

Also the scene the spatial-filter tests run on (`scene`): the package's synthetic depth has neighbours that differ by more than any
sensible delta almost everywhere, so the filter would hardly do anything on it.

Not a test module: the spatial-filter tests import it."""
import numpy as np

DEFAULTS = dict(alpha=0.5, delta=20, iterations=2, hole_radius=0)
BRANCHES = ("blend", "equal", "edge", "fill", "fill_exhausted")


def _constants(alpha):
    a = np.float32(alpha)
    return a, np.float32(1.0) - a                     # fp32, each computed once


def line_pass_loop(x, alpha, delta, hole_radius, fill_on):
    """One line pass over the 1-D uint16 array x, in place, exactly as the text says it."""
    a, oma = _constants(alpha)
    n = x.shape[0]
    if n <= 1:
        return
    v0, run = int(x[0]), 0
    for u in range(1, n):
        v1 = int(x[u])
        if v1 != 0:
            run = 0
        if v0 != 0 and v1 != 0:
            d = abs(v1 - v0)
            if 1 <= d <= delta:
                f = np.float32(np.float32(a * np.float32(v1)) + np.float32(oma * np.float32(v0)))      # two products, one sum
                v1 = min(int(np.float32(f + np.float32(0.5))), 65535)                                   # int() truncates
                x[u] = v1
        if v0 != 0 and v1 == 0 and fill_on and run < hole_radius:
            run += 1
            v1 = v0
            x[u] = v1
        v0 = v1


def spatial_filter_loop(raster, alpha=0.5, delta=20, iterations=2, hole_radius=0):
    """The whole filter by the plain loop: per iteration rows forward, rows backward (fill on), columns down, columns up (off)."""
    out = np.array(raster, np.uint16, copy=True)
    assert out.ndim == 2
    for _ in range(iterations):
        for r in range(out.shape[0]):
            line_pass_loop(out[r, :], alpha, delta, hole_radius, True)
        for r in range(out.shape[0]):
            line_pass_loop(out[r, ::-1], alpha, delta, hole_radius, True)
        for c in range(out.shape[1]):
            line_pass_loop(out[:, c], alpha, delta, hole_radius, False)
        for c in range(out.shape[1]):
            line_pass_loop(out[::-1, c], alpha, delta, hole_radius, False)
    return out


def _pass_all_lines(x, a, oma, delta, hole_radius, fill_on, census):
    """x: [lines, n] uint16 view, modified in place; every line takes the same step at the same time."""
    n = x.shape[1]
    if n <= 1:
        return
    v0 = x[:, 0].astype(np.int32)
    run = np.zeros(x.shape[0], np.int32)
    for u in range(1, n):
        v1 = x[:, u].astype(np.int32)
        run = np.where(v1 != 0, 0, run)
        both = (v0 != 0) & (v1 != 0)
        d = np.abs(v1 - v0)
        blend = both & (d >= 1) & (d <= delta)
        f = ((a * v1.astype(np.float32)).astype(np.float32) + (oma * v0.astype(np.float32)).astype(np.float32)).astype(np.float32)
        blended = np.minimum((f + np.float32(0.5)).astype(np.float32).astype(np.int32), 65535)          # the cast truncates
        v1 = np.where(blend, blended, v1)
        gap = (v0 != 0) & (v1 == 0) & bool(fill_on)
        fill = gap & (run < hole_radius)
        run = run + fill
        v1 = np.where(fill, v0, v1)
        x[:, u] = v1.astype(np.uint16)
        v0 = v1
        census["blend"] += int(blend.sum())
        census["equal"] += int((both & (d == 0)).sum())
        census["edge"] += int((both & (d > delta)).sum())
        census["fill"] += int(fill.sum())
        census["fill_exhausted"] += int((gap & ~fill).sum())


def spatial_filter(raster, alpha=0.5, delta=20, iterations=2, hole_radius=0):
    """The whole filter, vectorised across lines. Returns (output, census): census[b] is how often branch b of the step fired
    (fill_exhausted: a zero pixel behind a valid one in a row pass that was NOT filled because the gap's hole_radius was used up)."""
    out = np.array(raster, np.uint16, copy=True)
    assert out.ndim == 2
    a, oma = _constants(alpha)
    census = {b: 0 for b in BRANCHES}
    for _ in range(iterations):
        _pass_all_lines(out, a, oma, delta, hole_radius, True, census)
        _pass_all_lines(out[:, ::-1], a, oma, delta, hole_radius, True, census)
        _pass_all_lines(out.T, a, oma, delta, hole_radius, False, census)
        _pass_all_lines(out.T[:, ::-1], a, oma, delta, hole_radius, False, census)
    return out, census


BAND_WIDTHS = (1, 2, 3, 5, 9)


def scene(w, h, seed):
    """A Z16 raster the filter has something to do on: a plane 1000 + 3 c + 2 r with integer noise in [-6, 6] (neighbours blend at
    any delta >= 15), a +400 step at column 5 w / 8 (an edge), constant patches on every fourth cell of an 8 x 8 checker (ties,
    d = 0), zero bands 1, 2, 3, 5 and 9 pixels wide across the rows (columns k w / 7 .., rows h / 8 .. 7 h / 8) and across the
    columns (rows k h / 7 .., columns w / 8 .. 7 w / 8), a row and a column that begin with zeros."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:h, 0:w]
    d = 1000 + 3 * c + 2 * r + rng.integers(-6, 7, (h, w))
    d = d + np.where(c >= (5 * w) // 8, 400, 0)
    flat = ((r // 8 + c // 8) % 4) == 0
    corner = 1000 + 3 * (c // 8 * 8) + 2 * (r // 8 * 8) + np.where(c // 8 * 8 >= (5 * w) // 8, 400, 0)
    d = np.where(flat, corner, d)
    for k, width in enumerate(BAND_WIDTHS, start=1):
        c0, r0 = k * w // 7, k * h // 7
        d[h // 8:max(7 * h // 8, h // 8 + 1), c0:c0 + width] = 0
        d[r0:r0 + width, w // 8:max(7 * w // 8, w // 8 + 1)] = 0
    d[1 % h, 0:4] = 0
    d[0:3, 2 % w] = 0
    return np.ascontiguousarray(d.astype(np.uint16))


# the shapes and parameter sets both spatial-filter test modules run
SCENE_SHAPES = [(64, 48), (100, 37), (200, 70), (24, 130), (2056, 3), (1, 7), (9, 1)]          # (w, h)
CENSUS_SHAPES = [(64, 48), (100, 37), (200, 70)]
PARAMS = {
    "defaults": dict(DEFAULTS),
    "radius2": dict(alpha=0.5, delta=20, iterations=2, hole_radius=2),
    "five-iterations": dict(alpha=0.25, delta=50, iterations=5, hole_radius=65535),
    "alpha1": dict(alpha=1.0, delta=1, iterations=1, hole_radius=1),
    "tiny-alpha": dict(alpha=2.0 ** -10, delta=65535, iterations=1, hole_radius=0),
}
FULL_RANGE = dict(alpha=0.4, delta=65535, iterations=3, hole_radius=3)


def full_range_raster(w=100, h=37, seed=77):
    """Every Z16 value may appear, a fifth of the pixels are zero, and 65535 / 65534 sit side by side along a row and a column."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.2] = 0
    d[5, 6:10] = 0                                   # a gap longer than the radius: 65535 enters the row pass with v0 = 0
    d[5, 10:14] = [65535, 65534, 65535, 65535]
    d[8:12, 20] = [65534, 65535, 65535, 65534]
    return d
