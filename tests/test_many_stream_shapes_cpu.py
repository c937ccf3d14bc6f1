"""The many-stream shape tables (tests/many_stream_shapes.py) without a GPU: the tables hold what they promise, the two forms of the
spatial restatement agree at the new widths, the spatial rasters reach every branch of the step, and the decimation sources hold
both kinds of block the kernel treats differently. These are conditions on the INPUTS of tests/test_filters_many_streams.py."""
import numpy as np
import pytest

import many_stream_shapes as M
import np_spatial_filter as SP

PARAMS = SP.PARAMS


def test_table_properties():
    both = M.NARROW + M.WIDE
    assert sorted(w for w, _ in both) == list(range(1, 129))                    # every width once
    assert sorted(h for _, h in both) == list(range(1, 129))                    # every height once
    assert sorted(w for w, _ in M.NARROW) == sorted(h for _, h in M.NARROW) == list(range(1, 65))
    assert sorted(w for w, _ in M.WIDE) == sorted(h for _, h in M.WIDE) == list(range(65, 129))
    assert any(h < 96 for _, h in M.WIDE) and any(h >= 96 for _, h in M.WIDE)
    for table in M.TABLES.values():
        assert 1 <= len(table) <= M.PCS_MAX_STREAMS
    assert len(M.NARROW) == len(M.WIDE) == M.PCS_MAX_STREAMS
    assert len(M.MIXED17) == 17 > M.LAUNCH_STREAMS
    for shape in [(2056, 3), (1, 7), (9, 1), (64, 48), (100, 37), (1280, 2)]:
        assert shape in M.MIXED17
    assert M.MIXED17[6:] == [(68, 48), (160, 96)] * 5 + [(68, 48)]
    assert max(w for w, _ in M.MIXED17) > 2048                                   # wider than one pass of the row kernels


def test_the_library_header_agrees_on_the_limits():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pcs_hip.h")).read()
    device = open(os.path.join(root, "pointcloud_stitching_amd", "csrc", "pcs_device.h")).read()
    assert int(re.search(r"#define\s+PCS_MAX_STREAMS\s+(\d+)", header).group(1)) == M.PCS_MAX_STREAMS
    assert int(re.search(r"kLaunchStreams\s*=\s*(\d+)", device).group(1)) == M.LAUNCH_STREAMS


def _two_form_subset():
    """Every width 1..16, the streams at w = 63, 64, 65 and 71 wherever the tables put them, and (2056, 3)."""
    by_width = {w: (name, s) for name in ("NARROW", "WIDE") for s, (w, _) in enumerate(M.TABLES[name])}
    picks = [by_width[w] for w in list(range(1, 17)) + [63, 64, 65, 71]]
    return picks + [("MIXED17", M.MIXED17.index((2056, 3)))]


@pytest.mark.parametrize("name,s", _two_form_subset())
def test_loop_and_vectorised_forms_agree_at_the_new_shapes(name, s):
    w, h = M.TABLES[name][s]
    d = M.spatial_rasters(name)[s]
    assert d.shape == (h, w) and d.dtype == np.uint16
    got, _ = SP.spatial_filter(d, **PARAMS["radius2"])
    assert np.array_equal(got, SP.spatial_filter_loop(d, **PARAMS["radius2"]))


def test_spatial_rasters_are_the_scene_by_stream():
    for name in M.TABLES:
        rasters = M.spatial_rasters(name)
        assert len(rasters) == len(M.TABLES[name])
        for s, (w, h) in enumerate(M.TABLES[name]):
            assert np.array_equal(rasters[s], SP.scene(w, h, M.SEEDS[name] + s))


def test_census_over_narrow_and_wide_reaches_every_branch():
    total = {b: 0 for b in SP.BRANCHES}
    changed = 0
    for name in ("NARROW", "WIDE"):
        for d in M.spatial_rasters(name):
            out, census = SP.spatial_filter(d, **PARAMS["radius2"])
            changed += not np.array_equal(out, d)
            for b in SP.BRANCHES:
                total[b] += census[b]
    print(total, changed)
    assert all(total[b] > 0 for b in SP.BRANCHES), total
    assert changed > 100                                                         # the filter did something on nearly every stream


@pytest.mark.parametrize("n", range(2, 9))
def test_decimation_sources_hold_both_kinds_of_block(n):
    for name, table in M.TABLES.items():
        shapes = M.source_shapes(name, n)
        sources = M.decimation_sources(name, n)
        empty = partly = whole = 0
        for s, ((w, h), d) in enumerate(zip(table, sources)):
            assert d.shape == shapes[s] == (n * h + (s // 2) % n, n * w + s % n) and d.dtype == np.uint16
            assert d.shape[0] // n == h and d.shape[1] // n == w
            k = (d[:n * h, :n * w].reshape(h, n, w, n) != 0).sum(axis=(1, 3))
            empty += int((k == 0).sum())
            partly += int(((k > 0) & (k < n * n)).sum())
            whole += int((k == n * n).sum())
        print(name, n, empty, partly, whole)
        assert empty > 0 and partly > 0, (name, n)
        if n <= 4:
            assert whole > 0, (name, n)
        # sources that are and are not multiples of the scale
        assert any(sh[1] % n == 0 for sh in shapes) and any(sh[1] % n != 0 for sh in shapes)
        assert any(sh[0] % n == 0 for sh in shapes) and any(sh[0] % n != 0 for sh in shapes)
    # ... and of 8 (the wide and the narrow source accesses), over the three tables together, next to outputs of either kind
    every = [(sh[1], w) for name, table in M.TABLES.items() for sh, (w, _) in zip(M.source_shapes(name, n), table)]
    for ws_wide in (True, False):
        for wd_wide in (True, False):
            assert any((ws % 8 == 0) == ws_wide and (wd % 8 == 0) == wd_wide for ws, wd in every), (n, ws_wide, wd_wide)


def test_temporal_frames_have_histories_and_a_disagreement():
    for name in ("NARROW", "MIXED17"):
        frames = M.temporal_frames(name)
        assert len(frames) == 6 and all(len(f) == len(M.TABLES[name]) for f in frames)
        s = M.TABLES[name].index((64, 48)) if name == "MIXED17" else 63          # a stream of a few thousand pixels
        stack = np.stack([f[s] for f in frames])
        valid = (stack != 0).sum(axis=0)
        assert (valid == 6).any() and ((valid > 0) & (valid < 6)).any()          # always valid; sometimes valid
        assert (np.abs(stack[3].astype(int) - stack[2].astype(int))[(stack[3] != 0) & (stack[2] != 0)] > 100).any()
