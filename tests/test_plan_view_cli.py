"""-H (the plan-view maps of the cloud that leaves the filter chain) of pcs-multicamera-optimized on the GPU: the option's refusals
(malformed, with -G), and runs over the cameras of the node itself — -H alone, behind -E, and ahead of -V: the three Netpbm files
byte for byte what the restatement (tests/np_plan_view.py) makes of the cloud the same run dumped with -o, the `Plan view:` line,
and -L's, -J's, -W's and the dumped cloud's bytes with and without -H."""
import re
import subprocess

import numpy as np
import pytest

import np_plan_view as NP
from test_cluster_objects_cli import option
from test_tracks_cli import STABLE
from test_wire import CENTRAL, CLI_DIR

pytestmark = pytest.mark.gpu

BASE = ["-i", "synth:64x48", "-N", "2", "-q", "-r", "2"]
SPEC = ("+y", 40, 96, 80)                      # <up>, cell_mm, W, H: centred on 0
SPEC_E = ("-z", 50, 160, 150, -4000, -3700, -4000, 3000)     # ... an origin and a band of its own


def spec_option(prefix, spec):
    up, cell, w, h = spec[:4]
    return ",".join([prefix, up, str(cell), f"{w}x{h}"] + [str(v) for v in spec[4:]])


def spec_params(spec):
    up, cell, w, h = spec[:4]
    return NP.params(up=up, cell_mm=cell, width=w, height=h, origin=tuple(spec[4:6]) if len(spec) >= 6 else None,
                     band=tuple(spec[6:8]) if len(spec) == 8 else None)


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def run(args, cwd=None):
    return subprocess.run([CENTRAL] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)


def cloud_of(path):
    raw = open(path, "rb").read()
    size = int(np.frombuffer(raw[:4], "<i4")[0])
    assert size == len(raw) - 4 and size % 10 == 0
    return np.frombuffer(raw[4:], "<i2").reshape(-1, 5)


def files_of(prefix):
    return tuple(open(prefix + suffix, "rb").read() for suffix in (".rgb.ppm", ".top.pgm", ".count.pgm"))


def restated(cloud, spec):
    P = spec_params(spec)
    count, top, _, rgb, stats = NP.plan_np(cloud, P)
    return NP.netpbm_bytes(count, top, rgb, P), stats, P


def plan_line(stats, P):
    return (f"Plan view: {stats['considered']} considered, {stats['in_band']} in band, {stats['mapped']} on the map, {stats['occupied']} occupied of "
            f"{P['width']} x {P['height']} cells, fullest {stats['fullest']}")


def test_help_lists_the_option():
    r = run(["-h"])
    assert r.returncode == 0 and " -H <prefix>,<up>,<cell_mm>,<W>x<H>[,<u0>,<v0>[,<lo>,<hi>]] " in r.stdout
    assert "no flip" in r.stdout and "File row r is map row cv = r" in r.stdout


@pytest.mark.parametrize("arg, word", [("", "expected"), ("m,+z,10", "expected"), ("m,up,10,4x4", "<up>"), ("m,+z,0,4x4", "cell_mm"),
                                       ("m,+z,10,4097x4", "W and H"), ("m,+z,10,4x4,1", "expected"), ("m,+z,10,4x4,1,2,9,3", "band"),
                                       ("-q,+z,10,4x4", "prefix")])
def test_a_malformed_option_is_refused(tmp_path, arg, word):
    r = run(BASE + ["-H", arg], cwd=str(tmp_path))
    assert r.returncode == 2 and r.stderr.startswith(f"-H {arg}: ") and word in r.stderr, r.stderr
    assert "pcs_create" not in r.stderr and not list(tmp_path.iterdir())


def test_refused_with_the_node_library_and_given_twice(tmp_path):
    r = run(["-i", "synth:64x48", "-N", "2", "-G", "1", "-q", "-r", "1", "-H", spec_option(str(tmp_path / "m"), SPEC)])
    assert r.returncode == 2 and "-H is not available with -G: the node library has no plan view" in r.stderr
    r = run(BASE + ["-H", spec_option(str(tmp_path / "m"), SPEC), "-H", spec_option(str(tmp_path / "n"), SPEC)])
    assert r.returncode == 2 and "given twice" in r.stderr
    assert not list(tmp_path.iterdir())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan")
    f = lambda name: str(tmp / name)
    out = {"f": f}
    out["alone"] = run(BASE + ["-t", "-H", spec_option(f("alone"), SPEC), "-o", f("alone.bin")])
    chain = BASE + ["-Z", "-t", "-E", option(STABLE)]
    out["chain"] = run(chain + ["-L", f("objects.txt"), "-W", f("boxes.txt"), "-J", f("tracks.txt"), "-o", f("chain.bin"),
                               "-H", spec_option(f("chain"), SPEC_E)])
    out["chain0"] = run(chain + ["-L", f("objects0.txt"), "-W", f("boxes0.txt"), "-J", f("tracks0.txt"), "-o", f("chain0.bin")])
    out["voxel"] = run(BASE + ["-Z", "-V", "50", "-o", f("voxel.bin"), "-H", spec_option(f("voxel"), SPEC)])
    out["voxel0"] = run(BASE + ["-Z", "-V", "50", "-o", f("voxel0.bin")])
    out["dropped"] = run(BASE + ["-Z", "-o", f("dropped.bin"), "-H", spec_option(f("dropped"), SPEC)])
    for name in ("alone", "chain", "chain0", "voxel", "voxel0", "dropped"):
        assert out[name].returncode == 0, (name, out[name].stderr)
    return out


def test_alone_against_the_dumped_cloud(runs):
    """No stage, no -V: the stitched cloud itself, zero-depth pixels and all."""
    cloud = cloud_of(runs["f"]("alone.bin"))
    assert cloud.shape[0] == 2 * 64 * 48
    want, stats, P = restated(cloud, SPEC)
    assert files_of(runs["f"]("alone")) == want
    assert stats["mapped"] > 1000 and stats["occupied"] > 50
    lines = runs["alone"].stdout.splitlines()
    assert lines.count(plan_line(stats, P)) >= 1 and sum(line.startswith("Plan view:") for line in lines) == 2       # one per frame-set
    assert all(re.fullmatch(r"Plan view: \d+ considered, \d+ in band, \d+ on the map, \d+ occupied of 96 x 80 cells, fullest \d+", line)
               for line in lines if line.startswith("Plan view:"))


def test_behind_the_cluster_filter(runs):
    """The cloud that LEAVES the chain: -o dumps it, the maps are its maps (an origin and a band given)."""
    cloud = cloud_of(runs["f"]("chain.bin"))
    assert 0 < cloud.shape[0] < 2 * 64 * 48
    want, stats, P = restated(cloud, SPEC_E)
    assert files_of(runs["f"]("chain")) == want
    assert stats["considered"] == cloud.shape[0] and stats["occupied"] > 10
    lines = runs["chain"].stdout.splitlines()
    assert lines[max(k for k, line in enumerate(lines) if line.startswith("Plan view:"))] == plan_line(stats, P)
    # the line follows the chain's own
    first_plan = min(k for k, line in enumerate(lines) if line.startswith("Plan view:"))
    assert any(line.startswith("Cluster filter:") for line in lines[:first_plan])


def test_the_other_files_do_not_change(runs):
    f = runs["f"]
    for name in ("objects", "boxes", "tracks", "chain"):
        ext = "bin" if name == "chain" else "txt"
        a, b = open(f(f"{name}.{ext}"), "rb").read(), open(f(f"{name}0.{ext}"), "rb").read()
        assert len(a) > 4 and a == b, name
    assert "Plan view:" not in runs["chain0"].stdout
    kept = ("Cluster filter:", "Objects:", "Boxes:", "Tracks:")
    assert [line for line in runs["chain"].stdout.splitlines() if line.startswith(kept)] == \
        [line for line in runs["chain0"].stdout.splitlines() if line.startswith(kept)]


def test_ahead_of_the_voxel_grid(runs):
    """-V serves the voxel cloud; the maps are of the cloud in front of it: the same bytes as without -V, and -V's own output is
    what it is without -H."""
    f = runs["f"]
    voxels = open(f("voxel.bin"), "rb").read()
    assert len(voxels) > 4 and voxels == open(f("voxel0.bin"), "rb").read()
    dropped = cloud_of(f("dropped.bin"))
    assert cloud_of(f("voxel.bin")).shape[0] < dropped.shape[0]
    want, _, _ = restated(dropped, SPEC)
    assert files_of(f("voxel")) == want == files_of(f("dropped"))
