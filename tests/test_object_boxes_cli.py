"""-W (the oriented boxes of the -E stage's objects) of pcs-multicamera-optimized on the GPU: the option's refusals (malformed,
without -E, with -G), and a three-frame-set run over the cameras of the node itself: the file's header, per frame-set one line of
29 integers per object held to the restatement (tests/np_object_boxes.py) under the comparison rules of tests/test_object_boxes.py,
-L's and -J's files and the dumped cloud byte for byte what they are without -W, the `Boxes:` line, and -W without -L."""
import subprocess

import numpy as np
import pytest

import np_cluster_objects as NO
import np_object_boxes as NB
from test_cluster_objects_cli import LOCAL, option
from test_tracks_cli import FRAMES, N_STABLE, STABLE, payload_of
from test_wire import CENTRAL, CLI_DIR

pytestmark = pytest.mark.gpu

HEADER = ("# frame k count sum_x sum_y sum_z m_xx m_xy m_xz m_yy m_yz m_zz a0_x a0_y a0_z a1_x a1_y a1_z a2_x a2_y a2_z rank "
          "lo_0 lo_1 lo_2 hi_0 hi_1 hi_2 reserved")
BASE = ["-i", "synth:64x48", "-N", "3", "-Z"]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", CLI_DIR], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def run(args, cwd=None):
    return subprocess.run([CENTRAL] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)


def test_help_lists_the_option():
    r = run(["-h"])
    assert r.returncode == 0 and " -W <file> " in r.stdout and "Boxes: <objects> objects, <r> of rank 3" in r.stdout


@pytest.mark.parametrize("arg, word", [("", "file name is empty"), ("f.txt,5", "nothing after it"), (",", "nothing after it"),
                                       ("f.txt,", "nothing after it"), ("-E", "not another option"), ("-q", "not another option")])
def test_a_malformed_option_is_refused(tmp_path, arg, word):
    r = run(BASE + ["-E", option(LOCAL), "-q", "-r", "1", "-W", arg], cwd=str(tmp_path))
    assert r.returncode == 2 and r.stderr.startswith(f"-W {arg}: ") and word in r.stderr, r.stderr
    assert "pcs_create" not in r.stderr and not list(tmp_path.iterdir())
    r = run(BASE + ["-E", option(LOCAL), "-q", "-r", "1", "-W"], cwd=str(tmp_path))      # no argument at all: getopt's refusal, the usage
    assert r.returncode == 2 and not list(tmp_path.iterdir())


def test_refused_without_the_cluster_filter_and_with_the_node_library(tmp_path):
    path = str(tmp_path / "boxes.txt")
    r = run(["-i", "synth:64x48", "-N", "3", "-q", "-r", "1", "-W", path])
    assert r.returncode == 2 and "-W boxes the objects of the cluster filter: it needs -E" in r.stderr
    r = run(["-i", "synth:64x48", "-N", "2", "-G", "1", "-E", option(LOCAL), "-q", "-r", "1", "-W", path])
    assert r.returncode == 2 and "-W is not available with -G" in r.stderr
    assert not list(tmp_path.iterdir())


def rows_of(path_or_lines):
    lines = open(path_or_lines).read().splitlines() if isinstance(path_or_lines, str) else path_or_lines
    assert lines[0] == HEADER
    return [[int(v) for v in line.split(" ")] for line in lines[1:]]


def entries_of(rows):
    """The rows of one frame-set as OBJECT_BOX_DTYPE entries."""
    out = np.zeros(len(rows), NB.OBJECT_BOX_DTYPE)
    for e, row in zip(out, rows):
        v = row[2:]
        e["count"], e["sum_xyz"], e["m2"], e["axis"], e["rank"] = v[0], v[1:4], v[4:10], np.array(v[10:19]).reshape(3, 3), v[19]
        e["ext_lo"], e["ext_hi"], e["reserved"] = v[20:23], v[23:26], v[26]
    return out


def held_to_the_restatement(rows, params, frames, max_unsure=0.01):
    """Every frame-set's lines against the restatement of what the chain clustered; -> (objects, of rank 3) over the run."""
    objects = rank3 = at = 0
    for f in range(frames):
        payload = payload_of(f)
        _, n_objects, object_of = NO.cluster_objects(payload, *params)
        mine = rows[at:at + n_objects]
        at += n_objects
        assert all(len(row) == 29 for row in mine)
        assert [row[0] for row in mine] == [f] * n_objects and [row[1] for row in mine] == list(range(n_objects)), f
        got = entries_of(mine)
        NB.compare(got, payload, object_of, n_objects, 1024, where=f"frame {f}", axes=True, max_unsure=max_unsure)
        NB.check_members(got, payload, object_of, n_objects, 1024, where=f"frame {f}")
        objects += n_objects
        rank3 += int((got["rank"] == 3).sum())
    assert at == len(rows)
    return objects, rank3


@pytest.fixture(scope="module")
def three_frame_sets(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("boxes")
    files = {name: str(tmp / name) for name in ("boxes.txt", "tracks.txt", "objects.txt", "cloud.bin", "tracks0.txt", "objects0.txt", "cloud0.bin")}
    common = BASE + ["-E", option(STABLE), "-q", "-r", str(FRAMES), "-t"]
    r = run(common + ["-L", files["objects.txt"], "-J", files["tracks.txt"], "-o", files["cloud.bin"], "-W", files["boxes.txt"]])
    assert r.returncode == 0, r.stderr
    r0 = run(common + ["-L", files["objects0.txt"], "-J", files["tracks0.txt"], "-o", files["cloud0.bin"]])
    assert r0.returncode == 0, r0.stderr
    return r, r0, files


def test_three_frame_sets_against_the_restatement(three_frame_sets):
    r, _, files = three_frame_sets
    rows = rows_of(files["boxes.txt"])
    assert len(rows) == FRAMES * N_STABLE
    objects, rank3 = held_to_the_restatement(rows, STABLE, FRAMES)
    lines = r.stdout.splitlines()
    assert lines.count(f"Boxes: {objects} objects, {rank3} of rank 3") == 1 and sum(line.startswith("Boxes:") for line in lines) == 1
    # a line joins -J's on (frame, k), and counts what -J's size column counts
    tracks = [[int(v) for v in line.split(" ")] for line in open(files["tracks.txt"]).read().splitlines()[1:]]
    assert [row[:2] for row in tracks] == [row[:2] for row in rows] and [row[7] for row in tracks] == [row[2] for row in rows]
    assert [row[14:17] for row in tracks] == [row[3:6] for row in rows]                     # sum_xyz


def test_the_other_files_do_not_change(three_frame_sets):
    r, r0, files = three_frame_sets
    for name in ("tracks", "objects"):
        assert open(files[f"{name}.txt"], "rb").read() == open(files[f"{name}0.txt"], "rb").read(), name
    cloud = open(files["cloud.bin"], "rb").read()
    assert len(cloud) > 4 and cloud == open(files["cloud0.bin"], "rb").read()
    assert "Boxes:" not in r0.stdout
    kept = ("Cluster filter:", "Objects:", "Tracks:")
    assert [line for line in r.stdout.splitlines() if line.startswith(kept)] == [line for line in r0.stdout.splitlines() if line.startswith(kept)]


def test_without_the_object_table_option_and_to_stdout(three_frame_sets, tmp_path):
    """-W alone: the table is made at -L's default size, no `Objects:` line, no -L or -J file; `-` is stdout."""
    _, _, files = three_frame_sets
    r = run(BASE + ["-E", option(STABLE), "-W", "-", "-q", "-r", str(FRAMES)], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert "Objects:" not in r.stdout and "Boxes:" not in r.stdout and "Tracks:" not in r.stdout and not list(tmp_path.iterdir())
    got = [line for line in lines if line == HEADER or (line[:1].isdigit() and len(line.split(" ")) == 29)]
    assert rows_of(got) == rows_of(files["boxes.txt"])


def test_objects_that_come_and_go(tmp_path):
    """Small clusters: more objects, some of them flat or thin — line for line under the same rules, except that whatever the
    cameras' noise makes of a small cluster may lie near an eigenvalue crossing: those axes are left out, however many they are."""
    path = str(tmp_path / "boxes.txt")
    r = run(BASE + ["-E", option(LOCAL), "-W", path, "-q", "-r", str(FRAMES), "-t"])
    assert r.returncode == 0, r.stderr
    objects, rank3 = held_to_the_restatement(rows_of(path), LOCAL, FRAMES, max_unsure=1.0)
    assert objects > 13 and f"Boxes: {objects} objects, {rank3} of rank 3" in r.stdout.splitlines()
