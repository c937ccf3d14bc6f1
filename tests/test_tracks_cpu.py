"""The object tracker's restatement (tests/np_tracks.py) without a GPU: against the hand-written expectations of the tiny sequences of
tests/track_cases.py, against a second, independent formulation (the votes as a dense m x m_prev numpy histogram, choice and keeper
by argmax) on random sequences, and the permutation rule."""
import numpy as np
import pytest

import np_tracks as N
import track_cases as K

EXPECTED = sorted(name for name, c in K.CASES.items() if c.expect is not None)


def run_case(case, make=N.Tracker):
    tr = make(case.cell_mm, case.max_cells, case.max_objects)
    out = []
    for s in case.steps:
        if s.reset is not None:
            tr.reset(s.reset)
        out.append(tr.update(s.rec, s.object_of, s.n_objects, s.max_objects, s.min_votes) + (tr.info(),))
    return out


@pytest.mark.parametrize("name", EXPECTED)
def test_hand_written_expectations(name):
    case = K.CASES[name]
    got = run_case(case)
    assert len(got) == len(case.expect)
    for t, ((tracks, stats, info), rows) in enumerate(zip(got, case.expect)):
        want = K.expected_tracks(rows)
        assert tracks.tobytes() == want.tobytes(), (name, t, tracks, want)
        assert stats["objects"] == len(rows) and stats["born"] == sum(r[2] < 0 for r in rows)
        assert stats["continued"] + stats["born"] == stats["objects"]
        assert info["objects"] == len(rows)


def test_statistics_of_a_known_sequence():
    (_, s0, i0), (_, s1, i1), (_, s2, _) = run_case(K.CASES["alternating"])
    assert s0 == {"considered": 80, "voted": 0, "objects": 2, "continued": 0, "born": 2, "lost": 0, "overflow": 0, "frames": 1}
    assert s1 == {"considered": 80, "voted": 80, "objects": 2, "continued": 2, "born": 0, "lost": 0, "overflow": 0, "frames": 2}
    assert s2 == {"considered": 62, "voted": 62, "objects": 2, "continued": 1, "born": 1, "lost": 1, "overflow": 0, "frames": 3}
    assert i0["next_id"] == 3 and i1["next_id"] == 3 and i0["frames"] == 1


def test_overflow_sequences():
    got = run_case(K.CASES["overflow_cells"])
    assert [s["overflow"] for _, s, _ in got] == [0, 0, 2, 0]
    assert [i["overflow"] for _, _, i in got] == [0, 4, 2, 0]
    assert got[1][1]["continued"] == 3 and got[2][1] == dict(got[2][1], continued=0, born=3, lost=3, voted=0)
    assert got[3][1]["continued"] == 3
    got = run_case(K.CASES["overflow_pairs"])
    assert [s["overflow"] for _, s, _ in got] == [0, 1, 0, 0]
    assert got[1][1] == dict(got[1][1], continued=0, born=80, lost=40, voted=160)
    assert got[2][1]["continued"] == 40 and got[3][1]["continued"] == 40


class DenseTracker:
    """The second formulation: no dict of votes — a dense histogram over (k, j) from numpy, the previous map as sorted unique cell keys
    with a per-cell minimum, choice and keeper by row and column arg-max with the tie rules spelled as lexicographic keys."""

    def __init__(self, cell_mm, max_cells, max_objects):
        self.cell_mm, self.max_cells, self.max_objects = cell_mm, max_cells, max_objects
        self.reset(1)

    def reset(self, first_id):
        self.keys, self.owner, self.bad_map = np.zeros(0, np.int64), np.zeros(0, np.int64), False
        self.ids, self.ages = np.zeros(0, np.int64), np.zeros(0, np.int64)
        self.next_id, self.frames, self.last = first_id, 0, 0

    def info(self):
        return {"cell_mm": self.cell_mm, "max_cells": self.max_cells, "max_objects": self.max_objects, "objects": len(self.ids),
                "frames": self.frames, "next_id": self.next_id, "overflow": self.last | (4 if self.bad_map else 0)}

    def update(self, rec, object_of, n_objects, max_objects, min_votes=1):
        xyz = np.asarray(rec, np.int16).reshape(-1, 5)[:, :3].astype(np.int64)
        c = np.floor_divide(xyz, self.cell_mm) + 32768
        key = c[:, 0] | c[:, 1] << 16 | c[:, 2] << 32
        obj = np.asarray(object_of, np.int64)
        m, mp = min(max(n_objects, 0), max_objects), len(self.ids)
        part = (obj >= 0) & (obj < m)
        key, obj = key[part], obj[part]
        hist = np.zeros((m, max(mp, 1)), np.int64)
        voted = 0
        if not self.bad_map and len(self.keys) and len(key):
            pos = np.clip(np.searchsorted(self.keys, key), 0, len(self.keys) - 1)
            hit = self.keys[pos] == key
            np.add.at(hist, (obj[hit], self.owner[pos[hit]]), 1)
            voted = int(hit.sum())
        overflow = (1 if np.count_nonzero(hist) > self.max_cells else 0) | (2 if self.bad_map else 0)
        if overflow:
            hist[:] = 0
        tracks = np.zeros(m, N.TRACK_DTYPE)
        if m:
            js = np.arange(hist.shape[1])
            choice = np.array([np.lexsort((js, -row))[0] for row in hist])          # most votes, then the smallest j
            has = hist[np.arange(m), choice] > 0
            claim = np.where(has[:, None] & (choice[:, None] == js[None, :]), hist, 0)     # claim[k, j]: k's votes for its choice j
            keeper = np.array([np.lexsort((np.arange(m), -col))[0] for col in claim.T])   # most votes, then the smallest k
            cont = has & (keeper[choice] == np.arange(m)) & (hist[np.arange(m), choice] >= min_votes)
        else:
            choice, cont = np.zeros(0, np.int64), np.zeros(0, bool)
        rank = np.cumsum(~cont) - 1
        ids, ages = np.zeros(m, np.int64), np.zeros(m, np.int64)
        for k in range(m):
            if cont[k]:
                j = choice[k]
                ids[k], ages[k] = self.ids[j], min(self.ages[j] + 1, N.INT32_MAX)
                tracks[k] = (ids[k], ages[k], j, hist[k, j], 0)
            else:
                ids[k] = self.next_id + rank[k]
                tracks[k] = (ids[k], 0, -1, 0, 0)
        born = int((~cont).sum())
        stats = {"considered": int(part.sum()), "voted": voted, "objects": m, "continued": m - born, "born": born, "lost": mp - (m - born),
                 "overflow": overflow, "frames": self.frames + 1}
        order = np.lexsort((obj, key))
        key, obj = key[order], obj[order]
        firsts = np.ones(len(key), bool)
        firsts[1:] = key[1:] != key[:-1]
        self.keys, self.owner = key[firsts], obj[firsts]
        self.bad_map = len(self.keys) > self.max_cells
        self.ids, self.ages, self.next_id, self.frames, self.last = ids, ages, self.next_id + born, self.frames + 1, overflow
        return tracks, stats


def random_case(seed):
    """Blobs that drift, touch, split and vanish: six steps of up to twelve objects over a small arena, a small tracker now and then."""
    rng = np.random.default_rng(seed)
    max_cells = int(rng.choice([24, 64, 4096]))
    steps, centres = [], rng.integers(-6, 6, (12, 3))
    for t in range(6):
        m = int(rng.integers(0, 13))
        centres = centres + rng.integers(-1, 2, centres.shape)
        groups = []
        for k in range(m):
            for _ in range(int(rng.integers(1, 4))):
                cell = tuple((centres[k] + rng.integers(-1, 2, 3)).tolist())
                groups.append(K.group(k if rng.random() > 0.05 else -1, cell, int(rng.integers(1, 9))))
        steps.append(K.step(groups, n_objects=m + int(rng.integers(0, 2)), max_objects=int(rng.choice([12, 8])),
                            min_votes=int(rng.choice([1, 1, 3])), shuffle=int(rng.integers(0, 1 << 30)) if groups else None))
    return K.Case(f"random{seed}", K.CELL, max_cells, 12, steps, None)


def same(a, b):
    assert len(a) == len(b)
    for t, ((ta, sa, ia), (tb, sb, ib)) in enumerate(zip(a, b)):
        assert ta.tobytes() == tb.tobytes(), (t, ta, tb)
        assert sa == sb and ia == ib, (t, sa, sb, ia, ib)


@pytest.mark.parametrize("seed", range(40))
def test_two_formulations_agree_on_random_sequences(seed):
    case = random_case(seed)
    same(run_case(case), run_case(case, DenseTracker))


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_two_formulations_agree_on_the_cases(name):
    same(run_case(K.CASES[name]), run_case(K.CASES[name], DenseTracker))


@pytest.mark.parametrize("name", ["moved", "collisions", "ignored", "overflow_pairs", "shared_cell"])
def test_a_permutation_of_the_records_changes_nothing(name):
    case = K.CASES[name]
    rng = np.random.default_rng(5)
    steps = []
    for s in case.steps:
        p = rng.permutation(s.rec.shape[0])
        steps.append(s._replace(rec=np.ascontiguousarray(s.rec[p]), object_of=np.ascontiguousarray(s.object_of[p])))
    same(run_case(case), run_case(case._replace(steps=steps)))


def test_ids_follow_the_objects_not_their_numbers():
    got = run_case(K.CASES["moved"])
    perm = [3, 0, 4, 1, 2]
    assert got[0][0]["id"].tolist() == [1, 2, 3, 4, 5]
    assert [int(got[1][0]["id"][perm[k]]) for k in range(5)] == [1, 2, 3, 4, 5]
    assert got[2][0]["id"].tolist() == [1, 2, 3, 4, 5] and got[2][0]["age"].tolist() == [2] * 5
    assert got[2][1]["born"] == 0 and got[2][1]["lost"] == 0
