"""Frame-set sequences for the object tracker (tests/test_tracks_cpu.py, tests/test_tracks.py). A sequence is a tracker geometry and
a list of steps; a step is what pcs_cluster_objects_device* would leave: records, object_of, the object count, max_objects, plus
min_votes and an optional reset in front of it. `expect` (tiny sequences only) is hand-written: per step the (id, age, prev, votes)
of every object."""
from collections import namedtuple

import numpy as np

Step = namedtuple("Step", "rec object_of n_objects max_objects min_votes reset")
Case = namedtuple("Case", "name cell_mm max_cells max_objects steps expect")

CELL = 100


def group(obj, cell, count, cell_mm=CELL, shift=(0, 0, 0)):
    """`count` records of object `obj` in the cell whose signed coordinates are `cell` (records spread over the cell's lower half,
    then moved by `shift` millimetres); colour differs per record and is never read."""
    r = np.arange(count)
    half = max(cell_mm // 2, 1)
    rec = np.zeros((count, 5), np.int64)
    for a in range(3):
        rec[:, a] = cell[a] * cell_mm + (r * (3 + 2 * a)) % half + shift[a]
    rec[:, 3] = (r * 37 + obj) & 0x7FFF
    rec[:, 4] = (r * 11) & 0xFF
    assert np.abs(rec[:, :3]).max() <= 32767
    return rec.astype(np.int16), np.full(count, obj, np.int32)


def step(groups, n_objects=None, max_objects=None, min_votes=1, shuffle=None, interleave=False, reset=None, default_max=16):
    recs = [g[0] for g in groups] or [np.zeros((0, 5), np.int16)]
    objs = [g[1] for g in groups] or [np.zeros(0, np.int32)]
    if interleave:                      # record by record: a, b, a, b, ...
        n = min(r.shape[0] for r in recs)
        rec = np.stack([r[:n] for r in recs], 1).reshape(-1, 5)
        obj = np.stack([o[:n] for o in objs], 1).reshape(-1)
    else:
        rec, obj = np.concatenate(recs), np.concatenate(objs)
    if shuffle is not None:
        p = np.random.default_rng(shuffle).permutation(rec.shape[0])
        rec, obj = rec[p], obj[p]
    if n_objects is None:
        n_objects = int(obj.max()) + 1 if obj.shape[0] else 0
    return Step(np.ascontiguousarray(rec, np.int16), np.ascontiguousarray(obj, np.int32), n_objects,
                default_max if max_objects is None else max_objects, min_votes, reset)


def relabel(s, perm):
    """The same step with object k renamed perm[k] (a consistent renaming) — what another record order does to `rank by first record`."""
    perm = np.asarray(perm, np.int32)
    obj = np.where(s.object_of >= 0, perm[np.clip(s.object_of, 0, len(perm) - 1)], s.object_of).astype(np.int32)
    return s._replace(object_of=obj)


def _blob(obj, origin, cells=3, per_cell=7, shift=(0, 0, 0)):
    return [group(obj, (origin[0] + c, origin[1], origin[2]), per_cell, shift=shift) for c in range(cells)]


def _objects(n, shift=(0, 0, 0), per_cell=7):
    out = []
    for k in range(n):
        out += _blob(k, (-40 + 8 * k, 3 * k - 5, k), shift=shift, per_cell=per_cell)
    return out


def _cases():
    A, B, C_, D = (0, 0, 0), (5, 0, 0), (10, 0, 0), (15, 0, 0)
    born = lambda i: (i, 0, -1, 0)
    yield Case("first_still", CELL, 256, 16, [step(_objects(5)), step(_objects(5))],
               [[born(i) for i in range(1, 6)], [(i, 1, i - 1, 21) for i in range(1, 6)]])
    # every object moved by 45 mm (less than a cell), the records shuffled, the objects renamed as another record order would
    perm = [3, 0, 4, 1, 2]
    yield Case("moved", CELL, 256, 16,
               [step(_objects(5)), relabel(step(_objects(5, shift=(45, 0, 0)), shuffle=7), perm), step(_objects(5, shift=(90, 0, 0)), shuffle=8)], None)
    yield Case("run200", CELL, 64, 4, [step([group(0, A, 200)], max_objects=4), step([group(0, A, 200)], max_objects=4)],
               [[born(1)], [(1, 1, 0, 200)]])
    yield Case("alternating", CELL, 64, 4,
               [step([group(0, A, 40), group(1, B, 40)], interleave=True, max_objects=4),
                step([group(1, A, 40), group(0, B, 40)], interleave=True, max_objects=4),
                step([group(0, A, 31), group(1, A, 31)], interleave=True, max_objects=4)],       # one cell, two objects: P = 0
               [[born(1), born(2)], [(2, 1, 1, 40), (1, 1, 0, 40)], [(1, 2, 1, 31), born(3)]])
    yield Case("many_workgroups", CELL, 64, 4,
               [step([group(0, A, 4500), group(1, B, 4500)], interleave=True, max_objects=4),
                step([group(0, A, 4500), group(1, B, 4500)], interleave=True, max_objects=4)],
               [[born(1), born(2)], [(1, 1, 0, 4500), (2, 1, 1, 4500)]])
    yield Case("split_70_30", CELL, 64, 4, [step([group(0, A, 7), group(0, B, 3)]), step([group(0, B, 3), group(1, A, 7)])],
               [[born(1)], [born(2), (1, 1, 0, 7)]])
    yield Case("split_50_50", CELL, 64, 4, [step([group(0, A, 5), group(0, B, 5)]), step([group(0, B, 5), group(1, A, 5)])],
               [[born(1)], [(1, 1, 0, 5), born(2)]])
    yield Case("merge_60_40", CELL, 64, 4, [step([group(0, A, 4), group(1, B, 6)]), step([group(0, A, 4), group(0, B, 6)])],
               [[born(1), born(2)], [(2, 1, 1, 6)]])
    yield Case("merge_50_50", CELL, 64, 4, [step([group(0, A, 5), group(1, B, 5)]), step([group(0, A, 5), group(0, B, 5)])],
               [[born(1), born(2)], [(1, 1, 0, 5)]])
    # choice(1) = 0 but keeper(0) = 0: object 1 is born although it also voted for 1, which is lost
    yield Case("chain", CELL, 64, 4, [step([group(0, A, 10), group(1, B, 4)]),
                                      step([group(0, A, 10), group(1, A, 6), group(1, B, 4)])],
               [[born(1), born(2)], [(1, 1, 0, 10), born(3)]])
    # a cell far above any cluster tolerance: two previous objects share it, the map keeps the smallest j
    yield Case("shared_cell", 1000, 64, 4,
               [step([group(0, A, 3, 1000), group(1, A, 9, 1000, shift=(600, 0, 0)), group(2, B, 2, 1000)]),
                step([group(0, A, 9, 1000, shift=(600, 0, 0))]), step([group(0, B, 1, 1000), group(1, A, 4, 1000)])],
               [[born(1), born(2), born(3)], [(1, 1, 0, 9)], [born(4), (1, 2, 0, 4)]])
    yield Case("min_votes", CELL, 64, 4,
               [step([group(0, A, 5)]), step([group(0, A, 5)], min_votes=5), step([group(0, A, 5)], min_votes=4),
                step([group(0, A, 5)], min_votes=6), step([group(0, A, 5)], min_votes=1)],
               [[born(1)], [(1, 1, 0, 5)], [(1, 2, 0, 5)], [born(2)], [(2, 1, 0, 5)]])
    ends = np.array([[-32768, -32768, -32768, 1, 2], [32767, 32767, 32767, 3, 4], [-32768, 32767, 0, 5, 6], [0, -32768, 32767, 7, 8]], np.int16)
    for cell_mm in (1, 1000):
        s = Step(ends, np.arange(4, dtype=np.int32), 4, 4, 1, None)
        yield Case(f"range_ends_cell{cell_mm}", cell_mm, 64, 4, [s, s._replace(object_of=np.array([3, 2, 1, 0], np.int32))],
                   [[born(i) for i in range(1, 5)], [(4 - k, 1, 3 - k, 1) for k in range(4)]])
    # -1, a k at and beyond max_objects, an n_objects above max_objects (m = 3): objects 3 and 4 and the -1 records are ignored
    ign = [group(0, A, 4), group(-1, A, 9), group(1, B, 4), group(3, C_, 5), group(2, C_, 2), group(4, D, 6), group(70000, D, 2)]
    yield Case("ignored", CELL, 64, 8, [step(ign, n_objects=5, max_objects=3), step(ign, n_objects=70000, max_objects=3, shuffle=3)],
               [[born(1), born(2), born(3)], [(1, 1, 0, 4), (2, 1, 1, 4), (3, 1, 2, 2)]])
    # about 1 500 distinct cells in 4 096 slots: probes collide
    rng = np.random.default_rng(11)
    cells = rng.integers(-20, 20, (1500, 3))
    many = [group(int(i % 37), tuple(c), 1 + int(i % 3)) for i, c in enumerate(cells)]
    yield Case("collisions", CELL, 2048, 64, [step(many, max_objects=64), step(many, shuffle=5, max_objects=64),
                                               step(many[:900], shuffle=6, max_objects=64)], None)
    # overflow (b): 100 cells in a tracker of 64: that update is normal, the next is all born (bit 1), the one after normal again
    wide = [group(k % 3, (k, 1, 0), 2) for k in range(100)]
    small = [group(k, (k, 1, 0), 3) for k in range(3)]
    yield Case("overflow_cells", CELL, 64, 4, [step(small), step(wide), step(small), step(small)], None)
    # overflow (a): 40 cells, two objects in each: 80 pairs
    forty = [group(k, (k - 20, 0, 0), 2) for k in range(40)]
    eighty = [group(2 * (k // 2) + k % 2, (k // 2 - 20, 0, 0), 2) for k in range(80)]
    yield Case("overflow_pairs", CELL, 64, 128, [step(forty, max_objects=128), step(eighty, max_objects=128), step(forty, max_objects=128, shuffle=2),
                                                  step(forty, max_objects=128)], None)
    first = 2 ** 32 - 2
    yield Case("reset_ids", CELL, 64, 8, [step(_objects(2)), step(_objects(4), reset=first), step(_objects(4))],
               [[born(1), born(2)], [born(first + i) for i in range(4)], [(first + i, 1, i, 21) for i in range(4)]])
    empty = np.zeros((0, 5), np.int16)
    yield Case("zero", CELL, 64, 8,
               [step(_objects(3)), step(_objects(3), n_objects=0), step(_objects(3)), Step(empty, np.zeros(0, np.int32), 3, 16, 1, None),
                step(_objects(3))],
               [[born(1), born(2), born(3)], [], [born(4), born(5), born(6)], [born(7), born(8), born(9)], [born(10), born(11), born(12)]])


def _fit(c):          # no step asks for more objects than its tracker holds
    return c._replace(steps=[s._replace(max_objects=min(s.max_objects, c.max_objects)) for s in c.steps])


CASES = {c.name: _fit(c) for c in _cases()}


def expected_tracks(rows):
    from np_tracks import TRACK_DTYPE
    out = np.zeros(len(rows), TRACK_DTYPE)
    for k, (i, age, prev, votes) in enumerate(rows):
        out[k] = (i, age, prev, votes, 0)
    return out
