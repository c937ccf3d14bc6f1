"""Object tracks (DESIGN.md section 3 "Object tracks"), restated: Python dicts for the map and the votes and the rules literally.
Shares no code with the library; slow on purpose."""
import numpy as np

TRACK_DTYPE = np.dtype([("id", "<i8"), ("age", "<i4"), ("prev", "<i4"), ("votes", "<i4"), ("reserved", "<i4")])
STATS_FIELDS = ("considered", "voted", "objects", "continued", "born", "lost", "overflow", "frames")
INT32_MAX = 2 ** 31 - 1


def cells_of(rec, cell_mm):
    """One (cx, cy, cz) tuple per packed record: floor(v / cell_mm) + 32768 per axis (Python's // floors)."""
    xyz = np.asarray(rec, np.int16).reshape(-1, 5)[:, :3].astype(np.int64)
    return [tuple(c) for c in (xyz // int(cell_mm) + 32768).tolist()]


class Tracker:
    def __init__(self, cell_mm, max_cells, max_objects):
        assert 1 <= cell_mm <= 1000 and 1 <= max_cells and 1 <= max_objects <= 65536
        self.cell_mm, self.max_cells, self.max_objects = int(cell_mm), int(max_cells), int(max_objects)
        self.reset(1)

    def reset(self, first_id):
        assert 1 <= first_id <= 2 ** 62
        self.m, self.ids, self.ages = 0, [], []
        self.map, self.map_overflow = {}, False
        self.next_id, self.frames, self.last_overflow = int(first_id), 0, 0

    def info(self):
        return {"cell_mm": self.cell_mm, "max_cells": self.max_cells, "max_objects": self.max_objects, "objects": self.m,
                "frames": self.frames, "next_id": self.next_id, "overflow": self.last_overflow | (4 if self.map_overflow else 0)}

    def update(self, rec, object_of, n_objects, max_objects, min_votes=1):
        """-> (tracks[m] as TRACK_DTYPE, the statistics block as a dict)."""
        assert 0 <= max_objects <= self.max_objects and 1 <= min_votes <= 2 ** 30
        object_of = np.asarray(object_of, np.int64).reshape(-1)
        cells = cells_of(rec, self.cell_mm)
        assert len(cells) == object_of.shape[0]
        m = min(max(int(n_objects), 0), int(max_objects))
        taking_part = [i for i in range(len(cells)) if 0 <= object_of[i] < m]

        # VOTES — an overflowed previous map is not read at all
        votes, voted = {}, 0
        if not self.map_overflow:
            for i in taking_part:
                j = self.map.get(cells[i])
                if j is not None:
                    voted += 1
                    key = (int(object_of[i]), j)
                    votes[key] = votes.get(key, 0) + 1
        overflow = (1 if len(votes) > self.max_cells else 0) | (2 if self.map_overflow else 0)
        if overflow:
            votes = {}              # this update continues nothing

        # CHOICE: the j with the most votes(k, j) > 0, on a tie the smallest j
        choice = {}
        for (k, j), v in votes.items():
            if k not in choice or (v, -j) > (votes[(k, choice[k])], -choice[k]):
                choice[k] = j
        # KEEPER: among the k with choice(k) = j the one with the most votes(k, j), on a tie the smallest k
        keeper = {}
        for k, j in choice.items():
            if j not in keeper or (votes[(k, j)], -k) > (votes[(keeper[j], j)], -keeper[j]):
                keeper[j] = k

        tracks = np.zeros(m, TRACK_DTYPE)
        ids, ages, born = [0] * m, [0] * m, 0
        for k in range(m):
            j = choice.get(k)
            if j is not None and keeper[j] == k and votes[(k, j)] >= min_votes:
                ids[k], ages[k] = self.ids[j], min(self.ages[j] + 1, INT32_MAX)
                tracks[k] = (ids[k], ages[k], j, votes[(k, j)], 0)
            else:
                ids[k], ages[k] = self.next_id + born, 0
                tracks[k] = (ids[k], 0, -1, 0, 0)
                born += 1
        continued = m - born
        lost = self.m - continued

        # STATE
        new_map = {}
        for i in taking_part:
            k = int(object_of[i])
            new_map[cells[i]] = min(new_map.get(cells[i], k), k)
        self.map, self.map_overflow = new_map, len(new_map) > self.max_cells
        self.m, self.ids, self.ages = m, ids, ages
        self.next_id += born
        self.frames += 1
        self.last_overflow = overflow
        stats = {"considered": len(taking_part), "voted": voted, "objects": m, "continued": continued, "born": born, "lost": lost,
                 "overflow": overflow, "frames": self.frames}
        return tracks, stats
