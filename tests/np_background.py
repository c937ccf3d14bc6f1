"""The background model and its subtraction (DESIGN.md section 3 "Background model and subtraction"), restated: a Python dict keyed
by (cx, cy, cz), brute force over the up-to-27 cells with explicit clipping, and the "PCB1" container (section 4) written entry by
entry. Shares no code with the library; slow on purpose."""
import struct

import numpy as np

FRAMES_MAX = 65535


def cells_of(rec, cell_mm):
    """(n, 3) cell coordinates of packed records: floor(v / cell_mm) + 32768 per axis (Python's // floors)."""
    xyz = np.asarray(rec, np.int16).reshape(-1, 5)[:, :3].astype(np.int64)
    return xyz // int(cell_mm) + 32768


class Model:
    def __init__(self, cell_mm, max_cells):
        assert 1 <= cell_mm <= 1000 and max_cells >= 1
        self.cell_mm, self.max_cells = int(cell_mm), int(max_cells)
        self.seen, self.frames, self.overflow = {}, 0, False

    def learn(self, rec):
        assert self.frames < FRAMES_MAX
        self.frames += 1
        for c in sorted(set(map(tuple, cells_of(rec, self.cell_mm).tolist()))):
            self.seen[c] = self.seen.get(c, 0) + 1
        if len(self.seen) > self.max_cells:
            self.overflow = True        # (which of the surplus cells a real table holds is unspecified: nothing below is defined then)

    def background_mask(self, rec, min_seen, dilate):
        """True where a record is background. Not defined for an overflowed model (subtract keeps everything then)."""
        assert not self.overflow and 1 <= min_seen <= FRAMES_MAX and dilate in (0, 1)
        out = []
        for cx, cy, cz in cells_of(rec, self.cell_mm).tolist():
            hit = False
            for dz in range(-dilate, dilate + 1):
                for dy in range(-dilate, dilate + 1):
                    for dx in range(-dilate, dilate + 1):
                        ax, ay, az = cx + dx, cy + dy, cz + dz
                        if ax < 0 or ax > 65535 or ay < 0 or ay > 65535 or az < 0 or az > 65535:
                            continue                        # no such cell: nothing wraps at the ends of the range
                        hit = hit or self.seen.get((ax, ay, az), 0) >= min_seen
            out.append(hit)
        return np.array(out, bool).reshape(-1)

    def subtract_mask(self, rec, min_seen, dilate, mode=0):
        """The KEEP mask of subtract: mode 0 keeps what is not background, mode 1 what is; an overflowed model keeps everything."""
        n = np.asarray(rec).reshape(-1, 5).shape[0]
        if self.overflow:
            return np.ones(n, bool)
        bg = self.background_mask(rec, min_seen, dilate)
        return bg if mode else ~bg

    def export(self):
        assert not self.overflow
        out = [b"PCB1", struct.pack("<IiII", 1, self.cell_mm, self.frames, len(self.seen)), bytes(12)]
        for (cx, cy, cz), seen in sorted(self.seen.items(), key=lambda kv: kv[0][0] | kv[0][1] << 16 | kv[0][2] << 32):
            out.append(struct.pack("<HHHHI", cx, cy, cz, 0, seen))
        return b"".join(out)


def learned(cell_mm, max_cells, frames):
    m = Model(cell_mm, max_cells)
    for rec in frames:
        m.learn(rec)
    return m
