"""Hand-made chunk layouts for the minimum-quality tests: regions given as a start, draft bytes and inserts are cut into
chunks the builder's way (seq_length rows that overlap by seq_overlap, the last chunk padded with -1), small enough that many
chunks cost nothing. Labels start out spelling the draft; tests plant edits row by row."""
import types
from typing import Dict, Sequence, Tuple

import numpy as np

BASES = "ACGT"


def upper(b: int) -> str:
    return chr(b - 32) if 97 <= b <= 122 else chr(b)


class Layout:
    """position, index [n, L], region, chunk_id [n]; ref_start, ref_end, ref_off, ref of the batch; rows[g]: the (position,
    index) of every row of region g in order. `out` and `batch` are what Context's host forms take."""

    def __init__(self, regions: Sequence[Tuple[int, bytes, Dict[int, int]]], L: int, O: int):
        self.L, self.O, step = L, O, L - O
        pos, idx, reg, cid, self.rows = [], [], [], [], []
        for g, (start, draft, inserts) in enumerate(regions):
            rows = []
            for p in range(start, start + len(draft)):
                rows += [(p, x) for x in range(1 + inserts.get(p, 0))]
            self.rows.append(rows)
            c = 0
            while True:
                part = rows[c * step:c * step + L]
                part = part + [(-1, -1)] * (L - len(part))
                pos.append([p for p, _ in part]); idx.append([x for _, x in part]); reg.append(g); cid.append(c)
                if c * step + L >= len(rows):
                    break
                c += 1
        self.position, self.index = np.array(pos, np.int64), np.array(idx, np.int32)
        self.region, self.chunk_id = np.array(reg, np.int32), np.array(cid, np.int32)
        self.ref_start = np.array([s for s, _, _ in regions], np.int64)
        self.ref_end = np.array([s + len(d) - 1 for s, d, _ in regions], np.int64)
        self.ref_off = np.concatenate([[0], np.cumsum([len(d) for _, d, _ in regions])]).astype(np.int64)
        self.ref = np.frombuffer(b"".join(d for _, d, _ in regions), np.uint8).copy()
        self.n, self.n_regions = len(cid), len(regions)
        self.out = types.SimpleNamespace(position=self.position, index=self.index, region=self.region, chunk_id=self.chunk_id)
        self.batch = types.SimpleNamespace(ref_start=self.ref_start, ref_end=self.ref_end, ref_off=self.ref_off, ref=self.ref,
                                           n_regions=self.n_regions)
        for a in (self.position, self.index, self.region, self.chunk_id, self.ref_start, self.ref_end, self.ref_off, self.ref):
            a.setflags(write=False)

    def args(self):
        """what the checker takes behind labels and row qualities"""
        return self.position, self.index, self.region, self.chunk_id, self.ref_start, self.ref_off, self.ref

    def draft(self, g: int, p: int) -> int:
        return int(self.ref[int(self.ref_off[g]) + p - int(self.ref_start[g])])

    def where(self, g: int, r: int):
        """(chunks, rows) of every copy of row r of region g"""
        p, x = self.rows[g][r]
        return np.nonzero((self.position == p) & (self.index == x) & (self.region == g)[:, None])

    def _draft_rank(self):
        """for every row: the place in ACGT of the upper-cased draft byte under it (-1: none spells it; base rows only),
        and whether it is a base row"""
        g = np.broadcast_to(self.region[:, None], self.position.shape)
        base_row = (self.position >= 0) & (self.index == 0)
        at = np.where(base_row, self.ref_off[g] + self.position - self.ref_start[g], 0)
        d = self.ref[at]
        d = np.where((d >= 97) & (d <= 122), d - 32, d)
        rank = np.full(self.position.shape, -1, np.int64)
        for i, c in enumerate(b"ACGT"):
            rank[d == c] = i
        return rank, base_row

    def spelled(self, qual: int = 60):
        """labels that spell the draft (label 1 over a byte that cannot be spelled: a pinned substitution), no inserted base,
        padding 0; row qualities `qual` everywhere"""
        rank, base_row = self._draft_rank()
        lab = np.where(base_row, np.where(rank >= 0, 1 + rank, 1), 0).astype(np.uint8)
        return lab, np.full(self.position.shape, qual, np.uint8)

    def plant(self, lab, rq, g: int, r: int, what, q: int):
        """an edit on every copy of row r of region g: what = 'sub' (the next base after the draft's), 'del', or a label
        0..4 as it is; quality q"""
        p, x = self.rows[g][r]
        if what == "sub":
            assert x == 0
            u = upper(self.draft(g, p))
            what = 1 + (BASES.index(u) + 1) % 4 if u in BASES else 2
        elif what == "del":
            what = 0
        at = self.where(g, r)
        lab[at], rq[at] = what, q

    def all_edited(self, qual: int = 60):
        """every row an edit: a substitution on every base row (the next base after the draft's, C over a byte that cannot
        be spelled), an inserted base on every insert row"""
        rank, base_row = self._draft_rank()
        lab = np.where(base_row, np.where(rank >= 0, 1 + (rank + 1) % 4, 2), 0)
        lab = np.where(self.index > 0, 1 + (self.position + self.index) % 4, lab).astype(np.uint8)
        return lab, np.full(self.position.shape, qual, np.uint8)


def acgt(rng, n: int, lower: float = 0.3) -> bytes:
    d = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    d[rng.random(n) < lower] += 32
    return d.astype(np.uint8).tobytes()
