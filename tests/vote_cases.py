"""Hand-computed rows for the majority vote (include/pepper_hip.h, pv_polish_vote), shared by the CPU and the GPU tests, and
the planting of counts planes on the hand-made layouts of min_qual_cases."""
import numpy as np


def row(a=0, c=0, g=0, t=0, other=0):
    """ten counts with these reads behind A, C, G, T and the deleted / not-ACGT planes: half of each (rounded down) on the
    reverse strand, the rest on the forward strand"""
    v = [a, c, g, t]
    return [x // 2 for x in v] + [x - x // 2 for x in v] + [other // 2, other - other // 2]


# (name, ten counts, draft byte, expected label, expected n[0..4]) of base rows (index 0); the depth is not looked at
BASE_ROWS = [
    ("tie AC, draft A in it", row(a=5, c=5), b"A", 1, [0, 5, 5, 0, 0]),
    ("tie AC, draft C in it", row(a=5, c=5), b"C", 2, [0, 5, 5, 0, 0]),
    ("tie AC, draft G outside", row(a=5, c=5), b"G", 1, [0, 5, 5, 0, 0]),
    ("tie CT, draft A outside", row(c=5, t=5), b"A", 2, [0, 0, 5, 0, 5]),
    ("tie GT, draft T in it", row(g=4, t=4), b"T", 4, [0, 0, 0, 4, 4]),
    ("tie AT, draft T in it", row(a=4, t=4), b"T", 4, [0, 4, 0, 0, 4]),
    ("tie ACG, draft T outside", row(a=3, c=3, g=3, t=1), b"T", 1, [0, 3, 3, 3, 1]),
    ("tie CGT, draft g in it (lower case)", row(c=2, g=2, t=2), b"g", 3, [0, 0, 2, 2, 2]),
    ("tie CGT, draft A outside", row(a=1, c=2, g=2, t=2), b"A", 2, [0, 1, 2, 2, 2]),
    ("tie ACGT, draft G in it", row(a=3, c=3, g=3, t=3), b"G", 3, [0, 3, 3, 3, 3]),
    ("tie ACGT, draft N", row(a=3, c=3, g=3, t=3), b"N", 1, [0, 3, 3, 3, 3]),
    ("tie GT, draft n", row(g=3, t=3), b"n", 3, [0, 0, 0, 3, 3]),
    ("deletion level with C, draft A", row(c=5, other=5), b"A", 2, [5, 0, 5, 0, 0]),
    ("deletion level with the draft's A", row(a=5, other=5), b"A", 1, [5, 5, 0, 0, 0]),
    ("deletion level with G and T, draft T", row(g=5, t=5, other=5), b"T", 4, [5, 0, 0, 5, 5]),
    ("deletion strictly ahead", row(c=5, other=6), b"C", 0, [6, 0, 5, 0, 0]),
    ("deletion alone", row(other=1), b"A", 0, [1, 0, 0, 0, 0]),
    ("a single winner that is not the draft", row(a=2, t=7), b"A", 4, [0, 2, 0, 0, 7]),
    ("a single winner that is the draft", row(a=2, t=7), b"t", 4, [0, 2, 0, 0, 7]),
    ("one strand only", [0, 0, 0, 0, 0, 0, 9, 0, 0, 0], b"A", 3, [0, 0, 0, 9, 0]),
    ("no reads, draft G", row(), b"G", 3, [0, 0, 0, 0, 0]),
    ("no reads, draft c (lower case)", row(), b"c", 2, [0, 0, 0, 0, 0]),
    ("no reads, draft N: no label spells it", row(), b"N", 0, [0, 0, 0, 0, 0]),
]

# (name, ten counts, depth of the anchor, expected label, expected n[0..4]) of insert rows (index > 0)
INSERT_ROWS = [
    ("half the reads insert A: nothing wins the tie", row(a=3), 6, 0, [3, 3, 0, 0, 0]),
    ("most reads insert A", row(a=4), 6, 1, [2, 4, 0, 0, 0]),
    ("tie of inserted A and C ahead of nothing", row(a=2, c=2), 5, 1, [1, 2, 2, 0, 0]),
    ("tie of inserted G and T", row(g=3, t=3), 6, 3, [0, 0, 0, 3, 3]),
    ("depth below the sum of the counts", row(c=3, g=3), 5, 2, [0, 0, 3, 3, 0]),
    ("depth below the sum, not-ACGT bytes still count", row(c=3, g=2, other=2), 5, 2, [2, 0, 3, 2, 0]),
    ("not-ACGT bytes level with C", row(c=3, other=3), 6, 0, [3, 0, 3, 0, 0]),
    ("nothing inserted by any read", row(), 10, 0, [10, 0, 0, 0, 0]),
    ("no reads at all", row(), 0, 0, [0, 0, 0, 0, 0]),
]


def keyed(lay, table_of):
    """values that are functions of (region, position, index), so that the copies of a row agree: table_of(size) -> a table"""
    top = int(lay.position.max()) + 1
    g = np.broadcast_to(lay.region[:, None], lay.position.shape)
    key = (g * top + np.maximum(lay.position, 0)) * 8 + np.maximum(lay.index, 0)
    return table_of(int(key.max()) + 1)[key]


def random_planes(lay, rng, top=41):
    """counts uint16 [n, L, 10] with values below `top` and depth uint16 [n, L], equal on the copies of a row, zero on padding.
    A base row's depth is the sum of its counts (the builder's invariant); an insert row's is drawn around the sum of its own
    counts, so that it is above, equal and below; a third of the rows repeat one value in several planes, for ties."""
    counts = np.stack([keyed(lay, lambda m: rng.integers(0, top, m)) for _ in range(10)], -1).astype(np.int64)
    tied = keyed(lay, lambda m: rng.random(m) < 0.35)
    same = keyed(lay, lambda m: rng.integers(0, min(top, 4), m))
    mask = np.stack([keyed(lay, lambda m: rng.random(m) < 0.6) for _ in range(10)], -1)
    counts = np.where(tied[..., None], np.where(mask, same[..., None], 0), counts)
    empty = keyed(lay, lambda m: rng.random(m) < 0.05)
    counts[empty] = 0
    pad = (lay.position < 0) | (lay.index < 0)
    counts[pad] = 0
    total = counts.sum(-1)
    around = total + keyed(lay, lambda m: rng.integers(-6, 12, m))
    depth = np.where(lay.index > 0, np.clip(around, 0, 65535), np.minimum(total, 65535))
    depth[pad] = 0
    return counts.astype(np.uint16), depth.astype(np.uint16)


def plant(lay, counts, depth, g, r, ten, d=None):
    """ten counts (and a depth; None: their sum) on every copy of row r of region g"""
    at = lay.where(g, r)
    counts[at] = np.asarray(ten, np.uint16)
    depth[at] = min(65535, int(sum(ten))) if d is None else d
