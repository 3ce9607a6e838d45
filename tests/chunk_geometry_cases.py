"""Chunk batches at every chunk geometry the polisher's chunk passes accept (row qualities, minimum-depth mask, minimum-quality
filter, stitch, stitch with qualities, edits), with what the host checkers make of them.

A case is a min_qual_cases.Layout of three regions (one at 0, two that start later and lose their first 200 positions, one
of them with insert rows) with random labels that disagree between the two copies of every shared column, row qualities that
disagree there too, a depth plane on which the copies agree, and softmax sums with qual_ref.threshold_rows() on the batch's
first rows. Case holds the inputs read-only and computes every checker result once, on first use, so that the tests of one
geometry share them.

The one-block folds split n chunks into ceil(n / 1024) per thread: count_case(n) gives 8 / 4 batches of n chunks; the
decimal string order of chunk ids differs from the numeric one where the digit count grows: decade_layout() has a region of
1024 chunks.
"""
import functools
import types

import numpy as np

import depth_ref as dr
import edits_ref as er
import min_qual_cases as mc
import min_qual_ref as mq
import qual_ref as qr
import stitch_ref as sr

THREADS, MAX_CPT = 256, 16           # polish_stitch_common.hpp: one block of 256 threads per chunk, cpt columns per thread
FOLD_THREADS = 1024                  # the one-block folds over all chunks
MIN_QUAL = 20

# (seq_length, seq_overlap): what each is there for
GEOMETRIES = [
    (1, 0),                                   # one column, one live thread, every row a chunk
    (2, 1),                                   # smallest 2 * O = L
    (7, 3),                                   # odd, under one wave
    (63, 31), (64, 32), (65, 32),             # the wave edge
    (255, 127), (256, 128), (257, 128),       # cpt 1 -> 2; at 257 only 129 threads have columns
    (513, 256),                               # cpt 3, 171 threads
    (1000, 0), (1000, 50), (1000, 500),       # the production length at both overlap ends
    (2049, 1024),                             # cpt 9
    (3840, 50),                               # cpt 15, exactly full
    (3841, 1920),                             # cpt 16: 240 full threads, one thread of one column, 15 idle
    (4095, 2047), (4096, 0), (4096, 50), (4096, 2048),      # the top of the range
]
CUT_SHORT = [(257, 128), (2049, 1024), (3841, 1920), (4095, 2047)]      # a thread whose columns end mid-way
RAGGED = CUT_SHORT + [(513, 256)]                                        # ... or threads without columns behind a full one
FULL = [(256, 128), (3840, 50), (4096, 0), (4096, 50), (4096, 2048)]    # every thread holds cpt columns


def geo_id(g) -> str:
    return "%d_%d" % tuple(g)


def cpt(L: int) -> int:
    return -(-L // THREADS)


def _draft(rng, n: int) -> bytes:
    d = np.frombuffer(mc.acgt(rng, n, lower=0.3), np.uint8).copy()
    d[rng.random(n) < 0.01] = ord("N")
    d[n // 2] = ord("n")
    return d.tobytes()


def geometry_layout(L: int, O: int, seed: int = 0) -> mc.Layout:
    """three regions of 3 * L rows or more (a few hundred at the least, so that a late region keeps something): a middle
    chunk with both neighbours exists in each. The second carries inserts of 1..3 rows at about one position in twenty."""
    rng = np.random.default_rng(1000 * L + O + seed)
    n0, n1 = max(3 * L, 300), max(3 * L, 420)
    ins = {700 + int(p): int(rng.integers(1, 4)) for p in np.flatnonzero(rng.random(n1) < 0.05)}
    return mc.Layout([(0, _draft(rng, n0), {}), (700, _draft(rng, n1), ins), (9_000, _draft(rng, n1 + 1), {})], L, O)


def shared_pairs(lay: mc.Layout) -> np.ndarray:
    """k of every pair (k, k + 1) of adjacent chunks of one region"""
    return np.flatnonzero(lay.region[1:] == lay.region[:-1])


def shared_columns(lay: mc.Layout):
    """the columns two chunks hold -> (k, j, k + 1, j - step) index arrays: row j of chunk k is row j - step of chunk k + 1"""
    L, O, step = lay.L, lay.O, lay.L - lay.O
    ks = shared_pairs(lay)
    if O == 0 or len(ks) == 0:
        e = np.zeros(0, np.int64)
        return e, e, e, e
    k = np.repeat(ks, O)
    i = np.tile(np.arange(O), len(ks))
    real = lay.position[k + 1, i] >= 0
    k, i = k[real], i[real]
    assert np.array_equal(lay.position[k, step + i], lay.position[k + 1, i]) and np.array_equal(lay.index[k, step + i], lay.index[k + 1, i])
    return k, step + i, k + 1, i


def make_inputs(lay: mc.Layout, seed: int):
    """-> labels, row qualities, depth, acc, {flat row: the hand-worked quality planted there}"""
    rng = np.random.default_rng(seed)
    n, L, O = lay.n, lay.L, lay.O
    labels = rng.integers(0, 5, (n, L)).astype(np.uint8)
    rq = rng.integers(0, 94, (n, L)).astype(np.uint8)
    # the two copies of a shared column: different labels in a fixed pattern (its phase moves from pair to pair, so that an
    # overlap of one column sees all of it): base / other base, base / none, none / base, base / other base
    k, j, k2, j2 = shared_columns(lay)
    t = j2 + k
    m, v = t % 4, (t // 4) % 4
    labels[k, j] = np.where(m == 2, 0, 1 + np.where(m == 3, (v + 2) % 4, v))
    labels[k2, j2] = np.where(m == 1, 0, 1 + np.where(m == 0, (v + 1) % 4, v))
    same = rq[k, j] == rq[k2, j2]
    rq[k2[same], j2[same]] = (rq[k2[same], j2[same]] + 1) % 94
    assert (rq[k, j] != rq[k2, j2]).all() and (labels[k, j] != labels[k2, j2]).all()
    # depth by (region, position, index): the copies of a row agree; padding rows 0
    top = int(lay.position.max()) + 1
    key = (lay.region[:, None] * top + np.maximum(lay.position, 0)) * 4 + np.maximum(lay.index, 0)
    depth = rng.integers(0, 10, int(key.max()) + 1)[key].astype(np.uint16)
    depth[lay.position < 0] = 0
    # softmax sums in [0, 2], half of the rows confident; the rows around the thresholds on the first rows of either count
    acc = (rng.random((n, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
    near = rng.random((n, L)) < 0.5
    acc[near] = np.float32(2.0) - (np.float32(10.0) ** -(rng.random((int(near.sum()), 5), dtype=np.float32) * 9)).astype(np.float32)
    planted = plant_thresholds(labels, acc, O)
    return labels, rq, depth, acc, planted


def plant_thresholds(labels, acc, O: int):
    """qual_ref.threshold_rows() on the first rows of the batch for each count the geometry has, under the label the row has
    -> {flat row: expected quality}"""
    n, L = labels.shape
    cnt = np.tile(qr.row_counts(L, O), n)
    flat_acc, flat_lab = acc.reshape(-1, 5), labels.reshape(-1)
    planted = {}
    for c in (1.0, 2.0):
        mine = [r for r in qr.threshold_rows() if r[2] == c]
        for t, (_, v, _, q) in zip(np.flatnonzero(cnt == c)[:len(mine)].tolist(), mine):
            flat_acc[t, flat_lab[t]] = v
            planted[t] = q
    return planted


class Case:
    """a layout with its inputs (read-only) and, on first use, what the checkers make of them"""

    def __init__(self, lay: mc.Layout, labels, rq, depth=None, acc=None, planted=None):
        self.lay, self.labels, self.rq, self.depth, self.acc, self.planted = lay, labels, rq, depth, acc, planted
        for a in (labels, rq, depth, acc):
            if a is not None:
                a.setflags(write=False)
        self.chunks = lay.out if depth is None else types.SimpleNamespace(depth=depth, **vars(lay.out))

    @property
    def spans(self):
        return list(zip(self.lay.ref_start.tolist(), self.lay.ref_end.tolist()))

    def region_draft(self, g: int) -> bytes:
        return self.lay.ref[int(self.lay.ref_off[g]):int(self.lay.ref_off[g + 1])].tobytes()

    def contig_draft(self, g: int) -> bytes:
        """region g's draft as a contig of its own: positions below the region's start filled in"""
        return b"A" * int(self.lay.ref_start[g]) + self.region_draft(g)

    def cut(self, g: int):
        """what the stitch leaves out of contig_draft(g): the filler and the 200-position buffer of a late region"""
        s = int(self.lay.ref_start[g])
        return [(0, s + sr.BUFFER_POSITIONS)] if s > 0 else []

    @functools.cached_property
    def stitch_seq(self):
        """stitch_ref.create_consensus_sequence per region"""
        lay = self.lay
        regs = sr.regions_from_chunks(lay.position, lay.index, lay.region, lay.chunk_id, self.labels, self.spans)
        return [sr.create_consensus_sequence([r]).encode() for r in regs]

    @functools.cached_property
    def stitch_qual(self):
        """qual_ref.create_consensus_qual per region -> [(bases, raw qualities)]"""
        lay = self.lay
        regs = qr.regions_with_qual(lay.position, lay.index, lay.region, lay.chunk_id, self.labels, self.rq, self.spans)
        return [(s.encode(), q) for s, q in (qr.create_consensus_qual([r]) for r in regs)]

    @functools.cached_property
    def dicts(self):
        lay = self.lay
        return er.region_dicts(lay.position, lay.index, lay.region, lay.chunk_id, self.labels, self.spans, self.rq)

    def edits(self, with_qual: bool):
        """edits_ref.primitive_edits per region -> (all records, region offsets); without row qualities every record
        carries 255"""
        per = self._edits_per_region
        if not with_qual:
            per = [[r[:5] + (255,) for r in p] for p in per]
        return [e for p in per for e in p], np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)

    @functools.cached_property
    def _edits_per_region(self):
        return [er.primitive_edits(d, self.region_draft(g), int(self.lay.ref_start[g])) for g, d in enumerate(self.dicts)]

    @functools.cached_property
    def min_depth(self) -> int:
        return int(np.median(self.depth[self.lay.position >= 0]))

    @functools.cached_property
    def masked(self):
        """depth_ref.mask at the median depth -> (labels, row qualities, masked rows, unmaskable rows)"""
        lay = self.lay
        return dr.mask(self.labels, self.rq, self.depth, lay.position, lay.index, lay.region, lay.ref_start, lay.ref_off, lay.ref,
                       self.min_depth)

    @functools.cached_property
    def filtered(self):
        """min_qual_ref.filter_low_qual at MIN_QUAL"""
        return mq.filter_low_qual(self.labels, self.rq, *self.lay.args(), MIN_QUAL)

    @functools.cached_property
    def owned(self):
        lay = self.lay
        return mq.owned_mask(lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, self.labels.shape)

    @functools.cached_property
    def chained(self) -> "Case":
        """the case behind mask and filter"""
        m_lab, m_q = self.masked[:2]
        f_lab, f_q, reverted, pinned, _ = mq.filter_low_qual(m_lab, m_q, *self.lay.args(), MIN_QUAL)
        out = Case(self.lay, f_lab, f_q)
        out.filter_counts = (reverted, pinned)
        return out


@functools.lru_cache(maxsize=None)
def geometry_case(L: int, O: int) -> Case:
    lay = geometry_layout(L, O)
    return Case(lay, *make_inputs(lay, 7 * L + O))


# ---- chunk counts at the one-block folds -------------------------------------------------------------------------------------

COUNT_L, COUNT_O = 8, 4
_COUNT_REGIONS = (1, 1, 1021, 1, 1, 1022, 1, 1)                  # chunks per region: every prefix ends at one of N_CHUNKS
N_CHUNKS = tuple(int(v) for v in np.cumsum(_COUNT_REGIONS))      # 1, 2, 1023, 1024, 1025, 2047, 2048, 2049


@functools.lru_cache(maxsize=None)
def count_case(n_chunks: int) -> Case:
    """an 8 / 4 batch of exactly n_chunks chunks: the regions of the 2049-chunk batch up to a region's end. The region of 1022
    chunks starts late (its first 50 chunks are buffer), every other at 0."""
    g = N_CHUNKS.index(n_chunks) + 1
    rng = np.random.default_rng(5)
    regs = [(500 if m == 1022 else 0, _draft(rng, 4 * m + 2), {}) for m in _COUNT_REGIONS]
    lay = mc.Layout(regs[:g], COUNT_L, COUNT_O)
    assert lay.n == n_chunks and [int((lay.region == r).sum()) for r in range(g)] == list(_COUNT_REGIONS[:g])
    return Case(lay, *make_inputs(lay, 90 + g))


# ---- chunk-id decade steps -----------------------------------------------------------------------------------------------------

DECADE_C = (8, 9, 10, 98, 99, 100, 998, 999, 1000)
DECADE_STRING_OWNER = (9, 99, 999)          # str(c) > str(c + 1): the earlier chunk owns what it shares with the next


@functools.lru_cache(maxsize=None)
def decade_layout() -> mc.Layout:
    """8 / 4: a region of 1024 chunks over an all-A draft and a short late one. Rows 4 (c + 1) .. 4 (c + 1) + 3 are columns
    4..7 of chunk c and columns 0..3 of chunk c + 1."""
    lay = mc.Layout([(0, b"A" * 4_100, {}), (300, b"A" * 260, {})], 8, 4)
    assert int((lay.region == 0).sum()) == 1024 and lay.chunk_id[:1024].tolist() == list(range(1024)) and lay.n == 1024 + 64
    return lay


def decade_labels(lay: mc.Layout) -> np.ndarray:
    """all 1 (the draft), but on the columns chunk c shares with chunk c + 1: 2 in chunk c, 3 in chunk c + 1"""
    labels = np.ones((lay.n, lay.L), np.uint8)
    for c in DECADE_C:
        labels[c, 4:], labels[c + 1, :4] = 2, 3
    return labels
