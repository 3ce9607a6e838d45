"""Read batches that take the run vote (pv_polish_vote_runs, csrc/polish_vote_runs.hip) to the limits of its own kernels,
built on vote_runs_cases.py. What a case reaches is worked out here from the header's rule and plain arithmetic on the
constants below, never from a kernel's output; tests/test_polish_vote_runs_limits_cpu.py asserts it case by case, so a case that
is edited away from its limit fails there, and tests/test_polish_vote_runs_limits_gpu.py runs every case on the device.

A tile is TILE flat draft bytes (ref_off + offset, all regions of the batch one behind the other) and owns the runs that start in
it; a region's reads are looked at ROUND at a time in batch order, and a tile keeps of a round the reads that can hold a flank
of one of its runs: mapping quality above 0 and a base or deleted column inside [a - 1, b + MAX_RUN] for the tile's draft
positions [a, b] inside the region (a voter has an aligned base at s - 1 >= a - 1 and at e + 1 <= b + MAX_RUN).
"""
import functools
import types
from typing import Dict, List, Sequence, Tuple

import numpy as np

import vote_runs_cases as rc
import vote_runs_ref as rr
from pepper_thesis_amd.batch import Read, Region, pack_cigar, pack_regions

TILE = 256          # draft bytes per workgroup of k_runs_vote (VR_THREADS)
ROUND = 256         # reads compacted at a time
SLOTS = 88          # runs that may start in one tile (VR_SLOTS)
MAX_RUN = 48        # longest candidate
MAX_LEN = 63        # longest length a read may show and still vote
M, I, D, N, S, H, P, EQ, X = range(9)         # BAM CIGAR codes
L, O = 64, 8                                  # the chunk geometry of every case but `geometries`


# ---- arithmetic on a batch ------------------------------------------------------------------------------------------------------

def read_span(batch, r: int) -> Tuple[int, int]:
    """[first, behind the last) draft position read r covers with a base or a deleted column"""
    rp = int(batch.read_pos[r])
    end = rp
    for w in batch.cigar[int(batch.cigar_off[r]):int(batch.cigar_off[r + 1])]:
        if int(w) & 0xF in rr.ALIGNED + rr.DRAFT_ONLY:
            end += int(w) >> 4
    return rp, end


def spans(read: Read, s: int, n: int) -> bool:
    """the read has an aligned base at both flanks of the run [s, s + n)"""
    at = rr.aligned_offsets(read.pos, read.cigar)
    return s - 1 in at and s + n in at


def overlaps(read: Read, s: int, n: int) -> bool:
    b = types.SimpleNamespace(read_pos=[read.pos], cigar=read.cigar, cigar_off=[0, len(read.cigar)])
    first, end = read_span(b, 0)
    return first < s + n and end > s


def flat(batch, run: rr.Run) -> int:
    """the flat draft byte of a run's first base"""
    return int(batch.ref_off[run.region]) + run.s - int(batch.ref_start[run.region])


def tile_of(batch, run: rr.Run) -> int:
    return flat(batch, run) // TILE


def all_runs(batch, min_run: int = 3):
    """-> (the runs voted on with their votes, candidates seen, skipped) over all regions"""
    runs, seen, skipped = [], 0, 0
    for g in range(batch.n_regions):
        r, a, b = rr.region_runs(batch, g, min_run)
        runs, seen, skipped = runs + r, seen + a, skipped + b
    return runs, seen, skipped


def runs_per_tile(batch, min_run: int = 3) -> Dict[int, int]:
    out: Dict[int, int] = {}
    for r in all_runs(batch, min_run)[0]:
        out[tile_of(batch, r)] = out.get(tile_of(batch, r), 0) + 1
    return out


def kept_per_round(batch, g: int, tile: int) -> List[int]:
    """how many reads of each round of region g the tile keeps (see the module text); [] where the tile holds none of g"""
    lo, hi, rs = int(batch.ref_off[g]), int(batch.ref_off[g + 1]), int(batch.ref_start[g])
    t0, t1 = max(tile * TILE, lo), min((tile + 1) * TILE, hi)
    if t0 >= t1:
        return []
    a, b = rs + t0 - lo, rs + t1 - 1 - lo
    r0, r1 = int(batch.read_off[g]), int(batch.read_off[g + 1])
    out = []
    for rb in range(r0, r1, ROUND):
        n = 0
        for r in range(rb, min(rb + ROUND, r1)):
            first, end = read_span(batch, r)
            n += int(batch.read_mapq[r]) > 0 and first <= b + MAX_RUN and end > a - 1
        out.append(n)
    return out


def first_reads(batch, k: int):
    """the batch with only the first k reads of every region"""
    regs = []
    for g in range(batch.n_regions):
        reg = batch.region(g)
        reg.reads = reg.reads[:k]
        regs.append(reg)
    return pack_regions(regs)


def flat_rows(lay, g: int = 0) -> Dict[Tuple[int, int], int]:
    """(position, index) -> flat row inside region g of a min_qual_cases.Layout"""
    return {key: i for i, key in enumerate(lay.rows[g])}


def span_rows(lay, run: rr.Run) -> List[int]:
    """the flat rows of a run's span: its base rows and the insert rows from its left flank on"""
    e = run.s + run.n - 1
    return sorted(i for (p, x), i in flat_rows(lay, run.region).items() if run.s <= p <= e or (p == run.s - 1 and x > 0))


# ---- reads from explicit CIGAR words ----------------------------------------------------------------------------------------------

def read_words(draft: str, start: int, a: int, words: Sequence[tuple], **kw) -> Read:
    """the read at draft offset a with the CIGAR words (op, length[, bases]): M, = and X show the draft's letters unless bases
    are given, I and S show `bases` (S: T's by default); D, N and P move over the draft, H over nothing"""
    seq, i, ops = [], a, []
    for w in words:
        op, n = w[0], w[1]
        text = w[2] if len(w) > 2 else None
        assert text is None or len(text) == n
        if op in (M, EQ, X):
            seq.append(text or draft[i:i + n].upper())
            i += n
        elif op in (I, S):
            assert text is not None or op == S
            seq.append(text or "T" * n)
        elif op in (D, N, P):
            i += n
        ops.append((op, n))
    assert i <= len(draft)
    return Read.make(start + a, pack_cigar(ops), "".join(seq), **kw)


def _merge(*edits):
    out = {}
    for e in edits:
        assert not set(e) & set(out)
        out.update(e)
    return out


class Case(types.SimpleNamespace):
    """batch, min_run, L, O, and whatever the CPU test wants to know about the case"""

    def __init__(self, batch, min_run=3, L_=L, O_=O, **more):
        super().__init__(batch=batch, min_run=min_run, L=L_, O=O_, **more)

    @functools.cached_property
    def runs(self):
        return all_runs(self.batch, self.min_run)


# ---- rounds ------------------------------------------------------------------------------------------------------------------------

ROUNDS_START = 5000
ROUNDS_RUNS = {40: ("A", 5), 250: ("C", 8), 262: ("G", 4)}


@functools.lru_cache(maxsize=None)
def rounds() -> Case:
    """one region of 300 bytes (tiles of 256 and 44), 600 reads in rounds of 256, 256 and 88. Round 0 ends at 240: tile 1 keeps
    none of it. Round 1 covers everything with mapping quality 60: both tiles keep all 256. Round 2 alternates whole reads
    and reads that start at 259..261, behind tile 0's runs. A quarter of rounds 0 and 2 has mapping quality 0 (round 1 cannot:
    it has to be kept whole). The lengths shown differ from round to round: A x 5 is 4 by round 0 alone and 5 by all reads, C x 8
    is 7 by round 1 alone and 9 with round 2, G x 4 ties in round 1 and is 3 by round 2."""
    rng = np.random.default_rng(101)
    draft = rc.draft_with_runs(rng, 300, ROUNDS_RUNS)
    reads = []
    for i in range(600):
        rnd = i // ROUND
        if rnd == 0:
            a, b, mapq = 0, 240, 0 if i % 4 == 3 else 60
            ed = rc.run_edits(40, 5, "A", (4, 4, 4, 5, 6)[i % 5], (39, 41, 44)[i % 3])
        elif rnd == 1:
            a, b, mapq = 0, 300, 60
            ed = _merge(rc.run_edits(40, 5, "A", 4 if i % 4 == 0 else 5),
                        rc.run_edits(250, 8, "C", (7, 8, 9)[i % 3], (249, 252, 257)[(i // 3) % 3]),
                        rc.run_edits(262, 4, "G", (3, 4)[i % 2]))
        elif i % 2 == 0:
            a, b, mapq = 0, 300, 0 if i % 8 == 6 else 60
            ed = _merge(rc.run_edits(40, 5, "A", 6, 42), rc.run_edits(250, 8, "C", 9, (249, 255)[(i // 2) % 2]),
                        rc.run_edits(262, 4, "G", 3))
        else:
            a, b, mapq = 259 + (i // 2) % 3, 300, 0 if i % 8 == 3 else 60
            ed = rc.run_edits(262, 4, "G", 3)
        reads.append(rc.read_over(draft, ROUNDS_START, a, b, ed, is_reverse=bool(i % 2), mapq=mapq))
    return Case(rc.one_region(draft, reads, ROUNDS_START), draft=draft)


ROUND_COUNTS = (255, 256, 257)


@functools.lru_cache(maxsize=None)
def round_counts() -> Case:
    """three regions with exactly 255, 256 and 257 voting reads over one run T x 6: even reads show 5, odd reads 6, so the
    winner is 5, 6 (a tie goes to n) and 5: the 257th read decides, and it is alone in its round. Behind every 50th voter
    sits a read of mapping quality 0 that shows 3, so a round's reads and the reads it keeps are not the same."""
    rng = np.random.default_rng(102)
    regs = []
    for g, count in enumerate(ROUND_COUNTS):
        draft = rc.draft_with_runs(rng, 60, {25: ("T", 6)})
        reads = []
        for i in range(count):
            reads.append(rc.read_over(draft, 1000 * g, 0, 60, rc.run_edits(25, 6, "T", 5 if i % 2 == 0 else 6), is_reverse=bool(i % 2)))
            if i % 50 == 49:
                reads.append(rc.read_over(draft, 1000 * g, 0, 60, rc.run_edits(25, 6, "T", 3), mapq=0))
        regs.append(Region(1000 * g, 1000 * g + 59, draft.encode(), reads))
    return Case(pack_regions(regs))


# ---- slots --------------------------------------------------------------------------------------------------------------------------

SLOTS_DRAFT = ("T" + "AACGGTCCATTG" * 60)[:700]
SLOTS_PER_TILE = (85, 86, 62)


def _slots_length(i: int, k: int) -> int:
    """what read i shows for run k: most reads 7 k mod 5, the others something else"""
    base = (7 * k) % 5
    return base if i < 6 + k % 3 else (base + i) % 5


@functools.lru_cache(maxsize=None)
def slots(min_run: int = 2) -> Case:
    """runs of two with one byte between them, four in twelve bytes: 85, 86 and 62 start in the three tiles. Twelve whole reads,
    every run's histogram its own."""
    draft = SLOTS_DRAFT
    runs = [(s, n, b) for s, n, b in rr.stretches(draft.encode()) if n == 2 and s > 0 and s + n < len(draft)]
    reads = []
    for i in range(12):
        ed = _merge(*(rc.run_edits(s, 2, b, _slots_length(i, k)) for k, (s, n, b) in enumerate(runs)))
        reads.append(rc.read_over(draft, 0, 0, len(draft), ed, is_reverse=bool(i % 2)))
    return Case(rc.one_region(draft, reads), min_run=min_run, draft=draft)


@functools.lru_cache(maxsize=None)
def small() -> Case:
    """one small region: what runs between the two `slots` batches of the workspace test"""
    rng = np.random.default_rng(103)
    draft = rc.draft_with_runs(rng, 90, {20: ("C", 4), 50: ("G", 6)})
    reads = [rc.read_over(draft, 300, 0, 90, _merge(rc.run_edits(20, 4, "C", 5 if i < 5 else 4), rc.run_edits(50, 6, "G", 5)),
                          is_reverse=bool(i % 2)) for i in range(7)]
    return Case(rc.one_region(draft, reads, 300))


# ---- tile edges --------------------------------------------------------------------------------------------------------------------

# offset: (letter, n, what the majority of the ten reads shows; None: no candidate), in one region of 1600 bytes at flat offset 0
EDGE_RUNS = {
    208: ("A", 48, 50),      # ends on tile 0's last byte; the right flank is tile 1's first
    300: ("C", 49, None),
    360: ("G", 96, None),
    511: ("T", 6, 5),        # starts on tile 1's last byte
    530: ("A", 97, None),
    768: ("G", 5, 7),        # starts on tile 3's first byte; the left flank is tile 2's last
    1000: ("C", 48, 48),     # crosses byte 1024; owned by tile 3
    1100: ("T", 200, None),  # crosses byte 1280; one byte behind it:
    1301: ("C", 3, 2),       # ... a candidate that is not adjacent to one
    1532: ("A", 4, None),    # two candidates that touch at byte 1536: both skipped
    1536: ("G", 4, None),
}
EDGE_ANCHORS = {208: (207, 230), 768: (767, 770)}      # where the reads that show n + 2 hold the two inserted letters


@functools.lru_cache(maxsize=None)
def tile_edges() -> Case:
    rng = np.random.default_rng(104)
    draft = rc.draft_with_runs(rng, 1600, {off: (b, n) for off, (b, n, _) in EDGE_RUNS.items()})
    reads = []
    for i in range(10):
        ed = {}
        for off, (b, n, major) in EDGE_RUNS.items():
            if major is not None:
                anchors = EDGE_ANCHORS.get(off)
                ed.update(rc.run_edits(off, n, b, major if i < 6 else n, anchors and anchors[i % 2]))
        reads.append(rc.read_over(draft, 0, 0, 1600, ed, is_reverse=bool(i % 2)))
    return Case(rc.one_region(draft, reads), draft=draft)


# ---- regions inside a tile ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def regions_in_a_tile(across: bool) -> Case:
    """seven regions. Their flat offsets are 0, 42, 92, 142, 192, 256, 316 (region 5 starts tile 1), or with `across` 0, 42, 79,
    129, 179, 243, 303 (region 5 lies across byte 256).
    0: C A x 40 G: the run's flanks are the region's first and last byte; 1: a run and no reads; 2: a run and reads of mapping
    quality 0 only; 3: reads and no candidate; 4 ends in CAAA and 5 begins with AAAT: neither AAA is a candidate, and in the
    flat draft they are six A's in a row; 5 and 6 overlap on the draft ([5000, 5060) and [5020, 5080)) and hold the same run
    G x 5 at 5030: 5's reads show 4, 6's reads show 7."""
    rng = np.random.default_rng(105)

    def whole(draft, start, count, edits, **kw):
        return [rc.read_over(draft, start, 0, len(draft), edits(i), is_reverse=bool(i % 2), **kw) for i in range(count)]
    d0 = "C" + "A" * 40 + "G"
    d1 = rc.draft_with_runs(rng, 37 if across else 50, {10: ("G", 4)})
    d2 = rc.draft_with_runs(rng, 50, {20: ("T", 5)})
    d3 = rc.plain(rng, 50)
    d4 = rc.draft_with_runs(rng, 61, {30: ("G", 4), 60: ("C", 1)}) + "AAA"
    d5 = "AAA" + rc.draft_with_runs(rng, 57, {0: ("T", 1), 27: ("G", 5)})
    d6 = d5[20:] + rc.plain(rng, 20, d5[-1])
    assert d5[30:35] == "GGGGG" and d6[10:15] == "GGGGG"
    sub3 = "ACGT"[("ACGT".index(d3[25]) + 1) % 4]
    regs = [
        Region(100, 141, d0.encode(), whole(d0, 100, 8, lambda i: rc.run_edits(1, 40, "A", 39 if i < 6 else 40))),
        Region(1000, 1000 + len(d1) - 1, d1.encode(), []),
        Region(2000, 2049, d2.encode(), whole(d2, 2000, 5, lambda i: rc.run_edits(20, 5, "T", 4), mapq=0)),
        Region(3000, 3049, d3.encode(), whole(d3, 3000, 4, lambda i: {25: ("sub", sub3)})),
        Region(4000, 4063, d4.encode(), whole(d4, 4000, 6, lambda i: _merge(rc.run_edits(30, 4, "G", 3), {61: ("del", 1)} if i < 4 else {}))),
        Region(5000, 5059, d5.encode(), whole(d5, 5000, 7, lambda i: _merge(rc.run_edits(30, 5, "G", 4), {1: ("del", 1)} if i < 4 else {}))),
        Region(5020, 5079, d6.encode(), whole(d6, 5020, 7, lambda i: rc.run_edits(10, 5, "G", 7, (9, 12)[i % 2]))),
    ]
    return Case(pack_regions(regs), seen=[1, 1, 1, 0, 1, 1, 1], decided=[1, 0, 0, 0, 1, 1, 1])


# ---- CIGAR words ---------------------------------------------------------------------------------------------------------------------

WORDS_START = 2000
WORDS_RUNS = {40: ("A", 6), 100: ("C", 5), 160: ("G", 4)}


def _alternating(a: int, b: int):
    return [((M, EQ, X)[i % 3], 1) for i in range(a, b)]


# kind -> [(draft offset of the read's first base or deleted column, words)]
WORDS_KINDS = {
    "soft_clips": [(0, [(S, 5), (M, 220), (S, 7)]), (40, [(S, 5), (M, 180), (S, 7)])],
    "hard_clips": [(0, [(H, 9), (M, 220), (H, 4)]), (161, [(H, 9), (M, 59)])],
    "one_base_words": [(0, _alternating(0, 220)), (0, _alternating(0, 41) + [(D, 1)] + _alternating(42, 220)), (0, _alternating(0, 103))],
    "x_flank_with_the_runs_letter": [(0, [(M, 39), (X, 1, "A"), (M, 180)]), (39, [(X, 1, "A"), (M, 5)])],
    "n_over_the_left_flank": [(0, [(M, 39), (N, 1), (M, 180)])],
    "n_and_d_inside_a_run": [(0, [(M, 42), (N, 1), (M, 1), (D, 1), (M, 175)]), (0, [(M, 42), (N, 1), (M, 1), (D, 3), (M, 173)])],
    "p_in_front_of_a_run": [(0, [(M, 38), (P, 1), (M, 181)]), (0, [(M, 39), (P, 1), (M, 180)])],
    "i_first_behind_s": [(39, [(S, 3), (I, 2, "AA"), (M, 181)]), (40, [(S, 3), (I, 2, "AA"), (M, 180)])],
    "i_outside_the_flanks": [(0, [(M, 39), (I, 1, "A"), (M, 8), (I, 1, "A"), (M, 173)]), (0, [(M, 39), (I, 1, "A"), (M, 5)])],
    "i_inside_the_flanks": [(0, [(M, 40), (I, 1, "A"), (M, 6), (I, 1, "A"), (M, 174)]), (0, [(M, 40), (I, 1, "A"), (M, 6), (I, 1, "A")])],
    "d_over_the_right_flank": [(0, [(M, 46), (D, 1), (M, 173)])],
    "one_word": [(38, [(M, 10)]), (40, [(M, 8)])],
}
# what the first read of a kind shows for A x 6 at 40 (None: it does not span the run, "impure": it spans and does not vote)
WORDS_SHOWN = {"soft_clips": 6, "hard_clips": 6, "one_base_words": 6, "x_flank_with_the_runs_letter": "impure", "n_over_the_left_flank": None,
               "n_and_d_inside_a_run": 4, "p_in_front_of_a_run": 6, "i_first_behind_s": 6, "i_outside_the_flanks": 6,
               "i_inside_the_flanks": 8, "d_over_the_right_flank": None, "one_word": 6}


@functools.lru_cache(maxsize=None)
def cigar_words() -> Case:
    """one region of 220 bytes with three runs; the reads of WORDS_KINDS, and behind them twenty ordinary reads that show 7, 4
    and 4 for the runs, so that every run is decided against most of the hand-made reads"""
    rng = np.random.default_rng(106)
    draft = rc.draft_with_runs(rng, 220, WORDS_RUNS)
    kinds = {k: [read_words(draft, WORDS_START, a, w, is_reverse=bool(j % 2)) for j, (a, w) in enumerate(v)] for k, v in WORDS_KINDS.items()}
    reads = [r for v in kinds.values() for r in v]
    for i in range(20):
        ed = _merge(rc.run_edits(40, 6, "A", 7, (39, 42, 45)[i % 3]), rc.run_edits(100, 5, "C", 4))
        reads.append(rc.read_over(draft, WORDS_START, 0, 220, ed, is_reverse=bool(i % 2)))
    return Case(rc.one_region(draft, reads, WORDS_START), draft=draft, kinds=kinds)


# ---- chunk geometries ------------------------------------------------------------------------------------------------------------------

def geometry_runs(L_: int, O_: int) -> Dict[str, int]:
    """{what the run does: draft offset} of three runs of three letters. The grown run gets four insert rows (two behind each
    of the anchors s - 1 and s + 1), so with them it takes seven flat rows; no other run gives rise to an insert row.
    L >= 16, O >= 19: the shrinking run lies across flat rows step - 1 | step, the kept one inside chunk 0's overlap with chunk 1,
        the grown one ends on row L - 1 of chunk 0: its insert rows push its last base there and everything behind it on.
    L >= 16, O < 11:  the grown run comes first and ends on row L - 1; the shrinking one lies across rows 2 step - 1 | 2 step (four
        draft bytes earlier than that, for the insert rows in front of it), the kept one behind it.
    L < 16: every run lies in several chunks wherever it is."""
    step = L_ - O_
    if L_ < 16:
        return {"shrink": 10, "keep": 20, "grow": 30}
    if O_ >= 19:
        return {"shrink": step - 1, "keep": step + 4, "grow": L_ - 7}
    assert O_ < 11
    return {"grow": L_ - 7, "shrink": 2 * step - 1 - 4, "keep": 2 * step + 6}


GEOMETRY_LETTERS = {"shrink": "A", "keep": "C", "grow": "G"}


@functools.lru_cache(maxsize=None)
def geometry(L_: int, O_: int) -> Case:
    rng = np.random.default_rng(1000 * L_ + O_)
    where = geometry_runs(L_, O_)
    length = max(3 * L_, 200)
    draft = rc.draft_with_runs(rng, length, {off: (GEOMETRY_LETTERS[k], 3) for k, off in where.items()})
    reads = []
    for i in range(8):
        g = where["grow"]
        ed = _merge(rc.run_edits(where["shrink"], 3, "A", 2 if i < 5 else 3), rc.run_edits(where["keep"], 3, "C", 2 if i < 2 else 3),
                    rc.run_edits(g, 3, "G", 5 if i < 6 else 3, g - 1 if i < 3 else g + 1))
        reads.append(rc.read_over(draft, 0, 0, length, ed, is_reverse=bool(i % 2)))
    return Case(rc.one_region(draft, reads), L_=L_, O_=O_, where=where)


# ---- a layout that is short of insert rows ------------------------------------------------------------------------------------------

STATE_START = 700


@functools.lru_cache(maxsize=None)
def state() -> Case:
    """C x 4 at 30, which every read shows as 3, and A x 5 at 70, which every read shows as 7 with both inserted letters behind
    the left flank: the winner needs two insert rows there. `short` holds one, `enough` two (regions for min_qual_cases.Layout)."""
    rng = np.random.default_rng(107)
    draft = rc.draft_with_runs(rng, 120, {30: ("C", 4), 70: ("A", 5)})
    reads = [rc.read_over(draft, STATE_START, 0, 120, _merge(rc.run_edits(30, 4, "C", 3), rc.run_edits(70, 5, "A", 7)), is_reverse=bool(i % 2))
             for i in range(8)]
    at = STATE_START + 69
    return Case(rc.one_region(draft, reads, STATE_START), short=[(STATE_START, draft.encode(), {at: 1})],
                enough=[(STATE_START, draft.encode(), {at: 2})])
