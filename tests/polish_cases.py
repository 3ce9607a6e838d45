"""Inputs that drive the polisher's image builder (csrc/summary_polish.hip behind the front end of summary_front.hip) to the
limits its kernels have, as plain Region lists: test_polish_limits_cpu.py pins the oracle on them, test_polish_limits_gpu.py
judges the kernels by it. Nothing here needs a GPU or looks at kernel output.

The limits are written as literals; each mirrors a constant of the kernels:
    512    TILE_COLS   columns of one tile = one workgroup of k_polish_tiles (summary_types.hpp)
    128    PT_PB       (read, tile) pairs that k_polish_tiles takes up per batch
    512    PT_THREADS  threads of k_polish_tiles = ops per trip of a pair batch
    256    TF_CAP      tiles a read may span in k_tile_fill's boundary table; beyond it the op ranges are searched
    65535  the 16-bit op offsets of that table (a read with more ops is searched too), and the clamp of the depth plane
    1024   columns per block of the insert-row scan (k_polish_blk, k_polish_insoff)
"""
import itertools

import numpy as np

from pepper_thesis_amd.batch import Read, Region

TILE = 512          # TILE_COLS
PAIR_BATCH = 128    # PT_PB
THREADS = 512       # PT_THREADS
TABLE_TILES = 256   # TF_CAP
TABLE_OPS = 65535   # 16-bit op offsets of k_tile_fill's table
DEPTH_MAX = 65535   # the uint16 depth plane
SCAN_BLOCK = 1024   # k_polish_blk / k_polish_insoff

REF_CONSUMING = (0, 2, 3, 6, 7, 8)   # M D N P = X
_ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgtnRY*", np.uint8)


_LETTERS = np.frombuffer(b"ACGTacgt", np.uint8)


def _seq(rng, n, alphabet=_ALPHABET) -> bytes:
    """n read bases: mostly ACGT, some N, lower case and other letters"""
    return rng.choice(alphabet, size=int(n)).astype(np.uint8).tobytes()


def _cigar(pairs) -> np.ndarray:
    """[(length, 'M'), ...] -> BAM words"""
    code = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
    return np.asarray([(int(n) << 4) | code[c] for n, c in pairs], np.uint32)


def _filler(n) -> Region:
    """a read-less region of n columns at position 0: moves every region behind it n columns along the batch's column index"""
    return Region(0, n - 1, b"A" * n, [])


# ---- what the inputs alone say about the workspace --------------------------------------------------------------------

def read_span(region: Region, rd: Read):
    """(lo, hi) region-relative: from the column before the read's first base (a leading insert is anchored there) to its
    last reference-consumed column, clipped to the region; None for a read of mapping quality 0 or one outside the region"""
    if rd.mapq == 0:
        return None
    R = region.ref_end - region.ref_start + 1
    cg = np.asarray(rd.cigar, np.int64)
    consumed = int((cg >> 4)[np.isin(cg & 15, REF_CONSUMING)].sum())
    lo = max(rd.pos - region.ref_start - 1, 0)
    hi = min(rd.pos - region.ref_start + consumed - 1, R - 1)
    return (lo, hi) if hi >= lo else None


def tiles_of_read(regions, g, rd) -> int:
    """512-column tiles of the batch's column index (regions laid end to end by the length of their reference buffers) that
    the read overlaps"""
    span = read_span(regions[g], rd)
    if span is None:
        return 0
    c0 = sum(len(r.ref) for r in regions[:g])
    return (c0 + span[1]) // TILE - (c0 + span[0]) // TILE + 1


def exact_pairs(regions) -> int:
    """(read, tile) pairs of the batch: one per tile a read overlaps"""
    return sum(tiles_of_read(regions, g, rd) for g, reg in enumerate(regions) for rd in reg.reads)


def exact_insert_rows(regions) -> int:
    """insert rows of the batch: per column the longest insert anchored on it by a read of mapping quality above 0; an insert
    counts while it starts at or before the region's end and its anchor lies in the region"""
    total = 0
    for reg in regions:
        longest = {}
        for rd in reg.reads:
            if rd.mapq == 0:
                continue
            rp = rd.pos
            for w in np.asarray(rd.cigar).tolist():
                op, ln = w & 15, w >> 4
                if rp > reg.ref_end:
                    break
                if op == 1 and reg.ref_start <= rp - 1 <= reg.ref_end:
                    longest[rp - 1] = max(longest.get(rp - 1, 0), ln)
                elif op in REF_CONSUMING:
                    rp += ln
        total += sum(longest.values())
    return total


def pair_heuristic(regions) -> int:
    """polish_limits' first bound on the pairs: 2 * (n_bases / 512) + 3 * n_reads + 64"""
    n_bases = sum(len(rd.bases) for reg in regions for rd in reg.reads)
    n_reads = sum(len(reg.reads) for reg in regions)
    return 2 * (n_bases // TILE) + 3 * n_reads + 64


def insert_heuristic(regions) -> int:
    """polish_limits' first bound on the insert rows: 2 * n_cols + 4096 (n_cols: bytes of the reference buffers)"""
    return 2 * sum(len(reg.ref) for reg in regions) + 4096


# ---- the cases ---------------------------------------------------------------------------------------------------------

def owner_tables():
    """k_polish_tiles' op -> base-slot tables. One region of 1500 columns behind 200 filler columns (tile edges at its
    columns 312, 824 and 1336), 426 reads: every tile holds four batches of 128 pairs. 140 one-op reads fill 512 slots of
    a tile each (the upper s_blk blocks); 140 reads of 1M1I1M units put about 768 ops per pair on a tile, far beyond the 512
    threads of a trip, each match padded from 1 or 2 slots to 4; 140 reads of 1M1D units alternate ops with and without
    slots (s_pref flat over every other op); six reads carry 300 one-base inserts in a row behind one column."""
    rng = np.random.default_rng(4701)
    R, S = 1500, 50_000
    reads = [Read.make(S, "%dM" % R, _seq(rng, R), 20, i % 2 == 1) for i in range(140)]
    units = (R - 20) // 2
    for i in range(140):
        reads.append(Read.make(S + 10, np.tile(_cigar([(1, "M"), (1, "I"), (1, "M")]), units), _seq(rng, 3 * units), 20, i % 2 == 0))
    for i in range(140):
        reads.append(Read.make(S + 10 + (i & 1), np.tile(_cigar([(1, "M"), (1, "D")]), units), _seq(rng, units), 20, i % 3 == 0))
    for i in range(6):
        reads.append(Read.make(S + 40, _cigar([(300, "M")] + [(1, "I")] * 300 + [(560, "M")]), _seq(rng, 1160), 20, i % 2 == 0))
    return [_filler(200), Region(S, S + R - 1, _seq(rng, R), reads)]


TILE_EDGE_COLUMNS = (511, 512, 1023, 1024)   # last / first column of a 512-column tile, of a 1024-column scan block
# (edge, bare, tail): every edge in both forms; the tail lengths 1, 2, 3 turn up at least twice each
TILE_EDGE_CASES = [(e, b, 1 + k % 3) for k, (e, b) in enumerate(itertools.product(TILE_EDGE_COLUMNS, (False, True)))]


def tile_edges(edge, bare=False, tail=1):
    """The reference's odd rules on column `edge` of the batch's column index: [filler, region], the region's column 300 (position
    P) being that column. Both forms hold: an insert anchored on P by reads that begin on P + 1 (leading nI, with and without a
    soft clip before it); inserts behind the last column E of the region, which is the last column of the batch (the reference
    drops them: the op begins past ref_end, where the read loop ends), and the longest insert of column E - 1, seven rows that are
    the batch's last but one; a deletion that starts before the region and one that ends beyond it; a last read whose last op
    is a match of `tail` bases (the last bases of the batch: the byte-wise load).
    bare=False: two reads delete 1556 columns from P on (over three further tiles), all 1556 coverage bookings of each on P; inserts
    behind P - 1, P and P + 1; full-length reads cover everything; 32 short reads keep P's row and insert rows from going black.
    bare=True: no base of any read lies on P. Three reads of 2M2D3I2M delete P - 1 and P (booked on P - 1) and anchor their
    insert on P, so P's '*' counts and its insert rows are divided by max(1, 0): pixel = count * 254, low byte."""
    assert edge >= 300 and tail in (1, 2, 3)
    rng = np.random.default_rng(4800 + edge + (7 if bare else 0))

    def seq(n):   # A C G T in both cases only: planes 8 and 9 of this case hold nothing but deleted columns
        return _seq(rng, n, _LETTERS)

    c, R, S = 300, 2100, 100_000
    P, E = S + c, S + R - 1
    reads = [Read.make(P + 1, "4S3I20M", seq(27)), Read.make(P + 1, "2I10M", seq(12), is_reverse=True),
             Read.make(E - 5, "6M9I", seq(15)), Read.make(E - 2, "3M3I", seq(6), is_reverse=True),
             Read.make(E - 6, "6M7I1M", seq(14)), Read.make(E - 3, "3M3I1M", seq(7), is_reverse=True),
             Read.make(S - 30, "10M40D10M", seq(20)), Read.make(E - 29, "10M50D5M", seq(15), is_reverse=True)]
    if bare:
        reads += [Read.make(P - 3, "2M2D3I2M", seq(7), 20, i == 1) for i in range(3)]
        reads += [Read.make(S, "%dM" % c, seq(c), 20, i == 1) for i in range(2)]                      # S .. P - 1
        reads += [Read.make(P + 1, "%dM" % (R - c - 1), seq(R - c - 1), 20, i == 0) for i in range(2)]  # P + 1 .. E
    else:
        reads += [Read.make(P - 10, "10M1556D10M", seq(20), 20, i == 1) for i in range(2)]
        reads += [Read.make(P - 1, "1M2I1M1I1M5I3M", seq(14)), Read.make(P - 1, "2M4I2M", seq(8), is_reverse=True)]
        reads += [Read.make(S, "%dM" % R, seq(R), 20, i == 1) for i in range(3)]
        # (the 3112 bookings blacken every count below 13 on P: sixteen forward reads with A on P and sixteen with a leading
        # GGG behind P keep one plane of P's row and of its first three insert rows at pixel 1)
        reads += [Read.make(P - 1, "3M", b"TAT") for _ in range(16)] + [Read.make(P + 1, "3I5M", b"GGGCCCCC") for _ in range(16)]
    reads.append(Read.make(S + 50, "3M1I%dM" % tail, seq(4 + tail)))
    return [_filler(edge - c), Region(S, E, seq(R), reads)]


def all_bytes():
    """every byte value as a read base on both strands, under match ops and in inserts (k_polish_tiles' s_lut, k_polish_insert's
    polish_sym): only A C G T a c g t take planes 0-7"""
    every = bytes(range(256))
    S = 3000
    reads = []
    for i in range(4):   # shifted, so that a column sees four different bytes
        reads.append(Read.make(S + 5 + i, "256M", every, 20, i % 2 == 1))
    reads += [Read.make(S + 20, "2M256I2M", b"AC" + every + b"GT", 20, rev) for rev in (False, True)]
    reads.append(Read.make(S + 20, "2M200I2M", b"AC" + every[::-1][:200] + b"GT"))
    return [Region(S, S + 299, b"N" * 300, reads)]


def _deep_kind(i):
    """deep_column's read i: (cigar, bases)"""
    if i % 3 == 2 and i < 60_000:
        return "3M2D", b"AGT"       # columns 4 and 5 deleted, both bookings on column 4
    if i % 16 in (0, 7):
        return "1M1D1M", b"CT"      # the middle column (2) deleted
    return "3M", b"AGT"


DEEP_MAPQ0 = (5, 1000, 40_000)


def deep_column(n):
    """n reads that all begin on column 1 of a seven-column region (columns 0 and 6 stay empty). Read i is reverse when i is odd,
    has mapping quality 0 when i is in DEEP_MAPQ0, and is
        3M2D    when i % 3 == 2 and i < 60 000  (columns 1-3 matched, 4 and 5 deleted: column 4 takes both coverage bookings,
                                                 column 5 is covered by deletions alone, coverage 0),
        1M1D1M  else when i % 16 is 0 or 7      (the middle column 2 deleted),
        3M      otherwise."""
    S = 700
    reads = []
    for i in range(n):
        cigar, bases = _deep_kind(i)
        reads.append(Read.make(S + 1, cigar, bases, 20, i % 2 == 1, 0 if i in DEEP_MAPQ0 else 60))
    return [Region(S, S + 6, b"ACGTACG", reads)]


def many_tiles():
    """one region of 140 000 columns = 274 tiles, more than the 256 of k_tile_fill's table: the reads' op ranges are searched.
    Four one-op reads, four of 900M1I900M2D units and two of 1M138000D1M."""
    rng = np.random.default_rng(4741)
    R = 140_000
    reads = [Read.make(200, "%dM" % (R - 1000), _seq(rng, R - 1000), 20, i % 2 == 0) for i in range(4)]
    units = (R - 800) // 1802
    for i in range(4):
        reads.append(Read.make(300 + i, np.tile(_cigar([(900, "M"), (1, "I"), (900, "M"), (2, "D")]), units),
                               _seq(rng, 1801 * units), 20, i % 2 == 1))
    for i in range(2):
        reads.append(Read.make(700 + 300 * i, "1M138000D1M", _seq(rng, 2), 20, i == 1))
    return [Region(0, R - 1, _seq(rng, R), reads)]


def many_ops():
    """five reads of 1M1D x 34 000 = 68 000 ops, more than the 65 535 of the table's 16-bit op offsets, two reads of 65 898 ops
    whose two-column ops lie across tile edges, and five ordinary reads over the same columns. The two: 523 units of 1M1D x 62,
    2M, 2D = 126 ops on 128 columns; from column 129 the 2D of every fourth unit covers the last column of a tile and the first
    of the next (511 and 512 first), from column 3 the 2M does: the op before the first one that begins in a tile reaches into it."""
    rng = np.random.default_rng(4743)
    units = 34_000
    R = 2 * units + 400
    reads = [Read.make(100 + i, np.tile(_cigar([(1, "M"), (1, "D")]), units), _seq(rng, units), 20, i % 2 == 0) for i in range(5)]
    unit = np.concatenate([np.tile(_cigar([(1, "M"), (1, "D")]), 62), _cigar([(2, "M"), (2, "D")])])
    reads += [Read.make(start, np.tile(unit, 523), _seq(rng, 64 * 523), 20, start == 3) for start in (129, 3)]
    reads += [Read.make(50, "%dM" % (R - 100), _seq(rng, R - 100), 20, i % 2 == 1) for i in range(5)]
    return [Region(0, R - 1, _seq(rng, R), reads)]


def _overflow_reads(rng, S):
    reads = [Read.make(S + 40 + i, "1M20400D1M", _seq(rng, 2), 20, i % 2 == 1) for i in range(10)]
    reads += [Read.make(S + 30, "40M", _seq(rng, 40)), Read.make(S + 10_000, "30M2I30M", _seq(rng, 62), is_reverse=True),
              Read.make(S + 20_430, "50M", _seq(rng, 50))]
    return reads


def pair_overflow():
    """20 500 columns (41 tiles) under ten reads of 1M20400D1M: 40 pairs or more per read from 22 bases, against a pair bound that
    grows with bases and reads"""
    rng = np.random.default_rng(4751)
    S, R = 7000, 20_500
    return [Region(S, S + R - 1, _seq(rng, R), _overflow_reads(rng, S))]


def pair_and_insert_overflow():
    """pair_overflow()'s region and reads, and one read with a single insert of 46 000 bases"""
    rng = np.random.default_rng(4751)
    S, R = 7000, 20_500
    ref = _seq(rng, R)
    reads = _overflow_reads(rng, S)
    reads.insert(4, Read.make(S + 5000, "5M46000I5M", _seq(rng, 46_010)))
    return [Region(S, S + R - 1, ref, reads)]


def many_regions():
    """1500 regions of 1 to 3 columns, 0 to 3 reads each (reads begin before their region and end behind it, some carry inserts,
    some have mapping quality 0); every tenth region brings a reference buffer longer than itself. Several hundred regions
    share each tile. For seq_length 7, seq_overlap 3."""
    rng = np.random.default_rng(4761)
    regs = []
    for g in range(1500):
        R = int(rng.integers(1, 4))
        S = 1000 + 10 * g
        reads = []
        for _ in range(int(rng.integers(0, 4))):
            kind = int(rng.integers(0, 5))
            pos = S + int(rng.integers(-2, R))
            cigar = ("6M", "1M3I4M", "2S2I5M", "2M2D2M", "1M9I1M1D2M")[kind]
            n = (6, 8, 9, 4, 13)[kind]
            reads.append(Read.make(pos, cigar, _seq(rng, n), 20, bool(rng.integers(0, 2)), 0 if rng.integers(0, 12) == 0 else 60))
        regs.append(Region(S, S + R - 1, _seq(rng, R + (3 if g % 10 == 0 else 0)), reads))
    return regs


# name -> (builder, seq_length, seq_overlap); tile_edges, with its parameters, stands beside it
CASES = {
    "owner_tables": (owner_tables, 1000, 50),
    "all_bytes": (all_bytes, 1000, 50),
    "deep_column": (lambda: deep_column(65_540), 1000, 50),
    "many_tiles": (many_tiles, 1000, 50),
    "many_ops": (many_ops, 1000, 50),
    "pair_overflow": (pair_overflow, 1000, 50),
    "pair_and_insert_overflow": (pair_and_insert_overflow, 1000, 50),
    "many_regions": (many_regions, 7, 3),
}
