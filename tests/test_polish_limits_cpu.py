"""CPU: the oracle of the polisher's image builder on the inputs of tests/polish_cases.py, before test_polish_limits_gpu.py judges
the kernels by it. The C oracle (oracle/polish_summary_oracle.c) against the independent dictionary restatement of
test_oracle_polish.py on every case, and against the reference library itself where oracle/_ref was built; the depth checker
(tests/depth_ref.py) against depths written out by hand; and what makes each case a limit case (pairs and insert rows beyond
the workspace heuristics, tiles and ops per read beyond k_tile_fill's table, reads per column beyond the depth plane) asserted
from the inputs alone."""
import functools

import numpy as np
import pytest

import depth_ref as dr
import polish_cases as pc
from test_oracle_polish import _check_region_against_dict, dict_summary
from test_oracle_polish_ref import _need_reference
from pepper_thesis_amd.batch import Region, pack_regions


@functools.lru_cache(maxsize=None)
def regions(name):
    return pc.CASES[name][0]()


# ---- the C oracle against the dictionary restatement -----------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in pc.CASES if n not in ("many_tiles", "many_ops")])
def test_oracle_equals_dict(oracle_lib, name):
    _, L, O = pc.CASES[name]
    _check_region_against_dict(oracle_lib, regions(name), L, O)


@pytest.mark.parametrize("edge,bare,tail", pc.TILE_EDGE_CASES)
def test_oracle_equals_dict_tile_edges(oracle_lib, edge, bare, tail):
    _check_region_against_dict(oracle_lib, pc.tile_edges(edge, bare, tail))
    _check_region_against_dict(oracle_lib, pc.tile_edges(edge, bare, tail), 7, 3)


@pytest.mark.parametrize("name", ["many_tiles", "many_ops"])
def test_oracle_equals_dict_on_a_stride_of_columns(oracle_lib, name):
    """the two long regions (140 000 and 68 400 columns) are too slow for the pure-Python side as a whole: the dictionary
    restatement runs on windows of them instead - 700 columns at the region's start, at its end and every 9973 columns (a
    prime, so that the windows fall on ever different places of the 512-column tiles) - each window being a region of its own
    with all the reads. A region's rows depend on nothing outside it but the reads, so the oracle's rows of the whole region
    must hold the window's rows at the window's place."""
    reg = regions(name)[0]
    whole = oracle_lib.polish_summarize(pack_regions([reg]), 1000, 50, want_flat=True)
    R = reg.ref_end - reg.ref_start + 1
    n_ins = 0
    for w0 in sorted(set(list(range(0, R - 700, 9973)) + [R - 700])):
        win = Region(reg.ref_start + w0, reg.ref_start + w0 + 699, reg.ref[w0:w0 + 700], reg.reads)
        img, gpos = dict_summary(win)
        first = int(np.searchsorted(whole.flat_position, win.ref_start, "left"))
        last = int(np.searchsorted(whole.flat_position, win.ref_end, "right"))
        assert last - first == len(gpos), w0
        assert np.array_equal(whole.flat_images[first:last], img), w0
        assert whole.flat_position[first:last].tolist() == [p for p, _ in gpos]
        assert whole.flat_index[first:last].tolist() == [i for _, i in gpos]
        n_ins += len(gpos) - 700
        _check_region_against_dict(oracle_lib, [win])
    if name == "many_tiles":
        assert n_ins > 0


# ---- the cases hold what they are meant to hold ------------------------------------------------------------------------

def _row(out, pos, index=0):
    k = np.flatnonzero((out.flat_position == pos) & (out.flat_index == index))
    assert len(k) == 1, (pos, index)
    return out.flat_images[int(k[0])].tolist()


@pytest.mark.parametrize("edge", pc.TILE_EDGE_COLUMNS)
def test_tile_edges_rules_by_hand(oracle_lib, edge):
    """the oracle's rows on the edge column P, worked out by hand from the reads of polish_cases.tile_edges"""
    S, P, E = 100_000, 100_300, 102_099
    # covered form. On P: three full-length reads, 1M of 1M2I1M1I1M5I3M, the second M of 2M4I2M, the A of sixteen TAT = 21 bases,
    # and two deletions of 1556 columns that start there: coverage 21 + 2 * 1556 = 3133. A forward has 16 to 19 of them,
    # 16 / 3133 * 254 = 1.3 and 19 / 3133 * 254 = 1.5: pixel 1; no other count exceeds 3: pixel 0. Insert rows 1-3 hold the sixteen
    # leading GGG and at most two more forward G: pixel 1; row 4 the last base of 4I alone. P + 1 carries no booking: its
    # 7 + 16 + 16 bases and 2 deletions are over a coverage of 39
    regs = pc.tile_edges(edge)
    assert sum(len(r.ref) for r in regs[:1]) + (P - S) == edge
    out = oracle_lib.polish_summarize(pack_regions(regs), want_flat=True)
    assert _row(out, P) == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert [_row(out, P, i) for i in range(1, 5)] == [[0, 0, 0, 0, 0, 0, 1, 0, 0, 0]] * 3 + [[0] * 10]
    assert int(((out.flat_position == P) & (out.flat_index > 0)).sum()) == 4
    assert int(((out.flat_position == P - 1) & (out.flat_index > 0)).sum()) == 2
    assert int(((out.flat_position == P + 1) & (out.flat_index > 0)).sum()) == 5
    r1 = _row(out, P + 1)
    assert r1[8] == r1[9] == int(1 / 39 * 254) and sum(1 for v in r1 if v) >= 3
    # the insert behind the last column is dropped, the one behind E - 1 kept: 7 rows, then the row of E ends the batch
    assert int(((out.flat_position == E) & (out.flat_index > 0)).sum()) == 0
    assert out.flat_position[-9:].tolist() == [E - 1] * 8 + [E] and out.flat_index[-9:].tolist() == list(range(8)) + [0]
    # the deletion that starts 20 columns before the region books nothing inside; the one that starts on E - 19 books the 20
    # columns to E (not the 50 of its length) on E - 19
    assert _row(out, S)[9] == int(1 / 3 * 254)                      # '*' forward over the three full-length reads
    assert _row(out, E - 19)[8] == int(1 / (3 + 20) * 254)
    # bare form. On P: no base; '*' of three 2M2D3I2M reads, two forward and one reverse, over max(1, 0): 2 * 254 = 508 -> 252
    # and 254. Their coverage bookings (2 each) are on P - 1, next to two bases.
    regs = pc.tile_edges(edge, bare=True)
    out = oracle_lib.polish_summarize(pack_regions(regs), want_flat=True)
    assert _row(out, P) == [0] * 8 + [254, (2 * 254) & 0xFF]
    assert int(((out.flat_position == P) & (out.flat_index > 0)).sum()) == 3
    for i in (1, 2, 3):   # five reads anchor an insert here (3I 3I 3I, and the leading 3I and 2I): counts * 254, low byte
        row = _row(out, P, i)
        assert sum(row) > 0 and all(v in (0, 254, 252, 250, 248, 246) for v in row), row
    assert _row(out, P - 1)[8:] == [int(1 / 8 * 254), int(2 / 8 * 254)]


def test_all_bytes_take_ten_planes(oracle_lib):
    """only the eight letters ACGTacgt reach planes 0-7; each of the other 248 byte values counts as 'other' of its strand"""
    reg = pc.all_bytes()[0]
    out = oracle_lib.polish_summarize(pack_regions([reg]), want_flat=True)
    ins = out.flat_images[(out.flat_position == reg.ref_start + 21) & (out.flat_index > 0)]
    assert len(ins) == 256
    # insert row v + 1 holds byte v of the forward and of the reverse read, and byte 255 - v of the 200-base forward insert;
    # coverage of the anchor column (S + 21): the four 256M reads and the three reads with the inserts
    for v in range(256):
        want = [0] * 10
        for byte, rev in [(v, False), (v, True)] + ([(255 - v, False)] if v < 200 else []):
            sym = "ACGT".find(chr(byte).upper()) if byte < 128 else -1
            want[(8 if rev else 9) if sym < 0 else sym + (0 if rev else 4)] += 1
        assert ins[v].tolist() == [int(c / 7 * 254) for c in want], v


def test_deep_column_depth_by_hand():
    """depth_ref.region_depth on deep_column(65 540). Reads of mapping quality above 0, counted from the case's rule (forward +
    reverse): 3M 19 922 + 19 924, 1M1D1M 2 846 + 2 846, 3M2D 10 000 + 9 999; three reads have mapping quality 0. Columns 1-3
    are reached by all 65 537 (a deleted column counts), which the plane clamps to 65 535; columns 4 and 5 by the 3M2D reads."""
    regs = regions("deep_column")
    reads = regs[0].reads
    assert len(reads) == 65_540 and sum(1 for r in reads if r.mapq == 0) == 3
    kinds = {}
    for i, r in enumerate(reads):
        if r.mapq:
            k = (pc._deep_kind(i)[0], r.is_reverse)
            kinds[k] = kinds.get(k, 0) + 1
    assert kinds == {("3M", False): 19_922, ("3M", True): 19_924, ("1M1D1M", False): 2_846, ("1M1D1M", True): 2_846,
                     ("3M2D", False): 10_000, ("3M2D", True): 9_999}
    raw = 19_922 + 19_924 + 2_846 + 2_846 + 10_000 + 9_999
    assert raw == 65_537 > pc.DEPTH_MAX
    depth = dr.region_depth(pack_regions(regs), 0)
    assert depth.tolist() == [0, 65_535, 65_535, 65_535, 19_999, 19_999, 0]


def _region_depth_loop(batch, g):
    """depth_ref's rule as a plain loop over reads and operations (depth_ref.region_depth works on whole arrays)"""
    start, end = int(batch.ref_start[g]), int(batch.ref_end[g])
    depth = np.zeros(end - start + 1, np.int64)
    for r in range(int(batch.read_off[g]), int(batch.read_off[g + 1])):
        if int(batch.read_mapq[r]) == 0:
            continue
        ref = int(batch.read_pos[r])
        for w in batch.cigar[int(batch.cigar_off[r]):int(batch.cigar_off[r + 1])].tolist():
            op, ln = w & 0xF, w >> 4
            if ref > end:
                break
            if op in dr.M_OPS or op in dr.D_OPS:
                a, b = max(ref, start), min(ref + ln - 1, end)
                if a <= b:
                    depth[a - start:b - start + 1] += 1
                ref += ln
    return np.minimum(depth, dr.DEPTH_MAX)


def test_depth_checker_equals_its_rule_as_a_loop():
    """on every case; owner_tables and many_ops with every twentieth and every fourth read (the loop takes seconds on all)"""
    batches = [regions(n) for n in pc.CASES if n not in ("owner_tables", "many_ops")] + [pc.tile_edges(*p) for p in pc.TILE_EDGE_CASES]
    for name, k in (("owner_tables", 20), ("many_ops", 4)):
        batches.append([Region(r.ref_start, r.ref_end, r.ref, r.reads[::k]) for r in regions(name)])
    for regs in batches:
        b = pack_regions(regs)
        for g in range(b.n_regions):
            assert np.array_equal(dr.region_depth(b, g), _region_depth_loop(b, g)), g


def test_deep_column_pixels_by_hand(oracle_lib):
    """column 1 (all 65 537 reads, A but for the C of the 1M1D1M reads) and the columns of the 3M2D deletions: column 4 has both
    bookings of every read, column 5 none (counts of ten thousand over max(1, 0))"""
    out = oracle_lib.polish_summarize(pack_regions(regions("deep_column")), want_flat=True)
    assert out.flat_position.tolist() == list(range(700, 707)) and not out.flat_index.any()
    assert out.flat_images[1].tolist() == DEEP_FULL_COLUMN
    assert out.flat_images[4].tolist() == DEEP_BOOKED_COLUMN
    assert out.flat_images[5].tolist() == DEEP_DELETIONS_ONLY_COLUMN
    assert out.flat_images[0].tolist() == [0] * 10 == out.flat_images[6].tolist()


# rows of deep_column(65 540), by hand: planes A C G T reverse, A C G T forward, other reverse, other forward
DEEP_FULL_COLUMN = [int((19_924 + 9_999) / 65_537 * 254), int(2_846 / 65_537 * 254), 0, 0,
                    int((19_922 + 10_000) / 65_537 * 254), int(2_846 / 65_537 * 254), 0, 0, 0, 0]
DEEP_BOOKED_COLUMN = [0] * 8 + [int(9_999 / (2 * 19_999) * 254), int(10_000 / (2 * 19_999) * 254)]
DEEP_DELETIONS_ONLY_COLUMN = [0] * 8 + [(9_999 * 254) & 0xFF, (10_000 * 254) & 0xFF]


# ---- the limits, from the inputs alone ---------------------------------------------------------------------------------

# name -> (pairs, pair heuristic, insert rows, insert-row heuristic, most tiles of a read, most ops of a read)
FIGURES = {
    "owner_tables": (1698, 3808, 741, 7496, 4, 2220),
    "pair_overflow": (403, 103, 2, 45_096, 40, 3),
    "pair_and_insert_overflow": (404, 286, 46_002, 45_096, 40, 3),
    "many_tiles": (2717, 4432, 308, 284_096, 272, 308),
    "many_ops": (1603, 2358, 0, 140_896, 134, 68_000),
}


def figures(regs):
    tiles = [pc.tiles_of_read(regs, g, rd) for g, reg in enumerate(regs) for rd in reg.reads]
    ops = [len(rd.cigar) for reg in regs for rd in reg.reads]
    return (pc.exact_pairs(regs), pc.pair_heuristic(regs), pc.exact_insert_rows(regs), pc.insert_heuristic(regs),
            max(tiles), max(ops))


def assert_limits_crossed(name, regs):
    """what makes the case a limit case; the GPU tests assert it again before they run the kernels"""
    pairs, pair_bound, ins, ins_bound, tiles, ops = figures(regs)
    if name in ("pair_overflow", "pair_and_insert_overflow"):
        assert pairs > pair_bound, (pairs, pair_bound)             # the first launch overflows the pair workspace
    if name == "pair_overflow":
        assert ins <= ins_bound                                    # ... and only that
    if name == "pair_and_insert_overflow":
        assert ins > ins_bound, (ins, ins_bound)                   # the second launch overflows the insert rows
    if name == "many_tiles":
        assert tiles > pc.TABLE_TILES and ops <= pc.TABLE_OPS and pairs <= pair_bound
    if name == "many_ops":
        assert ops > pc.TABLE_OPS and tiles <= pc.TABLE_TILES and pairs <= pair_bound
        # ... and on that path the op before a tile's first one reaches into the tile: a 2M and a 2D across the edge 511 | 512
        across = set()
        for rd in regs[0].reads:
            cg = np.asarray(rd.cigar, np.int64)
            begin = rd.pos + np.cumsum(cg >> 4) - (cg >> 4)          # (every op of these reads consumes the reference)
            if len(cg) > pc.TABLE_OPS:
                across |= {int(o) for o in (cg & 15)[((cg >> 4) == 2) & (begin % pc.TILE == pc.TILE - 1)]}
        assert across == {0, 2}
    if name == "owner_tables":
        # four pair batches on every tile, ops per batch far beyond one trip of 512 threads
        assert pairs <= pair_bound and ins <= ins_bound
        assert min(len(rd.cigar) for rd in regs[1].reads[140:280]) * pc.PAIR_BATCH > 100 * pc.THREADS
        assert len(regs[1].reads) > 3 * pc.PAIR_BATCH


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_limits_from_the_inputs(oracle_lib, name):
    regs = regions(name)
    assert figures(regs) == FIGURES[name]
    assert_limits_crossed(name, regs)
    # the oracle counts the same insert rows
    out = oracle_lib.polish_summarize(pack_regions(regs), want_flat=True)
    cols = sum(r.ref_end - r.ref_start + 1 for r in regs)
    assert int(out.region_row_off[-1]) - cols == FIGURES[name][2]


def test_many_regions_share_tiles():
    regs = regions("many_regions")
    assert len(regs) == 1500 and {r.ref_end - r.ref_start + 1 for r in regs} == {1, 2, 3}
    assert {len(r.reads) for r in regs} == {0, 1, 2, 3}
    assert sum(len(r.ref) for r in regs) < 8 * pc.TILE               # several hundred regions per tile
    assert pc.exact_insert_rows(regs) > 500
    assert any(len(r.ref) > r.ref_end - r.ref_start + 1 for r in regs)


# ---- live: the reference library itself (only where oracle/_ref was built) --------------------------------------------

def _assert_oracle_is_reference(oracle_lib, regs, tag):
    b = pack_regions(regs)
    img, pos, idx, off = oracle_lib.reference_polish_flat(b)
    out = oracle_lib.polish_summarize(b, 1000, 50, want_flat=True)
    assert np.array_equal(out.region_row_off, off), tag
    assert np.array_equal(out.flat_images, img), tag
    assert np.array_equal(out.flat_position, pos) and np.array_equal(out.flat_index, idx), tag


@pytest.mark.parametrize("name", [n for n in pc.CASES if n != "all_bytes"])
def test_live_oracle_vs_reference(oracle_lib, name):
    """the C oracle against the reference's SummaryGenerator on the limit cases. all_bytes is left out: the reference hands
    a plain char to toupper, which the C standard leaves undefined for the negative values that bytes above 127 are there, so
    its rows for them pin nothing (the dictionary restatement and test_all_bytes_take_ten_planes stand for that case)."""
    _need_reference(oracle_lib)
    _assert_oracle_is_reference(oracle_lib, regions(name), name)


@pytest.mark.parametrize("edge,bare,tail", pc.TILE_EDGE_CASES)
def test_live_oracle_vs_reference_tile_edges(oracle_lib, edge, bare, tail):
    _need_reference(oracle_lib)
    _assert_oracle_is_reference(oracle_lib, pc.tile_edges(edge, bare, tail), (edge, bare, tail))
