"""GPU: the polisher's image builder (pv_polish_summarize_regions[_dev]: k_polish_* of csrc/summary_polish.hip behind the front
end of csrc/summary_front.hip) at the limits its own kernels have, on the inputs of tests/polish_cases.py: the op -> slot tables
of k_polish_tiles, tile and scan-block edges, every base byte, more reads on a column than the depth plane counts, k_tile_fill's
search path, both workspace retries one after the other, hundreds of regions per tile, and the capacities of the device and the
host form. Everything is compared bit for bit with the CPU oracle, which test_polish_limits_cpu.py pins on the same inputs to
the dictionary restatement and to the reference library, and the depth plane with tests/depth_ref.py. No tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

import depth_ref as dr
import polish_cases as pc
from test_oracle_polish import py_chunks
from test_polish_gpu import CHUNK_FIELDS, assert_polish_equal
from test_polish_limits_cpu import (DEEP_BOOKED_COLUMN, DEEP_DELETIONS_ONLY_COLUMN, DEEP_FULL_COLUMN, FIGURES, assert_limits_crossed,
                                    figures)
from pepper_thesis_amd import _ffi
from pepper_thesis_amd.batch import pack_regions
from pepper_thesis_amd.polish_summary import PolishBuffers

pytestmark = pytest.mark.gpu
GUARD = 0x5A
DEV_FIELDS = CHUNK_FIELDS + ("depth",)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(regions, batch, seq_length, seq_overlap) of a case of polish_cases.CASES, built once"""
    fn, L, O = pc.CASES[name]
    regs = fn()
    return regs, pack_regions(regs), L, O


@functools.lru_cache(maxsize=None)
def _edge_case(edge, bare, tail):
    regs = pc.tile_edges(edge, bare, tail)
    return regs, pack_regions(regs), 1000, 50


_EXPECTED = {}


def _expected(oracle_lib, key, b, L, O):
    """the oracle's answer and the checker's depth plane for a batch, computed once per (case, L, O) and left alone"""
    k = (key, L, O)
    if k not in _EXPECTED:
        exp = oracle_lib.polish_summarize(b, L, O, want_flat=True)
        _EXPECTED[k] = (exp, dr.row_depth(b, exp.position, exp.index, exp.region))
    return _EXPECTED[k]


def _exact(hip_ctx, oracle_lib, key, b, L, O):
    """host form with flat arrays and depth == oracle and depth checker; host form without flat arrays: the same chunks"""
    exp, depth = _expected(oracle_lib, key, b, L, O)
    got = hip_ctx.polish_summarize(b, L, O, want_flat=True, want_depth=True)
    assert_polish_equal(got, exp, key)
    assert got.depth.dtype == np.uint16 and np.array_equal(got.depth, depth), key
    lean = hip_ctx.polish_summarize(b, L, O, want_flat=False, want_depth=True)
    assert lean.flat_images is None and lean.region_row_off is None
    for f in DEV_FIELDS:
        assert np.array_equal(getattr(lean, f), getattr(got, f)), (key, f)
    return got


def _run_case(hip_ctx, oracle_lib, name):
    regs, b, L, O = _case(name)
    if name in FIGURES:
        assert figures(regs) == FIGURES[name]
        assert_limits_crossed(name, regs)
    return regs, b, _exact(hip_ctx, oracle_lib, name, b, L, O)


# ---- 1. the cases, host form ---------------------------------------------------------------------------------------------

def test_owner_tables(hip_ctx, oracle_lib):
    """k_polish_tiles' slot -> op lookup: `owc = s_blk[j >> 6]; while (s_pref[owc] <= j) owc++` with s_blk filled by
    `for (bb = (incl - effp + 63) >> 6; (bb << 6) < incl; bb++) s_blk[bb] = tid`. 140 one-op reads own 8 blocks of 64 slots each
    (s_blk up to index 4095); 140 reads of 1M1I1M give each pair about 768 ops on a tile, so p_off runs to about 98 000 ops per
    batch of 128 pairs = 190 trips of 512 threads, every match op padded by `effp = (eff + 3) & ~3` from 1 or 2 slots to 4;
    140 reads of 1M1D leave s_pref flat over every other op; 300 one-base inserts in a row share one anchor column
    (atomicMax on s_cnt[Q_LONG]). Tile edges lie inside the region (200 filler columns before it)."""
    _, _, got = _run_case(hip_ctx, oracle_lib, "owner_tables")
    assert int(got.region_row_off[-1]) == 200 + 1500 + FIGURES["owner_tables"][2]


@pytest.mark.parametrize("edge,bare,tail", pc.TILE_EDGE_CASES)
def test_tile_edges(hip_ctx, oracle_lib, edge, bare, tail):
    """the column `edge` of the batch's column index (last / first of a 512-column tile of k_polish_tiles, of a 1024-column
    block of k_polish_blk / k_polish_insoff) carries: an insert whose read begins on the next column - k_cigar_scan's
    `lo = read_pos - ref_start - 1` puts the read on the anchor's tile and k_polish_tiles' `anchor >= clo && anchor <= chi`
    gives the op to that tile alone; a deletion over three further tiles whose bookings all go to the start column
    (`if (ref_rel >= clo && ref_rel <= chi) atomicAdd(&s_cnt[Q_DCOV]..., n)`, n clipped to the region, in the start column's tile
    only); in the bare form an insert anchored on a deleted column of coverage 0 (polish_pixel's `cov > 1.0 ? cov : 1.0`).
    Inserts behind the region's last column are dropped and the rows of the column before it end at ins_off[n_cols]; the last
    read of the batch ends with a match of `tail` bases, which k_polish_tiles must load byte by byte
    (`if (bi + 4 <= a.n_bases) ... else for (e < nv)`). The rows are hand-worked in test_polish_limits_cpu.py."""
    regs, b, L, O = _edge_case(edge, bare, tail)
    assert len(regs[0].ref) + 300 == edge and b.cigar[-1] == (tail << 4) and b.base_off[-1] == b.n_bases
    got = _exact(hip_ctx, oracle_lib, ("tile_edges", edge, bare, tail), b, L, O)
    P = regs[1].ref_start + 300
    at = np.flatnonzero((got.flat_position == P) & (got.flat_index == 0))
    assert len(at) == 1 and at[0] >= edge
    assert got.flat_images[at[0]].tolist() == ([0] * 8 + [254, 252] if bare else [0, 0, 0, 0, 1, 0, 0, 0, 0, 0])


def test_all_bytes(hip_ctx, oracle_lib):
    """s_lut[256] of k_polish_tiles (`s_lut[tid] = polish_sym(tid)` for tid < 256, read as `s_lut[(bw >> (8 * e)) & 0xFF]`) and
    polish_sym in k_polish_insert: every byte value, bytes above 127 included, under match ops and in inserts on both strands"""
    _run_case(hip_ctx, oracle_lib, "all_bytes")


def test_deep_column_beyond_the_depth_plane(hip_ctx, oracle_lib):
    """65 540 reads on three columns: polish_launch has no front_check_depth, the counters are int32, and k_polish_image clamps
    the depth plane (`depth = (uint16_t)(d > 65535 ? 65535 : d)`) while polish_pixel takes the unclamped counts. One tile holds
    65 537 pairs = 513 batches of 128. Hand-worked (test_polish_limits_cpu.py): 65 537 reads of mapping quality above 0 reach
    columns 1-3; column 5 carries 10 000 + 9 999 deleted bases over a coverage of 0."""
    regs, b, got = _run_case(hip_ctx, oracle_lib, "deep_column")
    raw = sum(1 for r in regs[0].reads if r.mapq > 0)
    assert raw == 65_537 > pc.DEPTH_MAX
    assert got.flat_position.tolist() == list(range(700, 707))
    assert got.depth[0, :7].tolist() == [0, 65_535, 65_535, 65_535, 19_999, 19_999, 0] and not got.depth[0, 7:].any()
    assert got.flat_images[1].tolist() == DEEP_FULL_COLUMN
    assert got.flat_images[4].tolist() == DEEP_BOOKED_COLUMN
    assert got.flat_images[5].tolist() == DEEP_DELETIONS_ONLY_COLUMN


def test_read_over_more_than_256_tiles_takes_the_search_path(hip_ctx, oracle_lib):
    """k_tile_fill: `table = nb <= TF_CAP + 1 && c1 - c0 <= 65535` is false for reads over 272 tiles, so op_lo / op_hi come from
    the two binary searches over op_ref and pr.subw stays 0; k_polish_tiles clips whatever range it is given to the tile. One-op
    reads, reads of 900M1I900M2D units and two deletions of 138 000 columns."""
    _run_case(hip_ctx, oracle_lib, "many_tiles")


def test_read_with_more_than_65535_ops(hip_ctx, oracle_lib):
    """k_tile_fill's other way into the search path: 68 000 ops exceed the 16-bit op offsets of s_lo (`c1 - c0 <= 65535`), at
    134 tiles per read; k_polish_tiles then meets about 512 ops per pair, of one base or one deleted column. Two reads of
    65 898 ops lay a 2M and a 2D across every tile edge: `op_lo = lo > c0 ? lo - 1 : c0` must hand the tile the op before the
    first one that begins in it"""
    _run_case(hip_ctx, oracle_lib, "many_ops")


def test_pair_workspace_overflow_is_retried(hip_ctx, oracle_lib):
    """403 pairs against polish_limits' 2 * (n_bases / 512) + 3 * n_reads + 64 = 103: k_scan_tiles reports PV_ERR_LIMIT and
    zeroes tile_cnt, the first launch piles up nothing, pv_polish_summarize_regions' enlarge step sets
    `mp = n_reads * (tiles + 2)` and the second launch is exact"""
    _run_case(hip_ctx, oracle_lib, "pair_overflow")


def test_pair_then_insert_overflow_needs_the_third_launch(hip_ctx, oracle_lib):
    """the only path through all three launches of launch_and_count: the first overflows the pairs (404 against 286) and counts
    its insert rows over an empty pileup (counts[3] = 0, so `if (counts[3] > mi)` leaves mi alone); the second, with room for
    the pairs, finds 46 002 insert rows against 2 * n_cols + 4096 = 45 096 (k_polish_regions: `diag[D_NINS] > max_ins_rows`);
    the third, with mi = counts[3], is exact. The 66 502 rows also exceed run_polish_summarizer's first guess, so the host
    buffers are grown once (PV_ERR_CAPACITY) and the call made again."""
    regs, b, got = _run_case(hip_ctx, oracle_lib, "pair_and_insert_overflow")
    cols = int(b.ref.shape[0])
    assert int(got.region_row_off[-1]) == cols + 46_002 > cols + cols // 2 + 1024


def test_many_regions_share_a_tile(hip_ctx, oracle_lib):
    """1500 regions of 1-3 columns, seq_length 7, overlap 3: k_polish_tiles' `clo = tlo - col_base; chi = thi - col_base` clipped
    to [0, R - 1] for hundreds of regions per tile, k_polish_image's region search (`upper_bound_i64(a.in.ref_off, ...)`, and
    `if (i >= R) return` on the padded reference buffers), k_polish_regions' sequential chunk layout and k_polish_chunks'
    `upper_bound_i64(a.reg_chunks, ...)`"""
    _, b, got = _run_case(hip_ctx, oracle_lib, "many_regions")
    assert len(got.images) > 1500 and set(np.unique(got.region)) == set(range(1500))


# ---- 2. the device form -----------------------------------------------------------------------------------------------------

def _dev_out(n_alloc, L, O, capacity=None):
    """a DevicePolishOut with the depth plane whose tensors hold n_alloc chunks, all bytes GUARD; capacity: what the struct says"""
    import torch
    from pepper_thesis_amd.device import DevicePolishOut
    dout = DevicePolishOut(n_alloc, L, O, depth=True)
    for f in DEV_FIELDS:
        getattr(dout, f).view(torch.uint8).fill_(GUARD)
    if capacity is not None:
        dout.c.chunk_capacity = capacity
    return dout


def _run_dev(hip_ctx, b, dout):
    import torch
    from pepper_thesis_amd.device import DeviceBatch
    db = DeviceBatch(b)
    torch.cuda.synchronize()
    hip_ctx.polish_summarize_dev(db, dout)
    hip_ctx.synchronize()
    return dout.counts.cpu().tolist()


def _dev_field(dout, f):
    a = getattr(dout, f).cpu().numpy()
    return a.view(np.uint16) if f == "depth" else a


def _guard_from(dout, k):
    """every byte of chunk k and the chunks behind it is still GUARD, in all six arrays"""
    return all(bool((_dev_field(dout, f)[k:].reshape(-1).view(np.uint8) == GUARD).all()) for f in DEV_FIELDS)


def _dev_batches(which):
    """(key, batch, seq_length, seq_overlap) of the device-form comparisons"""
    if which != "tile_edges":
        return [(which,) + _case(which)[1:]]
    return [(("tile_edges",) + p,) + _edge_case(*p)[1:] for p in (pc.TILE_EDGE_CASES[2], pc.TILE_EDGE_CASES[5])]   # 512 covered, 1023 bare


@pytest.mark.parametrize("which", ["owner_tables", "many_regions", "tile_edges"])
def test_device_form_equals_host_form(hip_ctx, oracle_lib, which):
    """pv_polish_summarize_regions_dev (one launch, caller-owned chunk tensors in HBM with the depth plane): images, position,
    index, depth, region and chunk_id equal the host form's, counts = [chunks, rows, 0, insert rows] as k_polish_regions writes
    them, and the two spare chunks behind the result keep their guard bytes"""
    for key, b, L, O in _dev_batches(which):
        host = _exact(hip_ctx, oracle_lib, key, b, L, O)
        n = len(host.images)
        dout = _dev_out(n + 2, L, O)
        counts = _run_dev(hip_ctx, b, dout)
        rows = int(host.region_row_off[-1])
        assert counts == [n, rows, 0, rows - int((b.ref_end - b.ref_start + 1).sum())], (key, counts)
        for f in DEV_FIELDS:
            assert np.array_equal(_dev_field(dout, f)[:n], getattr(host, f)), (key, f)
        assert _guard_from(dout, n), key


@pytest.mark.parametrize("which", ["owner_tables", "many_regions"])
def test_device_form_chunk_capacity_one_short(hip_ctx, oracle_lib, which):
    """k_polish_chunks: `if (nck > a.pout.chunk_capacity) nck = a.pout.chunk_capacity` clips silently while k_polish_regions'
    `d_counts[0] = chunks` reports the true number with status 0: the first n - 1 chunks are the host form's, chunk n - 1 and
    the two spare ones behind it keep every guard byte"""
    _, b, L, O = _case(which)
    exp, depth = _expected(oracle_lib, which, b, L, O)
    n = len(exp.images)
    assert n >= 4
    dout = _dev_out(n + 2, L, O, capacity=n - 1)
    counts = _run_dev(hip_ctx, b, dout)
    assert counts[0] == n and counts[1] == int(exp.region_row_off[-1]) and counts[2] == 0, counts
    for f in CHUNK_FIELDS:
        assert np.array_equal(_dev_field(dout, f)[:n - 1], getattr(exp, f)[:n - 1]), f
    assert np.array_equal(_dev_field(dout, "depth")[:n - 1], depth[:n - 1])
    assert _guard_from(dout, n - 1)


def test_device_form_reports_the_pair_limit_and_writes_no_chunk(hip_ctx):
    """the device form makes no second launch: on pair_overflow() k_scan_tiles sets PV_ERR_LIMIT, and k_polish_insert,
    k_polish_image and k_polish_chunks all return on `a.diag[D_STATUS] != 0`: status PV_ERR_LIMIT, no byte of a chunk array
    written. (counts[0] and counts[1] come from an empty pileup and mean nothing here.)"""
    regs, b, L, O = _case("pair_overflow")
    assert_limits_crossed("pair_overflow", regs)
    dout = _dev_out(40, L, O)
    counts = _run_dev(hip_ctx, b, dout)
    assert counts[2] == _ffi.PV_ERR_LIMIT == dout.status(), counts
    assert _guard_from(dout, 0)


# ---- 3. the host form's capacities ------------------------------------------------------------------------------------------

HOST_ARRAYS = DEV_FIELDS + ("flat_images", "flat_position", "flat_index", "region_row_off")


@pytest.mark.parametrize("short", ["chunks", "rows", "both"])
def test_host_form_capacity_reports_the_needs_and_copies_nothing(hip_ctx, oracle_lib, short):
    """pv_polish_summarize_regions with caller buffers one chunk or one row too small: `if (out->n_chunks > ccap ||
    (out->flat_images && out->n_rows > rcap))` returns PV_ERR_CAPACITY before any copy, with the true needs in n_chunks / n_rows
    and in the message. (The kernels ran with flat_cap = row_capacity: k_polish_image's `row < a.flat_cap` keeps them inside.)
    run_polish_summarizer on the same batch grows its buffers and ends exact."""
    key = ("tile_edges",) + pc.TILE_EDGE_CASES[6]
    _, b, _, _ = _edge_case(*pc.TILE_EDGE_CASES[6])
    L, O = 64, 8
    exp, _ = _expected(oracle_lib, key, b, L, O)
    n, rows = len(exp.images), int(exp.region_row_off[-1])
    ccap = n - 1 if short in ("chunks", "both") else n
    rcap = rows - 1 if short in ("rows", "both") else rows
    pb = PolishBuffers(b.n_regions, ccap, rcap, L, want_flat=True, want_depth=True)
    for f in HOST_ARRAYS:
        getattr(pb, f).view(np.uint8).fill(GUARD)
    cin = b.as_c()
    rc = hip_ctx.lib.pv_polish_summarize_regions(hip_ctx.handle, C.byref(cin), L, O, C.byref(pb.c))
    assert rc == _ffi.PV_ERR_CAPACITY
    assert (int(pb.c.n_chunks), int(pb.c.n_rows)) == (n, rows)
    msg = hip_ctx.lib.pv_last_error().decode()
    assert "%d chunks" % n in msg and "%d rows" % rows in msg, msg
    for f in HOST_ARRAYS:
        assert (getattr(pb, f).view(np.uint8) == GUARD).all(), f
    # with exactly enough room the same direct call succeeds ...
    pb = PolishBuffers(b.n_regions, n, rows, L, want_flat=True, want_depth=True)
    assert hip_ctx.lib.pv_polish_summarize_regions(hip_ctx.handle, C.byref(cin), L, O, C.byref(pb.c)) == 0
    assert_polish_equal(pb.result(), exp, short)
    # ... and so does the growing caller
    _exact(hip_ctx, oracle_lib, key, b, L, O)


def test_seq_length_and_overlap_at_their_ends(hip_ctx, oracle_lib):
    """k_polish_regions' chunk count `n <= seq_len ? 1 : 1 + (n - seq_len + seq_step - 1) / seq_step` and k_polish_chunks'
    `r = kk * seq_step + j` at seq_length 1 (every row a chunk), (2, 1), and seq_length = the region's rows, one more, one fewer
    (one chunk, one chunk with a padding row, two chunks)"""
    edge, bare, tail = pc.TILE_EDGE_CASES[4]
    _, b, _, _ = _edge_case(edge, bare, tail)
    base, _ = _expected(oracle_lib, ("tile_edges", edge, bare, tail), b, 1000, 50)
    per_region = np.diff(base.region_row_off).tolist()
    rows = per_region[1]
    for L, O, second in ((1, 0, rows), (2, 1, rows - 1), (rows, 50, 1), (rows + 1, 50, 1), (rows - 1, 50, 2)):
        got = _exact(hip_ctx, oracle_lib, ("tile_edges", edge, bare, tail), b, L, O)
        assert len(py_chunks(rows, L, O)) == second
        assert len(got.images) == sum(len(py_chunks(n, L, O)) for n in per_region), (L, O)
        assert np.bincount(got.region).tolist() == [len(py_chunks(n, L, O)) for n in per_region]
