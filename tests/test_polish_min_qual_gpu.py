"""GPU: `polish --min_qual`: pv_polish_filter_low_qual[_dev] against the host checker (tests/min_qual_ref.py) on hand-made chunk
layouts (tests/min_qual_cases.py; seq_length 40, overlap 10, so that many chunks cost nothing, and the real 1000 / 50 once),
the error statuses, the identity with the edits and the stitch, the chain's calls as one captured graph, and the command end
to end on a small BAM. Device form = host form = checker, row for row, owned or not. Nothing here has a tolerance."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import depth_ref as dr
import edits_ref as er
import min_qual_cases as mc
import min_qual_ref as mq
import qual_ref as qr
import stitch_ref as sr
from pepper_thesis_amd import _ffi, bamio, cli, polish, polish_edits as pe, synth
from pepper_thesis_amd.device import DevicePolishOut

pytestmark = pytest.mark.gpu
L, O = 40, 10
MARK = 0xEE


def _device_chunks(lay, chunk_id=None, depth=None):
    do = DevicePolishOut(max(lay.n, 1), lay.L, lay.O, depth=depth is not None)
    for name in ("position", "index", "region", "chunk_id"):
        a = np.array(getattr(lay, name) if name != "chunk_id" or chunk_id is None else chunk_id)
        getattr(do, name)[:lay.n].copy_(torch.from_numpy(a))
    if depth is not None:
        do.set_depth(depth)
    return do


def _dev_filter(ctx, lay, labels, rq, min_qual, in_place=False, ref=True, qual=True, chunk_id=None, overlap=None, ref_off=None):
    """the device-resident form on uploaded copies; out of place the outputs are pre-filled with a marker -> (labels out, row
    qualities out, labels in and row qualities in as they are afterwards, counts), with the error code of the call in front
    when it was refused"""
    do = _device_chunks(lay, chunk_id)
    if overlap is not None:
        do.seq_overlap = overlap
    lab, drq = torch.from_numpy(np.array(labels)).cuda(), torch.from_numpy(np.array(rq)).cuda()
    lab_out = lab if in_place else torch.full_like(lab, MARK)
    rq_out = drq if in_place else torch.full_like(drq, MARK)
    rs = torch.from_numpy(np.array(lay.ref_start)).cuda()
    ro = torch.from_numpy(np.array(lay.ref_off if ref_off is None else ref_off)).cuda()
    d_ref = torch.from_numpy(np.array(lay.ref)).cuda()          # always as long as the layout's own ref_off says
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code = None
    try:
        ctx.polish_filter_low_qual_dev(do, lay.n, lab.data_ptr(), drq.data_ptr() if qual else 0, rs.data_ptr(), ro.data_ptr(),
                                       d_ref.data_ptr() if ref else 0, lay.n_regions, min_qual, lab_out.data_ptr(),
                                       rq_out.data_ptr() if qual else 0, counts.data_ptr())
    except _ffi.PepperHipError as e:
        code = e.code
    ctx.synchronize()
    res = (lab_out.cpu().numpy(), rq_out.cpu().numpy(), lab.cpu().numpy(), drq.cpu().numpy(), counts.cpu().numpy().tolist())
    return res if code is None else (code,) + res


def _check(ctx, lay, labels, rq, min_qual, runs):
    """all four forms against the checker -> the checker's (labels, qualities, reverted, pinned rows, reverted runs)"""
    want = mq.filter_low_qual(labels, rq, *lay.args(), min_qual, runs=runs)
    want_lab, want_q, reverted, pinned = want[:4]
    counts = (C.c_int64 * 4)()
    got_lab, got_q = ctx.polish_filter_low_qual(lay.out, labels, lay.batch, min_qual, rq, lay.L, lay.O, counts=counts)
    assert list(counts) == [reverted, 0, -1, pinned], min_qual
    assert np.array_equal(got_lab, want_lab) and np.array_equal(got_q, want_q), min_qual
    lab2, q2 = labels.copy(), rq.copy()                                                     # in place on the host
    r_lab, r_q = ctx.polish_filter_low_qual(lay.out, lab2, lay.batch, min_qual, q2, lay.L, lay.O, in_place=True)
    assert r_lab is lab2 and r_q is q2 and np.array_equal(lab2, want_lab) and np.array_equal(q2, want_q), min_qual
    for in_place in (False, True):
        out_lab, out_q, in_lab, in_q, c = _dev_filter(ctx, lay, labels, rq, min_qual, in_place=in_place)
        assert c == [reverted, 0, -1, pinned], (min_qual, in_place)
        assert np.array_equal(out_lab, want_lab) and np.array_equal(out_q, want_q), (min_qual, in_place)
        if not in_place:                                                                    # the inputs are read only
            assert np.array_equal(in_lab, labels) and np.array_equal(in_q, rq)
    # rows that own nothing are never written
    own = mq.owned_mask(lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, labels.shape) if lay.n < 100 else None
    assert own is None or (np.array_equal(want_lab[~own], labels[~own]) and np.array_equal(want_q[~own], rq[~own]))
    return want


def _sweep(ctx, lay, labels, rq, m):
    """min_qual in {0, 1, m, m + 1, 93, 94} for a run minimum m of the case -> {min_qual: checker result}"""
    runs = mq.region_runs(labels, rq, *lay.args())
    assert m in {r.minimum for r in runs}
    out = {q: _check(ctx, lay, labels, rq, q, runs) for q in sorted({0, 1, m, m + 1, 93, 94})}
    assert out[0][2:4] == (0, 0) and np.array_equal(out[0][0], labels) and np.array_equal(out[0][1], rq)      # the identity
    assert out[m][2] < out[m + 1][2] or out[m][3] < out[m + 1][3]                        # the run with minimum m goes at m + 1
    n_records, n_pinned = sum(len(r.records) for r in runs), sum(len(r.records) for r in runs if r.pinned)
    assert out[94][2:4] == (n_records - n_pinned, n_pinned)                               # every run that is not pinned
    return out, runs


def _row(lay, g, p, x=0):
    return lay.rows[g].index((p, x))


# ---- 1. sparse planted edits on labels that spell the draft, runs across chunk boundaries ----------------------------------

@pytest.fixture(scope="module")
def sparse():
    """a 13-chunk region (chunk ids 9 and 10 meet) with inserts; -> (layout, {variant: (labels, row qualities)}): variant
    'early' / 'late' puts the low quality of the run across the 9 -> 10 boundary on the side chunk 9 / chunk 10 owns"""
    rng = np.random.default_rng(11)
    lay = mc.Layout([(0, mc.acgt(rng, 380), {150: 3, 151: 1, 200: 5, 330: 6})], L, O)
    assert lay.n == 13 and len(lay.rows[0]) == 395
    out = {}
    for variant in ("early", "late"):
        lab, rq = lay.spelled(60)
        P = lambda r, what, q: lay.plant(lab, rq, 0, r, what, q)
        P(5, "sub", 10)                                                     # one record
        P(20, "del", 30); P(21, "del", 8)                                   # DEL + DEL
        for r, q in zip(range(40, 45), (50, 50, 6, 50, 50)):                # five substitutions, the minimum in the middle
            P(r, "sub", q)
        for r in range(100, 104):                                           # qualities at the ceiling: only 94 takes it back
            P(r, "sub", 93)
        # SUB + INS + INS, then DEL + INS at the next position: five records, the minimum on the third
        r0 = _row(lay, 0, 150)
        P(r0, "sub", 40); P(r0 + 1, 3, 40); P(r0 + 2, 1, 7); P(_row(lay, 0, 151), "del", 40); P(_row(lay, 0, 151, 1), 2, 40)
        P(_row(lay, 0, 200, 2), 4, 9)                                       # an inserted base alone, not the first of its position
        # across the ordinary hand-off 3 -> 4 (rows 120..129 are in both, chunk 4 owns them): the low column on chunk 3's side
        for r in range(116, 125):
            P(r, "sub", 5 if r == 117 else 50)
        # across 2 -> 3 (rows 90..99): the low column on chunk 3's side, chunk 2 holds the run's first records
        for r in range(86, 95):
            P(r, "del" if r % 2 else "sub", 4 if r == 93 else 50)
        # across 9 -> 10 (rows 300..309 are in both, and the EARLIER chunk owns them: "9" sorts behind "10")
        low = 298 if variant == "early" else 312
        for r in range(296, 315):
            P(r, "sub", 3 if r == low else 50)
        # a non-owned duplicate with another label and quality 0 (chunk 7's copy of row 243; chunk 8 owns and spells the draft)
        k, j = 7, 243 - 7 * (L - O)
        assert lay.position[k, j] == lay.position[8, j - (L - O)] and j >= L - O
        lab[k, j], rq[k, j] = (lab[k, j] % 4) + 1, 0
        # and the other way round: the owner holds a low edit, the duplicate spells the draft
        P(245, "sub", 2)
        lab[7, 245 - 7 * (L - O)], rq[7, 245 - 7 * (L - O)] = lay.spelled(77)[0][7, 245 - 7 * (L - O)], 77
        for a in (lab, rq):
            a.setflags(write=False)
        out[variant] = (lab, rq)
    return lay, out


@pytest.mark.parametrize("variant", ["early", "late"])
def test_sparse_edits_and_runs_across_chunk_boundaries(hip_ctx, sparse, variant):
    lay, cases = sparse
    lab, rq = cases[variant]
    out, runs = _sweep(hip_ctx, lay, lab, rq, 7)
    assert sorted(len(r.records) for r in runs) == [1, 1, 1, 2, 4, 5, 5, 9, 9, 19]
    kinds = {rec[2] for r in runs for rec in r.records}
    assert kinds == {er.SUB, er.DEL, er.INS}
    # the run over the 9 -> 10 boundary goes whole at 4 whichever side held its low column: rows of both chunks are rewritten
    want_lab = mq.filter_low_qual(lab, rq, *lay.args(), 4, runs=runs)[0]
    changed = np.argwhere(want_lab != lab)
    rows9 = {int(j) for k, j in changed if k == 9}
    rows10 = {int(j) for k, j in changed if k == 10}
    assert rows9 == set(range(296 - 270, 40)) and rows10 == set(range(10, 315 - 300))     # chunk 9 owns the overlap
    got = _dev_filter(hip_ctx, lay, lab, rq, 4, in_place=True)
    assert np.array_equal(got[0], want_lab)
    # the duplicates: chunk 7's copies are as they were, at every threshold
    for q in out:
        assert out[q][0][7, 243 - 210] == lab[7, 243 - 210] != lab[8, 243 - 240] and out[q][1][7, 243 - 210] == 0
        assert out[q][0][7, 245 - 210] == lab[7, 245 - 210] and out[q][1][7, 245 - 210] == 77
    assert out[94][0][8, 245 - 240] == lab[7, 245 - 210] != lab[8, 245 - 240]             # the owner's edit went
    # chunks without an owned edit stand between chunks with edits
    edited = {k for r in runs for k, _ in r.rows}
    assert {0, 1, 5, 6, 8, 9, 10} <= edited and 11 not in edited and 12 not in edited and 7 not in edited


# ---- 2. every column edited: a region is one run through all its chunks ------------------------------------------------------

def test_a_region_that_is_one_run(hip_ctx):
    rng = np.random.default_rng(12)
    lay = mc.Layout([(0, mc.acgt(rng, 90), {10: 4, 50: 6})], L, O)
    assert lay.n == 3 and len(lay.rows[0]) == 100
    lab, rq = lay.all_edited(50)
    out, runs = _sweep(hip_ctx, lay, lab, rq, 50)                  # every quality >= Q = 50: nothing goes; at 51 everything
    assert len(runs) == 1 and len(runs[0].records) == 100 and out[50][2] == 0 and out[51][2] == 100
    rq = rq.copy()
    rq[lay.where(0, 45)] = 5                                       # the minimum in the middle chunk (rows 40..59 are its own)
    out, runs = _sweep(hip_ctx, lay, lab, rq, 5)
    assert {k for k, _ in runs[0].rows} == {0, 1, 2} and runs[0].rows[45] == (1, 15)
    assert out[5][2] == 0 and out[6][2] == 100
    spelled = lay.spelled()[0]
    own = mq.owned_mask(*lay.args()[:5], lab.shape)
    assert np.array_equal(out[6][0][own], spelled[own]) and not out[6][1][own].any()


# ---- 3. regions: runs end where the region ends; the dropped buffer of a region that starts late ----------------------------

@pytest.mark.parametrize("low_in", [0, 1])
def test_adjacent_regions_are_judged_apart(hip_ctx, low_in):
    """region 0 ends at position 259 with a run on its last columns; region 1 = [59, 400] keeps 260.. and starts with a run on
    its first kept columns: in the VCF they are one block, here two runs, and only the one that holds the low column goes.
    Region 1's copies of 258 and 259 lie in its dropped buffer: their low edits belong to no run."""
    rng = np.random.default_rng(13)
    lay = mc.Layout([(0, mc.acgt(rng, 260), {}), (59, mc.acgt(rng, 342), {})], L, O)
    lab, rq = lay.spelled(60)
    for p in (257, 258, 259):
        lay.plant(lab, rq, 0, _row(lay, 0, p), "sub", 3 if low_in == 0 and p == 259 else 50)
    for p in (260, 261):
        lay.plant(lab, rq, 1, _row(lay, 1, p), "sub", 3 if low_in == 1 and p == 260 else 50)
    for p in (258, 259):
        lay.plant(lab, rq, 1, _row(lay, 1, p), "del", 1)          # inside the buffer, adjacent to the kept edit at 260
    out, runs = _sweep(hip_ctx, lay, lab, rq, 3)
    assert [(r.region, [rec[0] for rec in r.records]) for r in runs] == [(0, [257, 258, 259]), (1, [260, 261])]
    gone = out[4][4]
    assert [r.region for r in gone] == [low_in] and out[4][2] == (3, 2)[low_in] and out[3][2] == 0
    buffered = lay.where(1, _row(lay, 1, 259))
    assert (out[94][0][buffered] == 0).all() and (out[94][1][buffered] == 1).all()        # never touched


# ---- 4. random layouts: bytes that cannot be spelled, several regions, the real sizes ---------------------------------------

def _random_case(seed, regions, LL, OO, p_edit):
    rng = np.random.default_rng(seed)
    regs = []
    for start, n, n_ins in regions:
        d = np.frombuffer(mc.acgt(rng, n), np.uint8).copy()
        odd = rng.random(n) < 0.03
        d[odd] = rng.choice(np.frombuffer(b"NnRYkMs", np.uint8), int(odd.sum()))
        ins = {int(p): int(rng.integers(1, 4)) for p in rng.choice(np.arange(start, start + n), n_ins, replace=False)}
        regs.append((start, d.tobytes(), ins))
    lay = mc.Layout(regs, LL, OO)
    # labels and qualities are functions of (region, position, index), so that the copies of a row agree
    lab, _ = lay.spelled()
    top = int(lay.position.max()) + 1
    g = np.broadcast_to(lay.region[:, None], lay.position.shape)
    key = (g * top + np.maximum(lay.position, 0)) * 4 + np.maximum(lay.index, 0)
    table_e, table_l = rng.random(int(key.max()) + 1) < p_edit, rng.integers(0, 5, int(key.max()) + 1)
    table_q = rng.integers(1, 94, int(key.max()) + 1)
    lab = np.where(table_e[key] & (lay.position >= 0), table_l[key], lab).astype(np.uint8)
    rq = table_q[key].astype(np.uint8)
    return lay, lab, rq


@pytest.mark.parametrize("sizes", [(40, 10), (1000, 50)], ids=["40_10", "1000_50"])
def test_random_layouts(hip_ctx, sizes):
    LL, OO = sizes
    n, n_ins = (12_300, 20) if LL == 1000 else (370, 10)           # 13 chunks either way: chunk ids 9 and 10 meet
    lay, lab, rq = _random_case(21, [(0, n, n_ins), (500, 290 if LL == 40 else 1_100, 3), (900, 300, 5)], LL, OO, 0.5)
    assert 13 in [int((lay.region == g).sum()) for g in range(3)]
    runs = mq.region_runs(lab, rq, *lay.args())
    lengths = [len(r.records) for r in runs]
    assert max(lengths) >= 5 and min(lengths) == 1 and any(r.pinned for r in runs) and len({r.region for r in runs}) == 3
    m = sorted(r.minimum for r in runs if not r.pinned)[len(runs) // 3]
    _sweep(hip_ctx, lay, lab, rq, m)


def test_a_few_thousand_chunks(hip_ctx):
    """3667 chunks: every thread of the one-block pass holds several. Region 0 is one run through 1667 chunks with its minimum
    far from either end; region 1 holds sparse runs; region 2 is all edits again and starts late."""
    rng = np.random.default_rng(31)
    lay = mc.Layout([(0, mc.acgt(rng, 50_000), {}), (0, mc.acgt(rng, 30_000), {7: 2}), (1_000, mc.acgt(rng, 30_000), {})], L, O)
    assert lay.n == 3667 > 3 * 1024 and int((lay.region == 0).sum()) == 1667
    lab, rq = lay.all_edited(60)
    spelled = lay.spelled()[0]
    g = np.broadcast_to(lay.region[:, None], lay.position.shape)
    edit_at = rng.random(31_001) < 0.1
    q_at = rng.integers(1, 94, 31_001)
    sparse_rows = (g == 1) & ~edit_at[np.clip(lay.position, 0, 31_000)]
    lab = np.where(sparse_rows, spelled, lab)
    rq = np.where(g == 1, q_at[np.clip(lay.position, 0, 31_000)], rq).astype(np.uint8)
    rq[lay.where(0, 20_000)] = 9
    out, runs = _sweep(hip_ctx, lay, lab, rq, 9)
    assert len(runs[0].records) == 50_000 and runs[0].minimum == 9 and len(runs[-1].records) == 30_000 - 201
    assert out[10][2] >= 50_000 and out[9][2] < 50_000 and len(runs) > 1_000


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------

def _untouched(res, labels, rq, in_place):
    out_lab, out_q, in_lab, in_q = res[:4]
    assert np.array_equal(in_lab, labels) and np.array_equal(in_q, rq)
    if not in_place:
        assert (out_lab == MARK).all() and (out_q == MARK).all()


@pytest.mark.parametrize("in_place", [False, True])
def test_invalid_calls_touch_nothing(hip_ctx, sparse, in_place):
    lay, cases = sparse
    lab, rq = cases["early"]
    for kw, q in ((dict(qual=False), 20), (dict(ref=False), 20), (dict(), 95), (dict(), -1), (dict(overlap=21), 20)):
        res = _dev_filter(hip_ctx, lay, lab, rq, q, in_place=in_place, **kw)
        assert res[0] == _ffi.PV_ERR_INVALID and res[-1] == [-7] * 4, (kw, q)               # refused by the call itself
        _untouched(res[1:], lab, rq, in_place)
    # a broken chunk layout
    ids = lay.chunk_id.copy()
    ids[[4, 5]] = ids[[5, 4]]
    res = _dev_filter(hip_ctx, lay, lab, rq, 94, in_place=in_place, chunk_id=ids)
    assert res[-1] == [0, _ffi.PV_ERR_INVALID, 4, 0]
    _untouched(res, lab, rq, in_place)
    # the draft one byte shorter than the region: its last position is owned and has no draft byte
    short = lay.ref_off.copy()
    short[-1] -= 1
    res = _dev_filter(hip_ctx, lay, lab, rq, 94, in_place=in_place, ref_off=short)
    assert res[-1] == [0, _ffi.PV_ERR_INVALID, 12, 0]
    _untouched(res, lab, rq, in_place)
    # an owned label 5: PV_ERR_STATE and nothing written; on a column that owns nothing it is not an error
    bad = lab.copy()
    bad[3, 7] = 5
    res = _dev_filter(hip_ctx, lay, bad, rq, 94, in_place=in_place)
    assert res[-1] == [0, _ffi.PV_ERR_STATE, 3, 0]
    _untouched(res, bad, rq, in_place)
    bad[4, 20] = 5
    bad[5, 9] = 5                                                       # with a broken layout before it: the first bad chunk decides
    res = _dev_filter(hip_ctx, lay, bad, rq, 94, in_place=in_place, chunk_id=np.array([0, 2, 1] + list(range(3, 13)), np.int32))
    assert res[-1] == [0, _ffi.PV_ERR_INVALID, 1, 0]
    loser = lab.copy()
    loser[7, 35] = 5                                                    # chunk 7's copy of row 245, which chunk 8 owns
    res = _dev_filter(hip_ctx, lay, loser, rq, 94, in_place=in_place)
    want = mq.filter_low_qual(lab, rq, *lay.args(), 94)
    want[0][7, 35] = 5
    assert res[-1][1] == 0 and np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1])


def test_invalid_calls_of_the_host_form(hip_ctx, sparse):
    lay, cases = sparse
    lab, rq = cases["late"]
    no_ref = types.SimpleNamespace(ref_start=lay.ref_start, ref_off=lay.ref_off, ref=None)
    bad = lab.copy()
    bad[3, 7] = 5
    swapped = types.SimpleNamespace(position=lay.position, index=lay.index, region=lay.region,
                                    chunk_id=np.array([0, 2, 1] + list(range(3, 13)), np.int32))
    for chunks, batch, labels, q, o, code in ((lay.out, no_ref, lab, 20, O, _ffi.PV_ERR_INVALID), (lay.out, lay.batch, lab, 95, O, _ffi.PV_ERR_INVALID),
                                              (lay.out, lay.batch, lab, 20, 21, _ffi.PV_ERR_INVALID),
                                              (swapped, lay.batch, lab, 20, O, _ffi.PV_ERR_INVALID),
                                              (lay.out, lay.batch, bad, 20, O, _ffi.PV_ERR_STATE)):
        lab2, q2 = labels.copy(), rq.copy()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_filter_low_qual(chunks, lab2, batch, q, q2, L, o, in_place=True)
        assert e.value.code == code
        assert np.array_equal(lab2, labels) and np.array_equal(q2, rq)
    with pytest.raises(_ffi.PepperHipError) as e:                       # no row qualities
        hip_ctx.polish_filter_low_qual(lay.out, lab.copy(), lay.batch, 20, None, L, O)
    assert e.value.code == _ffi.PV_ERR_INVALID


def test_no_chunks(hip_ctx, sparse):
    lay = sparse[0]
    none = types.SimpleNamespace(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32), region=np.zeros(0, np.int32),
                                 chunk_id=np.zeros(0, np.int32))
    counts = (C.c_int64 * 4)()
    lab, q = hip_ctx.polish_filter_low_qual(none, np.zeros((0, L), np.uint8), lay.batch, 20, np.zeros((0, L), np.uint8), L, O, counts=counts)
    assert list(counts) == [0, 0, -1, 0] and lab.shape == (0, L) and q.shape == (0, L)


# ---- 6. the identity with the edits and the stitch ---------------------------------------------------------------------------

@pytest.mark.parametrize("min_qual", [8, 51, 94])
def test_identity_with_edits_and_stitch(hip_ctx, sparse, min_qual):
    """edits(labels_out) = edits(labels) minus the records of the reverted runs; stitch(labels_out) = those records applied
    to the draft; every record that is left has QUAL >= min_qual"""
    lay, cases = sparse
    lab, rq = cases["late"]
    want_lab, want_q, reverted, pinned, gone = mq.filter_low_qual(lab, rq, *lay.args(), min_qual)
    assert 0 < len(gone)
    lab_out, q_out = hip_ctx.polish_filter_low_qual(lay.out, lab, lay.batch, min_qual, rq, L, O)
    eoff, before = hip_ctx.polish_edits(lay.out, lab, lay.batch, row_qual=rq, seq_length=L, seq_overlap=O)
    eoff2, after = hip_ctx.polish_edits(lay.out, lab_out, lay.batch, row_qual=q_out, seq_length=L, seq_overlap=O)
    dropped = {(rec[0], rec[1]) for r in gone for rec in r.records}
    keep = np.array([(int(p), int(x)) not in dropped for p, x in zip(before["position"], before["index"])], bool)
    assert len(dropped) == reverted == int((~keep).sum()) and np.array_equal(after, before[keep])
    roff, seq, qual = hip_ctx.polish_stitch_qual(lay.out, lab_out, q_out, lay.ref_start, seq_length=L, seq_overlap=O)
    draft = lay.ref.tobytes()
    records = pe.compose_records("c", after, draft, True)
    assert er.apply([tuple(r) for r in records], draft) == seq.decode()
    assert all(r.qual >= min_qual for r in records) and (len(records) > 0) == (min_qual < 94)
    if min_qual == 94:
        assert seq.decode() == draft.decode().upper()


# ---- 7. one linear graph -------------------------------------------------------------------------------------------------------

def test_graph_of_row_qual_mask_filter_stitch_qual_and_edits(hip_ctx):
    """row qualities, minimum-depth mask (in place), minimum-quality filter (in place), stitch with qualities and edits captured
    as one graph on one stream; replays on refilled labels and softmax sums equal the eager calls, and those the checkers"""
    lay, _, _ = _random_case(41, [(0, 380, 20), (500, 300, 5)], L, O, 0.3)
    n, G = lay.n, lay.n_regions
    rng = np.random.default_rng(42)
    key = np.maximum(lay.position, 0) * 4 + np.maximum(lay.index, 0) + 4_000 * lay.region[:, None]
    depth = rng.integers(0, 6, int(key.max()) + 1)[key].astype(np.uint16)
    do = _device_chunks(lay, depth=depth)
    rs, ro, ref = (torch.from_numpy(np.array(a)).cuda() for a in (lay.ref_start, lay.ref_off, lay.ref))
    fills = []
    for s in range(3):
        r = np.random.default_rng(70 + s)
        lab = r.integers(0, 5, int(key.max()) + 1)[key].astype(np.uint8)
        lab = np.where(r.random(int(key.max()) + 1)[key] < 0.6, lay.spelled()[0], lab).astype(np.uint8)
        # the winning softmax sum 2 * (1 - 10^-5u), u uniform: qualities spread over 0..50
        acc = (1.0 - 10.0 ** (-5.0 * r.random(int(key.max()) + 1)))[key][..., None].astype(np.float32) * np.ones(5, np.float32) * 2.0
        acc[:, :O] /= 2
        acc[:, L - O:] /= 2
        fills.append((lab, acc))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq, qual = (torch.zeros(n * L, dtype=torch.uint8, device="cuda") for _ in range(2))
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    roff, eoff = (torch.zeros(G + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    c_rq, c_mk, c_fl, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(5))
    st = hip_ctx.stream
    MD, MQ = 2, 30

    def passes():
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_rq.data_ptr(), L, O, stream=st)
        hip_ctx.polish_mask_low_depth_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G,
                                          MD, lab_d.data_ptr(), rq_d.data_ptr(), c_mk.data_ptr(), stream=st)
        hip_ctx.polish_filter_low_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G,
                                           MQ, lab_d.data_ptr(), rq_d.data_ptr(), c_fl.data_ptr(), stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), G, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G,
                                 eoff.data_ptr(), buf.data_ptr(), n * L, c_ed.data_ptr(), stream=st)

    def state():
        t, e = int(c_st[0].item()), int(c_ed[0].item())
        return (lab_d.cpu().numpy().tobytes(), rq_d.cpu().numpy().tobytes(), seq[:t].cpu().numpy().tobytes(),
                qual[:t].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(), roff.cpu().numpy().tolist(),
                eoff.cpu().numpy().tolist(), c_mk.cpu().numpy().tolist(), c_fl.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(),
                c_ed.cpu().numpy().tolist())

    eager = []
    for lab, acc in fills:
        lab_d.copy_(torch.from_numpy(lab)); acc_d.copy_(torch.from_numpy(acc))
        torch.cuda.synchronize()
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        q0 = qr.row_qual(lab, acc, O)
        m_lab, m_q, masked, unmaskable = dr.mask(lab, q0, depth, lay.position, lay.index, lay.region, lay.ref_start, lay.ref_off,
                                                 lay.ref, MD)
        want_lab, want_q, reverted, pinned, gone = mq.filter_low_qual(m_lab, m_q, *lay.args(), MQ)
        assert eager[-1][0] == want_lab.tobytes() and eager[-1][1] == want_q.tobytes()
        assert eager[-1][7] == [masked, 0, -1, unmaskable] and eager[-1][8] == [reverted, 0, -1, pinned] and reverted > 20 and masked > 20
        h_roff, h_seq, h_qual = hip_ctx.polish_stitch_qual(lay.out, want_lab, want_q, lay.ref_start, seq_length=L, seq_overlap=O)
        assert (eager[-1][2], eager[-1][3], eager[-1][5]) == (h_seq, h_qual, h_roff.tolist())
    assert eager[0][2] != eager[1][2]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        lab_d.copy_(torch.from_numpy(fills[k][0])); acc_d.copy_(torch.from_numpy(fills[k][1]))
        for t in (rq_d, seq, qual, buf, roff, eoff, c_mk, c_fl, c_st, c_ed):
            t.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 8. the command ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two contigs of a few kb with an ACGT / acgt draft (nothing pinned), covered by reads; seeded P2 weights"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("min_qual")
    rng = np.random.default_rng(43)
    contigs = [("ctgA", "".join(rng.choice(list("ACGTacgt"), size=3_200))), ("ctgB", "".join(rng.choice(list("ACGTacgt"), size=2_100)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=900)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    # dense gain 100: the seeded weights then give row qualities from 3 to 93 with about two in three at 20 or above (gain 3
    # gives nothing above 2), so that at --min_qual 20 some runs go and some stay
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(37, 100.0))
    return tmp, dict(contigs)


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what the filter of every launch was given and what it left"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        ctx, real, seen = self.ctx, self.ctx.polish_filter_low_qual_dev, {}

        def spy(dout, n_chunks, *a, **k):
            ctx.synchronize()
            seen.update(labels_in=self.labels[:n_chunks].cpu().numpy(), row_qual_in=self.row_qual[:n_chunks].cpu().numpy(),
                        acc=self.acc[:n_chunks].cpu().numpy())
            return real(dout, n_chunks, *a, **k)
        ctx.polish_filter_low_qual_dev = spy
        try:
            res = super()._labels_and_stitch(db, n, n_regions)
        finally:
            del ctx.polish_filter_low_qual_dev
        if n:
            d = self.dout
            seen.update(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(), region=d.region[:n].cpu().numpy(),
                        chunk_id=d.chunk_id[:n].cpu().numpy(), labels=self.labels[:n].cpu().numpy(),
                        row_qual=self.row_qual[:n].cpu().numpy(),
                        ref_start=db.t["ref_start"][:n_regions].cpu().numpy(), ref_end=db.t["ref_end"][:n_regions].cpu().numpy(),
                        ref_off=db.t["ref_off"][:n_regions + 1].cpu().numpy(), ref=db.t["ref"].cpu().numpy(), filtered=res.filtered)
            self.launches.append(seen)
        return res


def _recording_opener(hip_ctx, chains):
    def open_chain(device, shared, state_dict, dtype, **kw):
        hip_ctx.load_p2(state_dict, dtype)
        chains.append(_RecordingChain(hip_ctx, **kw))
        return chains[-1]
    return open_chain


def _fasta(path):
    lines = open(path).read().split("\n")
    return dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))


def _polish(inputs, hip_ctx, name, flags, chains=None):
    t, _ = inputs
    out_dir = str(t / name)
    argv = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8", "-o", out_dir] + flags
    kw = {} if chains is None else dict(open_chain=_recording_opener(hip_ctx, chains))
    if chains is None:
        def open_chain(device, shared, state_dict, dtype, **k):
            hip_ctx.load_p2(state_dict, dtype)
            return polish._DeviceChain(hip_ctx, **k)
        kw = dict(open_chain=open_chain)
    assert polish.run(cli.polish_parser().parse_args(argv), **kw) == 0
    return out_dir


def test_min_qual_94_gives_the_draft(inputs, hip_ctx, opts):
    """weight-independent: no quality reaches 94 and the drafts hold no byte that cannot be spelled, so every edit goes"""
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    out_dir = _polish(inputs, hip_ctx, "all", ["--min_qual", "94", "--edits"], chains)
    assert chains[0].min_qual == 94 and not chains[0].qualities and len(chains[0].launches) > 1
    for la in chains[0].launches:
        assert la["filtered"][0] > 100 and la["filtered"][1] == 0 and (la["labels"] != la["labels_in"]).any()
    assert _fasta(os.path.join(out_dir, "_pepper_polished.fa")) == {c: d.upper() for c, d in drafts.items()}
    assert not os.path.exists(os.path.join(out_dir, "_pepper_polished.fq"))               # no --qualities: no FASTQ
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(os.path.join(out_dir, "_pepper_polished.edits.vcf.gz")).decode())
    assert recs == [] and header[3:] == ["contig=<ID=ctgA,length=3200>", "contig=<ID=ctgB,length=2100>", "pepper_min_qual=94"]


@pytest.mark.parametrize("flags", [[], ["--realign", "--gpu_decode", "--min_depth", "3"]], ids=["plain", "all_flags"])
def test_min_qual_20_end_to_end(inputs, hip_ctx, opts, flags):
    from pepper_thesis_amd.bamio import BamHandler, FastaHandler
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    out_dir = _polish(inputs, hip_ctx, "twenty_" + ("flags" if flags else "plain"), ["--min_qual", "20", "--edits", "--qualities"] + flags,
                      chains)
    launches = chains[0].launches
    work, _ = polish.polish_work(FastaHandler(str(t / "ref.fa")), BamHandler(str(t / "reads.bam")), None)
    parts, quals, w, reverted = {}, {}, 0, 0
    for la in launches:
        if not flags:      # nothing stands between the row qualities and the filter: they are the checker's of labels and acc
            assert np.array_equal(la["row_qual_in"], qr.row_qual(la["labels_in"], la["acc"], 50))
        want_lab, want_q, n_rev, n_pin, gone = mq.filter_low_qual(la["labels_in"], la["row_qual_in"], la["position"], la["index"],
                                                                  la["region"], la["chunk_id"], la["ref_start"], la["ref_off"],
                                                                  la["ref"], 20)
        assert np.array_equal(la["labels"], want_lab) and np.array_equal(la["row_qual"], want_q) and la["filtered"] == (n_rev, n_pin)
        reverted += n_rev
        spans = list(zip(la["ref_start"].tolist(), la["ref_end"].tolist()))
        regs = qr.regions_with_qual(la["position"], la["index"], la["region"], la["chunk_id"], want_lab, want_q, spans)
        for g, reg in enumerate(regs):
            while (work[w].start, work[w].end) != spans[g]:
                w += 1
            _, _, parts[work[w].index], quals[work[w].index] = qr.small_chunk_stitch_qual([reg])
            w += 1
    assert reverted > 100 and len(parts) == len(work)
    assert sum(int((la["labels"] != la["labels_in"]).sum()) for la in launches) == reverted
    want = {c: "".join(parts[wk.index] for wk in work if wk.contig == c) for c in drafts}
    want_q = {c: b"".join(quals[wk.index] for wk in work if wk.contig == c) for c in drafts}
    got = _fasta(os.path.join(out_dir, "_pepper_polished.fa"))
    assert got == want
    fq = open(os.path.join(out_dir, "_pepper_polished.fq")).read().split("\n")
    assert fq[0::4][:2] == ["@ctgA", "@ctgB"] and fq[1::4] == [want["ctgA"], want["ctgB"]]
    assert fq[3::4] == ["".join(chr(33 + q) for q in want_q[c]) for c in ("ctgA", "ctgB")]
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(os.path.join(out_dir, "_pepper_polished.edits.vcf.gz")).decode())
    assert header[3:] == ["contig=<ID=ctgA,length=3200>", "contig=<ID=ctgB,length=2100>"] + (["pepper_min_depth=3"] if flags else []) + \
        ["pepper_min_qual=20"]
    for c in drafts:
        mine = [r[1:] for r in recs if r[0] == c]
        assert er.apply(mine, drafts[c].encode()) == got[c] and mine, c                    # the records applied to the draft
        assert all(r[3] >= 20 for r in mine), c


def test_min_qual_0_changes_no_byte(inputs, hip_ctx, opts):
    opts(shared_device=1)
    a = _polish(inputs, hip_ctx, "plain", ["--edits", "--qualities"])
    b = _polish(inputs, hip_ctx, "zero", ["--edits", "--qualities", "--min_qual", "0"])
    names = sorted(os.listdir(a))
    assert len(names) == 4 and names == sorted(os.listdir(b))
    for f in names:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
