"""GPU: `polish --min_support`: pv_polish_filter_low_support[_dev] against the host checker (tests/min_support_ref.py) on hand-made
chunk layouts (tests/min_qual_cases.py; seq_length 40, overlap 10, so that many chunks cost nothing, and the real 1000 / 50
once) with planted counts planes, the error statuses, the commutation with the minimum-quality filter, the identity with the
edits, their evidence and the stitch, the chain's calls as one captured graph, and the command end to end on small BAMs.
Device form = host form = checker, row for row, owned or not. Nothing here has a tolerance."""
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
import min_support_ref as ms
import qual_ref as qr
from pepper_thesis_amd import _ffi, bamio, cli, polish, polish_edits as pe, synth
from pepper_thesis_amd.device import DevicePolishOut
from test_polish_hp_gpu import inputs as hp_inputs         # the tagged BAM and its two pre-split files

pytestmark = pytest.mark.gpu
L, O = 40, 10
MARK = 0xEE
TOP = 65535


# ---- planes and calls ----------------------------------------------------------------------------------------------------------

def _counts_for(lab, fwd, rev):
    """a counts plane [n, L, 10] in which fwd[k, j] forward and rev[k, j] reverse reads spell row (k, j)'s own label (label 0:
    the deleted planes) and 40 forward reads hold another base"""
    b = lab.astype(np.int64)
    kk, jj = np.indices(lab.shape)
    c = np.zeros(lab.shape + (10,), np.uint16)
    c[kk, jj, 4 + b % 4] = 40
    c[kk, jj, np.where(b == 0, 8, b - 1)] = rev
    c[kk, jj, np.where(b == 0, 9, 4 + b - 1)] = fwd
    return c


def _keyed(lay, table_of):
    """values that are functions of (region, position, index), so that the copies of a row agree: table_of(size) -> a table"""
    top = int(lay.position.max()) + 1
    g = np.broadcast_to(lay.region[:, None], lay.position.shape)
    key = (g * top + np.maximum(lay.position, 0)) * 8 + np.maximum(lay.index, 0)
    return table_of(int(key.max()) + 1)[key]


def _host_out(lay, counts, depth, chunk_id=None):
    return types.SimpleNamespace(position=lay.position, index=lay.index, region=lay.region,
                                 chunk_id=lay.chunk_id if chunk_id is None else chunk_id, depth=depth, counts=counts)


def _device_chunks(lay, counts, depth, chunk_id=None, planes=(True, True)):
    do = DevicePolishOut(max(lay.n, 1), lay.L, lay.O, depth=planes[0], counts=planes[1])
    for name in ("position", "index", "region", "chunk_id"):
        a = np.array(getattr(lay, name) if name != "chunk_id" or chunk_id is None else chunk_id)
        getattr(do, name)[:lay.n].copy_(torch.from_numpy(a))
    if planes[0]:
        do.set_depth(np.array(depth))        # (copies: the fixtures' planes are read-only)
    if planes[1]:
        do.set_row_counts(np.array(counts))
    return do


def _dev_filter(ctx, lay, labels, rq, counts, depth, k, in_place=False, ref=True, qual=(True, True), chunk_id=None, overlap=None,
                ref_off=None, planes=(True, True)):
    """the device-resident form on uploaded copies; out of place the outputs are pre-filled with a marker -> (labels out, row
    qualities out, labels in and row qualities in as they are afterwards, counts, the planes as they are afterwards), with
    the error code of the call in front when it was refused. rq None: no quality plane (a dummy is carried along)."""
    do = _device_chunks(lay, counts, depth, chunk_id, planes)
    if overlap is not None:
        do.seq_overlap = overlap
    if rq is None:
        rq, qual = np.zeros_like(labels), (False, False)
    lab, drq = torch.from_numpy(np.array(labels)).cuda(), torch.from_numpy(np.array(rq)).cuda()
    lab_out = lab if in_place else torch.full_like(lab, MARK)
    rq_out = drq if in_place else torch.full_like(drq, MARK)
    rs = torch.from_numpy(np.array(lay.ref_start)).cuda()
    ro = torch.from_numpy(np.array(lay.ref_off if ref_off is None else ref_off)).cuda()
    d_ref = torch.from_numpy(np.array(lay.ref)).cuda()          # always as long as the layout's own ref_off says
    cnt = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code = None
    try:
        ctx.polish_filter_low_support_dev(do, lay.n, lab.data_ptr(), drq.data_ptr() if qual[0] else 0, rs.data_ptr(), ro.data_ptr(),
                                          d_ref.data_ptr() if ref else 0, lay.n_regions, k, lab_out.data_ptr(),
                                          rq_out.data_ptr() if qual[1] else 0, cnt.data_ptr())
    except _ffi.PepperHipError as e:
        code = e.code
    ctx.synchronize()
    after = (do.row_counts_numpy(lay.n) if planes[1] else None, do.depth_numpy(lay.n) if planes[0] else None)
    res = (lab_out.cpu().numpy(), rq_out.cpu().numpy(), lab.cpu().numpy(), drq.cpu().numpy(), cnt.cpu().numpy().tolist(), after)
    return res if code is None else (code,) + res


def _check(ctx, lay, labels, rq, counts, depth, k, runs):
    """all four forms against the checker -> the checker's (labels, qualities, reverted, pinned rows, reverted runs)"""
    want = ms.filter_low_support(labels, rq, counts, depth, *lay.args(), k, runs=runs)
    want_lab, want_q, reverted, pinned = want[:4]
    out = _host_out(lay, counts, depth)
    cnt = (C.c_int64 * 4)()
    got_lab, got_q = ctx.polish_filter_low_support(out, labels, lay.batch, k, rq, lay.L, lay.O, counts=cnt)
    assert list(cnt) == [reverted, 0, -1, pinned], k
    assert np.array_equal(got_lab, want_lab) and (rq is None and got_q is None or np.array_equal(got_q, want_q)), k
    lab2, q2 = labels.copy(), None if rq is None else rq.copy()                             # in place on the host
    r_lab, r_q = ctx.polish_filter_low_support(out, lab2, lay.batch, k, q2, lay.L, lay.O, in_place=True)
    assert r_lab is lab2 and r_q is q2 and np.array_equal(lab2, want_lab) and (rq is None or np.array_equal(q2, want_q)), k
    for in_place in (False, True):
        out_lab, out_q, in_lab, in_q, c, planes = _dev_filter(ctx, lay, labels, rq, counts, depth, k, in_place=in_place)
        assert c == [reverted, 0, -1, pinned], (k, in_place)
        assert np.array_equal(out_lab, want_lab), (k, in_place)
        if rq is not None:
            assert np.array_equal(out_q, want_q), (k, in_place)
        elif not in_place:
            assert (out_q == MARK).all()                                                    # no quality plane: none written
        assert np.array_equal(planes[0], counts) and np.array_equal(planes[1], depth)       # the inputs are read only
        if not in_place:
            assert np.array_equal(in_lab, labels) and (rq is None or np.array_equal(in_q, rq))
    # rows that own nothing are never written
    own = mq.owned_mask(lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, labels.shape) if lay.n < 100 else None
    assert own is None or np.array_equal(want_lab[~own], labels[~own])
    return want


def _sweep(ctx, lay, labels, rq, counts, depth, s):
    """min_support in {0, 1, s, s + 1, 65535} for a run minimum s of the case -> ({min_support: checker result}, runs)"""
    runs = ms.region_runs(labels, counts, depth, *lay.args())
    assert s in {r.minimum for r in runs}
    out = {k: _check(ctx, lay, labels, rq, counts, depth, k, runs) for k in sorted({0, 1, s, s + 1, TOP})}
    assert out[0][2:4] == (0, 0) and np.array_equal(out[0][0], labels)                          # the identity
    assert out[s][2] < out[s + 1][2] or out[s][3] < out[s + 1][3]                        # the run with minimum s goes at s + 1
    for r in runs:                                                                        # at s + 1 and not at s
        if r.minimum == s and not r.pinned:
            assert r not in out[s][4] and r in out[s + 1][4]
    n_records, n_pinned = sum(len(r.records) for r in runs), sum(len(r.records) for r in runs if r.pinned)
    assert out[TOP][2:4] == (n_records - n_pinned, n_pinned)                              # every run that is not pinned (no count is 65535)
    return out, runs


def _row(lay, g, p, x=0):
    return lay.rows[g].index((p, x))


# ---- 1. sparse planted edits on labels that spell the draft, runs across chunk boundaries ----------------------------------

@pytest.fixture(scope="module")
def sparse():
    """a 13-chunk region (chunk ids 9 and 10 meet) with inserts; -> (layout, {variant: (labels, row qualities, counts, depth)}):
    variant 'early' / 'late' puts the weak column of each run across a hand-off (3 -> 4, 2 -> 3, 9 -> 10) on the side of the
    earlier / the later chunk"""
    rng = np.random.default_rng(11)
    lay = mc.Layout([(0, mc.acgt(rng, 380), {150: 3, 151: 1, 200: 5, 330: 6})], L, O)
    assert lay.n == 13 and len(lay.rows[0]) == 395
    out = {}
    for variant in ("early", "late"):
        early = variant == "early"
        lab, rq = lay.spelled(60)
        fwd, rev = np.full(lab.shape, 30, np.uint16), np.full(lab.shape, 20, np.uint16)

        def P(r, what, f, v):       # an edit on row r that f forward and v reverse reads spell
            lay.plant(lab, rq, 0, r, what, 60)
            fwd[lay.where(0, r)], rev[lay.where(0, r)] = f, v
        P(5, "sub", 6, 4)                                                   # one record
        P(12, "sub", 0, 0)                                                  # to a base no read holds (another has 40 reads)
        P(20, "del", 15, 15); P(21, "del", 8, 0)                            # DEL + DEL
        for r, f in zip(range(40, 45), (50, 50, 6, 50, 50)):                # five substitutions, the minimum in the middle,
            P(r, "sub", f, 0)                                               # all on the forward strand only
        # SUB + INS + INS, then DEL + INS at the next position: five records, the minimum on the third
        r0 = _row(lay, 0, 150)
        P(r0, "sub", 20, 20); P(r0 + 1, 3, 20, 20); P(r0 + 2, 1, 3, 4); P(_row(lay, 0, 151), "del", 20, 20); P(_row(lay, 0, 151, 1), 2, 20, 20)
        P(_row(lay, 0, 200, 2), 4, 0, 9)                                    # an inserted base alone, not the first of its position
        # across the ordinary hand-off 3 -> 4 (rows 120..129 are in both, chunk 4 owns them)
        for r in range(116, 125):
            P(r, "sub", 5 if r == (117 if early else 123) else 50, 0)
        # across 2 -> 3 (rows 90..99 are in both, chunk 3 owns them)
        for r in range(86, 95):
            P(r, "del" if r % 2 else "sub", 2 if r == (87 if early else 93) else 25, 2 if r == (87 if early else 93) else 25)
        # across 9 -> 10 (rows 300..309 are in both, and the EARLIER chunk owns them: "9" sorts behind "10")
        for r in range(296, 315):
            P(r, "sub", 3 if r == (298 if early else 312) else 50, 0)
        counts = _counts_for(lab, fwd, rev)
        # a non-owned duplicate with another label that no read spells (chunk 7's copy of row 243; chunk 8 owns and spells the draft)
        k, j = 7, 243 - 7 * (L - O)
        assert lay.position[k, j] == lay.position[8, j - (L - O)] and j >= L - O
        lab[k, j], rq[k, j] = (lab[k, j] % 4) + 1, 0
        counts[k, j] = 0
        # and the other way round: the owner holds an edit without a read, the duplicate spells the draft
        lay.plant(lab, rq, 0, 245, "sub", 60)
        counts[lay.where(0, 245)] = 0
        lab[7, 245 - 7 * (L - O)] = lay.spelled()[0][7, 245 - 7 * (L - O)]
        depth = np.full(lab.shape, 60, np.uint16)
        for a in (lab, rq, counts, depth):
            a.setflags(write=False)
        out[variant] = (lab, rq, counts, depth)
    return lay, out


@pytest.mark.parametrize("variant", ["early", "late"])
def test_sparse_edits_and_runs_across_chunk_boundaries(hip_ctx, sparse, variant):
    lay, cases = sparse
    lab, rq, counts, depth = cases[variant]
    out, runs = _sweep(hip_ctx, lay, lab, rq, counts, depth, 7)
    assert sorted(len(r.records) for r in runs) == [1, 1, 1, 1, 2, 5, 5, 9, 9, 19]
    assert {rec[2] for r in runs for rec in r.records} == {er.SUB, er.DEL, er.INS}
    assert sorted(r.minimum for r in runs) == [0, 0, 3, 4, 5, 6, 7, 8, 9, 10]
    assert out[1][2] == 2 and {r.records[0][0] for r in out[1][4]} == {12, lay.rows[0][245][0]}   # the edits without a read go at 1
    # each run over a hand-off goes whole, at its own minimum + 1 and not before, whichever side held its weak column
    for (first, last), s in (((116, 124), 5), ((86, 94), 4), ((296, 314), 3)):
        want_s = ms.filter_low_support(lab, rq, counts, depth, *lay.args(), s, runs=runs)
        want = ms.filter_low_support(lab, rq, counts, depth, *lay.args(), s + 1, runs=runs)
        mine = [r for r in want[4] if r.records[0][0] == lay.rows[0][first][0]]
        assert len(mine) == 1 and len(mine[0].records) == last - first + 1 and len({k for k, _ in mine[0].rows}) == 2
        assert not [r for r in want_s[4] if r.records[0][0] == lay.rows[0][first][0]]
        for in_place in (False, True):
            got_s = _dev_filter(hip_ctx, lay, lab, rq, counts, depth, s, in_place=in_place)
            got = _dev_filter(hip_ctx, lay, lab, rq, counts, depth, s + 1, in_place=in_place)
            assert np.array_equal(got_s[0], want_s[0]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the run over the 9 -> 10 boundary: rows of both chunks are rewritten, chunk 9 owns the overlap
    changed = np.argwhere(ms.filter_low_support(lab, rq, counts, depth, *lay.args(), 4, runs=runs)[0] != lab)
    assert {int(j) for k, j in changed if k == 9} == set(range(296 - 270, 40))
    assert {int(j) for k, j in changed if k == 10} == set(range(10, 315 - 300))
    # the duplicates: chunk 7's copies are as they were, at every minimum
    for k in out:
        assert out[k][0][7, 243 - 210] == lab[7, 243 - 210] != lab[8, 243 - 240] and out[k][1][7, 243 - 210] == 0
        assert out[k][0][7, 245 - 210] == lab[7, 245 - 210] and out[k][1][7, 245 - 210] == 60
    assert out[1][0][8, 245 - 240] == lab[7, 245 - 210] != lab[8, 245 - 240]              # the owner's edit went
    # without a quality plane: the same labels
    _check(hip_ctx, lay, lab, None, counts, depth, 8, runs)


# ---- 2. the three kinds -------------------------------------------------------------------------------------------------------

def test_the_three_kinds_alone_and_in_one_run(hip_ctx):
    rng = np.random.default_rng(14)
    lay = mc.Layout([(0, mc.acgt(rng, 60), {10: 2, 30: 1})], L, O)
    lab, rq = lay.spelled(60)
    fwd, rev = np.full(lab.shape, 30, np.uint16), np.full(lab.shape, 20, np.uint16)

    def P(r, what, f, v):
        lay.plant(lab, rq, 0, r, what, 60)
        fwd[lay.where(0, r)], rev[lay.where(0, r)] = f, v
    P(_row(lay, 0, 3), "sub", 0, 0)                  # a base with zero reads: goes at 1
    P(_row(lay, 0, 6), "sub", 1, 2)                  # SUB alone: 3
    P(_row(lay, 0, 10, 2), 2, 4, 1)                  # INS alone, the second insert row of its position: 5
    P(_row(lay, 0, 20), "del", 0, 4)                 # DEL alone: 4
    P(_row(lay, 0, 30), "sub", 9, 0); P(_row(lay, 0, 30, 1), 3, 1, 1); P(_row(lay, 0, 31), "del", 5, 4)   # mixed: 9, 2, 9
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, 60, np.uint16)
    runs = ms.region_runs(lab, counts, depth, *lay.args())
    assert [([rec[2] for rec in r.records], r.supports) for r in runs] == [
        ([er.SUB], (0,)), ([er.SUB], (3,)), ([er.INS], (5,)), ([er.DEL], (4,)), ([er.SUB, er.INS, er.DEL], (9, 2, 9))]
    for k, reverted in ((0, 0), (1, 1), (2, 1), (3, 4), (4, 5), (5, 6), (6, 7), (TOP, 7)):
        assert _check(hip_ctx, lay, lab, rq, counts, depth, k, runs)[2] == reverted, k


# ---- 3. every column edited: a region is one run through all its chunks; regions -------------------------------------------

def test_a_region_that_is_one_run(hip_ctx):
    rng = np.random.default_rng(12)
    lay = mc.Layout([(0, mc.acgt(rng, 90), {10: 4, 50: 6})], L, O)
    assert lay.n == 3 and len(lay.rows[0]) == 100
    lab, rq = lay.all_edited(50)
    fwd, rev = np.full(lab.shape, 30, np.uint16), np.full(lab.shape, 20, np.uint16)
    fwd[lay.where(0, 45)], rev[lay.where(0, 45)] = 2, 3            # the minimum in the middle chunk (rows 40..59 are its own)
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, 60, np.uint16)
    out, runs = _sweep(hip_ctx, lay, lab, rq, counts, depth, 5)
    assert len(runs) == 1 and len(runs[0].records) == 100 and {k for k, _ in runs[0].rows} == {0, 1, 2}
    assert runs[0].rows[45] == (1, 15) and out[5][2] == 0 and out[6][2] == 100
    spelled = lay.spelled()[0]
    own = mq.owned_mask(*lay.args()[:5], lab.shape)
    assert np.array_equal(out[6][0][own], spelled[own]) and not out[6][1][own].any()


@pytest.mark.parametrize("weak_in", [0, 1])
def test_adjacent_regions_are_judged_apart(hip_ctx, weak_in):
    """region 0 ends at position 259 with a run on its last columns; region 1 = [59, 400] keeps 260.. and starts with a run on
    its first kept columns: in the VCF they are one block, here two runs, and only the one that holds the weak column goes.
    Region 1's copies of 258 and 259 lie in its dropped buffer: their unsupported edits belong to no run."""
    rng = np.random.default_rng(13)
    lay = mc.Layout([(0, mc.acgt(rng, 260), {}), (59, mc.acgt(rng, 342), {})], L, O)
    lab, rq = lay.spelled(60)
    fwd, rev = np.full(lab.shape, 30, np.uint16), np.full(lab.shape, 20, np.uint16)
    for g, ps, weak in ((0, (257, 258, 259), 259), (1, (260, 261), 260)):
        for p in ps:
            lay.plant(lab, rq, g, _row(lay, g, p), "sub", 60)
            if g == weak_in and p == weak:
                fwd[lay.where(g, _row(lay, g, p))], rev[lay.where(g, _row(lay, g, p))] = 1, 2
    for p in (258, 259):
        lay.plant(lab, rq, 1, _row(lay, 1, p), "del", 1)          # inside the buffer, adjacent to the kept edit at 260
        fwd[lay.where(1, _row(lay, 1, p))], rev[lay.where(1, _row(lay, 1, p))] = 0, 0
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, 60, np.uint16)
    out, runs = _sweep(hip_ctx, lay, lab, rq, counts, depth, 3)
    assert [(r.region, [rec[0] for rec in r.records]) for r in runs] == [(0, [257, 258, 259]), (1, [260, 261])]
    gone = out[4][4]
    assert [r.region for r in gone] == [weak_in] and out[4][2] == (3, 2)[weak_in] and out[3][2] == 0
    buffered = lay.where(1, _row(lay, 1, 259))
    assert (out[TOP][0][buffered] == 0).all() and (out[TOP][1][buffered] == 1).all()      # never touched


# ---- 4. pinned runs ------------------------------------------------------------------------------------------------------------

def test_pinned_runs_are_copied_and_counted(hip_ctx):
    d = bytearray(mc.acgt(np.random.default_rng(15), 100))
    d[10], d[40], d[70] = ord("N"), ord("n"), ord("R")
    lay = mc.Layout([(0, bytes(d), {40: 1})], L, O)
    lab, rq = lay.spelled(60)                                       # label 1 over N, n and R: three pinned substitutions
    fwd, rev = np.full(lab.shape, 0, np.uint16), np.full(lab.shape, 0, np.uint16)
    lay.plant(lab, rq, 0, _row(lay, 0, 11), "sub", 60)              # N + a substitution beside it
    lay.plant(lab, rq, 0, _row(lay, 0, 40, 1), 3, 60)               # n + its inserted base
    lay.plant(lab, rq, 0, _row(lay, 0, 55), "del", 60)              # and one run that is not pinned
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, 60, np.uint16)
    counts[lay.where(0, _row(lay, 0, 70))] = _counts_for(np.array([[1]], np.uint8), 3, 3)[0, 0]   # the R alone: support 6
    out, runs = _sweep(hip_ctx, lay, lab, rq, counts, depth, 6)
    assert [([rec[0] for rec in r.records], r.minimum, r.pinned) for r in runs] == [
        ([10, 11], 0, True), ([40, 40], 0, True), ([55], 0, False), ([70], 6, True)]
    assert out[1][2:4] == (1, 4) and out[6][2:4] == (1, 4) and out[7][2:4] == (1, 5)
    keep = np.ones(lab.shape, bool)
    keep[lay.where(0, _row(lay, 0, 55))] = False
    assert np.array_equal(out[TOP][0][keep], lab[keep]) and np.array_equal(out[TOP][1][keep], rq[keep])


# ---- 5. the clamp ------------------------------------------------------------------------------------------------------------

def test_counts_at_the_ceiling(hip_ctx):
    lay = mc.Layout([(0, mc.acgt(np.random.default_rng(16), 50), {})], L, O)
    lab, rq = lay.spelled(60)
    fwd, rev = np.full(lab.shape, 30, np.uint16), np.full(lab.shape, 20, np.uint16)
    for r, f, v in ((5, TOP, TOP), (15, TOP - 1, 0), (25, 0, TOP), (35, TOP - 1, 1)):
        lay.plant(lab, rq, 0, r, "sub", 60)
        fwd[lay.where(0, r)], rev[lay.where(0, r)] = f, v
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, TOP, np.uint16)
    runs = ms.region_runs(lab, counts, depth, *lay.args())
    assert [r.minimum for r in runs] == [2 * TOP, TOP - 1, TOP, TOP]                       # 131070 is not clamped again
    want = _check(hip_ctx, lay, lab, rq, counts, depth, TOP, runs)
    assert want[2] == 1 and [r.records[0][0] for r in want[4]] == [15]                     # 65534 + 0 goes, 131070 stays
    assert _check(hip_ctx, lay, lab, rq, counts, depth, TOP - 1, runs)[2] == 0


# ---- 6. random layouts: bytes that cannot be spelled, several regions, the real sizes ---------------------------------------

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
    # labels, qualities and counts are functions of (region, position, index), so that the copies of a row agree
    lab, _ = lay.spelled()
    is_edit = _keyed(lay, lambda n: rng.random(n) < p_edit)
    lab = np.where(is_edit & (lay.position >= 0), _keyed(lay, lambda n: rng.integers(0, 5, n)), lab).astype(np.uint8)
    rq = _keyed(lay, lambda n: rng.integers(1, 94, n)).astype(np.uint8)
    counts = np.stack([_keyed(lay, lambda n: rng.integers(0, 9, n)) for _ in range(10)], axis=-1).astype(np.uint16)
    counts[lay.position < 0] = 0
    depth = np.minimum(counts.sum(axis=-1) + _keyed(lay, lambda n: rng.integers(0, 5, n)), TOP).astype(np.uint16)
    return lay, lab, rq, counts, depth


@pytest.mark.parametrize("sizes", [(40, 10), (1000, 50)], ids=["40_10", "1000_50"])
def test_random_layouts(hip_ctx, sizes):
    LL, OO = sizes
    n, n_ins = (12_300, 20) if LL == 1000 else (370, 10)           # 13 chunks either way: chunk ids 9 and 10 meet
    lay, lab, rq, counts, depth = _random_case(21, [(0, n, n_ins), (500, 290 if LL == 40 else 1_100, 3), (900, 300, 5)], LL, OO, 0.5)
    assert 13 in [int((lay.region == g).sum()) for g in range(3)]
    runs = ms.region_runs(lab, counts, depth, *lay.args())
    lengths = [len(r.records) for r in runs]
    assert max(lengths) >= 5 and min(lengths) == 1 and any(r.pinned for r in runs) and len({r.region for r in runs}) == 3
    s = sorted(r.minimum for r in runs if not r.pinned)[len(runs) // 3]
    _sweep(hip_ctx, lay, lab, rq, counts, depth, s)


# ---- 7. a few thousand chunks ------------------------------------------------------------------------------------------------

def test_a_few_thousand_chunks(hip_ctx):
    """3667 chunks: every thread of the one-block pass holds several. Region 0 is one run through 1667 chunks with its weakest
    column far from either end; region 1 holds sparse runs; region 2 is all edits again and starts late."""
    rng = np.random.default_rng(31)
    lay = mc.Layout([(0, mc.acgt(rng, 50_000), {}), (0, mc.acgt(rng, 30_000), {7: 2}), (1_000, mc.acgt(rng, 30_000), {})], L, O)
    assert lay.n == 3667 > 3 * 1024 and int((lay.region == 0).sum()) == 1667
    lab, rq = lay.all_edited(60)
    spelled = lay.spelled()[0]
    g = np.broadcast_to(lay.region[:, None], lay.position.shape)
    at = np.clip(lay.position, 0, 31_000)
    lab = np.where((g == 1) & ~(rng.random(31_001) < 0.1)[at], spelled, lab)
    fwd = np.where(g == 1, rng.integers(0, 40, 31_001)[at], 30).astype(np.uint16)
    rev = np.where(g == 1, rng.integers(0, 40, 31_001)[at], 20).astype(np.uint16)
    fwd[lay.where(0, 20_000)], rev[lay.where(0, 20_000)] = 4, 5
    counts, depth = _counts_for(lab, fwd, rev), np.full(lab.shape, 90, np.uint16)
    out, runs = _sweep(hip_ctx, lay, lab, rq, counts, depth, 9)
    assert len(runs[0].records) == 50_000 and runs[0].minimum == 9 and len(runs[-1].records) == 30_000 - 201
    assert len({k for k, _ in runs[0].rows}) > 1_600
    assert out[10][2] >= 50_000 and out[9][2] < 50_000 and len(runs) > 1_000


# ---- 8. statuses -------------------------------------------------------------------------------------------------------------

def _untouched(res, labels, rq, in_place):
    out_lab, out_q, in_lab, in_q = res[:4]
    assert np.array_equal(in_lab, labels) and np.array_equal(in_q, rq)
    if not in_place:
        assert (out_lab == MARK).all() and (out_q == MARK).all()


@pytest.mark.parametrize("in_place", [False, True])
def test_invalid_calls_touch_nothing(hip_ctx, sparse, in_place):
    lay, cases = sparse
    lab, rq, counts, depth = cases["early"]
    for kw, k in ((dict(planes=(True, False)), 2), (dict(planes=(False, True)), 2), (dict(ref=False), 2), (dict(), TOP + 1), (dict(), -1),
                  (dict(overlap=21), 2), (dict(qual=(True, False)), 2), (dict(qual=(False, True)), 2)):
        res = _dev_filter(hip_ctx, lay, lab, rq, counts, depth, k, in_place=in_place, **kw)
        assert res[0] == _ffi.PV_ERR_INVALID and res[5] == [-7] * 4, (kw, k)                # refused by the call itself
        _untouched(res[1:], lab, rq, in_place)
    # a broken chunk layout
    ids = lay.chunk_id.copy()
    ids[[4, 5]] = ids[[5, 4]]
    res = _dev_filter(hip_ctx, lay, lab, rq, counts, depth, TOP, in_place=in_place, chunk_id=ids)
    assert res[4] == [0, _ffi.PV_ERR_INVALID, 4, 0]
    _untouched(res, lab, rq, in_place)
    # the draft one byte shorter than the region: its last position is owned and has no draft byte
    short = lay.ref_off.copy()
    short[-1] -= 1
    res = _dev_filter(hip_ctx, lay, lab, rq, counts, depth, TOP, in_place=in_place, ref_off=short)
    assert res[4] == [0, _ffi.PV_ERR_INVALID, 12, 0]
    _untouched(res, lab, rq, in_place)
    # an owned label 5: PV_ERR_STATE and nothing written; on a column that owns nothing it is not an error
    bad = lab.copy()
    bad[3, 7] = 5
    res = _dev_filter(hip_ctx, lay, bad, rq, counts, depth, TOP, in_place=in_place)
    assert res[4] == [0, _ffi.PV_ERR_STATE, 3, 0]
    _untouched(res, bad, rq, in_place)
    bad[5, 9] = 5                                                       # with a broken layout before it: the first bad chunk decides
    res = _dev_filter(hip_ctx, lay, bad, rq, counts, depth, TOP, in_place=in_place,
                      chunk_id=np.array([0, 2, 1] + list(range(3, 13)), np.int32))
    assert res[4] == [0, _ffi.PV_ERR_INVALID, 1, 0]
    loser = lab.copy()
    loser[7, 35] = 5                                                    # chunk 7's copy of row 245, which chunk 8 owns
    res = _dev_filter(hip_ctx, lay, loser, rq, counts, depth, TOP, in_place=in_place)
    want = ms.filter_low_support(lab, rq, counts, depth, *lay.args(), TOP)
    want[0][7, 35] = 5
    assert res[4][1] == 0 and np.array_equal(res[0], want[0]) and np.array_equal(res[1], want[1])


def test_invalid_calls_of_the_host_form(hip_ctx, sparse):
    lay, cases = sparse
    lab, rq, counts, depth = cases["late"]
    out = _host_out(lay, counts, depth)
    no_ref = types.SimpleNamespace(ref_start=lay.ref_start, ref_off=lay.ref_off, ref=None)
    bad = lab.copy()
    bad[3, 7] = 5
    swapped = _host_out(lay, counts, depth, np.array([0, 2, 1] + list(range(3, 13)), np.int32))
    for chunks, batch, labels, k, o, code in ((out, no_ref, lab, 2, O, _ffi.PV_ERR_INVALID), (out, lay.batch, lab, TOP + 1, O, _ffi.PV_ERR_INVALID),
                                              (out, lay.batch, lab, 2, 21, _ffi.PV_ERR_INVALID),
                                              (_host_out(lay, None, depth), lay.batch, lab, 2, O, _ffi.PV_ERR_INVALID),
                                              (_host_out(lay, counts, None), lay.batch, lab, 2, O, _ffi.PV_ERR_INVALID),
                                              (swapped, lay.batch, lab, 2, O, _ffi.PV_ERR_INVALID),
                                              (out, lay.batch, bad, 2, O, _ffi.PV_ERR_STATE)):
        lab2, q2 = labels.copy(), rq.copy()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_filter_low_support(chunks, lab2, batch, k, q2, L, o, in_place=True)
        assert e.value.code == code
        assert np.array_equal(lab2, labels) and np.array_equal(q2, rq)


def test_no_chunks(hip_ctx, sparse):
    lay = sparse[0]
    none = types.SimpleNamespace(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32), region=np.zeros(0, np.int32),
                                 chunk_id=np.zeros(0, np.int32), depth=np.zeros((0, L), np.uint16), counts=np.zeros((0, L, 10), np.uint16))
    cnt = (C.c_int64 * 4)()
    lab, q = hip_ctx.polish_filter_low_support(none, np.zeros((0, L), np.uint8), lay.batch, 2, np.zeros((0, L), np.uint8), L, O, counts=cnt)
    assert list(cnt) == [0, 0, -1, 0] and lab.shape == (0, L) and q.shape == (0, L)


# ---- 9. the two run filters commute ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(40, 10)], ids=["40_10"])
def test_the_filter_commutes_with_the_quality_filter(hip_ctx, sizes):
    LL, OO = sizes
    lay, lab, rq, counts, depth = _random_case(23, [(0, 370, 10), (500, 290, 3)], LL, OO, 0.4)
    Q, K = 30, 6
    out = _host_out(lay, counts, depth)
    q_runs, s_runs = mq.region_runs(lab, rq, *lay.args()), ms.region_runs(lab, counts, depth, *lay.args())
    assert [r.rows for r in q_runs] == [r.rows for r in s_runs]                            # "run" has one definition
    union = [s for q, s in zip(q_runs, s_runs) if not s.pinned and (q.minimum < Q or s.minimum < K)]
    only_q = sum(q.minimum < Q and s.minimum >= K for q, s in zip(q_runs, s_runs) if not s.pinned)
    only_s = sum(q.minimum >= Q and s.minimum < K for q, s in zip(q_runs, s_runs) if not s.pinned)
    assert only_q > 3 and only_s > 3 and len(union) > only_q + only_s
    want_lab, want_q = lab.copy(), rq.copy()
    spelled = lay.spelled()[0]
    for r in union:
        for (k, j), rec in zip(r.rows, r.records):
            want_lab[k, j], want_q[k, j] = (spelled[k, j] if rec[1] == 0 else 0), 0
    n_union = sum(len(r.records) for r in union)
    pin_q = sum(len(q.records) for q in q_runs if q.pinned and q.minimum < Q)
    pin_s = sum(len(s.records) for s in s_runs if s.pinned and s.minimum < K)
    cq, cs = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    a_lab, a_q = hip_ctx.polish_filter_low_qual(lay.out, lab, lay.batch, Q, rq, LL, OO, counts=cq)
    a_lab, a_q = hip_ctx.polish_filter_low_support(out, a_lab, lay.batch, K, a_q, LL, OO, counts=cs)
    assert np.array_equal(a_lab, want_lab) and np.array_equal(a_q, want_q)
    assert cq[0] + cs[0] == n_union and (cq[3], cs[3]) == (pin_q, pin_s) and cq[0] == mq.filter_low_qual(lab, rq, *lay.args(), Q)[2]
    b_lab, b_q = hip_ctx.polish_filter_low_support(out, lab, lay.batch, K, rq, LL, OO, counts=cs)
    b_lab, b_q = hip_ctx.polish_filter_low_qual(lay.out, b_lab, lay.batch, Q, b_q, LL, OO, counts=cq)
    assert np.array_equal(b_lab, want_lab) and np.array_equal(b_q, want_q)
    assert cq[0] + cs[0] == n_union and (cq[3], cs[3]) == (pin_q, pin_s)
    assert cs[0] == ms.filter_low_support(lab, rq, counts, depth, *lay.args(), K)[2]
    # and the checkers, one behind the other, say the same
    c_lab, c_q = mq.filter_low_qual(lab, rq, *lay.args(), Q)[:2]
    c_lab, c_q = ms.filter_low_support(c_lab, c_q, counts, depth, *lay.args(), K)[:2]
    assert np.array_equal(c_lab, want_lab) and np.array_equal(c_q, want_q)


# ---- 10. the identity with the edits, their evidence and the stitch -----------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, TOP])
def test_identity_with_edits_evidence_and_stitch(hip_ctx, sparse, k):
    """edits(labels_out) = edits(labels) minus the records of the reverted runs; every composed record's weakest column has
    alt_fwd + alt_rev >= k; stitch(labels_out) = those records applied to the draft"""
    lay, cases = sparse
    lab, rq, counts, depth = cases["late"]
    out = _host_out(lay, counts, depth)
    want_lab, want_q, reverted, pinned, gone = ms.filter_low_support(lab, rq, counts, depth, *lay.args(), k)
    assert 0 < len(gone)
    lab_out, q_out = hip_ctx.polish_filter_low_support(out, lab, lay.batch, k, rq, L, O)
    eoff, before, ev_before = hip_ctx.polish_edits_evidence(out, lab, lay.batch, row_qual=rq, seq_length=L, seq_overlap=O)
    eoff2, after, ev_after = hip_ctx.polish_edits_evidence(out, lab_out, lay.batch, row_qual=q_out, seq_length=L, seq_overlap=O)
    dropped = {(rec[0], rec[1]) for r in gone for rec in r.records}
    keep = np.array([(int(p), int(x)) not in dropped for p, x in zip(before["position"], before["index"])], bool)
    assert len(dropped) == reverted == int((~keep).sum())
    assert np.array_equal(after, before[keep]) and np.array_equal(ev_after, ev_before[keep])
    assert (ev_after["alt_fwd"].astype(int) + ev_after["alt_rev"] >= k).all()
    roff, seq, qual = hip_ctx.polish_stitch_qual(lay.out, lab_out, q_out, lay.ref_start, seq_length=L, seq_overlap=O)
    draft = lay.ref.tobytes()
    records = pe.compose_records("c", after, draft, True, evidence=ev_after)
    assert er.apply([tuple(r)[:4] for r in records], draft) == seq.decode()
    assert all(r.evidence[2] + r.evidence[3] >= k for r in records) and (len(records) > 0) == (k < TOP)
    if k == TOP:
        assert seq.decode() == draft.decode().upper()


# ---- 11. one linear graph -------------------------------------------------------------------------------------------------------

def test_graph_of_row_qual_mask_both_filters_stitch_qual_and_evidence(hip_ctx):
    """row qualities, minimum-depth mask, minimum-quality filter, minimum-support filter (all in place), stitch with qualities
    and edits with evidence captured as one graph on one stream; replays on refilled labels and softmax sums equal the eager
    calls, and those the checkers"""
    lay, _, _, counts, _ = _random_case(41, [(0, 380, 20), (500, 300, 5)], L, O, 0.3)
    n, G = lay.n, lay.n_regions
    rng = np.random.default_rng(42)
    depth = _keyed(lay, lambda m: rng.integers(0, 6, m)).astype(np.uint16)
    do = _device_chunks(lay, counts, depth)
    rs, ro, ref = (torch.from_numpy(np.array(a)).cuda() for a in (lay.ref_start, lay.ref_off, lay.ref))
    fills = []
    for s in range(3):
        r = np.random.default_rng(70 + s)
        lab = _keyed(lay, lambda m: r.integers(0, 5, m)).astype(np.uint8)
        lab = np.where(_keyed(lay, lambda m: r.random(m)) < 0.6, lay.spelled()[0], lab).astype(np.uint8)
        # the winning softmax sum 2 * (1 - 10^-5u), u uniform: qualities spread over 0..50
        acc = (1.0 - 10.0 ** (-5.0 * _keyed(lay, lambda m: r.random(m))))[..., None].astype(np.float32) * np.ones(5, np.float32) * 2.0
        acc[:, :O] /= 2
        acc[:, L - O:] /= 2
        fills.append((lab, acc))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq, qual = (torch.zeros(n * L, dtype=torch.uint8, device="cuda") for _ in range(2))
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    evb = torch.zeros((n * L, 8), dtype=torch.uint8, device="cuda")
    roff, eoff = (torch.zeros(G + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    c_rq, c_mk, c_fl, c_su, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(6))
    st = hip_ctx.stream
    MD, MQ, MS = 2, 12, 8     # (on these fills each pass takes back more than 20 rows and some 50 records stay)
    common = (rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G)

    def passes():
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_rq.data_ptr(), L, O, stream=st)
        hip_ctx.polish_mask_low_depth_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, MD, lab_d.data_ptr(), rq_d.data_ptr(),
                                          c_mk.data_ptr(), stream=st)
        hip_ctx.polish_filter_low_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, MQ, lab_d.data_ptr(), rq_d.data_ptr(),
                                           c_fl.data_ptr(), stream=st)
        hip_ctx.polish_filter_low_support_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, MS, lab_d.data_ptr(), rq_d.data_ptr(),
                                              c_su.data_ptr(), stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), G, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_evidence_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, eoff.data_ptr(), buf.data_ptr(),
                                          evb.data_ptr(), n * L, c_ed.data_ptr(), stream=st)

    def state():
        t, e = int(c_st[0].item()), int(c_ed[0].item())
        return (lab_d.cpu().numpy().tobytes(), rq_d.cpu().numpy().tobytes(), seq[:t].cpu().numpy().tobytes(),
                qual[:t].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(), evb[:e].cpu().numpy().tobytes(),
                roff.cpu().numpy().tolist(), eoff.cpu().numpy().tolist(), c_mk.cpu().numpy().tolist(), c_fl.cpu().numpy().tolist(),
                c_su.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(), c_ed.cpu().numpy().tolist())

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
        f_lab, f_q, reverted, pinned, _ = mq.filter_low_qual(m_lab, m_q, *lay.args(), MQ)
        want_lab, want_q, unsupported, pinned_s, _ = ms.filter_low_support(f_lab, f_q, counts, depth, *lay.args(), MS)
        assert eager[-1][0] == want_lab.tobytes() and eager[-1][1] == want_q.tobytes()
        assert eager[-1][8] == [masked, 0, -1, unmaskable] and eager[-1][9] == [reverted, 0, -1, pinned]
        assert eager[-1][10] == [unsupported, 0, -1, pinned_s] and unsupported > 20 and reverted > 20 and masked > 20
        h_roff, h_seq, h_qual = hip_ctx.polish_stitch_qual(lay.out, want_lab, want_q, lay.ref_start, seq_length=L, seq_overlap=O)
        assert (eager[-1][2], eager[-1][3], eager[-1][6]) == (h_seq, h_qual, h_roff.tolist())
        h_eoff, h_ed, h_ev = hip_ctx.polish_edits_evidence(_host_out(lay, counts, depth), want_lab, lay.batch, row_qual=want_q, seq_length=L,
                                                      seq_overlap=O)
        assert (eager[-1][4], eager[-1][5]) == (h_ed.tobytes(), h_ev.tobytes()) and len(h_ed) > 20
        assert (h_ev["alt_fwd"].astype(int) + h_ev["alt_rev"])[~_pinned_records(h_eoff, h_ed)].min() >= MS
    assert eager[0][2] != eager[1][2]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        lab_d.copy_(torch.from_numpy(fills[k][0])); acc_d.copy_(torch.from_numpy(fills[k][1]))
        for t in (rq_d, seq, qual, buf, evb, roff, eoff, c_mk, c_fl, c_su, c_st, c_ed):
            t.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


def _pinned_records(edit_off, edits):
    """bool per edit record: it belongs to a pinned run (runs cut per region, as the filter cuts them)"""
    out = np.zeros(len(edits), bool)
    recs = [tuple(int(v) for v in e) for e in edits.tolist()]
    for a, b in zip(edit_off[:-1].tolist(), edit_off[1:].tolist()):
        at = a
        for run in mq.runs_of(recs[a:b]):
            out[at:at + len(run)] = any(r[1] == 0 and er.upper(r[3]) not in er.BASES for r in run)
            at += len(run)
    return out


# ---- 12. the command ------------------------------------------------------------------------------------------------------------

READ_NOISE, MODEL_SEED, MODEL_GAIN = 0.3, 37, 100.0


def _write_inputs(tmp, noise=READ_NOISE, seed=MODEL_SEED, gain=MODEL_GAIN):
    """two contigs of a few kb with an ACGT / acgt draft (nothing pinned), 60 reads of some 900 bases each, and seeded P2
    weights, as the minimum-quality test has them. Unlike there, a read is a copy of the draft under it in which every base is
    another one with probability `noise`: reads of random bases keep their place only until --realign, which clips them to
    the few bases that happen to match, so that behind --realign --min_depth 3 no column is left where two reads spell
    anything but the draft, whatever the weights. With these reads a column under 17 reads shows each other base once or
    twice, so at --min_support 2 some runs go and some stay, with and without the other flags. -> {contig: draft}"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    rng = np.random.default_rng(43)
    contigs = [("ctgA", "".join(rng.choice(list("ACGTacgt"), size=3_200))), ("ctgB", "".join(rng.choice(list("ACGTacgt"), size=2_100)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        for i in range(60):
            pos = int(rng.integers(0, len(seq) - 200))
            n = min(len(seq) - pos, int(max(60, rng.normal(900, 270))))
            b = np.array(["ACGT".index(c) for c in seq[pos:pos + n].upper()])
            b = np.where(rng.random(n) < noise, (b + rng.integers(1, 4, n)) % 4, b)
            recs.append(dict(tid=tid, pos=pos, mapq=60, flag=int(rng.choice([0, 16])), cigar=[(0, n)], seq="".join("ACGT"[v] for v in b),
                             qual=[30] * n, name="read%d_%d" % (tid, i), hp=None))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(seed, gain))
    return dict(contigs)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("min_support")
    return tmp, _write_inputs(tmp)


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what the support filter of every launch was given and what it left"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        ctx, real, seen = self.ctx, self.ctx.polish_filter_low_support_dev, {}

        def spy(dout, n_chunks, *a, **k):
            ctx.synchronize()
            seen.update(labels_in=self.labels[:n_chunks].cpu().numpy(),
                        row_qual_in=None if self.row_qual is None or not self.qualities else self.row_qual[:n_chunks].cpu().numpy())
            return real(dout, n_chunks, *a, **k)
        ctx.polish_filter_low_support_dev = spy
        try:
            res = super()._labels_and_stitch(db, n, n_regions)
        finally:
            del ctx.polish_filter_low_support_dev
        if n:
            d = self.dout
            seen.update(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(), region=d.region[:n].cpu().numpy(),
                        chunk_id=d.chunk_id[:n].cpu().numpy(), labels=self.labels[:n].cpu().numpy(),
                        row_qual=self.row_qual[:n].cpu().numpy() if self.qualities else None,
                        depth=d.depth_numpy(n), counts=d.row_counts_numpy(n),
                        ref_start=db.t["ref_start"][:n_regions].cpu().numpy(), ref_off=db.t["ref_off"][:n_regions + 1].cpu().numpy(),
                        ref=db.t["ref"].cpu().numpy(), supported=res.supported)
            self.launches.append(seen)
        return res


def _polish(t, hip_ctx, name, flags, chains=None, bam="reads.bam"):
    out_dir = str(t / name)
    argv = ["-b", str(t / bam), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8", "-o", out_dir] + flags

    def open_chain(device, shared, state_dict, dtype, **k):
        hip_ctx.load_p2(state_dict, dtype)
        chain = (polish._DeviceChain if chains is None else _RecordingChain)(hip_ctx, **k)
        if chains is not None:
            chains.append(chain)
        return chain
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(out_dir)):
        if not f.endswith(".tbi"):
            out[f] = bamio.bgzf_read_all(os.path.join(out_dir, f)) if f.endswith(".vcf.gz") else open(os.path.join(out_dir, f), "rb").read()
    return out


def _fasta(data: bytes):
    lines = data.decode().split("\n")
    return dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))


def test_min_support_65535_gives_the_draft(inputs, hip_ctx, opts):
    """weight-independent: no column has 65535 reads and the drafts hold no byte that cannot be spelled, so every edit goes.
    The chain needs none of --qualities and --evidence."""
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    got = _polish(t, hip_ctx, "all", ["--min_support", "65535", "--edits"], chains)
    assert chains[0].min_support == TOP and not chains[0].qualities and not chains[0].evidence and len(chains[0].launches) > 1
    for la in chains[0].launches:
        assert la["supported"][0] > 100 and la["supported"][1] == 0 and (la["labels"] != la["labels_in"]).any()
    assert list(got) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.fa"]
    assert _fasta(got["_pepper_polished.fa"]) == {c: d.upper() for c, d in drafts.items()}
    header, cols, recs = er.parse_vcf(got["_pepper_polished.edits.vcf.gz"].decode())
    assert recs == [] and header[3:] == ["contig=<ID=ctgA,length=3200>", "contig=<ID=ctgB,length=2100>", "pepper_min_support=65535"]


@pytest.mark.parametrize("flags", [[], ["--realign", "--gpu_decode", "--min_depth", "3", "--min_qual", "20"]], ids=["plain", "all_flags"])
def test_min_support_2_end_to_end(inputs, hip_ctx, opts, flags):
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    got = _polish(t, hip_ctx, "two_" + ("flags" if flags else "plain"), ["--min_support", "2", "--edits", "--evidence", "--qualities"] + flags,
                  chains)
    launches = chains[0].launches
    assert len(launches) > 1
    reverted = 0
    for la in launches:
        want_lab, want_q, n_rev, n_pin, gone = ms.filter_low_support(
            la["labels_in"], la["row_qual_in"], la["counts"], la["depth"], la["position"], la["index"], la["region"], la["chunk_id"],
            la["ref_start"], la["ref_off"], la["ref"], 2)
        assert np.array_equal(la["labels"], want_lab) and np.array_equal(la["row_qual"], want_q) and la["supported"] == (n_rev, n_pin)
        reverted += n_rev
    print("min_support 2 (%s): %d rows reverted in %d launches" % (flags, reverted, len(launches)))
    assert reverted > 0 and sum(int((la["labels"] != la["labels_in"]).sum()) for la in launches) == reverted
    fasta = _fasta(got["_pepper_polished.fa"])
    fq = got["_pepper_polished.fq"].decode().split("\n")
    assert fq[0::4][:2] == ["@ctgA", "@ctgB"] and fq[1::4] == [fasta["ctgA"], fasta["ctgB"]]
    text = got["_pepper_polished.edits.vcf.gz"].decode()
    header = [l[2:] for l in text.split("\n") if l.startswith("##")]
    info = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    recs = [(f[0], int(f[1]), f[3], f[4], int(f[5])) for f in info]
    assert [h for h in header if h.startswith("pepper_")] == (["pepper_min_depth=3", "pepper_min_qual=20"] if flags else []) + \
        ["pepper_min_support=2"]
    assert len(recs) > 0 and all(f[2] == "." and f[6] == "PASS" for f in info)
    ad = [int(f[7].split(";")[1].split(",")[1]) for f in info]
    print("  %d VCF records, AD alt from %d to %d" % (len(ad), min(ad), max(ad)))
    assert all(f[7].split(";")[1].startswith("AD=") for f in info) and min(ad) >= 2       # some edits survive, none below 2
    for c in drafts:
        mine = [r[1:] for r in recs if r[0] == c]
        assert er.apply(mine, drafts[c].encode()) == fasta[c] and mine, c                  # the records applied to the draft


def test_min_support_0_changes_no_byte(inputs, hip_ctx, opts):
    t, _ = inputs
    opts(shared_device=1)
    a = _polish(t, hip_ctx, "plain", ["--edits", "--qualities", "--evidence"])
    b = _polish(t, hip_ctx, "zero", ["--edits", "--qualities", "--evidence", "--min_support", "0"])
    assert len(a) == 3 and list(a) == list(b)
    for f in a:
        assert a[f] == b[f], f


def test_each_haplotype_filters_with_its_own_counts(hp_inputs, hip_ctx, opts):
    """-hp --min_support 1: haplotype h's files are those of a plain run with the flag on the file that holds only its reads"""
    t = hp_inputs
    opts(shared_device=1)
    flags = ["--min_support", "1", "--edits", "--evidence"]
    got = _polish(t, hip_ctx, "hp", ["-hp"] + flags, bam="tagged.bam")
    loose = _polish(t, hip_ctx, "hp_loose", ["-hp", "--edits", "--evidence"], bam="tagged.bam")
    assert list(got) == ["_pepper_polished_hp%d%s" % (h, x) for h in (1, 2) for x in (".edits.vcf.gz", ".fa")]
    for h in (1, 2):
        want = _polish(t, hip_ctx, "split%d" % h, flags, bam="split%d.bam" % h)
        assert got["_pepper_polished_hp%d.fa" % h] == want["_pepper_polished.fa"], h
        mine = got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode().split("\n")
        assert mine.count("##pepper_haplotype=%d" % h) == 1 and mine.count("##pepper_min_support=1") == 1
        mine.remove("##pepper_haplotype=%d" % h)
        theirs = want["_pepper_polished.edits.vcf.gz"].decode().split("\n")
        assert mine == theirs and sum(bool(l) and not l.startswith("#") for l in theirs) >= 5, h
        assert got["_pepper_polished_hp%d.fa" % h] != loose["_pepper_polished_hp%d.fa" % h], h   # the filter took something back
    assert got["_pepper_polished_hp1.fa"] != got["_pepper_polished_hp2.fa"]
