"""GPU: the polisher's chunk passes at every chunk geometry they accept: pv_polish_row_qual, pv_polish_mask_low_depth,
pv_polish_filter_low_qual, pv_polish_stitch, pv_polish_stitch_qual and pv_polish_edits, host form and _dev form, against the
host checkers on the cases of tests/chunk_geometry_cases.py (every columns-per-thread count from 1 to 16 that the table holds,
ragged and idle threads, no overlap and an overlap of half a chunk), then the chain the polisher runs (mask, filter, stitch
with qualities and edits: the edits applied to the draft spell the stitch), the chunk-id decade steps 9/10, 99/100 and 999/1000,
chunk counts around the 1024 threads of the one-block folds, and the sizes just outside the accepted range, which are refused
and touch nothing. Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import chunk_geometry_cases as cg
import edits_ref as er
import min_qual_cases as mc
import qual_ref as qr
from pepper_thesis_amd import _ffi, polish_edits as pe
from pepper_thesis_amd.device import DevicePolishOut
from pepper_thesis_amd.polish_edits import EDIT_DTYPE

pytestmark = pytest.mark.gpu
GEO = pytest.mark.parametrize("geo", cg.GEOMETRIES, ids=cg.geo_id)
MARK, QMARK = 0xEE, 0xDD


def _up(a):
    return torch.from_numpy(np.array(a)).cuda()


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


class _Dev:
    """a case's chunk arrays and draft on the device, and the _dev forms on tensors; seq_length / seq_overlap: what the calls
    are told, where that is not the layout's own. Every method returns the error code of the call (None: accepted) in front."""

    def __init__(self, ctx, case, seq_length=None, seq_overlap=None):
        lay = case.lay
        self.ctx, self.n, self.G, self.width = ctx, lay.n, lay.n_regions, lay.L
        self.do = DevicePolishOut(max(lay.n, 1), lay.L, lay.O, depth=case.depth is not None)
        for name in ("position", "index", "region", "chunk_id"):
            getattr(self.do, name)[:lay.n].copy_(torch.from_numpy(np.array(getattr(lay, name))))
        if case.depth is not None:
            self.do.set_depth(np.array(case.depth))
        if seq_length is not None:
            self.do.seq_length = seq_length
        if seq_overlap is not None:
            self.do.seq_overlap = seq_overlap
        self.rs, self.ro, self.ref = _up(lay.ref_start), _up(lay.ref_off), _up(lay.ref)
        self.cap = lay.n * lay.L

    def _call(self, fn, *args):
        counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        code = None
        try:
            fn(*args, counts.data_ptr())
        except _ffi.PepperHipError as e:
            code = e.code
        self.ctx.synchronize()
        return code, counts.cpu().numpy().tolist()

    def stitch(self, lab, rq=None):
        """lab, rq: device tensors -> (code, region_off, seq, qual, counts); the outputs pre-filled"""
        seq = torch.full((max(self.cap, 1),), MARK, dtype=torch.uint8, device="cuda")
        qual = torch.full((max(self.cap, 1),), QMARK, dtype=torch.uint8, device="cuda")
        roff = torch.full((self.G + 1,), -7, dtype=torch.int64, device="cuda")
        if rq is None:
            code, c = self._call(self.ctx.polish_stitch_dev, self.do, self.n, lab.data_ptr(), self.rs.data_ptr(), self.G, roff.data_ptr(),
                                 seq.data_ptr(), self.cap)
        else:
            code, c = self._call(self.ctx.polish_stitch_qual_dev, self.do, self.n, lab.data_ptr(), rq.data_ptr(), self.rs.data_ptr(), self.G,
                                 roff.data_ptr(), seq.data_ptr(), qual.data_ptr(), self.cap)
        return code, roff.cpu().numpy(), seq.cpu().numpy(), qual.cpu().numpy(), c

    def edits(self, lab, rq=None):
        """-> (code, region_edit_off, records of the whole buffer, its raw bytes, counts)"""
        buf = torch.full((max(self.cap, 1), 16), MARK, dtype=torch.uint8, device="cuda")
        eoff = torch.full((self.G + 1,), -7, dtype=torch.int64, device="cuda")
        code, c = self._call(self.ctx.polish_edits_dev, self.do, self.n, lab.data_ptr(), rq.data_ptr() if rq is not None else 0,
                             self.rs.data_ptr(), self.ro.data_ptr(), self.ref.data_ptr(), self.G, eoff.data_ptr(), buf.data_ptr(), self.cap)
        raw = buf.cpu().numpy()
        return code, eoff.cpu().numpy(), raw.view(EDIT_DTYPE).reshape(-1), raw, c

    def mask(self, lab, rq, min_depth, lab_out, rq_out):
        return self._call(self.ctx.polish_mask_low_depth_dev, self.do, self.n, lab.data_ptr(), rq.data_ptr() if rq is not None else 0,
                          self.rs.data_ptr(), self.ro.data_ptr(), self.ref.data_ptr(), self.G, min_depth, lab_out.data_ptr(),
                          rq_out.data_ptr() if rq_out is not None else 0)

    def filter(self, lab, rq, min_qual, lab_out, rq_out):
        return self._call(self.ctx.polish_filter_low_qual_dev, self.do, self.n, lab.data_ptr(), rq.data_ptr(), self.rs.data_ptr(),
                          self.ro.data_ptr(), self.ref.data_ptr(), self.G, min_qual, lab_out.data_ptr(), rq_out.data_ptr())

    def rewrite(self, which, labels, rq, threshold, in_place):
        """mask or filter on uploaded copies; out of place the outputs are pre-filled -> (code, labels out, row qualities out
        or None, labels in and row qualities in as they are afterwards, counts)"""
        lab, drq = _up(labels), None if rq is None else _up(rq)
        lab_out = lab if in_place else torch.full_like(lab, MARK)
        rq_out = None if rq is None else (drq if in_place else torch.full_like(drq, MARK))
        code, c = getattr(self, which)(lab, drq, threshold, lab_out, rq_out)
        host = lambda t: None if t is None else t.cpu().numpy()
        return code, host(lab_out), host(rq_out), host(lab), host(drq), c


# ---- the six passes against their checkers, on any case ------------------------------------------------------------------------

def _check_stitch(ctx, case, dev):
    lay = case.lay
    seqs, quals = case.stitch_seq, [q for _, q in case.stitch_qual]
    assert [s for s, _ in case.stitch_qual] == seqs
    off = _offsets(seqs)
    total = int(off[-1])
    kw = dict(seq_length=lay.L, seq_overlap=lay.O)
    counts = (C.c_int64 * 4)()
    roff, seq = ctx.polish_stitch(lay.out, case.labels, lay.ref_start, counts=counts, **kw)
    assert list(counts) == [total, 0, -1, 0] and np.array_equal(roff, off)
    assert [seq[off[g]:off[g + 1]] for g in range(lay.n_regions)] == seqs
    counts = (C.c_int64 * 4)()
    roff, seq2, qual = ctx.polish_stitch_qual(lay.out, case.labels, case.rq, lay.ref_start, counts=counts, **kw)
    assert list(counts) == [total, 0, -1, 0] and np.array_equal(roff, off) and seq2 == seq
    assert [qual[off[g]:off[g + 1]] for g in range(lay.n_regions)] == quals
    lab, drq = _up(case.labels), _up(case.rq)
    for with_qual in (False, True):
        code, droff, dseq, dqual, c = dev.stitch(lab, drq if with_qual else None)
        assert code is None and c == [total, 0, -1, 0] and np.array_equal(droff, off), with_qual
        assert dseq[:total].tobytes() == seq and (dseq[total:] == MARK).all(), with_qual
        if with_qual:
            assert dqual[:total].tobytes() == qual and (dqual[total:] == QMARK).all()
        else:
            assert (dqual == QMARK).all()
    return total


def _check_edits(ctx, case, dev, with_qual):
    lay = case.lay
    q = case.rq if with_qual else None
    want, want_off = case.edits(with_qual)
    total = len(want)
    counts = (C.c_int64 * 4)()
    eoff, recs = ctx.polish_edits(lay.out, case.labels, lay.batch, row_qual=q, seq_length=lay.L, seq_overlap=lay.O, counts=counts)
    assert list(counts) == [total, 0, -1, 0] and np.array_equal(eoff, want_off) and recs.tolist() == want
    code, deoff, drecs, raw, c = dev.edits(_up(case.labels), None if q is None else _up(q))
    assert code is None and c == [total, 0, -1, 0] and np.array_equal(deoff, want_off)
    assert drecs[:total].tolist() == want and (raw[total:] == MARK).all()
    return total


def _check_mask(ctx, case, dev, with_qual):
    lay = case.lay
    q = case.rq if with_qual else None
    want_lab, want_q, masked, unmaskable = case.masked
    md = case.min_depth
    counts = (C.c_int64 * 4)()
    got_lab, got_q = ctx.polish_mask_low_depth(case.chunks, case.labels, lay.batch, md, row_qual=q, seq_length=lay.L, counts=counts)
    assert list(counts) == [masked, 0, -1, unmaskable]
    assert np.array_equal(got_lab, want_lab) and (got_q is None if q is None else np.array_equal(got_q, want_q))
    lab2, q2 = case.labels.copy(), None if q is None else q.copy()                              # in place on the host
    r_lab, r_q = ctx.polish_mask_low_depth(case.chunks, lab2, lay.batch, md, row_qual=q2, seq_length=lay.L, in_place=True)
    assert r_lab is lab2 and r_q is q2 and np.array_equal(lab2, want_lab) and (q is None or np.array_equal(q2, want_q))
    for in_place in (False, True):
        code, out_lab, out_q, in_lab, in_q, c = dev.rewrite("mask", case.labels, q, md, in_place)
        assert code is None and c == [masked, 0, -1, unmaskable], in_place
        assert np.array_equal(out_lab, want_lab) and (q is None or np.array_equal(out_q, want_q)), in_place
        if not in_place:                                                                        # the inputs are read only
            assert np.array_equal(in_lab, case.labels) and (q is None or np.array_equal(in_q, q))
    return masked


def _check_filter(ctx, case, dev):
    lay = case.lay
    want_lab, want_q, reverted, pinned, _ = case.filtered
    counts = (C.c_int64 * 4)()
    got_lab, got_q = ctx.polish_filter_low_qual(lay.out, case.labels, lay.batch, cg.MIN_QUAL, case.rq, lay.L, lay.O, counts=counts)
    assert list(counts) == [reverted, 0, -1, pinned]
    assert np.array_equal(got_lab, want_lab) and np.array_equal(got_q, want_q)
    lab2, q2 = case.labels.copy(), case.rq.copy()                                               # in place on the host
    r_lab, r_q = ctx.polish_filter_low_qual(lay.out, lab2, lay.batch, cg.MIN_QUAL, q2, lay.L, lay.O, in_place=True)
    assert r_lab is lab2 and r_q is q2 and np.array_equal(lab2, want_lab) and np.array_equal(q2, want_q)
    for in_place in (False, True):
        code, out_lab, out_q, in_lab, in_q, c = dev.rewrite("filter", case.labels, case.rq, cg.MIN_QUAL, in_place)
        assert code is None and c == [reverted, 0, -1, pinned], in_place
        assert np.array_equal(out_lab, want_lab) and np.array_equal(out_q, want_q), in_place
        if not in_place:
            assert np.array_equal(in_lab, case.labels) and np.array_equal(in_q, case.rq)
    return reverted


# ---- 3. every pass, every geometry -----------------------------------------------------------------------------------------------

@GEO
def test_stitch_and_stitch_qual(hip_ctx, geo):
    case = cg.geometry_case(*geo)
    assert _check_stitch(hip_ctx, case, _Dev(hip_ctx, case)) > 400


@GEO
@pytest.mark.parametrize("with_qual", [False, True], ids=["plain", "qual"])
def test_edits(hip_ctx, geo, with_qual):
    case = cg.geometry_case(*geo)
    assert _check_edits(hip_ctx, case, _Dev(hip_ctx, case), with_qual) > 500


@GEO
@pytest.mark.parametrize("with_qual", [False, True], ids=["plain", "qual"])
def test_mask_low_depth(hip_ctx, geo, with_qual):
    case = cg.geometry_case(*geo)
    assert _check_mask(hip_ctx, case, _Dev(hip_ctx, case), with_qual) > 500


@GEO
def test_filter_low_qual(hip_ctx, geo):
    case = cg.geometry_case(*geo)
    assert _check_filter(hip_ctx, case, _Dev(hip_ctx, case)) > 300


def _dev_row_qual(ctx, labels, acc, O, shift):
    """the device-resident form on uploaded copies -> (qual, counts); shift: floats by which acc is moved off its 16-byte
    alignment (the kernel then stages with 4-byte loads)"""
    B, L = labels.shape
    lab = _up(labels)
    buf = torch.zeros(acc.size + 4, dtype=torch.float32, device="cuda")
    a = buf[shift:shift + acc.size]
    a.copy_(torch.from_numpy(np.array(acc).ravel()))
    assert a.data_ptr() % 16 == 4 * shift
    qual = torch.full((B, L), MARK, dtype=torch.uint8, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.polish_row_qual_dev(lab.data_ptr(), a.data_ptr(), B, qual.data_ptr(), counts.data_ptr(), L, O)
    ctx.synchronize()
    return qual.cpu().numpy(), counts.cpu().numpy().tolist()


def _check_row_qual(ctx, labels, acc, O, planted):
    B, L = labels.shape
    want = qr.row_qual(labels, acc, O)
    assert all(want.reshape(-1)[t] == q for t, q in planted.items()) and len(planted) >= min(16, B * L)
    # the checker's count plane: without an overlap no row is divided by 1, with half a chunk of it none by 2; and the rows
    # tell: dividing by the other count gives other qualities
    cnt = qr.row_counts(L, O)
    assert O > 0 or (cnt == 2.0).all()
    assert 2 * O < L or (cnt == 1.0).all()
    v = np.take_along_axis(np.asarray(acc), labels.astype(np.intp)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        other = qr.qual_of_err(np.float32(1.0) - v / (np.float32(3.0) - cnt)[None, :])
    assert (other != want).any()
    got = ctx.polish_row_qual(labels, acc, O)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for shift in (0, 1):
        dq, c = _dev_row_qual(ctx, labels, acc, O, shift)
        assert c == [B * L, 0, -1, 0] and np.array_equal(dq, want), shift


@GEO
def test_row_qual(hip_ctx, geo):
    case = cg.geometry_case(*geo)
    _check_row_qual(hip_ctx, case.labels, case.acc, geo[1], case.planted)


@pytest.mark.parametrize("sizes", [(1, 0), (255, 127), (256, 128), (257, 128)], ids=cg.geo_id)
def test_row_qual_of_one_chunk(hip_ctx, sizes):
    """1, 255, 256 and 257 rows in all: fewer than a block of the row kernel, one block exactly, one row more"""
    L, O = sizes
    rng = np.random.default_rng(L)
    labels = rng.integers(0, 5, (1, L)).astype(np.uint8)
    acc = (rng.random((1, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
    _check_row_qual(hip_ctx, labels, acc, O, cg.plant_thresholds(labels, acc, O))


@GEO
def test_chain_mask_filter_stitch_and_edits(hip_ctx, geo):
    """what the polisher runs, in place on one pair of device arrays: minimum depth, minimum quality, then the stitch with
    qualities and the edits on what is left. Each pass equals its checker, and the edits applied to the draft spell the
    stitch: the passes agree on who owns a shared column."""
    case = cg.geometry_case(*geo)
    lay, dev = case.lay, _Dev(hip_ctx, case)
    lab, rq = _up(case.labels), _up(case.rq)
    code, c_mk = dev.mask(lab, rq, case.min_depth, lab, rq)
    assert code is None and c_mk == [case.masked[2], 0, -1, case.masked[3]]
    code, c_fl = dev.filter(lab, rq, cg.MIN_QUAL, lab, rq)
    after = case.chained
    assert code is None and c_fl == [after.filter_counts[0], 0, -1, after.filter_counts[1]]
    assert np.array_equal(lab.cpu().numpy(), after.labels) and np.array_equal(rq.cpu().numpy(), after.rq)
    code, roff, seq, qual, c_st = dev.stitch(lab, rq)
    seqs = [s for s, _ in after.stitch_qual]
    off = _offsets(seqs)
    total = int(off[-1])
    assert code is None and c_st == [total, 0, -1, 0] and np.array_equal(roff, off)
    assert seq[:total].tobytes() == b"".join(seqs) and qual[:total].tobytes() == b"".join(q for _, q in after.stitch_qual)
    code, eoff, recs, raw, c_ed = dev.edits(lab, rq)
    want, want_off = after.edits(True)
    assert code is None and c_ed == [len(want), 0, -1, 0] and np.array_equal(eoff, want_off) and recs[:len(want)].tolist() == want
    assert 0 < len(want) < len(case.edits(True)[0])
    for g in range(lay.n_regions):
        draft = case.contig_draft(g)
        records = pe.compose_records("c", recs[eoff[g]:eoff[g + 1]], draft, True)
        assert er.apply([tuple(r) for r in records], draft, case.cut(g)) == seq[off[g]:off[g + 1]].tobytes().decode(), g
        assert len(records) > 0


# ---- 4. chunk-id decade steps ------------------------------------------------------------------------------------------------------

def test_chunk_id_decade_steps(hip_ctx):
    """chunks 9, 99 and 999 own what they share with the next chunk ("9" sorts behind "10"); 8, 10, 98, 100, 998 and 1000 do
    not. Stitch, edits and filter name the same owner."""
    lay = cg.decade_layout()
    labels = cg.decade_labels(lay)
    rq = np.broadcast_to((20 + np.arange(lay.n) % 50).astype(np.uint8)[:, None], labels.shape).copy()
    case = cg.Case(lay, labels, rq)
    dev = _Dev(hip_ctx, case)
    _check_stitch(hip_ctx, case, dev)
    _check_edits(hip_ctx, case, dev, True)
    owner = {c: c if c in cg.DECADE_STRING_OWNER else c + 1 for c in cg.DECADE_C}
    roff, seq, qual = hip_ctx.polish_stitch_qual(lay.out, labels, rq, lay.ref_start, seq_length=8, seq_overlap=4)
    assert roff.tolist() == [0, 4_100, 4_100 + 59] and seq.count(b"A") == len(seq) - 36
    eoff, recs = hip_ctx.polish_edits(lay.out, labels, lay.batch, row_qual=rq, seq_length=8, seq_overlap=4)
    assert eoff.tolist() == [0, 36, 36]
    for i, c in enumerate(cg.DECADE_C):
        at = slice(4 * (c + 1), 4 * (c + 1) + 4)
        mine = c in cg.DECADE_STRING_OWNER
        assert seq[at] == (b"CCCC" if mine else b"GGGG"), c
        assert list(qual[at]) == [20 + owner[c] % 50] * 4, c
        assert recs[4 * i:4 * i + 4].tolist() == [(p, 0, er.SUB, ord("A"), ord("C" if mine else "G"), 20 + owner[c] % 50)
                                                  for p in range(at.start, at.stop)], c
    # the filter: low qualities on both copies of those columns only -> the rows it takes back are the owner's
    low = np.full(labels.shape, 60, np.uint8)
    cells = set()
    for c in cg.DECADE_C:
        low[c, 4:], low[c + 1, :4] = 5, 5
        cells |= {(c, 4 + i) if owner[c] == c else (c + 1, i) for i in range(4)}
    case = cg.Case(lay, labels, low)
    _check_filter(hip_ctx, case, dev)
    got_lab, got_q = hip_ctx.polish_filter_low_qual(lay.out, labels, lay.batch, cg.MIN_QUAL, low, 8, 4)
    assert {(int(k), int(j)) for k, j in np.argwhere(got_lab != labels)} == cells
    assert {(int(k), int(j)) for k, j in np.argwhere(got_q != low)} == cells
    assert all(got_lab[k, j] == 1 and got_q[k, j] == 0 for k, j in cells)


# ---- 5. chunk counts at the one-block folds ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_chunks", cg.N_CHUNKS)
def test_chunk_counts_around_the_fold_width(hip_ctx, n_chunks):
    case = cg.count_case(n_chunks)
    dev = _Dev(hip_ctx, case)
    assert _check_stitch(hip_ctx, case, dev) > 0
    for with_qual in (False, True):
        _check_edits(hip_ctx, case, dev, with_qual)
        _check_mask(hip_ctx, case, dev, with_qual)
    _check_filter(hip_ctx, case, dev)


def _poisoned(ctx, case, dev, chunks, first):
    """label 255 on an owned column of each of `chunks`: stitch, edits and filter report PV_ERR_STATE and the chunk `first`,
    and write no base, quality, record or label (the region offsets, which the fold writes under any status once the layout
    is in order, are not looked at)"""
    lay = case.lay
    bad = case.labels.copy()
    for k in chunks:
        bad[k, int(np.flatnonzero(case.owned[k])[0])] = 255
    lab, rq = _up(bad), _up(case.rq)
    for with_qual in (False, True):
        code, _, seq, qual, c = dev.stitch(lab, rq if with_qual else None)
        assert code is None and c[1:] == [_ffi.PV_ERR_STATE, first, 0] and (seq == MARK).all() and (qual == QMARK).all(), chunks
    code, _, _, raw, c = dev.edits(lab, rq)
    assert code is None and c[1:] == [_ffi.PV_ERR_STATE, first, 0] and (raw == MARK).all(), chunks
    for in_place in (False, True):
        code, out_lab, out_q, in_lab, in_q, c = dev.rewrite("filter", bad, case.rq, 94, in_place)
        assert code is None and c == [0, _ffi.PV_ERR_STATE, first, 0], chunks
        assert np.array_equal(in_lab, bad) and np.array_equal(in_q, case.rq)
        assert in_place or ((out_lab == MARK).all() and (out_q == MARK).all())
    for call in (lambda: ctx.polish_stitch(lay.out, bad, lay.ref_start, seq_length=lay.L, seq_overlap=lay.O),
                 lambda: ctx.polish_edits(lay.out, bad, lay.batch, seq_length=lay.L, seq_overlap=lay.O),
                 lambda: ctx.polish_filter_low_qual(lay.out, bad, lay.batch, 94, case.rq, lay.L, lay.O)):
        with pytest.raises(_ffi.PepperHipError) as e:
            call()
        assert e.value.code == _ffi.PV_ERR_STATE and ("chunk %d " % first) in str(e.value)


@pytest.mark.parametrize("n_chunks", [1025, 2049])
def test_first_poisoned_chunk_across_the_fold_segments(hip_ctx, n_chunks):
    """a fold thread holds `per` chunks: the bad chunk in the first and the last chunk, and either side of the boundary between
    the first two threads' segments; of two bad chunks the first is reported"""
    case = cg.count_case(n_chunks)
    dev = _Dev(hip_ctx, case)
    per = -(-n_chunks // cg.FOLD_THREADS)
    assert per == {1025: 2, 2049: 3}[n_chunks]
    for k in (0, n_chunks - 1, per - 1, per):
        _poisoned(hip_ctx, case, dev, [k], k)
    _poisoned(hip_ctx, case, dev, [per - 1, per], per - 1)
    _poisoned(hip_ctx, case, dev, [n_chunks - 1, per], per)


# ---- 6. the range's outer edge ---------------------------------------------------------------------------------------------------------

def _blank_case(width):
    """two chunks of `width` columns over an all-A draft, every array as large as a call that is told `width` may read"""
    lay = mc.Layout([(0, b"A" * (2 * width), {})], width, 0)
    assert lay.n == 2
    return cg.Case(lay, np.full((2, width), 2, np.uint8), np.full((2, width), 30, np.uint8), depth=np.zeros((2, width), np.uint16))


def _refused(case, dev, mask=False):
    lab, rq = _up(case.labels), _up(case.rq)
    for with_qual in (False, True):
        code, roff, seq, qual, c = dev.stitch(lab, rq if with_qual else None)
        assert code == _ffi.PV_ERR_INVALID and c == [-7] * 4 and (roff == -7).all() and (seq == MARK).all() and (qual == QMARK).all()
        code, eoff, _, raw, c = dev.edits(lab, rq if with_qual else None)
        assert code == _ffi.PV_ERR_INVALID and c == [-7] * 4 and (eoff == -7).all() and (raw == MARK).all()
    for which in ("filter", "mask") if mask else ("filter",):
        for in_place in (False, True):
            code, out_lab, out_q, in_lab, in_q, c = dev.rewrite(which, case.labels, case.rq, 20, in_place)
            assert code == _ffi.PV_ERR_INVALID and c == [-7] * 4, (which, in_place)
            assert np.array_equal(in_lab, case.labels) and np.array_equal(in_q, case.rq)
            assert in_place or ((out_lab == MARK).all() and (out_q == MARK).all())


@pytest.mark.parametrize("seq_length", [0, 4097])
def test_seq_length_outside_the_range_is_refused(hip_ctx, seq_length):
    case = _blank_case(max(seq_length, 1))
    _refused(case, _Dev(hip_ctx, case, seq_length=seq_length, seq_overlap=0), mask=seq_length == 0)


@pytest.mark.parametrize("sizes", [(7, 7), (7, 4), (4096, 4096), (4096, 2049)], ids=cg.geo_id)
def test_seq_overlap_outside_the_range_is_refused(hip_ctx, sizes):
    """seq_overlap = seq_length, and the smallest overlap above half a chunk (2 * 4 = 7 + 1; 4096 is even, so 2 * 2049 = 4096 + 2)"""
    L, O = sizes
    assert O == L or O == L // 2 + 1
    case = cg.geometry_case(L, L // 2)
    _refused(case, _Dev(hip_ctx, case, seq_overlap=O))
    if L == 7:                                                        # the host forms refuse it too, and return nothing
        lay = case.lay
        for call in (lambda: hip_ctx.polish_stitch(lay.out, case.labels, lay.ref_start, seq_length=L, seq_overlap=O),
                     lambda: hip_ctx.polish_stitch_qual(lay.out, case.labels, case.rq, lay.ref_start, seq_length=L, seq_overlap=O),
                     lambda: hip_ctx.polish_edits(lay.out, case.labels, lay.batch, seq_length=L, seq_overlap=O),
                     lambda: hip_ctx.polish_filter_low_qual(lay.out, case.labels, lay.batch, 20, case.rq, L, O)):
            with pytest.raises(_ffi.PepperHipError) as e:
                call()
            assert e.value.code == _ffi.PV_ERR_INVALID
