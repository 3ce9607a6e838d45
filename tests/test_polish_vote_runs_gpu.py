"""GPU: `polish --vote --runs`: pv_polish_vote_runs[_dev] against the host checker (tests/vote_runs_ref.py). Every kernel test
goes builder -> column vote -> run vote on the device, from hand-made reads (tests/vote_runs_cases.py), and asks for the
checker's labels, acc and six counters byte for byte, in the device form and in the host form; then the command end to end
against a known true sequence, and against the column vote alone on reads with ordinary run-length noise. Nothing here has a
tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import edits_ref as er
import vote_runs_cases as rc
import vote_runs_ref as rr
from pepper_thesis_amd import _ffi, assess, bamio, cli, polish
from pepper_thesis_amd.batch import Region, pack_regions
from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut
from test_polish_hp_gpu import inputs as hp_inputs         # noqa: F401  the tagged BAM and its two pre-split files

pytestmark = pytest.mark.gpu
L, O = 64, 8
MARK, ACC_MARK = 0xEE, -7.5
BASES = "ACGT"


# ---- builder -> vote -> run vote ------------------------------------------------------------------------------------------------

class _Chain:
    """the builder and the column vote of a batch on the device; run() then votes the runs on a copy of the vote's planes"""

    def __init__(self, ctx, batch, L_=L, O_=O):
        self.ctx, self.batch, self.L, self.O = ctx, batch, L_, O_
        self.db = DeviceBatch(batch)
        cols = int((batch.ref_end - batch.ref_start + 1).sum())
        cap = 3 * cols // (L_ - O_) + 3 * batch.n_regions + 4
        self.do = DevicePolishOut(cap, L_, O_, depth=True, counts=True)
        self.lab = torch.full((cap, L_), MARK, dtype=torch.uint8, device="cuda")
        self.acc = torch.full((cap, L_, 5), ACC_MARK, dtype=torch.float32, device="cuda")
        self.cnt = torch.full((6,), -7, dtype=torch.int64, device="cuda")
        vcnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.polish_summarize_dev(self.db, self.do)
        ctx.synchronize()
        self.n = self.do.n_chunks()
        assert self.do.status() == 0 and 0 < self.n <= cap, (self.do.status(), self.n, cap)
        self.common = (self.db.t["ref_start"].data_ptr(), self.db.t["ref_off"].data_ptr(), self.db.t["ref"].data_ptr(), batch.n_regions)
        ctx.polish_vote_dev(self.do, self.n, *self.common, self.lab.data_ptr(), self.acc.data_ptr(), vcnt.data_ptr())
        ctx.synchronize()
        assert vcnt.tolist()[1:3] == [0, -1]
        n = self.n
        self.position, self.index = self.do.position[:n].cpu().numpy(), self.do.index[:n].cpu().numpy()
        self.region, self.chunk_id = self.do.region[:n].cpu().numpy(), self.do.chunk_id[:n].cpu().numpy()
        self.lab0, self.acc0 = self.lab[:n].cpu().numpy(), self.acc[:n].cpu().numpy()
        self.out = type("Out", (), dict(position=self.position, index=self.index, region=self.region, chunk_id=self.chunk_id))

    def want(self, min_run=3, acc=True, batch=None):
        return rr.vote_runs(batch or self.batch, self.position, self.index, self.region, self.chunk_id, self.lab0,
                            self.acc0 if acc else None, self.O, min_run)

    def run(self, min_run=3, acc=True, n=None, db=None):
        """the device form on fresh copies of the vote's planes -> (labels, acc, d_counts), the call's error code in front when
        it was refused"""
        self.lab[:self.n].copy_(torch.from_numpy(self.lab0))
        self.acc[:self.n].copy_(torch.from_numpy(self.acc0))
        self.cnt.fill_(-7)
        torch.cuda.synchronize()
        code = None
        try:
            self.ctx.polish_vote_runs_dev(self.do, self.n if n is None else n, db or self.db, *self.common, min_run,
                                          self.lab.data_ptr(), self.acc.data_ptr() if acc else 0, self.cnt.data_ptr())
        except _ffi.PepperHipError as e:
            code = e.code
        self.ctx.synchronize()
        res = (self.lab[:self.n].cpu().numpy(), self.acc[:self.n].cpu().numpy(), self.cnt.tolist())
        return res if code is None else (code,) + res

    def host(self, min_run=3, acc=True):
        c = (C.c_int64 * 6)()
        lab, a = self.lab0.copy(), self.acc0.copy() if acc else None
        self.ctx.polish_vote_runs(self.out, self.batch, lab, a, min_run, self.L, self.O, counts=c)
        return lab, a, list(c)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(ctx, batch, L_=L, O_=O, min_run=3):
    """device form and host form against the checker, with and without acc -> (chain, checker's labels, counters, runs)"""
    ch = _Chain(ctx, batch, L_, O_)
    w_lab, w_acc, w_cnt, runs = ch.want(min_run)
    lab, acc, cnt = ch.run(min_run)
    assert cnt == w_cnt, (cnt, w_cnt)
    assert np.array_equal(lab, w_lab) and np.array_equal(_bits(acc), _bits(w_acc))
    lab, acc, cnt = ch.run(min_run, acc=False)                       # acc == NULL: the plane stays as the vote left it
    assert cnt == w_cnt and np.array_equal(lab, w_lab) and np.array_equal(_bits(acc), _bits(ch.acc0))
    lab, acc, cnt = ch.host(min_run)
    assert cnt == w_cnt and np.array_equal(lab, w_lab) and np.array_equal(_bits(acc), _bits(w_acc))
    lab, _, cnt = ch.host(min_run, acc=False)
    assert cnt == w_cnt and np.array_equal(lab, w_lab)
    # the copies of a row two chunks share agree
    seen = {}
    for k, j in zip(*np.nonzero(ch.position >= 0)):
        key = (int(ch.region[k]), int(ch.position[k, j]), int(ch.index[k, j]))
        assert seen.setdefault(key, int(w_lab[k, j])) == int(w_lab[k, j]), key
    return ch, w_lab, w_cnt, runs


def _reads(draft, start, lengths, s, n, anchors=None, span=None, **kw):
    """reads over span (default: the whole draft) that show lengths[i] letters for the run [s, s + n)"""
    a, b = span or (0, len(draft))
    return [rc.read_over(draft, start, a, b, rc.run_edits(s, n, draft[s].upper(), ln, None if anchors is None else anchors[i]),
                         is_reverse=bool(i % 2), **kw) for i, ln in enumerate(lengths)]


def _spelled(ch, lab, g=0):
    return rc.spelled(ch, lab, g)


# ---- 1. random regions -------------------------------------------------------------------------------------------------------------

def _random_region(rng, start, length, n_reads, lower=True):
    runs, off = {}, int(rng.integers(5, 15))
    while off + 14 < length - 5:
        n = int(rng.integers(3, 11))
        runs[off] = (BASES[int(rng.integers(4))], n)
        off += n + int(rng.integers(3, 20))
    draft = rc.draft_with_runs(rng, length, runs)
    reads = []
    for i in range(n_reads):
        a = 0 if rng.random() < 0.5 else int(rng.integers(0, length // 2))
        b = length if rng.random() < 0.5 else int(rng.integers(length // 2 + 1, length))
        edits = {}
        for s, (letter, n) in runs.items():
            if a > s - 1 or b < s + n + 1:
                continue                                           # the read starts or ends inside the run or its flanks
            u = rng.random()
            ln = n if u < 0.45 else n - 1 if u < 0.65 else n + 1 if u < 0.85 else max(0, n - 2) if u < 0.93 else n + 2
            edits.update(rc.run_edits(s, n, letter, ln, int(rng.integers(s - 1, s + n))))
        for p in rng.choice(np.arange(a + 1, b - 1), size=4, replace=False).tolist():   # wrong bases, in runs and flanks too
            if p not in edits:
                edits[p] = ("sub", BASES[int(rng.integers(4))])
        reads.append(rc.read_over(draft, start, a, b, edits, is_reverse=bool(rng.integers(2)), mapq=0 if rng.random() < 0.1 else 60))
    if lower:
        draft = "".join(c.lower() if rng.random() < 0.3 else c for c in draft)
    return Region(start, start + length - 1, draft.encode(), reads)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_regions(hip_ctx, seed):
    rng = np.random.default_rng(seed)
    batch = pack_regions([_random_region(rng, 0, 300 + 17 * seed, 24), _random_region(rng, 5000, 131, 9),
                          _random_region(rng, 9000, 260, 30)])
    ch, lab, cnt, runs = _check(hip_ctx, batch)
    assert cnt[0] >= 20 and cnt[3] >= 3 and cnt[4] >= cnt[0] and ch.n >= 8
    assert not np.array_equal(lab, ch.lab0)                       # the run vote changed what the column vote left
    _check(hip_ctx, batch, min_run=5)


def test_the_real_chunk_geometry(hip_ctx):
    """seq_length 1000, overlap 50: several rounds of 256 rows in the write pass, and nine tiles of 256 draft bytes"""
    rng = np.random.default_rng(5)
    batch = pack_regions([_random_region(rng, 0, 2300, 22), _random_region(rng, 7000, 700, 12)])
    ch, lab, cnt, runs = _check(hip_ctx, batch, 1000, 50)
    assert ch.n >= 4 and cnt[0] >= 100


# ---- 2. where a run lies ----------------------------------------------------------------------------------------------------------

def test_a_run_across_a_chunk_boundary_and_one_inside_the_overlap(hip_ctx):
    """chunk 1 starts at flat row 56 and chunk 0 ends behind row 63: the run at 57..61 lies in both, the run at 60 + 56.. crosses
    from chunk 1 into chunk 2; both copies of every shared row are rewritten alike"""
    rng = np.random.default_rng(7)
    draft = rc.draft_with_runs(rng, 200, {57: ("A", 5), 116: ("C", 8)})
    reads = []
    for i in range(20):
        ed = dict(rc.run_edits(57, 5, "A", 4 if i < 12 else 5))
        ed.update(rc.run_edits(116, 8, "C", 8 if i < 9 else 7 if i < 15 else 6))
        reads.append(rc.read_over(draft, 300, 0, 200, ed, is_reverse=bool(i % 2)))
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads, 300))
    assert cnt == [2, 0, -1, 1, 2, 0] and [r.L for r in runs] == [4, 8]
    for lo, hi in ((357, 361), (416, 423)):
        chunks = sorted(set(np.nonzero((ch.position >= lo) & (ch.position <= hi))[0].tolist()))
        assert len(chunks) == 2, (lo, chunks)
    assert _spelled(ch, ch.lab0) == draft[:57] + "A" * 4 + draft[62:116] + "C" * 7 + draft[124:]     # the column vote: 4 and 7
    assert _spelled(ch, lab) == draft[:57] + "A" * 4 + draft[62:]                                   # the run vote: 4 and 8


def test_a_run_at_the_first_or_last_column_is_no_candidate(hip_ctx):
    rng = np.random.default_rng(8)
    draft = "TTTT" + rc.plain(rng, 40, "T", "G") + "GGGGG" + rc.plain(rng, 40, "G", "A") + "AAAA"
    reads = [rc.read_over(draft, 0, 0, len(draft), {44: ("del", 1)}, is_reverse=bool(i % 2)) for i in range(12)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert cnt == [1, 0, -1, 1, 1, 0] and (runs[0].s, runs[0].n, runs[0].L) == (44, 5, 4)


def test_run_lengths_min_run_48_and_49(hip_ctx):
    rng = np.random.default_rng(9)
    draft = rc.draft_with_runs(rng, 260, {10: ("A", 2), 30: ("C", 3), 60: ("G", 48), 130: ("T", 49), 200: ("A", 4)})
    reads = []
    for i in range(14):
        ed = {}
        for s, n in ((10, 2), (30, 3), (60, 48), (130, 49), (200, 4)):
            ed.update(rc.run_edits(s, n, draft[s], n - 1 if i < 9 else n))
        reads.append(rc.read_over(draft, 0, 0, 260, ed, is_reverse=bool(i % 2)))
    batch = rc.one_region(draft, reads)
    ch, lab, cnt, runs = _check(hip_ctx, batch)
    assert cnt == [3, 0, -1, 3, 3, 0] and [(r.s, r.n, r.L) for r in runs] == [(30, 3, 2), (60, 48, 47), (200, 4, 3)]
    ch, lab, cnt, runs = _check(hip_ctx, batch, min_run=4)
    assert cnt == [2, 0, -1, 2, 2, 0]
    ch, lab, cnt, runs = _check(hip_ctx, batch, min_run=2)
    assert cnt == [4, 0, -1, 4, 4, 0]
    ch, lab, cnt, runs = _check(hip_ctx, batch, min_run=48)
    assert cnt == [1, 0, -1, 1, 1, 0]


def test_read_lengths_0_63_and_64(hip_ctx):
    """a read that shows 64 letters spans the run and does not vote; 63 and 0 are lengths like any other"""
    rng = np.random.default_rng(10)
    draft = rc.draft_with_runs(rng, 200, {40: ("A", 40), 130: ("T", 6)})
    reads = []
    for i in range(10):
        ed = dict(rc.run_edits(40, 40, "A", 63 if i < 5 else 64 if i < 8 else 0, 50))
        ed.update(rc.run_edits(130, 6, "T", 0 if i < 6 else 6))
        reads.append(rc.read_over(draft, 0, 0, 200, ed, is_reverse=bool(i % 2)))
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert [(r.S, r.V, r.L) for r in runs] == [(10, 7, 63), (10, 10, 0)] and runs[0].h[63] == 5 and runs[0].h[0] == 2
    assert cnt == [2, 0, -1, 2, 2, 0]
    assert _spelled(ch, lab) == draft[:40] + "A" * 63 + draft[80:130] + draft[136:]
    # three voters of 64 and two of 63: the three span and do not vote, 2 * 2 <= 5 leaves the run alone
    reads = _reads(draft, 0, [64] * 3 + [63] * 2, 40, 40, anchors=[50] * 5)
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert (runs[0].S, runs[0].V, runs[0].L) == (5, 2, None) and np.array_equal(lab, ch.lab0)


def test_adjacent_candidates_are_skipped_and_counted(hip_ctx):
    rng = np.random.default_rng(11)
    draft = rc.plain(rng, 30, "", "A") + "AAAATTTTT" + rc.plain(rng, 30, "T", "C") + "CCCC" + rc.plain(rng, 1, "C", "G") + "GGG" + \
        rc.plain(rng, 30, "G")
    reads = [rc.read_over(draft, 0, 0, len(draft), {30: ("del", 1), 34: ("del", 1), 69: ("del", 1), 74: ("del", 1)},
                          is_reverse=bool(i % 2)) for i in range(9)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    # AAAA and TTTTT touch: both stay with the column vote; CCCC and GGG share a flank, which is no adjacency
    assert cnt == [2, 0, -1, 2, 4, 2] and [(r.s, r.b) for r in runs] == [(69, "C"), (74, "G")]


def test_a_draft_n_inside_a_stretch_of_one_letter(hip_ctx):
    """AAANAAA is two runs of three with the N as a flank of each; a read that shows A under the N is impure for both"""
    rng = np.random.default_rng(12)
    draft = rc.plain(rng, 30, "", "A") + "AAANAAA" + rc.plain(rng, 30, "A")
    pure = [rc.read_over(draft, 0, 0, len(draft), {30: ("del", 1), 33: ("sub", "C")}, is_reverse=bool(i % 2)) for i in range(8)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, pure))
    assert cnt == [2, 0, -1, 1, 2, 0] and [(r.s, r.n, r.L) for r in runs] == [(30, 3, 2), (34, 3, 3)]
    impure = [rc.read_over(draft, 0, 0, len(draft), {30: ("del", 1), 33: ("sub", "A")}, is_reverse=bool(i % 2)) for i in range(8)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, impure))
    assert cnt == [0, 0, -1, 0, 2, 0] and [(r.S, r.V) for r in runs] == [(8, 0), (8, 0)] and np.array_equal(lab, ch.lab0)


# ---- 3. who votes -----------------------------------------------------------------------------------------------------------------

def test_mapq_0_reads_are_not_counted(hip_ctx):
    rng = np.random.default_rng(13)
    draft = rc.draft_with_runs(rng, 120, {50: ("G", 6)})
    reads = _reads(draft, 0, [6] * 6 + [5] * 3, 50, 6) + _reads(draft, 0, [4] * 30, 50, 6, mapq=0)
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert (runs[0].S, runs[0].V, runs[0].L) == (9, 9, 6) and runs[0].h[4] == 0


def test_a_read_that_starts_or_ends_inside_the_run_does_not_span_it(hip_ctx):
    rng = np.random.default_rng(14)
    draft = rc.draft_with_runs(rng, 120, {50: ("C", 6)})
    reads = _reads(draft, 0, [5] * 4 + [6] * 2, 50, 6)
    reads += [rc.read_over(draft, 0, 52, 120), rc.read_over(draft, 0, 0, 54), rc.read_over(draft, 0, 50, 120),
              rc.read_over(draft, 0, 0, 56), rc.read_over(draft, 0, 49, 56), rc.read_over(draft, 0, 0, 49), rc.read_over(draft, 0, 57, 120)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert (runs[0].S, runs[0].V, runs[0].L) == (6, 6, 5)
    # the flanks alone are enough: [49, 57) spans
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads + [rc.read_over(draft, 0, 49, 57)]))
    assert (runs[0].S, runs[0].V) == (7, 7)
    # a flank the read deletes, or reaches only with a clipped base, is no aligned base
    more = [rc.read_over(draft, 0, 0, 120, {49: ("del", 1)}), rc.read_over(draft, 0, 0, 120, {56: ("del", 2)})]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads + more))
    assert (runs[0].S, runs[0].V) == (6, 6)


def test_a_read_whose_flank_byte_is_the_runs_letter_spans_and_does_not_vote(hip_ctx):
    rng = np.random.default_rng(15)
    draft = rc.draft_with_runs(rng, 120, {50: ("T", 5)})
    reads = _reads(draft, 0, [4] * 5, 50, 5)
    reads += [rc.read_over(draft, 0, 0, 120, {49: ("sub", "T")}), rc.read_over(draft, 0, 0, 120, {55: ("sub", "T")}),
              rc.read_over(draft, 0, 0, 120, {52: ("sub", "N")}), rc.read_over(draft, 0, 0, 120, {52: ("sub", "t")})]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert (runs[0].S, runs[0].V, runs[0].L) == (9, 6, 4) and runs[0].h[5] == 1      # the lower-case t is a T


def test_an_impure_majority_leaves_the_run_and_the_inserted_base_survives(hip_ctx):
    """a C inserted behind an A run in 15 of 20 reads: most reads are impure, the run is undecided, and the column vote's
    inserted C stays where it is"""
    rng = np.random.default_rng(16)
    draft = rc.draft_with_runs(rng, 120, {50: ("A", 5)})
    reads = [rc.read_over(draft, 0, 0, 120, {54: ("ins", "C")} if i < 15 else rc.run_edits(50, 5, "A", 4), is_reverse=bool(i % 2))
             for i in range(20)]
    ch, lab, cnt, runs = _check(hip_ctx, rc.one_region(draft, reads))
    assert (runs[0].S, runs[0].V, runs[0].L) == (20, 5, None) and cnt == [0, 0, -1, 0, 1, 0]
    assert np.array_equal(lab, ch.lab0) and lab[(ch.position == 54) & (ch.index == 1)].tolist() == [2]
    assert _spelled(ch, lab) == draft[:55] + "C" + draft[55:]


# ---- 4. what the call refuses, and what it leaves --------------------------------------------------------------------------------

def test_no_chunks_and_a_bad_min_run(hip_ctx):
    rng = np.random.default_rng(17)
    draft = rc.draft_with_runs(rng, 120, {50: ("A", 5)})
    ch = _Chain(hip_ctx, rc.one_region(draft, _reads(draft, 0, [4] * 6, 50, 5)))
    lab, acc, cnt = ch.run(n=0)
    assert cnt == [0, 0, -1, 0, 0, 0] and np.array_equal(lab, ch.lab0) and np.array_equal(_bits(acc), _bits(ch.acc0))
    for bad in (1, 0, -3, 49, 1000):
        code, lab, acc, cnt = ch.run(min_run=bad)
        assert code == _ffi.PV_ERR_INVALID and cnt == [-7] * 6 and np.array_equal(lab, ch.lab0), bad
        c = (C.c_int64 * 6)()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_vote_runs(ch.out, ch.batch, ch.lab0.copy(), None, bad, L, O, counts=c)
        assert e.value.code == _ffi.PV_ERR_INVALID and list(c) == [0] * 6 and "min_run" in str(e.value)
    none = type("Out", (), dict(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32), region=np.zeros(0, np.int32),
                                chunk_id=np.zeros(0, np.int32)))
    c = (C.c_int64 * 6)()
    hip_ctx.polish_vote_runs(none, ch.batch, np.zeros((0, L), np.uint8), np.zeros((0, L, 5), np.float32), 3, L, O, counts=c)
    assert list(c) == [0, 0, -1, 0, 0, 0]
    assert rr.vote_runs(ch.batch, none.position, none.index, none.region, none.chunk_id, np.zeros((0, L), np.uint8), None, O, 3)[2] == list(c)


def test_a_broken_layout_leaves_everything_but_the_counts(hip_ctx):
    rng = np.random.default_rng(18)
    draft = rc.draft_with_runs(rng, 200, {50: ("A", 5), 150: ("G", 4)})
    reads = []
    for i in range(8):
        ed = dict(rc.run_edits(50, 5, "A", 4))
        ed.update(rc.run_edits(150, 4, "G", 5))
        reads.append(rc.read_over(draft, 1000, 0, 200, ed, is_reverse=bool(i % 2)))
    batch = pack_regions([Region(1000, 1199, draft.encode(), reads), Region(3000, 3199, draft.encode(), [
        rc.read_over(draft, 3000, 0, 200, rc.run_edits(50, 5, "A", 4)) for _ in range(4)])])
    ch = _Chain(hip_ctx, batch)
    w_lab, w_acc, w_cnt, _ = ch.want()
    assert w_cnt == [4, 0, -1, 3, 4, 0] and ch.run()[2] == w_cnt
    k = int(np.flatnonzero(ch.region == 1)[1])
    j = int(np.flatnonzero(ch.index[k] == 0)[3])
    keep_cid, keep_pos = ch.do.chunk_id.clone(), ch.do.position.clone()
    for what, bad in (("cid", 2), ("high", k), ("low", k)):
        if what == "cid":
            ch.do.chunk_id[2] = 7                                  # chunk ids 0, 1, 7 inside region 0
        else:
            ch.do.position[k, j] = 3200 if what == "high" else 2999   # one past the last, one below the first draft byte of region 1
        pos, cid = ch.do.position[:ch.n].cpu().numpy(), ch.do.chunk_id[:ch.n].cpu().numpy()
        with pytest.raises(rr.BadChunk) as e:
            rr.vote_runs(batch, pos, ch.index, ch.region, cid, ch.lab0, ch.acc0, O, 3)
        assert e.value.chunk == bad
        lab, acc, cnt = ch.run()
        assert cnt == [0, _ffi.PV_ERR_INVALID, bad, 0, 4, 0], what
        assert np.array_equal(lab, ch.lab0) and np.array_equal(_bits(acc), _bits(ch.acc0))
        out = type("Out", (), dict(position=pos, index=ch.index, region=ch.region, chunk_id=cid))
        c = (C.c_int64 * 6)()
        h_lab, h_acc = ch.lab0.copy(), ch.acc0.copy()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_vote_runs(out, batch, h_lab, h_acc, 3, L, O, counts=c)
        assert e.value.code == _ffi.PV_ERR_INVALID and list(c) == [0, _ffi.PV_ERR_INVALID, bad, 0, 4, 0] and "chunk %d" % bad in str(e.value)
        assert np.array_equal(h_lab, ch.lab0) and np.array_equal(_bits(h_acc), _bits(ch.acc0))
        ch.do.chunk_id.copy_(keep_cid)
        ch.do.position.copy_(keep_pos)
    lab, acc, cnt = ch.run()
    assert cnt == w_cnt and np.array_equal(lab, w_lab)


def test_vote_and_run_vote_replay_as_one_graph(hip_ctx):
    """the column vote and the run vote captured together; between replays the reads change under the same chunks (some get
    mapping quality 0), and every replay gives the bytes of the eager calls on the same reads"""
    rng = np.random.default_rng(19)
    batch = pack_regions([_random_region(rng, 0, 330, 26), _random_region(rng, 4000, 150, 10)])
    ch = _Chain(hip_ctx, batch)
    vcnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    st = hip_ctx.stream
    mapq = [batch.read_mapq.copy() for _ in range(3)]
    mapq[1][::3] = 0
    mapq[2][1::2] = 0
    variants = []
    for m in mapq:
        b = pack_regions([batch.region(g) for g in range(batch.n_regions)])
        b.read_mapq[:] = m
        variants.append(b)

    def passes():
        hip_ctx.polish_vote_dev(ch.do, ch.n, *ch.common, ch.lab.data_ptr(), ch.acc.data_ptr(), vcnt.data_ptr(), stream=st)
        hip_ctx.polish_vote_runs_dev(ch.do, ch.n, ch.db, *ch.common, 3, ch.lab.data_ptr(), ch.acc.data_ptr(), ch.cnt.data_ptr(), stream=st)

    def refill(k):
        ch.db.t["read_mapq"].copy_(torch.from_numpy(mapq[k]))
        for t in (ch.lab, ch.acc, ch.cnt, vcnt):
            t.zero_()
        torch.cuda.synchronize()

    def state():
        return ch.lab[:ch.n].cpu().numpy().tobytes(), ch.acc[:ch.n].cpu().numpy().tobytes(), ch.cnt.tolist(), vcnt.tolist()
    eager = []
    for k in range(3):
        refill(k)
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        w_lab, w_acc, w_cnt, _ = ch.want(batch=variants[k])
        assert eager[-1][:3] == (w_lab.tobytes(), w_acc.tobytes(), w_cnt), k
    assert eager[0][0] != eager[1][0] and eager[1][0] != eager[2][0]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        refill(k)
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 5. end to end against a known truth --------------------------------------------------------------------------------------

class _Planted:
    """a draft without accidental runs that holds, several times and away from the region boundaries: a correct run of 8
    under reads of which 9 show 8, 6 show 7 and 5 show 6 (deletions left-aligned); a run of 5 whose truth is 6, under reads of
    which 12 show 6 with the inserted base at three anchors, 4 reads each; and substitutions every read shows. 20 reads, each
    over the whole contig."""

    def __init__(self, rng, name, length=3400):
        self.name = name
        self.keep = {off: 8 for off in (300, 1400, 2400, 3250) if off < length - 100}   # offset -> n of the correct runs
        self.grow = {off: 5 for off in (600, 1600, 2600) if off < length - 100}         # offset -> n of the runs one short
        letters = {}
        for k, off in enumerate(sorted(list(self.keep) + list(self.grow))):
            letters[off] = BASES[k % 4]
        self.letter = letters
        self.D = rc.draft_with_runs(rng, length, {off: (letters[off], n) for off, n in list(self.keep.items()) + list(self.grow.items())})
        self.subs = {}
        for p in (p for p in (200, 700, 1250, 1700, 2300, 2700, 3200) if p < length - 100):
            self.subs[p] = next(b for b in BASES if b not in (self.D[p - 1], self.D[p], self.D[p + 1]))
        t = list(self.D)
        for p, b in self.subs.items():
            t[p] = b
        for off in sorted(self.grow, reverse=True):
            t.insert(off, letters[off])
        self.T = "".join(t)
        v = list(self.D)                                             # what the column vote alone gives: the correct runs one short
        for p, b in self.subs.items():
            v[p] = b
        for off in sorted(self.keep, reverse=True):
            del v[off]
        self.column_vote = "".join(v)
        self.D = self.D[:2000] + self.D[2000:2500].lower() + self.D[2500:]

    def records(self, tid):
        recs = []
        for i in range(20):
            ed = {p: ("sub", b) for p, b in self.subs.items()}
            for k, (off, n) in enumerate(sorted(self.keep.items())):
                j = (i + 7 * k) % 20
                ed.update(rc.run_edits(off, n, self.letter[off], 8 if j < 9 else 7 if j < 15 else 6))
            for k, (off, n) in enumerate(sorted(self.grow.items())):
                j = (i + 3 * k) % 20
                if j < 12:
                    ed.update(rc.run_edits(off, n, self.letter[off], 6, (off - 1, off + 1, off + 3)[j // 4]))
            recs.append(rc.bam_record(self.D, tid, 0, len(self.D), ed, 16 * (i % 2), "p%d_%d" % (tid, i)))
        return recs


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("vote_runs")
    rng = np.random.default_rng(71)
    truths = [_Planted(rng, "ctgA"), _Planted(rng, "ctgB", 2900)]
    bw.write_fasta(str(tmp / "draft.fa"), [(t.name, t.D) for t in truths])
    bw.write_fasta(str(tmp / "truth.fa"), [(t.name, t.T) for t in truths])
    recs = [r for tid, t in enumerate(truths) for r in t.records(tid)]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(t.name, len(t.D)) for t in truths], recs)
    return tmp, truths


def _polish(t, hip_ctx, name, flags, bam="reads.bam", fasta="draft.fa", want_runs=None):
    out_dir = str(t / name)
    argv = ["-b", str(t / bam), "-f", str(t / fasta), "-t", "3", "-bs", "8", "-o", out_dir, "--vote"] + flags

    def open_chain(device, shared, state_dict, dtype, **k):
        assert state_dict is None and k.get("vote") is True and k.get("vote_runs") == want_runs
        return polish._DeviceChain(hip_ctx, **k)
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(out_dir)):
        if not f.endswith(".tbi"):
            out[f] = bamio.bgzf_read_all(os.path.join(out_dir, f)) if f.endswith(".vcf.gz") else open(os.path.join(out_dir, f), "rb").read()
    return out


def _fasta(data: bytes):
    lines = data.decode().split("\n")
    return dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))


def _errors(hip_ctx, fasta: dict, truths):
    total = assess.tables(hip_ctx, [(n, s.encode()) for n, s in fasta.items()], [(t.name, t.T.encode()) for t in truths], 256, 64)[2]
    return total


def test_the_column_vote_alone_misses_the_runs_and_the_run_vote_recovers_the_truth(planted, hip_ctx, capsys):
    t, truths = planted
    alone = _fasta(_polish(t, hip_ctx, "alone", [])["_pepper_polished.fa"])
    # byte for byte what the column vote gives by its rule: the substitutions mended, the correct runs of 8 cut to 7 by the
    # piled-up deletions, the short runs left short
    assert alone == {tr.name: tr.column_vote for tr in truths}
    tot = _errors(hip_ctx, alone, truths)
    assert alone != {tr.name: tr.T for tr in truths} and tot["hp_ins"] + tot["hp_del"] > 0
    capsys.readouterr()
    got = _polish(t, hip_ctx, "runs", ["--runs", "--edits", "--qualities"], want_runs=3)
    err = capsys.readouterr().err
    assert list(got) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.fa", "_pepper_polished.fq"]
    fasta = _fasta(got["_pepper_polished.fa"])
    assert fasta == {tr.name: tr.T for tr in truths}
    tot = _errors(hip_ctx, fasta, truths)
    assert tot["sub"] + tot["ins"] + tot["del"] == 0 and tot["hp_ins"] + tot["hp_del"] == 0
    m = re.search(r"RUNS \(MIN RUN 3\): (\d+) CANDIDATE RUNS SEEN, (\d+) DECIDED BY THEIR READS, (\d+) OF THEM WITH A LENGTH THAT IS NOT "
                  r"THE DRAFT'S, (\d+) SKIPPED AS ADJACENT", err)
    n_runs, n_short = sum(len(tr.keep) + len(tr.grow) for tr in truths), sum(len(tr.grow) for tr in truths)
    assert m and [int(v) for v in m.groups()] == [n_runs, n_runs, n_short, 0]      # (no planted run lies where two regions overlap)
    # the draft with the VCF's records applied is the FASTA, and the FASTQ holds the same sequence
    text = got["_pepper_polished.edits.vcf.gz"].decode()
    header = [l[2:] for l in text.split("\n") if l.startswith("##pepper_")]
    assert header == ["pepper_consensus=vote+runs", "pepper_min_run=3"]
    info = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    for tr in truths:
        mine = [(int(f[1]), f[3], f[4], None if f[5] == "." else int(f[5])) for f in info if f[0] == tr.name]
        assert len(mine) >= 9 and er.apply(mine, tr.D.encode()) == tr.T, tr.name
    fq = got["_pepper_polished.fq"].decode().split("\n")
    assert fq[0::4][:2] == ["@" + tr.name for tr in truths] and fq[1::4] == [tr.T for tr in truths]
    # a run's rows carry the fraction of its voters that agree: 9 of 20 is Phred 2, 12 of 20 Phred 3
    q = np.frombuffer(fq[3].encode(), np.uint8) - 33
    assert q[300:308].tolist() == [2] * 8 and q[600:606].tolist() == [3] * 6


def test_gpu_decode_realign_and_the_filters_give_the_same_sequence(planted, hip_ctx):
    """the device read path and the realigner in front of the run vote, and the depth mask, the quality filter (a run-voted
    insertion that 12 of 20 voters hold has quality 3) and the evidence behind it"""
    t, truths = planted
    for name, flags in (("decode", ["--gpu_decode"]), ("realign", ["--realign"]), ("both", ["--gpu_decode", "--realign", "--min_run", "4"]),
                        ("filters", ["--edits", "--evidence", "--min_depth", "3", "--min_qual", "2"])):
        fasta = _fasta(_polish(t, hip_ctx, name, ["--runs"] + flags, want_runs=4 if "--min_run" in flags else 3)["_pepper_polished.fa"])
        assert fasta == {tr.name: tr.T for tr in truths}, name


def test_each_haplotype_votes_its_runs_with_its_own_reads(hp_inputs, hip_ctx):  # noqa: F811
    """-hp --vote --runs: haplotype h's files are those of a plain --vote --runs run on the file that holds only its reads"""
    t = hp_inputs
    got = _polish(t, hip_ctx, "runs_hp", ["--runs", "-hp", "--edits"], "tagged.bam", "ref.fa", want_runs=3)
    assert list(got) == ["_pepper_polished_hp1.edits.vcf.gz", "_pepper_polished_hp1.fa", "_pepper_polished_hp2.edits.vcf.gz",
                         "_pepper_polished_hp2.fa"]
    for h in (1, 2):
        want = _polish(t, hip_ctx, "runs_split%d" % h, ["--runs", "--edits"], "split%d.bam" % h, "ref.fa", want_runs=3)
        assert got["_pepper_polished_hp%d.fa" % h] == want["_pepper_polished.fa"], h
        mine = [l for l in got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode().split("\n") if not l.startswith("##")]
        assert mine == [l for l in want["_pepper_polished.edits.vcf.gz"].decode().split("\n") if not l.startswith("##")], h
    assert got["_pepper_polished_hp1.fa"] != got["_pepper_polished_hp2.fa"]


# ---- 6. ordinary data ---------------------------------------------------------------------------------------------------------------

def test_on_reads_with_ordinary_run_length_noise_the_run_vote_makes_no_more_errors(tmp_path, hip_ctx):
    """a random truth (its natural runs, adjacent ones and runs at region boundaries included); a draft with a few wrong bases and
    a few runs one off; 20 reads of the truth in which every stretch of two letters or more is one longer or one shorter at a
    rate of 30 %, independently, resampled until the truth is each stretch's most frequent length. Nothing is promised but
    that --runs is no worse than the column vote alone. Measured on an MI355X: 1 error either way (the same hp_del); 154 of the
    185 candidates decided, 31 skipped as adjacent."""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    rng = np.random.default_rng(83)
    T = "".join(rng.choice(list(BASES), size=3300))
    st = [(s, n, b) for s, n, b in rr.stretches(T.encode()) if n >= 2 and s > 0 and s + n < len(T)]
    # the draft, and for every truth stretch where it lies in the draft and how long it is there
    d, shift, where = [], 0, {}
    wrong_runs = set(rng.choice(len(st), size=14, replace=False).tolist())
    at = {s: (k, n) for k, (s, n, b) in enumerate(st)}
    i = 0
    while i < len(T):
        if i in at:
            k, n = at[i]
            nd = n + (int(rng.choice([-1, 1])) if k in wrong_runs and n >= 3 else 0)
            where[k] = (len(d), nd)
            d += [T[i]] * nd
            i += n
        else:
            d.append(T[i])
            i += 1
    D = "".join(d)
    wrong = {}                                                   # draft offset -> the wrong base the draft holds there
    for p in rng.choice(np.arange(50, len(D) - 50), size=40, replace=False).tolist():
        free = [b for b in BASES if b not in (D[p - 1], D[p], D[p + 1])]
        if D[p - 1] != D[p] != D[p + 1] and free and len(wrong) < 12 and not any(abs(p - q) < 3 for q in wrong):
            wrong[p] = free[0]
    draft = "".join(wrong.get(p, c) for p, c in enumerate(D))
    lengths = {}
    for k, (s, n, b) in enumerate(st):
        while True:
            ln = [n + (int(rng.choice([-1, 1])) if rng.random() < 0.30 else 0) for _ in range(20)]
            if all(ln.count(n) > ln.count(x) for x in (n - 1, n + 1)):
                break
        lengths[k] = ln
    recs = []
    for i in range(20):
        ed = {p: ("sub", D[p]) for p in wrong}
        for k, (s, n, b) in enumerate(st):
            ds, nd = where[k]
            ed.update(rc.run_edits(ds, nd, b, lengths[k][i], int(rng.integers(ds, ds + nd))))
        recs.append(rc.bam_record(draft, 0, 0, len(D), ed, 16 * (i % 2), "n%d" % i))
    assert len(wrong) >= 8 and draft != T
    bw.write_fasta(str(tmp_path / "draft.fa"), [("ctg", draft)])
    bw.write_bam(str(tmp_path / "reads.bam"), [("ctg", len(D))], recs)
    truth = [type("T", (), dict(name="ctg", T=T))]
    alone = _fasta(_polish(tmp_path, hip_ctx, "alone", [])["_pepper_polished.fa"])
    runs = _fasta(_polish(tmp_path, hip_ctx, "runs", ["--runs"], want_runs=3)["_pepper_polished.fa"])
    e0, e1 = _errors(hip_ctx, alone, truth), _errors(hip_ctx, runs, truth)
    n0, n1 = (e["sub"] + e["ins"] + e["del"] for e in (e0, e1))
    print("errors against the truth: --vote %d (hp_ins %d, hp_del %d), --vote --runs %d (hp_ins %d, hp_del %d)"
          % (n0, e0["hp_ins"], e0["hp_del"], n1, e1["hp_ins"], e1["hp_del"]))
    assert n1 <= n0
