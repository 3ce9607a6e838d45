"""GPU: `polish --vote`: pv_polish_vote[_dev] against the host checker (tests/vote_ref.py) on hand-made chunk layouts
(tests/min_qual_cases.py; seq_length 40, overlap 10, and the real 1000 / 50 once) with planted counts planes, every tie row of
the CPU list at the edges of a chunk, the error statuses, the identity with the row qualities, the stitch, the edits, their
evidence and the support filter, the same calls as one captured graph, and the command end to end against a known true
sequence: the first test here that asks whether the polished sequence is the right one. Device form = host form = checker,
row for row, bit for bit. Nothing here has a tolerance."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import edits_ref as er
import min_qual_cases as mc
import min_support_ref as ms
import qual_ref as qr
import vote_cases as vc
import vote_ref as vr
from pepper_thesis_amd import _ffi, bamio, cli, polish, polish_edits as pe
from pepper_thesis_amd.device import DevicePolishOut
from test_polish_hp_gpu import inputs as hp_inputs         # the tagged BAM and its two pre-split files

pytestmark = pytest.mark.gpu
L, O = 40, 10
MARK, ACC_MARK = 0xEE, -7.5


# ---- planes and calls ----------------------------------------------------------------------------------------------------------

def _host_out(lay, counts, depth, chunk_id=None, position=None):
    return types.SimpleNamespace(position=lay.position if position is None else position, index=lay.index, region=lay.region,
                                 chunk_id=lay.chunk_id if chunk_id is None else chunk_id, depth=depth, counts=counts)


def _device_chunks(lay, counts, depth, chunk_id=None, position=None, planes=(True, True)):
    do = DevicePolishOut(max(lay.n, 1), lay.L, lay.O, depth=planes[0], counts=planes[1])
    given = {"chunk_id": chunk_id, "position": position}
    for name in ("position", "index", "region", "chunk_id"):
        a = np.array(getattr(lay, name) if given.get(name) is None else given[name])
        getattr(do, name)[:lay.n].copy_(torch.from_numpy(a))
    if planes[0]:
        do.set_depth(np.array(depth))
    if planes[1]:
        do.set_row_counts(np.array(counts))
    return do


def _dev_vote(ctx, lay, counts, depth, want_acc=True, ref=True, chunk_id=None, position=None, planes=(True, True), overlap=None,
              n=None):
    """the device-resident form on uploaded copies, every output pre-filled with a marker -> (labels, acc, d_counts), with the
    error code of the call in front when it was refused. want_acc False: acc is not passed, and comes back as it was."""
    do = _device_chunks(lay, counts, depth, chunk_id, position, planes)
    if overlap is not None:
        do.seq_overlap = overlap
    n = lay.n if n is None else n
    lab = torch.full((max(lay.n, 1), lay.L), MARK, dtype=torch.uint8, device="cuda")
    acc = torch.full((max(lay.n, 1), lay.L, 5), ACC_MARK, dtype=torch.float32, device="cuda")
    rs, ro, d_ref = (torch.from_numpy(np.array(a)).cuda() for a in (lay.ref_start, lay.ref_off, lay.ref))
    cnt = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code = None
    try:
        ctx.polish_vote_dev(do, n, rs.data_ptr(), ro.data_ptr(), d_ref.data_ptr() if ref else 0, lay.n_regions, lab.data_ptr(),
                            acc.data_ptr() if want_acc else 0, cnt.data_ptr())
    except _ffi.PepperHipError as e:
        code = e.code
    ctx.synchronize()
    res = (lab.cpu().numpy()[:lay.n], acc.cpu().numpy()[:lay.n], cnt.cpu().numpy().tolist())
    return res if code is None else (code,) + res


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(ctx, lay, counts, depth):
    """the device form with and without acc and the host form with and without acc against the checker -> the checker's
    (labels, acc, changed, no reads)"""
    want_lab, want_acc, changed, no_reads = vr.vote(counts, depth, *lay.args()[:4], lay.ref_start, lay.ref_off, lay.ref, lay.O)
    lab, acc, cnt = _dev_vote(ctx, lay, counts, depth)
    assert cnt == [changed, 0, -1, no_reads]
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(acc), _bits(want_acc))
    lab, acc, cnt = _dev_vote(ctx, lay, counts, depth, want_acc=False)
    assert cnt == [changed, 0, -1, no_reads] and np.array_equal(lab, want_lab)
    assert (acc == ACC_MARK).all()                                   # acc == NULL: a marker-filled buffer stays as it was
    out = _host_out(lay, counts, depth)
    c = (C.c_int64 * 4)()
    h_lab, h_acc = ctx.polish_vote(out, lay.batch, lay.L, lay.O, want_acc=True, counts=c)
    assert list(c) == [changed, 0, -1, no_reads]
    assert np.array_equal(h_lab, want_lab) and np.array_equal(_bits(h_acc), _bits(want_acc))
    c = (C.c_int64 * 4)()
    assert np.array_equal(ctx.polish_vote(out, lay.batch, lay.L, lay.O, counts=c), want_lab) and list(c) == [changed, 0, -1, no_reads]
    # the copies of a row two chunks share agree
    top = int(lay.position.max()) + 1
    key = ((np.broadcast_to(lay.region[:, None], lay.position.shape) * top + lay.position) * 8 + lay.index)[lay.position >= 0]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    flat = want_lab[lay.position >= 0][order]
    assert same.any() and np.array_equal(flat[1:][same], flat[:-1][same])
    return want_lab, want_acc, changed, no_reads


def _layout(seed, regions, L_=L, O_=O, other=0.02):
    """regions: [(start, columns, insert sites)]; drafts of ACGT / acgt with a few bytes no label spells"""
    rng = np.random.default_rng(seed)
    regs = []
    for start, cols, n_ins in regions:
        d = bytearray(mc.acgt(rng, cols))
        for i in np.flatnonzero(rng.random(cols) < other):
            d[i] = b"NnRy"[i % 4]
        sites = rng.choice(cols, size=min(n_ins, cols), replace=False)
        regs.append((start, bytes(d), {start + int(p): int(rng.integers(1, 4)) for p in sites}))
    return mc.Layout(regs, L_, O_), rng


# ---- 1. the forms agree ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_layouts(hip_ctx, seed):
    lay, rng = _layout(seed, [(0, 95 + 7 * seed, 6), (300, 41, 2), (1000, 230, 12), (5000, 11, 1)])
    counts, depth = vc.random_planes(lay, rng)
    lab, acc, changed, no_reads = _check(hip_ctx, lay, counts, depth)
    assert changed > 20 and no_reads > 0 and len(set(lab.ravel().tolist())) == 5


def test_the_real_chunk_geometry(hip_ctx):
    """seq_length 1000, overlap 50: four rounds of 256 rows in the write pass, the last of 232"""
    lay, rng = _layout(5, [(0, 2300, 40), (7000, 700, 10)], 1000, 50)
    counts, depth = vc.random_planes(lay, rng)
    assert lay.n >= 4
    _check(hip_ctx, lay, counts, depth)


def test_counts_at_65535(hip_ctx):
    """every count and depth at the top of its range: sums of two stay exact in 32 bits and as floats (below 2^24)"""
    lay, rng = _layout(7, [(0, 130, 8)])
    counts, depth = vc.random_planes(lay, rng)
    live = lay.position >= 0
    counts[live] = np.where(vc.keyed(lay, lambda m: rng.random(m) < 0.5)[live][:, None], 65535, counts[live])
    full = vc.keyed(lay, lambda m: rng.random(m) < 0.3) & live
    counts[full] = 65535
    depth[live & (lay.index > 0)] = 65535
    lab, acc, _, _ = _check(hip_ctx, lay, counts, depth)
    assert acc[full & (lay.index == 0)].max() <= 2.0 and (lab[full & (lay.index == 0)] >= 1).all()


def test_a_few_thousand_chunks(hip_ctx):
    """more chunks than the finish block has threads"""
    lay, rng = _layout(9, [(1000 * g, 29 * 60 + 40, 0) for g in range(50)])
    assert lay.n == 50 * 59 and lay.n > 2048
    counts, depth = vc.random_planes(lay, rng, top=12)
    _check(hip_ctx, lay, counts, depth)


# ---- 2. every tie row, at the edges of a chunk -------------------------------------------------------------------------------------

def test_every_tie_row_at_the_first_and_last_row_of_a_chunk_and_on_a_shared_row(hip_ctx):
    """rows 0 (first of chunk 0), 30 (first of chunk 1, shared), 39 (last of chunk 0, shared), 51 (inside) and 99 (last of the
    last chunk) of a region of exactly 100 rows hold the case; both copies of a shared row get the same label, the expected one"""
    rng = np.random.default_rng(11)
    spots = (0, 30, 39, 51, 99)
    for name, ten, draft, label, n in vc.BASE_ROWS:
        d = bytearray(mc.acgt(rng, 100))
        for r in spots:
            d[r] = draft[0]
        lay = mc.Layout([(0, bytes(d), {})], L, O)
        assert lay.n == 3 and (lay.position[2] >= 0).all()
        counts, depth = vc.random_planes(lay, rng)
        for r in spots:
            vc.plant(lay, counts, depth, 0, r, ten)
        lab, acc, _, _ = _check(hip_ctx, lay, counts, depth)
        for r in spots:
            at = lay.where(0, r)
            assert len(at[0]) == (2 if r in (30, 39) else 1) and lab[at].tolist() == [label] * len(at[0]), (name, r)
            for kk, jj in zip(*at):                          # the hand-computed reads per label, under the weight of the copy's row
                assert np.array_equal(_bits(acc[kk, jj]), _bits(vr.fractions(np.array([n] * L), O)[jj])), (name, r)
    for name, ten, d_anchor, label, n in vc.INSERT_ROWS:
        lay = mc.Layout([(0, mc.acgt(rng, 95), {28: 2, 36: 1, 47: 1, 94: 1})], L, O)
        spots = [r for r, (p, x) in enumerate(lay.rows[0]) if x > 0]
        assert spots == [29, 30, 39, 51, 99] and lay.n == 3 and (lay.position[2] >= 0).all()
        counts, depth = vc.random_planes(lay, rng)
        for r in spots:
            vc.plant(lay, counts, depth, 0, r, ten, d_anchor)
        lab, acc, _, _ = _check(hip_ctx, lay, counts, depth)
        for r in spots:
            at = lay.where(0, r)
            assert len(at[0]) == (2 if r in (30, 39) else 1) and lab[at].tolist() == [label] * len(at[0]), (name, r)


# ---- 3. error paths ---------------------------------------------------------------------------------------------------------------

def test_a_broken_layout_leaves_everything_but_the_counts(hip_ctx):
    lay, rng = _layout(13, [(0, 100, 4), (400, 100, 3)])
    counts, depth = vc.random_planes(lay, rng)
    cid = lay.chunk_id.copy()
    cid[2] = 5                                               # chunk ids 0, 1, 5 inside region 0
    pos = lay.position.copy()
    k = int(np.flatnonzero(lay.region == 1)[1])
    j = int(np.flatnonzero(lay.index[k] == 0)[3])
    pos[k, j] = 400 + 100                                    # one past the last draft byte of region 1
    low = lay.position.copy()
    low[k, j] = 399                                          # one below the first draft byte of region 1
    for kw, bad in ((dict(chunk_id=cid), 2), (dict(position=pos), k), (dict(position=low), k)):
        with pytest.raises(vr.BadChunk) as e:
            vr.vote(counts, depth, kw.get("position", lay.position), lay.index, lay.region, kw.get("chunk_id", lay.chunk_id),
                    lay.ref_start, lay.ref_off, lay.ref, O)
        assert e.value.chunk == bad
        lab, acc, cnt = _dev_vote(hip_ctx, lay, counts, depth, **kw)
        assert cnt == [0, _ffi.PV_ERR_INVALID, bad, 0], kw.keys()
        assert (lab == MARK).all() and (acc == ACC_MARK).all()
        c = (C.c_int64 * 4)()
        h_lab, h_acc = np.full(lay.position.shape, MARK, np.uint8), np.full(lay.position.shape + (5,), ACC_MARK, np.float32)
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_vote(_host_out(lay, counts, depth, **kw), lay.batch, L, O, counts=c, labels=h_lab, acc=h_acc)
        assert e.value.code == _ffi.PV_ERR_INVALID and list(c) == [0, _ffi.PV_ERR_INVALID, bad, 0] and "chunk %d" % bad in str(e.value)
        assert (h_lab == MARK).all() and (h_acc == ACC_MARK).all()


def test_what_the_call_itself_refuses(hip_ctx):
    lay, rng = _layout(15, [(0, 100, 4)])
    counts, depth = vc.random_planes(lay, rng)
    for kw in (dict(planes=(False, True)), dict(planes=(True, False)), dict(ref=False), dict(overlap=L // 2 + 1)):
        code, lab, acc, cnt = _dev_vote(hip_ctx, lay, counts, depth, **kw)
        assert code == _ffi.PV_ERR_INVALID and cnt == [-7] * 4 and (lab == MARK).all() and (acc == ACC_MARK).all(), kw
    no_ref = types.SimpleNamespace(ref_start=lay.ref_start, ref_off=lay.ref_off, ref=None)
    for out, batch, o in ((_host_out(lay, None, depth), lay.batch, O), (_host_out(lay, counts, None), lay.batch, O),
                          (_host_out(lay, counts, depth), no_ref, O), (_host_out(lay, counts, depth), lay.batch, L // 2 + 1)):
        c = (C.c_int64 * 4)()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_vote(out, batch, L, o, want_acc=True, counts=c)
        assert e.value.code == _ffi.PV_ERR_INVALID and list(c) == [0] * 4
    # the largest overlap that is allowed passes
    lay2 = mc.Layout([(0, mc.acgt(rng, 100), {})], L, L // 2)
    _check(hip_ctx, lay2, *vc.random_planes(lay2, rng))


def test_no_chunks(hip_ctx):
    lay, rng = _layout(17, [(0, 100, 4)])
    counts, depth = vc.random_planes(lay, rng)
    lab, acc, cnt = _dev_vote(hip_ctx, lay, counts, depth, n=0)
    assert cnt == [0, 0, -1, 0] and (lab == MARK).all() and (acc == ACC_MARK).all()
    none = types.SimpleNamespace(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32), region=np.zeros(0, np.int32),
                                 chunk_id=np.zeros(0, np.int32), depth=np.zeros((0, L), np.uint16), counts=np.zeros((0, L, 10), np.uint16))
    c = (C.c_int64 * 4)()
    h_lab, h_acc = hip_ctx.polish_vote(none, lay.batch, L, O, want_acc=True, counts=c)
    assert h_lab.shape == (0, L) and h_acc.shape == (0, L, 5) and list(c) == [0, 0, -1, 0]


# ---- 4. identity with the chain, eager and as one graph ------------------------------------------------------------------------------

def test_vote_row_qual_stitch_and_evidence_agree_and_replay_as_one_graph(hip_ctx):
    lay, rng = _layout(19, [(0, 380, 20), (500, 300, 5)])
    n, G = lay.n, lay.n_regions
    fills = [vc.random_planes(lay, np.random.default_rng(80 + s)) for s in range(3)]
    do = _device_chunks(lay, *fills[0])
    rs, ro, ref = (torch.from_numpy(np.array(a)).cuda() for a in (lay.ref_start, lay.ref_off, lay.ref))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq, qual = (torch.zeros(n * L, dtype=torch.uint8, device="cuda") for _ in range(2))
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    evb = torch.zeros((n * L, 8), dtype=torch.uint8, device="cuda")
    roff, eoff = (torch.zeros(G + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    c_vt, c_rq, c_su, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(5))
    st = hip_ctx.stream
    common = (rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G)

    def passes():
        hip_ctx.polish_vote_dev(do, n, *common, lab_d.data_ptr(), acc_d.data_ptr(), c_vt.data_ptr(), stream=st)
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_rq.data_ptr(), L, O, stream=st)
        hip_ctx.polish_filter_low_support_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, 1, lab_d.data_ptr(), rq_d.data_ptr(),
                                              c_su.data_ptr(), stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), G, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_evidence_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), *common, eoff.data_ptr(), buf.data_ptr(),
                                          evb.data_ptr(), n * L, c_ed.data_ptr(), stream=st)

    def state():
        t, e = int(c_st[0].item()), int(c_ed[0].item())
        return (lab_d.cpu().numpy().tobytes(), acc_d.cpu().numpy().tobytes(), rq_d.cpu().numpy().tobytes(),
                seq[:t].cpu().numpy().tobytes(), qual[:t].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(),
                evb[:e].cpu().numpy().tobytes(), roff.cpu().numpy().tolist(), eoff.cpu().numpy().tolist(), c_vt.cpu().numpy().tolist(),
                c_su.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(), c_ed.cpu().numpy().tolist())

    def refill(k):
        do.set_row_counts(np.array(fills[k][0]))
        do.set_depth(np.array(fills[k][1]))
        for t in (lab_d, acc_d, rq_d, seq, qual, buf, evb, roff, eoff, c_vt, c_rq, c_su, c_st, c_ed):
            t.zero_()
        torch.cuda.synchronize()

    eager = []
    for k, (counts, depth) in enumerate(fills):
        refill(k)
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        want_lab, want_acc, changed, no_reads, reads = vr.vote(counts, depth, *lay.args()[:4], lay.ref_start, lay.ref_off, lay.ref, O,
                                                               want_reads=True)
        want_q = qr.row_qual(want_lab, want_acc, O)
        assert eager[-1][0] == want_lab.tobytes() and eager[-1][1] == want_acc.tobytes() and eager[-1][2] == want_q.tobytes()
        assert eager[-1][9] == [changed, 0, -1, no_reads] and changed > 50
        # the quality is the Phred value of the fraction of reads that disagree with the winner; no reads: 0; all agree: 93
        live = lay.position >= 0
        won = np.take_along_axis(reads, want_lab[..., None].astype(np.int64), -1)[..., 0]
        total = reads.sum(-1)
        assert (want_q[live & (total == 0)] == 0).all() and (want_q[live & (total > 0) & (won == total)] == 93).all()
        assert (live & (total > 0) & (won == total)).any() and (want_q[live & (won < total)] < 93).all()
        # no edit of a vote is without a read: the support filter at 1 takes nothing back (a column without reads over a draft
        # byte no label spells is pinned)
        assert eager[-1][10][:3] == [0, 0, -1]
        assert ms.filter_low_support(want_lab, want_q, counts, depth, *lay.args(), 1)[2] == 0
        h_roff, h_seq, h_qual = hip_ctx.polish_stitch_qual(lay.out, want_lab, want_q, lay.ref_start, seq_length=L, seq_overlap=O)
        assert (eager[-1][3], eager[-1][4], eager[-1][7]) == (h_seq, h_qual, h_roff.tolist())
        h_eoff, h_ed, h_ev = hip_ctx.polish_edits_evidence(_host_out(lay, counts, depth), want_lab, lay.batch, row_qual=want_q,
                                                           seq_length=L, seq_overlap=O)
        assert (eager[-1][5], eager[-1][6], eager[-1][8]) == (h_ed.tobytes(), h_ev.tobytes(), h_eoff.tolist()) and len(h_ed) > 50
        # every record's alt_fwd + alt_rev is the winner's n
        g_of = np.searchsorted(h_eoff, np.arange(len(h_ed)), "right") - 1
        for i in range(len(h_ed)):
            at = np.nonzero((lay.position == h_ed["position"][i]) & (lay.index == h_ed["index"][i]) & (lay.region == g_of[i])[:, None])
            kk, jj = int(at[0][0]), int(at[1][0])
            assert int(h_ev["alt_fwd"][i]) + int(h_ev["alt_rev"][i]) == reads[kk, jj, want_lab[kk, jj]], i
    assert eager[0][3] != eager[1][3]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        refill(k)
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 5. truth recovery end to end -------------------------------------------------------------------------------------------------

def _other(rng, b):
    return "ACGT"[("ACGT".index(b) + int(rng.integers(1, 4))) % 4]


class _Truth:
    """a true sequence T, a draft D made from it by planted edits, and the alignment of the two as a list of columns
    (t base or None, d base or None); reads are slices of it. boundary: draft columns at a region boundary that carry a
    substitution. The regions of a contig are [0, 1100], [900, 2100], [1900, 3100], ... and region g > 0 keeps the columns
    above its start + 200, so the stitch changes regions between columns 1100 and 1101. The shared inputs plant column 1101,
    the first column region 1 keeps. Column 1100, the last column of region 0, is planted in a file of its own
    (test_a_substitution_in_a_regions_last_column): --realign clips every read to its region and then aligns it locally, and
    a local alignment drops a mismatching last base (-6) from every read there, so under --realign no read shows that
    substitution, whatever turns the pileup into labels: with column 1100 planted in the shared inputs, the --realign run
    differed from T in exactly that one base of each contig and counted the column among the rows without reads."""

    def __init__(self, rng, length, name, boundary=(1101,)):
        self.name = name
        t = list(rng.choice(list("ACGT"), size=length))
        self.homo = (400, 2600)                            # two homopolymer runs of seven, one for an indel each
        for h in self.homo:
            t[h:h + 7] = t[h] * 7
            t[h - 1] = _other(rng, t[h])
            t[h + 7] = _other(rng, t[h])
        self.T = "".join(t)
        sites = {}                                         # T index -> (kind, size)
        kinds = ["sub", "ins", "del", "sub", "del", "ins"]
        i, k = 60, 0
        while i < length - 150:
            if not any(abs(i - h) < 40 for h in self.homo) and not any(abs(i - b) < 60 for b in boundary):
                sites[i] = (kinds[k % 6], 1 + (k // 6) % 3)
                k += 1
            i += 130 + int(rng.integers(0, 40))
        sites[self.homo[0] + 3] = ("ins", 1)               # the draft lacks one base of the run
        sites[self.homo[1] + 3] = ("del", 1)               # the draft holds one base too many
        self.aln, self.subs = [], []                       # subs: (T index, D column) of the planted substitutions
        d_col, i = 0, 0
        while i < length:
            kind, size = sites.get(i, ("", 0))
            if kind == "ins":                              # the polisher must insert T[i:i+size]: the draft lacks them
                for j in range(size):
                    self.aln.append((self.T[i + j], None))
                i += size
                continue
            if kind == "sub" or (d_col in boundary and not kind):   # the region boundary columns carry a substitution too
                self.subs.append((i, d_col))
                self.aln.append((self.T[i], _other(rng, self.T[i])))
            else:
                self.aln.append((self.T[i], self.T[i]))
            d_col += 1
            if kind == "del":                              # the polisher must delete: the draft holds `size` bases too many
                extra = self.T[i] * size if i - 3 in self.homo else "".join(rng.choice(list("ACGT"), size=size))
                for b in extra:
                    self.aln.append((None, b))
                    d_col += 1
            i += 1
        d = [b for _, b in self.aln if b is not None]
        for a in range(min(3000, len(d)), min(3300, len(d))):   # a lower-case stretch over several edits
            d[a] = d[a].lower()
        self.D = "".join(d)
        self.t_at = np.cumsum([t is not None for t, _ in self.aln]) - 1      # T index of every alignment column (of the last t base)
        self.d_at = np.cumsum([b is not None for _, b in self.aln]) - 1      # D column of every alignment column
        self.a_of_t = np.flatnonzero([t is not None for t, _ in self.aln])   # alignment column of every T index
        self.edited = np.array([t is None or b is None or t != b for t, b in self.aln])
        assert all(any(dc == b for _, dc in self.subs) for b in boundary) and len(sites) > 15

    def clean(self, t, step):
        """the nearest T index from t in direction step whose 15 alignment columns on either side hold no edit"""
        while True:
            a = int(self.a_of_t[t])
            if not self.edited[max(0, a - 15):a + 16].any():
                return t
            t += step

    def read_spans(self, rng, depth=20):
        """[(T start, T end)] of reads 800-2500 long, `depth` tilings of T: the first starts at 0 and its last read ends at the
        end of T; no read begins or ends beside an edit"""
        n, spans = len(self.T), []
        for p in range(depth):
            s = 0 if p == 0 else -int(rng.integers(0, 800))
            while s < n - 60:
                e = s + int(rng.integers(800, 2501))
                if p == 0 and n - e < 800:
                    e = n
                a, b = (0 if s <= 0 else self.clean(s, 1)), (n if e >= n else self.clean(e, -1))
                if b - a >= 400:
                    spans.append((a, b))
                s = e
        assert spans[0][0] == 0 and any(b == n for _, b in spans)
        return spans

    def columns(self, a, b):
        """the alignment columns of the read T[a:b] as a list of [t base or None, d base or None, alignment column]"""
        lo, hi = int(self.a_of_t[a]), int(self.a_of_t[b - 1])
        return [[t, d, lo + i] for i, (t, d) in enumerate(self.aln[lo:hi + 1])]


def _record(truth, tid, cols, flag, name):
    """alignment columns -> a BAM record; a column [None, d, _] is a deleted draft column, [t, None, _] an inserted base"""
    while cols and (cols[0][0] is None or cols[0][1] is None):
        cols = cols[1:]
    while cols and (cols[-1][0] is None or cols[-1][1] is None):
        cols = cols[:-1]
    if len(cols) < 30:
        return None
    cigar = []
    for t, d, _ in cols:
        op = 0 if t is not None and d is not None else 1 if d is None else 2
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += 1
        else:
            cigar.append([op, 1])
    seq = "".join(t for t, _, _ in cols if t is not None)
    return dict(tid=tid, pos=int(truth.d_at[cols[0][2]]), mapq=60, flag=flag, cigar=[(o, l) for o, l in cigar], seq=seq,
                qual=[30] * len(seq), name=name, hp=None)


def _write_bam(path, truths, spans, edit=None):
    """edit(truth, i, cols) -> the read's parts as lists of columns (default: the read as it is)"""
    import bam_writer as bw
    recs = []
    for tid, (truth, sp) in enumerate(zip(truths, spans)):
        for i, (a, b) in enumerate(sp):
            cols = truth.columns(a, b)
            for part, c in enumerate([cols] if edit is None else edit(truth, i, cols)):
                r = _record(truth, tid, c, 16 * (i % 2), "r%d_%d_%d" % (tid, i, part))
                if r is not None:
                    recs.append(r)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(path, [(t.name, len(t.D)) for t in truths], recs)


NOISE_AT, HOLE_SUB = 4200, 5     # contig 0: the D column where the noisy window starts; the planted substitution under the hole


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("vote_truth")
    rng = np.random.default_rng(61)
    truths = [_Truth(rng, 6_100, "ctgA"), _Truth(rng, 5_700, "ctgB")]
    bw.write_fasta(str(tmp / "draft.fa"), [(t.name, t.D) for t in truths])
    spans = [t.read_spans(rng) for t in truths]
    _write_bam(str(tmp / "clean.bam"), truths, spans)
    # a third of the reads wrong in one 60-column window of contig 0 that holds no planted edit: every fourth column another base,
    # one column deleted
    t0 = truths[0]
    w0 = next(c for c in range(NOISE_AT, NOISE_AT + 400) if not t0.edited[np.flatnonzero(t0.d_at == c)[0] - 5:][:75].any())

    def noisy(tr, i, cols):
        if tr is not t0 or i % 3:
            return [cols]
        out = []
        for t, d, a in cols:
            c = int(tr.d_at[a])
            if w0 <= c < w0 + 60 and t is not None and d is not None:
                if c == w0 + 30:
                    t = None                                # a spurious deletion
                elif (c - w0) % 4 == 0:
                    t = "ACGT"[("ACGT".index(t) + 1) % 4]   # a wrong base
            out.append([t, d, a])
        return [out]
    _write_bam(str(tmp / "noisy.bam"), truths, spans, noisy)
    # no read over the 50 draft columns around one planted substitution of contig 0
    sub_t, sub_d = t0.subs[HOLE_SUB]
    assert 1200 < sub_d < 5000

    def holed(tr, i, cols):
        if tr is not t0:
            return [cols]
        left = [c for c in cols if tr.d_at[c[2]] < sub_d - 25]
        right = [c for c in cols if tr.d_at[c[2]] >= sub_d + 25]
        return [left, right]
    _write_bam(str(tmp / "hole.bam"), truths, spans, holed)
    kept = t0.T[:sub_t] + t0.D[sub_d].upper() + t0.T[sub_t + 1:]
    return tmp, truths, {"w0": w0, "hole": (sub_d - 25, sub_d + 25), "hole_fasta": kept}


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back the planes every launch voted on and what it left"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        res = super()._labels_and_stitch(db, n, n_regions)
        if n:
            d = self.dout
            self.launches.append(dict(
                position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(), region=d.region[:n].cpu().numpy(),
                chunk_id=d.chunk_id[:n].cpu().numpy(), labels=self.labels[:n].cpu().numpy(), depth=d.depth_numpy(n),
                counts=d.row_counts_numpy(n), row_qual=self.row_qual[:n].cpu().numpy() if self.row_qual is not None else None,
                ref_start=db.t["ref_start"][:n_regions].cpu().numpy(), ref_off=db.t["ref_off"][:n_regions + 1].cpu().numpy(),
                ref=db.t["ref"].cpu().numpy(), voted=res.voted))
        return res


def _vote(t, hip_ctx, name, flags, bam, chains=None, fasta="draft.fa", bs="8"):
    """`polish --vote` with no -m, on the session's context, which may hold no weights at all"""
    out_dir = str(t / name)
    argv = ["-b", str(t / bam), "-f", str(t / fasta), "-t", "3", "-bs", bs, "-o", out_dir, "--vote"] + flags

    def open_chain(device, shared, state_dict, dtype, **k):
        assert state_dict is None and k.get("vote") is True
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


def _diff(got: str, want: str):
    """the first places where two sequences of one length differ, with what stands there"""
    return [(i, got[i], want[i]) for i in range(min(len(got), len(want))) if got[i] != want[i]][:20]


def _log_counts(err):
    m = re.search(r"VOTE: (\d+) CHUNK ROWS WHERE THE READS' MAJORITY IS NOT THE DRAFT, (\d+) BASE ROWS WITHOUT READS", err)
    assert m, err
    return int(m.group(1)), int(m.group(2))


def test_the_vote_recovers_the_true_sequence(truth, hip_ctx, capsys):
    """error-free reads of T aligned to a draft with planted substitutions, insertions and deletions (in homopolymers, at a
    region's last column, under lower case): `polish --vote` with no model gives T, its edits applied to the draft give T, and
    every edit has a read behind it. The checker alone, on the planes of every launch, gives the labels the device gave."""
    t, truths, _ = truth
    chains = []
    got = _vote(t, hip_ctx, "clean", ["--edits", "--evidence"], "clean.bam", chains)
    changed, no_reads = _log_counts(capsys.readouterr().err)
    assert list(got) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.fa"]
    launches = chains[0].launches
    assert len(launches) > 2 and chains[0].vote and not chains[0].qualities
    for la in launches:
        lab, _, ch, nr = vr.vote(la["counts"], la["depth"], la["position"], la["index"], la["region"], la["chunk_id"], la["ref_start"],
                                 la["ref_off"], la["ref"], 50, want_acc=False)
        assert np.array_equal(lab, la["labels"]) and la["voted"] == (ch, nr)
    assert (changed, no_reads) == (sum(la["voted"][0] for la in launches), 0) and changed > 60
    fasta = _fasta(got["_pepper_polished.fa"])
    assert fasta == {tr.name: tr.T for tr in truths}
    text = got["_pepper_polished.edits.vcf.gz"].decode()
    header = [l[2:] for l in text.split("\n") if l.startswith("##")]
    assert [h for h in header if h.startswith("pepper_")] == ["pepper_consensus=vote"]
    info = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    for tr in truths:
        mine = [(int(f[1]), f[3], f[4], None if f[5] == "." else int(f[5])) for f in info if f[0] == tr.name]
        assert len(mine) > 30 and er.apply(mine, tr.D.encode()) == tr.T, tr.name
    ad = [int(f[7].split(";")[1].split(",")[1]) for f in info]
    assert all(f[7].split(";")[1].startswith("AD=") for f in info) and min(ad) >= 1


def test_a_third_of_the_reads_wrong_in_a_window_changes_nothing(truth, hip_ctx, capsys):
    t, truths, at = truth
    chains = []
    got = _vote(t, hip_ctx, "noisy", ["--qualities"], "noisy.bam", chains)
    assert _fasta(got["_pepper_polished.fa"]) == {tr.name: tr.T for tr in truths}
    # the window was seen: some of its rows hold reads that disagree with the winner, and their quality is below the ceiling
    low = 0
    for la in chains[0].launches:
        inside = (la["position"] >= at["w0"]) & (la["position"] < at["w0"] + 60) & (la["index"] == 0)   # (of either contig)
        low += int((la["row_qual"][inside] < 93).sum())
    assert low >= 15
    assert _log_counts(capsys.readouterr().err)[1] == 0


def test_a_coverage_hole_keeps_the_draft_and_is_counted(truth, hip_ctx, capsys):
    t, truths, at = truth
    got = _vote(t, hip_ctx, "hole", [], "hole.bam")
    fasta = _fasta(got["_pepper_polished.fa"])
    assert fasta[truths[1].name] == truths[1].T
    assert fasta[truths[0].name] == at["hole_fasta"] and at["hole_fasta"] != truths[0].T
    assert 50 <= _log_counts(capsys.readouterr().err)[1] <= 100          # the hole's 50 rows, once more where two chunks share them


def test_gpu_decode_realign_and_qualities_give_the_same_sequence(truth, hip_ctx):
    """the device read path and the realigner in front of the vote: the same FASTA, and quality 93 wherever all reads of a row agree"""
    t, truths, _ = truth
    chains = []
    got = _vote(t, hip_ctx, "all", ["--gpu_decode", "--realign", "--qualities"], "clean.bam", chains)
    assert list(got) == ["_pepper_polished.fa", "_pepper_polished.fq"]
    fasta = _fasta(got["_pepper_polished.fa"])
    for tr in truths:
        assert len(fasta[tr.name]) == len(tr.T) and _diff(fasta[tr.name], tr.T) == [], tr.name
    fq = got["_pepper_polished.fq"].decode().split("\n")
    assert fq[0::4][:2] == ["@" + tr.name for tr in truths] and fq[1::4] == [tr.T for tr in truths]
    rows = agree = 0
    for la in chains[0].launches:
        lab, acc, _, _, reads = vr.vote(la["counts"], la["depth"], la["position"], la["index"], la["region"], la["chunk_id"],
                                        la["ref_start"], la["ref_off"], la["ref"], 50, want_reads=True)
        assert np.array_equal(lab, la["labels"]) and np.array_equal(la["row_qual"], qr.row_qual(lab, acc, 50))
        total, won = reads.sum(-1), np.take_along_axis(reads, lab[..., None].astype(np.int64), -1)[..., 0]
        same = (la["position"] >= 0) & (total > 0) & (won == total)
        assert (la["row_qual"][same] == 93).all()
        rows, agree = rows + int((la["position"] >= 0).sum()), agree + int(same.sum())
    assert agree > 0.9 * rows
    # where every read of every kept column agrees, the FASTQ says so: nearly all of it is at the ceiling
    q = np.frombuffer("".join(fq[3::4]).encode(), np.uint8) - 33
    assert (q == 93).mean() > 0.9 and q.max() == 93


def test_a_substitution_in_a_regions_last_column(tmp_path, hip_ctx):
    """columns 1100 and 2100, the last of regions 0 and 1 and the last the stitch takes from them: recovered from reads as
    they are aligned in the BAM (see _Truth on why not under --realign)"""
    import bam_writer as bw
    rng = np.random.default_rng(67)
    tr = _Truth(rng, 3_400, "edge", boundary=(1100, 2100))
    bw.write_fasta(str(tmp_path / "draft.fa"), [(tr.name, tr.D)])
    _write_bam(str(tmp_path / "edge.bam"), [tr], [tr.read_spans(rng)])
    got = _vote(tmp_path, hip_ctx, "edge", [], "edge.bam")
    assert _diff(_fasta(got["_pepper_polished.fa"])[tr.name], tr.T) == [] and len(tr.T) == len(_fasta(got["_pepper_polished.fa"])[tr.name])


# ---- 6. -hp -------------------------------------------------------------------------------------------------------------------------

def test_each_haplotype_votes_with_its_own_reads(hp_inputs, hip_ctx):
    """-hp --vote: haplotype h's FASTA is that of a plain --vote run on the file that holds only its reads"""
    t = hp_inputs
    got = _vote(t, hip_ctx, "vote_hp", ["-hp"], "tagged.bam", fasta="ref.fa")
    assert list(got) == ["_pepper_polished_hp1.fa", "_pepper_polished_hp2.fa"]
    for h in (1, 2):
        want = _vote(t, hip_ctx, "vote_split%d" % h, [], "split%d.bam" % h, fasta="ref.fa")
        assert got["_pepper_polished_hp%d.fa" % h] == want["_pepper_polished.fa"], h
    assert got["_pepper_polished_hp1.fa"] != got["_pepper_polished_hp2.fa"]
