"""GPU: the polisher's edit list: pv_polish_edits[_dev] against the host checker (tests/edits_ref.py) record for record, the
identity that ties the records to the stitch, the error statuses, the three passes of --qualities --edits as a captured graph,
and `polish --edits` end to end on a small BAM. Nothing here has a tolerance."""
import ctypes as C
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

import edits_ref as er
from pepper_thesis_amd import _ffi, bamio, cli, polish, synth
from pepper_thesis_amd.batch import Read, Region, pack_regions
from pepper_thesis_amd.device import DevicePolishOut
from pepper_thesis_amd.polish_edits import EDIT_DTYPE

pytestmark = pytest.mark.gpu
L, O = 1000, 50
MARK = 0xEE


def _draft(rng, n, clean=False):
    """random draft bytes: ACGT with lower-case ones; unless clean, also N, n and IUPAC codes in either case"""
    d = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    low = rng.random(n) < 0.2
    d[low] += 32
    if not clean:
        odd = rng.random(n) < 0.08
        d[odd] = rng.choice(np.frombuffer(b"NnRYkMs", np.uint8), int(odd.sum()))
    return d.astype(np.uint8)


def _build_case(ctx, seed):
    """regions of 13 chunks (a 12000-base insert: chunk ids 9 and 10 meet, and one position's insert rows cross eleven chunk
    boundaries), 1 chunk and 2 chunks, the last two with region_start > 0; drafts with lower-case, N and IUPAC bytes; random
    labels with label-0 runs on both sides of every overlap; row qualities that differ between the chunks on shared columns"""
    rng = np.random.default_rng(seed)
    ins = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 12_000))
    regs = [Region(0, 299, b"A" * 300, [Read.make(10, "5M12000I60M", b"C" * 5 + ins + b"G" * 60), Read.make(0, "250M", "A" * 250)]),
            synth.synth_region(300, region_len=400, depth=8, read_len=300, site_every=50, ref_start=5000),
            synth.synth_region(301, region_len=1200, depth=8, read_len=500, site_every=50, ref_start=8000)]
    for r in regs:
        r.ref = _draft(rng, len(r.ref)).tobytes()      # (the builder reads the draft for its length only)
    b = pack_regions(regs)
    out = ctx.polish_summarize(b)
    per_region = [int((out.region == g).sum()) for g in range(3)]
    assert per_region[0] >= 11 and per_region[1] == 1 and per_region[2] == 2, per_region
    n = len(out.chunk_id)
    labels = rng.integers(0, 5, (n, L)).astype(np.uint8)
    rq = rng.integers(0, 94, (n, L)).astype(np.uint8)
    for k in range(1, n):
        if out.region[k] == out.region[k - 1]:
            assert np.array_equal(out.position[k, :O], out.position[k - 1, L - O:]) and np.array_equal(out.index[k, :O], out.index[k - 1, L - O:])
            labels[k - 1, L - O - 10:L - O + 15] = 0
            labels[k, O - 20:O + 10] = 0
            same = rq[k, :O] == rq[k - 1, L - O:]
            rq[k, :O][same] = (rq[k, :O][same] + 1) % 94
    return b, out, labels, rq


@pytest.fixture(scope="module")
def case(hip_ctx):
    """the batch, its chunks, labels and row qualities: shared and left unchanged (tests copy what they alter)"""
    b, out, labels, rq = _build_case(hip_ctx, 5)
    for a in (out.position, out.index, out.region, out.chunk_id, labels, rq, b.ref, b.ref_off, b.ref_start):
        a.setflags(write=False)
    return b, out, labels, rq


def _dicts(b, out, labels, rq=None):
    spans = list(zip(b.ref_start.tolist(), b.ref_end.tolist()))
    return er.region_dicts(out.position, out.index, out.region, out.chunk_id, labels, spans, rq)


def _region_draft(b, g):
    return b.ref[int(b.ref_off[g]):int(b.ref_off[g + 1])].tobytes()


def _expected(b, out, labels, rq=None):
    """the checker's records per region -> (all of them, region offsets)"""
    per = [er.primitive_edits(d, _region_draft(b, g), int(b.ref_start[g])) for g, d in enumerate(_dicts(b, out, labels, rq))]
    return [e for p in per for e in p], np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)


def _dev_edits(ctx, out, labels, rq, b, capacity=None, ref=True, ref_off=None):
    """the device-resident form on uploaded copies, every output pre-filled with a marker -> (region_edit_off, records of
    the whole buffer, the buffer's raw bytes, counts) or the error code the call itself returned"""
    n = len(out.chunk_id)
    do = DevicePolishOut(max(n, 1))
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(np.array(getattr(out, name))))
    lab = torch.from_numpy(np.array(labels)).cuda()
    drq = torch.from_numpy(np.array(rq)).cuda() if rq is not None else None
    rs = torch.from_numpy(np.asarray(b.ref_start, np.int64).copy()).cuda()
    ro = torch.from_numpy(np.asarray(b.ref_off if ref_off is None else ref_off, np.int64).copy()).cuda()
    d_ref = torch.from_numpy(np.array(b.ref)).cuda()          # always as long as the batch's own ref_off says
    cap = n * L if capacity is None else capacity
    buf = torch.full((max(cap, 1), 16), MARK, dtype=torch.uint8, device="cuda")
    eoff = torch.full((len(rs) + 1,), -7, dtype=torch.int64, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ctx.polish_edits_dev(do, n, lab.data_ptr(), drq.data_ptr() if drq is not None else 0, rs.data_ptr(), ro.data_ptr(),
                             d_ref.data_ptr() if ref else 0, len(rs), eoff.data_ptr(), buf.data_ptr(), cap, counts.data_ptr())
    except _ffi.PepperHipError as e:
        return e.code
    ctx.synchronize()
    raw = buf.cpu().numpy()
    return eoff.cpu().numpy(), raw.view(EDIT_DTYPE).reshape(-1), raw, counts.cpu().numpy().tolist()


# ---- 1. checker comparison ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_qual", [False, True])
def test_edits_equal_checker(hip_ctx, case, with_qual):
    b, out, labels, rq = case
    q = rq if with_qual else None
    want, want_off = _expected(b, out, labels, q)
    total = len(want)
    kinds = [e[2] for e in want]
    assert total > 5_000 and all(kinds.count(k) > 100 for k in (er.SUB, er.DEL, er.INS))   # (some 1500 of the columns are draft positions)
    assert any(e[2] == er.SUB and chr(e[3]) in "NnRYkMs" for e in want) and any(e[2] == er.DEL and chr(e[3]) in "acgt" for e in want)
    assert with_qual or all(e[5] == 255 for e in want)
    counts = (C.c_int64 * 4)()
    eoff, recs = hip_ctx.polish_edits(out, labels, b, row_qual=q, counts=counts)
    assert recs.dtype == EDIT_DTYPE and list(counts) == [total, 0, -1, 0]
    assert np.array_equal(eoff, want_off) and recs.tolist() == want
    deoff, drecs, raw, c = _dev_edits(hip_ctx, out, labels, q, b)
    assert c == [total, 0, -1, 0] and np.array_equal(deoff, want_off)
    assert drecs[:total].tolist() == want and (raw[total:] == MARK).all()


# ---- 2. identity with the stitch ----------------------------------------------------------------------------------------

def test_records_rebuild_the_stitch(hip_ctx, case):
    b, out, labels, _ = case
    eoff, recs = hip_ctx.polish_edits(out, labels, b)
    roff, seq = hip_ctx.polish_stitch(out, labels, b.ref_start)
    assert len(seq) > 10_000
    for g, d in enumerate(_dicts(b, out, labels)):
        draft, start = _region_draft(b, g), int(b.ref_start[g])
        mine = recs[eoff[g]:eoff[g + 1]]
        own, tail = {}, {}
        for p, x, kind, _, base, _ in mine.tolist():
            if x == 0:
                own[p] = chr(base) if kind == er.SUB else ""
            else:
                tail[p] = tail.get(p, "") + chr(base)
        got = "".join(own.get(p, er.upper(draft[p - start])) + tail.get(p, "") for p in sorted(p for p, x in d if x == 0))
        assert got.encode() == seq[roff[g]:roff[g + 1]], g
        assert got == er.polished(d, draft, start)


# ---- 3. the winner of a shared column -----------------------------------------------------------------------------------

def test_chunk_9_owns_what_it_shares_with_chunk_10(hip_ctx, case):
    b, out, labels, rq = case
    labels, rq = labels.copy(), rq.copy()
    k9, k10 = (int(np.flatnonzero((out.region == 0) & (out.chunk_id == c_))[0]) for c_ in (9, 10))
    keys = set(zip(out.position[k9, L - O:].tolist(), out.index[k9, L - O:].tolist()))
    assert len(keys) == O and all(x > 0 for _, x in keys)        # insert rows: the draft's code there is 0 (no base)
    labels[k9, L - O:], labels[k10, :O] = 0, 2
    _, recs = hip_ctx.polish_edits(out, labels, b, row_qual=rq)
    assert not [r for r in recs.tolist() if (r[0], r[1]) in keys]
    assert recs.tolist() == _expected(b, out, labels, rq)[0]
    labels[k9, L - O:], labels[k10, :O] = 2, 0
    rq[k9, L - O:], rq[k10, :O] = np.arange(40, 40 + O), 7
    _, recs = hip_ctx.polish_edits(out, labels, b, row_qual=rq)
    there = [r for r in recs.tolist() if (r[0], r[1]) in keys]
    assert len(there) == O and [r[5] for r in there] == list(range(40, 40 + O))
    assert all(r[2] == er.INS and r[3] == 0 and r[4] == ord("C") for r in there)
    assert recs.tolist() == _expected(b, out, labels, rq)[0]


# ---- 4. densities -------------------------------------------------------------------------------------------------------

def _owned(b, out):
    """numpy count of the owned columns: the distinct kept (region, position, index) -> (all, those with index 0) per region"""
    g = np.broadcast_to(out.region[:, None], out.position.shape)
    rs = b.ref_start[g]
    keep = (out.position >= 0) & (out.index >= 0) & ~((rs > 0) & (out.position <= rs + 200))
    keys = np.unique(np.stack([g[keep], out.position[keep], out.index[keep]], 1), axis=0)
    return [(int((keys[:, 0] == r).sum()), int(((keys[:, 0] == r) & (keys[:, 2] == 0)).sum())) for r in range(b.n_regions)]


def test_densities(hip_ctx, case):
    b, out, _, _ = case
    rng = np.random.default_rng(44)
    owned = _owned(b, out)
    assert sum(a for a, _ in owned) > 10_000 and all(z > 0 for _, z in owned)
    # every label equal to the draft's code (0 on insert rows): no edit
    clean = dataclasses.replace(b, ref=_draft(rng, len(b.ref), clean=True))
    g = np.broadcast_to(out.region[:, None], out.position.shape)
    at = np.clip(clean.ref_off[g] + out.position - clean.ref_start[g], 0, len(clean.ref) - 1)
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), clean.ref[at] & 0xDF) + 1
    labels = np.where(out.index == 0, code, 0).astype(np.uint8)
    counts = (C.c_int64 * 4)()
    eoff, recs = hip_ctx.polish_edits(out, labels, clean, counts=counts)
    assert list(counts) == [0, 0, -1, 0] and len(recs) == 0 and not eoff.any()
    # every label 0: one deletion per owned index-0 column
    eoff, recs = hip_ctx.polish_edits(out, np.zeros_like(labels), b)
    assert np.array_equal(np.diff(eoff), [z for _, z in owned]) and (recs["kind"] == er.DEL).all()
    assert (recs["index"] == 0).all() and (recs["base"] == 0).all() and len(recs) == eoff[-1]
    # every label C over an all-A draft (either case): one edit per owned column
    all_a = dataclasses.replace(b, ref=np.where(rng.random(len(b.ref)) < 0.3, ord("a"), ord("A")).astype(np.uint8))
    eoff, recs = hip_ctx.polish_edits(out, np.full_like(labels, 2), all_a)
    assert np.array_equal(np.diff(eoff), [a for a, _ in owned]) and (recs["base"] == ord("C")).all()
    assert np.array_equal(recs["kind"] == er.SUB, recs["index"] == 0) and np.array_equal(recs["kind"] == er.INS, recs["index"] > 0)


# ---- 5. errors ----------------------------------------------------------------------------------------------------------

def test_capacity(hip_ctx, case):
    b, out, labels, rq = case
    want, want_off = _expected(b, out, labels, rq)
    total = len(want)
    eoff, _, raw, c = _dev_edits(hip_ctx, out, labels, rq, b, capacity=total - 1)
    assert c == [total, _ffi.PV_ERR_CAPACITY, -1, 0] and np.array_equal(eoff, want_off) and (raw == MARK).all()
    counts, heoff = (C.c_int64 * 4)(), np.full(4, -7, np.int64)
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_edits(out, labels, b, row_qual=rq, edit_capacity=total - 1, counts=counts, region_edit_off=heoff)
    assert e.value.code == _ffi.PV_ERR_CAPACITY and ("need %d records" % total) in str(e.value)
    assert counts[0] == total and np.array_equal(heoff, want_off)
    eoff, recs, raw, c = _dev_edits(hip_ctx, out, labels, rq, b, capacity=total)      # the retry
    assert c == [total, 0, -1, 0] and recs.tolist() == want


def test_poisoned_label(hip_ctx, case):
    b, out, labels, rq = case
    want, _ = _expected(b, out, labels, rq)
    k = len(out.chunk_id) - 2
    assert out.region[k] == 2 and out.position[k, 700] > 8200
    bad = labels.copy()
    bad[k, 700] = 255                                        # an owned column of a middle chunk
    _, _, raw, c = _dev_edits(hip_ctx, out, bad, rq, b)
    assert c == [c[0], _ffi.PV_ERR_STATE, k, 0] and (raw == MARK).all()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_edits(out, bad, b, row_qual=rq)
    assert e.value.code == _ffi.PV_ERR_STATE and ("chunk %d" % k) in str(e.value)
    # on columns no label is read from: the loser of a shared column, the buffer behind a region start, the padding
    k9, k10 = (int(np.flatnonzero((out.region == 0) & (out.chunk_id == c_))[0]) for c_ in (9, 10))
    ok = labels.copy()
    ok[k10, :O] = 255                                        # chunk 9 owns these
    ok[k9 - 1, L - O:] = 255                                 # chunk 9 owns these too ("9" is after "8")
    buffer_ = (out.region == 2)[:, None] & (out.position >= 0) & (out.position <= 8200)
    pad = out.position < 0
    assert buffer_.sum() > 100 and pad.sum() > 100
    ok[buffer_ | pad] = 255
    _, recs, _, c = _dev_edits(hip_ctx, out, ok, rq, b)
    assert c == [len(want), 0, -1, 0] and recs[:len(want)].tolist() == want


def test_invalid_inputs(hip_ctx, case):
    b, out, labels, rq = case
    n = len(out.chunk_id)
    ids = out.chunk_id.copy()
    ids[[3, 4]] = ids[[4, 3]]
    swapped = types.SimpleNamespace(position=out.position, index=out.index, region=out.region, chunk_id=ids)
    _, _, raw, c = _dev_edits(hip_ctx, swapped, labels, rq, b)
    assert c[1:3] == [_ffi.PV_ERR_INVALID, 3] and (raw == MARK).all()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_edits(swapped, labels, b)
    assert e.value.code == _ffi.PV_ERR_INVALID
    # the last region's draft one byte shorter than its span: its last position has an owned column and no draft byte. The
    # device copy of ref keeps its full length, so nothing foreign could be touched either way.
    short = b.ref_off.copy()
    short[-1] -= 1
    assert (out.position[n - 1] == b.ref_end[2]).any()
    _, _, raw, c = _dev_edits(hip_ctx, out, labels, rq, b, ref_off=short)
    assert c[1:3] == [_ffi.PV_ERR_INVALID, n - 1] and (raw == MARK).all()
    # no draft bytes: the builder takes such a batch, this call does not
    assert _dev_edits(hip_ctx, out, labels, rq, b, ref=False) == _ffi.PV_ERR_INVALID
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.polish_edits(out, labels, dataclasses.replace(b, ref=None))
    assert e.value.code == _ffi.PV_ERR_INVALID


def test_no_chunks(hip_ctx, case):
    b = case[0]
    none = types.SimpleNamespace(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32),
                                 region=np.zeros(0, np.int32), chunk_id=np.zeros(0, np.int32))
    counts = (C.c_int64 * 4)()
    eoff, recs = hip_ctx.polish_edits(none, np.zeros((0, L), np.uint8), b, counts=counts)
    assert list(counts) == [0, 0, -1, 0] and len(recs) == 0 and eoff.tolist() == [0, 0, 0, 0]
    eoff, _, raw, c = _dev_edits(hip_ctx, none, np.zeros((0, L), np.uint8), None, b)
    assert c == [0, 0, -1, 0] and eoff.tolist() == [0, 0, 0, 0] and (raw == MARK).all()


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------

def test_graph_of_row_qual_stitch_qual_and_edits(hip_ctx, case):
    """the three passes of --qualities --edits captured as one graph; replays on refilled labels and acc equal the eager calls"""
    import qual_ref as qr
    b, out, _, _ = case
    n = len(out.chunk_id)
    do = DevicePolishOut(n)
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(np.array(getattr(out, name))))
    rs = torch.from_numpy(b.ref_start.astype(np.int64)).cuda()
    ro = torch.from_numpy(b.ref_off.astype(np.int64)).cuda()
    ref = torch.from_numpy(np.array(b.ref)).cuda()
    fills = []
    for s in range(3):
        rng = np.random.default_rng(60 + s)
        lab = rng.integers(0, 5, (n, L)).astype(np.uint8)
        acc = (rng.random((n, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
        acc[:, ::3] = np.float32(2.0) - np.float32(10.0) ** -(rng.random((n, len(range(0, L, 3)), 5), dtype=np.float32) * 9)
        fills.append((lab, acc))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    qual = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    roff = torch.zeros(4, dtype=torch.int64, device="cuda")
    eoff = torch.zeros(4, dtype=torch.int64, device="cuda")
    c_row, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(3))
    st = hip_ctx.stream

    def passes():
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_row.data_ptr(), L, O, stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), 3, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), 3,
                                 eoff.data_ptr(), buf.data_ptr(), n * L, c_ed.data_ptr(), stream=st)

    def state():
        t, e = int(c_st[0].item()), int(c_ed[0].item())
        return (seq[:t].cpu().numpy().tobytes(), qual[:t].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(),
                roff.cpu().numpy().tolist(), eoff.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(), c_ed.cpu().numpy().tolist())

    eager = []
    for lab, acc in fills:
        lab_d.copy_(torch.from_numpy(lab)); acc_d.copy_(torch.from_numpy(acc))
        torch.cuda.synchronize()
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        want, want_off = _expected(b, out, lab, qr.row_qual(lab, acc, O))
        assert np.frombuffer(eager[-1][2], EDIT_DTYPE).tolist() == want and eager[-1][4] == want_off.tolist()
        assert eager[-1][6] == [len(want), 0, -1, 0]
    assert eager[0][2] != eager[1][2]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        lab_d.copy_(torch.from_numpy(fills[k][0])); acc_d.copy_(torch.from_numpy(fills[k][1]))
        for t in (rq_d, seq, qual, buf, roff, eoff, c_row, c_st, c_ed):
            t.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 7. end to end ------------------------------------------------------------------------------------------------------

GAP = (2_300, 5_900)      # no read of ctg2 touches these positions: two regions in a row get no reads


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two contigs with reads, ctg2 with a read-free stretch longer than a region; drafts with N and IUPAC bytes; seeded P2
    weights"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("edits")
    rng = np.random.default_rng(23)
    contigs = [("ctg2", "".join(rng.choice(list("ACGTNRY"), size=9_500, p=[.24, .24, .24, .24, .02, .01, .01]))),
               ("ctg10", "".join(rng.choice(list("ACGTN"), size=4_200, p=[.245, .245, .245, .245, .02])))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 70, len(seq), tid=tid, mean_len=1200)
    recs = [r for r in recs if r["tid"] != 0 or r["pos"] + bw.ref_len(r["cigar"]) <= GAP[0] or r["pos"] > GAP[1]]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    return tmp, dict(contigs)


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what every launch's edit pass was given"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        res = super()._labels_and_stitch(db, n, n_regions)
        if n and self.edits:
            d = self.dout
            self.launches.append(dict(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(),
                                      region=d.region[:n].cpu().numpy(), chunk_id=d.chunk_id[:n].cpu().numpy(),
                                      labels=self.labels[:n].cpu().numpy(),
                                      row_qual=self.row_qual[:n].cpu().numpy() if self.qualities else None,
                                      ref_start=db.t["ref_start"][:n_regions].cpu().numpy(),
                                      ref_end=db.t["ref_end"][:n_regions].cpu().numpy(),
                                      ref_off=db.t["ref_off"][:n_regions + 1].cpu().numpy(), ref=db.t["ref"].cpu().numpy()))
        return res


def _recording_opener(hip_ctx, chains):
    def open_chain(device, shared, state_dict, dtype, qualities=False, edits=False):
        hip_ctx.load_p2(state_dict, dtype)
        chains.append(_RecordingChain(hip_ctx, qualities=qualities, edits=edits))
        return chains[-1]
    return open_chain


def _check_vcf(t, drafts, out_dir, launches, qualities):
    """the VCF of a run against the checker on what the device held, and against the run's own FASTA"""
    from pepper_thesis_amd.bamio import BamHandler, FastaHandler
    names = sorted(os.listdir(out_dir))
    assert names == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa"] + (
        ["_pepper_polished.fq"] if qualities else [])
    assert open(os.path.join(out_dir, names[1]), "rb").read(2) == b"\x1f\x8b"           # the tabix index is BGZF too
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(os.path.join(out_dir, names[0])).decode())
    assert header[0] == "fileformat=VCFv4.2" and header[1].startswith("source=") and header[2].startswith("reference=")
    assert header[3:5] == ["contig=<ID=ctg2,length=9500>", "contig=<ID=ctg10,length=4200>"]
    assert all(h.startswith("pepper_no_reads=") for h in header[5:]) and len(header) > 5
    assert cols == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    # the launches' regions are the run's regions with reads, in run order
    work, _ = polish.polish_work(FastaHandler(str(t / "ref.fa")), BamHandler(str(t / "reads.bam")), None)
    rep = {c: {} for c in drafts}
    w = 0
    for la in launches:
        spans = list(zip(la["ref_start"].tolist(), la["ref_end"].tolist()))
        for g, d in enumerate(er.region_dicts(la["position"], la["index"], la["region"], la["chunk_id"], la["labels"], spans,
                                              la["row_qual"])):
            while (work[w].start, work[w].end) != spans[g]:
                w += 1
            contig, draft = work[w].contig, drafts[work[w].contig].encode()
            w += 1
            assert la["ref"][la["ref_off"][g]:la["ref_off"][g + 1]].tobytes() == draft[spans[g][0]:spans[g][1] + 1]
            new = er.replacements(d, draft, 0)
            assert not set(new) & set(rep[contig])
            rep[contig].update(new)
    fasta = open(os.path.join(out_dir, "_pepper_polished.fa")).read().split("\n")
    seqs = dict(zip((l[1:] for l in fasta[0:-1:2]), fasta[1:-1:2]))
    assert list(seqs) == ["ctg2", "ctg10"]
    for c in drafts:
        mine = [r[1:] for r in recs if r[0] == c]
        assert mine == er.vcf_records(rep[c], drafts[c].encode(), qualities) and len(mine) > 100, c
        assert all((r[3] is None) != qualities for r in mine)
        cut = er.no_read_ranges(header, c)
        assert er.apply(mine, drafts[c].encode(), cut) == seqs[c], c
    cut = er.no_read_ranges(header, "ctg2")
    assert any(a <= 3_101 and 5_100 <= b < GAP[1] for a, b in cut)       # regions [2900, 4100] and [3900, 5100] as one run
    assert [r[0] for r in recs] == ["ctg2"] * sum(r[0] == "ctg2" for r in recs) + ["ctg10"] * sum(r[0] == "ctg10" for r in recs)


def test_polish_edits_end_to_end(inputs, hip_ctx, opts, monkeypatch):
    t, drafts = inputs
    monkeypatch.setenv("PV_SHARED_DEVICE", "1")
    opts(shared_device=1)
    chains = []
    base = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8"]
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "plain")]), open_chain=_recording_opener(hip_ctx, chains)) == 0
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "edits"), "--edits"]),
                      open_chain=_recording_opener(hip_ctx, chains)) == 0
    assert [(c.qualities, c.edits) for c in chains] == [(False, False), (False, True)]
    assert os.listdir(str(t / "plain")) == ["_pepper_polished.fa"]
    assert open(str(t / "edits" / "_pepper_polished.fa"), "rb").read() == open(str(t / "plain" / "_pepper_polished.fa"), "rb").read()
    assert len(chains[1].launches) > 1                       # -bs 8: 4 regions per launch
    _check_vcf(t, drafts, str(t / "edits"), chains[1].launches, False)


def test_polish_edits_with_qualities_realign_and_gpu_decode(inputs, hip_ctx, opts):
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    base = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "--qualities", "--realign",
            "--gpu_decode"]
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "plain_q")]), open_chain=_recording_opener(hip_ctx, chains)) == 0
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "edits_q"), "--edits"]),
                      open_chain=_recording_opener(hip_ctx, chains)) == 0
    for name in ("_pepper_polished.fa", "_pepper_polished.fq"):
        assert open(str(t / "edits_q" / name), "rb").read() == open(str(t / "plain_q" / name), "rb").read()
    _check_vcf(t, drafts, str(t / "edits_q"), chains[1].launches, True)
