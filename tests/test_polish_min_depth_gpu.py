"""GPU: `polish --min_depth`: the builder's depth plane and pv_polish_mask_low_depth[_dev] against the host checker
(tests/depth_ref.py), the error statuses, mask -> stitch -> edits as one captured graph, and the command end to end on a small
BAM: with a threshold no depth reaches the output is the draft whatever the weights are, and with a real threshold it is the
stitch checker's string over the checker-masked labels. Nothing here has a tolerance."""
import ctypes as C
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

import depth_ref as dr
import edits_ref as er
import stitch_ref as sr
from test_oracle_polish_ref import case_batch, load_golden, names
from pepper_thesis_amd import _ffi, bamio, cli, polish, synth
from pepper_thesis_amd.batch import Read, Region, pack_regions
from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut

pytestmark = pytest.mark.gpu
L, O = 1000, 50
MARK = 0xEE
PLANES = ("images", "position", "index", "region", "chunk_id", "flat_images", "flat_position", "flat_index", "region_row_off")


def _acgt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def _hand_regions():
    """three regions in one batch: reads that start before the region and run past its end; a hole in coverage, columns only
    deletions cover, inserts of 1 and 40 bases behind a column one read covers; 1100 columns whose rows cross the 512-column
    tile edge, the 1024-column scan block and (with their inserts) a chunk boundary"""
    rng = np.random.default_rng(7)
    before = Region(5_000, 5_399, _acgt(rng, 400),
                    [Read.make(4_700, "10S500M", _acgt(rng, 510)), Read.make(4_990, "20M5D400M", _acgt(rng, 420), is_reverse=True),
                     Read.make(5_100, "50M2I100M3N200M", _acgt(rng, 352)), Read.make(5_350, "100M", _acgt(rng, 100), mapq=0),
                     Read.make(5_399, "1M", "A")])
    thin = Region(0, 299, _acgt(rng, 300),
                  [Read.make(0, "100M", _acgt(rng, 100)), Read.make(20, "30M1I10M40I40M", _acgt(rng, 121)),      # inserts behind 49 and 59
                   Read.make(95, "5M", "ACGTA", is_reverse=True),
                   Read.make(200, "10M8D10M", _acgt(rng, 20)), Read.make(205, "5M8D10M", _acgt(rng, 15)),       # 210..217: deletions only
                   Read.make(250, "20M2P20M", _acgt(rng, 40))])
    wide = synth.synth_region(11, region_len=1_100, depth=6, read_len=300, site_every=40, ref_start=20_000)
    # (no read of 300 bases spans 400 positions: whatever could reach 20500..20529 goes, then one short read is put there)
    wide.reads = sorted([r for r in wide.reads if not 20_100 < r.pos < 20_530] + [Read.make(20_508, "8M", "ACGTACGT")],
                        key=lambda r: r.pos)
    return [before, thin, wide]


def _summaries(ctx, b, seq_length, seq_overlap):
    plain = ctx.polish_summarize(b, seq_length, seq_overlap, want_flat=True)
    got = ctx.polish_summarize(b, seq_length, seq_overlap, want_flat=True, want_depth=True)
    assert plain.depth is None and got.depth.dtype == np.uint16 and got.depth.shape == got.position.shape
    for f in PLANES:     # every other output: byte for byte that of a call without the plane
        assert np.array_equal(getattr(got, f), getattr(plain, f)), f
    return got


def _dev_summary(ctx, b, n, seq_length, seq_overlap, depth):
    """the device form into marked buffers -> the planes of its n chunks on the host (depth None without the plane)"""
    dev = "cuda:%d" % ctx.device_id
    db = DeviceBatch(b, dev)
    do = DevicePolishOut(n + 1, seq_length, seq_overlap, device=dev, depth=depth)
    for t in (do.images, do.position, do.index, do.region, do.chunk_id) + ((do.depth,) if depth else ()):
        t.fill_(-17 if t.dtype != torch.uint8 else MARK)
    torch.cuda.synchronize()
    ctx.polish_summarize_dev(db, do)
    ctx.synchronize()
    assert (do.n_chunks(), do.status()) == (n, 0)
    out = {f: getattr(do, f)[:n].cpu().numpy() for f in PLANES[:5]}
    out["depth"] = do.depth_numpy(n) if depth else None
    return out


def _check_depth(ctx, b, seq_length, seq_overlap, tag):
    got = _summaries(ctx, b, seq_length, seq_overlap)
    want = dr.row_depth(b, got.position, got.index, got.region)
    assert np.array_equal(got.depth, want), tag
    assert not got.depth[got.position < 0].any(), tag                     # padding rows
    n = len(got.chunk_id)
    with_plane, without = (_dev_summary(ctx, b, n, seq_length, seq_overlap, d) for d in (True, False))
    assert np.array_equal(with_plane["depth"], got.depth), tag            # the device form is the host form
    for f in PLANES[:5]:
        assert np.array_equal(with_plane[f], getattr(got, f)) and np.array_equal(without[f], getattr(got, f)), (tag, f)
    return got


# ---- 1. the depth plane ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1000, 50), (16, 3)])
def test_depth_plane_of_hand_made_regions(hip_ctx, sizes):
    b = pack_regions(_hand_regions())
    got = _check_depth(hip_ctx, b, *sizes, tag=sizes)
    per = [dr.region_depth(b, g) for g in range(3)]
    assert per[0][0] == 2 and per[0][-1] == 3 and per[0].max() == 3 and per[0][350] == 2   # reads from before the region; mapq 0 left out
    assert per[1][120:200].max() == 0 and per[1][210:218].tolist() == [2] * 8            # the hole; deletions only
    assert per[1][49] == 2 and per[1][59] == 2 and per[1][250:292].min() == 1           # the inserts' anchors; P takes its columns
    assert per[2][500:508].max() == 0 and per[2][508] == 1                                # the thin stretch across column 512
    # insert rows carry their anchor's depth: 1 and 40 rows behind positions 49 and 59 of region 1
    in1 = (got.region == 1)[:, None] & (got.index > 0)
    assert sorted(set(got.position[in1].tolist())) == [49, 59] and int(in1.sum()) >= 41 and (got.depth[in1] == 2).all()
    if sizes == (1000, 50):
        assert (got.region == 2).sum() == 2 and len(got.chunk_id) == 4                   # region 2's rows cross a chunk boundary


def test_depth_plane_of_the_golden_cases(hip_ctx):
    g = load_golden()
    keys = names(g)
    assert len(keys) >= 3
    seen = 0
    for key in keys:
        b = case_batch(g, key)
        got = _check_depth(hip_ctx, b, 1000, 50, key)
        seen += int(got.depth.max(initial=0))
    assert seen > 0
    # all of them as one batch
    from pepper_thesis_amd.batch import merge_batches
    _check_depth(hip_ctx, merge_batches([case_batch(g, k) for k in keys]), 1000, 50, "all")


# ---- 2. the mask ----------------------------------------------------------------------------------------------------------

def _draft(rng, n):
    """random draft bytes: ACGT with lower-case ones, and N, n and IUPAC codes in either case"""
    d = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    d[rng.random(n) < 0.3] += 32
    odd = rng.random(n) < 0.08
    d[odd] = rng.choice(np.frombuffer(b"NnRYkMs", np.uint8), int(odd.sum()))
    return d.astype(np.uint8)


def _mask_regions():
    """a 13-chunk region (a 12000-base insert: chunk ids 9 and 10 meet; depth 0, 1 and 2), a 1-chunk and a 2-chunk region
    with region_start > 0: depths 0..2 (all but its last 80 columns bare) and 3..15"""
    rng = np.random.default_rng(5)
    ins = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 12_000))
    regs = [Region(0, 299, b"A" * 300, [Read.make(10, "5M12000I60M", b"C" * 5 + ins + b"G" * 60), Read.make(0, "250M", "A" * 250)]),
            synth.synth_region(300, region_len=400, depth=8, read_len=300, site_every=50, ref_start=5000),
            synth.synth_region(301, region_len=1200, depth=8, read_len=500, site_every=50, ref_start=8000)]
    regs[1].reads = [r for r in regs[1].reads if not 4_800 < r.pos < 5_230]     # a hole in the 1-chunk region, 5200..5229 at the least
    for r in regs:
        r.ref = _draft(rng, len(r.ref)).tobytes()
    return regs


@pytest.fixture(scope="module")
def mask_cases(hip_ctx):
    """{chunks: (batch, its chunks with the depth plane, labels, row qualities)} for 1, 3 and 16 chunks: shared and left
    unchanged (tests copy what they alter)"""
    regs = _mask_regions()
    out = {}
    for pick in ([1], [1, 2], [0, 1, 2]):
        b = pack_regions([regs[g] for g in pick])
        po = hip_ctx.polish_summarize(b, want_depth=True)
        n = len(po.chunk_id)
        rng = np.random.default_rng(100 + n)
        labels = rng.integers(0, 5, (n, L)).astype(np.uint8)
        rq = rng.integers(1, 94, (n, L)).astype(np.uint8)
        k, j = np.unravel_index(int(np.argmax(po.depth)), po.depth.shape)
        labels[k, j] = 255                                            # a poisoned label on the deepest row
        for a in (po.position, po.index, po.region, po.chunk_id, po.depth, labels, rq, b.ref, b.ref_off, b.ref_start):
            a.setflags(write=False)
        out[n] = (b, po, labels, rq)
    assert sorted(out) == [1, 3, 16]
    return out


def _want(b, po, labels, rq, min_depth, depth=None):
    return dr.mask(labels, rq, po.depth if depth is None else depth, po.position, po.index, po.region, b.ref_start, b.ref_off,
                   b.ref, min_depth)


def _dev_mask(ctx, po, labels, rq, b, min_depth, in_place=False, ref=True, ref_off=None, depth=True):
    """the device-resident form on uploaded copies; out of place the outputs are pre-filled with a marker -> (labels out,
    row qualities out or None, labels in and row qualities in as they are afterwards, counts) or the error code of the call"""
    n = len(po.chunk_id)
    do = DevicePolishOut(max(n, 1), depth=depth)
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(np.array(getattr(po, name))))
    if depth:
        do.set_depth(np.array(po.depth))
    lab = torch.from_numpy(np.array(labels)).cuda()
    drq = torch.from_numpy(np.array(rq)).cuda() if rq is not None else None
    lab_out = lab if in_place else torch.full_like(lab, MARK)
    rq_out = None if rq is None else (drq if in_place else torch.full_like(drq, MARK))
    rs = torch.from_numpy(np.asarray(b.ref_start, np.int64).copy()).cuda()
    ro = torch.from_numpy(np.asarray(b.ref_off if ref_off is None else ref_off, np.int64).copy()).cuda()
    d_ref = torch.from_numpy(np.array(b.ref)).cuda()          # always as long as the batch's own ref_off says
    counts = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    code = None
    try:
        ctx.polish_mask_low_depth_dev(do, n, lab.data_ptr(), drq.data_ptr() if rq is not None else 0, rs.data_ptr(), ro.data_ptr(),
                                      d_ref.data_ptr() if ref else 0, len(rs), min_depth, lab_out.data_ptr(),
                                      rq_out.data_ptr() if rq is not None else 0, counts.data_ptr())
    except _ffi.PepperHipError as e:
        code = e.code
    ctx.synchronize()
    res = (lab_out.cpu().numpy(), None if rq is None else rq_out.cpu().numpy(), lab.cpu().numpy(),
           None if rq is None else drq.cpu().numpy(), counts.cpu().numpy().tolist())
    return res if code is None else (code,) + res


@pytest.mark.parametrize("with_qual", [False, True])
@pytest.mark.parametrize("n_chunks", [1, 3, 16])
def test_mask_equals_checker(hip_ctx, mask_cases, n_chunks, with_qual):
    b, po, labels, rq = mask_cases[n_chunks]
    q = rq if with_qual else None
    real = po.depth[po.position >= 0]
    uniq = np.unique(real[real > 0])
    d = int(uniq[len(uniq) // 2])                     # a depth that occurs, with smaller ones that occur too
    assert len(uniq) >= 2 and uniq[0] < d and (real == 0).any() and (real == d).any()
    if n_chunks == 16:   # the 9 / 10 overlap: both chunks hold the same rows with the same depth
        k9, k10 = (int(np.flatnonzero((po.region == 0) & (po.chunk_id == c_))[0]) for c_ in (9, 10))
        assert np.array_equal(po.position[k9, L - O:], po.position[k10, :O]) and np.array_equal(po.depth[k9, L - O:], po.depth[k10, :O])
    seen = []
    for md in (0, 1, d, d + 1, 65535):
        want_lab, want_q, masked, unmaskable = _want(b, po, labels, q, md)
        seen.append((masked, unmaskable))
        counts = (C.c_int64 * 4)()
        got_lab, got_q = hip_ctx.polish_mask_low_depth(po, labels, b, md, row_qual=q, counts=counts)
        assert list(counts) == [masked, 0, -1, unmaskable], md
        assert np.array_equal(got_lab, want_lab) and (got_q is None if q is None else np.array_equal(got_q, want_q)), md
        lab2, q2 = labels.copy(), None if q is None else q.copy()                                # in place on the host
        r_lab, r_q = hip_ctx.polish_mask_low_depth(po, lab2, b, md, row_qual=q2, in_place=True)
        assert r_lab is lab2 and r_q is q2 and np.array_equal(lab2, want_lab) and (q is None or np.array_equal(q2, want_q)), md
        for in_place in (False, True):
            out_lab, out_q, in_lab, in_q, c = _dev_mask(hip_ctx, po, labels, q, b, md, in_place=in_place)
            assert c == [masked, 0, -1, unmaskable], (md, in_place)
            assert np.array_equal(out_lab, want_lab) and (q is None or np.array_equal(out_q, want_q)), (md, in_place)
            if not in_place:                                                                      # the inputs are read only
                assert np.array_equal(in_lab, labels) and (q is None or np.array_equal(in_q, q))
        if md <= po.depth.max():                      # the label 255 sits on a row that is not masked: copied
            assert (want_lab == 255).sum() == 1 and np.array_equal(want_lab == 255, labels == 255)
    assert seen[0] == (0, 0) and 0 < seen[1][0] < seen[2][0] < seen[3][0] <= seen[4][0]
    assert seen[4][1] > 0 and seen[4][0] + seen[4][1] == int((po.position >= 0).sum())            # N and IUPAC bytes: counted, kept


def test_masked_labels_spell_the_draft_through_stitch_and_edits(hip_ctx, mask_cases):
    """every row masked: the stitch gives the upper-cased draft wherever it can be spelled, and the edits are those of the
    unmaskable columns alone"""
    b, po, labels, rq = mask_cases[16]
    labels = np.where(labels == 255, 1, labels).astype(np.uint8)      # (it may lie over an unmaskable byte, which keeps its label)
    lab, q = hip_ctx.polish_mask_low_depth(po, labels, b, 65535, row_qual=rq)
    roff, seq, qual = hip_ctx.polish_stitch_qual(po, lab, q, b.ref_start)
    eoff, recs = hip_ctx.polish_edits(po, lab, b, row_qual=q)
    for g in range(b.n_regions):
        start, end = int(b.ref_start[g]), int(b.ref_end[g])
        draft = b.ref[int(b.ref_off[g]):int(b.ref_off[g + 1])].tobytes()
        mine = recs[eoff[g]:eoff[g + 1]]
        first = start + 201 if start > 0 else start
        hard = [p for p in range(first, end + 1) if er.upper(draft[p - start]) not in "ACGT"]
        assert len(hard) > 5 and mine["position"].tolist() == hard and (mine["index"] == 0).all()
        pred = er.region_dicts(po.position, po.index, po.region, po.chunk_id, lab, list(zip(b.ref_start.tolist(), b.ref_end.tolist())), q)[g]
        assert seq[roff[g]:roff[g + 1]].decode() == er.polished(pred, draft, start)
        rep = er.replacements(pred, draft, start)     # position -> what stands for it, inserted bases included
        assert sorted(rep) == list(range(first, end + 1))
        assert all(rep[p][0] == er.upper(draft[p - start]) for p in rep if p not in set(hard))
    assert set(qual) <= set(range(94)) and qual.count(0) >= int(0.9 * len(qual))


# ---- 3. statuses ----------------------------------------------------------------------------------------------------------

def _untouched(res, labels, rq, in_place):
    """a refused call or an invalid device status leaves labels and qualities as they were (out of place: the marker)"""
    out_lab, out_q, in_lab, in_q = res[:4]
    assert np.array_equal(in_lab, labels) and np.array_equal(in_q, rq)
    if not in_place:
        assert (out_lab == MARK).all() and (out_q == MARK).all()


@pytest.mark.parametrize("in_place", [False, True])
def test_invalid_calls_touch_nothing(hip_ctx, mask_cases, in_place):
    b, po, labels, rq = mask_cases[3]
    n = len(po.chunk_id)
    for kw, md in ((dict(depth=False), 3), (dict(ref=False), 3), (dict(), 65536), (dict(), -1)):
        res = _dev_mask(hip_ctx, po, labels, rq, b, md, in_place=in_place, **kw)
        assert res[0] == _ffi.PV_ERR_INVALID and res[-1] == [-7] * 4, (kw, md)             # refused by the call itself
        _untouched(res[1:], labels, rq, in_place)
    # the last region's draft one byte shorter than its span: its last position is masked and has no draft byte. The device
    # copy of ref keeps its full length, so nothing foreign could be touched either way.
    short = b.ref_off.copy()
    short[-1] -= 1
    assert (po.position[n - 1] == b.ref_end[1]).any()
    res = _dev_mask(hip_ctx, po, labels, rq, b, 65535, in_place=in_place, ref_off=short)
    assert res[-1] == [0, _ffi.PV_ERR_INVALID, n - 1, 0]
    _untouched(res, labels, rq, in_place)
    # the same position is fine while its rows are deep enough not to be masked
    md = int(po.depth[n - 1][po.position[n - 1] == b.ref_end[1]].min())
    res = _dev_mask(hip_ctx, po, labels, rq, b, md, in_place=in_place, ref_off=short)
    want_lab, want_q, masked, unmaskable = _want(b, po, labels, rq, md)
    assert res[-1] == [masked, 0, -1, unmaskable] and np.array_equal(res[0], want_lab) and np.array_equal(res[1], want_q)
    # a broken chunk layout
    ids = po.chunk_id.copy()
    ids[[1, 2]] = ids[[2, 1]]
    swapped = types.SimpleNamespace(position=po.position, index=po.index, region=po.region, chunk_id=ids, depth=po.depth)
    res = _dev_mask(hip_ctx, swapped, labels, rq, b, 3, in_place=in_place)
    assert res[-1] == [0, _ffi.PV_ERR_INVALID, 1, 0]
    _untouched(res, labels, rq, in_place)


def test_invalid_calls_of_the_host_form(hip_ctx, mask_cases):
    b, po, labels, rq = mask_cases[3]
    no_depth = types.SimpleNamespace(position=po.position, index=po.index, region=po.region, chunk_id=po.chunk_id)
    short = b.ref_off.copy()
    short[-1] -= 1
    for chunks, batch, md in ((no_depth, b, 3), (po, dataclasses.replace(b, ref=None), 3), (po, b, 65536),
                              (po, dataclasses.replace(b, ref_off=short), 65535)):
        lab2, q2 = labels.copy(), rq.copy()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_mask_low_depth(chunks, lab2, batch, md, row_qual=q2, in_place=True)
        assert e.value.code == _ffi.PV_ERR_INVALID
        assert np.array_equal(lab2, labels) and np.array_equal(q2, rq)


def test_no_chunks(hip_ctx, mask_cases):
    b = mask_cases[3][0]
    none = types.SimpleNamespace(position=np.zeros((0, L), np.int64), index=np.zeros((0, L), np.int32), region=np.zeros(0, np.int32),
                                 chunk_id=np.zeros(0, np.int32), depth=np.zeros((0, L), np.uint16))
    counts = (C.c_int64 * 4)()
    lab, q = hip_ctx.polish_mask_low_depth(none, np.zeros((0, L), np.uint8), b, 4, counts=counts)
    assert list(counts) == [0, 0, -1, 0] and lab.shape == (0, L) and q is None
    assert _dev_mask(hip_ctx, none, np.zeros((0, L), np.uint8), None, b, 4)[-1] == [0, 0, -1, 0]


# ---- 4. one linear graph --------------------------------------------------------------------------------------------------

def test_graph_of_mask_stitch_qual_and_edits(hip_ctx, mask_cases):
    """mask (in place), stitch with qualities and edits captured as one graph on one stream; replays on refilled labels and
    row qualities equal the eager calls"""
    b, po, _, _ = mask_cases[16]
    n, G = len(po.chunk_id), b.n_regions
    do = DevicePolishOut(n, depth=True)
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(np.array(getattr(po, name))))
    do.set_depth(np.array(po.depth))
    rs = torch.from_numpy(b.ref_start.astype(np.int64)).cuda()
    ro = torch.from_numpy(b.ref_off.astype(np.int64)).cuda()
    ref = torch.from_numpy(np.array(b.ref)).cuda()
    fills = []
    for s in range(3):
        rng = np.random.default_rng(70 + s)
        fills.append((rng.integers(0, 5, (n, L)).astype(np.uint8), rng.integers(1, 94, (n, L)).astype(np.uint8)))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    qual = torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    roff = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
    eoff = torch.zeros(G + 1, dtype=torch.int64, device="cuda")
    c_mk, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(3))
    st = hip_ctx.stream
    MD = 2

    def passes():
        hip_ctx.polish_mask_low_depth_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G,
                                          MD, lab_d.data_ptr(), rq_d.data_ptr(), c_mk.data_ptr(), stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), G, roff.data_ptr(), seq.data_ptr(),
                                       qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), rs.data_ptr(), ro.data_ptr(), ref.data_ptr(), G,
                                 eoff.data_ptr(), buf.data_ptr(), n * L, c_ed.data_ptr(), stream=st)

    def state():
        t, e = int(c_st[0].item()), int(c_ed[0].item())
        return (lab_d.cpu().numpy().tobytes(), rq_d.cpu().numpy().tobytes(), seq[:t].cpu().numpy().tobytes(),
                qual[:t].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(), roff.cpu().numpy().tolist(),
                eoff.cpu().numpy().tolist(), c_mk.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(), c_ed.cpu().numpy().tolist())

    eager = []
    for lab, rq in fills:
        lab_d.copy_(torch.from_numpy(lab)); rq_d.copy_(torch.from_numpy(rq))
        torch.cuda.synchronize()
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        want_lab, want_q, masked, unmaskable = _want(b, po, lab, rq, MD)
        assert eager[-1][0] == want_lab.tobytes() and eager[-1][1] == want_q.tobytes() and eager[-1][7] == [masked, 0, -1, unmaskable]
        h_roff, h_seq, h_qual = hip_ctx.polish_stitch_qual(po, want_lab, want_q, b.ref_start)
        assert (eager[-1][2], eager[-1][3], eager[-1][5]) == (h_seq, h_qual, h_roff.tolist()) and masked > 100
    assert eager[0][2] != eager[1][2]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 2, 2):
        lab_d.copy_(torch.from_numpy(fills[k][0])); rq_d.copy_(torch.from_numpy(fills[k][1]))
        for t in (seq, qual, buf, roff, eoff, c_mk, c_st, c_ed):
            t.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 5. and 6. the command ------------------------------------------------------------------------------------------------

HOLE = (1_500, 1_700)     # no read of ctgA touches these positions: a hole inside region [900, 2100]
HALF = 2_000              # no read of ctgB reaches past this position: its last regions have no reads


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two contigs of a few kb with an ACGT / acgt draft (nothing unmaskable); seeded P2 weights"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("min_depth")
    rng = np.random.default_rng(41)
    contigs = [("ctgA", "".join(rng.choice(list("ACGTacgt"), size=4_200))), ("ctgB", "".join(rng.choice(list("ACGTacgt"), size=4_000)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 70, len(seq), tid=tid, mean_len=900)
    recs = [r for r in recs if (r["tid"] == 0 and (r["pos"] + bw.ref_len(r["cigar"]) <= HOLE[0] or r["pos"] >= HOLE[1])) or
            (r["tid"] == 1 and r["pos"] + bw.ref_len(r["cigar"]) <= HALF)]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(37, 3.0))
    return tmp, dict(contigs)


class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what the mask of every launch was given and what it left"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches = []

    def _labels_and_stitch(self, db, n, n_regions):
        ctx, real, seen = self.ctx, self.ctx.polish_mask_low_depth_dev, {}

        def spy(dout, n_chunks, *a, **k):
            ctx.synchronize()
            seen.update(labels_in=self.labels[:n_chunks].cpu().numpy(),
                        row_qual_in=self.row_qual[:n_chunks].cpu().numpy() if self.qualities else None)
            return real(dout, n_chunks, *a, **k)
        ctx.polish_mask_low_depth_dev = spy
        try:
            res = super()._labels_and_stitch(db, n, n_regions)
        finally:
            del ctx.polish_mask_low_depth_dev
        if n:
            d = self.dout
            seen.update(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(), region=d.region[:n].cpu().numpy(),
                        chunk_id=d.chunk_id[:n].cpu().numpy(), depth=d.depth_numpy(n), labels=self.labels[:n].cpu().numpy(),
                        row_qual=self.row_qual[:n].cpu().numpy() if self.qualities else None,
                        ref_start=db.t["ref_start"][:n_regions].cpu().numpy(), ref_end=db.t["ref_end"][:n_regions].cpu().numpy(),
                        ref_off=db.t["ref_off"][:n_regions + 1].cpu().numpy(), ref=db.t["ref"].cpu().numpy(), masked=res.masked)
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


def test_a_threshold_no_depth_reaches_gives_the_draft(inputs, hip_ctx, opts):
    """weight-independent: every depth is below 65535 and the drafts hold no unmaskable byte, so every column is masked"""
    t, drafts = inputs
    opts(shared_device=1)
    assert all(set(d) <= set("ACGTacgt") for d in drafts.values())           # checked on the host: nothing unmaskable
    chains = []
    argv = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8", "-o", str(t / "all"),
            "--min_depth", "65535", "--qualities", "--edits"]
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=_recording_opener(hip_ctx, chains)) == 0
    assert chains[0].min_depth == 65535 and len(chains[0].launches) > 1
    for la in chains[0].launches:
        assert la["masked"] == (int((la["position"] >= 0).sum()), 0) and (la["labels"] != la["labels_in"]).any()
    assert _fasta(str(t / "all" / "_pepper_polished.fa")) == {c: d.upper() for c, d in drafts.items()}
    fq = open(str(t / "all" / "_pepper_polished.fq")).read().split("\n")
    assert fq == [x for c, d in drafts.items() for x in ("@" + c, d.upper(), "+", "!" * len(d))] + [""]
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(str(t / "all" / "_pepper_polished.edits.vcf.gz")).decode())
    assert recs == [] and header[3:] == ["contig=<ID=ctgA,length=4200>", "contig=<ID=ctgB,length=4000>", "pepper_min_depth=65535"]


@pytest.mark.parametrize("flags", [[], ["--realign", "--gpu_decode", "--qualities", "--edits"]], ids=["plain", "all_flags"])
def test_min_depth_3_end_to_end(inputs, hip_ctx, opts, flags):
    from pepper_thesis_amd.bamio import BamHandler, FastaHandler
    t, drafts = inputs
    opts(shared_device=1)
    chains = []
    out_dir = str(t / ("three_" + ("flags" if flags else "plain")))
    argv = ["-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8", "-o", out_dir,
            "--min_depth", "3"] + flags
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=_recording_opener(hip_ctx, chains)) == 0
    launches = chains[0].launches
    work, _ = polish.polish_work(FastaHandler(str(t / "ref.fa")), BamHandler(str(t / "reads.bam")), None)
    parts = {w.index: None for w in work}            # what every region of the run gives, by the checkers
    thin = masked_rows = 0
    w = 0
    for la in launches:
        # the chain's mask did what the checker does with the labels, qualities and depth the device held
        want_lab, want_q, masked, unmaskable = dr.mask(la["labels_in"], la["row_qual_in"], la["depth"], la["position"], la["index"],
                                                       la["region"], la["ref_start"], la["ref_off"], la["ref"], 3)
        assert np.array_equal(la["labels"], want_lab) and la["masked"] == (masked, unmaskable) and unmaskable == 0
        assert la["row_qual"] is None or np.array_equal(la["row_qual"], want_q)
        masked_rows += masked
        spans = list(zip(la["ref_start"].tolist(), la["ref_end"].tolist()))
        regs = sr.regions_from_chunks(la["position"], la["index"], la["region"], la["chunk_id"], want_lab, spans)
        for g, reg in enumerate(regs):
            while (work[w].start, work[w].end) != spans[g]:
                w += 1
            draft = drafts[work[w].contig]
            parts[work[w].index] = sr.small_chunk_stitch([reg])[2]
            # every kept position below the threshold keeps its draft base, and nothing is inserted behind it
            pred = er.column_dict(reg)
            rows = la["region"] == g
            below = set(la["position"][rows][(la["depth"][rows] < 3) & (la["position"][rows] >= 0)].tolist())
            for (p, x), (label, _) in pred.items():
                if p in below:
                    thin += 1
                    assert label == (0 if x else 1 + "ACGT".index(draft[p].upper())), (work[w], p, x)
            w += 1
    assert masked_rows > 300 and thin > 300
    for wk in work:                                   # the regions without reads: the draft of their kept range
        if parts[wk.index] is None:
            first, last = polish.kept_range(wk)
            parts[wk.index] = drafts[wk.contig][first:last + 1].upper()
    empty = [(wk.contig, wk.start) for wk in work if not any((wk.start, wk.end) in zip(la["ref_start"].tolist(), la["ref_end"].tolist())
                                                               for la in launches)]
    assert ("ctgB", 2900) in empty and all(c == "ctgB" for c, _ in empty)
    want = {c: "".join(parts[wk.index] for wk in work if wk.contig == c) for c in drafts}
    got = _fasta(os.path.join(out_dir, "_pepper_polished.fa"))
    assert got == want
    for c, (a, z) in (("ctgA", HOLE), ("ctgB", (HALF + 200, 4_000))):
        # the draft's coordinates hold up to the stretch nobody covers only if nothing before it changed length; look for the
        # stretch itself instead: it stands in the output as it stands in the draft
        assert drafts[c][a:z].upper() in got[c], c
    if flags:
        header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(os.path.join(out_dir, "_pepper_polished.edits.vcf.gz")).decode())
        assert header[3:] == ["contig=<ID=ctgA,length=4200>", "contig=<ID=ctgB,length=4000>", "pepper_min_depth=3"]
        for c in drafts:
            mine = [r[1:] for r in recs if r[0] == c]
            assert er.apply(mine, drafts[c].encode()) == got[c] and mine, c                # the records applied to the draft
            assert not [r for r in mine if r[0] + len(r[1]) - 1 > (HALF + 250 if c == "ctgB" else 10**9)]
        fq = open(os.path.join(out_dir, "_pepper_polished.fq")).read().split("\n")
        assert fq[0::4][:2] == ["@ctgA", "@ctgB"] and fq[1::4] == [got["ctgA"], got["ctgB"]]
        at = got["ctgA"].index(drafts["ctgA"][HOLE[0]:HOLE[1]].upper())
        assert set(fq[3][at:at + HOLE[1] - HOLE[0]]) == {"!"}


def test_chain_host_fallback_carries_the_depth(hip_ctx, opts, mask_cases, monkeypatch):
    """a batch beyond the device builder's workspace heuristics (the 12000-base insert) takes the host form: the depth plane
    is uploaded with the other planes and the mask sees it"""
    from pepper_thesis_amd import polish_summary
    b, po, _, _ = mask_cases[16]
    b = dataclasses.replace(b, **{f: np.array(getattr(b, f)) for f in ("ref", "ref_off", "ref_start")})    # writable copies
    opts(shared_device=1)
    hip_ctx.load_p2(synth.make_weights_p2(37, 3.0))
    host_calls, real = [], polish_summary.polish_summarize
    monkeypatch.setattr(polish_summary, "polish_summarize", lambda *a, **k: host_calls.append(k) or real(*a, **k))
    chain = _RecordingChain(hip_ctx, min_depth=2)
    res = chain.run(b)
    assert host_calls == [{"want_depth": True}]                       # the host form ran, once, and was asked for the plane
    la, = chain.launches
    assert np.array_equal(la["depth"], po.depth) and np.array_equal(la["position"], po.position)
    want_lab, _, masked, unmaskable = _want(b, po, la["labels_in"], None, 2)
    assert masked == int(((po.depth < 2) & (po.position >= 0)).sum()) - unmaskable and masked > 0 and unmaskable > 0
    assert np.array_equal(la["labels"], want_lab) and res.masked == (masked, unmaskable)
    roff, seq = hip_ctx.polish_stitch(po, want_lab, b.ref_start)
    assert np.array_equal(res.region_off, roff) and res.bases == seq
