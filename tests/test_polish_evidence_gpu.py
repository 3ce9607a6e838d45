"""GPU: `polish --edits --evidence`: the builder's counts plane and pv_polish_edits_evidence[_dev] against the host checker
(tests/counts_ref.py), the statuses and refusals, one captured graph, and the command end to end on a small BAM. Nothing
here has a tolerance."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

import counts_ref as cr
import depth_ref as dr
import edits_ref as er
import min_qual_cases as mq
import polish_cases as pc
from test_polish_edits_gpu import inputs                   # the small synthetic BAM of the edits tests (a module fixture)
from test_polish_hp_gpu import inputs as hp_inputs         # the tagged BAM and its two pre-split files
from pepper_thesis_amd import _ffi, bamio, cli, polish
from pepper_thesis_amd.batch import Read, Region, pack_regions
from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut
from pepper_thesis_amd.polish_edits import EDIT_DTYPE, EVIDENCE_DTYPE

pytestmark = pytest.mark.gpu
MARK = 0xEE
CHUNK_PLANES = ("images", "position", "index", "region", "chunk_id")
PLANES = CHUNK_PLANES + ("flat_images", "flat_position", "flat_index", "region_row_off")


# ---- 1. the counts plane ----------------------------------------------------------------------------------------------------

def _acgt(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def _ten(c):
    """reads that make all ten counts of column c non-zero: A C G T and N on either strand"""
    return [Read.make(c, "1M", base, 20, rev) for base, rev in itertools.product("ACGTN", (False, True))]


def _ins(c, n, rng):
    """an n-base insert behind column c on either strand"""
    return [Read.make(c, "1M%dI1M" % n, _acgt(rng, n + 2), 20, rev) for rev in (False, True)]


def _edge_regions():
    """[a 7-column filler, a region of 1100 columns]: the region's columns 504, 505 / 1016, 1017 are the batch's 511, 512 /
    1023, 1024, the last and first columns of a 512-column tile and of a 1024-column scan block; all four hold all ten counts
    and 3 insert rows. With the 6 insert rows of 504 and 505 in front, column 991 is the region's row 997 and its 6 insert rows
    are rows 998..1003: at 1000/50 they fall in two chunks (rows 950..999 are shared, 1000.. are the second chunk's alone);
    columns 991 and 992 hold all ten counts. Column 700 lies under 300 reads of one base."""
    rng = np.random.default_rng(17)
    S = 30_000
    reads = [Read.make(S, "1100M", _acgt(rng, 1100), 20, rev) for rev in (False, True)]
    for c in (504, 505, 1016, 1017):
        reads += _ten(S + c) + _ins(S + c, 3, rng)
    reads += _ten(S + 991) + _ten(S + 992) + _ins(S + 991, 6, rng)
    reads += [Read.make(S + 700, "1M", "A") for _ in range(300)]
    reads.sort(key=lambda r: r.pos)
    return [Region(0, 6, b"ACGTACG", []), Region(S, S + 1099, _acgt(rng, 1100), reads)]


def _dev_summary(ctx, b, n, seq_length, seq_overlap, depth, counts):
    """the device form into marked buffers of n + 1 chunks -> the planes of its n chunks on the host; chunk n must stay marked"""
    dev = "cuda:%d" % ctx.device_id
    db = DeviceBatch(b, dev)
    do = DevicePolishOut(n + 1, seq_length, seq_overlap, device=dev, depth=depth, counts=counts)
    marked = (do.images, do.position, do.index, do.region, do.chunk_id) + ((do.depth,) if depth else ()) + ((do.row_counts,) if counts else ())
    for t in marked:
        t.fill_(-17 if t.dtype != torch.uint8 else MARK)
    torch.cuda.synchronize()
    ctx.polish_summarize_dev(db, do)
    ctx.synchronize()
    assert (do.n_chunks(), do.status()) == (n, 0)
    out = {f: getattr(do, f)[:n].cpu().numpy() for f in CHUNK_PLANES}
    out["depth"] = do.depth_numpy(n) if depth else None
    out["counts"] = do.row_counts_numpy(n) if counts else None
    if counts:
        assert (do.row_counts[n:].cpu().numpy() == -17).all()       # nothing beyond n_chunks
    if depth:
        assert (do.depth[n:].cpu().numpy() == -17).all()
    return out


def _check_counts(ctx, b, seq_length, seq_overlap, tag, device_form=True, combos=((False, False), (False, True), (True, False), (True, True))):
    """host form under the combinations of the two planes (depth, counts) given; the plane against the checker; the device
    form against the host form"""
    got = {(d, c): ctx.polish_summarize(b, seq_length, seq_overlap, want_flat=True, want_depth=d, want_counts=c) for d, c in combos}
    plain, both = got[(False, False)], got[(True, True)]
    assert plain.counts is None and plain.depth is None
    for key, o in got.items():
        assert (o.depth is None) != key[0] and (o.counts is None) != key[1], (tag, key)
        for f in PLANES:     # every other output: byte for byte that of a call without either plane
            assert np.array_equal(getattr(o, f), getattr(plain, f)), (tag, key, f)
        assert o.depth is None or np.array_equal(o.depth, both.depth), (tag, key)
        assert o.counts is None or np.array_equal(o.counts, both.counts), (tag, key)
    assert both.counts.dtype == np.uint16 and both.counts.shape == both.position.shape + (10,)
    want = cr.row_counts(b, both.position, both.index, both.region)
    assert np.array_equal(both.counts, want), tag
    assert np.array_equal(both.depth, dr.row_depth(b, both.position, both.index, both.region)), tag
    assert not both.counts[both.position < 0].any(), tag                                         # padding rows
    base = both.index == 0
    # the header's invariant (the depth clamped as the header says: deep_column has more reads than a region can hold)
    assert np.array_equal(np.minimum(both.counts[base].astype(np.int64).sum(axis=1), 65535), both.depth[base]), tag
    assert not both.images[both.counts == 0].any(), tag                                           # no read, no pixel
    if device_form:
        n = len(both.chunk_id)
        for d, c in got:
            dev = _dev_summary(ctx, b, n, seq_length, seq_overlap, d, c)
            for f in CHUNK_PLANES:
                assert np.array_equal(dev[f], getattr(plain, f)), (tag, d, c, f)
            assert dev["depth"] is None if not d else np.array_equal(dev["depth"], both.depth), (tag, d, c)
            assert dev["counts"] is None if not c else np.array_equal(dev["counts"], both.counts), (tag, d, c)
    return both


@pytest.mark.parametrize("sizes", [(1000, 50), (16, 3)])
def test_counts_plane_across_tile_block_and_chunk_edges(hip_ctx, sizes):
    regions = _edge_regions()
    b = pack_regions(regions)
    got = _check_counts(hip_ctx, b, *sizes, tag=sizes)
    S = int(b.ref_start[1])
    table, _ = cr.region_tables(b, 1)
    for c in (504, 505, 1016, 1017, 991, 992):
        assert table[c].min() >= 1, c                                        # all ten counts on either side of every edge
    assert table[700][4] >= 300
    at = (got.position == S + 700) & (got.index == 0)
    assert at.any() and (got.counts[at][:, 4] >= 300).all() and (got.depth[at] >= 300).all()        # above a byte
    if sizes == (1000, 50):
        assert (got.region == 1).sum() == 2
        rows = [(k, j) for k, j in zip(*np.nonzero((got.position == S + 991) & (got.index > 0)))]
        assert sorted(set(k for k, _ in rows)) == [1, 2] and len(rows) == 2 + 6       # rows 998, 999 twice, 1000..1003 once
        for x in range(1, 7):
            assert got.counts[(got.position == S + 991) & (got.index == x)].sum(axis=1).tolist() in ([2], [2, 2])


GOLDEN = sorted(pc.CASES) + ["tile_edges_%d_%s" % (e, "bare" if bare else "full") for e, bare in ((512, False), (1023, True))]


@pytest.mark.parametrize("name", GOLDEN)
def test_counts_plane_of_the_builder_cases(hip_ctx, name):
    if name.startswith("tile_edges"):
        _, _, e, kind = name.split("_")
        regions, (L, O) = pc.tile_edges(int(e), kind == "bare", 2), (1000, 50)
    else:
        make, L, O = pc.CASES[name]
        regions = make()
    b = pack_regions(regions)
    # (the overflow cases need the host form's retry: the device form reports PV_ERR_LIMIT there, as without the plane)
    _check_counts(hip_ctx, b, L, O, name, device_form="overflow" not in name, combos=((False, False), (True, True)))


# ---- 2. the evidence call ---------------------------------------------------------------------------------------------------

def _layout(kind, clean=False):
    """hand-made chunk layouts: 1, 3 and 13 chunks of 40 rows that overlap by 10 (13: chunk ids 9 and 10 meet), and a random
    one of 1000-row chunks (two regions, the second with a start above 0), where a lane owns four columns; drafts with
    lower-case and, unless clean, N and IUPAC bytes, which no label spells"""
    rng = np.random.default_rng({"1": 1, "3": 3, "13": 13, "big": 99}[kind])

    def draft(n):
        d = np.frombuffer(mq.acgt(rng, n), np.uint8).copy()
        odd = rng.random(n) < 0.06
        if not clean:
            d[odd] = rng.choice(np.frombuffer(b"NnRy", np.uint8), int(odd.sum()))
        return d.tobytes()
    if kind in ("1", "3", "13"):
        lay = mq.Layout({"1": [(0, draft(30), {4: 2, 9: 1})], "3": [(0, draft(88), {7: 3, 61: 2})],
                         "13": [(0, draft(370), {100: 20, 250: 3})]}[kind], 40, 10)
        assert lay.n == int(kind)
        return lay
    ins = {int(p): int(rng.integers(1, 4)) for p in rng.choice(3_000, 200, replace=False)}
    return mq.Layout([(0, draft(3_000), ins), (50_000, draft(1_500), {50_700: 30})], 1000, 50)


def _random_counts(lay, seed):
    """counts uint16 [n, L, 10] and depth uint16 [n, L]: random; a base row's depth is the sum of its counts, an insert row
    carries its anchor's depth (of the same chunk where the anchor is there, else any larger number) and sometimes more reads
    than that, so that the clamp at 0 is met; the two copies of a shared row get different numbers; padding rows 0"""
    rng = np.random.default_rng(seed)
    n, L = lay.position.shape
    counts = rng.integers(0, 40, (n, L, 10)).astype(np.uint16)
    counts[rng.random((n, L, 10)) < 0.3] = 0
    counts[rng.random((n, L)) < 0.01] = 40_000              # ref = c[k] + c[4 + k] beyond 16 bits
    depth = np.minimum(counts.astype(np.int64).sum(axis=2), 65535).astype(np.uint16)
    for k in range(n):
        for j in range(L):
            if lay.index[k, j] > 0:
                anchor = depth[k, j - lay.index[k, j]] if j - lay.index[k, j] >= 0 else 300
                counts[k, j] = counts[k, j] // 4
                depth[k, j] = anchor if rng.random() < 0.8 else min(int(anchor), 3)
    pad = lay.position < 0
    counts[pad], depth[pad] = 0, 0
    return counts, depth


def _labels(lay, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "all":
        return lay.all_edited(60)
    lab, rq = lay.spelled(60)
    if kind == "none":
        return lab, rq
    n, L = lab.shape
    rq = rng.integers(0, 94, (n, L)).astype(np.uint8)
    if kind == "random":
        return rng.integers(0, 5, (n, L)).astype(np.uint8), rq
    # planted: edits in the first and last column of every chunk and on either side of every wave edge; every copy of a row
    # gets the edit, so the owner has it whichever chunk that is
    assert kind == "planted"
    cols = sorted({0, L - 1} | {c for e in range(64, L, 64) for c in (e - 1, e)})
    for k in range(n):
        for j in cols:
            p, x = int(lay.position[k, j]), int(lay.index[k, j])
            if p < 0:
                continue
            g = int(lay.region[k])
            r = lay.rows[g].index((p, x))
            lay.plant(lab, rq, g, r, ("sub", "del")[(k + j) % 2] if x == 0 else 1 + (p + x) % 4, int(rng.integers(0, 94)))
    return lab, rq


def _spans(lay):
    return list(zip(lay.ref_start.tolist(), lay.ref_end.tolist()))


def _want(lay, labels, rq, counts, depth):
    """the checker: records per region from the owned-column dictionary of tests/edits_ref.py, and beside each the evidence
    rule on the counts and depth of the OWNED copy of its row -> (records, evidence, region offsets)"""
    n, L = labels.shape
    rowid = np.arange(n * L).reshape(n, L)
    owner = er.region_dicts(lay.position, lay.index, lay.region, lay.chunk_id, labels, _spans(lay), rowid)
    dicts = er.region_dicts(lay.position, lay.index, lay.region, lay.chunk_id, labels, _spans(lay), rq)
    flat_c, flat_d = counts.reshape(-1, 10), depth.reshape(-1)
    recs, evs, off = [], [], [0]
    for g, d in enumerate(dicts):
        draft = lay.ref[int(lay.ref_off[g]):int(lay.ref_off[g + 1])].tobytes()
        prim = er.primitive_edits(d, draft, int(lay.ref_start[g]))
        rows = {key: (flat_c[rid], int(flat_d[rid])) for key, (_, rid) in owner[g].items()}
        recs += prim
        evs += cr.evidence_rows(prim, rows)
        off.append(len(recs))
    return recs, evs, off


def _upload(ctx, lay, counts, depth):
    dev = "cuda:%d" % ctx.device_id
    n = lay.n
    do = DevicePolishOut(max(n, 1), lay.L, lay.O, device=dev, depth=depth is not None, counts=counts is not None)
    for name in ("position", "index", "region", "chunk_id"):
        getattr(do, name)[:n].copy_(torch.from_numpy(np.array(getattr(lay, name))))
    if depth is not None:
        do.set_depth(depth)
    if counts is not None:
        do.set_row_counts(counts)
    t = {"rs": torch.from_numpy(np.array(lay.ref_start)).to(dev), "ro": torch.from_numpy(np.array(lay.ref_off)).to(dev),
         "ref": torch.from_numpy(np.array(lay.ref)).to(dev)}
    return do, t


def _dev_call(ctx, lay, labels, rq, counts, depth, capacity=None, evidence=True, ev_shift=0):
    """pv_polish_edits_evidence_dev (evidence False: pv_polish_edits_dev) on uploaded copies, every output pre-filled with a
    marker -> (region_edit_off, the whole record buffer's bytes, the whole evidence buffer's bytes, counts), or the error code
    the call itself returned. ev_shift: bytes by which the evidence pointer is moved off its alignment."""
    do, t = _upload(ctx, lay, counts, depth)
    n, L = lay.n, lay.L
    dev = do.images.device
    lab = torch.from_numpy(np.array(labels)).to(dev)
    drq = torch.from_numpy(np.array(rq)).to(dev) if rq is not None else None
    cap = n * L if capacity is None else capacity
    buf = torch.full((max(cap, 1), 16), MARK, dtype=torch.uint8, device=dev)
    ev = torch.full((max(cap, 1) + 1, 8), MARK, dtype=torch.uint8, device=dev)
    eoff = torch.full((lay.n_regions + 1,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((4,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    head = (do, n, lab.data_ptr(), drq.data_ptr() if drq is not None else 0, t["rs"].data_ptr(), t["ro"].data_ptr(), t["ref"].data_ptr(),
            lay.n_regions, eoff.data_ptr(), buf.data_ptr())
    try:
        if evidence:
            ctx.polish_edits_evidence_dev(*head, ev.data_ptr() + ev_shift, cap, cnt.data_ptr())
        else:
            ctx.polish_edits_dev(*head, cap, cnt.data_ptr())
    except _ffi.PepperHipError as e:
        return e.code
    ctx.synchronize()
    return eoff.cpu().numpy().tolist(), buf.cpu().numpy().tobytes(), ev.cpu().numpy().tobytes(), cnt.cpu().numpy().tolist()


def _host_out(lay, counts, depth):
    return types.SimpleNamespace(position=lay.position, index=lay.index, region=lay.region, chunk_id=lay.chunk_id, depth=depth,
                                 counts=counts)


UNTOUCHED = bytes([MARK]) * 8


@pytest.mark.parametrize("with_qual", [False, True], ids=["noqual", "qual"])
@pytest.mark.parametrize("labels_kind", ["planted", "random", "all", "none"])
@pytest.mark.parametrize("kind", ["1", "3", "13", "big"])
def test_evidence_equals_checker(hip_ctx, kind, labels_kind, with_qual):
    lay = _layout(kind, clean=labels_kind == "none")
    labels, rq = _labels(lay, labels_kind, 7)
    rq = rq if with_qual else None
    counts, depth = _random_counts(lay, 11)
    recs, evs, off = _want(lay, labels, rq, counts, depth)
    if labels_kind == "none":
        assert recs == []
    if labels_kind == "all":        # every owned column is an edit
        assert len(recs) == sum(len(d) for d in er.region_dicts(lay.position, lay.index, lay.region, lay.chunk_id, labels, _spans(lay)))
    if labels_kind == "planted" and kind in ("13", "big"):
        # some edit's owned row has a losing copy in the neighbouring chunk, with other counts
        shared = [e for e in recs if len(lay.where(*_row_of(lay, e))[0]) == 2]
        assert shared and any(not np.array_equal(counts[k0, j0], counts[k1, j1])
                              for (k0, k1), (j0, j1) in (lay.where(*_row_of(lay, e)) for e in shared))
    eoff, raw, raw_ev, cnt = _dev_call(hip_ctx, lay, labels, rq, counts, depth)
    total = len(recs)
    assert cnt == [total, 0, -1, 0] and eoff == off
    assert np.frombuffer(raw, EDIT_DTYPE)[:total].tolist() == recs
    assert [tuple(e) for e in np.frombuffer(raw_ev, EVIDENCE_DTYPE)[:total].tolist()] == evs          # record for record
    assert raw_ev[8 * total:] == UNTOUCHED * (len(raw_ev) // 8 - total)                                  # untouched beyond the total
    # edits, offsets and counters: byte for byte those of the edits call
    eoff0, raw0, _, cnt0 = _dev_call(hip_ctx, lay, labels, rq, None, None, evidence=False)
    assert (eoff0, raw0, cnt0) == (eoff, raw, cnt)
    # the host form
    h_off, h_recs, h_ev = hip_ctx.polish_edits_evidence(_host_out(lay, counts, depth), labels, lay.batch, rq, seq_length=lay.L,
                                                        seq_overlap=lay.O)
    assert h_off.tolist() == off and h_recs.tolist() == recs and [tuple(e) for e in h_ev.tolist()] == evs


def _row_of(lay, e):
    g = int(np.searchsorted(lay.ref_start, e[0], side="right") - 1)
    return g, lay.rows[g].index((e[0], e[1]))


def test_evidence_buffer_is_left_alone_under_every_status(hip_ctx):
    lay = _layout("13")
    labels, rq = _labels(lay, "random", 3)
    counts, depth = _random_counts(lay, 5)
    recs, _, off = _want(lay, labels, rq, counts, depth)
    # capacity short by one: offsets and the count are valid, nothing else is written
    eoff, raw, raw_ev, cnt = _dev_call(hip_ctx, lay, labels, rq, counts, depth, capacity=len(recs) - 1)
    assert cnt == [len(recs), _ffi.PV_ERR_CAPACITY, -1, 0] and eoff == off
    assert raw == bytes([MARK]) * len(raw) and raw_ev == bytes([MARK]) * len(raw_ev)
    assert _dev_call(hip_ctx, lay, labels, rq, None, None, capacity=len(recs) - 1, evidence=False)[3] == cnt
    # an owned label of 255
    owned = er.region_dicts(lay.position, lay.index, lay.region, lay.chunk_id, labels, _spans(lay), np.arange(labels.size).reshape(labels.shape))
    rid = sorted(owned[0].items())[len(owned[0]) // 2][1][1]
    bad = labels.copy()
    bad.reshape(-1)[rid] = 255
    eoff, raw, raw_ev, cnt = _dev_call(hip_ctx, lay, bad, rq, counts, depth)
    assert cnt[1:3] == [_ffi.PV_ERR_STATE, rid // lay.L] and raw_ev == bytes([MARK]) * len(raw_ev) and raw == bytes([MARK]) * len(raw)
    assert _dev_call(hip_ctx, lay, bad, rq, None, None, evidence=False)[3] == cnt
    # a broken layout: a chunk id out of sequence
    broken = types.SimpleNamespace(**vars(lay))
    broken.chunk_id = lay.chunk_id.copy()
    broken.chunk_id[5] = 7
    eoff, raw, raw_ev, cnt = _dev_call(hip_ctx, broken, labels, rq, counts, depth)
    assert cnt[1:3] == [_ffi.PV_ERR_INVALID, 5] and raw_ev == bytes([MARK]) * len(raw_ev) and raw == bytes([MARK]) * len(raw)
    assert _dev_call(hip_ctx, broken, labels, rq, None, None, evidence=False)[3] == cnt
    # the host form raises the same statuses
    for what, code in ((dict(labels=bad), _ffi.PV_ERR_STATE), (dict(edit_capacity=len(recs) - 1), _ffi.PV_ERR_CAPACITY)):
        ev = np.full(lay.n * lay.L, 0xEEEE, np.uint16).repeat(4).view(EVIDENCE_DTYPE)
        kw = dict(labels=labels, row_qual=rq, seq_length=lay.L, seq_overlap=lay.O, evidence=ev)
        kw.update(what)
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_edits_evidence(_host_out(lay, counts, depth), kw.pop("labels"), lay.batch, **kw)
        assert e.value.code == code and (ev.view(np.uint16) == 0xEEEE).all()


def test_the_call_refuses_missing_planes_and_a_misaligned_buffer(hip_ctx):
    lay = _layout("3")
    labels, rq = _labels(lay, "random", 3)
    counts, depth = _random_counts(lay, 5)
    assert _dev_call(hip_ctx, lay, labels, rq, None, depth) == _ffi.PV_ERR_INVALID          # counts == NULL
    assert _dev_call(hip_ctx, lay, labels, rq, counts, None) == _ffi.PV_ERR_INVALID         # depth == NULL
    assert _dev_call(hip_ctx, lay, labels, rq, counts, depth, ev_shift=4) == _ffi.PV_ERR_INVALID
    assert _dev_call(hip_ctx, lay, labels, rq, counts, depth, ev_shift=8)[3][1] == 0        # (moved by a whole record: fine)
    for c, d in ((None, depth), (counts, None)):
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_edits_evidence(_host_out(lay, c, d), labels, lay.batch, rq, seq_length=lay.L, seq_overlap=lay.O)
        assert e.value.code == _ffi.PV_ERR_INVALID


def test_graph_of_row_qual_stitch_qual_and_evidence(hip_ctx):
    """the three passes of --qualities --edits --evidence captured as one linear graph (one stream, no parallel branches);
    replays on refilled labels and acc equal the eager calls, and those the checker"""
    import qual_ref as qr
    lay = _layout("big")
    n, L, O = lay.n, lay.L, lay.O
    counts, depth = _random_counts(lay, 21)
    do, t = _upload(hip_ctx, lay, counts, depth)
    fills = []
    for s in range(2):
        rng = np.random.default_rng(60 + s)
        fills.append((rng.integers(0, 5, (n, L)).astype(np.uint8), (rng.random((n, L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)))
    lab_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    acc_d = torch.zeros((n, L, 5), dtype=torch.float32, device="cuda")
    rq_d = torch.zeros((n, L), dtype=torch.uint8, device="cuda")
    seq, qual = (torch.zeros(n * L, dtype=torch.uint8, device="cuda") for _ in range(2))
    buf = torch.zeros((n * L, 16), dtype=torch.uint8, device="cuda")
    ev = torch.zeros((n * L, 8), dtype=torch.uint8, device="cuda")
    roff, eoff = (torch.zeros(lay.n_regions + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    c_row, c_st, c_ed = (torch.zeros(4, dtype=torch.int64, device="cuda") for _ in range(3))
    st = hip_ctx.stream

    def passes():
        hip_ctx.polish_row_qual_dev(lab_d.data_ptr(), acc_d.data_ptr(), n, rq_d.data_ptr(), c_row.data_ptr(), L, O, stream=st)
        hip_ctx.polish_stitch_qual_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), t["rs"].data_ptr(), lay.n_regions, roff.data_ptr(),
                                       seq.data_ptr(), qual.data_ptr(), n * L, c_st.data_ptr(), stream=st)
        hip_ctx.polish_edits_evidence_dev(do, n, lab_d.data_ptr(), rq_d.data_ptr(), t["rs"].data_ptr(), t["ro"].data_ptr(),
                                          t["ref"].data_ptr(), lay.n_regions, eoff.data_ptr(), buf.data_ptr(), ev.data_ptr(), n * L,
                                          c_ed.data_ptr(), stream=st)

    def state():
        b, e = int(c_st[0].item()), int(c_ed[0].item())
        return (seq[:b].cpu().numpy().tobytes(), qual[:b].cpu().numpy().tobytes(), buf[:e].cpu().numpy().tobytes(),
                ev[:e].cpu().numpy().tobytes(), eoff.cpu().numpy().tolist(), c_st.cpu().numpy().tolist(), c_ed.cpu().numpy().tolist())

    eager = []
    for lab, acc in fills:
        lab_d.copy_(torch.from_numpy(lab)); acc_d.copy_(torch.from_numpy(acc))
        torch.cuda.synchronize()
        passes()
        hip_ctx.synchronize()
        eager.append(state())
        recs, evs, off = _want(lay, lab, qr.row_qual(lab, acc, O), counts, depth)
        assert np.frombuffer(eager[-1][2], EDIT_DTYPE).tolist() == recs and eager[-1][4] == off
        assert [tuple(e) for e in np.frombuffer(eager[-1][3], EVIDENCE_DTYPE).tolist()] == evs
    assert eager[0][3] != eager[1][3]
    with hip_ctx.graph_capture(st) as g:
        passes()
    for k in (1, 0, 1):
        lab_d.copy_(torch.from_numpy(fills[k][0])); acc_d.copy_(torch.from_numpy(fills[k][1]))
        for x in (rq_d, seq, qual, buf, ev, roff, eoff, c_row, c_st, c_ed):
            x.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert state() == eager[k], k
    g.close()


# ---- 3. the command ---------------------------------------------------------------------------------------------------------

class _RecordingChain(polish._DeviceChain):
    """polish's device chain, reading back what every launch's evidence pass was given, and the host copy of the very batch the
    builder took (realigned, decoded or selected as the run's flags have it)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.launches, self._batch = [], None

    def _summarize(self, db, sizes, host_batch):
        self._batch = host_batch()
        return super()._summarize(db, sizes, host_batch)

    def _labels_and_stitch(self, db, n, n_regions):
        res = super()._labels_and_stitch(db, n, n_regions)
        if n and self.evidence:
            d = self.dout
            self.launches.append(dict(position=d.position[:n].cpu().numpy(), index=d.index[:n].cpu().numpy(),
                                      region=d.region[:n].cpu().numpy(), chunk_id=d.chunk_id[:n].cpu().numpy(),
                                      labels=self.labels[:n].cpu().numpy(), depth=d.depth_numpy(n), counts=d.row_counts_numpy(n),
                                      batch=self._batch))
        return res


def _polish(t, hip_ctx, name, flags, chains, bam="reads.bam"):
    argv = ["-b", str(t / bam), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-t", "3", "-bs", "8", "-o", str(t / name)]

    def open_chain(device, shared, state_dict, dtype, **k):
        hip_ctx.load_p2(state_dict, dtype)
        chains.append(_RecordingChain(hip_ctx, **k))
        return chains[-1]
    assert polish.run(cli.polish_parser().parse_args(argv + flags), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(str(t / name))):
        if not f.endswith(".tbi"):
            out[f] = bamio.bgzf_read_all(str(t / name / f)) if f.endswith(".vcf.gz") else open(str(t / name / f), "rb").read()
    return out


def _vcf_lines(data: bytes):
    lines = data.decode().split("\n")
    assert lines[-1] == ""
    return [l for l in lines[:-1] if l.startswith("#")], [l.split("\t") for l in lines[:-1] if not l.startswith("#")]


def _same_but_info(with_flag: bytes, without: bytes):
    head, recs = _vcf_lines(with_flag)
    head0, recs0 = _vcf_lines(without)
    assert [l for l in head if not l.startswith("##INFO=")] == head0 and sum(l.startswith("##INFO=") for l in head) == 4
    first = min(i for i, l in enumerate(head) if l.startswith("##pepper_") or l.startswith("#CHROM"))
    assert all(l.startswith("##INFO=") for l in head[first - 4:first])              # in front of the pepper_* lines
    assert [r[:7] + ["."] for r in recs] == recs0 and {r[7] for r in recs0} == {"."}
    return recs


def _check_info(t, drafts, recs, launches):
    """every record's INFO against the checker: the labels read back, the checker's counts of the builder's own batch"""
    from pepper_thesis_amd.bamio import BamHandler, FastaHandler
    work, _ = polish.polish_work(FastaHandler(str(t / "ref.fa")), BamHandler(str(t / "reads.bam")), None)
    prim, evs = {c: [] for c in drafts}, {c: [] for c in drafts}
    w = 0
    for la in launches:
        b = la["batch"]
        want = cr.row_counts(b, la["position"], la["index"], la["region"])
        assert np.array_equal(la["counts"], want)                                   # the plane the evidence pass read
        assert np.array_equal(la["depth"], dr.row_depth(b, la["position"], la["index"], la["region"]))
        n, L = la["labels"].shape
        spans = list(zip(np.asarray(b.ref_start).tolist(), np.asarray(b.ref_end).tolist()))
        args = (la["position"], la["index"], la["region"], la["chunk_id"], la["labels"], spans)
        owner = er.region_dicts(*args, np.arange(n * L).reshape(n, L))
        flat_c, flat_d = want.reshape(-1, 10), la["depth"].reshape(-1)
        for g, d in enumerate(er.region_dicts(*args)):
            while (work[w].start, work[w].end) != spans[g]:
                w += 1
            contig = work[w].contig
            w += 1
            mine = er.primitive_edits(d, drafts[contig].encode(), 0)
            prim[contig] += mine
            evs[contig] += cr.evidence_rows(mine, {key: (flat_c[rid], int(flat_d[rid])) for key, (_, rid) in owner[g].items()})
    seen = 0
    for c in drafts:
        want_info = [cr.info_text(e) for e in cr.record_evidence(prim[c], evs[c])]
        assert [r[7] for r in recs if r[0] == c] == want_info, c
        seen += len(want_info)
    assert seen == len(recs) and seen > 100


@pytest.mark.parametrize("flags", [[], ["--qualities", "--realign", "--gpu_decode", "--min_depth", "3", "--min_qual", "20"]],
                         ids=["plain", "all_flags"])
def test_polish_evidence_end_to_end(inputs, hip_ctx, opts, flags):
    t, drafts = inputs
    opts(shared_device=1)
    tag = "all" if flags else "plain"
    chains = []
    without = _polish(t, hip_ctx, "ev_without_" + tag, flags + ["--edits"], chains)
    got = _polish(t, hip_ctx, "ev_with_" + tag, flags + ["--edits", "--evidence"], chains)
    assert [c.evidence for c in chains] == [False, True] and list(got) == list(without)
    for name in got:
        if not name.endswith(".vcf.gz"):
            assert got[name] == without[name], name                    # FASTA (and FASTQ) as without the flag
    recs = _same_but_info(got["_pepper_polished.edits.vcf.gz"], without["_pepper_polished.edits.vcf.gz"])
    assert len(chains[1].launches) > 1
    _check_info(t, drafts, recs, chains[1].launches)


def test_polish_evidence_per_haplotype_equals_the_split_files(hip_ctx, opts, hp_inputs):
    t = hp_inputs
    opts(shared_device=1)
    flags = ["--edits", "--evidence"]
    got = _polish(t, hip_ctx, "ev_hp", ["-hp"] + flags, [], bam="tagged.bam")
    plain = _polish(t, hip_ctx, "ev_hp_plain", ["-hp", "--edits"], [], bam="tagged.bam")
    assert list(got) == ["_pepper_polished_hp%d%s" % (h, x) for h in (1, 2) for x in (".edits.vcf.gz", ".fa")]
    infos = []
    for h in (1, 2):
        want = _polish(t, hip_ctx, "ev_split%d" % h, flags, [], bam="split%d.bam" % h)
        assert got["_pepper_polished_hp%d.fa" % h] == want["_pepper_polished.fa"] == plain["_pepper_polished_hp%d.fa" % h], h
        mine = got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode().split("\n")
        assert mine.count("##pepper_haplotype=%d" % h) == 1
        mine.remove("##pepper_haplotype=%d" % h)
        theirs = want["_pepper_polished.edits.vcf.gz"].decode().split("\n")
        assert mine == theirs and sum(bool(l) and not l.startswith("#") for l in theirs) >= 5, h
        recs = _same_but_info(got["_pepper_polished_hp%d.edits.vcf.gz" % h], plain["_pepper_polished_hp%d.edits.vcf.gz" % h])
        infos.append([r[7] for r in recs])
    assert infos[0] != infos[1]                                         # each pass's own reads
