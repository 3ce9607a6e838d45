"""GPU: pv_batch_select_hp[_dev], the device-side selection of a flat batch by haplotype (`polish -hp`), against the host
checker (tests/select_ref.py). Device form = host form = checker, byte for byte, on every output array; every output buffer is
filled with a sentinel first and every byte at and beyond the kept totals must still hold it. Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import select_ref as sel
from test_oracle_polish_ref import case_batch, load_golden, names
from pepper_thesis_amd import _ffi, realign
from pepper_thesis_amd.batch import merge_batches
from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut, DeviceSelectOut, SelectedDeviceBatch

pytestmark = pytest.mark.gpu
MARK = 0xEE
CHUNK = 4096          # reads per workgroup of the scans
LENS = [0, 1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 20001]


def _arrays(so):
    """every array of a DeviceSelectOut on the host, as bytes-comparable numpy arrays"""
    out = {f: t.cpu().numpy() for f, t in so.t.items()}
    out["cigar"] = out["cigar"].view(np.uint32)
    out["read_hp"], out["src_read"] = so.read_hp.cpu().numpy(), so.src_read.cpu().numpy()
    return out


def _dev_select(ctx, batch, h, caps=None, shift=None):
    """the device form on an uploaded copy, into buffers pre-filled with MARK -> (arrays, counts) or the error code of a call
    that was refused. shift: (bases, quals, cigar) byte offsets of the payload pointers into their buffers."""
    db = DeviceBatch(batch)
    cr, cb, cc = (batch.n_reads, batch.n_bases, batch.n_cigar) if caps is None else caps
    pad = 16 if shift else 0
    so = DeviceSelectOut(batch.n_regions, cr, cb + pad, cc + pad // 4, fill=MARK)
    if shift:
        so.c.base_capacity, so.c.cigar_capacity = cb, cc
        so.c.bases, so.c.quals, so.c.cigar = (so.t[f].data_ptr() + s for f, s in zip(("bases", "quals", "cigar"), shift))
    so.counts.fill_(-7)
    torch.cuda.synchronize()
    try:
        ctx.batch_select_hp_dev(db, h, so)
    except _ffi.PepperHipError as e:
        ctx.synchronize()
        assert (so.counts.cpu().numpy() == -7).all()
        return e.code, _arrays(so)
    ctx.synchronize()
    return _arrays(so), so.counts.cpu().numpy().tolist()


def _marked(a, start=0):
    return bool((a.reshape(-1).view(np.uint8)[start * a.itemsize:] == MARK).all())


def _check_prefixes(got, want, src, tag, shift=None):
    """got: the device arrays; want: the checker's batch. Every array holds the checker's values and MARK behind them."""
    k = want.n_reads
    for f, n in (("read_off", want.n_regions + 1), ("read_pos", k), ("read_flags", k), ("read_mapq", k), ("base_off", k + 1),
                 ("cigar_off", k + 1)):
        assert got[f][:n].tobytes() == getattr(want, f).tobytes(), (tag, f)
        assert _marked(got[f], n), (tag, f, "beyond")
    hp = np.zeros(k, np.int32) if want.read_hp is None else want.read_hp
    assert got["read_hp"][:k].tobytes() == hp.tobytes() and _marked(got["read_hp"], k), tag
    assert got["src_read"][:k].tobytes() == src.tobytes() and _marked(got["src_read"], k), tag
    for f, s in zip(("bases", "quals", "cigar"), shift or (0, 0, 0)):
        raw, w = got[f].view(np.uint8), getattr(want, f).view(np.uint8)
        assert raw[s:s + len(w)].tobytes() == w.tobytes(), (tag, f)
        assert (raw[:s] == MARK).all() and (raw[s + len(w):] == MARK).all(), (tag, f, "outside")


def _check(ctx, batch, h, tag="", host=True, shift=None):
    """device form = host form = checker -> the checker's (batch, src_read)"""
    want, src = sel.select(batch, h)
    got, counts = _dev_select(ctx, batch, h, shift=shift)
    assert counts == [want.n_reads, want.n_bases, want.n_cigar, _ffi.PV_OK], (tag, counts)
    _check_prefixes(got, want, src, tag, shift)
    if host:
        hb, hsrc = ctx.batch_select_hp(batch, h)
        for f in sel.READ_FIELDS:
            assert getattr(hb, f).tobytes() == getattr(want, f).tobytes(), (tag, "host", f)
        assert hsrc.tobytes() == src.tobytes() and (hb.read_hp is None) == (want.read_hp is None), tag
        assert hb.read_hp is None or hb.read_hp.tobytes() == want.read_hp.tobytes(), tag
    return want, src


def _tiny(n, tags, seed):
    """n reads of 1 to 3 bases and one cigar word in up to 7 regions"""
    rng = np.random.default_rng(seed)
    G = min(n, 7)
    cuts = np.sort(rng.integers(0, n + 1, G - 1))
    per = np.diff(np.concatenate([[0], cuts, [n]]))
    return sel.make_batch(rng.integers(1, 4, n), np.ones(n, np.int64), per, tags, seed)


# ---- 1. the scans' edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 8191, 8192, 8193, 3 * 8192 + 5])
def test_scan_edges(hip_ctx, n):
    rng = np.random.default_rng(n)
    b = _tiny(n, rng.integers(0, 4, n), n)
    for h in (1, 2):
        want, _ = _check(hip_ctx, b, h, "n=%d h=%d" % (n, h), host=n in (65, CHUNK + 1))
        assert n < 64 or 0 < want.n_reads < n
    b.read_hp = np.where(rng.random(n) < 0.5, 0, 2).astype(np.int32)          # all kept: the identity
    want, src = _check(hip_ctx, b, 2, "n=%d kept" % n, host=False)
    assert src.tolist() == list(range(n))
    for f in sel.READ_FIELDS:
        assert getattr(want, f).tobytes() == getattr(b, f).tobytes(), f
    b.read_hp = np.full(n, 3, np.int32)                                       # all dropped
    got, counts = _dev_select(hip_ctx, b, 1)
    assert counts == [0, 0, 0, _ffi.PV_OK] and not got["read_off"].any()
    assert got["base_off"][0] == 0 and got["cigar_off"][0] == 0 and _marked(got["base_off"], 1) and _marked(got["cigar_off"], 1)
    for f in ("read_pos", "read_flags", "read_mapq", "bases", "quals", "cigar", "read_hp", "src_read"):
        assert _marked(got[f]), f


# ---- 2. the gather's alignment -------------------------------------------------------------------------------------------

def _alignment_batch():
    """kept reads (tag 0 or 1) with dropped reads (tag 2) between them: the first 16 dropped reads are one base and one cigar
    word long and the kept reads behind them at least 16 bases and one word, so the bytes dropped in front of those run
    through 1 .. 16 and the words through 1 .. 16; then kept and dropped reads of every length of LENS. The batch's first and
    last reads are kept."""
    rng = np.random.default_rng(77)
    lens, clens, tags = [33], [2], [1]
    long = [v for v in LENS if v >= 16]
    for k in range(40):
        dl = 1 if k < 16 else LENS[(3 * k) % len(LENS)]
        lens += [dl, long[k % len(long)] if k < 16 else LENS[k % len(LENS)]]
        clens += [1 if k < 16 else int(rng.integers(0, 6)), 1 + k % 5 if k < 16 else int(rng.integers(0, 6))]
        tags += [2, int(rng.integers(0, 2))]
    lens += [0, 0, 17]
    clens += [0, 3, 5]
    tags += [2, 1, 0]                        # a dropped and a kept read without bases; the last read is kept
    n = len(lens)
    return sel.make_batch(lens, clens, [5, n - 25, 20], tags, 78)


def test_gather_alignment(hip_ctx):
    b = _alignment_batch()
    keep = sel.keep_mask(b.read_hp, b.n_reads, 1)
    lens, clens = np.diff(b.base_off), np.diff(b.cigar_off)
    dropped_b = np.cumsum(np.where(keep, 0, lens)) - np.where(keep, 0, lens)      # bytes dropped in front of each read
    dropped_c = np.cumsum(np.where(keep, 0, clens)) - np.where(keep, 0, clens)
    long_enough = keep & (lens >= 16)
    assert {int(v) % 16 for v in dropped_b[long_enough]} == set(range(16))        # whole 16-byte groups at every shift
    assert {int(v) % 4 for v in dropped_c[keep & (clens > 0)]} == set(range(4))
    assert keep[0] and keep[-1] and (keep & (lens == 0)).any() and (~keep & (lens == 0)).any()
    assert set(LENS) <= set(lens[keep].tolist()) and set(LENS) <= set(lens[~keep].tolist())
    want, _ = _check(hip_ctx, b, 1, "alignment h=1")
    assert want.n_bases > 3 * 20001
    _check(hip_ctx, b, 2, "alignment h=2")                 # the roles swapped: the long runs of one-base reads are kept


@pytest.mark.parametrize("shift", [(3, 5, 4), (15, 1, 12), (8, 16, 8)])
def test_destinations_that_are_not_16_byte_aligned(hip_ctx, shift):
    b = _alignment_batch()
    _check(hip_ctx, b, 1, "shift %s" % (shift,), host=False, shift=shift)


# ---- 3. regions ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 300])
def test_regions_emptied(hip_ctx, G):
    rng = np.random.default_rng(G)
    per = rng.integers(1, 9, G)
    n = int(per.sum())
    tags = rng.integers(0, 3, n)
    region_of = np.repeat(np.arange(G), per)
    for g in {0, G // 2, G - 1}:
        tags[region_of == g] = 2
    b = sel.make_batch(rng.integers(0, 40, n), rng.integers(0, 4, n), per, tags, G + 1)
    want, _ = _check(hip_ctx, b, 1, "G=%d" % G)
    empty = np.flatnonzero(np.diff(want.read_off) == 0)
    assert {0, G // 2, G - 1} <= set(empty.tolist()) and (G == 1 or want.n_reads > 0)
    full, _ = _check(hip_ctx, b, 2, "G=%d h=2" % G, host=False)
    assert (np.diff(full.read_off)[[0, G // 2, G - 1]] == per[[0, G // 2, G - 1]]).all()


# ---- 4. tags -------------------------------------------------------------------------------------------------------------

def test_tag_values_and_no_tags(hip_ctx):
    rng = np.random.default_rng(9)
    n = 500
    tags = rng.choice(np.array([0, 1, 2, 3, -1, 2**31 - 1], np.int64), n).astype(np.int32)
    b = sel.make_batch(rng.integers(0, 60, n), rng.integers(0, 5, n), [100, 0, 250, 150], tags, 10)
    for h in (1, 2, 3, 2**31 - 1):
        want, src = _check(hip_ctx, b, h, "tags h=%d" % h)
        assert set(tags[src].tolist()) == {0, h}
    b.read_hp = None                                       # read_hp = NULL: the identity, and the tags out are 0
    want, src = _check(hip_ctx, b, 1, "no tags")
    assert src.tolist() == list(range(n))
    for f in sel.READ_FIELDS:
        assert getattr(want, f).tobytes() == getattr(b, f).tobytes(), f


# ---- 5. statuses ---------------------------------------------------------------------------------------------------------

def _status_batch():
    rng = np.random.default_rng(21)
    n = 200
    return sel.make_batch(rng.integers(1, 50, n), rng.integers(1, 4, n), [50, 70, 80], rng.integers(0, 3, n), 22)


@pytest.mark.parametrize("short", [0, 1, 2])
def test_a_capacity_short_by_one(hip_ctx, short):
    b = _status_batch()
    want, _ = sel.select(b, 1)
    caps = [want.n_reads, want.n_bases, want.n_cigar]
    got, counts = _dev_select(hip_ctx, b, 1, caps=tuple(caps))                       # exactly enough
    assert counts == caps + [_ffi.PV_OK]
    caps[short] -= 1
    got, counts = _dev_select(hip_ctx, b, 1, caps=tuple(caps))
    assert counts == [want.n_reads, want.n_bases, want.n_cigar, _ffi.PV_ERR_CAPACITY]
    for f in ("bases", "quals", "cigar"):
        assert _marked(got[f]), f
    assert got["read_off"].tobytes() == want.read_off.tobytes()
    k = caps[0]                                                                      # the records that fit, nothing behind them
    assert got["read_pos"][:k].tobytes() == want.read_pos[:k].tobytes() and _marked(got["read_pos"], k)
    assert got["base_off"][:k].tobytes() == want.base_off[:k].tobytes()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.batch_select_hp(b, 1, capacities=tuple(caps))
    assert e.value.code == _ffi.PV_ERR_CAPACITY


@pytest.mark.parametrize("fault", ["base_off", "cigar_off", "read_off_end", "read_off_step"])
def test_malformed_offsets(hip_ctx, fault):
    """every offset stays inside its array, so a kernel that missed the check would still touch nothing outside them"""
    b = _status_batch()
    if fault == "base_off":
        b.base_off = b.base_off.copy()
        b.base_off[120] = b.base_off[119] - 1
    elif fault == "cigar_off":
        b.cigar_off = b.cigar_off.copy()
        b.cigar_off[100] = b.cigar_off[99] - 1
    elif fault == "read_off_end":
        b.read_off = b.read_off.copy()
        b.read_off[-1] -= 1
    else:
        b.read_off = np.array([0, 120, 50, 200], np.int64)
    got, counts = _dev_select(hip_ctx, b, 1)
    assert counts == [0, 0, 0, _ffi.PV_ERR_INVALID]
    for f, a in got.items():
        assert _marked(a), f
    if fault != "read_off_end":       # (the host form takes the number of reads from read_off itself)
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.batch_select_hp(b, 1)
        assert e.value.code == _ffi.PV_ERR_INVALID


def test_totals_beyond_the_arrays_are_malformed(hip_ctx):
    b = _status_batch()
    db = DeviceBatch(b)
    for field in ("n_bases", "n_cigar"):
        so = DeviceSelectOut(b.n_regions, b.n_reads, b.n_bases, b.n_cigar, fill=MARK)
        setattr(db, field, getattr(b, field) - 1)          # base_off[n_reads] > n_bases
        torch.cuda.synchronize()
        hip_ctx.batch_select_hp_dev(db, 1, so)
        hip_ctx.synchronize()
        assert so.counts.cpu().numpy().tolist() == [0, 0, 0, _ffi.PV_ERR_INVALID], field
        assert all(_marked(a) for a in _arrays(so).values())
        setattr(db, field, getattr(b, field))


def test_haplotype_0_is_refused_by_the_call(hip_ctx):
    b = _status_batch()
    for h in (0, -1):
        code, got = _dev_select(hip_ctx, b, h)
        assert code == _ffi.PV_ERR_INVALID and all(_marked(a) for a in got.values())
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.batch_select_hp(b, h)
        assert e.value.code == _ffi.PV_ERR_INVALID


def test_no_reads_and_no_regions(hip_ctx):
    b = sel.make_batch([], [], [0, 0], [], 1)
    got, counts = _dev_select(hip_ctx, b, 1)
    assert counts == [0, 0, 0, _ffi.PV_OK] and got["read_off"].tolist() == [0, 0, 0]
    b = sel.make_batch([], [], [], [], 1)
    got, counts = _dev_select(hip_ctx, b, 2)
    assert counts == [0, 0, 0, _ffi.PV_OK] and got["read_off"].tolist() == [0]


# ---- 6. downstream: the builder and the realigner on the selected batch -------------------------------------------------

CHUNK_FIELDS = ("images", "position", "index", "region", "chunk_id")
_G = load_golden()


@pytest.fixture(scope="module")
def golden_tagged():
    """the polisher's golden cases in one batch (those the realigner's window limit of 2047 columns admits), tags dealt by a
    fixed generator; -> (batch, realignment windows: the regions' own draft bytes)"""
    keys = [k for k in names(_G) if int((case_batch(_G, k).ref_end - case_batch(_G, k).ref_start + 1).max()) <= 2000]
    assert len(keys) >= 20
    b = merge_batches([case_batch(_G, k) for k in keys])
    b.read_hp = np.random.default_rng(31).choice(np.array([0, 1, 2, 3], np.int32), b.n_reads, p=[0.3, 0.3, 0.3, 0.1])
    g1, g2 = np.flatnonzero(np.diff(b.read_off) >= 2)[:2]          # one region emptied for each haplotype
    b.read_hp[b.read_off[g1]:b.read_off[g1 + 1]] = 2
    b.read_hp[b.read_off[g2]:b.read_off[g2 + 1]] = 1
    wins = [b.ref[b.ref_off[g]:b.ref_off[g] + int(b.ref_end[g] - b.ref_start[g]) + 1].tobytes() for g in range(b.n_regions)]
    return b, wins


def _realigned(ctx, db, n_reads, n_bases, n_cigar, qmax, wins):
    """pv_polish_realign_dev on a device batch -> (a device batch with the realigner's positions and cigars, its outputs)"""
    woff, win = realign.pack_windows(wins)
    d_woff, d_win = realign.device_windows(woff, win)
    ro = realign.DeviceRealignOut(n_reads, n_cigar + 4 * n_reads + n_bases // 8 + 16 + 2 * n_bases)
    torch.cuda.synchronize()
    ctx.polish_realign_dev(db, d_woff.data_ptr(), d_win.data_ptr(), qmax, ro)
    ctx.synchronize()
    total, status, n_realigned = (int(v) for v in ro.counts[:3].tolist())
    assert status == _ffi.PV_OK and n_realigned > 0
    c = _ffi.pv_batch_in()
    for f, _ in _ffi.pv_batch_in._fields_:
        setattr(c, f, getattr(db.c, f))
    c.read_pos, c.cigar_off, c.cigar = ro.read_pos.data_ptr(), ro.cigar_off.data_ptr(), ro.cigar.data_ptr()
    out = type("B", (), {})()
    out.c, out.n_reads, out.n_bases, out.n_cigar, out.n_ref_bytes, out.keep = c, n_reads, n_bases, total, db.n_ref_bytes, (db, ro)
    return out, (ro.read_pos[:n_reads].cpu().numpy(), ro.cigar_off[:n_reads + 1].cpu().numpy(), ro.cigar[:total].cpu().numpy())


def _chunks(ctx, db):
    dout = DevicePolishOut(128)
    ctx.polish_summarize_dev(db, dout)
    ctx.synchronize()
    n = dout.n_chunks()
    assert dout.status() == _ffi.PV_OK and 0 < n <= 128
    return [getattr(dout, f)[:n].cpu().numpy() for f in CHUNK_FIELDS]


@pytest.mark.parametrize("with_realign", [False, True], ids=["builder", "realign_builder"])
@pytest.mark.parametrize("h", [1, 2])
def test_downstream_equals_the_checkers_batch_uploaded_fresh(hip_ctx, golden_tagged, h, with_realign):
    b, wins = golden_tagged
    want, _ = sel.select(b, h)
    assert 0 < want.n_reads < b.n_reads and (np.diff(want.read_off) == 0).any()
    db = DeviceBatch(b)
    so = DeviceSelectOut(b.n_regions, b.n_reads, b.n_bases, b.n_cigar, fill=MARK)
    torch.cuda.synchronize()
    hip_ctx.batch_select_hp_dev(db, h, so)
    hip_ctx.synchronize()
    kept, n_bases, n_cigar, status = so.counts.cpu().numpy().tolist()
    assert (kept, n_bases, n_cigar, status) == (want.n_reads, want.n_bases, want.n_cigar, _ffi.PV_OK)
    selected, fresh = SelectedDeviceBatch(db, so, kept, n_bases, n_cigar), DeviceBatch(want)
    if with_realign:
        qmax = int(np.diff(b.base_off).max())              # the input's longest read is still a bound
        selected, got_r = _realigned(hip_ctx, selected, kept, n_bases, n_cigar, qmax, wins)
        fresh, want_r = _realigned(hip_ctx, fresh, kept, n_bases, n_cigar, qmax, wins)
        for a, w in zip(got_r, want_r):
            assert a.tobytes() == w.tobytes()
    got, exp = _chunks(hip_ctx, selected), _chunks(hip_ctx, fresh)
    for f, a, w in zip(CHUNK_FIELDS, got, exp):
        assert a.shape == w.shape and a.tobytes() == w.tobytes(), f
