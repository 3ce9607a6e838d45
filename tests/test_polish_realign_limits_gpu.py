"""GPU: pv_polish_realign[_dev] at the kernels' own limits (realign_cases.limit_regions) against the host checker
(tests/realign_ref.py), which tests/test_polish_realign_cpu.py pins to the reference's aligner at these sizes. Every
comparison is integer equality; what a case is there for (a score of 8188, a band that doubled, a slot class, a word
count) is asserted from the checker's records before the kernel is looked at."""
import functools

import numpy as np
import pytest

import realign_cases as rc
import realign_ref as rr
from pepper_thesis_amd import _ffi, realign
from pepper_thesis_amd.batch import pack_regions
from test_polish_realign_gpu import _check_read

pytestmark = pytest.mark.gpu
SLOTS = (192 << 10, 1 << 20, 16 << 20)   # k_rl_band's slot classes below the whole pool


@functools.lru_cache(maxsize=None)
def _group(name):
    """-> {region name: (start, end, window, reads)} of one limit_regions group (built once, never changed)"""
    return {n: (s, e, w, reads) for n, s, e, w, reads in rc.limit_regions(name)}


@functools.lru_cache(maxsize=None)
def _expected(group, region, idx=None):
    """the checker's records of the reads idx (all when None) of one region, each read aligned once per session"""
    s, _, w, reads = _group(group)[region]
    return rr.realign_reads(s, w, reads if idx is None else [reads[k] for k in idx])


def _batch(parts):
    """parts: [(group, region, read indices or None)] -> (regions, windows, [records per region])"""
    regs, wins, exp = [], [], []
    for group, region, idx in parts:
        s, e, w, reads = _group(group)[region]
        regs.append(rc.as_region(s, e, w, reads if idx is None else [reads[k] for k in idx]))
        wins.append(w)
        exp.append(_expected(group, region, idx))
    return regs, wins, exp


def _run(ctx, regs, wins, **kw):
    woff, win = realign.pack_windows(wins)
    return ctx.polish_realign(pack_regions(regs), woff, win, **kw)


def _run_dev(ctx, regs, wins, capacity):
    """pv_polish_realign_dev on device-resident inputs -> (RealignResult without band, status)"""
    import torch
    from pepper_thesis_amd.device import DeviceBatch
    b = pack_regions(regs)
    dev = "cuda:%d" % ctx.device_id
    db = DeviceBatch(b, dev)
    d_woff, d_win = realign.device_windows(*realign.pack_windows(wins), dev)
    out = realign.DeviceRealignOut(b.n_reads, capacity, dev)
    torch.cuda.synchronize()
    ctx.polish_realign_dev(db, d_woff.data_ptr(), d_win.data_ptr(), int(np.diff(b.base_off).max()), out)
    ctx.synchronize()
    total, status, nre, ndr = out.counts.tolist()
    res = realign.RealignResult(out.read_pos.cpu().numpy(), out.cigar_off.cpu().numpy(),
                                out.cigar[:min(total, capacity)].cpu().numpy().view(np.uint32), out.score.cpu().numpy(),
                                out.ends.cpu().numpy(), out.state.cpu().numpy(), nre, ndr)
    return res, status


def _check_batch(res, regs, exp, tag):
    """state, score, ends, position, every cigar word, the band width, the offsets and the counts of a whole batch"""
    k, off = 0, [0]
    for reg, recs in zip(regs, exp):
        assert len(recs) == len(reg.reads)
        for j, (rec, read) in enumerate(zip(recs, reg.reads)):
            t = "%s: read %d (%d bases at %d)" % (tag, k, len(read.bases), read.pos - reg.ref_start)
            _check_read(res, k, rec, read, t)
            if res.band is not None:
                assert int(res.band[k]) == rec.band, t
            off.append(off[-1] + len(rec.cigar))
            k += 1
    assert k == len(res.state) == len(res.read_pos)
    assert res.cigar_off.tolist() == off and len(res.cigar) == off[-1], tag
    states = [rec.state for recs in exp for rec in recs]
    assert (res.n_realigned, res.n_dropped) == (states.count(rr.REALIGNED), states.count(rr.DROPPED)), tag


def _ends(rec):
    return rec.ref_begin, rec.ref_end, rec.query_begin, rec.query_end


def _spans(rec):
    return rec.ref_end - rec.ref_begin + 1, rec.query_end - rec.query_begin + 1


def _band_need(rec):
    """k_rl_band's scratch per read, restated: direction nibbles of the band (rows of ceil(min(2 w + 1, rspan) / 2) bytes,
    rounded up to 16 bytes) and one raw traceback word per step"""
    rspan, qspan = _spans(rec)
    row = (min(2 * rec.band + 1, rspan) + 1) // 2
    return ((qspan * row + 15) & ~15) + 4 * (qspan + rspan + 4)


@pytest.mark.parametrize("batch", ["all", "short"])
def test_query_length_sweep(hip_ctx, batch):
    """queries of 1 .. 16384 bases against one 2047-base window: all in one batch (the launch takes its 64 KB of LDS from
    the 16384-base query, strips of 256 rows; the short reads run with S = 1 inside it), then those of at most 64 bases
    alone (strip 1). Every read must be realigned, with a score above 255 where 4 x length allows one (64 bases and more)
    and with the full 4 x length below: 63 bases cannot score more than 252."""
    lens = [len(rd.bases) for rd in _group("sweep")["sweep"][3]]
    assert tuple(lens) == rc.SWEEP_LENGTHS
    idx = None if batch == "all" else tuple(k for k, n in enumerate(lens) if n <= 64)
    regs, wins, exp = _batch([("sweep", "sweep", idx)])
    qmax = max(len(rd.bases) for rd in regs[0].reads)
    assert (qmax + 63) // 64 == (256 if batch == "all" else 1) and len(wins[0]) == rc.MAX_WINDOW
    for rec, rd in zip(exp[0], regs[0].reads):
        n = len(rd.bases)
        assert rec.state == rr.REALIGNED, n
        assert rec.score > 255 if 4 * n > 255 else rec.score == 4 * n, (n, rec.score)
    _check_batch(_run(hip_ctx, regs, wins), regs, exp, "sweep " + batch)


def test_saturation(hip_ctx):
    """the largest score the 13-bit fields must hold, 4 x 2047 = 8188: the window against itself, the window in the middle
    of a 16384-base query, 5000 A against 2047 A; and a period-2 repeat, whose maxima tie across many lanes"""
    regs, wins, exp = _batch([("saturation", n, None) for n in ("full", "homopolymer", "period2")])
    alone, flanked = exp[0]
    assert (alone.score,) + _ends(alone) == (8188, 0, 2046, 0, 2046)
    assert (flanked.score,) + _ends(flanked) == (8188, 0, 2046, 7000, 9046)
    assert [len(rd.bases) for rd in regs[0].reads] == [2047, 16384]
    assert exp[1][0].score == 8188 and exp[2][0].score == 2400
    _check_batch(_run(hip_ctx, regs, wins), regs, exp, "saturation")


REFUSALS = {   # name: (the accepted side, the refused batch)
    "tail2048": ([("limits", "over_window", (2, 3))], [("limits", "over_window", (1, 2, 3))]),
    "tail2100": ([("limits", "over_window", (2,))], [("limits", "good", None), ("limits", "over_window", (0,))]),
    "query16385": ([("limits", "over_query", (1,))], [("limits", "over_query", (0, 1)), ("limits", "good", None)]),
}


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_both_sides_of_each_limit(hip_ctx, case, form):
    """a window tail of 2047 bases and a query of 16384 bases are aligned exactly (the read with the 2047-base tail lies
    in a 2100-base window and is taken once the reads before it are out of the batch); 2048 (and 2100) bases of tail and
    16385 bases of query are PV_ERR_LIMIT, raised by the host form with both limits in its message and written into the
    counts by the device form; the same context then aligns a good batch exactly"""
    s, _, w, reads = _group("limits")["over_window"]
    assert [len(w) - (rd.pos - s) for rd in reads] == [2100, 2048, 2047, 1600]
    assert [len(rd.bases) for rd in _group("limits")["over_query"][3]] == [16385, 16384]
    ok, refused = REFUSALS[case]
    good = [("limits", "good", None)]
    for parts in (ok, good):
        for recs in _batch(parts)[2]:
            assert all(r.state == rr.REALIGNED and r.score > 1 for r in recs)

    def exact(parts, tag):
        regs, wins, exp = _batch(parts)
        if form == "host":
            res = _run(hip_ctx, regs, wins)
        else:
            res, status = _run_dev(hip_ctx, regs, wins, sum(len(r.cigar) for recs in exp for r in recs))
            assert status == _ffi.PV_OK, tag
        _check_batch(res, regs, exp, "%s %s %s" % (case, form, tag))

    exact(ok, "accepted side")
    regs, wins, _ = _batch(refused)
    if form == "host":
        with pytest.raises(_ffi.PepperHipError) as e:
            _run(hip_ctx, regs, wins)
        assert e.value.code == _ffi.PV_ERR_LIMIT
        assert "query > 16384 bases" in str(e.value) and "window > 2047 bases" in str(e.value)
    else:
        _, status = _run_dev(hip_ctx, regs, wins, 4096)
        assert status == _ffi.PV_ERR_LIMIT
    exact(good, "after the refusal")


@pytest.mark.parametrize("period", sorted(rc.TIE_PERIODS))
def test_ties_at_depth(hip_ctx, period):
    """tandem repeats of period 1, 2, 3 and 7 under strips of 2, 3, 17 and 64 rows: the forward pass must take the first
    column and then the smallest row of a maximum that many lanes hold (partial last strips included), the reverse pass
    the first hit of the score, found before its early exit"""
    names = ["period%d_short" % period, "period%d_long" % period]
    regs, wins, exp = _batch([("ties%d" % period, n, None) for n in names])
    for reg, recs in zip(regs, exp):
        assert sorted({(len(rd.bases) + 63) // 64 for rd in reg.reads}) == sorted(rc.TIE_STRIPS)
        assert all(r.state == rr.REALIGNED for r in recs)
    # pure repeats longer than the window's own: every row of the right phase past the repeat's length holds the maximum
    assert sum(len(rd.bases) >= 48 + period + 16 and rec.score <= 4 * (48 + period + 2)
               for rd, rec in zip(regs[0].reads, exp[0])) >= 4
    _check_batch(_run(hip_ctx, regs, wins), regs, exp, "ties of period %d" % period)


def test_band_doubling_and_slot_classes(hip_ctx):
    """reads whose band starts at width 1 and doubles (an insertion and a deletion of the same length far apart), a read
    whose band is the whole window (1500 inserted bases), and with them one read in each scratch slot class of k_rl_band
    below the whole pool"""
    regs, wins, exp = _batch([("bands", "bands", None)])
    recs = exp[0]
    assert all(r.state == rr.REALIGNED for r in recs)
    for r in recs[:3]:
        assert _spans(r)[0] == _spans(r)[1]                 # banded_sw starts at |rspan - qspan| + 1 = 1
    assert [r.band for r in recs[:3]] == [4, 64, 128]      # 2, 6 and 7 doublings
    wide = recs[4]
    assert _spans(wide) == (2047, 3547) and 2 * wide.band + 1 >= 2047
    classes = {sum(_band_need(r) > s for s in SLOTS) for r in recs}
    assert {0, 1, 2} <= classes, sorted(_band_need(r) for r in recs)
    assert _band_need(wide) > SLOTS[1]                      # megabytes of direction bytes
    _check_batch(_run(hip_ctx, regs, wins), regs, exp, "bands")


def test_dense_cigars(hip_ctx):
    """more than 1000 cigar words per read (every third base substituted; every fourth base deleted): the words, the
    offsets and the count, and PV_ERR_CAPACITY with the words needed when the output is one word short"""
    regs, wins, exp = _batch([("dense", "dense", None)])
    assert all(r.state == rr.REALIGNED and len(r.cigar) > 1000 for r in exp[0])
    assert all(_spans(r)[0] >= 2000 for r in exp[0])
    need = sum(len(r.cigar) for r in exp[0])
    _check_batch(_run(hip_ctx, regs, wins), regs, exp, "dense")
    with pytest.raises(_ffi.PepperHipError) as e:
        _run(hip_ctx, regs, wins, cigar_capacity=need - 1)
    assert e.value.code == _ffi.PV_ERR_CAPACITY and ("need %d words" % need) in str(e.value)
    _check_batch(_run(hip_ctx, regs, wins, cigar_capacity=need), regs, exp, "dense at the exact capacity")
