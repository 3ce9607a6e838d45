"""pv_assess / pv_assess_errors and their device forms against the restatements on the cases of tests/assess_limits_cases.py:
the command's defaults (segment 1024, max_shift 8192), windows of 65 trips, more than 256 pairs, more anchors than k_as_chain
stages at a time, the ends of the segment range, the refusals that reach the device, and `pepper assess` without --segment and
--max_shift. Integers throughout: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_errors_cases as X  # noqa: E402
import assess_errors_ref as E  # noqa: E402
import assess_limits_cases as Z  # noqa: E402
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu


def seg_rows(segs):
    return np.stack([segs[f].astype(np.int64) for f in R.SEG_FIELDS], axis=1).reshape(-1, len(R.SEG_FIELDS))


def err_rows(errs):
    return np.stack([errs[f].astype(np.int64) for f in E.ERR_FIELDS], axis=1).reshape(-1, len(E.ERR_FIELDS))


def same_records(got, rows, what):
    assert got.shape == rows.shape, (what, got.shape, rows.shape)
    bad = np.nonzero((got != rows).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:5], got[bad[:3]], rows[bad[:3]])


def host_forms_equal_the_rule(ctx, x, what):
    """pv_assess on x's pairs = the rule; with error expectations, pv_assess_errors too, its shared outputs byte for byte
    those of pv_assess"""
    slots = Z.slots_of(x.pairs, x.L)
    counts = (C.c_int64 * 4)()
    segs, seg_off, totals = ctx.assess(x.pairs, x.L, x.shift, counts=counts)
    assert list(counts)[:3] == [len(x.rows), _ffi.PV_OK, slots], what
    assert np.array_equal(seg_off, x.off), what
    same_records(seg_rows(segs), x.rows, what)
    assert np.array_equal(totals, x.tot), what
    if not getattr(x, "errors", False):
        return
    counts = (C.c_int64 * 8)()
    e_segs, e_off, e_tot, errs, err_off, qhist = ctx.assess_errors(x.pairs, x.quals, x.L, x.shift, counts=counts)
    assert list(counts)[:3] == [len(x.rows), _ffi.PV_OK, slots] and list(counts)[4:] == [len(x.err_rows)] * 2 + [0, 0], what
    assert np.array_equal(err_off, x.err_off), what
    same_records(err_rows(errs), x.err_rows, what + " errors")
    assert (errs["pad"] == 0).all() and np.array_equal(qhist, x.hist), what
    assert e_segs.tobytes() == segs.tobytes() and np.array_equal(e_off, seg_off) and np.array_equal(e_tot, totals), what


@pytest.mark.parametrize("name", sorted(set(Z.CASES) - {"grid"}))
def test_device_equals_the_rule(hip_ctx, name):
    host_forms_equal_the_rule(hip_ctx, Z.expected(name), name)


@pytest.mark.parametrize("n_pairs", Z.GRID_PREFIXES)
def test_many_small_pairs(hip_ctx, n_pairs):
    x = Z.expected("grid")
    host_forms_equal_the_rule(hip_ctx, x if n_pairs == len(x.pairs) else Z.prefix(x, n_pairs), "grid %d" % n_pairs)


def dev_call(ctx, pairs, L, shift, seg_cap, quals=None, err_cap=None, scratch_bytes=None, a_off=None, raises=None):
    """pv_assess_dev, or with err_cap pv_assess_errors_dev, on buffers pre-filled with 7 -> every output as numpy. a_off: other
    offsets than the pairs' (the buffers stay those of the pairs); scratch_bytes: another size than the need to declare"""
    import torch
    n = len(pairs)
    true_a_off, b_off = Z.offsets_of(pairs)
    with_err = err_cap is not None
    need = (ctx.assess_errors_scratch_bytes if with_err else ctx.assess_scratch_bytes)(true_a_off, L)
    dev = lambda x, dt: torch.from_numpy(np.frombuffer(x, dt).copy()).cuda()  # noqa: E731
    full = lambda shape: torch.full(shape, 7, dtype=torch.int64, device="cuda")  # noqa: E731
    A = dev(b"".join(a for a, _ in pairs) + b"\0", np.uint8)
    B = dev(b"".join(b for _, b in pairs) + b"\0", np.uint8)
    ao = torch.from_numpy(np.ascontiguousarray(true_a_off if a_off is None else a_off, np.int64)).cuda()
    bo = torch.from_numpy(b_off).cuda()
    segs, so, tot = full((max(seg_cap, 1) + 1, 8)), full((n + 1,)), full((n, 16))
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0
    cnt = full((8 if with_err else 4,))
    out = dict(need=need)
    if with_err:
        Q = dev(b"".join(bytes(q) for q in quals) + b"\0", np.uint8)
        errs, eo, qh = full((err_cap + 1, 4)), full((n + 1,)), full((n, 94, 4))
    torch.cuda.synchronize()
    size = need if scratch_bytes is None else scratch_bytes
    try:
        if with_err:
            ctx.assess_errors_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), n, L, shift, seg_cap, segs.data_ptr(),
                                  so.data_ptr(), tot.data_ptr(), Q.data_ptr(), err_cap, errs.data_ptr(), eo.data_ptr(),
                                  qh.data_ptr(), scratch.data_ptr(), size, cnt.data_ptr())
        else:
            ctx.assess_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), n, L, shift, seg_cap, segs.data_ptr(),
                           so.data_ptr(), tot.data_ptr(), scratch.data_ptr(), size, cnt.data_ptr())
        assert raises is None, "the call should have returned %r" % raises
    except _ffi.PepperHipError as e:
        assert e.code == raises, (e.code, raises)
    ctx.synchronize()
    out.update(segs=segs.cpu().numpy(), so=so.cpu().numpy(), tot=tot.cpu().numpy(), cnt=cnt.cpu().numpy())
    if with_err:
        out.update(errs=errs.cpu().numpy(), eo=eo.cpu().numpy(), qh=qh.cpu().numpy())
    return out


def test_many_small_pairs_device_forms(hip_ctx):
    """1025 pairs, seg_capacity exactly the slot count: the scans over pairs with five pairs a thread"""
    x = Z.expected("grid")
    slots = Z.slots_of(x.pairs, x.L)
    assert slots == 1025 == len(x.rows)
    d = dev_call(hip_ctx, x.pairs, x.L, x.shift, slots)
    assert list(d["cnt"]) == [len(x.rows), _ffi.PV_OK, slots, d["need"]]
    same_records(seg_rows(d["segs"][:slots].view(np.dtype(_ffi.pv_assess_seg)).reshape(-1)), x.rows, "grid, device form")
    assert np.array_equal(d["so"], x.off) and np.array_equal(d["tot"], x.tot) and (d["segs"][slots:] == 7).all()
    e = dev_call(hip_ctx, x.pairs, x.L, x.shift, slots, x.quals, len(x.err_rows))
    assert list(e["cnt"]) == [len(x.rows), _ffi.PV_OK, slots, e["need"], len(x.err_rows), len(x.err_rows), 0, 0]
    assert e["need"] > d["need"]
    same_records(err_rows(e["errs"][:len(x.err_rows)].view(np.dtype(_ffi.pv_assess_error)).reshape(-1)), x.err_rows,
                 "grid, device form, errors")
    assert (e["errs"][len(x.err_rows):] == 7).all() and np.array_equal(e["eo"], x.err_off) and np.array_equal(e["qh"], x.hist)
    assert e["segs"].tobytes() == d["segs"].tobytes() and np.array_equal(e["so"], d["so"]) and np.array_equal(e["tot"], d["tot"])


def refusal_batch(which):
    """-> (pairs, quals, L, shift, number of error records)"""
    if which == "several_pairs":
        pairs, quals, shift, rows, _, _ = X.expected("several_pairs")
        assert len(pairs) == 12
        return pairs, quals, X.L, shift, len(rows)
    x = Z.expected("grid")
    return x.pairs, x.quals, x.L, x.shift, len(x.err_rows)


def poisoned(d, seg_cap, err_cap, with_err, status):
    assert d["cnt"][0] == 0 and d["cnt"][1] == status, d["cnt"]
    assert (d["segs"][:seg_cap] == -1).all() and (d["segs"][seg_cap:] == 7).all()   # all seg_capacity records, none beyond
    assert (d["so"] == -1).all() and (d["tot"] == -1).all()
    if with_err:
        assert list(d["cnt"][4:]) == [0, -1, 0, 0]
        assert (d["errs"][:err_cap] == -1).all() and (d["errs"][err_cap:] == 7).all()
        assert (d["eo"] == -1).all() and (d["qh"] == -1).all()


@pytest.mark.parametrize("with_err", [False, True], ids=["assess", "errors"])
@pytest.mark.parametrize("which", ["several_pairs", "grid"])
def test_a_scratch_below_the_head_is_limit_and_poisons(hip_ctx, which, with_err):
    """the host knows the status before any kernel has run (the scratch cannot hold the slot offsets): k_as_poison"""
    pairs, quals, L, shift, n_err = refusal_batch(which)
    slots = Z.slots_of(pairs, L)
    d = dev_call(hip_ctx, pairs, L, shift, slots, quals, n_err if with_err else None, scratch_bytes=256, raises=_ffi.PV_ERR_LIMIT)
    poisoned(d, slots, n_err, with_err, _ffi.PV_ERR_LIMIT)


@pytest.mark.parametrize("with_err", [False, True], ids=["assess", "errors"])
@pytest.mark.parametrize("which", ["several_pairs", "grid"])
def test_decreasing_offsets_are_invalid_and_poison(hip_ctx, which, with_err):
    """k_as_setup finds the step; the call itself returns PV_OK and every later kernel leaves on the status, so no sequence byte
    is read (the buffers are the valid batch's, whole)"""
    pairs, quals, L, shift, n_err = refusal_batch(which)
    slots = Z.slots_of(pairs, L)
    a_off = Z.offsets_of(pairs)[0]
    k = next(k for k in range(len(pairs) * 2 // 3, len(pairs)) if len(pairs[k - 1][0]) >= 2)
    a_off[k] = a_off[k - 1] - 1   # pair k-1 ends before it begins; every offset stays inside the buffer
    assert (np.diff(a_off) < 0).sum() == 1 and a_off.min() >= 0 and a_off.max() == a_off[-1]
    d = dev_call(hip_ctx, pairs, L, shift, slots, quals, n_err if with_err else None, a_off=a_off)
    poisoned(d, slots, n_err, with_err, _ffi.PV_ERR_INVALID)


@pytest.mark.parametrize("with_err", [False, True], ids=["assess", "errors"])
def test_capacity_one_short_at_many_pairs_is_limit_and_poisons(hip_ctx, with_err):
    """the loops that poison pair_seg_off, pair_err_off and qhist run more than one trip"""
    pairs, quals, L, shift, n_err = refusal_batch("grid")
    slots = Z.slots_of(pairs, L)
    d = dev_call(hip_ctx, pairs, L, shift, slots - 1, quals, n_err if with_err else None)
    poisoned(d, slots - 1, n_err, with_err, _ffi.PV_ERR_LIMIT)
    assert d["cnt"][2] == slots and d["cnt"][3] == d["need"]


def test_command_at_its_defaults(hip_ctx, tmp_path):
    """`pepper assess` with neither --segment nor --max_shift: the three tables are the rule's at 1024 / 8192"""
    from pepper_thesis_amd import pepper
    pol_a, truth_a, _ = Z.planted(271, 5000, 400)
    pol_b, truth_b, _ = Z.planted(272, 3200, 500)
    draft = [("ctgA", Z.planted(273, 5000, 70, truth=truth_a)[0]), ("ctgB", Z.planted(274, 3200, 70, truth=truth_b)[0])]
    polished = [("ctgA", pol_a), ("ctgB", pol_b.lower())]
    truth = [("ctgB", truth_b), ("ctgA", truth_a)]

    def fa(name, recs):
        p = tmp_path / name
        with open(p, "wb") as fh:
            for n, s in recs:
                fh.write(b">" + n.encode() + b"\n")
                for i in range(0, len(s), 70):
                    fh.write(s[i:i + 70] + b"\n")
        return str(p)
    prefix = str(tmp_path / "out" / "run")
    assert pepper.main(["assess", "-a", fa("polished.fa", polished), "-t", fa("truth.fa", truth), "-d", fa("draft.fa", draft),
                        "-o", prefix]) == 0
    exp_contig, exp_seg = R.tables(polished, truth, 1024, 8192)
    exp_draft, _ = R.tables(draft, truth, 1024, 8192)
    assert len(exp_seg.splitlines()) == 1 + (4 + 1) + (3 + 1)   # anchors every 1024 bases
    assert open(prefix + "_assess.tsv").read() == exp_contig
    assert open(prefix + "_assess.segments.tsv").read() == exp_seg
    assert open(prefix + "_assess_draft.tsv").read() == exp_draft
