"""pv_assess_errors / pv_assess_errors_dev against the restatement (tests/assess_errors_ref.py), record for record and bin for
bin, on the cases of tests/assess_errors_cases.py; what the call refuses and poisons; and `pepper assess --errors -q` end to end
against the restatement's text."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_errors_cases as X  # noqa: E402
import assess_errors_ref as E  # noqa: E402
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu
L = X.L


def err_rows(errs):
    return np.stack([errs[f].astype(np.int64) for f in E.ERR_FIELDS], axis=1).reshape(-1, len(E.ERR_FIELDS))


def same_records(got, rows, what):
    assert got.shape == rows.shape, (what, got.shape, rows.shape)
    bad = np.nonzero((got != rows).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:5], got[bad[:3]], rows[bad[:3]])


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_device_equals_the_rule(hip_ctx, name):
    pairs, quals, shift, rows, off, hist = X.expected(name)
    counts = (C.c_int64 * 8)()
    segs, seg_off, totals, errs, err_off, qhist = hip_ctx.assess_errors(pairs, quals, L, shift, counts=counts)
    assert list(counts)[1] == _ffi.PV_OK and list(counts)[4:] == [len(rows), len(rows), 0, 0]
    assert np.array_equal(err_off, off)
    same_records(err_rows(errs), rows, name)
    assert (errs["pad"] == 0).all()
    assert np.array_equal(qhist, hist)
    # segs, pair_seg_off and totals: byte for byte those of pv_assess
    p_segs, p_off, p_tot = hip_ctx.assess(pairs, L, shift)
    assert segs.tobytes() == p_segs.tobytes() and np.array_equal(seg_off, p_off) and np.array_equal(totals, p_tot)
    # the identities of the rule, on the device's own numbers
    assert np.array_equal(qhist[:, :, 0].sum(axis=1), totals[:, 4] + totals[:, 5] + totals[:, 6])
    assert np.array_equal(qhist[:, :, 1:].sum(axis=1), totals[:, 5:8])
    # the patch property on the device's records
    for p, (A, B) in enumerate(pairs):
        if totals[p, 2] == 0:
            recs = [dict(zip(E.ERR_FIELDS, (int(v) for v in x))) for x in err_rows(errs[int(err_off[p]):int(err_off[p + 1])])]
            assert E.apply_errors(A, recs) == B, (name, p)


@pytest.mark.parametrize("name", ["several_pairs", "deletions_at_the_ends"])
def test_without_qualities_every_qual_is_255(hip_ctx, name):
    pairs, quals, shift, rows, off, hist = X.expected(name)
    segs, seg_off, totals, errs, err_off, qhist = hip_ctx.assess_errors(pairs, None, L, shift)
    want = rows.copy()
    want[:, 8] = 255
    assert qhist is None and np.array_equal(err_off, off)
    same_records(err_rows(errs), want, name)


def test_default_capacity_grows_once(hip_ctx):
    # more records than (len A + len B) // 16 + 1024: pairs that are all errors
    pairs = [(b"", X.rnd(1, 90))] * 30 + [(X.rnd(2, 90), b"")] * 20
    rows, off, _ = E.errors_batch(pairs, L, 64)
    assert len(rows) == 2700 + 1800 and (2700 + 1800) // 16 + 1024 < len(rows)
    counts = (C.c_int64 * 8)()
    errs, err_off = hip_ctx.assess_errors(pairs, None, L, 64, counts=counts)[3:5]
    assert list(counts)[4:6] == [len(rows), len(rows)] and np.array_equal(err_off, off)
    same_records(err_rows(errs), np.where(np.arange(9) == 8, 255, rows), "grown")


def _dev_call(ctx, pairs, quals, shift, seg_cap, err_cap, scratch_delta=0, with_q=True, with_hist=True, err_shift=0):
    import torch
    n = len(pairs)
    a_off = np.zeros(n + 1, np.int64)
    b_off = np.zeros(n + 1, np.int64)
    a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
    b_off[1:] = np.cumsum([len(b) for _, b in pairs])
    need = ctx.assess_errors_scratch_bytes(a_off, L)
    assert need >= ctx.assess_scratch_bytes(a_off, L)
    dev = lambda x, dt: torch.from_numpy(np.frombuffer(x, dt).copy()).cuda()  # noqa: E731
    A = dev(b"".join(a for a, _ in pairs) + b"\0", np.uint8)
    B = dev(b"".join(b for _, b in pairs) + b"\0", np.uint8)
    Q = dev(b"".join(bytes(q) for q in quals) + b"\0", np.uint8)
    ao, bo = torch.from_numpy(a_off).cuda(), torch.from_numpy(b_off).cuda()
    segs = torch.full((max(seg_cap, 1), 8), 7, dtype=torch.int64, device="cuda")
    so = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    tot = torch.full((n, 16), 7, dtype=torch.int64, device="cuda")
    errs = torch.full((max(err_cap, 1) + 1, 4), 7, dtype=torch.int64, device="cuda")
    eo = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    qh = torch.full((n, 94, 4), 7, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0 and errs.data_ptr() % 8 == 0
    cnt = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.assess_errors_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), n, L, shift, seg_cap, segs.data_ptr(),
                          so.data_ptr(), tot.data_ptr(), Q.data_ptr() if with_q else 0, err_cap, errs.data_ptr() + err_shift,
                          eo.data_ptr(), qh.data_ptr() if with_hist else 0, scratch.data_ptr(), need + scratch_delta, cnt.data_ptr())
    ctx.synchronize()
    return dict(segs=segs.cpu().numpy(), so=so.cpu().numpy(), tot=tot.cpu().numpy(), errs=errs.cpu().numpy(), eo=eo.cpu().numpy(),
                qh=qh.cpu().numpy(), cnt=cnt.cpu().numpy(), need=need)


def test_device_form_equals_host_form(hip_ctx):
    pairs, quals, shift, rows, off, hist = X.expected("several_pairs")
    slots = sum(len(a) // L + 1 for a, _ in pairs)
    n_seg = int(X.totals_of(pairs, shift)[1][-1])   # segment records: at most one per slot
    d = _dev_call(hip_ctx, pairs, quals, shift, slots + 3, len(rows) + 5)
    assert list(d["cnt"]) == [n_seg, _ffi.PV_OK, slots, d["need"], len(rows), len(rows), 0, 0]
    got = d["errs"][:len(rows)].view(np.dtype(_ffi.pv_assess_error)).reshape(-1)
    same_records(err_rows(got), rows, "device form")
    assert (d["errs"][len(rows):] == 7).all() and (d["segs"][n_seg:] == 7).all()   # spare records stay as they were
    assert np.array_equal(d["eo"], off) and np.array_equal(d["qh"], hist)
    h = hip_ctx.assess_errors(pairs, quals, L, shift)
    assert h[3].tobytes() == d["errs"][:len(rows)].tobytes() and h[0].tobytes() == d["segs"][:n_seg].tobytes()
    assert np.array_equal(h[1], d["so"]) and np.array_equal(h[2], d["tot"]) and np.array_equal(h[4], d["eo"])
    assert np.array_equal(h[5], d["qh"])


def test_error_capacity_one_short_and_exact(hip_ctx):
    pairs, quals, shift, rows, off, hist = X.expected("several_pairs")
    slots = sum(len(a) // L + 1 for a, _ in pairs)
    p_segs, p_off, p_tot = hip_ctx.assess(pairs, L, shift)
    n_seg = len(p_segs)
    d = _dev_call(hip_ctx, pairs, quals, shift, slots, len(rows) - 1)
    assert list(d["cnt"]) == [n_seg, _ffi.PV_ERR_CAPACITY, slots, d["need"], 0, len(rows), 0, 0]
    assert (d["errs"] == 7).all()                                                     # no record is written
    assert d["segs"][:n_seg].tobytes() == p_segs.tobytes() and np.array_equal(d["so"], p_off) and np.array_equal(d["tot"], p_tot)
    assert np.array_equal(d["eo"], off) and np.array_equal(d["qh"], hist)             # every other output is valid
    d = _dev_call(hip_ctx, pairs, quals, shift, slots, len(rows))
    assert list(d["cnt"])[:2] == [n_seg, _ffi.PV_OK] and list(d["cnt"])[4:6] == [len(rows), len(rows)]
    assert (d["errs"][len(rows):] == 7).all()
    # the host form: the status, the need, errs untouched, the rest filled
    n = len(pairs)
    out = (np.zeros(slots, np.dtype(_ffi.pv_assess_seg)), np.zeros(n + 1, np.int64), np.zeros((n, 16), np.int64),
           np.full(len(rows) - 1, 7, np.int64).repeat(4).view(np.dtype(_ffi.pv_assess_error)), np.zeros(n + 1, np.int64),
           np.zeros((n, 94, 4), np.int64))
    counts = (C.c_int64 * 8)()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.assess_errors(pairs, quals, L, shift, err_capacity=len(rows) - 1, counts=counts, out=out)
    assert e.value.code == _ffi.PV_ERR_CAPACITY and counts[1] == _ffi.PV_ERR_CAPACITY and counts[5] == len(rows)
    assert (out[3].view(np.int64) == 7).all() and out[0][:n_seg].tobytes() == p_segs.tobytes() and np.array_equal(out[2], p_tot)
    assert np.array_equal(out[4], off) and np.array_equal(out[5], hist)


@pytest.mark.parametrize("short", ["seg_capacity", "scratch"])
def test_limit_poisons_every_output(hip_ctx, short):
    pairs, quals, shift, rows, off, hist = X.expected("several_pairs")
    n_seg = sum(len(a) // L + 1 for a, _ in pairs)   # slots
    cap = n_seg - 1 if short == "seg_capacity" else n_seg
    d = _dev_call(hip_ctx, pairs, quals, shift, cap, len(rows), scratch_delta=-1 if short == "scratch" else 0)
    assert list(d["cnt"]) == [0, _ffi.PV_ERR_LIMIT, n_seg, d["need"], 0, -1, 0, 0]
    assert (d["segs"][:cap] == -1).all() and (d["so"] == -1).all() and (d["tot"] == -1).all()
    assert (d["errs"][:len(rows)] == -1).all() and (d["errs"][len(rows):] == 7).all()   # all err_capacity records, none beyond
    assert (d["eo"] == -1).all() and (d["qh"] == -1).all()


def test_refused_arguments(hip_ctx):
    pairs, quals, shift, rows, off, hist = X.expected("deletions_at_the_ends")
    n_seg = len(pairs)
    for kw in (dict(with_q=False), dict(with_hist=False), dict(err_shift=4)):
        with pytest.raises(_ffi.PepperHipError) as e:
            _dev_call(hip_ctx, pairs, quals, shift, n_seg, len(rows), **kw)
        assert e.value.code == _ffi.PV_ERR_INVALID, kw
    bad = [q.copy() for q in quals]
    bad[2][5] = 94
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.assess_errors(pairs, bad, L, shift)
    assert e.value.code == _ffi.PV_ERR_INVALID and "94" in str(e.value)
    lib, h = hip_ctx.lib, hip_ctx.handle
    assert lib.pv_assess_errors(h, None, None, None, None, 1, 256, 64, 1, None, None, None, None, 0, None, None, None,
                                None) == _ffi.PV_ERR_INVALID
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.assess_errors([(b"ACGT", b"ACGT")], None, 250, 64)
    assert e.value.code == _ffi.PV_ERR_INVALID
    out = hip_ctx.assess_errors([], None, 256, 64)
    assert len(out[0]) == 0 and len(out[3]) == 0 and list(out[4]) == [0] and out[5] is None


def test_device_form_counts_a_quality_above_93_as_93(hip_ctx):
    pairs, quals, shift, rows, off, hist = X.expected("deletions_at_the_ends")
    loud = [np.where(q >= 60, q + 100, q).astype(np.uint8) for q in quals]
    rows2, off2, hist2 = E.errors_batch(pairs, L, shift, loud)
    assert hist2[:, 93].sum() > hist[:, 93].sum()
    d = _dev_call(hip_ctx, pairs, loud, shift, len(pairs), len(rows))
    same_records(err_rows(d["errs"][:len(rows)].view(np.dtype(_ffi.pv_assess_error)).reshape(-1)), rows2, "above 93")
    assert np.array_equal(d["qh"], hist2)


def test_command_end_to_end(hip_ctx, tmp_path, capfd):
    from pepper_thesis_amd import pepper
    pol_a, truth_a, where = X.planted(105, 2100, 300)
    truth_b = X.rnd(102, 500)
    draft = [("ctgA", X.planted(103, 2100, 60, truth=truth_a)[0]), ("ctgB", truth_b[:200] + truth_b[201:]), ("lonely", b"ACGTAC")]
    polished = [("ctgA", pol_a.lower()), ("ctgB", truth_b), ("lonely", b"ACGTAC"), ("void", b"")]
    truth = [("ctgB", truth_b), ("ctgA", truth_a[:1000].lower() + truth_a[1000:]), ("onlytruth", b"ACGT"), ("void", b"")]
    quals = {"ctgA": np.full(len(pol_a), 40, np.uint8), "ctgB": np.full(500, 30, np.uint8), "lonely": np.full(6, 10, np.uint8)}
    for _, a_pos in where:
        quals["ctgA"][a_pos] = 5

    def fa(name, recs):
        p = tmp_path / name
        with open(p, "wb") as fh:
            for n, s in recs:
                fh.write(b">" + n.encode() + b" a description\n")
                for i in range(0, len(s), 70):
                    fh.write(s[i:i + 70] + b"\n")
        return str(p)
    fq = tmp_path / "polished.fq"
    with open(fq, "wb") as fh:
        for n, s in polished[:3]:   # `void` is empty and may be missing
            fh.write(b"@" + n.encode() + b" x\n" + s.upper() + b"\n+\n" + bytes(quals[n] + 33) + b"\n")
    a, t, d_ = fa("polished.fa", polished), fa("truth.fa", truth), fa("draft.fa", draft)
    plain = str(tmp_path / "plain" / "run1")
    assert pepper.main(["assess", "-a", a, "-t", t, "-d", d_, "-o", plain, "--segment", "256", "--max_shift", "64"]) == 0
    prefix = str(tmp_path / "out" / "run1")
    rc = pepper.main(["assess", "-a", a, "-t", t, "-d", d_, "-q", str(fq), "--errors", "-o", prefix, "--segment", "256",
                      "--max_shift", "64"])
    assert rc == 0
    exp_err, exp_cal, total = E.error_tables(polished, truth, 256, 64, quals)
    exp_draft_err, _, _ = E.error_tables(draft, truth, 256, 64, None)
    assert open(prefix + "_assess.errors.tsv").read() == exp_err
    assert open(prefix + "_assess.calibration.tsv").read() == exp_cal
    assert open(prefix + "_assess_draft.errors.tsv").read() == exp_draft_err
    for tail in ("_assess.tsv", "_assess.segments.tsv", "_assess_draft.tsv"):
        assert open(prefix + tail).read() == open(plain + tail).read(), tail
    assert open(prefix + "_assess.tsv").read() == R.tables(polished, truth, 256, 64)[0]
    assert sorted(os.listdir(str(tmp_path / "out"))) == sorted("run1" + x for x in (
        "_assess.tsv", "_assess.segments.tsv", "_assess_draft.tsv", "_assess.errors.tsv", "_assess.calibration.tsv",
        "_assess_draft.errors.tsv"))
    assert sorted(os.listdir(str(tmp_path / "plain"))) == ["run1_assess.segments.tsv", "run1_assess.tsv", "run1_assess_draft.tsv"]
    # what the case was built to show: every planted error at Q5, nothing else wrong
    err_lines = [ln.split("\t") for ln in exp_err.splitlines()[1:]]
    assert len(err_lines) == len(where) and all(x[0] == "ctgA" and x[7] == "5" for x in err_lines)
    assert len(exp_draft_err.splitlines()) > 20 and all(ln.split("\t")[7] == "." for ln in exp_draft_err.splitlines()[1:])
    cal = [ln.split("\t") for ln in exp_cal.splitlines()[1:]]
    assert [x[:2] for x in cal] == [["ctgA", "5"], ["ctgA", "40"], ["ctgB", "30"], ["TOTAL", "5"], ["TOTAL", "30"], ["TOTAL", "40"]]
    assert cal[0][6] == str(len(where)) and cal[1][-1] == "inf" and E.calibrated_from(total) == 5   # a handful of errors in 2600 columns: QV 25 over all bases
    err = capfd.readouterr().err
    assert "calibration: from quality 5 up" in err
    # --errors alone: the list with '.' for the quality, no calibration table
    alone = str(tmp_path / "alone" / "x")
    assert pepper.main(["assess", "-a", a, "-t", t, "--errors", "-o", alone, "--segment", "256", "--max_shift", "64"]) == 0
    assert open(alone + "_assess.errors.tsv").read() == E.error_tables(polished, truth, 256, 64, None)[0]
    assert sorted(os.listdir(str(tmp_path / "alone"))) == ["x_assess.errors.tsv", "x_assess.segments.tsv", "x_assess.tsv"]
