"""pv_assess / pv_assess_dev against the rule's restatement (tests/assess_ref.py), integer for integer, at the smallest shapes
where the kernels can go wrong, and `pepper assess` end to end against the restatement's text."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu
L = 256


def rnd(seed, n):
    return bytes(b"ACGT"[x] for x in np.random.default_rng(seed).integers(0, 4, n))


def sparse(seed, a, every=90):
    """a with a substitution, a deletion and an insertion in turn about every `every` bases"""
    rng = np.random.default_rng(seed)
    out, pos, k = [], 0, 0
    while pos < len(a):
        nxt = min(len(a), pos + int(rng.integers(every // 2, every * 3 // 2)))
        out.append(a[pos:nxt])
        pos = nxt
        if pos >= len(a):
            break
        if k % 3 == 0:
            out.append(bytes([b"ACGT"[(b"ACGT".index(a[pos]) + 1) % 4]]))
            pos += 1
        elif k % 3 == 1:
            pos += 1
        else:
            out.append(bytes([b"ACGT"[(b"ACGT".index(a[pos]) + 2) % 4]]))
        k += 1
    return b"".join(out)


def with_n(a, k, upto):
    """an N at the first byte of the candidates t = 0 .. upto-1 of anchor k: the anchor is taken at t = upto"""
    b = bytearray(a)
    for t in range(upto):
        b[k * L + 32 * t] = ord("N")
    return bytes(b)


# name -> (pairs, max_shift, check(segs, totals) of what the case was built to hold)
def case_several_pairs():
    t = [rnd(1, 3000), rnd(2, 700), rnd(3, 200), b"", rnd(4, 1500), rnd(5, 256), rnd(6, 255), b""]
    pairs = [(sparse(10 + i, x), x) for i, x in enumerate(t)]
    pairs[7] = (b"", rnd(7, 50))      # an empty assembly against 50 truth bases: 50 deletions
    pairs.append((rnd(8, 120), b""))  # and the other way round: unaligned, 120 > 96

    def check(rows, off, tot):
        assert list(np.diff(off)) == [len(a) // L + 1 for a, _ in pairs]
        assert tot[3, 0] == 1 and tot[3, 4:8].sum() == 0 and tot[7, 7] == 50 and tot[8, 2] == 1 and tot[8, 10] == 120
        assert tot[:, 5:8].sum() > 40 and tot[:7, 2].sum() == 0
    return pairs, 64, check


def case_no_anchor():
    a = rnd(21, 97) * 31   # period 97: every 32-mer occurs many times inside the window, so no candidate is unique

    def check(rows, off, tot):
        assert len(rows) == 1 and rows[0, 3] == 3007 and tot[0, 13] == 0 and tot[0, 5:8].sum() > 5
    return [(sparse(23, a, 300), a)], 512, check


def case_pure_indels():
    t = rnd(31, 1400)
    t = with_n(with_n(t, 1, 7), 3, 5)
    # anchor 1 at 256 + 224 and anchor 2 at 512 are adjacent in the assembly; the truth holds 20 bases between them
    b = t[:512] + rnd(32, 20) + t[512:]
    # anchor 3 at 768 + 160 and anchor 4 at 1024: the truth lacks the 64 bases between them
    cut = 768 + 160 + 32
    b = b[:cut + 20] + b[cut + 20 + 64:]

    def check(rows, off, tot):
        shape = [(int(r[2]), int(r[3])) for r in rows]
        assert (0, 20) in shape and (64, 0) in shape, shape
        assert tot[0, 7] == 20 and tot[0, 6] == 64 and tot[0, 5] == 0 and tot[0, 2] == 0
    return [(t, b)], 128, check


def case_length_difference_limits():
    a = rnd(41, 150)
    x = rnd(42, 97)
    pairs = [(a, a[:90] + x[:96] + a[90:]), (a, a[:90] + x + a[90:]), (a[:90] + x[:96] + a[90:], a), (a[:90] + x + a[90:], a),
             (a, a + x[:96]), (x[:96] + a, a)]

    def check(rows, off, tot):
        assert [int(r[4]) for r in rows] == [0, 1, 0, 1, 0, 0]
        assert tot[0, 7] == 96 and tot[2, 6] == 96 and tot[1, 11] == 247 and tot[3, 10] == 247
    return pairs, 64, check


def case_band_edges():
    # d = +96 starts the path in band cell 15 and ends it in cell 111: 15 insertions ahead of a long matching stretch take
    # it down to cell 0; 112 deletions ahead of one, with 16 insertions behind, up to cell 127
    x, y, z = rnd(51, 10), rnd(52, 200), rnd(53, 10)
    ins, dele = rnd(54, 20), rnd(55, 20 + 96)
    pairs = [(x + ins[:15] + y + z, x + y + dele[:15 + 96] + z),   # down to cell 0
             (x + y + ins[:16] + z, x + dele[:112] + y + z),       # up to cell 127
             (x + ins[:20] + y + z, x + y + dele + z),             # 20 would leave the band: a dearer path inside it
             (x + ins[:14] + y + z, x + y + dele[:14 + 96] + z),   # 14: cell 1, no edge
             (x + y + ins[:15] + z, x + dele[:111] + y + z)]       # cell 126, no edge

    def check(rows, off, tot):
        assert [int(r[5]) for r in rows] == [1, 1, 0, 0, 0] and rows[2, 7] > 20
        assert [(int(r[7]), int(r[8]), int(r[9])) for r in rows[[0, 1, 3, 4]]] == [(0, 15, 111), (0, 16, 112), (0, 14, 110),
                                                                                  (0, 15, 111)]
    return pairs, 64, check


def case_seams():
    # single indels that walk the path over cells 63/64 (lanes 31/32) and back, one cell at a time, and over more seams
    a = rnd(61, 250)
    dels = a[:30] + a[31:60] + a[61:90] + a[91:]
    ins = a[:30] + b"T" + a[30:70] + b"G" + a[70:120] + b"C" + a[120:]
    both = a[:40] + a[42:100] + b"AC" + a[100:150] + a[153:200] + b"GTT" + a[200:]
    return [(dels, a), (a, dels), (ins, a), (a, ins), (both, a), (a, both)], 64, lambda rows, off, tot: None


def case_candidates():
    base = rnd(71, 600)
    low = with_n(base, 1, 2)                      # t = 0, 1 hold an N: anchor 1 at t = 2
    twice = bytearray(base)
    twice[224:256] = base[256:288]                # the 32-mer of t = 0 a second time, at the window's first position
    pre55, pre56 = rnd(72, 55) + base, rnd(73, 56) + base     # found at the window's last position / one past it
    lc = bytearray(base)                          # bytes the caller did not upper-case are not ACGT: t = 0 .. 2 are passed over
    for t in range(3):
        lc[256 + 32 * t + 31] = b"acgt"[t]
    pairs = [(low, low), (base, bytes(twice)), (base, pre55), (base, pre56), (base, base[56:]), (base, base[58:]),
             (bytes(lc), bytes(lc))]

    def check(rows, off, tot):
        found = [R.find_anchors(a, b, L, 32) for a, b in pairs]
        assert found[0][0] == (256 + 64, 256 + 64)
        assert found[1][0] == (288, 288)                                  # two hits at t = 0: rejected
        assert found[2][0] == (256, 311) and 256 * 655 // 600 + 32 == 311   # one hit, at the window's last position
        assert found[3][0][0] == 288                                      # one past the window: not seen
        assert found[4][0] == (256, 200) and 256 * 544 // 600 - 32 == 200   # at the window's first position
        assert found[5][0][0] == 288
        assert found[6][0] == (256 + 96, 256 + 96)
    return pairs, 32, check


def case_chain_drops():
    a = rnd(81, 1100)
    b = a[:200] + a[500:560] + a[200:500] + a[560:]   # anchor 2's 32-mer now lies before anchor 1's

    def check(rows, off, tot):
        assert tot[0, 13] == 4 and tot[0, 12] == 3 and len(rows) == 4
    return [(a, b)], 512, check


def case_homopolymers():
    rng = np.random.default_rng(91)
    runs = b"".join(bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(1, 7)) for _ in range(300))
    t = runs[:900]
    a = bytearray(t)
    for p in range(850, 20, -46):   # one base fewer or one more inside whatever run is there, and a substitution in turn
        if p % 3 == 0:
            del a[p]
        elif p % 3 == 1:
            a.insert(p, a[p])
        else:
            a[p] = b"ACGT"[(b"ACGT".index(a[p]) + 1) % 4]
    at = b"AT" * 200

    def check(rows, off, tot):
        assert tot[0, 8] > 2 and tot[0, 9] > 2 and tot[1, 7] == 2 and tot[2, 6] == 2
    return [(bytes(a), t), (at[:-2], at), (at, at[:-2])], 64, check


CASES = {f.__name__[5:]: f for f in (case_several_pairs, case_no_anchor, case_pure_indels, case_length_difference_limits,
                                     case_band_edges, case_seams, case_candidates, case_chain_drops, case_homopolymers)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case, and what the rule gives for it (computed once, checked against what the case was built for)"""
    pairs, shift, check = CASES[name]()
    rows, off, tot = R.assess_batch(pairs, L, shift)
    check(rows, off, tot)
    for r in (rows, off, tot):
        r.setflags(write=False)
    return pairs, shift, rows, off, tot


def seg_rows(segs):
    return np.stack([segs[f].astype(np.int64) for f in R.SEG_FIELDS], axis=1).reshape(-1, len(R.SEG_FIELDS))


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_rule(hip_ctx, name):
    pairs, shift, rows, off, tot = expected(name)
    counts = (C.c_int64 * 4)()
    segs, seg_off, totals = hip_ctx.assess(pairs, L, shift, counts=counts)
    assert list(counts)[:3] == [len(rows), _ffi.PV_OK, sum(len(a) // L + 1 for a, _ in pairs)]
    assert np.array_equal(seg_off, off)
    got = seg_rows(segs)
    bad = np.nonzero((got != rows).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:5], got[bad[:3]], rows[bad[:3]])
    assert np.array_equal(totals, tot)


def _dev_call(ctx, pairs, shift, cap, scratch_delta=0):
    import torch
    n = len(pairs)
    a_off = np.zeros(n + 1, np.int64)
    b_off = np.zeros(n + 1, np.int64)
    a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
    b_off[1:] = np.cumsum([len(b) for _, b in pairs])
    need = ctx.assess_scratch_bytes(a_off, L)
    dev = lambda x, dt: torch.from_numpy(np.frombuffer(x, dt).copy()).cuda()  # noqa: E731
    A = dev(b"".join(a for a, _ in pairs) + b"\0", np.uint8)
    B = dev(b"".join(b for _, b in pairs) + b"\0", np.uint8)
    ao, bo = torch.from_numpy(a_off).cuda(), torch.from_numpy(b_off).cuda()
    segs = torch.full((max(cap, 1), 8), 7, dtype=torch.int64, device="cuda")
    so = torch.full((n + 1,), 7, dtype=torch.int64, device="cuda")
    tot = torch.full((n, 16), 7, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0
    cnt = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.assess_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), n, L, shift, cap, segs.data_ptr(), so.data_ptr(),
                   tot.data_ptr(), scratch.data_ptr(), need + scratch_delta, cnt.data_ptr())
    ctx.synchronize()
    return segs.cpu().numpy(), so.cpu().numpy(), tot.cpu().numpy(), cnt.cpu().numpy(), need


def test_device_form_equals_host_form(hip_ctx):
    pairs, shift, rows, off, tot = expected("several_pairs")
    cap = int(off[-1]) + 3   # spare records stay as they were
    segs, so, totals, cnt, need = _dev_call(hip_ctx, pairs, shift, cap)
    assert list(cnt) == [len(rows), _ffi.PV_OK, len(rows), need]
    got = seg_rows(segs[:len(rows)].view(np.dtype(_ffi.pv_assess_seg)).reshape(-1))
    assert np.array_equal(got, rows) and np.array_equal(so, off) and np.array_equal(totals, tot)
    assert (segs[len(rows):] == 7).all()
    h_segs, h_off, h_tot = hip_ctx.assess(pairs, L, shift)
    assert h_segs.tobytes() == segs[:len(rows)].tobytes() and np.array_equal(h_off, so) and np.array_equal(h_tot, totals)


def test_capacity_one_short_is_limit_and_poisons(hip_ctx):
    pairs, shift, rows, off, tot = expected("several_pairs")
    cap = int(off[-1]) - 1
    segs, so, totals, cnt, need = _dev_call(hip_ctx, pairs, shift, cap)
    assert list(cnt) == [0, _ffi.PV_ERR_LIMIT, cap + 1, need]
    assert (segs == -1).all() and (so == -1).all() and (totals == -1).all()
    out = (np.zeros(cap, np.dtype(_ffi.pv_assess_seg)), np.zeros(len(pairs) + 1, np.int64), np.zeros((len(pairs), 16), np.int64))
    counts = (C.c_int64 * 4)()
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.assess(pairs, L, shift, seg_capacity=cap, counts=counts, out=out)
    assert e.value.code == _ffi.PV_ERR_LIMIT and counts[1] == _ffi.PV_ERR_LIMIT and counts[2] == cap + 1
    assert out[0].tobytes() == b"\xff" * (64 * cap) and (out[1] == -1).all() and (out[2] == -1).all()


def test_scratch_one_short_is_limit_and_poisons(hip_ctx):
    pairs, shift, rows, off, tot = expected("several_pairs")
    cap = int(off[-1])
    segs, so, totals, cnt, need = _dev_call(hip_ctx, pairs, shift, cap, scratch_delta=-1)
    assert list(cnt) == [0, _ffi.PV_ERR_LIMIT, cap, need]
    assert (segs == -1).all() and (so == -1).all() and (totals == -1).all()


def test_refused_arguments(hip_ctx):
    pairs = [(b"ACGT", b"ACGT")]
    for kw in (dict(segment=250), dict(segment=128), dict(segment=65568), dict(max_shift=31), dict(max_shift=1048577)):
        args = dict(segment=256, max_shift=64)
        args.update(kw)
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.assess(pairs, **args)
        assert e.value.code == _ffi.PV_ERR_INVALID
    assert hip_ctx.lib.pv_assess(hip_ctx.handle, None, None, None, None, 1, 256, 64, 1, None, None, None, None) == _ffi.PV_ERR_INVALID
    segs, off, tot = hip_ctx.assess([], 256, 64)
    assert len(segs) == 0 and list(off) == [0] and tot.shape == (0, 16)


def test_command_end_to_end(hip_ctx, tmp_path, capfd):
    from pepper_thesis_amd import pepper
    truth_a, truth_b = rnd(101, 2100), rnd(102, 500)
    draft = [("ctgA", sparse(103, truth_a, 60)), ("ctgB", sparse(104, truth_b, 60)), ("lonely", b"ACGTAC")]
    polished = [("ctgA", sparse(105, truth_a, 400).lower()), ("ctgB", truth_b), ("lonely", b"ACGTAC")]
    truth = [("ctgB", truth_b), ("ctgA", truth_a[:1000].lower() + truth_a[1000:]), ("onlytruth", b"ACGT")]

    def fa(name, recs):
        p = tmp_path / name
        with open(p, "wb") as fh:
            for n, s in recs:
                fh.write(b">" + n.encode() + b" a description\n")
                for i in range(0, len(s), 70):
                    fh.write(s[i:i + 70] + b"\n")
        return str(p)
    prefix = str(tmp_path / "out" / "run1")
    rc = pepper.main(["assess", "-a", fa("polished.fa", polished), "-t", fa("truth.fa", truth), "-d", fa("draft.fa", draft),
                      "-o", prefix, "--segment", "256", "--max_shift", "64"])
    assert rc == 0
    exp_contig, exp_seg = R.tables(polished, truth, 256, 64)
    exp_draft, _ = R.tables(draft, truth, 256, 64)
    assert open(prefix + "_assess.tsv").read() == exp_contig
    assert open(prefix + "_assess.segments.tsv").read() == exp_seg
    assert open(prefix + "_assess_draft.tsv").read() == exp_draft
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["run1_assess.segments.tsv", "run1_assess.tsv", "run1_assess_draft.tsv"]
    # the same tables when every pair is a launch of its own (a budget no pair fits)
    from pepper_thesis_amd import assess
    assert assess.tables(hip_ctx, polished, truth, 256, 64, budget=1)[:2] == (exp_contig, exp_seg)
    lines = {ln.split("\t")[0]: ln.rstrip("\n").split("\t") for ln in exp_contig.splitlines()}
    assert lines["ctgB"][-2:] == ["1.000000", "inf"] and lines["lonely"][1] == "unpaired" and lines["onlytruth"][1] == "unpaired"
    assert float(lines["TOTAL"][-1]) > float({ln.split("\t")[0]: ln.split("\t") for ln in exp_draft.splitlines()}["TOTAL"][-1])
    err = capfd.readouterr().err
    assert "lonely is only in the assembly" in err and "onlytruth is only in the truth" in err and "QV" in err and "->" in err
    # the polished assembly equal to the truth: no errors at all
    rc = pepper.main(["assess", "-a", fa("same.fa", [("ctgA", truth_a), ("ctgB", truth_b)]), "-t", fa("truth.fa", truth[:2]),
                      "-o", str(tmp_path / "same")])
    assert rc == 0
    total = open(str(tmp_path / "same") + "_assess.tsv").read().splitlines()[-1].split("\t")
    assert total[:2] == ["TOTAL", "total"] and total[4:9] == ["2600", "2600", "0", "0", "0"] and total[-2:] == ["1.000000", "inf"]
