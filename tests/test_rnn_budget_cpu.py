"""CPU: the ground tests/test_rnn_budget_gpu.py stands on (tests/rnn_budget.py), with the numbers printed (pytest -s).
  stability  for every (model, weight family, rows) the GPU tests use, on 256 CUs: the fp32 restatement within 1e-5 of float64
             on every compared output, P2 labels equal wherever the float64 top-two gap exceeds TIE. A family that fails this
             is chaotic, a budget means nothing there and it is not used: recurrent gain 8 fails it (asserted too).
  teeth      float64 arithmetic with h rounded to bf16 in front of every recurrent product - a 2^-9 relative defect, the size
             of a dropped h_lo.w_hi term - is at least 100 x the fp32 restatement's error, at gain 1 and 4, P1 and P2, and so
             fails `budget`; the 3-term restatement without lo.w_hi fails `budget` against the intact one.
  regime     at gain 4 the decoder's rms |h| is at least twice its value at gain 1."""
import numpy as np
import pytest

import rnn_budget as bud
import rnn_forms as rf
from oracle import rnn_oracle

STABLE = 1e-5


@pytest.fixture(scope="module")
def x1():
    return bud.p1_windows()


@pytest.fixture(scope="module")
def p1r(x1):
    return {g: bud.restated_p1(g, x1) for g in bud.GAINS}


@pytest.fixture(scope="module")
def p2r():
    y, ys = bud.p2_images(), bud.p2_sparse_images()
    return {(g, kind): bud.restated_p2(g, im) for g in bud.GAINS for kind, im in (("uniform", y), ("sparse", ys))}


@pytest.fixture(scope="module")
def p2wr():
    x, h = bud.p2_window_inputs()
    return {g: bud.restated_p2_window(g, x, h) for g in bud.GAINS}


def p1_case_rows():
    rows = set()
    for dtype, options, B, _ in bud.P1_CASES.values():
        rows.update(bud.p1_rows(rf.p1_call(dtype, B, bud.NUM_CU, options)))
    return sorted(rows)


def p2_case_rows(cases, cap, nwin):
    rows = set()
    for dtype, options, B, _ in cases.values():
        rows.update(bud.p2_rows(B, rf.p2_call(dtype, B, bud.NUM_CU, options, nwin=nwin), cap))
    return sorted(rows)


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


def test_trained_scale_touches_the_recurrent_and_decoder_input_weights_only():
    for w in (bud.synth.make_weights_p1(5, 2.0), bud.synth.make_weights_p2(17, 2.0)):
        s = bud.trained_scale(w, 4)
        assert set(s) == set(w)
        n = 0
        for k, v in w.items():
            scaled = "weight_hh_l0" in k or k.startswith(("decoder.weight_ih_l0", "gru_decoder.weight_ih_l0"))
            assert s[k].dtype == np.float32 and np.array_equal(s[k], v * np.float32(4) if scaled else v), k
            assert s[k] is not v
            n += scaled
        assert n == 6   # weight_hh of two layers and the decoder's weight_ih, two directions each
        assert all(np.array_equal(v, w[k]) for k, v in bud.trained_scale(w, 1).items())


def test_budget_bar_floor_and_message():
    ref = np.zeros((4, 3))
    plain = ref + 1e-6
    got = ref.copy()
    got[2, 1] = 7.9e-6
    assert bud.budget(got, ref, plain, 8, "under") == pytest.approx(7.9)
    got[2, 1] = 8.1e-6
    with pytest.raises(AssertionError, match="row 12 "):
        bud.budget(got, ref, plain, 8, "over", rows=[10, 11, 12, 13])
    # the largest plain error of a tuple counts; a plain error below FLOOR is raised to it
    assert bud.budget(got, ref, (plain, 2 * plain), 8, "two plains") == pytest.approx(4.05)
    got[2, 1] = 7 * bud.FLOOR
    bud.budget(got, ref, ref, 8, "floor")
    got[2, 1] = 9 * bud.FLOOR
    with pytest.raises(AssertionError):
        bud.budget(got, ref, ref, 8, "floor")


def test_own_recurrences_with_plain_products_equal_the_oracle(x1):
    """the copy of the two recurrences the 3-term restatement and the mutants run on is the oracle's arithmetic"""
    w1 = bud.weights_p1(4)
    for a, b in zip(bud._p1(bud.arith(w1, "plain"), x1[:3]), bud.p1(w1, x1[:3], "f64")):
        assert dist(a, b) < 1e-12
    w2 = bud.weights_p2(4)
    x, h = bud.p2_window_inputs()
    for a, b in zip(bud._p2_window(bud.arith(w2, "plain"), x[:2].astype(np.float64), h[:2].transpose(1, 0, 2).astype(np.float64)),
                    rnn_oracle.p2_window({k: v.astype(np.float64) for k, v in w2.items()}, x[:2].astype(np.float64),
                                         h[:2].transpose(1, 0, 2).astype(np.float64))):
        assert dist(a, b) < 1e-12
    l, acc = bud.p2(w2, bud.p2_images()[:1], "plain")
    lr, ar = bud.p2(w2, bud.p2_images()[:1], "f64")
    assert dist(acc, ar) < 1e-12 and np.array_equal(l, lr)


def test_split2_is_the_two_piece_rule():
    x = np.random.default_rng(0).standard_normal(4096) * np.logspace(-6, 3, 4096)
    hi, lo = bud.split2(x)
    assert np.abs(x - hi).max() <= np.abs(x).max() * 2.0 ** -8 and (np.abs(x - hi - lo) <= np.abs(x) * 2.0 ** -16).all()
    assert np.array_equal(hi, hi.astype(np.float32).view(np.uint32).__and__(0xFFFF0000).view(np.float32))   # hi is a bf16
    assert np.array_equal(lo, lo.astype(np.float32).view(np.uint32).__and__(0xFFFF0000).view(np.float32))


# ---- stability -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", bud.GAINS)
def test_stability_p1(g, p1r):
    rows = p1_case_rows()
    d = [dist(a, b) for a, b in zip(p1r[g](rows, "f32"), p1r[g](rows, "f64"))]
    print("\nP1 g=%d, %d rows: fp32 vs float64 probs %.2g enc %.2g dec %.2g" % ((g, len(rows)) + tuple(d)))
    assert max(d) <= STABLE, d


@pytest.mark.parametrize("kind", ["uniform", "sparse"])
@pytest.mark.parametrize("g", bud.GAINS)
def test_stability_p2(g, kind, p2r):
    rows = p2_case_rows(bud.P2_CASES, bud.P2_ROWS_CAP, rf.P2_NWIN)
    (l32, a32), (l64, a64) = p2r[g, kind](rows, "f32"), p2r[g, kind](rows, "f64")
    print("\nP2 g=%d %s images, %d chunks: fp32 vs float64 acc %.2g" % (g, kind, len(rows), dist(a32, a64)))
    assert dist(a32, a64) <= STABLE
    bud.labels_agree(l32, a64, l64, "fp32 labels")


@pytest.mark.parametrize("g", bud.GAINS)
def test_stability_p2_window(g, p2wr):
    rows = p2_case_rows(bud.P2_WINDOW_CASES, bud.P1_ROWS_CAP, 1)
    d = [dist(a, b) for a, b in zip(p2wr[g](rows, "f32"), p2wr[g](rows, "f64"))]
    print("\nP2 window g=%d, %d chunks: fp32 vs float64 logits %.2g hidden %.2g" % ((g, len(rows)) + tuple(d)))
    assert max(d) <= STABLE, d


def test_gain_8_is_out(x1):
    """the reason the family stops at 4: at gain 8 plain fp32 no longer stays within 1e-5 of float64"""
    w2 = bud.weights_p2(1)
    w2 = bud.trained_scale(w2, 8)
    y = bud.p2_images()[:2]
    d2 = dist(bud.p2(w2, y, "f32")[1], bud.p2(w2, y, "f64")[1])
    w1 = bud.trained_scale(bud.weights_p1(1), 8)
    rows = p1_case_rows()[:24]
    d1 = max(dist(a, b) for a, b in zip(bud.p1(w1, x1[rows], "f32"), bud.p1(w1, x1[rows], "f64")))
    print("\ng=8: fp32 vs float64 P2 acc %.2g, P1 (worst of probs / enc / dec) %.2g" % (d2, d1))
    assert d2 > STABLE and d1 > STABLE


# ---- teeth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", bud.GAINS)
def test_teeth_p1_h_rounded_to_bf16(g, p1r):
    rows = p1_case_rows()[:24]
    ref, plain, mut = p1r[g](rows, "f64"), p1r[g](rows, "f32"), p1r[g](rows, "hbf16")
    for k, name in enumerate(("probs", "enc", "dec")):
        ratio = dist(mut[k], ref[k]) / bud.plain_error(ref[k], plain[k])
        print("\nP1 g=%d %s: mutant %.2g, fp32 %.2g from float64: %.0f x" % (g, name, dist(mut[k], ref[k]), dist(plain[k], ref[k]), ratio))
        assert ratio >= 100, (name, ratio)
        with pytest.raises(AssertionError):
            bud.budget(mut[k], ref[k], plain[k], bud.FACTOR, "P1 g=%d mutant %s" % (g, name), rows)


@pytest.mark.parametrize("g", bud.GAINS)
def test_teeth_p2_h_rounded_to_bf16(g, p2r):
    rows = p2_case_rows(bud.P2_CASES, bud.P2_ROWS_CAP, rf.P2_NWIN)[:4]
    r = p2r[g, "uniform"]
    ref, plain, mut = r(rows, "f64")[1], r(rows, "f32")[1], r(rows, "hbf16")[1]
    ratio = dist(mut, ref) / bud.plain_error(ref, plain)
    print("\nP2 g=%d acc: mutant %.2g, fp32 %.2g from float64: %.0f x" % (g, dist(mut, ref), dist(plain, ref), ratio))
    assert ratio >= 100, ratio
    with pytest.raises(AssertionError):
        bud.budget(mut, ref, plain, bud.FACTOR, "P2 g=%d mutant acc" % g, rows)


@pytest.mark.parametrize("g", bud.GAINS)
def test_teeth_3term_without_lo_hi(g, p1r, p2r, p2wr):
    """the 3-term restatement is the bar of the bf16x3 mode: a kernel that drops lo.w_hi must not fit under it"""
    rows = p1_case_rows()[:24]
    ref, plain, mut = p1r[g](rows, "f64"), p1r[g](rows, "3term"), p1r[g](rows, "3term_drop")
    for k, name in ((0, "probs"), (2, "dec")):
        print("\nP1 g=%d %s: 3-term %.2g, without lo.w_hi %.2g from float64" % (g, name, dist(plain[k], ref[k]), dist(mut[k], ref[k])))
        with pytest.raises(AssertionError):
            bud.budget(mut[k], ref[k], plain[k], bud.FACTOR, "P1 g=%d 3-term without lo.w_hi %s" % (g, name), rows)
    rows = p2_case_rows(bud.P2_CASES, bud.P2_ROWS_CAP, rf.P2_NWIN)[:2]
    r = p2r[g, "uniform"]
    ref, plain, mut = r(rows, "f64")[1], r(rows, "3term")[1], r(rows, "3term_drop")[1]
    print("\nP2 g=%d acc: 3-term %.2g, without lo.w_hi %.2g from float64" % (g, dist(plain, ref), dist(mut, ref)))
    with pytest.raises(AssertionError):
        bud.budget(mut, ref, plain, bud.FACTOR, "P2 g=%d 3-term without lo.w_hi acc" % g, rows)
    rows = p2_case_rows(bud.P2_WINDOW_CASES, bud.P1_ROWS_CAP, 1)[:8]
    ref, plain, mut = p2wr[g](rows, "f64"), p2wr[g](rows, "3term"), p2wr[g](rows, "3term_drop")
    for k, name in enumerate(("logits", "hidden")):
        print("\nP2 window g=%d %s: 3-term %.2g, without lo.w_hi %.2g from float64" % (g, name, dist(plain[k], ref[k]), dist(mut[k], ref[k])))
        with pytest.raises(AssertionError):
            bud.budget(mut[k], ref[k], plain[k], bud.FACTOR, "P2 window g=%d 3-term without lo.w_hi %s" % (g, name), rows)


def test_3term_restatement_keeps_the_existing_bars(p1r, p2r):
    """the arithmetic the bf16x3 mode documents loses more than fp32 and still sits under the suite's 1e-4, at both gains"""
    rows = p1_case_rows()[:24]
    for g in bud.GAINS:
        ref, f32, t3, t3t = (p1r[g](rows, how) for how in ("f64", "f32", "3term", "3term_tail"))
        for k, name in ((0, "probs"), (2, "dec")):
            print("\nP1 g=%d %s: fp32 %.2g, 3-term %.2g, with the tail split %.2g" % (g, name, dist(f32[k], ref[k]), dist(t3[k], ref[k]), dist(t3t[k], ref[k])))
            assert dist(f32[k], ref[k]) < dist(t3[k], ref[k]) < 1e-4 and dist(t3t[k], ref[k]) < 1e-4


# ---- regime ----------------------------------------------------------------------------------------------------------
def test_regime_decoder_state_at_gain_4(p1r):
    rows = p1_case_rows()[:24]
    rms = {g: float(np.sqrt(np.mean(p1r[g](rows, "f64")[2] ** 2))) for g in bud.GAINS}
    print("\nP1 decoder rms |h|: g=1 %.3f, g=4 %.3f" % (rms[1], rms[4]))
    assert rms[4] >= 2 * rms[1]
