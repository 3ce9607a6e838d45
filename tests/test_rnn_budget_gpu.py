"""GPU: every RNN kernel form at trained-scale weights against float64, under an error budget (tests/rnn_budget.py).

The suite's other RNN tests run PyTorch's default init, U(+-1/sqrt(H)): a contractive recurrence (decoder rms |h| 0.12) in
which a defect of the recurrent product is damped before it reaches an output, under float64 bars of 1e-4 that are ~300 x what
fp32 loses. Here every weight_hh and the decoders' weight_ih are multiplied by g in {1, 4} (g = 4: rms |h| 0.31, fp32 still
within 1e-5 of float64; tests/test_rnn_budget_cpu.py holds that, and that g = 8 is chaotic), and the bar is
    max |kernel - float64|  <=  8 x max(max |plain - float64|, 2^-23)
on rows at every tile position of the form (rnn_forms.sample_rows), where `plain` is the same rows in plain arithmetic of the
kernel's precision: numpy fp32 for the fp32 and split-6 kernels, the larger of that and the documented 3-term split products
(in float64) for the bf16x3 mode. The factor is no kernel measurement: summation order (MFMA K blocks against numpy's blocked
sums), hardware exp / rcp against libm and FMA contraction in the cell update may each double the loss. Rounding h to bf16 in
front of the recurrent product - one dropped term - sits 250 to 7000 x over `plain`, 3-term products without lo.w_hi 55 to 360 x
(the CPU test): two orders of magnitude of discrimination remain.
Beside the budget the suite's absolute bars stay asserted: 1e-4 on probabilities, accumulated softmax and the bf16x3 decoder
tap, 2e-5 on the fp32 taps, 1e-4 on the fp32 window operator's logits and hidden state. (The bf16x3 window operator has the
budget alone: its documented arithmetic is itself 1.3e-4 from float64 on the hidden state at g = 4 with a random carried-in
state.) Labels equal float64's wherever its top-two gap exceeds TIE. Every case asserts the plan's form and the profile names
of the launch, so no case can silently run another form.

Measured ratios, kernel error / plain error (MI355X, worst output of the case; the bar is 8):
  P1 (probs / enc / dec; bf16x3: probs / dec)        g = 1                 g = 4
    f32 rows16        B = 33                        1.39 / 1.69 / 2.27    2.28 / 0.92 / 1.62
    f32 rows32        B = 33                        1.58 / 1.70 / 2.02    1.28 / 1.06 / 1.88
    f32 split4        B = 33                        1.39 / 1.69 / 2.27    2.28 / 0.92 / 1.62
    f32 split2        B = 513                       1.79 / 1.85 / 2.25    1.19 / 1.43 / 1.96
    split-6           B = 260                       1.70 / 1.14 / 1.81    2.05 / 1.50 / 1.22
    bf16x3 mt 1       B = 260                       0.91 / 1.02           0.96 / 0.90
    bf16x3 mt 2       B = 4130 (k_tail_bf16)        0.98 / 0.98           1.29 / 0.99
  P2, 19 windows, B = 33 (acc: uniform / sparse images)
    f32 us                                          1.24 / 1.13           1.23 / 1.37
    f32 dsplit                                      1.04 / 1.18           1.15 / 1.16
    f32 wg16                                        1.04 / 1.31           1.15 / 1.21
    f32 wg32                                        1.15 / 1.15           1.01 / 1.06
    bf16x3 gru16                                    0.99 / 1.00           1.04 / 0.99
  P2 window operator (logits / hidden)
    f32 us, dsplit, wg16, wg32   B = 33             1.00-1.24 / 1.00-1.27 1.07-1.21 / 1.01-1.23
    bf16x3 rec, 32 rows          B = 2049           0.98 / 0.99           1.00 / 1.00
    bf16x3 rec, 64 rows          B = 8200           1.00 / 1.00           1.00 / 0.99
  P2 long carry, columns 900..999, g = 4: f32 us 0.86, bf16x3 gru16 0.91
The fp32 and split-6 kernels sit at 0.9 to 2.3 x numpy's fp32, the bf16x3 kernels at 0.9 to 1.3 x the documented 3-term
arithmetic (absolute, g = 4: 1.0e-5 on probabilities, 6.1e-5 on the decoder tap, 4.2e-5 on acc, 1.3e-4 on the window
operator's hidden state). No case exceeded the factor; no restatement of fast-math was needed on the plain side.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import rnn_budget as bud
import rnn_forms as rf
from pepper_thesis_amd import _ffi, runtime

pytestmark = pytest.mark.gpu
TOL = 1e-4          # probabilities, accumulated softmax, bf16x3 taps, fp32 logits / hidden state
TOL_TAPS = 2e-5     # fp32 layer taps
FFI_DTYPE = {rf.F32: _ffi.PV_DTYPE_F32, rf.BF16X3: _ffi.PV_DTYPE_BF16_INPUT_GEMM}


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def x1():
    return bud.p1_windows()


@pytest.fixture(scope="module")
def y2():
    return {"uniform": bud.p2_images(), "sparse": bud.p2_sparse_images()}


@pytest.fixture(scope="module")
def win():
    return bud.p2_window_inputs()


@pytest.fixture(scope="module")
def p1r(x1):
    return {g: bud.restated_p1(g, x1) for g in bud.GAINS}


@pytest.fixture(scope="module")
def p2r(y2):
    return {(g, kind): bud.restated_p2(g, im) for g in bud.GAINS for kind, im in y2.items()}


@pytest.fixture(scope="module")
def p2wr(win):
    return {g: bud.restated_p2_window(g, *win) for g in bud.GAINS}


def options_of(ctx):
    return {k: ctx.get_option(k) for k in rf.OPTION_NAMES}


def profiled(ctx, run):
    ctx.profile_begin()
    out = run()
    prof = ctx.profile_end()
    return out, Counter({k: n for k, (_, n) in prof.items()})


def context(load, weights, dtype, options):
    """a private context (the session's option fixture does not know every option set here)"""
    ctx = runtime.Context(0)
    getattr(ctx, load)(weights, FFI_DTYPE[dtype])
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def near(got, ref, bar, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    assert err <= bar, "%s: %.3g from float64 (bar %g)" % (what, err, bar)


@pytest.mark.parametrize("g", bud.GAINS)
@pytest.mark.parametrize("case", list(bud.P1_CASES))
def test_p1_within_budget(case, g, num_cu, x1, p1r):
    dtype, options, B, want = bud.P1_CASES[case]
    ctx = context("load_p1", bud.weights_p1(g), dtype, options)
    call = rf.p1_call(dtype, B, num_cu, options_of(ctx))
    assert len(call) == 1
    f = call[0][2]
    assert (f.chain, f.lstm, f.mt, f.tail) == want, f
    (probs, enc, dec), names = profiled(ctx, lambda: ctx.forward_p1(x1[:B], taps=True))
    ctx.close()
    assert names == f.names, (case, names)
    assert np.abs(probs.sum(1) - 1).max() < 1e-5
    rows = bud.p1_rows(call)
    ref = p1r[g](rows, "f64")
    plain = p1r[g](rows, "f32")
    outs = {"probs": (0, probs, TOL), "enc": (1, enc, TOL_TAPS), "dec": (2, dec, TOL_TAPS)}
    if f.chain == "bf16x3":
        t3 = p1r[g](rows, "3term_tail" if f.tail == "k_tail_bf16" else "3term")
        plain = [(a, b) for a, b in zip(plain, t3)]
        outs = {"probs": (0, probs, TOL), "dec": (2, dec, TOL)}
    what = "P1 %s g=%d B=%d" % (case, g, B)
    fails = []
    for name, (k, got, bar) in outs.items():
        try:
            bud.budget(got[rows], ref[k], plain[k], bud.FACTOR, "%s %s" % (what, name), rows)
            near(got[rows], ref[k], bar, "%s %s" % (what, name))
        except AssertionError as e:   # (every output is measured and printed before the first failure is raised)
            fails.append(str(e))
    assert not fails, "\n".join(fails)


def run_p2(case, cases, g, num_cu, nwin):
    dtype, options, B, want = cases[case]
    ctx = context("load_p2", bud.weights_p2(g), dtype, options)
    f = rf.p2_call(dtype, B, num_cu, options_of(ctx), nwin=nwin)
    assert (f.kind, f.rows) == want, f
    return ctx, dtype, B, f


def p2_plain(r, rows, dtype):
    plain = r(rows, "f32")
    if dtype == rf.BF16X3:
        plain = [(a, b) for a, b in zip(plain, r(rows, "3term"))]
    return plain


@pytest.mark.parametrize("g", bud.GAINS)
@pytest.mark.parametrize("case", list(bud.P2_CASES))
def test_p2_within_budget(case, g, num_cu, y2, p2r):
    """the 19-window call on uniform and on sparse images: accumulated softmax and labels"""
    ctx, dtype, B, f = run_p2(case, bud.P2_CASES, g, num_cu, rf.P2_NWIN)
    rows = bud.p2_rows(B, f, bud.P2_ROWS_CAP)
    fails = []
    for kind, images in y2.items():
        (labels, acc), names = profiled(ctx, lambda: ctx.forward_p2(images[:B], want_acc=True))
        assert names == f.names, (case, names)
        r = p2r[g, kind]
        l64, a64 = r(rows, "f64")
        what = "P2 %s g=%d B=%d %s images" % (case, g, B, kind)
        try:
            bud.budget(acc[rows], a64, p2_plain(r, rows, dtype)[1], bud.FACTOR, what + " acc", rows)
            near(acc[rows], a64, TOL, what + " acc")
            bud.labels_agree(labels[rows], a64, l64, what + " labels")
        except AssertionError as e:
            fails.append(str(e))
    ctx.close()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("g", bud.GAINS)
@pytest.mark.parametrize("case", list(bud.P2_WINDOW_CASES))
def test_p2_window_operator_within_budget(case, g, num_cu, win, p2wr):
    """one window with a random carried-in hidden state: logits and the hidden state handed on"""
    ctx, dtype, B, f = run_p2(case, bud.P2_WINDOW_CASES, g, num_cu, 1)
    x, h_in = win
    (logits, hidden), names = profiled(ctx, lambda: ctx.forward_p2_window(x[:B], h_in[:B]))
    ctx.close()
    assert names == f.names, (case, names)
    rows = bud.p2_rows(B, f, bud.P1_ROWS_CAP)
    ref, plain = p2wr[g](rows, "f64"), p2_plain(p2wr[g], rows, dtype)
    what = "P2 window %s g=%d B=%d" % (case, g, B)
    fails = []
    for k, (name, got) in enumerate((("logits", logits), ("hidden", hidden))):
        try:
            bud.budget(got[rows], ref[k], plain[k], bud.FACTOR, "%s %s" % (what, name), rows)
            if dtype == rf.F32:
                near(got[rows], ref[k], TOL, "%s %s" % (what, name))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", ["f32-us", "bf16x3-gru16"])
def test_p2_long_carry_within_budget(case, num_cu, y2, p2r):
    """g = 4, the last window's columns 900 to 999 of the 19-window call: eighteen hand-overs of the hidden state lie behind
    them"""
    g = 4
    ctx, dtype, B, f = run_p2(case, bud.P2_CASES, g, num_cu, rf.P2_NWIN)
    (labels, acc), names = profiled(ctx, lambda: ctx.forward_p2(y2["uniform"][:B], want_acc=True))
    ctx.close()
    assert names == f.names, (case, names)
    rows = bud.p2_rows(B, f, bud.P2_ROWS_CAP)
    r = p2r[g, "uniform"]
    l64, a64 = r(rows, "f64")
    plain = p2_plain(r, rows, dtype)[1]
    plain = tuple(p[:, 900:] for p in plain) if isinstance(plain, tuple) else plain[:, 900:]
    what = "P2 %s g=%d B=%d columns 900..999" % (case, g, B)
    bud.budget(acc[rows][:, 900:], a64[:, 900:], plain, bud.FACTOR, what + " acc", rows)
    near(acc[rows][:, 900:], a64[:, 900:], TOL, what + " acc")
    bud.labels_agree(labels[rows][:, 900:], a64[:, 900:], l64[:, 900:], what + " labels")
