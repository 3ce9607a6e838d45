"""Test helper (no tests here): trained-scale RNN weights and an error budget against float64.

Weights. synth.make_weights_p1/p2 draw every LSTM/GRU tensor from PyTorch's default U(+-1/sqrt(H)): a strongly contractive
recurrence that damps a defect of the recurrent product before it reaches an output. `trained_scale(w, g)` multiplies every
weight_hh and the decoders' weight_ih by g: O(1) recurrent weights and long memory, the regime of a trained checkpoint. g = 4 is
used (fp32 stays within 1e-5 of float64); g = 8 is chaotic and is not (tests/test_rnn_budget_cpu.py holds both statements).

Restatements, each returning what the GPU entry points return (P1: probs, enc, dec; P2: labels, acc; the P2 window operator:
logits [B,100,5], hidden [B,2,128]):
  "f64"    oracle/rnn_oracle.py in float64: the reference
  "f32"    the same code in float32: what plain fp32 arithmetic loses
  "3term"  float64 arithmetic in which every product the bf16x3 chain runs on split operands is hi.w_hi + hi.w_lo + lo.w_hi,
           hi = bf16(x), lo = bf16(fp32(x - hi)) (round to nearest even, through torch's bfloat16): the recurrent h-parts, the
           decoder input projections, linear_1 and P2's dense1 (folded into the decoder as one more MFMA tile); byte inputs are
           exact in bf16 and take two terms; "3term_tail" also splits linear_2..5 (k_tail_bf16, the tail of large launches)
and two mutants that the budget must catch:
  "hbf16"       float64 arithmetic with h rounded to bf16 in front of every recurrent product (a dropped h_lo.w_hi term)
  "3term_drop"  "3term" without lo.w_hi
The last three run on this file's own copy of the two recurrences (`Arith` decides how each product is taken); with plain
products that copy equals rnn_oracle to rounding.

`budget(got, ref64, plain, factor, what)`: max |got - ref64| <= factor x max(max |plain - ref64|, FLOOR) on the rows given."""
import numpy as np
import torch

import rnn_forms as rf
from oracle import rnn_oracle
from pepper_thesis_amd import synth

FLOOR = 2.0 ** -23      # one ulp at 1.0: a lucky small `plain` error must not turn the bar into a demand for bit-exactness
FACTOR = 8              # summation order, hardware exp / rcp, FMA contraction: each may double the loss of the restatement
TIE = 2e-4              # labels must agree where the float64 top two accumulated scores are further apart
GAINS = (1, 4)
P1_ROWS_CAP, P2_ROWS_CAP = 48, 6
_SCALED = (".weight_hh_l0", "decoder.weight_ih_l0")   # (matches gru_decoder.weight_ih_l0 too)


def trained_scale(w, g):
    """a copy of a make_weights_p1/p2 dict with every *.weight_hh_l0*, decoder.weight_ih_l0* and gru_decoder.weight_ih_l0*
    multiplied by g"""
    return {k: (v * np.float32(g)).astype(np.float32) if any(s in k for s in _SCALED) else v.copy() for k, v in w.items()}


def weights_p1(g):
    return trained_scale(synth.make_weights_p1(5, 2.0), g)


def weights_p2(g):
    return trained_scale(synth.make_weights_p2(17, 2.0), g)


# ---- inputs: one array per kind, every case runs a prefix ----------------------------------------------------------------
P1_MAX, P2_MAX, P2_WIN_MAX = 4130, 33, 8200


def p1_windows():
    return synth.synth_windows(4245, P1_MAX)


def p2_images():
    return synth.synth_p2_images(4346, P2_MAX)


def p2_sparse_images(n=P2_MAX, seq_len=1000):
    """closer to what the image builder emits: one dominant feature per column, valued 100 to 254; 10 % of cells set to 12"""
    rng = np.random.default_rng(4347)
    y = np.where(rng.random((n, seq_len, 10)) < 0.1, 12, 0).astype(np.uint8)
    dom = rng.integers(0, 10, size=(n, seq_len))
    val = rng.integers(100, 255, size=(n, seq_len)).astype(np.uint8)
    np.put_along_axis(y, dom[..., None], val[..., None], axis=2)
    return y


def p2_window_inputs():
    """one 100-column window per chunk and a random carried-in hidden state [B,2,128]"""
    x = synth.synth_p2_images(4348, P2_WIN_MAX, seq_len=100)
    h = (np.random.default_rng(4349).standard_normal((P2_WIN_MAX, 2, 128)) * 0.3).astype(np.float32)
    return x, h


# ---- the cases of tests/test_rnn_budget_gpu.py: the smallest batch at which each form runs on 256 CUs -------------------------
NUM_CU = 256
X6_ON, BF16_ON = {"p1_f32x6_min_batch": 1}, {"p1_bf16_min_batch": 0}
# id: (dtype, options, windows, (chain, lstm, mt, tail) the plan must name)
P1_CASES = {
    "f32-rows16": (rf.F32, {"lstm_rows": 16}, 33, ("f32", "rows16", None, "k_head_tail")),
    "f32-rows32": (rf.F32, {"lstm_rows": 32}, 33, ("f32", "rows32", None, "k_head_tail")),
    "f32-split4": (rf.F32, {}, 33, ("f32", "split4", None, "k_head_tail")),
    "f32-split2": (rf.F32, {}, 513, ("f32", "split2", None, "k_head_tail")),
    "x6": (rf.F32, X6_ON, 260, ("x6", None, 1, "k_head_tail")),             # a ragged 256-row GEMM item
    "bf16x3-mt1": (rf.BF16X3, BF16_ON, 260, ("bf16x3", None, 1, "k_head_tail")),
    "bf16x3-mt2": (rf.BF16X3, BF16_ON, 4130, ("bf16x3", None, 2, "k_tail_bf16")),
}
# id: (dtype, options, chunks, (kind, rows)); the 19-window call and the window operator
P2_CASES = {
    "f32-us": (rf.F32, {}, 33, ("us", 16)),
    "f32-dsplit": (rf.F32, rf.P2_FORCE["dsplit", 16], 33, ("dsplit", 16)),
    "f32-wg16": (rf.F32, rf.P2_FORCE["wg", 16], 33, ("wg", 16)),
    "f32-wg32": (rf.F32, rf.P2_FORCE["wg", 32], 33, ("wg", 32)),
    "bf16x3-gru16": (rf.BF16X3, {}, 33, ("gru16", 16)),
}
P2_WINDOW_CASES = dict({k: v for k, v in P2_CASES.items() if v[0] == rf.F32},
                       **{"bf16x3-rec32": (rf.BF16X3, {}, 2049, ("rec", 32)), "bf16x3-rec64": (rf.BF16X3, {}, 8200, ("rec", 64))})


def capped(rows, cap):
    """at most `cap` of the sorted rows, spread evenly, the first and the last kept"""
    if len(rows) <= cap:
        return list(rows)
    return [rows[i] for i in sorted({int(round(k)) for k in np.linspace(0, len(rows) - 1, cap)})]


def p1_rows(call):
    return capped(rf.p1_sample_rows(call), P1_ROWS_CAP)


def p2_rows(B, form, cap):
    return capped(rf.sample_rows(B, rf.p2_tiles(form)), cap)


# ---- the arithmetic of one restatement -------------------------------------------------------------------------------
def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def split2(x):
    """the first two pieces of the split8 rule: hi = bf16(x), lo = bf16(fp32(x - hi))"""
    x = np.asarray(x, np.float64)
    hi = _bf16(x)
    return hi, _bf16(x - hi)


class Arith:
    """float64 products x . W^T by kind: "byte" (exact byte inputs), "rec" (h . W_hh^T), "proj" (decoder input projection),
    "lin1", "tail" (linear_2..5), "dense" (P2 dense1), "out" (P1 output layer). Kinds in `split` run on split operands."""

    def __init__(self, weights, split=(), h_bf16=False, drop_lo_hi=False):
        self.w = {k: np.asarray(v, np.float64) for k, v in weights.items()}
        self.split, self.h_bf16, self.drop = frozenset(split), h_bf16, drop_lo_hi
        self.pieces = {}

    def mm(self, kind, x, name):
        W = self.w[name]
        if kind == "rec" and self.h_bf16:
            x = _bf16(x)
        if kind not in self.split:
            return x @ W.T
        if name not in self.pieces:
            self.pieces[name] = split2(W)
        wh, wl = self.pieces[name]
        if kind == "byte":
            return x @ wh.T + x @ wl.T
        xh, xl = split2(x)
        y = xh @ wh.T + xh @ wl.T
        return y if self.drop else y + xl @ wh.T


SPLIT_P1 = ("byte", "rec", "proj", "lin1")
SPLIT_P2 = ("byte", "rec", "proj", "dense")


def arith(weights, how, tail=False):
    if how == "plain":
        return Arith(weights)
    if how == "hbf16":
        return Arith(weights, h_bf16=True)
    assert how in ("3term", "3term_drop"), how
    split = (SPLIT_P1 + (("tail",) if tail else ())) if "linear_1.weight" in weights else SPLIT_P2
    return Arith(weights, split, drop_lo_hi=how == "3term_drop")


_sig = rnn_oracle._sigmoid


def _lstm(a, x, kind, prefix):
    """bidirectional LSTM layer, zero initial state: x [B,T,K] -> [B,T,2H]"""
    outs = []
    for sfx, rev in (("", False), ("_reverse", True)):
        B, T, _ = x.shape
        pre = a.mm(kind, x.reshape(B * T, -1), prefix + ".weight_ih_l0" + sfx).reshape(B, T, -1)
        pre = pre + (a.w[prefix + ".bias_ih_l0" + sfx] + a.w[prefix + ".bias_hh_l0" + sfx])
        H = pre.shape[2] // 4
        h, c, out = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, T, H))
        for t in (range(T - 1, -1, -1) if rev else range(T)):
            g = pre[:, t] + a.mm("rec", h, prefix + ".weight_hh_l0" + sfx)
            c = _sig(g[:, H:2 * H]) * c + _sig(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
            h = _sig(g[:, 3 * H:]) * np.tanh(c)
            out[:, t] = h
        outs.append(out)
    return np.concatenate(outs, axis=2)


def _p1(a, images):
    x = np.asarray(images).astype(np.float64)
    enc = _lstm(a, x, "byte", "encoder")
    dec = _lstm(a, enc, "proj", "decoder")
    y = dec.reshape(len(dec), -1)
    for i in range(1, 6):
        y = rnn_oracle.selu(a.mm("lin1" if i == 1 else "tail", y, "linear_%d.weight" % i) + a.w["linear_%d.bias" % i])
    logits = a.mm("out", y, "output_layer_type.weight") + a.w["output_layer_type.bias"]
    return rnn_oracle.softmax(logits, 1), enc, dec


def _gru(a, x, hidden, kind, prefix):
    """bidirectional GRU layer: x [B,T,K], hidden [2,B,H] -> out [B,T,2H], final hidden [2,B,H]"""
    outs, hs = [], []
    for d, (sfx, rev) in enumerate((("", False), ("_reverse", True))):
        B, T, _ = x.shape
        pre = a.mm(kind, x.reshape(B * T, -1), prefix + ".weight_ih_l0" + sfx).reshape(B, T, -1) + a.w[prefix + ".bias_ih_l0" + sfx]
        H = pre.shape[2] // 3
        h, out = hidden[d].copy(), np.zeros((B, T, H))
        for t in (range(T - 1, -1, -1) if rev else range(T)):
            gh = a.mm("rec", h, prefix + ".weight_hh_l0" + sfx) + a.w[prefix + ".bias_hh_l0" + sfx]
            gi = pre[:, t]
            r = _sig(gi[:, :H] + gh[:, :H])
            z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1.0 - z) * n + z * h
            out[:, t] = h
        outs.append(out)
        hs.append(h)
    return np.concatenate(outs, axis=2), np.stack(hs)


def _p2_window(a, x, hidden):
    enc, h_enc = _gru(a, x, hidden, "byte", "gru_encoder")
    dec, h_dec = _gru(a, enc, h_enc, "proj", "gru_decoder")
    B, T, _ = dec.shape
    return a.mm("dense", dec.reshape(B * T, -1), "dense1.weight").reshape(B, T, -1) + a.w["dense1.bias"], h_dec


def _p2(a, images, seq_len=1000, window=100, jump=50):
    x = np.asarray(images).astype(np.float64)
    hidden = np.zeros((2, len(x), 128))
    acc = np.zeros((len(x), seq_len, 5))
    for i in range(0, seq_len - window + 1, jump):
        logits, hidden = _p2_window(a, x[:, i:i + window], hidden)
        acc[:, i:i + window] += rnn_oracle.softmax(logits, 2)
    return acc.argmax(axis=2).astype(np.uint8), acc


_DTYPES = {"f64": np.float64, "f32": np.float32}


def p1(w, images, how):
    """(probs [B,3], enc [B,33,512], dec [B,33,512]) of restatement `how`; "3term_tail": "3term" with linear_2..5 split too"""
    if how in _DTYPES:
        return rnn_oracle.p1_forward(w, images, _DTYPES[how], taps=True)[:3]
    if how == "3term_tail":
        return _p1(arith(w, "3term", tail=True), images)
    return _p1(arith(w, how), images)


def p2(w, images, how):
    """(labels [B,1000], acc [B,1000,5])"""
    if how in _DTYPES:
        return rnn_oracle.p2_forward(w, images, _DTYPES[how])
    return _p2(arith(w, how), images)


def p2_window(w, x, h_in, how):
    """(logits [B,100,5], hidden [B,2,128]); h_in [B,2,128] as the entry point takes it"""
    if how in _DTYPES:
        dt = _DTYPES[how]
        lg, h = rnn_oracle.p2_window({k: np.asarray(v, dtype=dt) for k, v in w.items()}, np.asarray(x).astype(dt),
                                     np.asarray(h_in).transpose(1, 0, 2).astype(dt))
    else:
        lg, h = _p2_window(arith(w, how), np.asarray(x).astype(np.float64), np.asarray(h_in).transpose(1, 0, 2).astype(np.float64))
    return lg, h.transpose(1, 0, 2)


class Restated:
    """answers of one function fn(rows, how) -> tuple of arrays with a leading row axis, computed once per (how, row) (rows are
    independent) and then left unchanged"""

    def __init__(self, fn):
        self.fn, self.cache = fn, {}

    def __call__(self, rows, how):
        rows = [int(i) for i in rows]
        need = [i for i in rows if (how, i) not in self.cache]
        if need:
            for i, r in zip(need, zip(*self.fn(need, how))):
                self.cache[how, i] = r
        n_out = len(self.cache[how, rows[0]])
        return [np.stack([self.cache[how, i][k] for i in rows]) for k in range(n_out)]


# ---- the bar ---------------------------------------------------------------------------------------------------------
def _row_err(a, ref):
    return np.abs(np.asarray(a, np.float64) - ref).reshape(len(ref), -1).max(1)


def plain_error(ref64, plain):
    """max |plain - ref64|, floored; `plain` is one array or a tuple of arrays (the largest error of them counts)"""
    plains = plain if isinstance(plain, (tuple, list)) else (plain,)
    return max(max(float(_row_err(p, ref64).max()) for p in plains), FLOOR)


def budget(got, ref64, plain, factor, what, rows=None):
    """asserts max |got - ref64| <= factor x max(max |plain - ref64|, FLOOR) over the rows given (arrays with one leading row
    axis, already cut to those rows; `rows` names them in the message); prints and returns the ratio error / plain error"""
    ref64 = np.asarray(ref64, np.float64)
    assert np.shape(got) == ref64.shape, (what, np.shape(got), ref64.shape)
    assert np.isfinite(got).all(), what
    e_plain = plain_error(ref64, plain)
    err = _row_err(got, ref64)
    ratio = float(err.max()) / e_plain
    print("budget %-58s err %.3g  plain %.3g  ratio %.2f  (bar %g)" % (what, err.max(), e_plain, ratio, factor))
    bad = np.flatnonzero(err > factor * e_plain)
    assert not len(bad), "%s: row %d is %.3g from float64 = %.1f x the plain arithmetic's %.3g (bar %g x)" % (
        what, bad[0] if rows is None else rows[bad[0]], err[bad[0]], err[bad[0]] / e_plain, e_plain, factor)
    return ratio


def labels_agree(labels, acc64, labels64, what):
    """labels equal float64's on every column whose float64 top-two gap exceeds TIE"""
    top2 = np.sort(acc64, axis=-1)
    clear = (top2[..., -1] - top2[..., -2]) > TIE
    assert np.array_equal(np.asarray(labels)[clear], labels64[clear]), what


# ---- per-row answers of every restatement on the shared inputs, at recurrent gain g ---------------------------------------
def restated_p1(g, x):
    w = weights_p1(g)
    return Restated(lambda rows, how: p1(w, x[rows], how))


def restated_p2(g, y):
    w = weights_p2(g)
    return Restated(lambda rows, how: p2(w, y[rows], how))


def restated_p2_window(g, x, h_in):
    w = weights_p2(g)
    return Restated(lambda rows, how: p2_window(w, x[rows], h_in[rows], how))
