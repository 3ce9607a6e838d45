"""GPU: every RNN kernel form at the batch sizes where the library switches forms (tests/rnn_forms.py: boundaries), P1 and P2,
fp32 and bf16x3, the split-6 chain and the chunked calls. At each size:
  1. the form that ran is the one the rules name: profile names (pv_profile_*) and, where names cannot tell two forms apart,
     bit-identity with the form forced by options (run on the same launch alone);
  2. every row against an independent form: bf16x3 vs fp32 1e-4, split-6 vs the f32 kernels 2e-6, the f32 tile forms vs each
     other 2e-6, P2 fp32 forms vs the one-workgroup form 1e-5; P2 labels equal away from ties, accumulated softmax summing to
     1 or 2 on every chunk;
  3. rows spread over every tile position of each launch (first and middle tile edges, last full tile, partial last tile,
     last row) against the float64 oracle at 1e-4.
The decoder input projections G of the P1 bf16x3 / split-6 chains (33 x Bp x 8 KB) and of P2 bf16x3 (100 x Bp x 3 KB) are
time-major, so past 15873 windows / 13953 chunks every row reads G beyond 4 GiB: those sizes are compared on every row.
Not told apart by names or options, and so left to the numbers: the bf16x3 chains' mt and split-K factors, and the unit-split
form's 4 or 2 parts."""
from collections import Counter

import numpy as np
import pytest
import torch

import rnn_forms as rf
from oracle import rnn_oracle
from pepper_thesis_amd import _ffi, runtime, synth

pytestmark = pytest.mark.gpu
OFF = 1 << 24           # p1_f32x6_min_batch above any batch: the f32 kernels
TOL = 1e-4              # against float64; bf16x3 against fp32
TOL_F32_FORMS = 2e-6    # split-6 vs the f32 kernels, f32 tile forms vs each other (P1 probabilities)
TOL_P2_FORMS = 1e-5     # P2 fp32 forms vs each other (accumulated softmax, logits, hidden state)
TIE = 2e-4              # labels must agree where the top two accumulated scores are further apart
W1 = synth.make_weights_p1(5, 2.0)
W2 = synth.make_weights_p2(17, 2.0)


class OracleRows:
    """float64 oracle answers per row index of one fixed input array, computed once per row (rows are independent)"""

    def __init__(self, x, fn):
        self.x, self.fn, self.cache = x, fn, {}

    def __call__(self, rows):
        need = [int(i) for i in rows if int(i) not in self.cache]
        if need:
            for i, r in zip(need, zip(*self.fn(self.x[need]))):
                self.cache[i] = r
        return [np.stack([self.cache[int(i)][k] for i in rows]) for k in range(len(self.cache[int(rows[0])]))]


def check_every_row(got, ref, bar, what):
    """|got - ref| <= bar on every element; reports the first row beyond it"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    for lo in range(0, len(got), 1024):
        err = np.abs(got[lo:lo + 1024] - ref[lo:lo + 1024]).reshape(min(1024, len(got) - lo), -1).max(1)
        bad = np.flatnonzero(err > bar)
        assert not len(bad), "%s: row %d off by %.3g (bar %g)" % (what, lo + bad[0], err[bad[0]], bar)


def check_rows(got, ref, rows, bar, what):
    err = np.abs(got[rows].astype(np.float64) - ref).reshape(len(rows), -1).max(1)
    bad = np.flatnonzero(err > bar)
    assert not len(bad), "%s: row %d off the float64 oracle by %.3g" % (what, rows[bad[0]], err[bad[0]])


def check_labels(labels, acc_ref, labels_ref, what):
    top2 = np.sort(acc_ref, axis=2)
    clear = (top2[..., -1] - top2[..., -2]) > TIE
    assert np.array_equal(labels[clear], labels_ref[clear]), what


def check_sums(acc, what):
    """every column is covered by one window (the first and last 50) or two: the accumulated softmax sums to 1 or 2"""
    s = acc.sum(2)
    assert np.abs(s[:, :50] - 1).max() < 1e-4 and np.abs(s[:, 50:950] - 2).max() < 1e-4 and np.abs(s[:, 950:] - 1).max() < 1e-4, what


def options_of(ctx):
    return {k: ctx.get_option(k) for k in rf.OPTION_NAMES}


def reset(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def profiled(ctx, run):
    ctx.profile_begin()
    out = run()
    prof = ctx.profile_end()
    return out, Counter({k: n for k, (_, n) in prof.items()})


@pytest.fixture(scope="module")
def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def bounds(num_cu):
    return rf.boundaries(num_cu)


@pytest.fixture(scope="module")
def x1(bounds):
    """P1 windows for the largest size; every size runs a prefix"""
    return synth.synth_windows(4242, max(max(bounds["p1_f32"]), max(bounds["p1_bf16x3"]), max(bounds["p1_f32_native"])))


@pytest.fixture(scope="module")
def y2(bounds):
    return synth.synth_p2_images(4343, max(max(bounds["p2_f32"]), max(bounds["p2_bf16x3"])))


@pytest.fixture(scope="module")
def p1_oracle(x1):
    return OracleRows(x1, lambda x: (rnn_oracle.p1_forward(W1, x, np.float64),))


@pytest.fixture(scope="module")
def p2_oracle(y2):
    return OracleRows(y2, lambda y: rnn_oracle.p2_forward(W2, y, np.float64))


@pytest.fixture(scope="module")
def p1_native(x1):
    """the f32 kernels over every window in one call (32-row tiles): the independent answer for the split-6 and bf16x3 chains"""
    ctx = runtime.Context(0)
    ctx.load_p1(W1)
    ctx.set_option("p1_f32x6_min_batch", OFF)
    p = ctx.forward_p1(x1)
    ctx.close()
    return p


@pytest.fixture(scope="module")
def p2_fp32(y2):
    """the fp32 mode over every chunk in one call: the independent answer for P2 bf16x3"""
    ctx = runtime.Context(0)
    ctx.load_p2(W2)
    out = ctx.forward_p2(y2, want_acc=True)
    ctx.close()
    return out


def p1_forced(f):
    """options that force P1 launch form f, where options can"""
    if f.chain == "f32":
        o = {"head_splits": f.splits, "tail_rows": f.tail_rows}
        if f.lstm.startswith("rows"):
            o["lstm_rows"] = f.rows
        return o
    return {"tail_rows": f.tail_rows} if f.tail == "k_head_tail" else {}


def walk_p1(ctx, dtype, sizes, num_cu, x1, oracle, native):
    opts = options_of(ctx)
    dev = "cuda:%d" % ctx.device_id
    xd = torch.from_numpy(x1).to(dev)
    for B in sizes:
        call = rf.p1_call(dtype, B, num_cu, opts)
        probs = torch.zeros((B, 3), dtype=torch.float32, device=dev)
        _, names = profiled(ctx, lambda: ctx.forward_p1_dev(xd.data_ptr(), B, probs.data_ptr()))
        ctx.synchronize()
        got = probs.cpu().numpy()
        want = sum((f.names for _, _, f in call), Counter())
        assert names == want, (dtype, B, call, names)
        assert np.abs(got.sum(1) - 1).max() < 1e-5, B
        for b0, nb, f in call:
            what = "%s B=%d launch [%d, %d) %s" % (dtype, B, b0, b0 + nb, f.chain)
            part, x = got[b0:b0 + nb], x1[b0:b0 + nb]
            # 1. the form: bit for bit the forced form, the launch run alone
            force = p1_forced(f)
            if force:
                reset(ctx, dict(opts, **force))
                alone = ctx.forward_p1(x)
                reset(ctx, opts)
                assert np.array_equal(alone.view(np.uint32), part.view(np.uint32)), (what, force)
            # 2. every row against an independent form
            if f.chain == "f32" and f.rows == 32:   # (the 32-row tiles are the form of `native`: take the 16-row tiles)
                reset(ctx, dict(opts, lstm_rows=16))
                check_every_row(part, ctx.forward_p1(x), TOL_F32_FORMS, what + " vs 16-row tiles")
                reset(ctx, opts)
            else:
                check_every_row(part, native[b0:b0 + nb], TOL if f.chain == "bf16x3" else TOL_F32_FORMS, what + " vs f32 kernels")
        # 3. rows at every tile position of every launch against float64
        rows = rf.p1_sample_rows(call)
        check_rows(got, oracle(rows)[0], rows, TOL, "%s B=%d" % (dtype, B))


@pytest.mark.parametrize("chain", ["p1_f32", "p1_f32_native"])
def test_p1_fp32_forms_at_every_switch(chain, num_cu, bounds, x1, p1_oracle, p1_native):
    """the fp32 mode: unit split 4 / 2 parts, 16 / 32-row tiles, k_head_splitk 33 / 11 slabs, the split-6 chain with its
    split-K factors, 16 / 32-row tails, G past 4 GiB, chunks of 16384 with an f32 remainder; p1_native: the f32 kernels beyond
    the split-6 threshold"""
    ctx = runtime.Context(0)
    ctx.load_p1(W1)
    if chain == "p1_f32_native":
        ctx.set_option("p1_f32x6_min_batch", OFF)
    walk_p1(ctx, rf.F32, bounds[chain], num_cu, x1, p1_oracle, p1_native)
    ctx.close()


def test_p1_bf16x3_forms_at_every_switch(num_cu, bounds, x1, p1_oracle, p1_native):
    """the bf16x3 mode: f32 kernels below 513 windows, every linear_1 split-K factor, k_head_tail / k_tail_bf16, 32 / 64-row
    tiles, G past 4 GiB, chunks of 16384 with an f32 remainder"""
    ctx = runtime.Context(0)
    ctx.load_p1(W1, _ffi.PV_DTYPE_BF16_INPUT_GEMM)
    walk_p1(ctx, rf.BF16X3, bounds["p1_bf16x3"], num_cu, x1, p1_oracle, p1_native)
    ctx.close()


def test_p2_fp32_forms_at_every_switch(num_cu, bounds, y2, p2_oracle):
    """k_gru_us up to 1024 chunks, the direction split up to 2048, one workgroup on 16 and then 32-row tiles"""
    ctx = runtime.Context(0)
    ctx.load_p2(W2)
    opts = options_of(ctx)
    for B in bounds["p2_f32"]:
        f = rf.p2_call(rf.F32, B, num_cu, opts)
        y, what = y2[:B], "p2 fp32 B=%d %s/%d" % (B, f.kind, f.rows)
        (labels, acc), names = profiled(ctx, lambda: ctx.forward_p2(y, want_acc=True))
        assert names == f.names, (what, names)
        check_sums(acc, what)
        force = rf.P2_FORCE.get((f.kind, f.rows))
        if force:
            reset(ctx, dict(opts, **force))
            l1, a1 = ctx.forward_p2(y, want_acc=True)
            reset(ctx, opts)
            assert np.array_equal(a1.view(np.uint32), acc.view(np.uint32)) and np.array_equal(l1, labels), (what, force)
        other = {"gru_rows": 32} if (f.kind, f.rows) == ("wg", 16) else {"gru_split": 0, "gru_rows": 16}
        reset(ctx, dict(opts, **other))
        l0, a0 = ctx.forward_p2(y, want_acc=True)
        reset(ctx, opts)
        if f.kind == "dsplit":   # (the forcing options alone cannot tell it from the one-workgroup form; the bits can)
            assert not np.array_equal(a0.view(np.uint32), acc.view(np.uint32)), what
        check_every_row(acc, a0, TOL_P2_FORMS, what + " vs %s" % other)
        check_labels(labels, a0, l0, what)
        rows = rf.sample_rows(B, rf.p2_tiles(f))
        lr, ar = p2_oracle(rows)
        check_rows(acc, ar, rows, TOL, what)
        check_labels(labels[rows], ar, lr, what + " vs float64")
    ctx.close()


def test_p2_bf16x3_forms_at_every_switch(num_cu, bounds, y2, p2_oracle, p2_fp32):
    """k_gru16_bf16 up to 2048 chunks, k_rec_bf16 on 32 and then 64-row tiles, p2b.G past 4 GiB from 13953 chunks, the
    polisher's 2121; dense1 always folded (k_p2_combine: k_p2_dense cannot run on 256 CUs)"""
    l32, a32 = p2_fp32
    ctx = runtime.Context(0)
    ctx.load_p2(W2, _ffi.PV_DTYPE_BF16_INPUT_GEMM)
    for B in bounds["p2_bf16x3"]:
        f = rf.p2_call(rf.BF16X3, B, num_cu)
        y, what = y2[:B], "p2 bf16x3 B=%d %s/%d" % (B, f.kind, f.rows)
        (labels, acc), names = profiled(ctx, lambda: ctx.forward_p2(y, want_acc=True))
        assert names == f.names, (what, names)
        check_sums(acc, what)
        check_every_row(acc, a32[:B], TOL, what + " vs fp32")
        check_labels(labels, a32[:B], l32[:B], what + " vs fp32")
        rows = rf.sample_rows(B, rf.p2_tiles(f))
        lr, ar = p2_oracle(rows)
        check_rows(acc, ar, rows, TOL, what)
        check_labels(labels[rows], ar, lr, what + " vs float64")
        del labels, acc
    ctx.close()


def test_p2_window_operator_at_the_16_row_switch(num_cu, bounds, y2):
    """the single-window operator (logits + carried hidden state, random hidden_in) on both sides of the switch where
    bf16x3 leaves k_gru16_bf16 and fp32 leaves the direction split: fp32 forms vs the one-workgroup form, bf16x3 vs fp32,
    spread rows vs float64"""
    pair = rf.switches(num_cu)["p2_bf16x3"][0]
    w64 = {k: v.astype(np.float64) for k, v in W2.items()}
    x = np.ascontiguousarray(y2[:max(pair), 300:400])
    h_in = (np.random.default_rng(5).standard_normal((len(x), 2, 128)) * 0.3).astype(np.float32)
    oracle = OracleRows(np.arange(len(x)), lambda i: (lambda lg, h: (lg, h.transpose(1, 0, 2)))(
        *rnn_oracle.p2_window(w64, x[i].astype(np.float64), h_in[i].transpose(1, 0, 2).astype(np.float64))))
    fp32 = {}
    for dtype in (rf.F32, rf.BF16X3):
        ctx = runtime.Context(0)
        ctx.load_p2(W2, _ffi.PV_DTYPE_F32 if dtype == rf.F32 else _ffi.PV_DTYPE_BF16_INPUT_GEMM)
        opts = options_of(ctx)
        for B in pair:
            f = rf.p2_call(dtype, B, num_cu, opts, nwin=1)
            what = "p2 window %s B=%d %s/%d" % (dtype, B, f.kind, f.rows)
            (lg, h), names = profiled(ctx, lambda: ctx.forward_p2_window(x[:B], h_in[:B]))
            assert names == f.names, (what, names)
            if dtype == rf.F32:
                force = rf.P2_FORCE.get((f.kind, f.rows))
                if force:
                    reset(ctx, dict(opts, **force))
                    lg1, h1 = ctx.forward_p2_window(x[:B], h_in[:B])
                    reset(ctx, opts)
                    assert np.array_equal(lg1.view(np.uint32), lg.view(np.uint32)) and np.array_equal(h1.view(np.uint32), h.view(np.uint32)), what
                other = {"gru_rows": 32} if (f.kind, f.rows) == ("wg", 16) else {"gru_split": 0, "gru_rows": 16}
                reset(ctx, dict(opts, **other))
                lg0, h0 = ctx.forward_p2_window(x[:B], h_in[:B])
                reset(ctx, opts)
                check_every_row(lg, lg0, TOL_P2_FORMS, what + " logits vs %s" % other)
                check_every_row(h, h0, TOL_P2_FORMS, what + " hidden vs %s" % other)
                fp32[B] = (lg, h)
            else:
                check_every_row(lg, fp32[B][0], TOL, what + " logits vs fp32")
                check_every_row(h, fp32[B][1], TOL, what + " hidden vs fp32")
            rows = rf.sample_rows(B, rf.p2_tiles(f))
            rl, rh = oracle(rows)
            check_rows(lg, rl, rows, TOL, what + " logits")
            check_rows(h, rh, rows, TOL, what + " hidden")
        ctx.close()
