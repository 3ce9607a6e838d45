"""GPU: the split-6 chain of the fp32 mode (P1 calls of at least `p1_f32x6_min_batch` windows). Every matrix product runs on
the bf16 MFMA as six terms of three-piece operands; the chain must stay fp32-class: against the f32 MFMA kernels on EVERY
window within 2e-6 on probabilities and 4e-6 on layer taps, and no further from the float64 oracle than 2x the f32 kernels.
(Measured over 8192 windows: 1.5e-6 / 2.7e-6 at most. The two f32 MFMA tile forms, 16 and 32 rows, differ by 1.1e-6 on the
same windows: twice the 1e-6 / 2e-6 bars the form-vs-form tests apply to small slices.)"""
import numpy as np
import pytest
import torch

from oracle import rnn_oracle
from pepper_thesis_amd import _ffi, runtime, synth
from pepper_thesis_amd.batch import PRESETS, pack_regions
from pepper_thesis_amd.device import DeviceBatch, DeviceOut

pytestmark = pytest.mark.gpu
OFF = 1 << 24   # above any batch: the split-6 chain never runs


@pytest.fixture
def x6_opt(hip_ctx):
    """the session context's p1_f32x6_min_batch, restored after the test"""
    keep = hip_ctx.get_option("p1_f32x6_min_batch")
    yield lambda v: hip_ctx.set_option("p1_f32x6_min_batch", v)
    hip_ctx.set_option("p1_f32x6_min_batch", keep)


def _gemm(ctx, A, W, b, splits, quads):
    lib = _ffi.load()
    M, K = A.shape
    N = W.shape[0]
    out = np.zeros((splits, M, N), np.float32)
    _ffi.check(lib.pv_debug_gemm_bf16x6(ctx.handle, A.ctypes.data, W.ctypes.data, None if b is None else b.ctypes.data,
                                        M, N, K, splits, quads, out.ctypes.data, None))
    if quads:
        out = out.reshape(M // 4, N, 4).transpose(0, 2, 1).reshape(1, M, N)
    return out.sum(0, dtype=np.float64) if splits > 1 else out[0].astype(np.float64)


@pytest.mark.parametrize("M,N,K,splits,quads", [(1028, 512, 512, 1, 0), (260, 2048, 512, 1, 1), (516, 512, 16896, 11, 0),
                                                (1028, 512, 16896, 33, 0)])
def test_gemm_bf16x6_is_fp32_class(hip_ctx, M, N, K, splits, quads):
    """operands from [-1, 1) plus rows spanning 1e-20 .. 1e3 and zero rows; ragged M (a partial 256-row tile). The 6-term
    GEMM's max error against float64 (relative to each output's magnitude sum) is at most twice numpy's fp32 matmul error on
    the same data. K = 16896 runs split-K as linear_1 does (one long fp32 accumulation chain is what the f32 MFMA kernels
    run too; numpy's blocked sums are shorter)"""
    rng = np.random.default_rng(M + K)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    A[:24] *= np.logspace(-20, 3, 24)[:, None].astype(np.float32)
    A[30] = 0.0
    W[40] = 0.0
    A[M - 1] = rng.uniform(-1, 1, K).astype(np.float32) * 1e3
    b = rng.uniform(-1, 1, N).astype(np.float32) if splits == 1 else None
    got = _gemm(hip_ctx, A, W, b, splits, quads)
    ref = A.astype(np.float64) @ W.astype(np.float64).T + (0 if b is None else b.astype(np.float64))
    f32 = (A @ W.T + (0 if b is None else b)).astype(np.float64)
    # scale each row by its magnitude so the tiny rows count too
    mag = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T + (0 if b is None else np.abs(b).astype(np.float64)) + 1e-300
    e6 = float(np.max(np.abs(got - ref) / mag))
    e32 = float(np.max(np.abs(f32 - ref) / mag))
    assert np.isfinite(got).all()
    assert np.all(got[30] == (0 if b is None else b)) and np.all(got[:, 40] == (0 if b is None else b[40]))
    assert e6 <= 2 * e32, (e6, e32)


@pytest.mark.parametrize("B", [8192, 8200])
def test_p1_split6_chain_matches_the_f32_kernels(hip_ctx, x6_opt, B):
    """forced split-6 against forced native fp32 on every window: probabilities within 1e-6, both layer taps within 2e-6; on
    sampled rows no further than 2x the native path from the float64 oracle; bit-identical run to run"""
    w = synth.make_weights_p1(5, 2.0)
    hip_ctx.load_p1(w)
    x = synth.synth_windows(7000 + B, B)
    x6_opt(1)
    p6, e6, d6 = hip_ctx.forward_p1(x, taps=True)
    x6_opt(OFF)
    pn, en, dn = hip_ctx.forward_p1(x, taps=True)
    assert np.isfinite(p6).all()
    np.testing.assert_allclose(p6, pn, atol=2e-6, rtol=0)
    np.testing.assert_allclose(e6, en, atol=4e-6, rtol=0)
    np.testing.assert_allclose(d6, dn, atol=4e-6, rtol=0)
    sel = np.r_[0:12, B // 2:B // 2 + 12, B - 12:B]
    rp, renc, rdec, _ = rnn_oracle.p1_forward(w, x[sel], np.float64, taps=True)
    for got, nat, ref in ((p6[sel], pn[sel], rp), (e6[sel], en[sel], renc), (d6[sel], dn[sel], rdec)):
        err6 = float(np.abs(got - ref).max())
        errn = float(np.abs(nat - ref).max())
        assert err6 <= 2 * errn + 1e-7, (err6, errn)
    x6_opt(1)
    again = hip_ctx.forward_p1(x)
    assert np.array_equal(again.view(np.uint32), p6.view(np.uint32))


def test_p1_split6_switch_follows_the_threshold():
    """below the threshold: the f32 kernels bit for bit; at it: the split-6 chain (within the bars); an explicit lstm_rows
    keeps the f32 kernels at any size"""
    ctx = runtime.Context(0)
    w = synth.make_weights_p1(9, 2.0)
    ctx.load_p1(w)
    default = ctx.get_option("p1_f32x6_min_batch")
    assert 1024 < default <= 8192
    x = synth.synth_windows(77, 3000)
    ctx.set_option("p1_f32x6_min_batch", OFF)
    native = ctx.forward_p1(x)
    ctx.set_option("p1_f32x6_min_batch", 3001)
    assert np.array_equal(ctx.forward_p1(x).view(np.uint32), native.view(np.uint32))
    ctx.set_option("p1_f32x6_min_batch", 3000)
    at = ctx.forward_p1(x)
    assert not np.array_equal(at.view(np.uint32), native.view(np.uint32))
    np.testing.assert_allclose(at, native, atol=2e-6, rtol=0)
    ctx.set_option("lstm_rows", 16)   # (the form the library picks for 3000 windows)
    assert np.array_equal(ctx.forward_p1(x).view(np.uint32), native.view(np.uint32))
    ctx.close()


def test_p1_f32x6_option_validation(hip_ctx, x6_opt):
    for bad in (0, -1, (1 << 24) + 1):
        with pytest.raises(_ffi.PepperHipError) as e:
            x6_opt(bad)
        assert e.value.code == _ffi.PV_ERR_INVALID
    for good in (1, 4096, 1 << 24):
        x6_opt(good)
        assert hip_ctx.get_option("p1_f32x6_min_batch") == good


def test_graph_of_builder_plus_split6_chain(hip_ctx, x6_opt):
    """image builder + the split-6 P1 chain as one captured graph: replays reproduce the eager bits"""
    dev = "cuda:%d" % hip_ctx.device_id
    hip_ctx.load_p1(synth.make_weights_p1(43, 2.0))
    x6_opt(1)
    P = PRESETS["ont_r9_guppy5_sup"]
    regs = [synth.synth_region(4300 + k, region_len=3000, depth=30, read_len=900, site_every=40) for k in range(2)]
    db = DeviceBatch(pack_regions(regs), dev)
    cap = 1024
    images = torch.zeros((cap, 33, 26), dtype=torch.int8, device=dev)
    dout = DeviceOut(cap, cap * 16, dev, images=images)
    probs = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    st = hip_ctx.stream

    def chain():
        hip_ctx.summarize_dev(db, P, dout, stream=st)
        hip_ctx.forward_p1_dev(images.data_ptr(), cap, probs.data_ptr(), stream=st)

    chain()
    hip_ctx.synchronize()
    n = dout.n_out()
    assert 50 < n <= cap and dout.status() == 0
    want_img, want_p = images.cpu().numpy().copy(), probs.cpu().numpy().copy()
    with hip_ctx.graph_capture(st) as g:
        chain()
    for _ in range(3):
        images.zero_(); probs.zero_(); dout.counts.zero_()
        torch.cuda.synchronize()
        g.launch()
        hip_ctx.synchronize()
        assert dout.n_out() == n and dout.status() == 0
        assert np.array_equal(images.cpu().numpy()[:n], want_img[:n])
        assert np.array_equal(probs.cpu().numpy()[:n].view(np.uint32), want_p[:n].view(np.uint32))
    g.close()
