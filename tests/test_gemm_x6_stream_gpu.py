"""GPU: k_gemm_x6_stream, the split-6 chain's decoder input projection with 48-row A tiles resident in LDS and W streamed from L2,
through pv_debug_gemm_x6_stream, against k_gemm_bf16x6 through pv_debug_gemm_bf16x6 on the same operands. Both entries keep guard
rows behind C and fail the call when a row is stored past M, so every ragged case also proves that rows past M are dropped.

Bit-identity: per output element the new kernel issues the MFMAs of gemm6_body (k-steps ascending, the six terms in its order, the
same lane-group-to-k map, bias added last), so C must be the same bits. M: below one row tile (4, 44), exactly one item (48), a
ragged second item (52, 100), and 48 * 257 + 4: more items than any MI355X has CUs, so some workgroup takes a second item, and the
last one is ragged. Operands: the recipe of test_gemm_x6_presplit_gpu.test_fp32_class_on_two_ragged_items.
Layout: integer operands in [-8, 8] against the float64 product: a wrong row, column, k position, ring slot or bias is a wrong integer.
Pieces: test_gemm_x6_presplit_gpu's "all three A pieces are routed" case at M = 52.
Chain: with p1_f32x6_min_batch = 32 the probabilities and the decoder tap are bit-identical between p1_gemm6_stream = 0 and 1."""
import numpy as np
import pytest

from pepper_thesis_amd import _ffi, runtime, synth

pytestmark = pytest.mark.gpu

K = 512
MS = [4, 44, 48, 52, 100, 48 * 257 + 4]
SHAPES = [(M, N, quads, bias) for M in MS for N in (512, 2048) for quads in (0, 1) for bias in (False, True)]


def _run(entry, ctx, A, W, b, quads):
    """C [M][N] fp32 through one of the two debug entries"""
    lib = _ffi.load()
    M, N = A.shape[0], W.shape[0]
    out = np.zeros((M, N), np.float32)
    bp = None if b is None else b.ctypes.data
    if entry == "stream":
        _ffi.check(lib.pv_debug_gemm_x6_stream(ctx.handle, A.ctypes.data, W.ctypes.data, bp, M, N, K, quads, out.ctypes.data, None))
    else:
        _ffi.check(lib.pv_debug_gemm_bf16x6(ctx.handle, A.ctypes.data, W.ctypes.data, bp, M, N, K, 1, quads, out.ctypes.data, None))
    if quads:
        out = np.ascontiguousarray(out.reshape(M // 4, N, 4).transpose(0, 2, 1)).reshape(M, N)
    return out


def _wide_operands(M, N, bias):
    """rows scaled over 1e-20 .. 1e3, a zero row, a large last row, a zero weight row"""
    rng = np.random.default_rng(M + N + K)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    ns = min(24, M - 2)
    A[:ns] *= np.logspace(-20, 3, ns)[:, None].astype(np.float32)
    zr = min(30, M - 2)
    A[zr] = 0.0
    W[40] = 0.0
    A[M - 1] = rng.uniform(-1, 1, K).astype(np.float32) * 1e3
    b = rng.uniform(-1, 1, N).astype(np.float32) if bias else None
    return A, W, b, zr


@pytest.mark.parametrize("M,N,quads,bias", SHAPES)
def test_bit_identical_to_the_staged_kernel(hip_ctx, M, N, quads, bias):
    A, W, b, zr = _wide_operands(M, N, bias)
    new = _run("stream", hip_ctx, A, W, b, quads)
    old = _run("staged", hip_ctx, A, W, b, quads)
    assert np.isfinite(new).all()
    bb = np.zeros(N, np.float32) if b is None else b
    assert np.all(new[zr] == bb) and np.all(new[:, 40] == bb[40])
    diff = new.view(np.uint32) != old.view(np.uint32)
    assert not diff.any(), "%d of %d words differ, first at %s" % (diff.sum(), diff.size, np.argwhere(diff)[0])


@pytest.mark.parametrize("M,N,quads,bias", SHAPES)
def test_layout_integer_operands_are_exact(hip_ctx, M, N, quads, bias):
    rng = np.random.default_rng(M * 7 + N + quads)
    A = rng.integers(-8, 9, (M, K)).astype(np.float32)
    W = rng.integers(-8, 9, (N, K)).astype(np.float32)
    b = rng.integers(-8, 9, N).astype(np.float32) if bias else None
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    if bias:
        ref = ref + b.astype(np.float64)
    got = _run("stream", hip_ctx, A, W, b, quads)
    assert np.array_equal(got.astype(np.float64), ref)


def _split3(x):
    """the three bf16 pieces of fp32 values, as float64 (the rule of split3_host.hpp, through torch's bfloat16)"""
    import torch
    bf = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).bfloat16().float().numpy()
    x0 = bf(x)
    r1 = (x - x0).astype(np.float32)
    x1 = bf(r1)
    x2 = bf((r1 - x1).astype(np.float32))
    return x0.astype(np.float64), x1.astype(np.float64), x2.astype(np.float64)


def test_layout_all_three_a_pieces_are_routed(hip_ctx):
    """A: four odd integers of 18 to 20 bits per row, all three pieces non-zero, else zero; W integers in [-2, 2] (one piece):
    every product and partial sum is an integer below 2^23, so the result is the exact integer product, and it is not if any A
    piece is dropped or takes another row tile's registers"""
    M, N = 52, 512
    rng = np.random.default_rng(11)
    pool = (rng.integers(1 << 17, 1 << 20, 4000) | 1).astype(np.float32)
    x0, x1, x2 = _split3(pool)
    assert np.array_equal(x0 + x1 + x2, pool.astype(np.float64))
    pool = pool[(x1 != 0) & (x2 != 0)]
    assert len(pool) >= 4 * M
    A = np.zeros((M, K), np.float32)
    for m in range(M):
        k = rng.choice(K, 4, replace=False)
        A[m, k] = pool[4 * m:4 * m + 4] * rng.choice([-1, 1], 4).astype(np.float32)
    p0, p1, p2 = _split3(A[A != 0])
    assert np.all(p0 != 0) and np.all(p1 != 0) and np.all(p2 != 0)
    W = rng.integers(-2, 3, (N, K)).astype(np.float32)
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    for drop in _split3(A):   # the case can see each piece: without it the integer differs in some output
        assert not np.array_equal((A.astype(np.float64) - drop) @ W.astype(np.float64).T, ref)
    for quads in (0, 1):
        assert np.array_equal(_run("stream", hip_ctx, A, W, None, quads).astype(np.float64), ref)


def test_other_shapes_are_refused(hip_ctx):
    lib = _ffi.load()
    A, W, out = np.zeros((48, 256), np.float32), np.zeros((512, 256), np.float32), np.zeros((48, 512), np.float32)
    assert lib.pv_debug_gemm_x6_stream(hip_ctx.handle, A.ctypes.data, W.ctypes.data, None, 48, 512, 256, 0, out.ctypes.data, None) != 0
    A, W = np.zeros((48, K), np.float32), np.zeros((256, K), np.float32)
    assert lib.pv_debug_gemm_x6_stream(hip_ctx.handle, A.ctypes.data, W.ctypes.data, None, 48, 256, K, 0, out.ctypes.data, None) != 0


@pytest.fixture(scope="module")
def chain_ctx():
    c = runtime.Context(0)
    c.set_option("p1_f32x6_min_batch", 32)
    c.load_p1(synth.make_weights_p1(5, 1.0), _ffi.PV_DTYPE_F32)
    yield c
    c.close()


@pytest.mark.parametrize("B", [32, 64, 33])
def test_chain_is_bit_identical_with_and_without_the_stream_launch(chain_ctx, B):
    assert chain_ctx.get_option("p1_gemm6_stream") in (0, 1)
    x = synth.synth_windows(977, 64)[:B]
    got = {}
    for v in (0, 1):
        chain_ctx.set_option("p1_gemm6_stream", v)
        chain_ctx.profile_begin()
        probs, _, dec = chain_ctx.forward_p1(x, taps=True)
        assert "k_gemm_bf16x6_dec" in chain_ctx.profile_end()
        got[v] = (probs.copy(), dec.copy())
    assert np.isfinite(got[1][0]).all()
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    assert np.array_equal(got[0][1].view(np.uint32), got[1][1].view(np.uint32))
