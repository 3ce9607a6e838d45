"""GPU: k_gemm_bf16x6 with host-split weight planes and 256 x 128 work items (one wave per 32 rows), through
pv_debug_gemm_bf16x6, which pre-splits W with the function the model load uses.

Layout cases: integer operands in [-8, 8] have one non-zero piece and every sum is exact, so the result must equal the integer
product exactly, slab by slab: a wrong row, column, K position, item walk, bias slot or epilogue offset shows as a wrong
integer. The debug entry keeps a guard of 256 rows behind C and fails the call when a row is stored past M, so the ragged
cases also prove that replicated rows are dropped by both epilogues. One case gives A odd integers of 18 to 20 bits whose
third piece is non-zero (asserted on the host split), four per row, with W integers in [-2, 2]: every partial sum is an integer
below 2^24, hence exact, and a dropped or misrouted A piece changes the integer.
Piece cases: every output is ONE six-term product a . w of full 24-bit values, within 2^-21 of the float64 product (three
dropped terms below 2^-24 each, five fp32 roundings of the accumulation).
fp32-class bar: the bar of test_p1_f32x6_gpu.test_gemm_bf16x6_is_fp32_class at a ragged two-item shape."""
import numpy as np
import pytest

from pepper_thesis_amd import _ffi

pytestmark = pytest.mark.gpu


def _gemm(ctx, A, W, b, splits, quads):
    """the slabs [splits][M][N] as float64"""
    lib = _ffi.load()
    M, K = A.shape
    N = W.shape[0]
    out = np.zeros((splits, M, N), np.float32)
    _ffi.check(lib.pv_debug_gemm_bf16x6(ctx.handle, A.ctypes.data, W.ctypes.data, None if b is None else b.ctypes.data,
                                        M, N, K, splits, quads, out.ctypes.data, None))
    if quads:
        out = out.reshape(M // 4, N, 4).transpose(0, 2, 1).reshape(1, M, N)
    return out.astype(np.float64)


def _slabs(A, W, b, splits):
    """the exact slabs in float64 (integer operands: every product and sum is exact)"""
    ks = A.shape[1] // splits
    ref = np.stack([A[:, s * ks:(s + 1) * ks].astype(np.float64) @ W[:, s * ks:(s + 1) * ks].astype(np.float64).T for s in range(splits)])
    return ref if b is None else ref + b.astype(np.float64)


LAYOUT = [(4, 256, 32, 1, 0, False),       # less than one wave's rows, a single K step
          (36, 256, 64, 1, 1, False),      # two waves, quads
          (252, 256, 64, 1, 0, False), (252, 256, 64, 1, 1, False),   # ragged last tile: replicated rows never stored
          (260, 256, 64, 1, 0, False), (260, 256, 64, 1, 1, False),
          (256, 256, 64, 2, 0, False),     # one K step per slab
          (4352, 2048, 64, 1, 1, True),    # 272 items on 256 workgroups: second item, n-tile wrap, cross-item prefetch, bias slots
          (516, 512, 1056, 11, 0, False)]  # linear_1's slab shape at 3 K steps per slab


@pytest.mark.parametrize("M,N,K,splits,quads,bias", LAYOUT)
def test_layout_integer_operands_are_exact(hip_ctx, M, N, K, splits, quads, bias):
    rng = np.random.default_rng(M * 7 + N + K + quads)
    A = rng.integers(-8, 9, (M, K)).astype(np.float32)
    W = rng.integers(-8, 9, (N, K)).astype(np.float32)
    b = rng.integers(-8, 9, N).astype(np.float32) if bias else None
    got = _gemm(hip_ctx, A, W, b, splits, quads)
    assert np.array_equal(got, _slabs(A, W, b, splits))


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
    every product and partial sum is an integer below 4 * 2^20 * 2 = 2^23, so the result is the exact integer product, and it
    is not if a2 . b0 (or any other A piece) is dropped or takes another row tile's registers"""
    M, N, K = 36, 256, 64
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
    ref = _slabs(A, W, None, 1)
    # the case can see each piece: without it the integer differs in some output
    for drop in _split3(A):
        assert not np.array_equal((A.astype(np.float64) - drop) @ W.astype(np.float64).T, ref[0])
    for quads in (0, 1):
        assert np.array_equal(_gemm(hip_ctx, A, W, None, 1, quads), ref)


@pytest.mark.parametrize("quads", [0, 1])
def test_single_products_keep_24_bits(hip_ctx, quads):
    M, N, K = 260, 256, 256
    rng = np.random.default_rng(5 + quads)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    A *= np.logspace(-20, 3, M)[:, None].astype(np.float32)
    kn = (np.arange(N) * 37 + 5) % K                       # a different k per row of W (37 is prime to 256)
    assert len(set(kn.tolist())) == N
    w = (rng.uniform(0.5, 2, N) * rng.choice([-1, 1], N)).astype(np.float32)
    w = (w.view(np.uint32) | np.uint32(1)).view(np.float32)   # full 24-bit values: the last significand bit set
    W = np.zeros((N, K), np.float32)
    W[np.arange(N), kn] = w
    got = _gemm(hip_ctx, A, W, None, 1, quads)[0]
    ref = A[:, kn].astype(np.float64) * w.astype(np.float64)[None, :]
    assert np.all(ref != 0)
    rel = np.abs(got - ref) / np.abs(ref)
    print("max relative error of a six-term product: 2^%.2f" % np.log2(rel.max() + 1e-300))
    assert rel.max() <= 2.0 ** -21, rel.max()


def test_fp32_class_on_two_ragged_items(hip_ctx):
    """the operand recipe and the bar of test_gemm_bf16x6_is_fp32_class"""
    M, N, K, splits, quads = 260, 256, 512, 1, 1
    rng = np.random.default_rng(M + K)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    A[:24] *= np.logspace(-20, 3, 24)[:, None].astype(np.float32)
    A[30] = 0.0
    W[40] = 0.0
    A[M - 1] = rng.uniform(-1, 1, K).astype(np.float32) * 1e3
    b = rng.uniform(-1, 1, N).astype(np.float32)
    got = _gemm(hip_ctx, A, W, b, splits, quads)[0]
    ref = A.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    f32 = (A @ W.T + b).astype(np.float64)
    mag = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b).astype(np.float64) + 1e-300
    e6 = float(np.max(np.abs(got - ref) / mag))
    e32 = float(np.max(np.abs(f32 - ref) / mag))
    assert np.isfinite(got).all()
    assert np.all(got[30] == b) and np.all(got[:, 40] == b[40])
    assert e6 <= 2 * e32, (e6, e32)
