"""pack_gemm6_stream (pepper_thesis_amd/csrc/rnn_pack_host.hpp) without a GPU: the weight stream of k_gemm_x6_stream, held bit for
bit against a numpy restatement of the slot order its comment documents. The header is compiled alone
(tests/gemm6_stream_pack_shim.cpp, system C++ compiler) and called through ctypes.

  stream [8 waves][N / 512 blocks][K / 32 k-steps][4 column tiles][3 pieces][64 lanes][8]
  lane -> weight row wave * N / 8 + 64 block + 16 tile + (lane & 15), values k = 32 ks + 8 (lane >> 4) + j

Shapes: the decoder projection's (N, K) = (2048, 512) and (512, 64), one block per wave and two k-steps. Beside the restatement,
on the packer's output itself: with weights that are distinct integers (exact in three bf16 pieces) every weight comes back
from exactly one (slot, lane, j); and with weights whose three pieces are all non-zero every piece sits in its own 1 KB of the
slot."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc")
_SRCS = [os.path.join(_HERE, "gemm6_stream_pack_shim.cpp"), os.path.join(_CSRC, "rnn_pack_host.hpp"), os.path.join(_CSRC, "split3_host.hpp")]
GUARD = 16
SHAPES = [(2048, 512), (512, 64)]


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_gemm6_stream_pack_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.shim_pack_gemm6_stream.restype = C.c_int64
    lib.shim_split3.restype = None
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pack(shim, w):
    """the packer's stream as [8][N / 512][K / 32][4][3][64][8]; the element count and a guard behind the buffer are checked"""
    N, K = w.shape
    n = 3 * N * K
    buf = np.full(n + GUARD, 0xAB, np.uint16)
    got = shim.shim_pack_gemm6_stream(_p(w), C.c_int64(N), C.c_int64(K), _p(buf), C.c_int64(n))
    assert got == n, "the packer made %d elements, the layout documents %d" % (got, n)
    assert np.all(buf[n:] == 0xAB)
    return buf[:n].reshape(8, N // 512, K // 32, 4, 3, 64, 8)


def pieces(shim, v):
    """bf16 pieces of values [..., 64 lanes, 8] as slots [..., 3, 64, 8]"""
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros(v.shape + (3,), np.uint16)
    shim.shim_split3(_p(v), C.c_int64(v.size), _p(out))
    return np.moveaxis(out, -1, -3)


def _ax(n, pos, ndim):
    shape = [1] * ndim
    shape[pos] = n
    return np.arange(n).reshape(shape)


def restate(w):
    """values of the slots [8][N / 512][K / 32][4][lane][j]"""
    N, K = w.shape
    wv, b, ks, ct, lane, j = (_ax(n, i, 6) for i, n in enumerate((8, N // 512, K // 32, 4, 64, 8)))
    return w[wv * (N // 8) + 64 * b + 16 * ct + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]


def values_of(slots):
    """x0 + x1 + x2 of every (slot, lane, j)"""
    f = (slots.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f.sum(axis=-3)


@pytest.mark.parametrize("N,K", SHAPES)
def test_stream_is_the_documented_slot_order(shim, N, K):
    w = np.random.default_rng(N + K).standard_normal((N, K)).astype(np.float32)
    assert np.array_equal(pack(shim, w), pieces(shim, restate(w)))


@pytest.mark.parametrize("N,K", SHAPES)
def test_every_weight_sits_in_exactly_one_place(shim, N, K):
    # distinct integers below 2^24: exact in fp32 and in three 8-bit pieces
    w = (1 + np.arange(N * K, dtype=np.float32)).reshape(N, K)
    got = values_of(pack(shim, w))
    assert np.array_equal(np.sort(got.ravel()), w.ravel().astype(np.float64))
    assert np.array_equal(got, restate(w).astype(np.float64))


@pytest.mark.parametrize("N,K", SHAPES)
def test_three_nonzero_pieces_each_in_its_own_plane_of_the_slot(shim, N, K):
    # odd integers of 18 to 24 bits: x1 and x2 are non-zero for most; keep those and tile them over W
    rng = np.random.default_rng(7 * N + K)
    pool = (rng.integers(1 << 17, 1 << 24, 8 * N * K // 4) | 1).astype(np.float32)
    sp = pieces(shim, np.resize(pool, (pool.size // 512, 64, 8)))
    ok = np.all(sp.reshape(-1, 3, 64, 8) != 0, axis=1).ravel()
    pool = np.resize(pool[:ok.size][ok], N * K)
    w = (pool * rng.choice([-1, 1], N * K)).astype(np.float32).reshape(N, K)
    got = pack(shim, w)
    assert np.all(got != 0)
    ref = pieces(shim, restate(w))
    for q in range(3):
        assert np.array_equal(got[..., q, :, :], ref[..., q, :, :]), "piece %d" % q
    assert np.array_equal(values_of(got), restate(w).astype(np.float64))
