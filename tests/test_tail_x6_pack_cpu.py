"""pack_tail_x6 (pepper_thesis_amd/csrc/rnn_pack_host.hpp) without a GPU: the three-piece fragment stream of the split-6 chain's
tail (k_tail_bf16<X6>: linear_2..5 as six-term products), held bit for bit against a numpy restatement of the slot order its
comment documents, on the real dimensions (four 512 x 512 layers). The header is compiled alone (tests/tail_x6_pack_shim.cpp,
system C++ compiler: the conventions of tests/rnn_pack_x6_shim.cpp) and called through ctypes.

  stream [8 waves][4 layers][32 k-steps][2 column tiles][3 pieces][64 lanes][8]
  lane -> weight row 64 wave + 32 tile + (lane & 31), values k = 16 ks + 8 (lane >> 5) + j

1. the stream equals the restatement, the pieces made by the header's own split3_bits;
2. the pieces equal torch's bfloat16 rounding (round to nearest even) of w, of fp32(w - x0) and of fp32(w - x0 - x1);
3. x0 + x1 + x2 == w exactly (float64 sum) for normal weights of trained magnitude;
4. with weights that are distinct integers (exact in three bf16 pieces) every weight of the four layers comes back from exactly
   one (slot, lane, j), and each piece plane holds that weight's own piece."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc")
_SRCS = [os.path.join(_HERE, "tail_x6_pack_shim.cpp"), os.path.join(_CSRC, "rnn_pack_host.hpp"), os.path.join(_CSRC, "split3_host.hpp")]
GUARD = 16
N, NW, NL, KS, NT = 512, 8, 4, 32, 2
COUNT = NW * NL * KS * NT * 3 * 512


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_tail_x6_pack_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.shim_pack_tail_x6.restype = C.c_int64
    lib.shim_split3.restype = None
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pack(shim, w):
    """the packer's stream as [8][4][32][2][3][64][8]; the element count and a guard behind the buffer are checked"""
    w = np.ascontiguousarray(w, np.float32)
    assert w.shape == (NL, N, N)
    buf = np.full(COUNT + GUARD, 0xAB, np.uint16)
    got = shim.shim_pack_tail_x6(_p(w), _p(buf), C.c_int64(COUNT))
    assert got == COUNT, "the packer made %d elements, the layout documents %d (6.3 MB)" % (got, COUNT)
    assert np.all(buf[COUNT:] == 0xAB)
    return buf[:COUNT].reshape(NW, NL, KS, NT, 3, 64, 8)


def _ax(n, pos, ndim):
    shape = [1] * ndim
    shape[pos] = n
    return np.arange(n).reshape(shape)


def restate(w):
    """values of the slots [8 waves][4 layers][32 ks][2 tiles][64 lanes][8]"""
    wv, l, ks, g, lane, j = (_ax(n, i, 6) for i, n in enumerate((NW, NL, KS, NT, 64, 8)))
    return w[l, 64 * wv + 32 * g + (lane & 31), 16 * ks + 8 * (lane >> 5) + j]


def pieces_shim(shim, v):
    """bf16 pieces of values [..., 64, 8] as [..., 3, 64, 8], by the header's split3_bits"""
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros(v.shape + (3,), np.uint16)
    shim.shim_split3(_p(v), C.c_int64(v.size), _p(out))
    return np.moveaxis(out, -1, -3)


def _bf16(x):
    """torch's bfloat16 rounding of fp32 values, as fp32"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _vals(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


@pytest.fixture(scope="module")
def trained():
    """weights of trained magnitude: N(0, 1/sqrt(512)) times a per-layer gain, a few exact powers of two and zeros among them"""
    rng = np.random.default_rng(71)
    w = (rng.standard_normal((NL, N, N)) / np.sqrt(N)).astype(np.float32) * np.array([1, 2, 0.5, 4], np.float32)[:, None, None]
    w[0, 0, :8] = [1.0, -1.0, 0.5, 0.0, 2.0 ** -10, 3.0, -0.0, 257.0]
    return w


@pytest.fixture(scope="module")
def trained_stream(shim, trained):
    return pack(shim, trained)


def test_stream_is_the_documented_slot_order(shim, trained, trained_stream):
    assert np.array_equal(trained_stream, pieces_shim(shim, restate(trained)))


def test_pieces_are_torch_bfloat16_roundings(trained, trained_stream):
    v = restate(trained)
    x0 = _bf16(v)
    r1 = v - x0                       # fp32, exact
    x1 = _bf16(r1)
    x2 = _bf16(r1 - x1)
    for p, want in enumerate((x0, x1, x2)):
        assert np.array_equal(trained_stream[..., p, :, :], _bits(want)), "piece %d" % p


def test_three_pieces_give_the_weight_back(trained, trained_stream):
    v = restate(trained)
    assert np.isfinite(v).all() and (np.abs(v[v != 0]) >= 2.0 ** -100).all()    # normal, third piece far from subnormal
    total = _vals(trained_stream).astype(np.float64).sum(axis=-3)
    assert np.array_equal(total, v.astype(np.float64))


def test_every_weight_sits_in_exactly_one_place_per_piece(shim):
    # distinct integers below 2^24 over the four layers: exact in fp32 and in three 8-bit pieces
    w = (1 + np.arange(NL * N * N, dtype=np.float32)).reshape(NL, N, N)
    got = pack(shim, w)
    total = _vals(got).astype(np.float64).sum(axis=-3)                        # [8][4][32][2][64][8]
    for l in range(NL):
        assert np.array_equal(np.sort(total[:, l].ravel()), w[l].ravel().astype(np.float64)), "layer %d" % l
    # ... and every piece plane holds, at the place of weight v, the piece of v: no plane is permuted against another
    want = pieces_shim(shim, total.astype(np.float32))
    assert np.array_equal(got, want)
