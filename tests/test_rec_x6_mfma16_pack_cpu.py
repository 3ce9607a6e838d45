"""pack_rec_x6_16 (pepper_thesis_amd/csrc/rnn_pack_host.hpp) without a GPU: the fragment stream of the split-6 LSTM form on
v_mfma_f32_16x16x32_bf16, held bit for bit against a numpy restatement of the slot order its comment documents, on the real
dimensions (H = 256; the encoder with kx = 26 features, the decoder without an x-part), both directions. The header is compiled
alone (tests/rnn_pack_x6_shim.cpp, system C++ compiler: the conventions of tests/rnn_pack_shim.cpp) and called through ctypes.

  stream [2 dirs][8 waves][slots][3 pieces][64 lanes][8], slots = [x-part: gate, half | h-part: k-step of 32, gate, half]
  lane -> weight row gate * 256 + 32 wave + 16 half + (lane & 15), values k = 32 ks + 8 (lane >> 4) + j

Beside the restatement, on the packer's output itself: with weights that are distinct integers (exact in three bf16 pieces) every
weight of W_hh, and of W_ih for the encoder, comes back from exactly one (slot, lane, j), and the padded x columns are zero."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc")
_SRCS = [os.path.join(_HERE, "rnn_pack_x6_shim.cpp"), os.path.join(_CSRC, "rnn_pack_host.hpp"), os.path.join(_CSRC, "split3_host.hpp")]
GUARD = 16
H, NW, NG, KS_H = 256, 8, 4, 8
KX, KXP = 26, 32


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_rnn_pack_x6_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.shim_pack_rec_x6_16.restype = C.c_int64
    lib.shim_split3.restype = None
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def pack(shim, w_ih, w_hh, kx):
    """the packer's stream as [2][8][slots][3][64][8]; the element count and a guard behind the buffer are checked"""
    nslot = (NG * 2 if kx else 0) + KS_H * NG * 2
    n = 2 * NW * nslot * 3 * 512
    buf = np.full(n + GUARD, 0xAB, np.uint16)
    got = shim.shim_pack_rec_x6_16(_p(w_ih), _p(w_hh), C.c_int(kx), _p(buf), C.c_int64(n))
    assert got == n, "the packer made %d elements, the layout documents %d" % (got, n)
    assert np.all(buf[n:] == 0xAB)
    return buf[:n].reshape(2, NW, nslot, 3, 64, 8)


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


def restate_h(w_hh):
    """values of the h-part slots [2][8][ks][gate][half][lane][j]"""
    d, w, ks, g, c, lane, j = (_ax(n, i, 7) for i, n in enumerate((2, NW, KS_H, NG, 2, 64, 8)))
    return w_hh[d, g * H + 32 * w + 16 * c + (lane & 15), 32 * ks + 8 * (lane >> 4) + j]


def restate_x(w_ih):
    """values of the x-part slots [2][8][gate][half][lane][j], K padded 26 -> 32 with zeros"""
    pad = np.zeros((2, NG * H, KXP), np.float32)
    pad[:, :, :KX] = w_ih
    d, w, g, c, lane, j = (_ax(n, i, 6) for i, n in enumerate((2, NW, NG, 2, 64, 8)))
    return pad[d, g * H + 32 * w + 16 * c + (lane & 15), 8 * (lane >> 4) + j]


def random_weights(seed, kx):
    rng = np.random.default_rng(seed)
    w_ih = rng.standard_normal((2, NG * H, kx)).astype(np.float32) if kx else None
    return w_ih, rng.standard_normal((2, NG * H, H)).astype(np.float32)


def test_decoder_stream_is_the_documented_slot_order(shim):
    _, w_hh = random_weights(61, 0)
    got = pack(shim, None, w_hh, 0)
    ref = pieces(shim, restate_h(w_hh)).reshape(2, NW, KS_H * NG * 2, 3, 64, 8)
    assert np.array_equal(got, ref)


def test_encoder_stream_has_the_x_slots_in_front(shim):
    w_ih, w_hh = random_weights(62, KX)
    got = pack(shim, w_ih, w_hh, KX)
    ref_x = pieces(shim, restate_x(w_ih)).reshape(2, NW, NG * 2, 3, 64, 8)
    ref_h = pieces(shim, restate_h(w_hh)).reshape(2, NW, KS_H * NG * 2, 3, 64, 8)
    assert np.array_equal(got[:, :, :NG * 2], ref_x)
    assert np.array_equal(got[:, :, NG * 2:], ref_h)


def values_of(slots):
    """x0 + x1 + x2 of every (slot, lane, j): exact for the integer weights below"""
    f = (slots.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f.sum(axis=-3)


@pytest.mark.parametrize("kx", [0, KX])
def test_every_weight_sits_in_exactly_one_place(shim, kx):
    # distinct integers below 2^24, a different set per direction and matrix: exact in fp32 and in three 8-bit pieces
    w_hh = (1 + np.arange(2 * NG * H * H, dtype=np.float32)).reshape(2, NG * H, H)
    w_ih = (-1 - np.arange(2 * NG * H * kx, dtype=np.float32)).reshape(2, NG * H, kx) if kx else None
    got = pack(shim, w_ih, w_hh, kx)
    nx = NG * 2 if kx else 0
    for d in range(2):
        vh = values_of(got[d, :, nx:])
        assert np.array_equal(np.sort(vh.ravel()), np.sort(w_hh[d].ravel().astype(np.float64)))
        if kx:
            vx = values_of(got[d, :, :nx])                                  # [8 waves][gate, half][64][8]
            real = (8 * (np.arange(64)[:, None] >> 4) + np.arange(8)[None, :]) < kx   # (lane, j) of a real feature
            assert np.array_equal(np.sort(vx[..., real].ravel()), np.sort(w_ih[d].ravel().astype(np.float64)))
            assert np.all(got[d, :, :nx][..., ~real] == 0)                  # all three pieces of the padded columns
