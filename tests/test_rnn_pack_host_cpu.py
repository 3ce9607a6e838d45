"""The weight packers of pepper_thesis_amd/csrc/rnn_pack_host.hpp without a GPU: every fragment layout the recurrent kernels
read, held bit for bit against a numpy restatement of the layout as its comment in the header documents it, on the models'
real dimensions (LSTM H = 256 with K = 26 and 512; GRU H = 128 with 10 and 256 features; the 512 x 512 and 512 x 16896
linear layers; the 5 x 256 dense layer), with random weights from a fixed seed. The header is compiled alone
(tests/rnn_pack_shim.cpp, system C++ compiler) and called through ctypes.

A restatement indexes the PyTorch-layout matrix with broadcast index arrays shaped like the packed stream; bf16 pieces come
from the shim's split3 (the rule itself: tests/test_split3_host_cpu.py). Padding positions - features beyond the real input
width, classes beyond five - are asserted zero on the packer's output itself."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc")
_SRCS = [os.path.join(_HERE, "rnn_pack_shim.cpp"), os.path.join(_CSRC, "rnn_pack_host.hpp"), os.path.join(_CSRC, "split3_host.hpp")]
GUARD = 16
LH, GH = 256, 128   # hidden units: P1's LSTM, P2's GRU


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_rnn_pack_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    for name in ("shim_split8_rows", "shim_pack_lstm", "shim_pack_lstm_split", "shim_pack_linear", "shim_pack_gru", "shim_pack_gru_us",
                 "shim_pack_rec_bf16", "shim_pack_gru16_bf16", "shim_pack_tail_bf16", "shim_pack_p2_dense"):
        getattr(lib, name).restype = C.c_int64
    lib.shim_split3.restype = None
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _i64(v):
    return C.c_int64(int(v))


def _out(n, dtype):
    """a buffer of the documented size with a guard behind it"""
    return np.full(n + GUARD, 0xAB if dtype == np.uint16 else 7.0, dtype)


def _done(buf, n, got):
    assert got == n, "the packer made %d elements, the layout documents %d" % (got, n)
    assert np.all(buf[n:] == (0xAB if buf.dtype == np.uint16 else 7.0))
    return buf[:n]


def _rnn(seed, gates, hid, k):
    """both directions of one layer in PyTorch layout: w_ih [2][G*H][K], w_hh [2][G*H][H], b_ih, b_hh [2][G*H]"""
    rng = np.random.default_rng(seed)
    rows = gates * hid
    w_ih = rng.standard_normal((2, rows, k)).astype(np.float32) if k else None
    return (w_ih, rng.standard_normal((2, rows, hid)).astype(np.float32), rng.standard_normal((2, rows)).astype(np.float32),
            rng.standard_normal((2, rows)).astype(np.float32))


def _xh(w_ih, w_hh, kp):
    """[x (K real columns, padded with zeros to KP) | h] per direction"""
    k = w_ih.shape[2]
    cat = np.zeros((2, w_ih.shape[1], kp + w_hh.shape[2]), np.float32)
    cat[:, :, :k] = w_ih
    cat[:, :, kp:] = w_hh
    return cat


def _ax(n, pos, ndim):
    """arange(n) along axis `pos` of an ndim-dimensional broadcast"""
    shape = [1] * ndim
    shape[pos] = n
    return np.arange(n).reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pieces(shim, v):
    """bf16 pieces of every value: [..., 3] uint16"""
    v = np.ascontiguousarray(v, np.float32)
    out = np.zeros(v.shape + (3,), np.uint16)
    shim.shim_split3(_p(v), _i64(v.size), _p(out))
    return out


def _slots(shim, v, pieces=2):
    """values [..., 64 lanes, 8] -> slots [..., pieces, 64, 8]: piece q of (lane, j) at 2-byte index 512 q + 8 lane + j"""
    return np.moveaxis(_pieces(shim, v)[..., :pieces], -1, -3)


# ---- split8 rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(768, 256), (2048, 512), (512, 16896)])
def test_split8_rows(shim, N, K):
    w = np.random.default_rng(8).standard_normal((N, K)).astype(np.float32)
    buf = _out(2 * N * K, np.uint16)
    rows = _done(buf, 2 * N * K, shim.shim_split8_rows(_p(w), _i64(N), _i64(K), _p(buf), _i64(2 * N * K))).reshape(N, 2 * K)
    k = np.arange(K)
    off = (k >> 3) * 32 + (k & 7) * 2       # byte offset of element k inside a row of K * 4 bytes; lo: + 16
    assert off.max() + 16 + 2 <= K * 4
    pc = _pieces(shim, w)
    assert np.array_equal(rows[:, off // 2], pc[:, :, 0])
    assert np.array_equal(rows[:, (off + 16) // 2], pc[:, :, 1])
    assert len(np.unique(np.concatenate([off, off + 16]))) == 2 * K   # every 2-byte cell of a row is written once


# ---- fp32 fragments --------------------------------------------------------------------------------------------------------
def _frag_nk(tr, col0, kb, lane, last):
    """(column, k) of the four values of a lane in the two tile forms (mfma_tiles.hpp): 32 rows: column col0 + (lane & 31),
    k = 8 kb + 4 (lane >> 5) + j; 16 rows: {t0 j0, t0 j1, t1 j0, t1 j1}, column col0 + 16 t + (lane & 15), k = 8 kb + 2 (lane >> 4) + j"""
    if tr == 32:
        return col0 + (lane & 31) + 0 * last, kb * 8 + 4 * (lane >> 5) + last
    t, j = last >> 1, last & 1
    return col0 + 16 * t + (lane & 15), kb * 8 + 2 * (lane >> 4) + j


@pytest.mark.parametrize("K,KP", [(26, 32), (512, 512)])
@pytest.mark.parametrize("TR", [32, 16])
def test_pack_lstm(shim, K, KP, TR):
    w_ih, w_hh, b_ih, b_hh = _rnn(11, 4, LH, K)
    nkb = (KP + LH) // 8
    n = 2 * 8 * nkb * 4 * 256
    buf, bias = _out(n, np.float32), _out(2 * 4 * LH, np.float32)
    nb = C.c_int64(0)
    got = shim.shim_pack_lstm(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), K, KP, TR, _p(buf), _i64(n), _p(bias), _i64(2 * 4 * LH), C.byref(nb))
    wp = _done(buf, n, got).reshape(2, 8, nkb, 4, 64, 4)   # [dir][wave][k-block][gate][lane][4]
    assert np.array_equal(_bits(_done(bias, 2 * 4 * LH, nb.value)), _bits((b_ih + b_hh).reshape(-1)))
    d, w, kb, nt, lane, last = (_ax(s, i, 6) for i, s in enumerate(wp.shape))
    col, k = _frag_nk(TR, nt * LH + 32 * w, kb, lane, last)
    assert np.array_equal(_bits(wp), _bits(_xh(w_ih, w_hh, KP)[d, col, k]))
    pad = np.broadcast_to((k >= K) & (k < KP), wp.shape)
    assert pad.any() == (K < KP) and np.all(_bits(wp)[pad] == 0)   # features beyond the real ones


@pytest.mark.parametrize("K,KP", [(26, 32), (512, 512)])
@pytest.mark.parametrize("parts", [4, 2])
def test_pack_lstm_split(shim, K, KP, parts):
    w_ih, w_hh, b_ih, b_hh = _rnn(12, 4, LH, K)
    nkb, nw = (KP + LH) // 8, 16 // parts
    n = 2 * 16 * nkb * 2 * 256
    buf = _out(n, np.float32)
    got = shim.shim_pack_lstm_split(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), K, KP, parts, _p(buf), _i64(n))
    wp = _done(buf, n, got).reshape(2, parts, nw, nkb, 2, 64, 4)   # [dir][part][wave][k-block][2][lane][4]
    d, p, w, kb, half, lane, last = (_ax(s, i, 7) for i, s in enumerate(wp.shape))
    gate, j = 2 * half + (last >> 1), last & 1    # {i j0, i j1, f j0, f j1}, {g j0, g j1, o j0, o j1}
    col = gate * LH + (LH // parts) * p + 16 * w + (lane & 15)
    k = 8 * kb + 2 * (lane >> 4) + j
    assert np.array_equal(_bits(wp), _bits(_xh(w_ih, w_hh, KP)[d, col, k]))
    pad = np.broadcast_to((k >= K) & (k < KP), wp.shape)
    assert pad.any() == (K < KP) and np.all(_bits(wp)[pad] == 0)


@pytest.mark.parametrize("K", [512, 16896])
@pytest.mark.parametrize("TR", [32, 16])
def test_pack_linear(shim, K, TR):
    W = np.random.default_rng(13).standard_normal((512, K)).astype(np.float32)
    nkb = K // 8
    n = 4 * nkb * 4 * 256
    buf = _out(n, np.float32)
    wp = _done(buf, n, shim.shim_pack_linear(_p(W), K, TR, _p(buf), _i64(n))).reshape(4, nkb, 4, 64, 4)   # [wave][k-block][tile][lane][4]
    w, kb, nt, lane, last = (_ax(s, i, 5) for i, s in enumerate(wp.shape))
    col, k = _frag_nk(TR, 128 * w + 32 * nt, kb, lane, last)
    assert np.array_equal(_bits(wp), _bits(W[col, k]))
    assert np.array_equal(np.sort(_bits(wp).reshape(-1)), np.sort(_bits(W).reshape(-1)))   # every weight exactly once


@pytest.mark.parametrize("K,KP", [(10, 32), (256, 256)])
@pytest.mark.parametrize("TR,hx", [(32, 0), (16, 0), (16, 1)])
def test_pack_gru(shim, K, KP, TR, hx):
    w_ih, w_hh, b_ih, b_hh = _rnn(14, 3, GH, K)
    nkb = (KP + GH) // 8
    n = 2 * 4 * nkb * 3 * 256
    buf, bias = _out(n, np.float32), _out(2 * 4 * GH, np.float32)
    nb = C.c_int64(0)
    got = shim.shim_pack_gru(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), K, KP, TR, hx, _p(buf), _i64(n), _p(bias), _i64(2 * 4 * GH), C.byref(nb))
    wp = _done(buf, n, got).reshape(2, 4, nkb, 3, 64, 4)   # [dir][wave][k-block][gate r,z,n][lane][4]
    bi, bh = b_ih.reshape(2, 3, GH), b_hh.reshape(2, 3, GH)
    want_bias = np.stack([bi[:, 0] + bh[:, 0], bi[:, 1] + bh[:, 1], bi[:, 2], bh[:, 2]], axis=1)   # b_ir + b_hr, b_iz + b_hz, b_in, b_hn
    assert np.array_equal(_bits(_done(bias, 2 * 4 * GH, nb.value)), _bits(want_bias.reshape(-1)))
    d, w, kb, nt, lane, last = (_ax(s, i, 6) for i, s in enumerate(wp.shape))
    col, pos = _frag_nk(TR, nt * GH + 32 * w, kb, lane, last)
    k = np.where(pos < GH, KP + pos, pos - GH) if hx else pos   # stream order [h | x] -> position in [x | h]
    assert np.array_equal(_bits(wp), _bits(_xh(w_ih, w_hh, KP)[d, col, k]))
    pad = np.broadcast_to((k >= K) & (k < KP), wp.shape)
    assert pad.any() == (K < KP) and np.all(_bits(wp)[pad] == 0)


@pytest.mark.parametrize("K,KP", [(10, 32), (256, 256)])
def test_pack_gru_us(shim, K, KP):
    w_ih, w_hh, b_ih, b_hh = _rnn(15, 3, GH, K)
    npair = (KP + GH) // 16
    n = 2 * 2 * 4 * npair * 3 * 256
    buf = _out(n, np.float32)
    got = shim.shim_pack_gru_us(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), K, KP, _p(buf), _i64(n))
    wp = _done(buf, n, got).reshape(2, 2, 4, npair, 3, 64, 4)   # [dir][half][wave][pair of k-blocks][gate][lane][4]
    d, hf, w, pp, g, lane, last = (_ax(s, i, 7) for i, s in enumerate(wp.shape))
    col = g * GH + 64 * hf + 16 * w + (lane & 15)
    pos = 16 * pp + 8 * (last >> 1) + 2 * (lane >> 4) + (last & 1)   # in the [h | x] stream
    hxw = np.zeros((2, 3 * GH, GH + KP), np.float32)
    hxw[:, :, :GH] = w_hh
    hxw[:, :, GH:GH + K] = w_ih
    assert np.array_equal(_bits(wp), _bits(hxw[d, col, pos]))
    pad = np.broadcast_to(pos >= GH + K, wp.shape)
    assert pad.any() == (K < KP) and np.all(_bits(wp)[pad] == 0)


# ---- bf16 pieces -------------------------------------------------------------------------------------------------------------
def _rec_values(w_ih, w_hh, cell, hid, kx, xpart, nks):
    """values [dir][wave][k-step][gate][lane][8] of k_rec_bf16's fragments: row gate * HID + 32 wave + (lane & 31),
    k = 16 ks + 8 (lane >> 5) + j; x-part features beyond kx are zero"""
    if xpart:
        m = np.zeros((2, cell * hid, 16 * nks), np.float32)
        m[:, :, :kx] = w_ih
    else:
        m = w_hh
    d, w, ks, g, lane, j = (_ax(s, i, 6) for i, s in enumerate((2, hid // 32, nks, cell, 64, 8)))
    return m[d, g * hid + 32 * w + (lane & 31), 16 * ks + 8 * (lane >> 5) + j]


@pytest.mark.parametrize("cell,kx,pieces", [(4, 26, 2), (4, 0, 2), (4, 26, 3), (4, 0, 3), (3, 10, 2), (3, 0, 2)])
def test_pack_rec_bf16(shim, cell, kx, pieces):
    hid = LH if cell == 4 else GH
    nw, ks_h = hid // 32, hid // 16
    ks_x = (2 if cell == 4 else 1) if kx else 0
    xres = bool(kx) and cell == 3                # the GRU encoder's x-part: a stream of its own, [dir][wave][gate] slots of 2 KB
    w_ih, w_hh, b_ih, b_hh = _rnn(16, cell, hid, kx)
    nslot = (0 if xres else ks_x * cell) + ks_h * cell
    n, nx = 2 * nw * nslot * pieces * 512, 2 * nw * cell * 1024 if xres else 0
    buf, bx = _out(n, np.uint16), _out(nx, np.uint16)
    c_nx = C.c_int64(-1)
    got = shim.shim_pack_rec_bf16(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), cell, kx, pieces, _p(buf), _i64(n), _p(bx), _i64(nx), C.byref(c_nx))
    wp = _done(buf, n, got).reshape(2, nw, nslot, pieces, 64, 8)   # slots: [x-part k-steps x gates | h-part k-steps x gates]
    wx = _done(bx, nx, c_nx.value)
    hpart = _slots(shim, _rec_values(w_ih, w_hh, cell, hid, kx, False, ks_h), pieces).reshape(2, nw, ks_h * cell, pieces, 64, 8)
    nxs = 0 if xres else ks_x * cell
    assert np.array_equal(wp[:, :, nxs:], hpart)
    if kx:
        xv = _rec_values(w_ih, w_hh, cell, hid, kx, True, ks_x)
        xpart = _slots(shim, xv, pieces).reshape(2, nw, ks_x * cell, pieces, 64, 8)
        got_x = wx.reshape(2, nw, cell, 2, 64, 8) if xres else wp[:, :, :nxs]
        assert np.array_equal(got_x, xpart)
        lane, j = _ax(64, 4, 6), _ax(8, 5, 6)
        k = 16 * _ax(ks_x, 2, 6) + 8 * (lane >> 5) + j + 0 * _ax(cell, 3, 6)
        pad = np.broadcast_to((k >= kx).reshape(1, 1, ks_x * cell, 1, 64, 8), got_x.shape)
        assert pad.any() and np.all(got_x[pad] == 0)       # features beyond kx, in every piece


@pytest.mark.parametrize("kx", [10, 0])
def test_pack_gru16_bf16(shim, kx):
    w_ih, w_hh, b_ih, b_hh = _rnn(17, 3, GH, kx)
    n, nx = 2 * 4 * 24 * 1024, 2 * 4 * 6 * 1024 if kx else 0
    buf, bx = _out(n, np.uint16), _out(nx, np.uint16)
    c_nx = C.c_int64(-1)
    got = shim.shim_pack_gru16_bf16(_p(w_ih), _p(w_hh), _p(b_ih), _p(b_hh), kx, _p(buf), _i64(n), _p(bx), _i64(nx), C.byref(c_nx))
    wp = _done(buf, n, got).reshape(2, 4, 4, 3, 2, 2, 64, 8)   # [dir][wave] 24 slots (ks * 3 + g) * 2 + nt of [hi | lo]
    wx = _done(bx, nx, c_nx.value)
    d, w, ks, g, nt, lane, j = (_ax(s, i, 7) for i, s in enumerate((2, 4, 4, 3, 2, 64, 8)))
    unit = g * GH + 32 * w + 16 * nt + (lane & 15)
    k = 32 * ks + 8 * (lane >> 4) + j
    assert np.array_equal(wp, _slots(shim, w_hh[d, unit, k]))
    if kx:
        m = np.zeros((2, 3 * GH, 32), np.float32)
        m[:, :, :kx] = w_ih
        got_x = wx.reshape(2, 4, 3, 2, 2, 64, 8)               # [dir][wave] 6 slots g * 2 + nt
        d, w, g, nt, lane, j = (_ax(s, i, 6) for i, s in enumerate((2, 4, 3, 2, 64, 8)))
        k = 8 * (lane >> 4) + j
        assert np.array_equal(got_x, _slots(shim, m[d, g * GH + 32 * w + 16 * nt + (lane & 15), k]))
        pad = np.broadcast_to((k >= kx).reshape(1, 1, 1, 1, 1, 64, 8), got_x.shape)
        assert pad.any() and np.all(got_x[pad] == 0)


def test_pack_tail_bf16(shim):
    w = np.random.default_rng(18).standard_normal((4, 512, 512)).astype(np.float32)
    n = 8 * 4 * 32 * 2 * 1024
    buf = _out(n, np.uint16)
    wp = _done(buf, n, shim.shim_pack_tail_bf16(_p(w), _p(buf), _i64(n))).reshape(8, 4, 32, 2, 2, 64, 8)   # [wave][layer][k-step][tile][hi | lo]
    wv, l, ks, g, lane, j = (_ax(s, i, 6) for i, s in enumerate((8, 4, 32, 2, 64, 8)))
    assert np.array_equal(wp, _slots(shim, w[l, 64 * wv + 32 * g + (lane & 31), 16 * ks + 8 * (lane >> 5) + j]))


@pytest.mark.parametrize("rows16", [0, 1])
def test_pack_p2_dense(shim, rows16):
    dense = np.random.default_rng(19).standard_normal((5, 2 * GH)).astype(np.float32)
    m = np.zeros((32, 2 * GH), np.float32)    # classes beyond the five are zero
    m[:5] = dense
    n = 2 * 4 * 1024 if rows16 else 2 * 4 * 2 * 1024
    buf = _out(n, np.uint16)
    f = _done(buf, n, shim.shim_pack_p2_dense(_p(dense), rows16, _p(buf), _i64(n)))
    if rows16:   # wave w of direction d: k-step w of 32 units; lane -> class lane & 15, k = 32 w + 8 (lane >> 4) + j
        f = f.reshape(2, 4, 2, 64, 8)
        d, w, lane, j = (_ax(s, i, 4) for i, s in enumerate((2, 4, 64, 8)))
        cls, k = (lane & 15) + 0 * d, 32 * w + 8 * (lane >> 4) + j
    else:        # k-steps 2w, 2w + 1 of 16 units; lane -> class lane & 31, k = 16 ks + 8 (lane >> 5) + j
        f = f.reshape(2, 4, 2, 2, 64, 8)
        d, w, kk, lane, j = (_ax(s, i, 5) for i, s in enumerate((2, 4, 2, 64, 8)))
        cls, k = (lane & 31) + 0 * d, 16 * (2 * w + kk) + 8 * (lane >> 5) + j
    assert np.array_equal(f, _slots(shim, m[cls, d * GH + k]))
    pad = np.broadcast_to(np.expand_dims(np.broadcast_to(cls >= 5, np.broadcast(cls, k).shape), -3), f.shape)
    assert pad.any() and np.all(f[pad] == 0)
