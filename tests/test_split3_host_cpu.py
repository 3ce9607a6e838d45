"""The host-side piece rule of the split-6 products (pepper_thesis_amd/csrc/split3_host.hpp: x0 = rne_bf16(x),
x1 = rne_bf16(x - x0), x2 = rne_bf16(x - x0 - x1)) without a GPU. The header is compiled alone (tests/split3_shim.cpp, system
C++ compiler) and called through ctypes; the reference is torch's float -> bfloat16 conversion on float64 residuals.

The exact-sum property is asserted where the value the third piece has to hold (the second residual) is zero or a normal
bf16: a residual below 2^-126 is lost or rounded whether the piece that comes out of it is subnormal, zero or 2^-126, so the
condition is taken on the residual, not on the piece."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, "split3_shim.cpp"), os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc", "split3_host.hpp")]
BF16_MIN_NORMAL = 2.0 ** -126


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_split3_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.shim_split3.argtypes, lib.shim_split3.restype = [C.c_void_p, C.c_int64, C.c_void_p], None
    lib.shim_split3_planes.argtypes, lib.shim_split3_planes.restype = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p], None
    return lib


def _values():
    rng = np.random.default_rng(20240)
    bits = rng.integers(0, 1 << 32, 50000, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every exponent, subnormals too
    bits = bits[np.isfinite(bits)]
    gauss = (rng.standard_normal(50000) * np.exp(rng.uniform(-20, 20, 50000))).astype(np.float32)
    pow2 = np.ldexp(np.float32(1), np.arange(-126, 128)).astype(np.float32)
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    # all 24 significand bits set, at exponents over the whole range
    ones = ((np.arange(1, 255, dtype=np.uint32) << 23) | np.uint32(0x7FFFFF)).view(np.float32)
    edge = np.array([0.0, -0.0, fmax, -fmax, fmin, -fmin], np.float32)
    return np.concatenate([bits, gauss, pow2, -pow2, ones, -ones, edge]).astype(np.float32)


def _bf16_bits(v64):
    """bits of torch's bfloat16 of float64 values (each of them exact in fp32 here)"""
    return torch.from_numpy(np.ascontiguousarray(v64)).to(torch.float32).bfloat16().view(torch.int16).numpy().view(np.uint16)


def _bf16_val(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _same(got, want):
    """equal bits, or both NaN (FLT_MAX rounds to inf: its residuals are -inf and NaN, whose sign is not specified)"""
    nan = lambda b: ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)
    return (got == want) | (nan(got) & nan(want))


def test_split3_pieces(shim):
    x = _values()
    assert len(x) > 100000
    out = np.zeros((len(x), 3), np.uint16)
    shim.shim_split3(x.ctypes.data, len(x), out.ctypes.data)
    p0, p1, p2 = out[:, 0], out[:, 1], out[:, 2]
    want0 = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(p0, want0)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        r1 = x64 - _bf16_val(p0)
        assert np.all(_same(p1, _bf16_bits(r1)))
        r2 = r1 - _bf16_val(p1)
        assert np.all(_same(p2, _bf16_bits(r2)))
        total = _bf16_val(p0) + _bf16_val(p1) + _bf16_val(p2)
    normal = np.isfinite(x) & (np.abs(x64) >= np.finfo(np.float32).tiny) & np.isfinite(_bf16_val(p0))
    exact = normal & ((r2 == 0) | (np.abs(r2) >= BF16_MIN_NORMAL))
    assert exact.sum() > 0.7 * len(x)
    assert np.array_equal(total[exact], x64[exact])
    # signed zeros stay zeros in every piece
    z = out[np.flatnonzero(x == 0)]
    assert np.all((z & 0x7FFF) == 0)


def test_split3_planes_layout(shim):
    N, K = 5, 24
    w = np.random.default_rng(3).standard_normal((N, K)).astype(np.float32)
    planes = np.full(3 * N * K + 8, 0xABCD, np.uint16)   # (a guard behind the planes)
    shim.shim_split3_planes(w.ctypes.data, N, K, planes.ctypes.data)
    assert np.all(planes[3 * N * K:] == 0xABCD)
    pieces = np.zeros((N * K, 3), np.uint16)
    shim.shim_split3(w.ctypes.data, N * K, pieces.ctypes.data)
    for p in range(3):
        for n in range(N):
            for k in range(K):
                assert planes[p * N * K + n * K + k] == pieces[n * K + k, p]
