"""The library's kernel-form plan (pepper_thesis_amd/csrc/rnn_plan.hpp, the header the launchers consume) against the Python
restatement tests/rnn_forms.py, field for field, without a GPU: every P1 launch size 1 .. 16384, the chunks of every call size
1 .. 17000, every P2 size 1 .. 14100; 256 and 128 CUs; the default options and each forcing option on its own.
The header is compiled alone (tests/rnn_plan_shim.cpp, system C++ compiler) and called through ctypes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rnn_forms as rf

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, "rnn_plan_shim.cpp")] + [os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc", h)
                                                      for h in ("rnn_plan.hpp", "pv_opts.hpp")]
DTYPES = {rf.F32: 0, rf.BF16X3: 1}   # PV_DTYPE_F32, PV_DTYPE_BF16_INPUT_GEMM (include/pepper_hip.h)
NUM_CUS = (256, 128)
OPTIONS = [{}] + [{k: v} for k, vs in (("lstm_split", (0,)), ("lstm_rows", (16, 32)), ("tail_rows", (16, 32)),
                                       ("head_splits", (1, 3, 11, 33)), ("shared_device", (1,)), ("gru_rows", (16, 32)),
                                       ("gru_split", (0,)), ("gru_usplit", (0,)), ("p1_bf16_min_batch", (0,)),
                                       ("p1_f32x6_min_batch", (1 << 24, 1))) for v in vs]   # (1: every split-K factor of the split-6 chain)
P1_MAX, CALL_MAX, P2_MAX = 16384, 17000, 14100
# the header's enums, in their order
CHAINS = ("f32", "x6", "bf16x3")
LSTMS = (None, "split4", "split2", "rows16", "rows32")
TAILS = ("k_head_tail", "k_tail_bf16")
KINDS = ("us", "dsplit", "wg", "gru16", "rec")


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_rnn_plan_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    i64p, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int)
    lib.shim_option_defaults.argtypes, lib.shim_option_defaults.restype = [ip], C.c_int
    lib.shim_plan_p1.argtypes, lib.shim_plan_p1.restype = [C.c_int, C.c_int64, C.c_int64, C.c_int, ip, i64p], None
    lib.shim_p1_chunk.argtypes, lib.shim_p1_chunk.restype = [C.c_int, C.c_int64, C.c_int64, ip, i64p], None
    lib.shim_plan_p2.argtypes, lib.shim_plan_p2.restype = [C.c_int, C.c_int64, C.c_int64, C.c_int, ip, i64p], None
    return lib


def _opt_vec(options):
    o = dict(rf.DEFAULTS, **options)
    return (C.c_int * len(rf.OPTION_NAMES))(*[o[k] for k in rf.OPTION_NAMES])


def _rows(fn, n, width, *args):
    out = np.zeros((n, width), np.int64)
    fn(*args, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out


def test_header_compiles_without_hip(tmp_path):
    """a translation unit of rnn_plan.hpp alone goes through the host compiler: no HIP header behind it"""
    src = tmp_path / "only_plan.cpp"
    src.write_text('#include "%s"\n' % os.path.abspath(_SRCS[1]))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)])


def test_option_defaults_are_the_librarys(shim):
    v = (C.c_int * 10)()
    assert shim.shim_option_defaults(v) == len(rf.OPTION_NAMES)
    assert dict(zip(rf.OPTION_NAMES, v)) == rf.DEFAULTS


@pytest.mark.parametrize("num_cu", NUM_CUS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_p1_launch_plan_equals_the_restatement(shim, dtype, num_cu):
    for options in OPTIONS:
        got = _rows(shim.shim_plan_p1, P1_MAX, 9, DTYPES[dtype], 1, P1_MAX, num_cu, _opt_vec(options))
        for B in range(1, P1_MAX + 1):
            f = rf.p1_launch_form(dtype, B, num_cu, options)
            chain, lstm, rows, mt, Bp, splits, head_map, tail, tail_rows = (int(x) for x in got[B - 1])
            assert (CHAINS[chain], LSTMS[lstm], rows, mt or None, splits, TAILS[tail], tail_rows) == \
                (f.chain, f.lstm, f.rows, f.mt, f.splits, f.tail, f.tail_rows), (dtype, B, num_cu, options)
            assert head_map == 1 and Bp % rows == 0 and 0 <= Bp - B < max(rows, rf.P1_ROWS), (dtype, B, num_cu, options, Bp)
            if f.chain != "f32":   # the padded batch, through the bytes of the decoder input projections
                assert Bp * rf.P1_T * 2048 * 4 == f.g_bytes, (dtype, B, num_cu, options)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_p1_chunk_rule_equals_the_restatement(shim, dtype):
    for options in OPTIONS:
        got = _rows(shim.shim_p1_chunk, CALL_MAX, 1, DTYPES[dtype], 1, CALL_MAX, _opt_vec(options))[:, 0]
        for B in range(1, CALL_MAX + 1):
            chunk = int(got[B - 1])
            assert [(b0, min(chunk, B - b0)) for b0 in range(0, B, chunk)] == rf.p1_chunks(dtype, B, options), (dtype, B, options)


@pytest.mark.parametrize("num_cu", NUM_CUS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_p2_plan_equals_the_restatement(shim, dtype, num_cu):
    for options in OPTIONS:
        got = _rows(shim.shim_plan_p2, P2_MAX, 5, DTYPES[dtype], 1, P2_MAX, num_cu, _opt_vec(options))
        for B in range(1, P2_MAX + 1):
            f = rf.p2_call(dtype, B, num_cu, options)
            kind, rows, mt, fold, Bp = (int(x) for x in got[B - 1])
            dense = None if dtype == rf.F32 else ("combine" if fold else "dense")
            assert (KINDS[kind], rows, mt or None, dense) == (f.kind, f.rows, f.mt, f.dense), (dtype, B, num_cu, options)
            assert Bp % rows == 0 and 0 <= Bp - B < rows, (dtype, B, num_cu, options, Bp)
            if dtype == rf.BF16X3:
                assert rf.P2_WIN * Bp * 6 * 128 * 4 == f.g_bytes, (dtype, B, num_cu, options)
