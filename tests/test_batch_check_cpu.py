"""The host-side validation of a flat batch (pepper_thesis_amd/csrc/batch_check.hpp: what pv_upload_batch, pv_upload_batches and
pv_polish_summarize_regions run before they upload) without a GPU: the four totals of a well-formed batch, every malformed
batch refused with the check that failed named, the degenerate batches that are accepted.
The header is compiled alone (tests/batch_check_shim.cpp, system C++ compiler) and called through ctypes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from pepper_thesis_amd import _ffi

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRCS = [os.path.join(_HERE, "batch_check_shim.cpp"), os.path.join(_HERE, "..", "pepper_thesis_amd", "csrc", "batch_check.hpp"),
         os.path.join(_HERE, "..", "include", "pepper_hip.h")]
# pv_batch_fault, in the header's order
OK, REGION_COUNT, OFFSET_START, REGION_EMPTY, REF_SHORT, READ_OFF, BASE_OFF, CIGAR_OFF = range(8)
ALL_ARRAYS = ["in." + f for f in ("ref_start", "ref_end", "cand_start", "cand_end", "ref_off", "ref", "read_off", "read_pos",
                                  "read_flags", "read_mapq", "base_off", "bases", "quals", "cigar_off", "cigar")]


@pytest.fixture(scope="module")
def shim():
    h = hashlib.sha1()
    for p in _SRCS:
        with open(p, "rb") as fh:
            h.update(fh.read())
    so = os.path.join(tempfile.gettempdir(), "pv_batch_check_shim_%d_%s.so" % (os.getuid(), h.hexdigest()[:12]))
    if not os.path.exists(so):
        tmp = so + ".%d" % os.getpid()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", tmp, _SRCS[0]])
        os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.shim_check_batch.argtypes = [C.POINTER(_ffi.pv_batch_in), C.c_uint, C.POINTER(C.c_int64)]
    lib.shim_check_batch.restype = C.c_char_p
    lib.shim_form.argtypes, lib.shim_form.restype = [C.c_int], C.c_uint
    lib.shim_arrays_read.argtypes, lib.shim_arrays_read.restype = [C.c_uint, C.c_char_p, C.c_int], C.c_int
    return lib


def arrays():
    """two regions (10 and 5 columns; the first with two reference bytes to spare), three reads (2 + 1)"""
    i64 = np.int64
    return dict(
        ref_start=np.array([100, 500], i64), ref_end=np.array([109, 504], i64),
        cand_start=np.array([100, 500], i64), cand_end=np.array([109, 504], i64),
        ref_off=np.array([0, 12, 17], i64), ref=np.full(17, ord("A"), np.uint8),
        read_off=np.array([0, 2, 3], i64), read_pos=np.array([100, 103, 500], i64),
        read_flags=np.zeros(3, np.uint8), read_mapq=np.full(3, 60, np.uint8),
        base_off=np.array([0, 4, 9, 12], i64), bases=np.full(12, ord("A"), np.uint8), quals=np.full(12, 30, np.uint8),
        cigar_off=np.array([0, 1, 3, 4], i64), cigar=np.array([4 << 4, 3 << 4, (2 << 4) | 2, 3 << 4], np.uint32))


TOTALS = (3, 12, 4, 17)   # reads, bases, CIGAR words, reference bytes


def check(shim, a, n_regions=2, polish=False, without=()):
    """-> (code, fault, index, totals, words) for the batch of the arrays `a`; arrays named in `without` are passed as null"""
    c = _ffi.pv_batch_in()
    c.n_regions = n_regions
    for f, v in a.items():
        setattr(c, f, None if f in without else _ffi.ptr(v))
    out = (C.c_int64 * 7)()
    what = shim.shim_check_batch(C.byref(c), shim.shim_form(1 if polish else 0), out)
    return int(out[0]), int(out[1]), int(out[2]), tuple(int(v) for v in out[3:7]), what.decode()


def test_header_compiles_without_hip(tmp_path):
    """a translation unit of batch_check.hpp alone goes through the host compiler: no HIP header behind it"""
    src = tmp_path / "only_check.cpp"
    src.write_text('#include "%s"\n' % os.path.abspath(_SRCS[1]))
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", str(src)])


@pytest.mark.parametrize("polish", [False, True])
def test_well_formed_batch_gives_its_totals(shim, polish):
    assert check(shim, arrays(), polish=polish) == (_ffi.PV_OK, OK, -1, TOTALS, "ok")


def _set(field, index, value):
    def edit(a):
        a[field][index] = value
    return edit


MALFORMED = {
    "read_off[0] != 0": (_set("read_off", 0, 1), OFFSET_START, -1),
    "ref_off[0] != 0": (_set("ref_off", 0, 1), OFFSET_START, -1),
    "R < 1": (_set("ref_end", 0, 99), REGION_EMPTY, 0),
    "reference one byte short": (_set("ref_off", 2, 16), REF_SHORT, 1),
    "read_off decreasing": (_set("read_off", 2, 1), READ_OFF, 1),
    "base_off decreasing": (_set("base_off", 2, 3), BASE_OFF, 1),
    "cigar_off decreasing": (_set("cigar_off", 2, 0), CIGAR_OFF, 1),
}


@pytest.mark.parametrize("polish", [False, True])
@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_batch_is_refused_with_the_check_named(shim, case, polish):
    edit, fault, index = MALFORMED[case]
    a = arrays()
    edit(a)
    code, got_fault, got_index, totals, what = check(shim, a, polish=polish)
    assert (code, got_fault, got_index) == (_ffi.PV_ERR_INVALID, fault, index), what
    assert totals == (0, 0, 0, 0) and what != "ok"


def test_negative_region_count_is_refused_before_any_array_is_read(shim):
    a = arrays()
    code, fault, index, totals, what = check(shim, a, n_regions=-1, without=tuple(a))
    assert (code, fault, index, totals) == (_ffi.PV_ERR_INVALID, REGION_COUNT, -1, (0, 0, 0, 0)) and "region count" in what


def test_batch_of_no_regions_is_accepted_without_reading_an_array(shim):
    a = arrays()
    assert check(shim, a, n_regions=0, without=tuple(a)) == (_ffi.PV_OK, OK, -1, (0, 0, 0, 0), "ok")


def test_region_of_no_reads_is_accepted(shim):
    a = arrays()
    a["read_off"][1] = 0   # all three reads belong to the second region
    assert check(shim, a) == (_ffi.PV_OK, OK, -1, TOTALS, "ok")
    a["read_off"][:] = 0   # no reads at all: base_off and cigar_off are not looked at
    assert check(shim, a, without=("base_off", "cigar_off")) == (_ffi.PV_OK, OK, -1, (0, 0, 0, 17), "ok")


def test_polisher_form_needs_neither_reference_bytes_nor_qualities(shim):
    assert check(shim, arrays(), polish=True, without=("ref", "quals", "cand_start", "cand_end")) == (_ffi.PV_OK, OK, -1, TOTALS, "ok")


def test_builder_form_without_qualities_is_not_caught_here(shim):
    """as before the checks became one function: only offsets and region bounds are validated, so a builder batch with
    bases but no qualities passes this level (pinned, not endorsed)"""
    assert check(shim, arrays(), without=("quals",)) == (_ffi.PV_OK, OK, -1, TOTALS, "ok")


def test_arrays_a_form_uploads(shim):
    def read(polish):
        buf = C.create_string_buffer(1024)
        n = shim.shim_arrays_read(shim.shim_form(polish), buf, len(buf))
        names = buf.value.decode().split("\n")
        assert n == len(names)
        return names
    assert read(0) == ALL_ARRAYS
    assert read(1) == [n for n in ALL_ARRAYS if n not in ("in.cand_start", "in.cand_end", "in.ref", "in.quals")]
