"""TEST INFRASTRUCTURE ONLY — ctypes access to the CPU oracle (oracle/liboracle.so, built from
region_summary_oracle.c) and, where it has been built in this container, the reference's own image
builders and polisher read loop (oracle/_ref/libref_*.so, built by oracle/Makefile from the sources under
/root/reference). Neither is ever used by the product path."""
import ctypes as C
import os
import subprocess

from pepper_thesis_amd import _ffi
from pepper_thesis_amd.batch import Params, RegionBatch, run_flat_summarizer

_HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_SO = os.path.join(_HERE, "liboracle.so")
REF_SO = os.path.join(_HERE, "_ref", "libref_region_summary.so")
REF_HP_SO = os.path.join(_HERE, "_ref", "libref_region_summary_hp.so")
REF_POLISH_SO = os.path.join(_HERE, "_ref", "libref_polish.so")

_SIG = [C.POINTER(_ffi.pv_batch_in), C.POINTER(_ffi.pv_params), C.POINTER(_ffi.pv_batch_out)]
_libs = {}


_made = False


def build(force=False):
    """(re)build liboracle.so and, if /root/reference exists, oracle/_ref (make decides what is stale)."""
    global _made
    if force or not _made:
        subprocess.check_call(["make", "-s", "-C", _HERE] + (["-B"] if force else []))
        _made = True


_SIG_HP = [_SIG[0], C.POINTER(C.c_int32), _SIG[1], _SIG[2]]


def _load(path, sym, sig=None):
    key = (path, sym)
    if key not in _libs:
        lib = C.CDLL(path)
        fn = getattr(lib, sym)
        fn.restype = C.c_int
        fn.argtypes = sig or _SIG
        _libs[key] = fn
    return _libs[key]


def have_reference():
    return os.path.exists(REF_SO)


def summarize(batch: RegionBatch, params: Params, want_i32=False):
    """CPU restatement (oracle) of generate_summary over a batch."""
    build()
    rc, out = run_flat_summarizer(_load(ORACLE_SO, "oracle_summarize_regions"), batch, params, want_i32)
    if rc:
        raise RuntimeError("oracle_summarize_regions failed: %d" % rc)
    return out


def reference_summarize(batch: RegionBatch, params: Params, want_i32=False):
    """The reference's own region_summary.cpp (only where oracle/_ref was built)."""
    rc, out = run_flat_summarizer(_load(REF_SO, "ref_summarize_regions"), batch, params, want_i32)
    if rc:
        raise RuntimeError("ref_summarize_regions failed: %d" % rc)
    return out


def have_reference_hp():
    return os.path.exists(REF_HP_SO)


def summarize_hp(batch: RegionBatch, params: Params, want_i32=False):
    """CPU restatement of RegionalSummaryGeneratorHP.generate_summary (region_summary_hp_oracle.c)."""
    build()
    rc, out = run_flat_summarizer(_load(ORACLE_SO, "oracle_summarize_regions_hp", _SIG_HP), batch, params, want_i32, hp=True)
    if rc:
        raise RuntimeError("oracle_summarize_regions_hp failed: %d" % rc)
    return out


def reference_summarize_hp(batch: RegionBatch, params: Params, want_i32=False):
    """The reference's own region_summary_hp.cpp (only where oracle/_ref was built)."""
    rc, out = run_flat_summarizer(_load(REF_HP_SO, "ref_summarize_regions_hp", _SIG_HP), batch, params, want_i32, hp=True)
    if rc:
        raise RuntimeError("ref_summarize_regions_hp failed: %d" % rc)
    return out


def polish_summarize(batch: RegionBatch, seq_length=1000, seq_overlap=50, want_flat=True):
    """CPU restatement of the polisher's SummaryGenerator.generate_summary + chunk_images (pinned by
    tests/golden/polish_golden.npz and, where oracle/_ref was built, by reference_polish_flat)."""
    from pepper_thesis_amd.polish_summary import run_polish_summarizer
    build()
    key = (ORACLE_SO, "oracle_polish_summarize_regions")
    if key not in _libs:
        fn = getattr(C.CDLL(ORACLE_SO), key[1])
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(_ffi.pv_batch_in), C.c_int, C.c_int, C.POINTER(_ffi.pv_polish_out)]
        _libs[key] = fn
    rc, out = run_polish_summarizer(_libs[key], batch, seq_length, seq_overlap, want_flat)
    if rc:
        raise RuntimeError("oracle_polish_summarize_regions failed: %d" % rc)
    return out


def have_reference_polish():
    return os.path.exists(REF_POLISH_SO)


def _ref_polish_fn(sym, argtypes):
    key = (REF_POLISH_SO, sym)
    if key not in _libs:
        fn = getattr(C.CDLL(REF_POLISH_SO), sym)
        fn.restype = C.c_int64
        fn.argtypes = argtypes
        _libs[key] = fn
    return _libs[key]


def reference_polish_flat(batch: RegionBatch):
    """The reference's own SummaryGenerator(ref, contig, start, end).generate_summary(reads, start, end), region by region
    (only where oracle/_ref was built). -> (image uint8 [n, 10], position int64 [n], index int32 [n], row_off [n_regions+1])"""
    import numpy as np
    P = C.c_void_p
    fn = _ref_polish_fn("ref_polish_flat", [C.POINTER(_ffi.pv_batch_in), P, P, P, P, C.c_int64])
    cin = batch.as_c()
    cap = int((batch.ref_end - batch.ref_start + 1).sum()) + 1024 if batch.n_regions else 1
    for _ in range(2):
        img = np.zeros((cap, 10), np.uint8)
        pos = np.zeros(cap, np.int64)
        idx = np.zeros(cap, np.int32)
        off = np.zeros(batch.n_regions + 1, np.int64)
        n = fn(C.byref(cin), img.ctypes.data, pos.ctypes.data, idx.ctypes.data, off.ctypes.data, cap)
        if n <= cap:
            return img[:n], pos[:n], idx[:n], off
        cap = n
    raise RuntimeError("ref_polish_flat: capacity")


REF_KEPT, REF_DROPPED, REF_UNDEFINED = 1, 2, 3


def reference_polish_realign(batch: RegionBatch, win_off, win):
    """The reference's own ReadAligner(start, end + 20, window).align_reads_to_reference(reads), region by region (only
    where oracle/_ref was built). -> (state uint8 [n_reads]: REF_KEPT / REF_DROPPED / REF_UNDEFINED (not handed to the
    reference, see ref_driver_polish.cpp), pos int64, pos_end int64, cigar_off int64 [n_reads+1], cigar uint32)"""
    import numpy as np
    P = C.c_void_p
    fn = _ref_polish_fn("ref_polish_realign", [C.POINTER(_ffi.pv_batch_in), P, P, P, P, P, P, P, C.c_int64])
    cin = batch.as_c()
    woff = np.ascontiguousarray(win_off, np.int64)
    wb = np.ascontiguousarray(win, np.uint8)
    n = batch.n_reads
    cap = batch.n_cigar + 4 * n + batch.n_bases // 4 + 16
    for _ in range(2):
        state = np.zeros(max(n, 1), np.uint8)
        pos = np.zeros(max(n, 1), np.int64)
        end = np.zeros(max(n, 1), np.int64)
        coff = np.zeros(n + 1, np.int64)
        cig = np.zeros(cap, np.uint32)
        w = fn(C.byref(cin), woff.ctypes.data, wb.ctypes.data, state.ctypes.data, pos.ctypes.data, end.ctypes.data,
               coff.ctypes.data, cig.ctypes.data, cap)
        if w < 0:
            raise RuntimeError("ref_polish_realign: outputs do not match inputs")
        if w <= cap:
            return state[:n], pos[:n], end[:n], coff, cig[:w]
        cap = w
    raise RuntimeError("ref_polish_realign: capacity")
