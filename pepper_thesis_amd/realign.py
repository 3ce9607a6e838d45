"""The polisher's read realignment on the GPU (pv_polish_realign[_dev], csrc/polish_realign.hip).

Replaces AlignmentSummarizer.reads_to_reference_realignment (pepper/modules/python/AlignmentSummarizer.py:159-177), which the
reference's polisher runs on every region between read sampling and the image builder: each read is aligned to the draft
window [region start, region end + 20) with its striped Smith-Waterman, and the realigned reads feed SummaryGenerator.
The result, with the input's bases, quals, flags and mapq, is a RegionBatch that the polisher's builder takes as it is
(`realigned_batch`); dropped reads stay in place with no cigar words, which the builder walks as nothing.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _ffi
from .batch import RegionBatch

SAFE_BASES = 20   # AlingerOptions.ALIGNMENT_SAFE_BASES (pepper/modules/python/Options.py:25)
UNCHANGED, REALIGNED, DROPPED = 0, 1, 2


@dataclass
class RealignResult:
    read_pos: np.ndarray    # [n_reads] int64
    cigar_off: np.ndarray   # [n_reads + 1] int64
    cigar: np.ndarray       # uint32, BAM packing
    score: np.ndarray       # [n_reads] int32
    ends: np.ndarray        # [n_reads, 4] int32: ref_begin, ref_end, query_begin, query_end (ref_* from the read's pos)
    state: np.ndarray       # [n_reads] uint8: 0 unchanged, 1 realigned, 2 dropped
    n_realigned: int
    n_dropped: int
    band: np.ndarray = None  # [n_reads] int32: banded_sw's final band width (realigned reads)


def pack_windows(windows: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """[window of each region] -> (win_off int64 [n+1], win uint8)"""
    off = np.zeros(len(windows) + 1, np.int64)
    off[1:] = np.cumsum([len(w) for w in windows])
    win = np.frombuffer(b"".join(windows), np.uint8).copy() if off[-1] else np.zeros(1, np.uint8)
    return off, win


def realign(ctx, batch: RegionBatch, win_off: np.ndarray, win: np.ndarray, cigar_capacity: int = None) -> RealignResult:
    """pv_polish_realign (host buffers). cigar_capacity None: sized from the batch and grown on PV_ERR_CAPACITY; an explicit
    one that is too small raises PepperHipError(PV_ERR_CAPACITY) with the words needed in its message."""
    n = batch.n_reads
    cin = batch.as_c()
    woff = np.ascontiguousarray(win_off, np.int64)
    wb = np.ascontiguousarray(win, np.uint8)
    cap = int(cigar_capacity) if cigar_capacity is not None else max(16, batch.n_cigar + 4 * n + batch.n_bases // 8)
    for _ in range(2):
        pos = np.zeros(max(n, 1), np.int64)
        coff = np.zeros(n + 1, np.int64)
        cig = np.zeros(max(cap, 1), np.uint32)
        score = np.zeros(max(n, 1), np.int32)
        ends = np.zeros((max(n, 1), 4), np.int32)
        state = np.zeros(max(n, 1), np.uint8)
        band = np.zeros(max(n, 1), np.int32)
        o = _ffi.pv_realign_out()
        o.cigar_capacity = cap
        o.read_pos, o.cigar_off, o.cigar = _ffi.ptr(pos), _ffi.ptr(coff), _ffi.ptr(cig)
        o.score, o.ends, o.state, o.band = _ffi.ptr(score), _ffi.ptr(ends), _ffi.ptr(state), _ffi.ptr(band)
        rc = ctx.lib.pv_polish_realign(ctx.handle, C.byref(cin), _ffi.ptr(woff), _ffi.ptr(wb), C.byref(o))
        if rc == _ffi.PV_ERR_CAPACITY and cigar_capacity is None:
            cap = int(o.n_cigar)
            continue
        _ffi.check(rc)
        return RealignResult(pos[:n], coff, cig[:int(o.n_cigar)].copy(), score[:n], ends[:n], state[:n], int(o.n_realigned),
                             int(o.n_dropped), band[:n])
    raise _ffi.PepperHipError(_ffi.PV_ERR_CAPACITY, "realign: capacity retry failed")


def realigned_batch(batch: RegionBatch, res: RealignResult) -> RegionBatch:
    """the builder's input after realignment: new positions and cigars, everything else the input's"""
    return RegionBatch(batch.n_regions, batch.ref_start, batch.ref_end, batch.cand_start, batch.cand_end, batch.ref_off,
                       batch.ref, batch.read_off, np.ascontiguousarray(res.read_pos, np.int64), batch.read_flags,
                       batch.read_mapq, batch.base_off, batch.bases, batch.quals, np.ascontiguousarray(res.cigar_off, np.int64),
                       np.ascontiguousarray(res.cigar, np.uint32), list(batch.contigs), batch.read_hp)


class DeviceRealignOut:
    """Caller-owned pv_realign_out arrays in HBM for n_reads reads and cigar_capacity words."""

    def __init__(self, n_reads: int, cigar_capacity: int, device="cuda:0"):
        import torch
        self.n_reads, self.capacity = int(n_reads), int(cigar_capacity)
        n = max(self.n_reads, 1)
        self.read_pos = torch.zeros(n, dtype=torch.int64, device=device)
        self.cigar_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
        self.cigar = torch.zeros(max(self.capacity, 1), dtype=torch.int32, device=device)   # uint32 bits
        self.score = torch.zeros(n, dtype=torch.int32, device=device)
        self.ends = torch.zeros((n, 4), dtype=torch.int32, device=device)
        self.state = torch.zeros(n, dtype=torch.uint8, device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        c = _ffi.pv_realign_out()
        c.cigar_capacity = self.capacity
        c.read_pos, c.cigar_off, c.cigar = self.read_pos.data_ptr(), self.cigar_off.data_ptr(), self.cigar.data_ptr()
        c.score, c.ends, c.state = self.score.data_ptr(), self.ends.data_ptr(), self.state.data_ptr()
        c.band = None
        self.c = c


def device_windows(win_off: np.ndarray, win: np.ndarray, device="cuda:0"):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(win_off, np.int64)).to(device),
            torch.from_numpy(np.ascontiguousarray(win, np.uint8) if len(win) else np.zeros(1, np.uint8)).to(device))
