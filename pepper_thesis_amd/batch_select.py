"""Selection of a flat batch by haplotype, host-buffer form (pv_batch_select_hp): the reads whose HP tag is 0 or `haplotype`,
in input order, offsets rebuilt; the region arrays are the input's. The rule is stated in include/pepper_hip.h. `polish -hp`
selects on the device (Context.batch_select_hp_dev); this form serves its host fallback and the tests.
"""
import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from .batch import RegionBatch


def tag_counts(read_hp, n_reads: int) -> Tuple[int, int, int, int, int]:
    """(reads, untagged, HP1, HP2, other values) of a batch's tags: a numpy array, a torch tensor or None (no read tagged)"""
    n = int(n_reads)
    if read_hp is None or n == 0:
        return n, n, 0, 0, 0
    hp = read_hp[:n]
    c = [int((hp == v).sum()) for v in (0, 1, 2)]
    return n, c[0], c[1], c[2], n - sum(c)


def select_hp(ctx, batch: RegionBatch, haplotype: int, capacities: Optional[Tuple[int, int, int]] = None):
    """-> (RegionBatch of the kept reads, src_read int64 [kept]). capacities (reads, bases, cigar words) default to the
    input's totals, which cannot run short; a short one raises PepperHipError(PV_ERR_CAPACITY)."""
    cr, cb, cc = (batch.n_reads, batch.n_bases, batch.n_cigar) if capacities is None else (int(v) for v in capacities)
    G = batch.n_regions
    a = dict(read_off=np.zeros(G + 1, np.int64), read_pos=np.zeros(cr, np.int64), read_flags=np.zeros(cr, np.uint8),
             read_mapq=np.zeros(cr, np.uint8), base_off=np.zeros(cr + 1, np.int64), bases=np.zeros(cb, np.uint8),
             quals=np.zeros(cb, np.uint8), cigar_off=np.zeros(cr + 1, np.int64), cigar=np.zeros(cc, np.uint32),
             read_hp=np.zeros(cr, np.int32), src_read=np.zeros(cr, np.int64))
    o = _ffi.pv_select_out()
    o.read_capacity, o.base_capacity, o.cigar_capacity = cr, cb, cc
    for f, v in a.items():
        setattr(o, f, v.ctypes.data)
    cin = batch.as_c()
    hp = None if batch.read_hp is None else np.ascontiguousarray(batch.read_hp, np.int32)
    _ffi.check(ctx.lib.pv_batch_select_hp(ctx.handle, C.byref(cin), None if hp is None else hp.ctypes.data, int(haplotype),
                                          C.byref(o)))
    n, nb, nc = int(o.n_reads), int(o.n_bases), int(o.n_cigar)
    out = RegionBatch(G, batch.ref_start, batch.ref_end, batch.cand_start, batch.cand_end, batch.ref_off, batch.ref,
                      a["read_off"], a["read_pos"][:n], a["read_flags"][:n], a["read_mapq"][:n], a["base_off"][:n + 1],
                      a["bases"][:nb], a["quals"][:nb], a["cigar_off"][:n + 1], a["cigar"][:nc], list(batch.contigs),
                      None if batch.read_hp is None else a["read_hp"][:n])
    return out, a["src_read"][:n]
