"""Host checker of the polisher's depth plane and minimum-depth mask (include/pepper_hip.h: pv_polish_out.depth,
pv_polish_mask_low_depth). Plain numpy / Python; it looks at no kernel output.

Depth. The builder counts a read at a draft position when an M / = / X operation puts a base there or a D / N / P operation
covers it, inside the region; reads of mapping quality 0 are not counted at all (as in the images), and an operation that
begins behind the region's end ends the read. The depth of an insert row is that of its anchor position, of a padding row 0.

Mask. A row below min_depth that is no padding takes the label that spells the upper-cased draft byte under it (an insert
row: 0) and quality 0; a draft byte other than ACGT cannot be spelled: the row keeps what it had and counts as unmaskable.
"""
from typing import Optional, Tuple

import numpy as np

M_OPS, D_OPS = (0, 7, 8), (2, 3, 6)     # BAM CIGAR codes: M = X  /  D N P
DEPTH_MAX = 65535


def region_depth(batch, g: int) -> np.ndarray:
    """int64 [ref_end - ref_start + 1]: reads per draft position of region g of a flat batch (RegionBatch), from its CIGARs"""
    start, end = int(batch.ref_start[g]), int(batch.ref_end[g])
    # all operations of the region's reads at once (a Python loop over them takes seconds on a read of 68 000 operations)
    r0, r1 = int(batch.read_off[g]), int(batch.read_off[g + 1])
    first = np.asarray(batch.cigar_off[r0:r1 + 1], np.int64)          # of every read: its first operation
    words = np.asarray(batch.cigar[int(first[0]):int(first[-1])], np.int64)
    step = np.zeros(end - start + 2, np.int64)     # +1 where an operation enters the region, -1 behind its last position in it
    if len(words):
        op, ln = words & 0xF, words >> 4
        read = np.repeat(np.arange(r1 - r0), np.diff(first))         # of every operation: its read, counted from r0
        counted = np.isin(op, M_OPS + D_OPS)
        moves = np.where(counted, ln, 0)
        before = np.cumsum(moves) - moves                            # positions consumed before the operation, region-wide ...
        before -= before[np.minimum(first[:-1] - first[0], len(words) - 1)][read]     # ... and within its read
        begin = np.asarray(batch.read_pos[r0:r1], np.int64)[read] + before
        # an operation that begins behind the region's end ends the read (positions never decrease along a read)
        counted &= (begin <= end) & (np.asarray(batch.read_mapq[r0:r1])[read] != 0)
        a, b = np.maximum(begin[counted], start), np.minimum(begin[counted] + ln[counted] - 1, end)
        inside = a <= b
        np.add.at(step, a[inside] - start, 1)
        np.add.at(step, b[inside] - start + 1, -1)
    return np.minimum(np.cumsum(step)[:-1], DEPTH_MAX)


def row_depth(batch, position, index, region) -> np.ndarray:
    """uint16 [n_chunks, L]: the depth of every chunk row (position, index [n_chunks, L], region [n_chunks])"""
    position = np.asarray(position)
    out = np.zeros(position.shape, np.uint16)
    per = {}
    for k in range(position.shape[0]):
        g = int(region[k])
        if g not in per:
            per[g] = region_depth(batch, g)
        real = position[k] >= 0
        out[k, real] = per[g][position[k, real] - int(batch.ref_start[g])]
    return out


def mask(labels, row_qual: Optional[np.ndarray], depth, position, index, region, ref_start, ref_off, ref,
         min_depth: int) -> Tuple[np.ndarray, Optional[np.ndarray], int, int]:
    """the mask rule, row by row -> (labels, row_qual or None, masked rows, unmaskable rows); the inputs are left alone"""
    lab = np.array(labels, np.uint8)
    rq = None if row_qual is None else np.array(row_qual, np.uint8)
    masked = unmaskable = 0
    n, L = lab.shape
    for k in range(n):
        g = int(region[k])
        for j in np.flatnonzero((np.asarray(depth[k]).astype(np.int64) < min_depth) & (np.asarray(position[k]) >= 0)).tolist():
            if int(index[k, j]) > 0:
                new = 0
            else:
                u = chr(int(ref[int(ref_off[g]) + int(position[k, j]) - int(ref_start[g])])).upper()
                if u not in "ACGT":
                    unmaskable += 1
                    continue
                new = 1 + "ACGT".index(u)
            lab[k, j] = new
            if rq is not None:
                rq[k, j] = 0
            masked += 1
    return lab, rq, masked, unmaskable
