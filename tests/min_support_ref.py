"""Host checker of the polisher's minimum support (include/pepper_hip.h, pv_polish_filter_low_support).

It looks at no kernel output. It stands on the checkers of its neighbours: the owned columns and their records come from
tests/edits_ref.py (as in tests/min_qual_ref.py), "run" has the one definition of min_qual_ref.runs_of, and the support of a
record is alt_fwd + alt_rev of counts_ref.evidence_of on the counts row and the depth of the chunk row that owns it. A run
whose weakest column is below the minimum, and which stands over no draft byte that cannot be spelled, is written back as
the draft on the rows that own its columns.
"""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

import counts_ref as cr
import edits_ref as er
import min_qual_ref as mq


class Run(NamedTuple):
    region: int
    records: tuple      # edits_ref.primitive_edits tuples (position, index, kind, draft byte, base, qual)
    rows: tuple         # (chunk, row) that owns each record
    supports: tuple     # the support of each record
    minimum: int        # the weakest column's
    pinned: bool


def support_of(kind: int, draft: int, base: int, c, depth: int) -> int:
    """reads that spell the edit: alt_fwd + alt_rev of its evidence record (each a uint16 count; the sum is not clamped)"""
    _, _, fwd, rev = cr.evidence_of(kind, draft, base, c, depth)
    return fwd + rev


def region_runs(labels, counts, depth, position, index, region, chunk_id, ref_start, ref_off, ref) -> List[Run]:
    """every run of every region, regions ascending; counts [n, L, 10] and depth [n, L] as the builder leaves them"""
    labels, counts, depth = np.asarray(labels), np.asarray(counts), np.asarray(depth)
    n, L = labels.shape
    spans = [(int(s), int(s)) for s in ref_start]                 # (only the start is looked at)
    rowid = np.arange(n * L, dtype=np.int64).reshape(n, L)
    preds = er.region_dicts(position, index, region, chunk_id, labels, spans)
    owners = er.region_dicts(position, index, region, chunk_id, rowid, spans)
    draft_all = np.asarray(ref, np.uint8).tobytes()
    out = []
    for g, (pred, own) in enumerate(zip(preds, owners)):
        draft = draft_all[int(ref_off[g]):int(ref_off[g + 1])]
        for recs in mq.runs_of(er.primitive_edits(pred, draft, int(ref_start[g]))):
            rows = tuple(divmod(int(own[(r[0], r[1])][0]), L) for r in recs)
            sup = tuple(support_of(int(r[2]), int(r[3]), int(r[4]), counts[k, j], int(depth[k, j])) for r, (k, j) in zip(recs, rows))
            pinned = any(r[1] == 0 and er.upper(r[3]) not in er.BASES for r in recs)
            out.append(Run(g, tuple(recs), rows, sup, min(sup), pinned))
    return out


def filter_low_support(labels, row_qual: Optional[np.ndarray], counts, depth, position, index, region, chunk_id, ref_start, ref_off,
                       ref, min_support: int, runs=None) -> Tuple[np.ndarray, Optional[np.ndarray], int, int, List[Run]]:
    """-> (labels out, row qualities out or None, rows reverted, rows of pinned runs below min_support, the reverted runs).
    The inputs are not altered. runs: region_runs of the same arguments, when the caller has them already."""
    lab = np.array(labels, np.uint8)
    rq = None if row_qual is None else np.array(row_qual, np.uint8)
    reverted, pinned_rows, gone = 0, 0, []
    if runs is None:
        runs = region_runs(labels, counts, depth, position, index, region, chunk_id, ref_start, ref_off, ref)
    for run in runs:
        if run.minimum >= min_support:
            continue
        if run.pinned:
            pinned_rows += len(run.records)
            continue
        gone.append(run)
        for (pos, indx, kind, d, base, q), (k, j) in zip(run.records, run.rows):
            lab[k, j] = 1 + er.BASES.index(er.upper(d)) if indx == 0 else 0
            if rq is not None:
                rq[k, j] = 0
            reverted += 1
    return lab, rq, reverted, pinned_rows, gone
