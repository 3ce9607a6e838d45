"""Host checker of the polisher's minimum quality (include/pepper_hip.h, pv_polish_filter_low_qual).

It looks at no kernel output. It works on the checkers it stands on: the stitch checker's dictionary (tests/stitch_ref.py via
tests/edits_ref.py: one dict keyed by (position, index) per region, a region's chunk ids walked in STRING order so that the
later id overwrites) gives the owned columns, once with the labels and row qualities and once with the row numbers, so that
every key knows the chunk row that owns it; edits_ref.primitive_edits gives the records in (position, index) order; the records
are cut into runs where the position jumps by more than one; and a run whose lowest quality is below the threshold, and which
stands over no draft byte that cannot be spelled, is written back as the draft on the rows that own its columns.
"""
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

import edits_ref as er


class Run(NamedTuple):
    region: int
    records: tuple      # edits_ref.primitive_edits tuples (position, index, kind, draft byte, base, qual)
    rows: tuple         # (chunk, row) that owns each record
    minimum: int
    pinned: bool


def runs_of(records: Sequence[tuple]) -> List[List[tuple]]:
    """records in (position, index) order -> maximal stretches whose consecutive positions differ by at most one"""
    out: List[List[tuple]] = []
    for r in records:
        if out and r[0] - out[-1][-1][0] <= 1:
            out[-1].append(r)
        else:
            out.append([r])
    return out


def region_runs(labels, row_qual, position, index, region, chunk_id, ref_start, ref_off, ref) -> List[Run]:
    """every run of every region, regions ascending"""
    labels, row_qual = np.asarray(labels), np.asarray(row_qual)
    n, L = labels.shape
    spans = [(int(s), int(s)) for s in ref_start]                 # (only the start is looked at)
    rowid = np.arange(n * L, dtype=np.int64).reshape(n, L)
    preds = er.region_dicts(position, index, region, chunk_id, labels, spans, row_qual)
    owners = er.region_dicts(position, index, region, chunk_id, rowid, spans)
    draft_all = np.asarray(ref, np.uint8).tobytes()
    out = []
    for g, (pred, own) in enumerate(zip(preds, owners)):
        draft = draft_all[int(ref_off[g]):int(ref_off[g + 1])]
        assert sorted(pred) == sorted(own)
        for recs in runs_of(er.primitive_edits(pred, draft, int(ref_start[g]))):
            rows = tuple(divmod(int(own[(r[0], r[1])][0]), L) for r in recs)
            pinned = any(r[1] == 0 and er.upper(r[3]) not in er.BASES for r in recs)
            out.append(Run(g, tuple(recs), rows, min(r[5] for r in recs), pinned))
    return out


def filter_low_qual(labels, row_qual, position, index, region, chunk_id, ref_start, ref_off, ref, min_qual: int, runs=None
                    ) -> Tuple[np.ndarray, np.ndarray, int, int, List[Run]]:
    """-> (labels out, row qualities out, rows reverted, rows of pinned runs below min_qual, the reverted runs). The inputs
    are not altered. runs: region_runs of the same arguments, when the caller has them already."""
    lab, rq = np.array(labels, np.uint8), np.array(row_qual, np.uint8)
    reverted, pinned_rows, gone = 0, 0, []
    if runs is None:
        runs = region_runs(labels, row_qual, position, index, region, chunk_id, ref_start, ref_off, ref)
    for run in runs:
        if run.minimum >= min_qual:
            continue
        if run.pinned:
            pinned_rows += len(run.records)
            continue
        gone.append(run)
        for (pos, indx, kind, d, base, q), (k, j) in zip(run.records, run.rows):
            lab[k, j] = 1 + er.BASES.index(er.upper(d)) if indx == 0 else 0
            rq[k, j] = 0
            reverted += 1
    return lab, rq, reverted, pinned_rows, gone


def owned_mask(position, index, region, chunk_id, ref_start, shape) -> np.ndarray:
    """bool [n, L]: the rows that own their (position, index)"""
    n, L = shape
    spans = [(int(s), int(s)) for s in ref_start]
    rowid = np.arange(n * L, dtype=np.int64).reshape(n, L)
    m = np.zeros(n * L, bool)
    for own in er.region_dicts(position, index, region, chunk_id, rowid, spans):
        m[[int(v[0]) for v in own.values()]] = True
    return m.reshape(n, L)
