"""Host checker of the polisher's counts plane, of the evidence record of an edit and of the VCF composer's weakest-column
rule (include/pepper_hip.h: pv_polish_out.counts, pv_polish_evidence; polish_edits.compose_records). Plain numpy / Python; it
looks at no kernel output.

Counts. Ten per (position, index): A, C, G, T on reverse-strand reads (0-3) and on forward-strand reads (4-7), other or deleted
on reverse (8) and forward (9) reads. A read byte is upper-cased first; a byte that is not ACGT counts as other. An M / = / X
operation puts its bases on the positions it covers (index 0), a D / N / P operation a deleted column on each, an I operation
its bases on the insert rows 1, 2, ... of the position before it. Only positions inside the region count, an insert needs
its anchor inside; reads of mapping quality 0 are not counted at all, and an operation that begins behind the region's end
ends the read. S and I consume the read, H nothing.

Evidence. From the edit's own row: c its ten counts, depth its depth (an insert row carries its anchor's).
"""
from typing import Dict, List, Tuple

import numpy as np

M_OPS, D_OPS, I_OP, S_OP = (0, 7, 8), (2, 3, 6), 1, 4     # BAM CIGAR codes
COUNT_MAX = 65535
KIND_SUB, KIND_DEL, KIND_INS = 1, 2, 3


def _feature(base: np.ndarray, rev: np.ndarray) -> np.ndarray:
    """plane of every (read byte, strand)"""
    b = np.array(base, np.int64)
    b = np.where((b >= ord("a")) & (b <= ord("z")), b - 32, b)
    sym = np.full(b.shape, 4, np.int64)
    for k, ch in enumerate(b"ACGT"):
        sym[b == ch] = k
    rev = np.asarray(rev, bool)
    return np.where(sym < 4, np.where(rev, sym, 4 + sym), np.where(rev, 8, 9))


def _expand(n: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(item, i) for i in range(n[item]), items in order"""
    n = np.asarray(n, np.int64)
    item = np.repeat(np.arange(len(n)), n)
    first = np.cumsum(n) - n
    return item, np.arange(int(n.sum())) - first[item]


def region_tables(batch, g: int) -> Tuple[np.ndarray, Dict[Tuple[int, int], np.ndarray]]:
    """region g of a flat batch (RegionBatch) -> (int64 [ref_end - ref_start + 1, 10]: the counts of every position at index 0,
    {(position, index >= 1): int64 [10]}: those of every insert row some counted read reaches)"""
    start, end = int(batch.ref_start[g]), int(batch.ref_end[g])
    R = end - start + 1
    base = np.zeros((R, 10), np.int64)
    out: Dict[Tuple[int, int], np.ndarray] = {}
    r0, r1 = int(batch.read_off[g]), int(batch.read_off[g + 1])
    first = np.asarray(batch.cigar_off[r0:r1 + 1], np.int64)
    words = np.asarray(batch.cigar[int(first[0]):int(first[-1])], np.int64) if r1 > r0 else np.zeros(0, np.int64)
    if len(words):
        op, ln = words & 0xF, words >> 4
        read = np.repeat(np.arange(r1 - r0), np.diff(first))
        at_first = np.minimum(first[:-1] - first[0], len(words) - 1)

        def consumed_before(moves):
            c = np.cumsum(moves) - moves
            return c - c[at_first][read]
        begin = np.asarray(batch.read_pos[r0:r1], np.int64)[read] + consumed_before(np.where(np.isin(op, M_OPS + D_OPS), ln, 0))
        rd = consumed_before(np.where(np.isin(op, M_OPS + (I_OP, S_OP)), ln, 0))
        rd += np.asarray(batch.base_off[r0:r1], np.int64)[read]
        rev = (np.asarray(batch.read_flags[r0:r1])[read] & 1) != 0
        live = (begin <= end) & (np.asarray(batch.read_mapq[r0:r1])[read] != 0)
        bases = np.asarray(batch.bases)
        # bases under M / = / X
        m = np.flatnonzero(live & np.isin(op, M_OPS))
        item, i = _expand(ln[m])
        pos = begin[m][item] + i
        ok = (pos >= start) & (pos <= end)
        np.add.at(base, (pos[ok] - start, _feature(bases[(rd[m][item] + i)[ok]], rev[m][item][ok])), 1)
        # deleted columns under D / N / P
        d = np.flatnonzero(live & np.isin(op, D_OPS))
        lo, hi = np.maximum(begin[d], start), np.minimum(begin[d] + ln[d] - 1, end)
        item, i = _expand(np.maximum(hi - lo + 1, 0))
        np.add.at(base, (lo[item] + i - start, np.where(rev[d][item], 8, 9)), 1)
        # inserted bases, on the rows behind their anchor
        s = np.flatnonzero(live & (op == I_OP) & (begin - 1 >= start) & (begin - 1 <= end))
        item, i = _expand(ln[s])
        feat = _feature(bases[rd[s][item] + i], rev[s][item])
        for p, x, f in zip((begin[s][item] - 1).tolist(), (i + 1).tolist(), feat.tolist()):
            row = out.get((p, x))
            if row is None:
                row = out[(p, x)] = np.zeros(10, np.int64)
            row[f] += 1
    return base, out


def region_counts(batch, g: int) -> Dict[Tuple[int, int], np.ndarray]:
    """{(position, index): int64 [10]} of region g: every position of the region at index 0, and every insert row some counted
    read reaches"""
    base, out = region_tables(batch, g)
    start = int(batch.ref_start[g])
    for c in range(len(base)):
        out[(start + c, 0)] = base[c]
    return out


def row_counts(batch, position, index, region) -> np.ndarray:
    """uint16 [n_chunks, L, 10]: the counts of every chunk row (position, index [n_chunks, L], region [n_chunks]); padding rows
    (position < 0) all zero"""
    position, index = np.asarray(position), np.asarray(index)
    out = np.zeros(position.shape + (10,), np.uint16)
    per = {}
    for k in range(position.shape[0]):
        g = int(region[k])
        if g not in per:
            per[g] = region_tables(batch, g)
        base, ins = per[g]
        rows = (position[k] >= 0) & (index[k] == 0)
        out[k, rows] = np.minimum(base[position[k, rows] - int(batch.ref_start[g])], COUNT_MAX)
        for j in np.flatnonzero((position[k] >= 0) & (index[k] > 0)).tolist():
            out[k, j] = np.minimum(ins[(int(position[k, j]), int(index[k, j]))], COUNT_MAX)
    return out


def evidence_of(kind: int, draft: int, base: int, c, depth: int) -> Tuple[int, int, int, int]:
    """the evidence rule for one edit: (depth, ref, alt_fwd, alt_rev) from the ten counts c and the depth of its own row"""
    c = [int(v) for v in c]
    k = "ACGT".find

    def both(ch):
        return c[k(ch)] + c[4 + k(ch)] if ch in "ACGT" and len(ch) == 1 else 0
    u = chr(draft).upper() if kind != KIND_INS else ""
    if kind == KIND_DEL:
        rev, fwd, ref = c[8], c[9], both(u)
    elif kind == KIND_SUB:
        rev, fwd, ref = c[k(chr(base))], c[4 + k(chr(base))], both(u)
    else:
        assert kind == KIND_INS, kind
        rev, fwd, ref = c[k(chr(base))], c[4 + k(chr(base))], max(0, int(depth) - sum(c))
    return int(depth), min(ref, COUNT_MAX), fwd, rev


def evidence_rows(edits, rows: Dict[Tuple[int, int], Tuple[np.ndarray, int]]) -> List[Tuple[int, int, int, int]]:
    """the evidence of every edit record, row by row. A record is (position, index, kind, draft, base, ...): a tuple of
    tests/edits_ref.py's primitive_edits or an EDIT_DTYPE record. rows maps an edit's (position, index) to (its ten counts, its
    depth) - the OWNED column's where two chunks hold the row"""
    out = []
    for e in edits:
        c, depth = rows[(int(e[0]), int(e[1]))]
        out.append(evidence_of(int(e[2]), int(e[3]), int(e[4]), c, depth))
    return out


def weakest(block: List[Tuple[int, int, int, int]]) -> Tuple[int, int, int, int]:
    """the composer's rule: the evidence of a VCF record is that of its block's weakest column, the one with the lowest
    alt_fwd + alt_rev; the first such on a tie"""
    best = block[0]
    for ev in block[1:]:
        if ev[2] + ev[3] < best[2] + best[3]:
            best = ev
    return best


def blocks_of(edits) -> List[List[int]]:
    """record indices per VCF block: maximal runs of records (sorted by (position, index)) whose positions are equal or
    consecutive, which is how tests/edits_ref.py cuts its blocks"""
    out: List[List[int]] = []
    for i, e in enumerate(edits):
        if out and int(e[0]) - int(edits[out[-1][-1]][0]) <= 1:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def record_evidence(edits, evidence: List[Tuple[int, int, int, int]]) -> List[Tuple[int, int, int, int]]:
    """the evidence of every VCF block of a contig's records"""
    return [weakest([evidence[i] for i in blk]) for blk in blocks_of(edits)]


def info_text(ev: Tuple[int, int, int, int]) -> str:
    depth, ref, fwd, rev = ev
    return "DP=%d;AD=%d,%d;SAF=%d;SAR=%d" % (depth, ref, fwd + rev, fwd, rev)
