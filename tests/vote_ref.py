"""Host checker of the polisher's majority vote (include/pepper_hip.h, pv_polish_vote). Plain numpy / Python, row by row; it
looks at no kernel output."""
from typing import Optional, Tuple

import numpy as np

BASES = b"ACGT"
ONE, TWO = np.float32(1.0), np.float32(2.0)


def upper(b: int) -> int:
    return b - 32 if 97 <= b <= 122 else b


def draft_label(byte: int) -> Optional[int]:
    """1..4 for a draft byte whose upper-case form is A, C, G, T; None where no label spells it"""
    u = upper(int(byte))
    return 1 + BASES.index(bytes([u])) if bytes([u]) in (b"A", b"C", b"G", b"T") else None


def base_row(c, dl: Optional[int]) -> Tuple[int, list]:
    """a base row's ten counts and the label of its draft byte -> (label, n[0..4])"""
    c = [int(v) for v in c]
    n = [c[8] + c[9]] + [c[b - 1] + c[4 + b - 1] for b in (1, 2, 3, 4)]
    total = sum(n)
    if total == 0:
        return (dl if dl is not None else 0), n
    top = max(n[1:])
    if n[0] > top:                       # a deletion wins only strictly ahead of every base
        return 0, n
    if dl is not None and n[dl] == top:  # among equals the draft
        return dl, n
    return min(b for b in (1, 2, 3, 4) if n[b] == top), n


def insert_row(c, d: int) -> Tuple[int, list]:
    """an insert row's own ten counts and its anchor's depth -> (label, n[0..4])"""
    c = [int(v) for v in c]
    n = [max(0, int(d) - sum(c)) + c[8] + c[9]] + [c[b - 1] + c[4 + b - 1] for b in (1, 2, 3, 4)]
    top = max(n[1:])
    if n[0] >= top:                      # on a tie nothing, which is the draft
        return 0, n
    return min(b for b in (1, 2, 3, 4) if n[b] == top), n


def weight(j: int, L: int, O: int) -> np.float32:
    return ONE if j < O or j >= L - O else TWO


def fractions(n: np.ndarray, O: int) -> np.ndarray:
    """acc of rows whose reads per label are n int [..., L, 5]: w(j) * (n[b] / max(total, 1)), one float32 divide and one
    float32 multiply by 1 or 2 per element"""
    L = n.shape[-2]
    tot = np.maximum(n.sum(-1), 1).astype(np.float32)
    w = np.array([weight(j, L, O) for j in range(L)], np.float32)
    return (w[:, None] * (n.astype(np.float32) / tot[..., None])).astype(np.float32)


class BadChunk(Exception):
    """the layout is broken at this chunk: PV_ERR_INVALID, d_counts[2]"""

    def __init__(self, chunk):
        super().__init__("chunk %d" % chunk)
        self.chunk = chunk


def in_order(region, chunk_id, n_regions: int, k: int) -> bool:
    g, c = int(region[k]), int(chunk_id[k])
    if g < 0 or g >= n_regions or c < 0:
        return False
    if k == 0:
        return c == 0
    pg = int(region[k - 1])
    return c == int(chunk_id[k - 1]) + 1 if pg == g else (pg < g and c == 0)


def vote(counts, depth, position, index, region, chunk_id, ref_start, ref_off, ref, O: int, want_acc: bool = True,
         want_reads: bool = False):
    """-> (labels uint8 [n, L], acc float32 [n, L, 5] or None, rows whose winner is not the draft's, base rows without reads),
    and with want_reads n[0..4] of every row, int64 [n, L, 5]; BadChunk where the device reports PV_ERR_INVALID"""
    n_chunks, L = position.shape
    labels = np.zeros((n_chunks, L), np.uint8)
    reads = np.zeros((n_chunks, L, 5), np.int64)      # n[0..4] of every row; padding rows keep 0
    changed = no_reads = 0
    bad = []
    for k in range(n_chunks):
        if not in_order(region, chunk_id, len(ref_start), k):
            bad.append(k)
            continue
        g = int(region[k])
        o0, span, rs = int(ref_off[g]), int(ref_off[g + 1]) - int(ref_off[g]), int(ref_start[g])
        for j in range(L):
            p, x = int(position[k, j]), int(index[k, j])
            if p < 0 or x < 0:
                continue
            if x == 0:
                rel = p - rs
                if rel < 0 or rel >= span:
                    bad.append(k)
                    break
                dl = draft_label(ref[o0 + rel])
                lab, n = base_row(counts[k, j], dl)
                changed += lab != dl
                no_reads += sum(n) == 0
            else:
                lab, n = insert_row(counts[k, j], depth[k, j])
                changed += lab >= 1
            labels[k, j] = lab
            reads[k, j] = n
    if bad:
        raise BadChunk(min(bad))
    out = labels, (fractions(reads, O) if want_acc else None), int(changed), int(no_reads)
    return out + (reads,) if want_reads else out
