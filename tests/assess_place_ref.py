"""The placement rule of include/pepper_hip.h (pv_assess_place) restated by brute force: a Counter over the keys of every truth
32-mer, contig by contig (no junctions), and a loop over the samples. Test infrastructure only; nothing here is fast."""
from collections import Counter

import numpy as np

K = 32
PLACED, UNPLACED, MISPLACED = 0, 1, 2
REC_FIELDS = ("b_lo", "b_hi", "truth", "strand", "status", "tried", "hits", "agree")
CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def key_of(kmer: bytes):
    """the 64-bit key of a 32-mer of A, C, G, T (the first byte in the highest bits), or None"""
    assert len(kmer) == K
    x = 0
    for c in kmer:
        if c not in CODE:
            return None
        x = (x << 2) | CODE[c]
    return x


def rc_key(x: int) -> int:
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def revcomp(seq: bytes) -> bytes:
    """the reverse complement; bytes other than A, C, G, T stay as they are (reversed)"""
    return bytes(seq).translate(COMP)[::-1]


def truth_index(truth):
    """[truth bytes] -> (Counter of keys, {key: (t, j) of the smallest (t, j)})"""
    count, where = Counter(), {}
    for t, b in enumerate(truth):
        for j in range(len(b) - K + 1):
            x = key_of(b[j:j + K])
            if x is not None:
                count[x] += 1
                where.setdefault(x, (t, j))
    return count, where


def place_one(a: bytes, truth, index, step: int, min_hits: int):
    """-> the record of one assembly contig, as a tuple in the order of REC_FIELDS"""
    count, where = index
    n_a = len(a)
    tried, hits = 0, []   # hits: (t, strand, a', j)
    for pos in range(0, n_a - K + 1, step):
        x = key_of(a[pos:pos + K])
        if x is None or x == rc_key(x):
            continue
        tried += 1
        f, r = count.get(x, 0), count.get(rc_key(x), 0)
        if f + r != 1:
            continue
        if f == 1:
            hits.append(where[x] + (0, pos))
        else:
            hits.append(where[rc_key(x)] + (1, n_a - K - pos))
    tally = Counter((t, s) for t, _, s, _ in hits)
    if not tally:
        return (-1, -1, -1, -1, UNPLACED, tried, 0, 0)
    (t, s), H = min(tally.items(), key=lambda kv: (-kv[1], kv[0][0], kv[0][1]))
    N = len(hits)
    if not (H >= min_hits and 2 * H > N):
        return (-1, -1, -1, -1, UNPLACED, tried, N, H)
    mine = sorted((ap, j) for tt, j, ss, ap in hits if (tt, ss) == (t, s))
    (ap_first, j_first), (ap_last, j_last) = mine[0], mine[-1]
    n_b = len(truth[t])
    b_lo = min(max(j_first - ap_first, 0), n_b)
    b_hi = min(max(j_last + (n_a - ap_last), 0), n_b)
    bad = (len(mine) > 1 and j_last <= j_first) or b_hi <= b_lo
    return (b_lo, b_hi, t, s, MISPLACED if bad else PLACED, tried, N, H)


def place(asm, truth, step: int, min_hits: int) -> np.ndarray:
    """[assembly bytes], [truth bytes], upper-cased -> int64 [n_asm, 8] in the order of REC_FIELDS"""
    index = truth_index(truth)
    return np.array([place_one(a, truth, index, step, min_hits) for a in asm], np.int64).reshape(-1, len(REC_FIELDS))
