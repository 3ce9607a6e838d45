"""The k-mer support rule of include/pepper_hip.h (pv_kmer_support), restated on Python dicts: contigs and a list of read byte
strings in, counts, runs, segments and histogram out. test_kmer_qv_cpu.py checks it against a brute-force quadratic count; the
GPU tests compare every device output with it for equality."""
from collections import Counter

import numpy as np

NO_KEY = 0xFFFFFFFF
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}   # A C G T, upper case only


def key_of(kmer: bytes):
    """the 2k-bit key, first byte highest, or None if a byte is not A, C, G, T"""
    x = 0
    for c in kmer:
        if c not in _CODE:
            return None
        x = (x << 2) | _CODE[c]
    return x


def rc_key(x: int, k: int) -> int:
    y = 0
    for _ in range(k):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def canon(kmer: bytes):
    x = key_of(kmer)
    return None if x is None else min(x, rc_key(x, len(kmer)))


def canon_keys(seq: bytes, k: int):
    """(i, canonical key or None) for every i with i + k <= len(seq), rolling: the same values as canon(seq[i:i + k])"""
    mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
    fwd = rev = run = 0
    for j, c in enumerate(bytes(seq)):
        v = _CODE.get(c)
        run = run + 1 if v is not None else 0
        v = v or 0
        fwd = ((fwd << 2) | v) & mask
        rev = (rev >> 2) | ((3 - v) << top)
        if j >= k - 1:
            yield j - k + 1, (min(fwd, rev) if run >= k else None)


def read_counts(reads, k: int) -> Counter:
    """canonical key -> occurrences over every read and every offset j with j + k <= len"""
    c = Counter()
    for r in reads:
        for _, x in canon_keys(r, k):
            if x is not None:
                c[x] += 1
    return c


def position_counts(contigs, counts: Counter, k: int, cap: int):
    """per contig a uint32 array of its length: min(cap, count) at a keyed position, NO_KEY elsewhere (a position without a key,
    and the last k - 1 bytes, which start no k-mer)"""
    out = []
    for a in contigs:
        v = np.full(len(a), NO_KEY, np.uint32)
        for i, x in canon_keys(a, k):
            if x is not None:
                v[i] = min(cap, counts.get(x, 0))
        out.append(v)
    return out


def summarise(contigs, planes, k: int, min_count: int, segment: int):
    """-> (contig counts int64 [n][3], seg_off, segs, runs [r][3], hist [256])"""
    n = len(contigs)
    ctg = np.zeros((n, 3), np.int64)
    seg_off = np.zeros(n + 1, np.int64)
    segs, runs, hist = [], [], np.zeros(256, np.int64)
    for p, (a, v) in enumerate(zip(contigs, planes)):
        positions = max(0, len(a) - k + 1)
        seg = np.zeros((len(a) + segment - 1) // segment, np.int64)
        first = None
        for i in range(positions):
            c = int(v[i])
            bad = c != NO_KEY and c < min_count
            if c != NO_KEY:
                ctg[p, 0] += 1
                hist[min(c, 255)] += 1
            else:
                ctg[p, 2] += 1
            if bad:
                ctg[p, 1] += 1
                seg[i // segment] += 1
                if first is None:
                    first = i
            elif first is not None:
                runs.append((p, first, i - 1))
                first = None
        if first is not None:
            runs.append((p, first, positions - 1))
        segs.append(seg)
        seg_off[p + 1] = seg_off[p] + len(seg)
    return (ctg, seg_off, np.concatenate(segs) if segs else np.zeros(0, np.int64),
            np.array(runs, np.int64).reshape(-1, 3), hist)


def support(contigs, reads, k: int, cap: int = 1 << 30, min_count: int = 1, segment: int = 1024, counts: Counter = None):
    """the whole rule -> (contig counts, seg_off, segs, runs, hist, flat position counts uint32)"""
    counts = read_counts(reads, k) if counts is None else counts
    planes = position_counts(contigs, counts, k, cap)
    flat = np.concatenate(planes) if planes else np.zeros(0, np.uint32)
    return summarise(contigs, planes, k, min_count, segment) + (flat,)
