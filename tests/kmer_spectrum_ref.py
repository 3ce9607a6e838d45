"""The completeness rule of include/pepper_hip.h (the second k-mer section), restated on Python dicts on top of
tests/kmer_qv_ref.py: the hash and the parts, the reads-only counts, the assembly's spectrum and the completeness curve.
test_kmer_spectrum_cpu.py checks it on a worked example; the GPU tests compare every device output with it for equality."""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmer_qv_ref as R  # noqa: E402

M64 = (1 << 64) - 1


def mix(x: int) -> int:
    """the splitmix64 finaliser on 64 bits"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def part_of(x: int, n_parts: int) -> int:
    return (mix(x) >> 32) % n_parts


def home_of(x: int, slots: int) -> int:
    return mix(x) & (slots - 1)


def asm_keys(contigs, k: int) -> Counter:
    """canonical key -> the assembly positions that hold it (its multiplicity); a k-mer lies inside one contig"""
    m = Counter()
    for a in contigs:
        for _, x in R.canon_keys(a, k):
            if x is not None:
                m[x] += 1
    return m


def spectrum(contigs, reads, k: int, cap: int = 1 << 30, counts: Counter = None):
    """-> (ro_hist int64 [256], spectrum int64 [4][256]): the reads' keys the assembly lacks by min(count, cap, 255); the
    assembly's distinct keys by (min(multiplicity, 4) - 1, min(count, cap, 255))"""
    counts = R.read_counts(reads, k) if counts is None else counts
    mult = asm_keys(contigs, k)
    ro, sp = np.zeros(256, np.int64), np.zeros((4, 256), np.int64)
    for x, c in counts.items():
        if x not in mult:
            ro[min(c, cap, 255)] += 1
    for x, m in mult.items():
        sp[min(m, 4) - 1, min(counts.get(x, 0), cap, 255)] += 1
    return ro, sp


def part_counts(reads, k: int, part: int, n_parts: int) -> Counter:
    """the read counts of the keys of one part"""
    return Counter({x: c for x, c in R.read_counts(reads, k).items() if part_of(x, n_parts) == part})


def completeness(ro_hist, spec, s: int):
    """-> (total, found): read k-mers seen s times or more, and those of them the assembly holds"""
    found = int(np.asarray(spec)[:, s:].sum())
    return found + int(np.asarray(ro_hist)[s:].sum()), found
