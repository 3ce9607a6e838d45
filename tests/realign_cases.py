"""Seeded inputs of the realignment tests: polish regions (start, end, window, reads) shaped like what
polish_summary.region_from_files hands the realigner, plus hand-made edge cases. Data only; no expected values here."""
from typing import List, Tuple

import numpy as np

from pepper_thesis_amd.batch import Read, Region

ACGT = np.frombuffer(b"ACGT", np.uint8)


def _mutate(rng, seq: np.ndarray, sub=0.03, ins=0.01, dele=0.01, long_ins=0.0) -> np.ndarray:
    out = []
    for b in seq.tolist():
        u = rng.random()
        if u < dele:
            continue
        if u < dele + sub:
            b = int(ACGT[rng.integers(4)])
        out.append(b)
        if rng.random() < ins:
            out.extend(ACGT[rng.integers(0, 4, rng.integers(1, 4))].tolist())
        if long_ins and rng.random() < long_ins:
            out.extend(ACGT[rng.integers(0, 4, rng.integers(50, 400))].tolist())
    return np.asarray(out, np.uint8)


def random_region(seed: int, start: int = 5000, R: int = 1201, n_reads: int = 30, contig_len: int = None,
                  long_ins: float = 0.0005, alphabet: bytes = b"") -> Tuple[int, int, bytes, List[Read]]:
    """-> (start, end, window, reads): a draft window of R + 19 bases (fewer when contig_len cuts it), reads that start
    inside the region and run at most to its end (clipped), drawn from a mutated copy of the draft"""
    rng = np.random.default_rng(seed)
    end = start + R - 1
    wlen = R + 19 if contig_len is None else min(R + 19, contig_len - start)
    win = ACGT[rng.integers(0, 4, wlen)].copy()
    if alphabet:
        k = rng.integers(0, wlen, wlen // 50)
        win[k] = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), len(k))]
    reads = []
    for _ in range(n_reads):
        a = int(rng.integers(0, R)) if rng.random() < 0.5 else 0
        b = int(rng.integers(a + 1, R + 1)) if rng.random() < 0.5 else R
        q = _mutate(rng, win[a:b], long_ins=long_ins)
        if alphabet and len(q):
            k = rng.integers(0, len(q), max(1, len(q) // 80))
            q[k] = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), len(k))]
        if len(q) == 0:
            q = ACGT[rng.integers(0, 4, 1)]
        reads.append(Read.make(start + a, "%dM" % len(q), q.tobytes(), 30, bool(rng.random() < 0.5)))
    return start, end, win.tobytes(), reads


def _read(pos, bases):
    b = bases.encode() if isinstance(bases, str) else bases
    return Read.make(pos, "%dM" % max(1, len(b)), b, 20)


def edge_regions(high: bool = False) -> List[Tuple[str, int, int, bytes, List[Read]]]:
    """hand-made cases: ties, odd bytes, long queries, tiny scores, 1-base reads, a contig end, a dropped read.
    high: also bytes >= 128, which the reference reads out of its translation table (pinned to code 4 here; not in the
    fixture)"""
    rng = np.random.default_rng(7)
    cases = []
    hp = b"A" * 40 + b"C" * 30 + b"ACACACACACACACACAC" + b"GATTACA" * 10 + b"T" * 25
    cases.append(("ties", 100, 100 + len(hp) - 20, hp,
                  [_read(100, b"A" * 12), _read(100, b"AAAACCCC"), _read(105, b"ACAC"), _read(110, b"CACACACA"),
                   _read(100, b"GATTACAGATTACA"), _read(120, b"TTTTTAAAAA"), _read(100, b"AC" * 20),
                   _read(140, b"GATTACGATTACA"), _read(100, hp[30:90]), _read(101, b"CCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCC")]))
    odd = b"ACGTNNACGTacgtUuRYKMSWBDHVN" * 6 + (bytes([200, 65, 67, 255, 71, 84]) if high else b"")
    cases.append(("alphabet", 10, 10 + len(odd) - 20, odd,
                  [_read(10, odd[:60]), _read(12, b"NNNN"), _read(10, b"acgtacgtuuuu"), _read(20, odd[30:90].lower()),
                   _read(10, bytes([200, 65, 67, 255, 71, 84, 65]) if high else b"NACGT"), _read(11, b"RYKMSWBDHV" * 3)]))
    w = ACGT[rng.integers(0, 4, 300)].tobytes()
    long_q = w[:100] + ACGT[rng.integers(0, 4, 600)].tobytes() + w[100:280]
    cases.append(("long_query", 0, 280, w, [_read(0, long_q), _read(3, long_q[50:]), _read(0, w[:280] + w[:280])]))
    cases.append(("scores", 1000, 1100, w[:120],
                  [_read(1000, b"N" * 50), _read(1000, b"TTTTTT" if b"T" not in w[:120] else b"NNNN"),
                   _read(1000, w[:120]), _read(1010, w[10:110]), _read(1000, w[:40]), _read(1050, w[50:52])]))
    cases.append(("one_base", 0, 99, w[:119], [_read(0, w[0:1]), _read(50, w[50:51]), _read(99, b"N"), _read(40, b"T"),
                                              _read(7, b"G")]))
    cases.append(("contig_end", 500, 560, w[:66], [_read(500, w[:66]), _read(540, w[40:66]), _read(560, w[60:66])]))
    cases.append(("dropped", 200, 300, w[:120], [_read(200, w[:50]), _read(150, w[:80]), _read(199, w[:20]),
                                                 _read(250, w[50:100])]))
    return cases


def as_region(start, end, win, reads, contig="ctg") -> Region:
    R = end - start + 1
    ref = win[:R] + b"N" * max(0, R - len(win))
    return Region(start, end, ref, reads, contig=contig)


def fast_region(rng, start: int, R: int = 1201, n_reads: int = 30, long_ins: float = 0.02) -> Region:
    """a vectorised random_region for large batches: reads of a window with 3 % substitutions, 1 % 1-3 base insertions and
    deletions, and now and then one 50-400 base insert; Region.window holds the window"""
    win = ACGT[rng.integers(0, 4, R + 19)]
    reads = []
    for _ in range(n_reads):
        a = int(rng.integers(0, R // 2)) if rng.random() < 0.5 else 0
        b = int(rng.integers(a + 1, R + 1)) if rng.random() < 0.5 else R
        q = win[a:b].copy()
        m = rng.random(len(q)) < 0.03
        q[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
        q = np.delete(q, np.flatnonzero(rng.random(len(q)) < 0.01))
        at = np.flatnonzero(rng.random(len(q)) < 0.01)
        q = np.insert(q, at, ACGT[rng.integers(0, 4, len(at))])
        if rng.random() < long_ins:
            k = int(rng.integers(0, len(q) + 1))
            q = np.concatenate([q[:k], ACGT[rng.integers(0, 4, int(rng.integers(50, 400)))], q[k:]])
        if len(q) == 0:
            q = ACGT[:1].copy()
        reads.append(Read.make(start + a, "%dM" % len(q), q.tobytes(), 30, bool(rng.random() < 0.5)))
    reg = as_region(start, start + R - 1, win.tobytes(), reads)
    reg.window = win.tobytes()
    return reg
