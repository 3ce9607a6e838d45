"""Seeded inputs of the realignment tests: polish regions (start, end, window, reads) shaped like what
polish_summary.region_from_files hands the realigner, plus hand-made edge cases. Data only; no expected values here."""
import hashlib
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


MAX_WINDOW = 2047        # the realigner's longest window tail (RL_MAX_WINDOW)
MAX_QUERY = 16384        # and its longest query (64 lanes x RL_MAX_STRIP rows)
SWEEP_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 193, 4095, 4096, 4097, 16383, 16384)
TIE_PERIODS = {1: b"A", 2: b"AC", 3: b"ACG", 7: b"GATTACA"}
TIE_STRIPS = (2, 3, 17, 64)
FIXTURE_CASES = (("saturation", "full", 0), ("saturation", "full", 1), ("saturation", "homopolymer", 0),
                 ("saturation", "period2", 0), ("bands", "bands", 4), ("dense", "dense", 0))   # (group, region, read)


def _rand(rng, n: int) -> bytes:
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


def _window_region(name, start, win, queries, offsets=None):
    reads = [_read(start + (offsets[k] if offsets else 0), q) for k, q in enumerate(queries)]
    return name, start, start + max(1, len(win) - 19) - 1, win, reads


def _flanked(rng, core: bytes, n: int, left: int = None) -> bytes:
    left = int(rng.integers(0, n - len(core) + 1)) if left is None else left
    return _rand(rng, left) + core + _rand(rng, n - len(core) - left)


def _clean_cut(rng, win: bytes, mut: bytes, n: int) -> bytes:
    """n bases of the mutated copy, from a seeded place where no mutation fell (the window holds them as they are)"""
    for a in rng.permutation(len(mut) - n + 1).tolist():
        if win.find(mut[a:a + n]) >= 0:
            return mut[a:a + n]
    raise ValueError("no clean stretch of %d bases: choose another seed" % n)


def _sweep(rng):
    """one 2047-base window; a query of every SWEEP_LENGTHS length cut from a mutated copy of it (up to 65 bases from a
    stretch without a mutation, so that 64 and 65 bases can score above 255), longer than the copy with random flanks"""
    win = _rand(rng, MAX_WINDOW)
    mut = _mutate(rng, np.frombuffer(win, np.uint8)).tobytes()
    qs = []
    for n in SWEEP_LENGTHS:
        if n <= 65:
            qs.append(_clean_cut(rng, win, mut, n))
        elif n <= len(mut):
            a = int(rng.integers(0, len(mut) - n + 1))
            qs.append(mut[a:a + n])
        else:
            qs.append(_flanked(rng, mut, n))
    return [_window_region("sweep", 7000, win, qs)]


def _saturation(rng):
    """the largest legal score 4 x 2047 = 8188 (alone, in the middle of a 16384-base query, on a homopolymer) and a
    period-2 repeat whose maxima tie across many lanes"""
    win = _rand(rng, MAX_WINDOW)
    return [_window_region("full", 100, win, [win, _flanked(rng, win, MAX_QUERY, left=7000)]),
            _window_region("homopolymer", 20_000, b"A" * MAX_WINDOW, [b"A" * 5000]),
            _window_region("period2", 40_000, (b"AC" * 1024)[:MAX_WINDOW], [b"AC" * 300])]


LIMIT_OVER_WINDOW = 2100   # window of the "over_window" region; its reads have tails 2100, 2048, 2047 and 1600


def _limits(rng):
    """both sides of each refusal: a 2100-base window with reads whose tails are 2100, 2048, 2047 and 1600 bases; a
    2047-base window with queries of 16385 and 16384 bases; a polisher-shaped region that every batch can take"""
    win = _rand(rng, LIMIT_OVER_WINDOW)
    offs = [0, LIMIT_OVER_WINDOW - MAX_WINDOW - 1, LIMIT_OVER_WINDOW - MAX_WINDOW, 500]
    qs = [_mutate(rng, np.frombuffer(win[o:o + 900 + 100 * k], np.uint8)).tobytes() for k, o in enumerate(offs)]
    win2 = _rand(rng, MAX_WINDOW)
    mut = _mutate(rng, np.frombuffer(win2, np.uint8)).tobytes()
    s, e, w, reads = random_region(911, start=90_000, R=601, n_reads=12)
    return [_window_region("over_window", 3000, win, qs, offs),
            _window_region("over_query", 50_000, win2, [_flanked(rng, mut, MAX_QUERY + 1), _flanked(rng, mut, MAX_QUERY)]),
            ("good", s, e, w, reads)]


def _ties(rng, period: int):
    """a tandem repeat of the period between random flanks, 48 + period bases of it in one window and 330 in another; per
    strip height S in TIE_STRIPS (query length in (64 (S - 1), 64 S]) a pure repeat and a repeat between random flanks, at
    varied phases, lengths and read positions. A query repeat longer than the window's ties the maximum over many rows of
    one column (many lanes, the partial last strip included); a shorter one ties it over many columns."""
    unit = TIE_PERIODS[period]
    out = []
    for tag, rep, total in (("short", 48 + period, 400), ("long", 330, 1200)):
        left = 150 + 11 * period
        body = (unit * (rep // period + 2))[1:1 + rep]
        win = _rand(rng, left) + body + _rand(rng, total - left - rep)
        qs, offs = [], []
        for S in TIE_STRIPS:
            for form in range(2):
                n = 64 * S - int(rng.integers(0, 63))      # any length of this strip height; most leave a partial last strip
                ph = int(rng.integers(0, period))
                if form == 0:
                    q = (unit * (n // period + 2))[ph:ph + n]
                else:
                    k = max(period + 1, n // 2 - int(rng.integers(0, 9)))
                    q = _flanked(rng, (unit * (k // period + 2))[ph:ph + k], n)
                qs.append(q)
                offs.append(int(rng.integers(0, left - 20)))
        out.append(_window_region("period%d_%s" % (period, tag), 1000 * period, win, qs, offs))
    return out


def _bands(rng):
    """one 2047-base window. Reads 0-2: an insertion of k random bases at 300 and a deletion of k bases at 1500
    (k = 3, 40, 100), so the reference span equals the query span and banded_sw starts at width 1; read 3: a plain mutated
    copy; read 4: 1500 random bases between the window's halves, so the band is the whole window."""
    win = _rand(rng, MAX_WINDOW)
    qs = [win[:300] + _rand(rng, k) + win[300:1500] + win[1500 + k:] for k in (3, 40, 100)]
    qs.append(_mutate(rng, np.frombuffer(win, np.uint8)).tobytes())
    qs.append(win[:1023] + _rand(rng, 1500) + win[1023:])
    return [_window_region("bands", 60_000, win, qs)]


def _dense(rng):
    """one 2047-base window in which no base repeats its neighbour (so that a deleted base has one place to go); read 0:
    every third base substituted, read 1: every fourth base deleted (about two cigar words per three query bases, the
    densest a local alignment with 4 / -6 / -8 / -2 keeps)"""
    code = np.cumsum(rng.integers(1, 4, MAX_WINDOW)) % 4
    win = ACGT[code]
    sub = win.copy()
    sub[2::3] = ACGT[(code[2::3] + rng.integers(1, 4, len(code[2::3]))) % 4]
    dele = np.delete(win, np.arange(3, len(win), 4))
    return [_window_region("dense", 80_000, win.tobytes(), [sub.tobytes(), dele.tobytes()])]


def limit_regions(group: str) -> List[Tuple[str, int, int, bytes, List[Read]]]:
    """inputs at the realigner's own limits, as edge_regions gives them: group is "sweep", "saturation", "limits",
    "ties1" / "ties2" / "ties3" / "ties7", "bands" or "dense". Seeded per group; data only."""
    seeds = {"sweep": 11, "saturation": 12, "limits": 13, "bands": 14, "dense": 15}
    if group.startswith("ties"):
        period = int(group[4:])
        return _ties(np.random.default_rng(1600 + period), period)
    rng = np.random.default_rng(seeds[group])
    return {"sweep": _sweep, "saturation": _saturation, "limits": _limits, "bands": _bands, "dense": _dense}[group](rng)


def fixture_case(group: str, region: str, read: int) -> Tuple[str, int, bytes, Read]:
    """one read of limit_regions for the reference fixture -> (fixture name, start, window, read)"""
    for name, start, _, win, reads in limit_regions(group):
        if name == region:
            return "limit/%s/%s/%d" % (group, region, read), start, win, reads[read]
    raise KeyError(region)


def input_digest(start: int, win: bytes, reads: List[Read]) -> np.ndarray:
    """SHA-1 (uint8 [20]) of a case's inputs: what the fixture keeps of the cases whose inputs it does not store"""
    h = hashlib.sha1(b"%d %d|" % (start, len(reads)) + win)
    for rd in reads:
        h.update(b"|%d|" % rd.pos + rd.bases)
    return np.frombuffer(h.digest(), np.uint8)


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
