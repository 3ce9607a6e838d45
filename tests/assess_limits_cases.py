"""The cases that take the assess kernels (csrc/assess.hip) to the command's defaults and past their block sizes, and what the
restatements (tests/assess_ref.py, tests/assess_errors_ref.py) give for them, computed once. Every case carries its own
`segment` (L) and `max_shift` and a check of what it was built to show; nothing here imports the package or torch.

The byte-equal shortcut. A segment whose rows and columns are the same bytes has the record `n` matches, no edge, nothing
else: a diagonal of cost 0 wins every `<=` of the rule, runs through band cell 63 and never meets cell 0 or 127. The cases with
hundreds of such segments (`fast`) write that record directly and send every other segment through the restatement as always;
tests/test_assess_limits_cpu.py compares the shortcut with align_segment / walk_segment."""
import functools
from types import SimpleNamespace

import numpy as np

import assess_errors_cases as X
import assess_errors_ref as E
import assess_ref as R

rnd, other, planted, quals_of = X.rnd, X.other, X.planted, X.quals_of


def derive(t, subs=(), dels=(), ins=()):
    """an assembly from the truth t: the truth positions in subs hold another base, those in dels are left out, and in front
    of every position in ins stands a base that differs from both neighbours"""
    subs, dels, ins = set(subs), set(dels), set(ins)
    out, last = [], 0
    for p in sorted(subs | dels | ins):
        out.append(t[last:p])
        last = p
        if p in ins:
            out.append(other(t[p - 1] if p else 0, t[p] if p < len(t) else 0))
        if p in dels:
            last = p + 1
        elif p in subs:
            out.append(other(t[p]))
            last = p + 1
    out.append(t[last:])
    return b"".join(out)


def sized(seed, n, extra_del=0):
    """a pair whose assembly has exactly n bases: a substitution and a deletion with an insertion 30 bases on, in turn, and
    extra_del more deletions near the end of a truth that much longer"""
    t = rnd(seed, n + extra_del)
    spots = list(range(40, n - 40, 90))
    a = derive(t, spots[0::2], spots[1::2] + list(range(n - 20, n - 20 + extra_del)), [p + 30 for p in spots[1::2]])
    assert len(a) == n
    return a, t


# ---- the byte-equal shortcut -----------------------------------------------------------------------------------------

def byte_equal(A, B, a0, b0, n, m):
    return n == m and A[a0:a0 + n] == B[b0:b0 + m]


def equal_counts(n):
    r = dict(match=n, sub=0, ins=0, hp_ins=0, hp_del=0)
    r["del"] = 0
    return r


def align_or_equal(A, B, a0, b0, n, m):
    if byte_equal(A, B, a0, b0, n, m):
        return dict(equal_counts(n), status=R.SEG_ALIGNED, edge=0)
    return R.align_segment(A, B, a0, b0, n, m)


def walk_or_equal(A, B, a0, b0, n, m, Q=None, pair=0, segment=0):
    if byte_equal(A, B, a0, b0, n, m):
        return E.ALIGNED, equal_counts(n), []
    return E.walk_segment(A, B, a0, b0, n, m, Q, pair, segment)


# ---- 1: the command's defaults ---------------------------------------------------------------------------------------

def case_defaults():
    a, t, where = planted(201, 20000, 200)
    exact, short = sized(202, 1024), sized(203, 1023, 1)
    clean = rnd(204, 2500)
    pairs = [(a, t), (b"", rnd(205, 40)), exact, short, (clean, clean), (rnd(206, 70), b"")]

    def check(x):
        assert len(a) // 1024 == 19 and slots_of(pairs, 1024) == 20 + 1 + 2 + 1 + 3 + 1
        assert list(np.diff(x.off)) == [20, 1, 1, 1, 3, 1] and x.tot[:, 2].sum() == 0   # 1024 bases: two slots, one record
        assert [(int(r[4]), int(r[0])) for r in x.err_rows[:x.err_off[1]]] == where and len(where) > 60
        assert x.tot[2, 13] == 0 and x.tot[3, 13] == 0 and x.tot[2, 5:8].sum() > 5 and x.tot[3, 7] > x.tot[3, 6]
        assert x.tot[4, 4] == 2500 and x.tot[4, 5:8].sum() == 0 and x.tot[1, 7] == 40 and x.tot[5, 6] == 70
    return dict(pairs=pairs, L=1024, shift=8192, errors=True, check=check)


# ---- 2: a shifted assembly -------------------------------------------------------------------------------------------

def shifted_pair():
    t = rnd(211, 30000)
    return t[:3000] + t[8000:20000] + rnd(212, 3000) + t[20000:], t


def case_shifted_64():
    def check(x):
        # only where the proportional place has caught up with the true one does a window of 64 hold the 32-mer: anchor 27
        assert x.tot[0, 13] == 1 and x.tot[0, 12] == 1 and len(x.rows) == 2
        assert [int(v) for v in x.rows[0, [2, 3, 4]]] == [27648, 29648, R.SEG_UNALIGNED] and x.rows[1, 4] == R.SEG_ALIGNED
    return dict(pairs=[shifted_pair()], L=1024, shift=64, check=check)


def case_shifted_8192():
    def check(x):
        # 27 slots with an anchor but the three that lie in the foreign bases; c = floor(a * 30000 / 28000) is up to 2000 off
        assert x.tot[0, 13] == 24 and x.tot[0, 12] == 24 and x.tot[0, 2] == 2 and x.tot[0, 10] == 5056 and x.tot[0, 11] == 7056
        assert (x.rows[x.rows[:, 4] == R.SEG_ALIGNED, 7:10].sum() == 0) and int(np.abs(x.rows[:, 1] - x.rows[:, 0]).max()) == 5000
    return dict(pairs=[shifted_pair()], L=1024, shift=8192, check=check)


# ---- 3: the ends of the search window, two hits in one lane, in two lanes of a wave, in two waves ------------------------

WINDOW_A = 9216   # candidate k = 9, t = 0 of the 20 000-base contig; the window of 8192 starts at 1024, thread 0's position
WINDOW_AT = (("first", -8192, True), ("last", 8192, True), ("same_lane", 7 * 256, True), ("same_wave", 256 + 5, True),
             ("other_wave", 197, True), ("before", -8193, False), ("behind", 8193, False))


def twice(t, a, at):
    """t with the 32-mer at a written at `at` too"""
    assert at + R.K <= a or a + R.K <= at
    return t[:at] + t[a:a + R.K] + t[at + R.K:]


def case_window():
    t = rnd(221, 20000)
    pairs = [(t, twice(t, WINDOW_A, WINDOW_A + delta)) for _, delta, _ in WINDOW_AT]

    def check(x):
        # k_as_anchor: thread th tries the positions lo + th + 256 * trip; its lanes are th % 64 of wave th // 64
        lo, hi = WINDOW_A - 8192, WINDOW_A + 8192
        assert lo > 0 and hi < len(t) - R.K and (hi - lo) // 256 + 1 == 65
        th = {name: ((WINDOW_A + delta - lo) % 256, (WINDOW_A + delta - lo) // 256) for name, delta, _ in WINDOW_AT}
        true_th = ((WINDOW_A - lo) % 256, (WINDOW_A - lo) // 256)
        assert WINDOW_A + WINDOW_AT[0][1] == lo and WINDOW_A + WINDOW_AT[1][1] == hi
        assert th["same_lane"][0] == true_th[0] and th["same_lane"][1] != true_th[1]
        assert th["same_wave"][0] != true_th[0] and th["same_wave"][0] // 64 == true_th[0] // 64
        assert th["other_wave"][0] // 64 != true_th[0] // 64
        assert WINDOW_A + WINDOW_AT[5][1] == lo - 1 and WINDOW_A + WINDOW_AT[6][1] == hi + 1
        for p, (name, delta, seen) in enumerate(WINDOW_AT):
            starts = set(int(r[0]) + int(r[2]) for r in x.rows[x.off[p]:x.off[p + 1] - 1])   # where the kept anchors lie
            want = WINDOW_A + 32 if seen else WINDOW_A
            assert want in starts and (WINDOW_A in starts) == (not seen), (name, sorted(starts))
            assert (want, want) in R.find_anchors(pairs[p][0], pairs[p][1], 1024, 8192)
    return dict(pairs=pairs, L=1024, shift=8192, fast=True, check=check)


def case_window_clamped():
    t = rnd(222, 3000)   # max_shift above both lengths: lo = 0 and hi = n_B - 32, the whole truth is searched
    pairs = [(t, twice(t, 1024, 0)), (t, twice(t, 1024, 3000 - 32)), (t, twice(twice(t, 1024, 0), 1024, 3000 - 32)), (t, t)]

    def check(x):
        found = [R.find_anchors(a, b, 1024, 1048576)[0] for a, b in pairs]
        assert found == [(1056, 1056)] * 3 + [(1024, 1024)] and 2048 - 1048576 < 0 and 1024 + 1048576 > 3000 - R.K
    return dict(pairs=pairs, L=1024, shift=1048576, check=check)


# ---- 4: a grid of small pairs, more than one block of them -------------------------------------------------------------

GRID_N = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 130)
GRID_D = (-96, -95, -33, -32, -1, 0, 1, 32, 33, 95, 96, 97)
GRID_PAIRS = 1025
GRID_PREFIXES = (255, 256, 257, 1025)


def grid_pair(rng, n, d):
    """a truth of m = n + d bases and an assembly of n: the difference in up to three runs, two substitutions where n allows"""
    m = n + d
    t = bytes(b"ACGT"[x] for x in rng.integers(0, 4, m))
    cuts = sorted(int(v) for v in rng.integers(0, m + 1, 3)) if m else [0, 0, 0]
    share = [abs(d) // 3 + (k < abs(d) % 3) for k in range(3)]
    out, last = [], 0
    for c, s in zip(cuts, share):
        c = max(c, last)
        out.append(t[last:c])
        last = c
        if d < 0:
            out.append(bytes(b"ACGT"[x] for x in rng.integers(0, 4, s)))
        else:
            last = min(m, c + s)
    out.append(t[last:])
    a = bytearray(b"".join(out))
    if d > 0 and len(a) != n:   # the runs ran into the truth's end: take the rest from the front
        a = a[len(a) - n:]
    assert len(a) == n, (n, d, len(a))
    if n >= 4:
        for p in rng.choice(n, 2, replace=False):
            a[p] = other(a[p])[0]
    return bytes(a), t


@functools.lru_cache(maxsize=None)
def grid_pairs():
    pairs, shape, seed = [], [], 230
    while len(pairs) < GRID_PAIRS:
        rng = np.random.default_rng(seed)
        seed += 1
        for n in GRID_N:
            for d in GRID_D:
                if n + d >= 0:
                    pairs.append(grid_pair(rng, n, d))
                    shape.append((n, d))
    return pairs[:GRID_PAIRS], shape[:GRID_PAIRS]


def case_grid():
    pairs, shape = grid_pairs()

    def check(x):
        assert len(pairs) == 1025 and (len(pairs) + 255) // 256 == 5 and set(shape) == {(n, d) for n in GRID_N for d in GRID_D if n + d >= 0}
        assert list(x.off) == list(range(1026))   # every pair is one segment: the segment's height is the pair's length
        assert [(int(r[2]), int(r[3]) - int(r[2])) for r in x.rows] == shape
        assert [int(r[4]) for r in x.rows] == [int(d == 97) for _, d in shape]
        assert x.tot[:, 5:8].sum() > 20000 and (np.diff(x.err_off) > 0).sum() > 800
    return dict(pairs=pairs, L=256, shift=64, errors=True, check=check)


def prefix(x, k):
    """the expectation of the batch's first k pairs (a pair's records do not depend on the pairs around it)"""
    return SimpleNamespace(pairs=x.pairs[:k], L=x.L, shift=x.shift, rows=x.rows[:x.off[k]], off=x.off[:k + 1], tot=x.tot[:k])


# ---- 5: more anchors in one pair than the chain stages at a time -------------------------------------------------------

STAGE = 1024           # CH_STAGE of k_as_chain
STAGED_SLOTS = 1030    # anchors 1 .. 1030 of the long pair, in slots 0 .. 1029


def case_staged():
    L = 256
    assert STAGED_SLOTS >= STAGE + 6, "the long pair has to reach past what k_as_chain stages at a time"
    n = STAGED_SLOTS * L + 100
    t = rnd(241, n)
    zone = (1021 * L, 1029 * L)   # nothing is planted here
    spots = [p for p in range(700, n - 200, 4900) if not zone[0] - 200 <= p < zone[1] + 200]
    subs = spots[0::2] + [n - 30]                           # the last one in the pair's last segment
    dels, ins = spots[1::2], [p + 60 for p in spots[1::2]]  # balanced: the drift is back to 0 after 60 bases
    a = bytearray(derive(t, subs, dels, ins))
    assert len(a) == n
    # slots 1022 .. 1025 (anchors 1023 .. 1026) have no ACGT-only candidate: the first stage ends and the second begins with
    # slots that hold no anchor, and what thread 0 carries over is anchor 1022's
    for k in range(1023, 1027):
        for c in range(8):
            a[k * L + 32 * c] = ord("N")
    # anchor 1027 is taken at its last candidate, which touches anchor 1028's first; the truth holds the two 32-mers the other
    # way round, so anchor 1028 lies 32 before anchor 1027 there and the chain drops it. (With max_shift = 64 an anchor can only
    # be dropped for a neighbour: the first anchor found behind the boundary, 1027, is 1280 bases behind 1022 and is kept.)
    for c in range(7):
        a[1027 * L + 32 * c] = ord("N")
    x0 = 1027 * L + 224
    b = t[:x0] + t[x0 + 32:x0 + 64] + t[x0:x0 + 32] + t[x0 + 64:]
    pairs = [planted(242, 500, 80)[:2], (bytes(a), b), planted(243, 500, 80)[:2]]

    def check(x):
        assert len(a) // L == STAGED_SLOTS
        found, kept = int(x.tot[1, 13]), int(x.tot[1, 12])
        assert found == STAGED_SLOTS - 4 > STAGE and kept == found - 1
        got = R.find_anchors(pairs[1][0], pairs[1][1], L, 64)
        assert sorted(set(range(1, STAGED_SLOTS + 1)) - {g[0] // L for g in got}) == [1023, 1024, 1025, 1026]
        assert (x0, x0 + 32) in got and (x0 + 32, x0) in got and (x0 + 32, x0) not in R.chain(got)
        assert x.off[2] - x.off[1] == kept + 1 > STAGE + 1
        big = x.err_rows[x.err_off[1]:x.err_off[2]]
        assert big[:, 3].max() > STAGE and (big[:, 3] < 5).any() and len(big) > 100 and x.tot[1, 2] == 0
        assert x.off[1] > 0 and x.off[3] > x.off[2] and x.err_off[3] > x.err_off[2]
    return dict(pairs=pairs, L=L, shift=64, errors=True, fast=True, check=check)


# ---- 6: the ends of the `segment` range --------------------------------------------------------------------------------

def case_segment_288():
    pairs = [planted(251, 3000, 90)[:2], sized(252, 288), sized(253, 287), planted(254, 1500, 60)[:2]]

    def check(x):
        assert [int(v) for v in x.tot[:, 12]] == [(len(a) - 32) // 288 for a, _ in pairs] == [10, 0, 0, 5]
        assert [len(a) // 288 + 1 for a, _ in pairs] == [11, 2, 1, 6]   # slots
        assert x.tot[:, 2].sum() == 0 and len(x.err_rows) > 50
    return dict(pairs=pairs, L=288, shift=8192, errors=True, check=check)


def case_segment_65536():
    n = 65536 + 400
    t = rnd(261, n)
    spots = list(range(900, 65000, 2100))
    a = derive(t, spots[0::3] + [n - 100], spots[1::3], [p + 700 for p in spots[1::3]])   # each deletion balanced 700 bases on
    assert len(a) == n

    def check(x):
        assert len(x.rows) == 2 and (x.rows[:, 4] == R.SEG_ALIGNED).all() and (x.rows[:, 5] == 0).all()
        assert x.rows[0, 2] > 65000 and abs(int(x.rows[0, 3]) - int(x.rows[0, 2])) <= 1 and x.tot[0, 12] == 1
        assert x.tot[0, 5] == len(spots[0::3]) + 1 and x.tot[0, 6] == x.tot[0, 7] == len(spots[1::3]) and x.rows[1, 7] == 1
    return dict(pairs=[(a, t)], L=65536, shift=8192, check=check)


CASES = {f.__name__[5:]: f for f in (case_defaults, case_shifted_64, case_shifted_8192, case_window, case_window_clamped, case_grid,
                                     case_staged, case_segment_288, case_segment_65536)}
WITH_ERRORS = ("defaults", "grid", "staged", "segment_288")


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case and what the rule gives for it, computed once, checked against what the case was built for and read-only:
    pairs, L, shift, rows [n_seg][14], off, tot [n_pairs][16]; with errors also quals, err_rows [n][9], err_off, hist"""
    c = CASES[name]()
    x = SimpleNamespace(pairs=c["pairs"], L=c["L"], shift=c["shift"], errors=c.get("errors", False))
    fast = c.get("fast", False)
    x.rows, x.off, x.tot = R.assess_batch(x.pairs, x.L, x.shift, align_or_equal if fast else None)
    made = [x.rows, x.off, x.tot]
    if x.errors:
        x.quals = quals_of(x.pairs)
        x.err_rows, x.err_off, x.hist = E.errors_batch(x.pairs, x.L, x.shift, x.quals, walk_or_equal if fast else None)
        made += [x.err_rows, x.err_off, x.hist]
    c["check"](x)
    for r in made:
        r.setflags(write=False)
    return x


def slots_of(pairs, L):
    return sum(len(a) // L + 1 for a, _ in pairs)


def offsets_of(pairs):
    a_off = np.zeros(len(pairs) + 1, np.int64)
    b_off = np.zeros(len(pairs) + 1, np.int64)
    a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
    b_off[1:] = np.cumsum([len(b) for _, b in pairs])
    return a_off, b_off
