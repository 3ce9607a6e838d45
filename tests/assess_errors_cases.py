"""The small cases that the tests of assess --errors / -q share: pairs built for the error list and the calibration table, their
qualities, and what the restatement (tests/assess_errors_ref.py) gives for them, computed once. L = 256 throughout."""
import functools

import numpy as np

import assess_errors_ref as E
import assess_ref as R

L = 256


def rnd(seed, n):
    return bytes(b"ACGT"[x] for x in np.random.default_rng(seed).integers(0, 4, n))


def other(*avoid):
    """a base that equals none of the given bytes"""
    return next(bytes([x]) for x in b"ACGT" if x not in avoid)


def quals_of(pairs, salt=0):
    """a different quality at neighbouring bases, every value 0..93 in use"""
    return [((np.arange(len(a), dtype=np.int64) * 7 + 3 * p + salt) % 94).astype(np.uint8) for p, (a, _) in enumerate(pairs)]


def planted(seed, n, every, kinds=(E.SUB, E.DEL, E.INS), truth=None):
    """a truth of n bases (or the given one) and an assembly with one unambiguous planted error about every `every` bases: a
    substitution, a deletion of a base that differs from both neighbours, or an inserted base that differs from both
    neighbours -> (assembly, truth, [(kind, a_pos)])"""
    rng = np.random.default_rng(seed)
    t = rnd(seed + 1000, n) if truth is None else truth
    out, where, pos, k, alen = [], [], 0, 0, 0
    while True:
        nxt = pos + int(rng.integers(every // 2, every * 3 // 2))
        while nxt < n - 40 and (t[nxt] == t[nxt - 1] or t[nxt] == t[nxt + 1]):
            nxt += 1
        if nxt >= n - 40:
            out.append(t[pos:])
            break
        out.append(t[pos:nxt])
        alen += nxt - pos
        pos = nxt
        kind = kinds[k % len(kinds)]
        k += 1
        where.append((kind, alen))
        if kind == E.SUB:
            out.append(other(t[pos]))
            alen += 1
            pos += 1
        elif kind == E.DEL:
            pos += 1
        else:
            out.append(other(t[pos - 1], t[pos]))
            alen += 1
    return b"".join(out), t, where


def case_several_pairs():
    t = [rnd(1, 3000), rnd(2, 700), rnd(3, 200), b"", rnd(4, 1500), rnd(5, 256), rnd(6, 255)]
    pairs = [(planted(10 + i, len(x), 90)[0], planted(10 + i, len(x), 90)[1]) if len(x) > 100 else (x, x) for i, x in enumerate(t)]
    pairs[1] = (pairs[1][1], pairs[1][1])                     # a pair without any error between pairs that have some
    pairs += [(b"", rnd(7, 50)),                              # an empty assembly: 50 deletions at a_pos = 0 = n_A, quality 0
              (rnd(8, 120), b""),                             # an empty truth, 120 > 96: unaligned, no record
              (rnd(9, 90), b""),                              # an empty truth within the band: 90 insertions at b_pos = 0 = n_B
              (rnd(20, 400), rnd(21, 100)),                   # unaligned between pairs with records
              planted(22, 900, 70)[:2]]

    def check(rows, off, hist):
        n = np.diff(off)
        assert n[1] == 0 and n[3] == 0 and n[7] == 50 and n[8] == 0 and n[9] == 90 and n[10] == 0 and n[11] > 5 and n[0] > 20
        assert (rows[off[7]:off[8], [0, 4, 8]] == [0, E.DEL, 0]).all() and (rows[off[9]:off[10], 1] == 0).all()
        assert hist[8].sum() == 0 and hist[10].sum() == 0 and hist[7, :, 0].sum() == 0 and hist[7, 0, 3] == 50
    return pairs, 64, check


def case_segment_edges():
    t = rnd(31, 600)   # anchor 1 at 256, anchor 2 at 512: segments [0, 256), [288, 512), [544, 600)
    sub = bytearray(t)
    for p in (0, 255, 288, 511, 544, 599):
        sub[p] = other(t[p])[0]
    pairs = [(bytes(sub), t),
             (t[:255] + t[256:], t), (t[:288] + t[289:], t), (t, t[:255] + t[256:]), (t, t[:288] + t[289:]),
             (t[:256] + other(t[255], t[256]) + t[256:], t)]

    def check(rows, off, hist):
        assert [(int(r[0]), int(r[3])) for r in rows[off[0]:off[1]]] == [(0, 0), (255, 0), (288, 1), (511, 1), (544, 2), (599, 2)]
        assert (rows[off[0]:off[1], 4] == E.SUB).all()
        assert all(off[k + 1] - off[k] >= 1 for k in range(1, 6))
    return pairs, 64, check


def case_deletions_at_the_ends():
    t = b"GA" + rnd(41, 196) + b"CT"   # the first and the last base differ from their neighbours
    pairs = [(t[1:], t), (t[:-1], t), (t[1:-1], t), (t, t[1:]), (t, t[:-1])]

    def check(rows, off, hist):
        q = quals_of(pairs)
        assert rows[off[0]:off[1]].tolist() == [[0, 0, 0, 0, E.DEL, 0, ord("G"), 0, int(q[0][0])]]
        assert rows[off[1]:off[2]].tolist() == [[199, 199, 1, 0, E.DEL, 0, ord("T"), 0, int(q[1][198])]]
        assert [int(r[0]) for r in rows[off[2]:off[3]]] == [0, 198]
        assert rows[off[3]:off[4]].tolist() == [[0, 0, 3, 0, E.INS, ord("G"), 0, 0, int(q[3][0])]]
        assert rows[off[4]:off[5]].tolist() == [[199, 199, 4, 0, E.INS, ord("T"), 0, 0, int(q[4][199])]]
    return pairs, 64, check


def case_adjacent_runs():
    t = rnd(51, 240)
    ins3 = t[:60] + rnd(52, 3) + t[60:150] + rnd(53, 5) + t[150:]
    del4 = t[:80] + t[84:180] + t[183:]
    both = t[:100] + rnd(54, 2) + t[104:]   # two inserted bases where four are missing
    pairs = [(ins3, t), (del4, t), (both, t), (t, ins3), (t, del4)]

    def check(rows, off, hist):
        for p in range(5):
            r = rows[off[p]:off[p + 1]]
            assert (np.diff(r[:, 0]) >= 0).all() and (np.diff(r[:, 1]) >= 0).all()
        assert (rows[off[1]:off[2], 4] == E.DEL).all() and off[2] - off[1] == 7
        r = rows[off[1]:off[2]]
        assert len(set(r[:4, 0])) == 1 and sorted(r[:4, 1]) == list(r[:4, 1]) and len(set(r[:4, 1])) == 4   # one a_pos, b_pos rising
    return pairs, 64, check


def case_homopolymers():
    rng = np.random.default_rng(91)
    runs = b"".join(bytes([b"ACGT"[int(rng.integers(0, 4))]]) * int(rng.integers(1, 7)) for _ in range(300))
    t = runs[:900]
    a = bytearray(t)
    for p in range(850, 20, -46):
        if p % 3 == 0:
            del a[p]
        elif p % 3 == 1:
            a.insert(p, a[p])
        else:
            a[p] = b"ACGT"[(b"ACGT".index(a[p]) + 1) % 4]
    at = b"AT" * 200

    def check(rows, off, hist):
        r = rows[off[0]:off[1]]
        assert r[r[:, 4] == E.INS, 7].sum() > 2 and r[r[:, 4] == E.DEL, 7].sum() > 2 and (r[r[:, 4] == E.SUB, 7] == 0).all()
        assert (r[:, 7] == 0).any()
    return [(bytes(a), t), (at[:-2], at), (at, at[:-2])], 64, check


def case_many_segments():
    a, t, where = planted(61, 70000, 300)
    pairs = [planted(62, 500, 80)[:2], (a, t), planted(63, 500, 80)[:2]]

    def check(rows, off, hist):
        big = rows[off[1]:off[2]]
        assert big[:, 3].max() > 256 and len(big) == len(where) and off[3] > off[2]
        assert [(int(r[4]), int(r[0])) for r in big] == where
    return pairs, 64, check


def case_q5_q40():
    pairs, quals, want = [], [], []
    for seed, n in ((71, 1500), (72, 300), (73, 2000)):
        a, t, where = planted(seed, n, 60)
        q = np.full(len(a), 40, np.uint8)
        tab = np.zeros((E.QBINS, 4), np.int64)
        for kind, a_pos in where:
            q[a_pos] = 5   # the wrong or extra base itself; for a deletion the base the missing one would stand before
            tab[5, kind] += 1
        tab[5, 0] = len(where)
        tab[40, 0] = len(a) - len(where)
        pairs.append((a, t))
        quals.append(q)
        want.append(tab)

    def check(rows, off, hist):
        assert np.array_equal(hist, np.array(want)) and (rows[:, 8] == 5).all()
    return pairs, 64, check, quals


CASES = {f.__name__[5:]: f for f in (case_several_pairs, case_segment_edges, case_deletions_at_the_ends, case_adjacent_runs,
                                     case_homopolymers, case_many_segments, case_q5_q40)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (pairs, quals, max_shift, records [n][9], pair_err_off, qhist): what the rule gives, computed once and checked
    against what the case was built for"""
    made = CASES[name]()
    pairs, shift, check = made[:3]
    quals = made[3] if len(made) > 3 else quals_of(pairs)
    rows, off, hist = E.errors_batch(pairs, L, shift, quals)
    check(rows, off, hist)
    for r in (rows, off, hist):
        r.setflags(write=False)
    return pairs, quals, shift, rows, off, hist


def totals_of(pairs, shift):
    return R.assess_batch(pairs, L, shift)
