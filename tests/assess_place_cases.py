"""The placement cases that the CPU tests (the checker against answers written out) and the GPU tests (the device against the
checker) share: the smallest shapes at which the kernels of assess_place.hip can go wrong. A case is (assembly contigs, truth
contigs, step, min_hits, check(records) of what it was built to hold); expected() computes the checker's records once."""
import functools

import numpy as np

import assess_place_ref as P

TILE = 4096   # PV_ASSESS_PLACE_TILE (the tests compare it with the library's)
B_LO, B_HI, TRUTH, STRAND, STATUS, TRIED, HITS, AGREE = range(8)


def rnd(seed, n):
    return bytes(b"ACGT"[x] for x in np.random.default_rng(seed).integers(0, 4, n))


def mutate(seed, a, every=300):
    """a with a substitution, a deletion and an insertion in turn about every `every` bases"""
    rng = np.random.default_rng(seed)
    out, pos, k = [], 0, 0
    while pos < len(a):
        nxt = min(len(a), pos + int(rng.integers(every // 2, every * 3 // 2)))
        out.append(a[pos:nxt])
        pos = nxt
        if pos >= len(a):
            break
        if k % 3 == 0:
            out.append(bytes([b"ACGT"[(b"ACGT".index(a[pos]) + 1) % 4]]))
            pos += 1
        elif k % 3 == 1:
            pos += 1
        else:
            out.append(bytes([b"ACGT"[(b"ACGT".index(a[pos]) + 2) % 4]]))
        k += 1
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def truth3():
    """three truth contigs of 2-6 kb"""
    return (rnd(1, 2100), rnd(2, 4500), rnd(3, 6000))


def _pieces(step):
    t = truth3()
    asm = [t[0][100:1900], P.revcomp(t[1][500:4000]), mutate(11, t[2][300:5800]), P.revcomp(mutate(12, t[2][1000:3000])),
           P.revcomp(t[0]), t[1].lower()]   # (the caller upper-cases: lower case is not A, C, G, T)

    def check(r):
        assert r[:5, STATUS].tolist() == [P.PLACED] * 5 and r[5, STATUS] == P.UNPLACED and r[5, TRIED] == 0
        assert r[:5, TRUTH].tolist() == [0, 1, 2, 2, 0] and r[:5, STRAND].tolist() == [0, 1, 0, 1, 1]
        assert r[0, B_LO:B_HI + 1].tolist() == [100, 1900] and r[1, B_LO:B_HI + 1].tolist() == [500, 4000]
        assert r[4, B_LO:B_HI + 1].tolist() == [0, 2100]
        assert abs(r[2, B_LO] - 300) < 5 and abs(r[2, B_HI] - 5800) < 5 and abs(r[3, B_LO] - 1000) < 5 and abs(r[3, B_HI] - 3000) < 5
        assert r[2, HITS] < r[2, TRIED] and r[0, HITS] == r[0, TRIED] == len(range(0, 1800 - 31, step))
    return asm, list(t), step, 3, check


def case_pieces_step32():
    return _pieces(32)


def case_pieces_step64():
    return _pieces(64)


def case_many_samples():
    """more than 4096 table entries, not a power of two: the sort's launches in global memory, and most keys sampled from
    several contigs (every copy is a hit)"""
    t = truth3()
    asm = [x for c in t for x in (c, P.revcomp(c))]
    for k in range(2):
        asm += [mutate(20 + 10 * k + i, c, 200) for i, c in enumerate(t)] + [P.revcomp(mutate(60 + 10 * k + i, c, 250)) for i, c in enumerate(t)]
    asm.append(rnd(40, 700))

    def check(r):
        assert 4096 < 2 * sum(len(range(0, len(a) - 31, 32)) for a in asm) < 8192
        assert r[:18, STATUS].tolist() == [P.PLACED] * 18 and r[18, STATUS] == P.UNPLACED and r[18, HITS] == 0
        assert r[:18, TRUTH].tolist() == [0, 0, 1, 1, 2, 2] + [0, 1, 2] * 4 and r[:18, STRAND].tolist() == [0, 1] * 3 + ([0] * 3 + [1] * 3) * 2
    return asm, list(t), 32, 3, check


def case_tile_border():
    """one occurrence at each position TILE - 33 .. TILE + 1 of the concatenated truth: the halo and the tile's border"""
    t = [rnd(51, 1000), rnd(52, TILE + 200)]
    at = list(range(TILE - 33, TILE + 2))
    asm = [t[1][g - 1000:g - 1000 + 32] for g in at]

    def check(r):
        assert (r[:, STATUS] == P.PLACED).all() and (r[:, TRUTH] == 1).all() and (r[:, STRAND] == 0).all()
        assert r[:, B_LO].tolist() == [g - 1000 for g in at] and (r[:, B_HI] - r[:, B_LO] == 32).all()
    return asm, t, 32, 1, check


def case_odd_samples():
    """32-mers across a junction, present twice (forward + forward, forward + reverse), palindromic, with an N; the same key
    twice in one contig and once each in two more"""
    x, y, z = rnd(61, 400), rnd(62, 500), rnd(63, 300)
    u, v, w = rnd(64, 32), rnd(65, 32), rnd(66, 32)
    half = rnd(67, 16)
    pal = half + P.revcomp(half)
    with_n = x[100:116] + b"N" + x[117:132]
    t = [x[:200] + u + x[200:300] + v + pal + x[300:], y[:100] + u + y[100:250] + w + y[250:], z[:50] + P.revcomp(v) + z[50:]]
    t[0] = t[0][:100] + with_n + t[0][132:]
    across = t[0][-16:] + t[1][:16]
    asm = [across, u, v, pal, with_n, w + rnd(68, 32) + w, w, P.revcomp(w), x[:31], x[:32]]

    def check(r):
        assert r[:5, STATUS].tolist() == [P.UNPLACED] * 5 and r[:5, TRIED].tolist() == [1, 1, 1, 0, 0] and (r[:5, HITS] == 0).all()
        # the same key twice in one contig: two hits, which name one truth position, so their order is none: misplaced
        assert r[5].tolist() == [282, 314, 1, 0, P.MISPLACED, 3, 2, 2]
        assert r[6].tolist() == [282, 314, 1, 0, P.PLACED, 1, 1, 1] and r[7].tolist() == [282, 314, 1, 1, P.PLACED, 1, 1, 1]
        assert r[8].tolist() == [-1, -1, -1, -1, P.UNPLACED, 0, 0, 0]     # n_A = 31: no sample
        assert r[9].tolist() == [0, 32, 0, 0, P.PLACED, 1, 1, 1]          # n_A = 32: one sample
    return asm, t, 32, 1, check


def case_overhang():
    """contigs that reach over either end of their truth contig: the clamps"""
    t = truth3()
    asm = [rnd(71, 50) + t[0][:500], t[1][-500:] + rnd(72, 50), P.revcomp(rnd(73, 50) + t[2][:500]), P.revcomp(t[0][-500:] + rnd(74, 50))]

    def check(r):
        assert (r[:, STATUS] == P.PLACED).all() and r[:, TRUTH].tolist() == [0, 1, 2, 0] and r[:, STRAND].tolist() == [0, 0, 1, 1]
        assert r[:, B_LO].tolist() == [0, 4000, 0, 1600] and r[:, B_HI].tolist() == [500, 4500, 500, 2100]
    return asm, list(t), 32, 3, check


def case_chimeras():
    """two truth contigs' pieces at 2:1 (placed on the larger part), at 1:1 in both orders (2 H > N fails), and hits in
    reversed order (misplaced)"""
    t = truth3()
    asm = [t[0][100:1380] + t[1][200:840], t[0][100:740] + t[1][200:840], P.revcomp(t[1][200:840]) + t[0][100:740],
           t[0][1000:1320] + t[0][200:520], P.revcomp(t[2][1000:1320] + t[2][200:520])]

    def check(r):
        assert r[0].tolist() == [100, 2020, 0, 0, P.PLACED, 60, 60, 40]
        assert r[1].tolist() == [-1, -1, -1, -1, P.UNPLACED, 40, 40, 20] and r[2].tolist() == r[1].tolist()
        assert r[3, TRUTH:].tolist() == [0, 0, P.MISPLACED, 20, 20, 20] and r[4, TRUTH:].tolist() == [2, 1, P.MISPLACED, 20, 20, 20]
    return asm, list(t), 32, 3, check


def case_min_hits():
    """H = min_hits places, H = min_hits - 1 does not"""
    t = truth3()
    asm = [t[1][1000:1000 + 32 * 5], t[1][2000:2000 + 32 * 4]]

    def check(r):
        assert r[:, STATUS].tolist() == [P.PLACED, P.UNPLACED] and r[:, AGREE].tolist() == [5, 4]
    return asm, list(t), 32, 5, check


def case_no_samples():
    """no contig holds a 32-mer: an empty table"""
    t = truth3()

    def check(r):
        assert (r[:, STATUS] == P.UNPLACED).all() and (r[:, TRIED] == 0).all()
    return [t[0][:31], b"", t[1][:5]], list(t), 32, 1, check


def case_no_truth():
    def check(r):
        assert r.tolist() == [[-1, -1, -1, -1, P.UNPLACED, 4, 0, 0]]
    return [rnd(81, 128)], [], 32, 1, check


CASES = {f.__name__[5:]: f for f in (case_pieces_step32, case_pieces_step64, case_many_samples, case_tile_border, case_odd_samples,
                                     case_overhang, case_chimeras, case_min_hits, case_no_samples, case_no_truth)}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the case, and what the rule gives for it: computed once, checked against what the case was built for, read-only"""
    asm, truth, step, min_hits, check = CASES[name]()
    recs = P.place(asm, truth, step, min_hits)
    check(recs)
    recs.setflags(write=False)
    return asm, truth, step, min_hits, recs


# ---- the command: a renamed, partly reverse-complemented assembly cut from one truth, with planted errors ----------------------

def planted(seed, a, every=150, margin=140):
    """mutate() away from the ends: a contig's placement interval is exact when no indel lies between an end and the nearest hit"""
    return a[:margin] + mutate(seed, a[margin:-margin], every) + a[-margin:]


@functools.lru_cache(maxsize=None)
def command_scenario():
    """-> dict: truth [(name, bytes)], asm [(name, bytes)] as an assembler would write it, quals {name: uint8}, and the same
    assembly by hand: hand_asm oriented like the truth, hand_truth the exact slice under each contig's own name, hand_quals,
    where = {name: (truth name, strand, lo, hi)}; the contig `junk` lies nowhere"""
    tA, tB = rnd(91, 5000), rnd(92, 3000)
    truth = [("chrA", tA[:2500] + tA[2500:].lower()), ("chrB", tB)]
    cut = [("contig_1", "chrA", 0, 0, 2000), ("contig_2", "chrA", 1, 2000, 5000), ("contig_3", "chrB", 0, 500, 2500),
           ("contig_4", "chrB", 1, 2400, 3000)]
    src = {"chrA": tA, "chrB": tB}
    asm, hand_asm, hand_truth, quals, hand_quals, where = [], [], [], {}, {}, {}
    for k, (name, tn, strand, lo, hi) in enumerate(cut):
        piece = planted(100 + k, src[tn][lo:hi])
        q = ((np.arange(len(piece)) * (7 + k)) % 60).astype(np.uint8)
        hand_asm.append((name, piece))
        hand_truth.append((name, src[tn][lo:hi]))
        hand_quals[name] = q
        asm.append((name, P.revcomp(piece) if strand else piece))
        quals[name] = q[::-1].copy() if strand else q
        where[name] = (tn, strand, lo, hi)
    junk = rnd(93, 200)
    for a, q in ((asm, quals), (hand_asm, hand_quals)):
        a.insert(2, ("junk", junk))
        q["junk"] = np.full(200, 30, np.uint8)
    return dict(truth=truth, asm=asm, quals=quals, hand_asm=hand_asm, hand_truth=hand_truth, hand_quals=hand_quals, where=where)


def write_fasta(path, recs, width=70):
    with open(path, "wb") as fh:
        for n, s in recs:
            fh.write(b">" + n.encode() + b" a description\n")
            for i in range(0, len(s), width):
                fh.write(s[i:i + width] + b"\n")
    return str(path)


def write_fastq(path, recs, quals):
    with open(path, "wb") as fh:
        for n, s in recs:
            fh.write(b"@" + n.encode() + b"\n" + s + b"\n+\n" + (quals[n] + 33).astype(np.uint8).tobytes() + b"\n")
    return str(path)


def shift_column(text, col, where, unplaced_word=None):
    """the hand-paired run's table in the placed run's coordinates: lo added to column `col` (several: a tuple) of every line
    whose name is in `where`; with unplaced_word, the status of the other contigs' lines becomes that word"""
    cols = col if isinstance(col, tuple) else (col,)
    out = []
    for ln in text.splitlines(True):
        f = ln.rstrip("\n").split("\t")
        if f[0] in where:
            for c in cols:
                f[c] = str(int(f[c]) + where[f[0]][2])
        elif unplaced_word and not f[0].startswith("#") and f[0] != "TOTAL":
            f[1] = unplaced_word
        out.append("\t".join(f) + "\n")
    return "".join(out)


def placement_table(asm, truth, recs):
    """the placement table from the checker's records"""
    out = ["#name\tstatus\ttruth\tstrand\ttruth_start\ttruth_end\tsamples\thits\tagreeing\n"]
    for (name, _), r in zip(asm, recs):
        r = [int(v) for v in r]
        where = [truth[r[TRUTH]][0], "+-"[r[STRAND]], str(r[B_LO]), str(r[B_HI])] if r[TRUTH] >= 0 else ["."] * 4
        out.append("\t".join([name, ("placed", "unplaced", "misplaced")[r[STATUS]]] + where + [str(v) for v in r[TRIED:]]) + "\n")
    return "".join(out)
