"""Pure NumPy/Python restatement of the assess rule (include/pepper_hip.h, pv_assess): anchors, chain, segments, the band
of 128 with its tie-breaks, the traceback's classification and the totals, plus the text of the two tables and a plain
full-matrix Levenshtein distance. Nothing here imports the package: the tests compare the device and the command with it."""
import math

import numpy as np

K = 32          # anchor length
W = 128         # band cells
DMAX = 96       # |columns - rows| above which a segment is not aligned
INF = 1 << 40

SEG_ALIGNED, SEG_UNALIGNED = 0, 1
SEG_FIELDS = ("a_start", "b_start", "n_rows", "n_cols", "status", "edge", "match", "sub", "ins", "del", "hp_ins", "hp_del",
              "anchor", "pair")
TOTAL_FIELDS = ("segments", "aligned", "unaligned", "edge", "match", "sub", "ins", "del", "hp_ins", "hp_del", "unaligned_a",
                "unaligned_b", "anchors_kept", "anchors_found")
_ACGT = frozenset(b"ACGT")


def upper(seq) -> bytes:
    """bytes a..z upper-cased, everything else as it stands"""
    a = np.frombuffer(bytes(seq), np.uint8).copy()
    low = (a >= ord("a")) & (a <= ord("z"))
    a[low] -= 32
    return a.tobytes()


def find_anchors(A: bytes, B: bytes, L: int, max_shift: int):
    """-> [(a, j)] of every k that has an anchor, in order of k (before the chain)"""
    nA, nB = len(A), len(B)
    out = []
    for k in range(1, nA // L + 1):
        for t in range(8):
            a = k * L + 32 * t
            if a + K > nA:
                break
            kmer = A[a:a + K]
            if not all(x in _ACGT for x in kmer):
                continue
            c = (a * nB) // nA
            lo, hi = max(0, c - max_shift), min(nB - K, c + max_shift)
            hits, j = [], lo
            while j <= hi:
                j = B.find(kmer, j, hi + K)
                if j < 0:
                    break
                hits.append(j)
                j += 1
            if len(hits) == 1:
                out.append((a, hits[0]))
                break
    return out


def chain(anchors):
    kept, ap, bp = [], -K, -K
    for a, b in anchors:
        if a >= ap + K and b >= bp + K:
            kept.append((a, b))
            ap, bp = a, b
    return kept


def segments(nA: int, nB: int, kept):
    """-> [(a0, b0, n, m, anchor)]: anchor = K where a kept anchor ends the segment, 0 for the last one"""
    out, a0, b0 = [], 0, 0
    for a, b in kept:
        out.append((a0, b0, a - a0, b - b0, K))
        a0, b0 = a + K, b + K
    out.append((a0, b0, nA - a0, nB - b0, 0))
    return out


def align_segment(A: bytes, B: bytes, a0: int, b0: int, n: int, m: int):
    """the band sweep and the traceback of one segment -> dict of its counts (status, edge, match, sub, ins, del, hp_*)"""
    r = dict(status=SEG_ALIGNED, edge=0, match=0, sub=0, ins=0, hp_ins=0, hp_del=0)
    r["del"] = 0
    d = m - n
    if abs(d) > DMAX:
        r["status"] = SEG_UNALIGNED
        return r
    dlo = min(0, d) - (W - 1 - abs(d)) // 2
    a = np.frombuffer(A, np.uint8)[a0:a0 + n]
    b = np.frombuffer(B, np.uint8)[b0:b0 + m]
    cs = np.arange(W, dtype=np.int64)
    H = np.full((n + 1, W), INF, np.int64)
    D = np.zeros((n + 1, W), np.uint8)   # 0 diag, 1 up, 2 left
    j = dlo + cs
    ok = (j >= 0) & (j <= m)
    H[0, ok] = j[ok]
    for i in range(1, n + 1):
        j = i + dlo + cs
        ok = (j >= 0) & (j <= m)
        prev = H[i - 1]
        jb = np.clip(j - 1, 0, max(m - 1, 0))
        neq = (b[jb] != a[i - 1]).astype(np.int64) if m > 0 else np.zeros(W, np.int64)
        diag = np.where(j >= 1, prev + neq, INF)
        up = np.concatenate([prev[1:], [INF]]) + 1
        T = np.where(diag <= up, diag, up)
        tdir = np.where(diag <= up, 0, 1)
        T = np.where(ok, T, INF)
        key = T - cs
        pm = np.minimum.accumulate(key)
        left = np.concatenate([[INF], pm[:-1] + cs[1:]])   # H[i][j-1] + 1
        take_left = left < T
        H[i] = np.where(ok, np.where(take_left, left, T), INF)
        D[i] = np.where(take_left, 2, tdir)
    nA, nB = len(A), len(B)
    Bf = B
    i, j = n, m
    while True:
        c = j - i - dlo
        assert 0 <= c < W and H[i, c] < INF, (i, j, c)
        if c == 0 or c == W - 1:
            r["edge"] = 1
        if i == 0 and j == 0:
            break
        step = 2 if i == 0 else int(D[i, c])
        if step == 0:
            if A[a0 + i - 1] == B[b0 + j - 1]:
                r["match"] += 1
            else:
                r["sub"] += 1
            i, j = i - 1, j - 1
        elif step == 1:
            x, q = A[a0 + i - 1], b0 + j      # inserted between truth bytes q-1 and q
            r["ins"] += 1
            if (q - 1 >= 0 and Bf[q - 1] == x) or (q < nB and Bf[q] == x):
                r["hp_ins"] += 1
            i -= 1
        else:
            q = b0 + j - 1
            r["del"] += 1
            if (q - 1 >= 0 and Bf[q - 1] == Bf[q]) or (q + 1 < nB and Bf[q + 1] == Bf[q]):
                r["hp_del"] += 1
            j -= 1
    return r


def assess_pair(A: bytes, B: bytes, L: int, max_shift: int, pair: int = 0, align=None):
    """A, B already upper-cased -> (list of segment dicts with SEG_FIELDS, totals dict with TOTAL_FIELDS). align: what stands
    in for align_segment (the limits cases write the record of a byte-equal segment directly)"""
    align = align or align_segment
    found = find_anchors(A, B, L, max_shift)
    kept = chain(found)
    segs = []
    tot = {f: 0 for f in TOTAL_FIELDS}
    tot["anchors_found"], tot["anchors_kept"] = len(found), len(kept)
    for a0, b0, n, m, anc in segments(len(A), len(B), kept):
        r = align(A, B, a0, b0, n, m)
        r.update(a_start=a0, b_start=b0, n_rows=n, n_cols=m, anchor=anc, pair=pair)
        segs.append(r)
        tot["segments"] += 1
        tot["match"] += anc
        if r["status"] == SEG_UNALIGNED:
            tot["unaligned"] += 1
            tot["unaligned_a"] += n
            tot["unaligned_b"] += m
        else:
            tot["aligned"] += 1
            tot["edge"] += r["edge"]
            for f in ("match", "sub", "ins", "del", "hp_ins", "hp_del"):
                tot[f] += r[f]
    return segs, tot


def assess_batch(pairs, L: int, max_shift: int, align=None):
    """pairs: [(A, B)] upper-cased -> (seg array [n_seg, len(SEG_FIELDS)] int64, pair_seg_off, totals [n_pairs, 16] int64)"""
    rows, off, totals = [], [0], []
    for p, (A, B) in enumerate(pairs):
        segs, tot = assess_pair(A, B, L, max_shift, p, align)
        rows += [[s[f] for f in SEG_FIELDS] for s in segs]
        off.append(len(rows))
        totals.append([tot[f] for f in TOTAL_FIELDS] + [0, 0])
    return (np.array(rows, np.int64).reshape(-1, len(SEG_FIELDS)), np.array(off, np.int64),
            np.array(totals, np.int64).reshape(-1, 16))


def levenshtein(a: bytes, b: bytes) -> int:
    """the full-matrix edit distance, unit costs"""
    x = np.frombuffer(a, np.uint8)
    y = np.frombuffer(b, np.uint8)
    prev = np.arange(len(y) + 1, dtype=np.int64)
    idx = np.arange(len(y) + 1, dtype=np.int64)
    for i in range(1, len(x) + 1):
        t = np.empty(len(y) + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[:-1] + (y != x[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1])


# ---- the text of the tables ------------------------------------------------------------------------------------------

CONTIG_HEADER = ("#name\tstatus\tassembly_length\ttruth_length\taligned_columns\tmatches\tsubstitutions\tinsertions\tdeletions\t"
                 "hp_ins\thp_del\tsegments_aligned\tsegments_unaligned\tsegments_edge\tunaligned_assembly_bases\t"
                 "unaligned_truth_bases\tidentity\tQV\n")
SEGMENT_HEADER = ("#name\tsegment\tassembly_start\tassembly_end\ttruth_start\ttruth_end\tstatus\tedge\tanchor_matches\tmatches\t"
                  "substitutions\tinsertions\tdeletions\thp_ins\thp_del\n")


def identity_qv(M, S, I, D):
    cols, err = M + S + I + D, S + I + D
    if cols == 0:
        return ".", "."
    return "%.6f" % (M / cols), ("inf" if err == 0 else "%.2f" % (-10.0 * math.log10(err / cols)))


def contig_line(name, status, la, lb, t):
    M, S, I, D = t["match"], t["sub"], t["ins"], t["del"]
    ident, qv = identity_qv(M, S, I, D) if status != "unpaired" else (".", ".")
    return "\t".join([name, status] + [str(v) for v in (la, lb, M + S + I + D, M, S, I, D, t["hp_ins"], t["hp_del"], t["aligned"],
                                                          t["unaligned"], t["edge"], t["unaligned_a"], t["unaligned_b"])]
                     + [ident, qv]) + "\n"


def tables(asm, truth, L: int, max_shift: int):
    """asm, truth: [(name, bytes)] as read from the FASTA files -> (text of _assess.tsv, text of _assess.segments.tsv)"""
    tr = dict(truth)
    zero = {f: 0 for f in TOTAL_FIELDS}
    total, la_sum, lb_sum = dict(zero), 0, 0
    contig, seg_txt = CONTIG_HEADER, SEGMENT_HEADER
    seen = set()
    for name, a in asm:
        if name not in tr:
            contig += contig_line(name, "unpaired", len(a), 0, zero)
            continue
        seen.add(name)
        A, B = upper(a), upper(tr[name])
        segs, t = assess_pair(A, B, L, max_shift)
        contig += contig_line(name, "paired", len(A), len(B), t)
        la_sum += len(A)
        lb_sum += len(B)
        for f in TOTAL_FIELDS:
            total[f] += t[f]
        for k, s in enumerate(segs):
            seg_txt += "\t".join([name] + [str(v) for v in (
                k, s["a_start"], s["a_start"] + s["n_rows"], s["b_start"], s["b_start"] + s["n_cols"],
                "unaligned" if s["status"] else "aligned", s["edge"], s["anchor"], s["match"], s["sub"], s["ins"], s["del"],
                s["hp_ins"], s["hp_del"])]) + "\n"
    for name, b in truth:
        if name not in seen:
            contig += contig_line(name, "unpaired", 0, len(b), zero)
    contig += contig_line("TOTAL", "total", la_sum, lb_sum, total)
    return contig, seg_txt
