"""Pure NumPy/Python restatement of the error list and the calibration table of assess (include/pepper_hip.h,
pv_assess_errors). Anchors, chain and segments come from assess_ref; the band sweep and the traceback are walked here again, so
that the path itself is kept. Also the text of the two new tables and a FASTQ reader. Nothing here imports the package."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_ref as R  # noqa: E402

K, W, DMAX, INF = R.K, R.W, R.DMAX, R.INF
QBINS = 94
SUB, INS, DEL = 1, 2, 3
KIND_NAME = {SUB: "sub", INS: "ins", DEL: "del"}
ERR_FIELDS = ("a_pos", "b_pos", "pair", "segment", "kind", "a_base", "b_base", "hp", "qual")
ALIGNED, UNALIGNED = 0, 1


def directions(a, b):
    """the band sweep of one segment (a: its rows, b: its columns, uint8 arrays) -> (dlo, D [n+1][W] with 0 diag, 1 up,
    2 left): the rule of pv_assess, tie-breaks included"""
    n, m = len(a), len(b)
    d = m - n
    dlo = min(0, d) - (W - 1 - abs(d)) // 2
    cs = np.arange(W, dtype=np.int64)
    D = np.zeros((n + 1, W), np.uint8)
    j = dlo + cs
    prev = np.where((j >= 0) & (j <= m), j, INF)
    for i in range(1, n + 1):
        j = i + dlo + cs
        ok = (j >= 0) & (j <= m)
        if m > 0:
            neq = (b[np.clip(j - 1, 0, m - 1)] != a[i - 1]).astype(np.int64)
        else:
            neq = np.zeros(W, np.int64)
        diag = np.where(j >= 1, prev + neq, INF)
        up = np.concatenate([prev[1:], [INF]]) + 1
        T = np.where(ok, np.where(diag <= up, diag, up), INF)
        tdir = np.where(diag <= up, 0, 1)
        pm = np.minimum.accumulate(T - cs)
        left = np.concatenate([[INF], pm[:-1] + cs[1:]])
        take_left = left < T
        prev = np.where(ok, np.where(take_left, left, T), INF)
        D[i] = np.where(take_left, 2, tdir)
    return dlo, D


def qual_of(kind, a_pos, Q, nA):
    """the quality an error is charged with; Q: the contig's raw Phred bytes or None"""
    if Q is None:
        return 255
    q = lambda k: min(int(Q[k]), QBINS - 1)  # noqa: E731
    if kind != DEL:
        return q(a_pos)
    if nA == 0:
        return 0
    return min([q(k) for k in (a_pos - 1, a_pos) if 0 <= k < nA])


def walk_segment(A, B, a0, b0, n, m, Q=None, pair=0, segment=0):
    """-> (status, counts dict, the segment's error records in path order from (0, 0) to (n, m))"""
    cnt = dict(match=0, sub=0, ins=0, hp_ins=0, hp_del=0)
    cnt["del"] = 0
    if abs(m - n) > DMAX:
        return UNALIGNED, cnt, []
    nA, nB = len(A), len(B)
    dlo, D = directions(np.frombuffer(A, np.uint8)[a0:a0 + n], np.frombuffer(B, np.uint8)[b0:b0 + m])
    i, j, recs = n, m, []

    def rec(kind, a_pos, b_pos, a_base, b_base, hp):
        recs.append(dict(a_pos=a_pos, b_pos=b_pos, pair=pair, segment=segment, kind=kind, a_base=a_base, b_base=b_base, hp=int(hp),
                         qual=qual_of(kind, a_pos, Q, nA)))
    while (i, j) != (0, 0):
        c = j - i - dlo
        assert 0 <= c < W and j >= 0, (i, j, c)
        step = 2 if i == 0 else int(D[i, c])
        if step == 0:
            x, y = A[a0 + i - 1], B[b0 + j - 1]
            if x == y:
                cnt["match"] += 1
            else:
                cnt["sub"] += 1
                rec(SUB, a0 + i - 1, b0 + j - 1, x, y, 0)
            i, j = i - 1, j - 1
        elif step == 1:
            x, q = A[a0 + i - 1], b0 + j
            hp = (q - 1 >= 0 and B[q - 1] == x) or (q < nB and B[q] == x)
            cnt["ins"] += 1
            cnt["hp_ins"] += int(hp)
            rec(INS, a0 + i - 1, q, x, 0, hp)
            i -= 1
        else:
            q = b0 + j - 1
            hp = (q - 1 >= 0 and B[q - 1] == B[q]) or (q + 1 < nB and B[q + 1] == B[q])
            cnt["del"] += 1
            cnt["hp_del"] += int(hp)
            rec(DEL, a0 + i, q, 0, B[q], hp)
            j -= 1
    return ALIGNED, cnt, recs[::-1]


def errors_pair(A, B, L, max_shift, Q=None, pair=0, walk=None):
    """A, B upper-cased; Q the assembly's raw Phred bytes or None -> (records, qhist [QBINS][4] or None, totals dict of
    match / sub / ins / del with the anchors' matches, number of unaligned segments). walk: what stands in for walk_segment"""
    walk = walk or walk_segment
    kept = R.chain(R.find_anchors(A, B, L, max_shift))
    recs, tot, unaligned = [], dict(match=0, sub=0, ins=0), 0
    tot["del"] = 0
    hist = None if Q is None else np.zeros((QBINS, 4), np.int64)
    for k, (a0, b0, n, m, anc) in enumerate(R.segments(len(A), len(B), kept)):
        status, cnt, rs = walk(A, B, a0, b0, n, m, Q, pair, k)
        recs += rs
        tot["match"] += anc
        unaligned += status == UNALIGNED
        for f in ("match", "sub", "ins", "del"):
            tot[f] += cnt[f]
        if hist is not None:
            lo = a0 if status == ALIGNED else a0 + n
            q = np.minimum(np.frombuffer(bytes(Q), np.uint8)[lo:a0 + n + anc], QBINS - 1)
            hist[:, 0] += np.bincount(q, minlength=QBINS)
            for r in rs:
                hist[r["qual"], r["kind"]] += 1
    return recs, hist, tot, unaligned


def errors_batch(pairs, L, max_shift, quals=None, walk=None):
    """-> (records as an int64 array [n, len(ERR_FIELDS)], pair_err_off, qhist [n_pairs][QBINS][4] or None)"""
    rows, off, hists = [], [0], []
    for p, (A, B) in enumerate(pairs):
        recs, hist, _, _ = errors_pair(A, B, L, max_shift, None if quals is None else quals[p], p, walk)
        rows += [[r[f] for f in ERR_FIELDS] for r in recs]
        off.append(len(rows))
        hists.append(hist)
    return (np.array(rows, np.int64).reshape(-1, len(ERR_FIELDS)), np.array(off, np.int64),
            None if quals is None else np.array(hists, np.int64).reshape(-1, QBINS, 4))


def apply_errors(A: bytes, recs) -> bytes:
    """the patch: replace at sub, drop at ins, insert b_base at del -> the truth, if no segment of the pair is unaligned"""
    out, pos = [], 0
    for r in recs:   # in order: a_pos never decreases, and a deletion before a_pos comes before what happens at a_pos
        assert r["a_pos"] >= pos, (r, pos)
        out.append(A[pos:r["a_pos"]])
        pos = r["a_pos"]
        if r["kind"] == SUB:
            out.append(bytes([r["b_base"]]))
            pos += 1
        elif r["kind"] == INS:
            pos += 1
        else:
            out.append(bytes([r["b_base"]]))
    out.append(A[pos:])
    return b"".join(out)


# ---- the FASTQ reader ------------------------------------------------------------------------------------------------

class FastqError(ValueError):
    pass


def read_fastq(path, asm):
    """four-line records (@name first word, sequence, +, quality) against asm = [(name, sequence)] of the -a FASTA ->
    {name: raw Phred uint8 array}; every refusal names the contig"""
    with open(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":   # what follows the last newline; an empty contig ends in an empty quality line
        lines.pop()
    want = {n: R.upper(s) for n, s in asm}
    out = {}
    for k in range(0, len(lines), 4):
        rec = [ln.rstrip(b"\r") for ln in lines[k:k + 4]]
        words = rec[0][1:].split()
        name = words[0].decode() if rec[0].startswith(b"@") and words else "record %d" % (k // 4 + 1)
        if len(rec) < 4 or not rec[0].startswith(b"@") or not rec[2].startswith(b"+"):
            raise FastqError("%s: %s is not a four-line record" % (path, name))
        if len(rec[3]) != len(rec[1]):
            raise FastqError("%s: contig %s has %d qualities for %d bases" % (path, name, len(rec[3]), len(rec[1])))
        q = np.frombuffer(rec[3], np.uint8)
        if len(q) and (q.min() < 33 or q.max() > 126):
            raise FastqError("%s: contig %s has a quality byte outside '!'..'~'" % (path, name))
        if name in out:
            raise FastqError("%s: contig %s occurs twice" % (path, name))
        if name in want and R.upper(rec[1]) != want[name]:
            raise FastqError("%s: the sequence of contig %s differs from the assembly's" % (path, name))
        out[name] = (q - 33).astype(np.uint8)
    for n, s in asm:
        if len(s) and n not in out:
            raise FastqError("%s: contig %s of the assembly is missing" % (path, n))
    return out


# ---- the text of the tables ------------------------------------------------------------------------------------------

ERRORS_HEADER = "#name\tkind\tassembly_pos\ttruth_pos\tassembly_base\ttruth_base\thp\tqual\tsegment\n"
CALIBRATION_HEADER = "#name\tqual\tbases\tsubstitutions\tinsertions\tdeletions\terrors\tcolumns\tobserved_QV\n"


def error_line(name, r):
    base = lambda x: chr(x) if x else "."  # noqa: E731
    return "\t".join([name, KIND_NAME[int(r["kind"])], str(int(r["a_pos"])), str(int(r["b_pos"])), base(int(r["a_base"])),
                      base(int(r["b_base"])), str(int(r["hp"])), "." if int(r["qual"]) == 255 else str(int(r["qual"])),
                      str(int(r["segment"]))]) + "\n"


def observed_qv(errors, columns):
    return "inf" if errors == 0 else "%.2f" % (-10.0 * math.log10(errors / columns) + 0.0)   # (+ 0.0: no "-0.00")


def calibration_lines(name, hist):
    out = ""
    for q in range(QBINS):
        b, s, i, d = (int(v) for v in hist[q])
        if b + s + i + d:
            out += "\t".join([name] + [str(v) for v in (q, b, s, i, d, s + i + d, b + d)] + [observed_qv(s + i + d, b + d)]) + "\n"
    return out


def calibrated_from(hist):
    """the lowest quality value q of the table such that the bases of quality >= q have an observed QV of at least q; None
    if no value of the table does"""
    for q in range(QBINS):
        if not hist[q].sum():
            continue
        err, cols = int(hist[q:, 1:].sum()), int(hist[q:, 0].sum() + hist[q:, 3].sum())
        if err == 0 or -10.0 * math.log10(err / cols) >= q:
            return q
    return None


def error_tables(asm, truth, L, max_shift, quals=None):
    """asm, truth: [(name, bytes)] as read from the FASTA files; quals: {name: raw Phred array} or None ->
    (text of _assess.errors.tsv, text of _assess.calibration.tsv or None, the TOTAL table or None)"""
    tr = dict(truth)
    err_txt, cal_txt = ERRORS_HEADER, CALIBRATION_HEADER
    total = np.zeros((QBINS, 4), np.int64)
    for name, a in asm:
        if name not in tr:
            continue
        Q = None if quals is None else quals.get(name, np.zeros(0, np.uint8))
        recs, hist, _, _ = errors_pair(R.upper(a), R.upper(tr[name]), L, max_shift, Q)
        err_txt += "".join(error_line(name, r) for r in recs)
        if quals is not None:
            cal_txt += calibration_lines(name, hist)
            total += hist
    if quals is None:
        return err_txt, None, None
    return err_txt, cal_txt + calibration_lines("TOTAL", total), total
