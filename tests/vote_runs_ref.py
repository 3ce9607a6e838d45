"""Host checker of the polisher's run vote (include/pepper_hip.h, pv_polish_vote_runs). Plain numpy / Python, written from the
header's text: draft bytes -> candidate runs, every read walked through its CIGAR on its own -> voters and histograms, the
decision, then the chunk rows of every decided run. It looks at no kernel output."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from vote_ref import BadChunk, in_order, weight

BASES = "ACGT"
MAX_RUN, MAX_LEN = 48, 63
ALIGNED, READ_ONLY, DRAFT_ONLY = (0, 7, 8), (1, 4), (2, 3, 6)     # BAM CIGAR codes: M = X / I S / D N P


class BadState(Exception):
    """a decided run needs more insert rows than the chunks hold: PV_ERR_STATE"""


class Run(NamedTuple):
    region: int
    s: int          # draft position of the first base
    n: int
    b: str
    S: int = 0
    V: int = 0
    h: tuple = ()
    L: Optional[int] = None   # the winner, None: undecided


def _up(c: int) -> str:
    return chr(c - 32) if 97 <= c <= 122 else chr(c)


def stretches(draft: bytes) -> List[Tuple[int, int, str]]:
    """(first offset, length, letter) of every maximal stretch of one of A, C, G, T (upper-cased)"""
    out, i = [], 0
    while i < len(draft):
        b = _up(draft[i])
        j = i + 1
        if b in BASES:
            while j < len(draft) and _up(draft[j]) == b:
                j += 1
            out.append((i, j - i, b))
        i = j
    return out


def candidates(draft: bytes, min_run: int) -> Tuple[List[Tuple[int, int, str]], int, int]:
    """-> (the runs voted on as (offset, n, b), candidates seen, candidates skipped as adjacent)"""
    cand = [(s, n, b) for s, n, b in stretches(draft) if min_run <= n <= MAX_RUN and s - 1 >= 0 and s + n < len(draft)]
    covered = set()
    for s, n, _ in cand:
        covered.update(range(s, s + n))
    kept = [(s, n, b) for s, n, b in cand if s - 1 not in covered and s + n not in covered]
    return kept, len(cand), len(cand) - len(kept)


def aligned_offsets(pos: int, cigar) -> Dict[int, int]:
    """draft position -> read offset of every base the read aligns (M, =, X)"""
    at, rp, qp = {}, int(pos), 0
    for w in cigar:
        op, ln = int(w) & 0xF, int(w) >> 4
        if op in ALIGNED:
            for i in range(ln):
                at[rp + i] = qp + i
            rp, qp = rp + ln, qp + ln
        elif op in READ_ONLY:
            qp += ln
        elif op in DRAFT_ONLY:
            rp += ln
    return at


def winner(h, n: int) -> int:
    top = max(h)
    best = [l for l, v in enumerate(h) if v == top]
    if n in best:
        return n
    return min(best, key=lambda l: (abs(l - n), l))


def region_runs(batch, g: int, min_run: int) -> Tuple[List[Run], int, int]:
    """the runs of region g with their votes, and (candidates seen, skipped)"""
    o0, o1, rs = int(batch.ref_off[g]), int(batch.ref_off[g + 1]), int(batch.ref_start[g])
    draft = bytes(np.asarray(batch.ref[o0:o1], np.uint8))
    kept, seen, skipped = candidates(draft, min_run)
    reads = []
    for r in range(int(batch.read_off[g]), int(batch.read_off[g + 1])):
        if int(batch.read_mapq[r]) == 0:
            continue
        cig = batch.cigar[int(batch.cigar_off[r]):int(batch.cigar_off[r + 1])]
        reads.append((aligned_offsets(int(batch.read_pos[r]), cig),
                      bytes(np.asarray(batch.bases[int(batch.base_off[r]):int(batch.base_off[r + 1])], np.uint8))))
    runs = []
    for off, n, b in kept:
        s = rs + off
        e = s + n - 1
        S = V = 0
        h = [0] * (MAX_LEN + 1)
        for at, seq in reads:
            if s - 1 not in at or e + 1 not in at:
                continue
            S += 1
            q0, q1 = at[s - 1], at[e + 1]
            ln = q1 - q0 - 1
            if ln > MAX_LEN or _up(seq[q0]) == b or _up(seq[q1]) == b or any(_up(c) != b for c in seq[q0 + 1:q1]):
                continue
            V += 1
            h[ln] += 1
        L = winner(h, n) if V >= 1 and 2 * V > S else None
        runs.append(Run(g, s, n, b, S, V, tuple(h), L))
    return runs, seen, skipped


def vote_runs(batch, position, index, region, chunk_id, labels, acc, O: int, min_run: int):
    """-> (labels, acc or None, [decided, PV_OK, -1, changed, seen, skipped], runs): the planes of the column vote with the rows
    of every decided run rewritten (the inputs are left alone). BadChunk / BadState where the device reports PV_ERR_INVALID /
    PV_ERR_STATE; min_run outside 2..48 is a ValueError (the call itself refuses it)."""
    if not 2 <= min_run <= MAX_RUN:
        raise ValueError("min_run")
    position, index = np.asarray(position), np.asarray(index)
    n_chunks, L_ = position.shape
    G = len(batch.ref_start)
    lab = np.array(labels, np.uint8)
    out_acc = None if acc is None else np.array(acc, np.float32)
    if n_chunks == 0 or int(batch.ref_off[G]) == 0:
        return lab, out_acc, [0, 0, -1, 0, 0, 0], []
    bad = []
    for k in range(n_chunks):
        if not in_order(region, chunk_id, G, k):
            bad.append(k)
            continue
        g = int(region[k])
        rs, span = int(batch.ref_start[g]), int(batch.ref_off[g + 1]) - int(batch.ref_off[g])
        base = (position[k] >= 0) & (index[k] == 0)
        if ((position[k][base] < rs) | (position[k][base] >= rs + span)).any():
            bad.append(k)
    runs, seen, skipped = [], 0, 0
    for g in range(G):
        r, a, b = region_runs(batch, g, min_run)
        runs, seen, skipped = runs + r, seen + a, skipped + b
    if bad:
        raise BadChunk(min(bad))
    decided = [r for r in runs if r.L is not None]
    for r in decided:
        e = r.s + r.n - 1
        # the span's rows over all chunks of the region, each (position, index) once, in order
        of_region = (np.asarray(region) == r.region)[:, None]
        in_span = of_region & (position >= 0) & (((position >= r.s) & (position <= e)) | ((position == r.s - 1) & (index > 0)))
        kk, jj = np.nonzero(in_span)
        keys = sorted(set(zip(position[kk, jj].tolist(), index[kk, jj].tolist())))
        inserts = [key for key in keys if key[1] > 0]
        want = {}
        if r.L <= r.n:
            for p, x in keys:
                want[(p, x)] = 0 if x > 0 or p - r.s < r.n - r.L else 1 + BASES.index(r.b)
        else:
            if len(inserts) < r.L - r.n:
                raise BadState("run at %d of region %d" % (r.s, r.region))
            for p, x in keys:
                want[(p, x)] = 1 + BASES.index(r.b) if x == 0 or inserts.index((p, x)) < r.L - r.n else 0
        frac = np.float32(r.h[r.L]) / np.float32(r.V)
        for k, j in zip(kk.tolist(), jj.tolist()):
            l = want[(int(position[k, j]), int(index[k, j]))]
            lab[k, j] = l
            if out_acc is not None:
                out_acc[k, j] = 0
                out_acc[k, j, l] = weight(j, L_, O) * frac
    changed = sum(r.L != r.n for r in decided)
    return lab, out_acc, [len(decided), 0, -1, changed, seen, skipped], runs
