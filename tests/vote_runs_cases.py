"""Hand-made reads for the run-vote tests: a read is a stretch of the draft with edits, turned into a CIGAR and bases; a
region is a draft without accidental runs (no letter twice in a row) with runs planted where the test wants them. On the
CPU the chunks come from min_qual_cases.Layout with the insert rows the reads ask for, the counts and depths from the host
checkers of the builder's planes (counts_ref, depth_ref), the column vote from vote_ref."""
from typing import Dict, List, Sequence, Tuple

import numpy as np

import counts_ref as cr
import depth_ref as dr
import min_qual_cases as mc
import vote_ref as vr
from pepper_thesis_amd.batch import Read, Region, pack_cigar, pack_regions

BASES = "ACGT"
M, I, D, S = 0, 1, 2, 4


def plain(rng, n: int, before: str = "", after: str = "") -> str:
    """n letters, none equal to its neighbour (nor to `before` in front or `after` behind): no stretch of two"""
    out = []
    for i in range(n):
        no = {out[-1] if out else before.upper()} | ({after.upper()} if i == n - 1 else set())
        out.append(str(rng.choice([b for b in BASES if b not in no])))
    return "".join(out)


def draft_with_runs(rng, length: int, runs: Dict[int, Tuple[str, int]]) -> str:
    """a draft of `length` letters with the runs {offset: (letter, n)} and no other stretch of two"""
    d, i = [], 0
    for off in sorted(runs):
        b, n = runs[off]
        assert off >= i
        d.append(plain(rng, off - i, d[-1][-1] if d else "", b))
        d.append(b * n)
        i = off + n
    d.append(plain(rng, length - i, d[-1][-1] if d else ""))
    return "".join(d)


def read_over(draft: str, start: int, a: int, b: int, edits: Dict[int, tuple] = None, **kw) -> Read:
    """the read that shows draft offsets [a, b) with edits {offset: ("del", k) | ("ins", text) | ("sub", letter)}: k draft
    bytes from the offset on deleted, text inserted behind the offset (its anchor), the byte replaced. Lower case is read as
    upper case unless the edit says otherwise."""
    ops, seq = read_parts(draft, a, b, edits)
    return Read.make(start + a, pack_cigar(ops), seq, **kw)


def bam_record(draft: str, tid: int, a: int, b: int, edits: Dict[int, tuple], flag: int, name: str, hp=None, mapq: int = 60) -> dict:
    """read_over as a record for bam_writer.write_bam (the contig starts at 0)"""
    ops, seq = read_parts(draft, a, b, edits)
    return dict(tid=tid, pos=a, mapq=mapq, flag=flag, cigar=ops, seq=seq, qual=[30] * len(seq), name=name, hp=hp)


def read_parts(draft: str, a: int, b: int, edits: Dict[int, tuple] = None) -> Tuple[List[Tuple[int, int]], str]:
    """-> ([(op, length)], bases) of read_over's read"""
    edits = edits or {}
    ops: List[List[int]] = []
    seq = []

    def add(op, n=1):
        if ops and ops[-1][0] == op:
            ops[-1][1] += n
        else:
            ops.append([op, n])
    i = a
    while i < b:
        e = edits.get(i)
        if e and e[0] == "del":
            add(D, e[1])
            i += e[1]
            continue
        seq.append(e[1] if e and e[0] == "sub" else draft[i].upper())
        add(M)
        if e and e[0] == "ins":
            seq.append(e[1])
            add(I, len(e[1]))
        i += 1
    return [(o, n) for o, n in ops], "".join(seq)


def run_edits(s: int, n: int, b: str, length: int, anchor: int = None) -> Dict[int, tuple]:
    """the edits of a read that shows `length` letters for the draft run [s, s + n): deletions left-aligned, inserted letters
    behind `anchor` (default s - 1)"""
    if length < n:
        return {s: ("del", n - length)}
    if length > n:
        return {(s - 1 if anchor is None else anchor): ("ins", b * (length - n))}
    return {}


def host_chain(batch, L: int, O: int):
    """batch -> (Layout, counts, depth, labels, acc) of the column vote, all on the host"""
    regs = []
    for g in range(batch.n_regions):
        _, ins = cr.region_tables(batch, g)
        longest: Dict[int, int] = {}
        for p, x in ins:
            longest[p] = max(longest.get(p, 0), x)
        o0, o1 = int(batch.ref_off[g]), int(batch.ref_off[g + 1])
        regs.append((int(batch.ref_start[g]), batch.ref[o0:o1].tobytes(), longest))
    lay = mc.Layout(regs, L, O)
    counts = cr.row_counts(batch, lay.position, lay.index, lay.region)
    depth = dr.row_depth(batch, lay.position, lay.index, lay.region)
    lab, acc, _, _ = vr.vote(counts, depth, lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, lay.ref_off, lay.ref, O)
    return lay, counts, depth, lab, acc


def spelled(lay, lab, g: int = 0) -> str:
    """the letters region g's rows spell, every (position, index) once"""
    seen, out = set(), []
    for k in np.flatnonzero(lay.region == g):
        for j in range(lay.position.shape[1]):
            key = (int(lay.position[k, j]), int(lay.index[k, j]))
            if key[0] >= 0 and key not in seen:
                seen.add(key)
                out.append((key, int(lab[k, j])))
    return "".join(BASES[l - 1] for _, l in sorted(out) if l)


def one_region(draft: str, reads: Sequence[Read], start: int = 0):
    return pack_regions([Region(start, start + len(draft) - 1, draft.encode(), list(reads))])
