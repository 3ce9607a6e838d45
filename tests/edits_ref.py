"""Host checker of the polisher's edit list (include/pepper_hip.h, pv_polish_edits) and of the VCF `polish --edits` writes.

It does not look at the device's records. It works on the stitch checker's dictionary (tests/stitch_ref.py: one dict keyed by
(position, index) per region, a region's chunk ids walked in STRING order so that the later id overwrites) and the draft:
walking the dictionary's keys in sorted order gives the primitive edits; walking the draft position by position gives, block
by block, the VCF records; and apply() puts VCF records back on a draft.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import stitch_ref as sr

SUB, DEL, INS = 1, 2, 3
BASES = "ACGT"


def upper(byte: int) -> str:
    return chr(byte - 32) if ord("a") <= byte <= ord("z") else chr(byte)


def column_dict(reg: sr.RegionChunks, row_q: Optional[Dict[int, np.ndarray]] = None) -> Dict[Tuple[int, int], Tuple[int, int]]:
    """sr.small_chunk_stitch's dictionary for one region: (position, index) -> (label, row quality or 255) of the chunk that
    is last in string order among those that hold the key"""
    pred = {}
    for name in sorted(str(c) for c in reg.chunks):
        positions, indices, bases = reg.chunks[int(name)][:3]
        quals = row_q[int(name)].tolist() if row_q is not None else [255] * len(positions)
        for pos, indx, base, q in zip(positions.tolist(), indices.tolist(), bases.tolist(), quals):
            if reg.start > 0 and pos <= reg.start + sr.BUFFER_POSITIONS:
                continue
            if indx < 0 or pos < 0:
                continue
            pred[(pos, indx)] = (base, q)
    return pred


def region_dicts(position, index, region, chunk_id, labels, spans, row_q=None) -> List[dict]:
    """the builder's chunk arrays + labels [+ row qualities] -> one column_dict per batch region"""
    regs = sr.regions_from_chunks(position, index, region, chunk_id, labels, spans)
    out = []
    for g, reg in enumerate(regs):
        rq = None
        if row_q is not None:
            rq = {int(chunk_id[k]): np.asarray(row_q[k]) for k in range(len(chunk_id)) if int(region[k]) == g}
        out.append(column_dict(reg, rq))
    return out


def primitive_edits(pred: dict, draft: bytes, draft_start: int) -> List[tuple]:
    """(position, index, kind, draft byte, base, qual) tuples in key order; draft[p - draft_start] is the draft byte at p"""
    out = []
    for (pos, indx) in sorted(pred):
        label, q = pred[(pos, indx)]
        assert 0 <= label <= 4
        if indx == 0:
            d = draft[pos - draft_start]
            if label == 0:
                out.append((pos, 0, DEL, d, 0, q))
            elif BASES[label - 1] != upper(d):
                out.append((pos, 0, SUB, d, ord(BASES[label - 1]), q))
        elif label != 0:
            out.append((pos, indx, INS, 0, ord(BASES[label - 1]), q))
    return out


def replacements(pred: dict, draft: bytes, draft_start: int) -> Dict[int, Tuple[str, Optional[int]]]:
    """position -> (what stands in the polished sequence for it: its own base or nothing, then its inserted bases; the minimum
    quality of the columns that changed something there, None if none did), for every position with an index-0 key"""
    out = {}
    for (pos, indx) in sorted(pred):
        label, q = pred[(pos, indx)]
        if indx == 0:
            u = upper(draft[pos - draft_start])
            s = BASES[label - 1] if label else ""
            out[pos] = (s, q if s != u else None)
        elif label:
            s, mq = out[pos]
            out[pos] = (s + BASES[label - 1], q if mq is None else min(mq, q))
    return out


def polished(pred: dict, draft: bytes, draft_start: int) -> str:
    """the identity's right-hand side without the stitch: the replacement strings of a region joined"""
    rep = replacements(pred, draft, draft_start)
    return "".join(rep[p][0] for p in sorted(rep))


def vcf_records(rep: Dict[int, Tuple[str, Optional[int]]], draft: bytes, qualities: bool) -> List[tuple]:
    """a contig's replacements (all its regions' dictionaries merged) + its whole draft -> (POS, REF, ALT, QUAL or None):
    blocks are maximal runs of consecutive changed positions"""
    changed = sorted(p for p in rep if rep[p][1] is not None)
    out, i = [], 0
    while i < len(changed):
        j = i
        while j + 1 < len(changed) and changed[j + 1] == changed[j] + 1:
            j += 1
        a, b = changed[i], changed[j]
        ref = "".join(upper(c) for c in draft[a:b + 1])
        alt = "".join(rep[p][0] for p in range(a, b + 1))
        q = min(rep[p][1] for p in range(a, b + 1)) if qualities else None
        if len(alt) == len(ref) or alt[:1] == ref[:1]:
            out.append((a + 1, ref, alt, q))
        elif a > 0:
            out.append((a, upper(draft[a - 1]) + ref, upper(draft[a - 1]) + alt, q))
        elif b + 1 < len(draft):
            out.append((1, ref + upper(draft[b + 1]), alt + upper(draft[b + 1]), q))
        elif alt:                              # the whole contig replaced: both sides non-empty, no anchor to be had
            out.append((1, ref, alt, q))
        i = j + 1
    return out


def parse_vcf(text: str):
    """-> (header lines without the leading ##, the column line, [(CHROM, POS, REF, ALT, QUAL or None)])"""
    header, cols, recs = [], None, []
    for line in text.split("\n"):
        if line.startswith("##"):
            assert cols is None
            header.append(line[2:])
        elif line.startswith("#"):
            cols = line
        elif line:
            f = line.split("\t")
            assert len(f) == 8 and f[2] == "." and f[6] == "PASS" and f[7] == ".", line
            recs.append((f[0], int(f[1]), f[3], f[4], None if f[5] == "." else int(f[5])))
    return header, cols, recs


def no_read_ranges(header: Sequence[str], contig: str) -> List[Tuple[int, int]]:
    """the pepper_no_reads lines of a contig as 0-based inclusive ranges"""
    out = []
    for h in header:
        if h.startswith("pepper_no_reads="):
            c, r = h[len("pepper_no_reads="):].rsplit(":", 1)
            if c == contig:
                first, last = r.split("-")
                out.append((int(first) - 1, int(last) - 1))
    return out


def apply(records: Sequence[tuple], draft: bytes, cut: Sequence[Tuple[int, int]] = ()) -> str:
    """(POS, REF, ALT, ...) records on the upper-cased draft, then the 0-based inclusive ranges of `cut` taken out. A record's
    first base, where REF and ALT share it and differ in length, is the anchor and stays with its own position; so does the last base of a record at POS 1 that is anchored behind."""
    own = [upper(c) for c in draft]           # what stands for every draft position ...
    tail = [""] * len(draft)                  # ... and what is inserted behind it
    last = 0
    for pos, ref, alt in (r[:3] for r in records):
        assert pos > last, (pos, last)        # POS strictly increasing
        last = pos
        p = pos - 1
        assert "".join(own[p:p + len(ref)]) == ref and not any(tail[p:p + len(ref)]), (pos, ref)
        if len(ref) != len(alt) and ref[:1] == alt[:1]:
            ref, alt = ref[1:], alt[1:]
            if not ref:
                tail[p] = alt
                continue
            p += 1
        elif len(ref) != len(alt) and pos == 1 and len(ref) > 1 and ref[-1:] == alt[-1:]:
            ref, alt = ref[:-1], alt[:-1]         # a block at the contig's start is anchored behind: that base stays too
        own[p] = alt
        for k in range(p + 1, p + len(ref)):
            own[k] = ""
    keep = np.ones(len(draft), bool)
    for a, b in cut:
        keep[a:b + 1] = False
    return "".join(own[p] + tail[p] for p in np.flatnonzero(keep).tolist())
