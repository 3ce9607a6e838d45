"""`polish --edits`: what the polisher changed in the draft, as a VCF beside the FASTA.

The device leaves one 16-byte record per edited column (pv_polish_edits_dev, the rule in include/pepper_hip.h): a
substitution or a deletion at a draft position, or one inserted base behind it. This module is the host side: the record
type, the composer that joins the records of a contig into VCF records, and the writer.

Composer. A contig's records, sorted by (position, index), are cut into blocks: maximal runs whose positions are equal or
consecutive. A block covers draft [a, b]; REF is the upper-cased draft there and ALT the replacements of a..b joined (per
position: the substituted base, nothing for a deletion or the upper-cased draft byte, then its inserted bases). Where ALT is
as long as REF, or starts with REF's first byte, the record stands at a; otherwise the draft byte before a is put in front of
both, or, at the contig start, the byte after b behind both. A block that covers the whole contig has neither: it is written
as it stands if anything is left, and a contig deleted as a whole gets a warning and no record. No left-alignment in repeats
and no splitting are applied.
"""
import os
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _ffi

EDIT_DTYPE = np.dtype([("position", "<i8"), ("index", "<i4"), ("kind", "u1"), ("draft", "u1"), ("base", "u1"), ("qual", "u1")])
assert EDIT_DTYPE.itemsize == 16
KIND_SUB, KIND_DEL, KIND_INS = _ffi.PV_EDIT_SUB, _ffi.PV_EDIT_DEL, _ffi.PV_EDIT_INS
# `polish --evidence`: one record beside every edit record (pv_polish_evidence, the rule in include/pepper_hip.h)
EVIDENCE_DTYPE = np.dtype([("depth", "<u2"), ("ref", "<u2"), ("alt_fwd", "<u2"), ("alt_rev", "<u2")])
assert EVIDENCE_DTYPE.itemsize == 8
EVIDENCE_INFO_LINES = (
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads over the weakest edited column of the record">',
    '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads that spell the draft, reads that spell the edit, at that column">',
    '##INFO=<ID=SAF,Number=A,Type=Integer,Description="Forward-strand reads that spell the edit at that column">',
    '##INFO=<ID=SAR,Number=A,Type=Integer,Description="Reverse-strand reads that spell the edit at that column">',
)


class VcfRecord(NamedTuple):
    """one line of the edits VCF: pos is 1-based; qual None gives `.`"""
    pos: int
    ref: str
    alt: str
    qual: Optional[int]


class EvidenceVcfRecord(NamedTuple):
    """a VcfRecord of a run with --evidence: evidence is (depth, ref, alt_fwd, alt_rev) of the record's weakest column"""
    pos: int
    ref: str
    alt: str
    qual: Optional[int]
    evidence: Tuple[int, int, int, int]


def info_text(evidence: Tuple[int, int, int, int]) -> str:
    """the INFO column of a record with evidence"""
    depth, ref, fwd, rev = (int(v) for v in evidence)
    return "DP=%d;AD=%d,%d;SAF=%d;SAR=%d" % (depth, ref, fwd + rev, fwd, rev)


def output_vcf_path(fasta_path: str) -> str:
    """the VCF of --edits lies beside the FASTA: ..._pepper_polished.fa -> ..._pepper_polished.edits.vcf.gz"""
    assert fasta_path.endswith(".fa"), fasta_path
    return fasta_path[:-3] + ".edits.vcf.gz"


def compose_records(contig: str, edits: np.ndarray, draft: bytes, qualities: bool, warn=None,
                    evidence: Optional[np.ndarray] = None) -> List[VcfRecord]:
    """the records of one contig (EDIT_DTYPE, the pieces in region-start order) + the contig's draft -> its VCF records, POS
    strictly increasing. ValueError (naming the contig) when the records are not strictly increasing in (position, index),
    as happens when -r lists overlapping ranges of one contig, or reach past the draft. qualities: QUAL is the minimum qual
    of the block's records, else None. warn(msg): told about a block that deletes the whole contig (no record is written).
    evidence (EVIDENCE_DTYPE, one per edit record): the records are EvidenceVcfRecords that carry the evidence of their
    block's weakest column, the one with the lowest alt_fwd + alt_rev (the first such on a tie); all four numbers are that
    column's."""
    n = len(edits)
    if evidence is not None and len(evidence) != n:
        raise ValueError("contig %s: %d evidence records for %d edit records" % (contig, len(evidence), n))
    if n == 0:
        return []
    pos, idx = edits["position"].astype(np.int64), edits["index"].astype(np.int64)
    if n > 1:
        step = (pos[1:] > pos[:-1]) | ((pos[1:] == pos[:-1]) & (idx[1:] > idx[:-1]))
        if not step.all():
            k = int(np.flatnonzero(~step)[0])
            raise ValueError("contig %s: the edit records are not in increasing (position, index) order at (%d, %d) -> (%d, %d): "
                             "overlapping ranges of one contig cannot share an edits VCF"
                             % (contig, pos[k], idx[k], pos[k + 1], idx[k + 1]))
    if int(pos[0]) < 0 or int(pos[-1]) >= len(draft):
        raise ValueError("contig %s: an edit at position %d lies outside the draft (%d bases)"
                         % (contig, int(pos[0]) if int(pos[0]) < 0 else int(pos[-1]), len(draft)))
    up = np.frombuffer(draft, np.uint8).copy()
    up[(up >= ord("a")) & (up <= ord("z"))] -= 32
    kind, base, qual = edits["kind"], edits["base"], edits["qual"]
    # what stands in ALT, in order: every record (a deletion gives nothing), and in front of a position's insert records the
    # draft byte they follow where the position has no record of its own
    new_pos = np.ones(n, bool)
    new_pos[1:] = pos[1:] != pos[:-1]
    lone = new_pos & (idx > 0)
    slot = np.cumsum(1 + lone) - 1             # a record's own place; its position's draft byte, if any, right before
    chars = np.zeros(int(slot[-1]) + 1, np.uint8)
    chars[slot] = base
    chars[slot[lone] - 1] = up[pos[lone]]
    gives = np.ones(len(chars), bool)
    gives[slot] = kind != KIND_DEL
    new_block = np.ones(n, bool)
    new_block[1:] = pos[1:] - pos[:-1] > 1
    first = np.flatnonzero(new_block)          # the first record of every block
    block = np.cumsum(new_block) - 1
    item_block = np.zeros(len(chars), np.int64)
    item_block[slot] = block
    item_block[slot[lone] - 1] = block[lone]
    alt_end = np.cumsum(np.bincount(item_block[gives], minlength=len(first))).tolist()
    alt_all = chars[gives].tobytes().decode("latin-1")
    ref_all = up.tobytes().decode("latin-1")
    a_all, b_all = pos[first].tolist(), pos[np.append(first[1:], n) - 1].tolist()
    q_all = np.minimum.reduceat(qual, first).tolist() if qualities else [None] * len(first)
    ev_all = [None] * len(first)
    if evidence is not None:
        alt = evidence["alt_fwd"].astype(np.int64) + evidence["alt_rev"].astype(np.int64)
        lowest = np.minimum.reduceat(alt, first)[block]
        # the first column of every block whose support is the block's lowest
        weakest = np.minimum.reduceat(np.where(alt == lowest, np.arange(n), n), first)
        ev_all = [tuple(int(v) for v in evidence[k]) for k in weakest.tolist()]
    out, o0 = [], 0
    for a, b, o1, q, ev in zip(a_all, b_all, alt_end, q_all, ev_all):
        ref, alt = ref_all[a:b + 1], alt_all[o0:o1]
        o0 = o1
        if len(alt) == len(ref) or (alt and alt[0] == ref[0]):
            vpos = a + 1
        elif a > 0:
            ref, alt, vpos = ref_all[a - 1] + ref, ref_all[a - 1] + alt, a
        elif b + 1 < len(draft):
            ref, alt, vpos = ref + ref_all[b + 1], alt + ref_all[b + 1], 1
        elif alt:
            vpos = 1                           # the whole contig replaced: REF and ALT are non-empty, no anchor is to be had
        else:
            if warn is not None:
                warn("contig %s: the edits delete the whole contig; no VCF record is written for it" % contig)
            continue
        out.append(VcfRecord(vpos, ref, alt, q) if ev is None else EvidenceVcfRecord(vpos, ref, alt, q, ev))
    return out


def no_read_runs(ranges: Iterable[Tuple[str, int, int]]) -> List[Tuple[str, int, int]]:
    """(contig, first, last) kept ranges (0-based, inclusive) of the regions that gave no chunks, in run order -> the maximal
    runs of adjacent ranges per contig, 1-based inclusive"""
    runs: List[List] = []
    for contig, first, last in ranges:
        if last < first:
            continue
        if runs and runs[-1][0] == contig and runs[-1][2] == first:   # (the run's 1-based last is the 0-based position behind it)
            runs[-1][2] = last + 1
        else:
            runs.append([contig, first + 1, last + 1])
    return [tuple(r) for r in runs]


def vcf_text(source: str, reference: str, contigs: Sequence[Tuple[str, int]], no_reads: Sequence[Tuple[str, int, int]],
             records: Dict[str, Sequence[VcfRecord]], min_depth: int = 0, min_qual: int = 0, haplotype: int = 0,
             evidence: bool = False, min_support: int = 0, consensus: str = "", min_run: int = 0) -> str:
    """header (fileformat, source, reference, one contig line per contig of the run in natural order, one pepper_no_reads line
    per read-free run, the column line) and the records, contigs in natural order; eight columns, no samples.
    min_depth >= 1 (`polish --min_depth`): one pepper_min_depth line stands in the place of the pepper_no_reads lines; the
    run then filled its read-free regions from the draft, so there are none to name.
    min_qual >= 1 (`polish --min_qual`): one pepper_min_qual line behind them, before the column line.
    min_support >= 1 (`polish --min_support`): one pepper_min_support line behind the pepper_min_qual line.
    haplotype >= 1 (`polish -hp`): one pepper_haplotype line, the last before the column line.
    consensus (`polish --vote`: "vote"): one pepper_consensus line, the first of the pepper_* lines: the labels came from the
    reads' majority, not from a model.
    min_run >= 2 (`polish --vote --runs`, consensus "vote+runs"): one pepper_min_run line directly behind the pepper_consensus line.
    evidence (`polish --evidence`): four ##INFO lines (DP, AD, SAF, SAR) in front of the pepper_* lines, and the INFO column of
    every EvidenceVcfRecord holds its numbers (info_text); any other record keeps `.`."""
    from .polish import natural_key
    names = sorted((c for c, _ in contigs), key=natural_key)
    length = dict(contigs)
    lines = ["##fileformat=VCFv4.2", "##source=" + source, "##reference=" + reference]
    lines += ["##contig=<ID=%s,length=%d>" % (c, length[c]) for c in names]
    if evidence:
        lines += list(EVIDENCE_INFO_LINES)
    if consensus:
        lines.append("##pepper_consensus=" + consensus)
    if min_run >= 2:
        lines.append("##pepper_min_run=%d" % min_run)
    if min_depth >= 1:
        assert not no_reads, no_reads
        lines.append("##pepper_min_depth=%d" % min_depth)
    lines += ["##pepper_no_reads=%s:%d-%d" % r for r in no_reads]
    if min_qual >= 1:
        lines.append("##pepper_min_qual=%d" % min_qual)
    if min_support >= 1:
        lines.append("##pepper_min_support=%d" % min_support)
    if haplotype >= 1:
        lines.append("##pepper_haplotype=%d" % haplotype)
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    for c in names:
        for r in records.get(c, ()):
            info = info_text(r.evidence) if evidence and len(r) > 4 else "."
            lines.append("%s\t%d\t.\t%s\t%s\t%s\tPASS\t%s" % (c, r.pos, r.ref, r.alt, "." if r.qual is None else str(r.qual), info))
    return "\n".join(lines) + "\n"


def write_edits_vcf(path: str, source: str, reference: str, contigs: Sequence[Tuple[str, int]],
                    no_reads: Sequence[Tuple[str, int, int]], records: Dict[str, Sequence[VcfRecord]], min_depth: int = 0,
                    min_qual: int = 0, haplotype: int = 0, evidence: bool = False, min_support: int = 0,
                    consensus: str = "", min_run: int = 0) -> None:
    """vcf_text through bamio.write_vcf_gz (bgzip + tabix): `path` and `path`.tbi, both written under temporary names and
    renamed when complete"""
    from . import bamio
    stem, ext = path[:-len(".vcf.gz")], ".vcf.gz"
    assert path.endswith(ext), path
    tmp = stem + ".partial" + ext
    try:
        bamio.write_vcf_gz(tmp, vcf_text(source, reference, contigs, no_reads, records, min_depth, min_qual, haplotype, evidence,
                                              **({"min_support": min_support} if min_support else {}),
                                              **({"consensus": consensus} if consensus else {}),
                                              **({"min_run": min_run} if min_run else {})))
        os.replace(tmp + ".tbi", path + ".tbi")
        os.replace(tmp, path)
    except BaseException:
        for p in (tmp, tmp + ".tbi"):
            try:
                os.remove(p)
            except FileNotFoundError:
                pass
        raise
