"""`pepper assess`: score a polished assembly (and, with -d, the draft it came from) against a truth FASTA on the device.

Contigs are paired by name, in the same orientation, and taken to be colinear: there is no reverse complement and no
rearrangement search. Per pair the device finds unique 32-mer anchors every --segment bases, chains them and aligns the
stretches between them globally in a band of 128 cells (the rule: include/pepper_hip.h, pv_assess). What is reported is that
alignment: substitutions + insertions + deletions is an upper bound of the edit distance and equals it where the errors are
sparse. Segments whose lengths differ by more than 96 are `unaligned` and never guessed at; `unaligned` and `edge` (the path
touched the band's rim) are the warning signs of a line. The reference has no counterpart.

--errors keeps the traceback's path: every substitution, insertion and deletion in assembly and truth coordinates
(<o>_assess.errors.tsv). -q FILE reads the qualities `polish --qualities` wrote for the assembly and tabulates, per contig and
quality value, how many bases carry it and how many errors were charged to it (<o>_assess.calibration.tsv): predicted quality
against observed error rate (the rule: include/pepper_hip.h, pv_assess_errors). The tool reports; it recommends no threshold.

--place drops the pairing by name: one device call places every assembly contig on the truth by content - truth contig, strand
and interval, from sampled 32-mers that occur once in the truth (the rule: include/pepper_hip.h, pv_assess_place). A placed
contig is reverse-complemented if need be and scored, as above, against its interval of the truth; truth positions in every
table are truth-contig coordinates, and the assembly positions and bases of a contig on the minus strand refer to the
reverse-complemented contig (<o>_assess.placement.tsv says which those are). One interval per contig: no rearrangement search.
"""
import math
import os
import sys
from datetime import datetime
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_CONTIG = 1 << 31
DEFAULT_WORKSPACE = 4 << 30
DEFAULT_PLACE_STEP, DEFAULT_MIN_HITS = 1024, 3
TOTAL_FIELDS = ("segments", "aligned", "unaligned", "edge", "match", "sub", "ins", "del", "hp_ins", "hp_del", "unaligned_a",
                "unaligned_b", "anchors_kept", "anchors_found")
CONTIG_HEADER = ("#name\tstatus\tassembly_length\ttruth_length\taligned_columns\tmatches\tsubstitutions\tinsertions\tdeletions\t"
                 "hp_ins\thp_del\tsegments_aligned\tsegments_unaligned\tsegments_edge\tunaligned_assembly_bases\t"
                 "unaligned_truth_bases\tidentity\tQV\n")
SEGMENT_HEADER = ("#name\tsegment\tassembly_start\tassembly_end\ttruth_start\ttruth_end\tstatus\tedge\tanchor_matches\tmatches\t"
                  "substitutions\tinsertions\tdeletions\thp_ins\thp_del\n")
PLACEMENT_HEADER = "#name\tstatus\ttruth\tstrand\ttruth_start\ttruth_end\tsamples\thits\tagreeing\n"
ERRORS_HEADER = "#name\tkind\tassembly_pos\ttruth_pos\tassembly_base\ttruth_base\thp\tqual\tsegment\n"
CALIBRATION_HEADER = "#name\tqual\tbases\tsubstitutions\tinsertions\tdeletions\terrors\tcolumns\tobserved_QV\n"
QBINS = 94
KIND_NAME = {1: "sub", 2: "ins", 3: "del"}


def log(msg):
    sys.stderr.write("[" + datetime.now().strftime("%m-%d-%Y %H:%M:%S") + "] INFO: " + msg + "\n")
    sys.stderr.flush()


class AssessError(ValueError):
    """what the command refuses (exit status 2)"""


def read_fasta(path: str) -> List[Tuple[str, bytes]]:
    """a plain multi-line FASTA reader (the polished FASTA has no .fai): [(name, sequence bytes)] in file order; the name is
    the header's first word, a record may be empty, blank lines and white space at line ends are dropped"""
    out, name, parts = [], None, []
    with open(path, "rb") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(b">"):
                if name is not None:
                    out.append((name, b"".join(parts)))
                words = line[1:].split()
                name, parts = (words[0].decode() if words else ""), []
            elif line:
                if name is None:
                    raise AssessError("%s: sequence before the first '>' header" % path)
                parts.append(line)
    if name is not None:
        out.append((name, b"".join(parts)))
    names = [n for n, _ in out]
    if len(set(names)) != len(names):
        raise AssessError("%s: a contig name occurs twice" % path)
    return out


def read_fastq(path: str, asm) -> Dict[str, np.ndarray]:
    """the qualities of the assembly asm = [(name, sequence)]: four-line records as `polish --qualities` writes them (@name
    first word, sequence, +, quality) -> {name: raw Phred uint8 array, 0..93}. Refused, naming the contig: a record that is
    not four lines, a quality string of another length than its sequence, a byte outside '!'..'~', a name that occurs twice, a
    sequence that differs from the assembly's (letter case aside), a non-empty contig of the assembly that is missing"""
    with open(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":   # what follows the last newline; an empty contig ends in an empty quality line
        lines.pop()
    want = {n: upper(s) for n, s in asm}
    out = {}
    for k in range(0, len(lines), 4):
        rec = [ln.rstrip(b"\r") for ln in lines[k:k + 4]]
        words = rec[0][1:].split()
        name = words[0].decode() if rec[0].startswith(b"@") and words else "record %d" % (k // 4 + 1)
        if len(rec) < 4 or not rec[0].startswith(b"@") or not rec[2].startswith(b"+"):
            raise AssessError("%s: %s is not a four-line record" % (path, name))
        if len(rec[3]) != len(rec[1]):
            raise AssessError("%s: contig %s has %d qualities for %d bases" % (path, name, len(rec[3]), len(rec[1])))
        q = np.frombuffer(rec[3], np.uint8)
        if len(q) and (int(q.min()) < 33 or int(q.max()) > 126):
            raise AssessError("%s: contig %s has a quality byte outside '!'..'~'" % (path, name))
        if name in out:
            raise AssessError("%s: contig %s occurs twice" % (path, name))
        if name in want and upper(rec[1]) != want[name]:
            raise AssessError("%s: the sequence of contig %s differs from the assembly's" % (path, name))
        out[name] = (q - 33).astype(np.uint8)
    for n, s in asm:
        if len(s) and n not in out:
            raise AssessError("%s: contig %s of the assembly is missing" % (path, n))
    return out


def upper(seq: bytes) -> bytes:
    """bytes a..z upper-cased; everything else stays"""
    a = np.frombuffer(seq, np.uint8).copy()
    low = (a >= ord("a")) & (a <= ord("z"))
    a[low] -= 32
    return a.tobytes()


def check_options(segment: int, max_shift: int) -> None:
    if not (256 <= segment <= 65536 and segment % 32 == 0):
        raise AssessError("--segment %d: must be a multiple of 32 in [256, 65536]" % segment)
    if not 32 <= max_shift <= 1048576:
        raise AssessError("--max_shift %d: must lie in [32, 1048576]" % max_shift)


def direction_bytes(n_a: int, segment: int) -> int:
    """the direction scratch one pair needs: 32 bytes per assembly base and 256 per segment slot"""
    return 32 * n_a + 256 * (n_a // segment + 1)


def error_bytes(n_a: int, segment: int) -> int:
    """what --errors / -q add to one pair's scratch: per segment slot an error count, an error offset and a partial quality
    table of 94 x 4 uint32"""
    return (8 + 8 + 4 * 4 * QBINS) * (n_a // segment + 1)


def pack_launches(lengths: Sequence[int], segment: int, budget: int = DEFAULT_WORKSPACE, errors: bool = False) -> List[List[int]]:
    """assembly lengths of the pairs, in order -> the pairs of each launch: consecutive pairs while their direction scratch
    (with errors: and the error pass's tables) stays within the budget; a pair that alone needs more gets a launch of its own"""
    out, cur, used = [], [], 0
    for i, n in enumerate(lengths):
        need = direction_bytes(n, segment) + (error_bytes(n, segment) if errors else 0)
        if cur and used + need > budget:
            out.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += need
    if cur:
        out.append(cur)
    return out


def assess_pairs(ctx, pairs: Sequence[Tuple[bytes, bytes]], segment: int, max_shift: int, budget: int = DEFAULT_WORKSPACE):
    """[(assembly, truth)] upper-cased -> per pair (segment records, totals dict), launch by launch under the budget"""
    res = [None] * len(pairs)
    for launch in pack_launches([len(a) for a, _ in pairs], segment, budget):
        segs, off, totals = ctx.assess([pairs[i] for i in launch], segment, max_shift)
        if len(segs) and int(segs["status"].max()) > 1:
            raise RuntimeError("assess: a traceback left its band (segment status %d)" % int(segs["status"].max()))
        for k, i in enumerate(launch):
            res[i] = (segs[int(off[k]):int(off[k + 1])].copy(), dict(zip(TOTAL_FIELDS, (int(v) for v in totals[k]))))
    return res


def assess_pairs_errors(ctx, pairs, quals, segment: int, max_shift: int, budget: int = DEFAULT_WORKSPACE):
    """as assess_pairs, through pv_assess_errors; quals: one raw Phred array per pair, or None -> per pair (segment records,
    totals dict, error records, qhist [94][4] or None)"""
    res = [None] * len(pairs)
    for launch in pack_launches([len(a) for a, _ in pairs], segment, budget, errors=True):
        segs, off, totals, errs, eoff, qhist = ctx.assess_errors([pairs[i] for i in launch],
                                                                 None if quals is None else [quals[i] for i in launch],
                                                                 segment, max_shift)
        if len(segs) and int(segs["status"].max()) > 1:
            raise RuntimeError("assess: a traceback left its band (segment status %d)" % int(segs["status"].max()))
        for k, i in enumerate(launch):
            res[i] = (segs[int(off[k]):int(off[k + 1])].copy(), dict(zip(TOTAL_FIELDS, (int(v) for v in totals[k]))),
                      errs[int(eoff[k]):int(eoff[k + 1])].copy(), None if qhist is None else qhist[k].copy())
    return res


def error_line(name: str, r, shift: int = 0) -> str:
    """shift: where the pair's truth begins in its truth contig"""
    def base(x):
        return chr(x) if x else "."
    return "\t".join([name, KIND_NAME[int(r["kind"])], str(int(r["a_pos"])), str(int(r["b_pos"]) + shift), base(int(r["a_base"])),
                      base(int(r["b_base"])), str(int(r["hp"])), "." if int(r["qual"]) == 255 else str(int(r["qual"])),
                      str(int(r["segment"]))]) + "\n"


def calibration_lines(name: str, hist) -> str:
    """one line per quality value that has a base or an error: columns = bases + deletions, errors = S + I + D"""
    out = []
    for q in range(QBINS):
        b, s, i, d = (int(v) for v in hist[q])
        if b + s + i + d:
            err, cols = s + i + d, b + d
            qv = "inf" if err == 0 else "%.2f" % (-10.0 * math.log10(err / cols) + 0.0)   # (+ 0.0: no "-0.00")
            out.append("\t".join([name] + [str(v) for v in (q, b, s, i, d, err, cols)] + [qv]) + "\n")
    return "".join(out)


def calibrated_from(hist):
    """the lowest quality value q of the table such that the bases of quality q or more have an observed QV of at least q;
    None if no value of the table does"""
    for q in range(QBINS):
        if not hist[q].sum():
            continue
        err, cols = int(hist[q:, 1:].sum()), int(hist[q:, 0].sum() + hist[q:, 3].sum())
        if err == 0 or -10.0 * math.log10(err / cols) >= q:
            return q
    return None


def identity_qv(M: int, S: int, I: int, D: int) -> Tuple[str, str]:
    cols, err = M + S + I + D, S + I + D
    if cols == 0:
        return ".", "."
    return "%.6f" % (M / cols), ("inf" if err == 0 else "%.2f" % (-10.0 * math.log10(err / cols)))


def contig_line(name: str, status: str, la: int, lb: int, t: Dict[str, int]) -> str:
    M, S, I, D = t["match"], t["sub"], t["ins"], t["del"]
    ident, qv = identity_qv(M, S, I, D) if status != "unpaired" else (".", ".")
    nums = (la, lb, M + S + I + D, M, S, I, D, t["hp_ins"], t["hp_del"], t["aligned"], t["unaligned"], t["edge"], t["unaligned_a"],
            t["unaligned_b"])
    return "\t".join([name, status] + [str(v) for v in nums] + [ident, qv]) + "\n"


def pair_names(asm, truth):
    """-> (names paired, in the assembly's order; [(name, in assembly?, length)] of the unpaired ones, the assembly's first)"""
    tr, am = dict(truth), dict(asm)
    paired = [n for n, _ in asm if n in tr]
    lone = [(n, True, len(s)) for n, s in asm if n not in tr] + [(n, False, len(s)) for n, s in truth if n not in am]
    return paired, lone


def tables(ctx, asm, truth, segment: int, max_shift: int, budget: int = DEFAULT_WORKSPACE):
    """-> (text of the contig table, text of the segment table, TOTAL's dict)"""
    return _tables(ctx, asm, truth, segment, max_shift, budget)[:3]


def error_tables(ctx, asm, truth, segment: int, max_shift: int, quals=None, budget: int = DEFAULT_WORKSPACE):
    """quals: {name: raw Phred array} of the assembly, or None -> (text of the contig table, of the segment table, TOTAL's
    dict, text of the error list, text of the calibration table or None, TOTAL's quality table or None)"""
    return _tables(ctx, asm, truth, segment, max_shift, budget, True, quals)


def _tables(ctx, asm, truth, segment: int, max_shift: int, budget: int, errors: bool = False, quals=None):
    paired, lone = pair_names(asm, truth)
    if not paired:
        raise AssessError("no contig name occurs in both files")
    tr, am = dict(truth), dict(asm)
    for n in paired:
        if len(am[n]) >= MAX_CONTIG or len(tr[n]) >= MAX_CONTIG:
            raise AssessError("contig %s holds 2^31 bytes or more" % n)
    rows = []
    for name, a in asm:
        if name in tr:
            q = None if quals is None else quals.get(name, np.zeros(0, np.uint8))
            rows.append((name, "paired", upper(a), upper(tr[name]), 0, q))
        else:
            rows.append((name, "unpaired", a, None, 0, None))
    tail = [contig_line(name, "unpaired", 0, ln, ZERO_TOTALS) for name, in_asm, ln in lone if not in_asm]
    return _score_rows(ctx, rows, tail, segment, max_shift, budget, errors, quals is not None)


ZERO_TOTALS = {f: 0 for f in TOTAL_FIELDS}


def _score_rows(ctx, rows, tail, segment: int, max_shift: int, budget: int, errors: bool, with_quals: bool):
    """rows: one per assembly contig, in order: (name, status, assembly, truth or None, truth offset, qualities or None). A row
    with a truth is scored against it (bytes already upper-cased, oriented and sliced) and the truth offset is added to its
    truth positions; a row without one gives a line of lengths only. tail: the contig lines behind the assembly's. -> as
    error_tables (without errors: as tables)"""
    scored = [r for r in rows if r[3] is not None]
    pairs = [(a, b) for _, _, a, b, _, _ in scored]
    if errors:
        res = assess_pairs_errors(ctx, pairs, [r[5] for r in scored] if with_quals else None, segment, max_shift, budget)
    else:
        res = assess_pairs(ctx, pairs, segment, max_shift, budget)
    res = iter(res)
    err_txt, cal_txt, cal_total = [ERRORS_HEADER], [CALIBRATION_HEADER], np.zeros((QBINS, 4), np.int64)
    total, la_sum, lb_sum = dict(ZERO_TOTALS), 0, 0
    contig, seg_txt = [CONTIG_HEADER], [SEGMENT_HEADER]
    for name, status, a, b, shift, _ in rows:
        if b is None:
            contig.append(contig_line(name, status, len(a), 0, ZERO_TOTALS))
            continue
        r = next(res)
        segs, t = r[:2]
        if errors:
            err_txt += [error_line(name, e, shift) for e in r[2]]
            if with_quals:
                cal_txt.append(calibration_lines(name, r[3]))
                cal_total += r[3]
        contig.append(contig_line(name, status, len(a), len(b), t))
        la_sum += len(a)
        lb_sum += len(b)
        for f in TOTAL_FIELDS:
            total[f] += t[f]
        for k, sg in enumerate(segs):
            a0, b0 = int(sg["a_start"]), int(sg["b_start"]) + shift
            vals = (k, a0, a0 + int(sg["n_rows"]), b0, b0 + int(sg["n_cols"]), "unaligned" if int(sg["status"]) else "aligned",
                    int(sg["edge"]), int(sg["anchor"]), int(sg["match"]), int(sg["sub"]), int(sg["ins"]), int(sg["del"]),
                    int(sg["hp_ins"]), int(sg["hp_del"]))
            seg_txt.append("\t".join([name] + [str(v) for v in vals]) + "\n")
    contig += tail
    contig.append(contig_line("TOTAL", "total", la_sum, lb_sum, total))
    if not errors:
        return "".join(contig), "".join(seg_txt), total
    if not with_quals:
        return "".join(contig), "".join(seg_txt), total, "".join(err_txt), None, None
    cal_txt.append(calibration_lines("TOTAL", cal_total))
    return "".join(contig), "".join(seg_txt), total, "".join(err_txt), "".join(cal_txt), cal_total


# ---- --place: contigs placed on the truth by content (the rule: include/pepper_hip.h, pv_assess_place) ------------------------

def check_place_options(step: int, min_hits: int) -> None:
    if not (32 <= step <= 65536 and step % 32 == 0):
        raise AssessError("--place_step %d: must be a multiple of 32 in [32, 65536]" % step)
    if not 1 <= min_hits <= 65535:
        raise AssessError("--min_hits %d: must lie in [1, 65535]" % min_hits)


_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq: bytes) -> bytes:
    """the reverse complement of an upper-cased sequence; bytes other than A, C, G, T keep their value"""
    return bytes(seq).translate(_COMPLEMENT)[::-1]


def place_rows(ctx, asm, truth, step: int, min_hits: int, quals=None):
    """one placement call for the whole assembly against the whole truth -> (the rows _score_rows takes, the placement records).
    A placed contig is reverse-complemented if it lies on the minus strand (its qualities reversed with it) and set against
    the truth's bytes [b_lo, b_hi); an unplaced or misplaced one gives a line of lengths only."""
    from . import _ffi
    if len(truth) > _ffi.PV_ASSESS_PLACE_MAX_TRUTH:
        raise AssessError("the truth holds %d contigs: --place takes at most %d" % (len(truth), _ffi.PV_ASSESS_PLACE_MAX_TRUTH))
    for n, seq in list(asm) + list(truth):
        if len(seq) >= MAX_CONTIG:
            raise AssessError("contig %s holds 2^31 bytes or more" % n)
    A, B = [upper(seq) for _, seq in asm], [upper(seq) for _, seq in truth]
    recs = ctx.assess_place(A, B, step, min_hits)
    rows = []
    for (name, _), a, r in zip(asm, A, recs):
        status = int(r["status"])
        if status != _ffi.PV_ASSESS_PLACED:
            rows.append((name, "misplaced" if status == _ffi.PV_ASSESS_MISPLACED else "unplaced", a, None, 0, None))
            continue
        minus, lo, hi = int(r["strand"]) == 1, int(r["b_lo"]), int(r["b_hi"])
        q = None if quals is None else quals.get(name, np.zeros(0, np.uint8))
        if minus:
            a, q = revcomp(a), (None if q is None else np.ascontiguousarray(q[::-1]))
        rows.append((name, "paired", a, B[int(r["truth"])][lo:hi], lo, q))
    return rows, recs


def placement_text(asm, truth, recs) -> str:
    """<o>_assess.placement.tsv: one line per assembly contig. For a contig on the minus strand every assembly position and
    base of the other tables refers to the reverse-complemented contig."""
    from . import _ffi
    word = {_ffi.PV_ASSESS_PLACED: "placed", _ffi.PV_ASSESS_UNPLACED: "unplaced", _ffi.PV_ASSESS_MISPLACED: "misplaced"}
    out = [PLACEMENT_HEADER]
    for (name, _), r in zip(asm, recs):
        t = int(r["truth"])
        where = [truth[t][0], "-" if int(r["strand"]) else "+", str(int(r["b_lo"])), str(int(r["b_hi"]))] if t >= 0 else ["."] * 4
        out.append("\t".join([name, word[int(r["status"])]] + where + [str(int(r[f])) for f in ("tried", "hits", "agree")]) + "\n")
    return "".join(out)


def truth_cover(truth, recs) -> Tuple[int, int]:
    """-> (truth bases that no placed interval covers, truth bases that more than one covers)"""
    from . import _ffi
    events = {}
    for r in recs:
        if int(r["status"]) == _ffi.PV_ASSESS_PLACED:
            events.setdefault(int(r["truth"]), []).extend([(int(r["b_lo"]), 1), (int(r["b_hi"]), -1)])
    bare = twice = 0
    for t, (_, seq) in enumerate(truth):
        depth, at, once = 0, 0, 0
        for x, d in sorted(events.get(t, [])):
            once += x - at if depth >= 1 else 0
            twice += x - at if depth >= 2 else 0
            depth, at = depth + d, x
        bare += len(seq) - once
    return bare, twice


def place_tables(ctx, asm, truth, step: int, min_hits: int, segment: int, max_shift: int, errors: bool = False, quals=None,
                 budget: int = DEFAULT_WORKSPACE, label: str = "assembly"):
    """--place: -> (what error_tables gives, or without errors and quals what tables gives) + (text of the placement table,)"""
    from . import _ffi
    rows, recs = place_rows(ctx, asm, truth, step, min_hits, quals)
    for (name, _), r in zip(asm, recs):
        if int(r["status"]) != _ffi.PV_ASSESS_PLACED:
            log("assess: contig %s of the %s is %s: %d samples tried, %d hits, %d agreeing" % (
                name, label, "misplaced" if int(r["status"]) == _ffi.PV_ASSESS_MISPLACED else "unplaced", int(r["tried"]),
                int(r["hits"]), int(r["agree"])))
    if all(b is None for _, _, _, b, _, _ in rows):
        raise AssessError("no contig of the %s could be placed on the truth" % label)
    bare, twice = truth_cover(truth, recs)
    log("assess: truth: %d bases lie in no placed interval of the %s, %d in more than one" % (bare, label, twice))
    return _score_rows(ctx, rows, [], segment, max_shift, budget, errors, quals is not None) + (placement_text(asm, truth, recs),)


def write_text(path: str, text: str) -> None:
    """written under a temporary name and renamed when complete"""
    tmp = path + ".partial"
    try:
        with open(tmp, "w") as fh:
            fh.write(text)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def _errors_qv(t):
    return t["sub"] + t["ins"] + t["del"], identity_qv(t["match"], t["sub"], t["ins"], t["del"])[1]


def run(args) -> int:
    try:
        check_options(int(args.segment), int(args.max_shift))
        want_errors, fastq = bool(getattr(args, "errors", False)), getattr(args, "fastq", None)
        place, step, min_hits = bool(getattr(args, "place", False)), getattr(args, "place_step", None), getattr(args, "min_hits", None)
        if not place and (step is not None or min_hits is not None):
            raise AssessError("--place_step and --min_hits belong to --place")
        step, min_hits = int(DEFAULT_PLACE_STEP if step is None else step), int(DEFAULT_MIN_HITS if min_hits is None else min_hits)
        if place:
            check_place_options(step, min_hits)
        for what, p in (("assembly", args.assembly), ("truth", args.truth), ("draft", args.draft)):
            if p is not None and not os.path.isfile(p):
                raise AssessError("cannot find the %s FASTA %s" % (what, p))
        if fastq is not None and not os.path.isfile(fastq):
            raise AssessError("cannot find the FASTQ %s" % fastq)
        asm, truth = read_fasta(args.assembly), read_fasta(args.truth)
        draft = read_fasta(args.draft) if args.draft else None
        quals = read_fastq(fastq, asm) if fastq is not None else None
        for label, seqs in (("assembly", asm), ("draft", draft)):
            for n, in_asm, _ in (pair_names(seqs, truth)[1] if seqs is not None and not place else ()):
                log("assess: contig %s is only in the %s FASTA: unpaired" % (n, label if in_asm else "truth"))
        from . import runtime
        ctx = runtime.Context(int(args.device_id))
        try:
            err_txt = cal_txt = cal_total = draft_err_txt = place_txt = draft_place_txt = None
            draft_txt = draft_total = None
            if place:
                seg, shift = int(args.segment), int(args.max_shift)
                if want_errors or quals is not None:
                    contig_txt, seg_txt, total, err_txt, cal_txt, cal_total, place_txt = place_tables(
                        ctx, asm, truth, step, min_hits, seg, shift, True, quals)
                else:
                    contig_txt, seg_txt, total, place_txt = place_tables(ctx, asm, truth, step, min_hits, seg, shift)
                if draft is not None:
                    r = place_tables(ctx, draft, truth, step, min_hits, seg, shift, want_errors, label="draft")
                    draft_txt, draft_total, draft_place_txt = r[0], r[2], r[-1]
                    draft_err_txt = r[3] if want_errors else None
            elif want_errors or quals is not None:
                contig_txt, seg_txt, total, err_txt, cal_txt, cal_total = error_tables(ctx, asm, truth, int(args.segment),
                                                                                       int(args.max_shift), quals)
            else:
                contig_txt, seg_txt, total = tables(ctx, asm, truth, int(args.segment), int(args.max_shift))
            if draft is not None and want_errors and not place:
                draft_txt, _, draft_total, draft_err_txt = error_tables(ctx, draft, truth, int(args.segment), int(args.max_shift))[:4]
            elif draft is not None and not place:
                draft_txt, _, draft_total = tables(ctx, draft, truth, int(args.segment), int(args.max_shift))
        finally:
            ctx.close()
    except AssessError as e:
        sys.stderr.write("ERROR: assess: %s\n" % e)
        return 2
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    write_text(args.output + "_assess.tsv", contig_txt)
    write_text(args.output + "_assess.segments.tsv", seg_txt)
    if place_txt is not None:
        write_text(args.output + "_assess.placement.tsv", place_txt)
    if draft_place_txt is not None:
        write_text(args.output + "_assess_draft.placement.tsv", draft_place_txt)
    if want_errors:
        write_text(args.output + "_assess.errors.tsv", err_txt)
        if draft_err_txt is not None:
            write_text(args.output + "_assess_draft.errors.tsv", draft_err_txt)
    if cal_txt is not None:
        write_text(args.output + "_assess.calibration.tsv", cal_txt)
        q = calibrated_from(cal_total)
        if q is None:
            log("assess: calibration: at no quality value q do the bases of quality q or more reach an observed QV of q")
        else:
            log("assess: calibration: from quality %d up the observed QV of the bases is at least the quality" % q)
    err, qv = _errors_qv(total)
    if draft_txt is not None:
        write_text(args.output + "_assess_draft.tsv", draft_txt)
        derr, dqv = _errors_qv(draft_total)
        log("assess: errors %d -> %d, QV %s -> %s (draft -> assembly)" % (derr, err, dqv, qv))
    else:
        log("assess: errors %d, QV %s" % (err, qv))
    if total["unaligned"] or total["edge"]:
        log("assess: %d segments unaligned, %d touched the band edge: distrust those lines" % (total["unaligned"], total["edge"]))
    return 0
