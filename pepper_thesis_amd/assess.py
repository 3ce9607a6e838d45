"""`pepper assess`: score a polished assembly (and, with -d, the draft it came from) against a truth FASTA on the device.

Contigs are paired by name, in the same orientation, and taken to be colinear: there is no reverse complement and no
rearrangement search. Per pair the device finds unique 32-mer anchors every --segment bases, chains them and aligns the
stretches between them globally in a band of 128 cells (the rule: include/pepper_hip.h, pv_assess). What is reported is that
alignment: substitutions + insertions + deletions is an upper bound of the edit distance and equals it where the errors are
sparse. Segments whose lengths differ by more than 96 are `unaligned` and never guessed at; `unaligned` and `edge` (the path
touched the band's rim) are the warning signs of a line. The reference has no counterpart.
"""
import math
import os
import sys
from datetime import datetime
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_CONTIG = 1 << 31
DEFAULT_WORKSPACE = 4 << 30
TOTAL_FIELDS = ("segments", "aligned", "unaligned", "edge", "match", "sub", "ins", "del", "hp_ins", "hp_del", "unaligned_a",
                "unaligned_b", "anchors_kept", "anchors_found")
CONTIG_HEADER = ("#name\tstatus\tassembly_length\ttruth_length\taligned_columns\tmatches\tsubstitutions\tinsertions\tdeletions\t"
                 "hp_ins\thp_del\tsegments_aligned\tsegments_unaligned\tsegments_edge\tunaligned_assembly_bases\t"
                 "unaligned_truth_bases\tidentity\tQV\n")
SEGMENT_HEADER = ("#name\tsegment\tassembly_start\tassembly_end\ttruth_start\ttruth_end\tstatus\tedge\tanchor_matches\tmatches\t"
                  "substitutions\tinsertions\tdeletions\thp_ins\thp_del\n")


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


def pack_launches(lengths: Sequence[int], segment: int, budget: int = DEFAULT_WORKSPACE) -> List[List[int]]:
    """assembly lengths of the pairs, in order -> the pairs of each launch: consecutive pairs while their direction scratch
    stays within the budget; a pair that alone needs more gets a launch of its own"""
    out, cur, used = [], [], 0
    for i, n in enumerate(lengths):
        need = direction_bytes(n, segment)
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
    paired, lone = pair_names(asm, truth)
    if not paired:
        raise AssessError("no contig name occurs in both files")
    tr, am = dict(truth), dict(asm)
    for n in paired:
        if len(am[n]) >= MAX_CONTIG or len(tr[n]) >= MAX_CONTIG:
            raise AssessError("contig %s holds 2^31 bytes or more" % n)
    pairs = [(upper(am[n]), upper(tr[n])) for n in paired]
    res = dict(zip(paired, assess_pairs(ctx, pairs, segment, max_shift, budget)))
    zero = {f: 0 for f in TOTAL_FIELDS}
    total, la_sum, lb_sum = dict(zero), 0, 0
    contig, seg_txt = [CONTIG_HEADER], [SEGMENT_HEADER]
    lone_asm = {n: ln for n, in_asm, ln in lone if in_asm}
    for name, a in asm:
        if name in lone_asm:
            contig.append(contig_line(name, "unpaired", len(a), 0, zero))
            continue
        segs, t = res[name]
        contig.append(contig_line(name, "paired", len(a), len(tr[name]), t))
        la_sum += len(a)
        lb_sum += len(tr[name])
        for f in TOTAL_FIELDS:
            total[f] += t[f]
        for k, s in enumerate(segs):
            a0, b0 = int(s["a_start"]), int(s["b_start"])
            vals = (k, a0, a0 + int(s["n_rows"]), b0, b0 + int(s["n_cols"]), "unaligned" if int(s["status"]) else "aligned",
                    int(s["edge"]), int(s["anchor"]), int(s["match"]), int(s["sub"]), int(s["ins"]), int(s["del"]), int(s["hp_ins"]),
                    int(s["hp_del"]))
            seg_txt.append("\t".join([name] + [str(v) for v in vals]) + "\n")
    for name, in_asm, ln in lone:
        if not in_asm:
            contig.append(contig_line(name, "unpaired", 0, ln, zero))
    contig.append(contig_line("TOTAL", "total", la_sum, lb_sum, total))
    return "".join(contig), "".join(seg_txt), total


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
        for what, p in (("assembly", args.assembly), ("truth", args.truth), ("draft", args.draft)):
            if p is not None and not os.path.isfile(p):
                raise AssessError("cannot find the %s FASTA %s" % (what, p))
        asm, truth = read_fasta(args.assembly), read_fasta(args.truth)
        draft = read_fasta(args.draft) if args.draft else None
        for label, seqs in (("assembly", asm), ("draft", draft)):
            for n, in_asm, _ in (pair_names(seqs, truth)[1] if seqs is not None else ()):
                log("assess: contig %s is only in the %s FASTA: unpaired" % (n, label if in_asm else "truth"))
        from . import runtime
        ctx = runtime.Context(int(args.device_id))
        try:
            contig_txt, seg_txt, total = tables(ctx, asm, truth, int(args.segment), int(args.max_shift))
            draft_txt = draft_total = None
            if draft is not None:
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
