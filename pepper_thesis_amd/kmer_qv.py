"""`pepper kmer_qv`: score an assembly by the support its k-mers have in the reads, on the device, where no truth exists.

What a user of `polish` has is the draft, the BAM and the polished FASTA. A k-mer of the assembly that no read (with
--min_count N: fewer than N read k-mers) contains is taken to be an error; from the share of such k-mers follow an error rate
and a QV, and their positions say where to look (the rule: include/pepper_hip.h, pv_kmer_support; the rule of Merqury and
yak). The reference has no counterpart.

The reads are what the polisher sees: the aligned part of the primary reads of the BAM (min_mapq 0, no supplementary reads, no
down-sampling), soft clips and leading insertions gone, read interval by interval (--interval bases) and clipped at the
interval edges, so a read k-mer that spans an interval edge is not counted - a share of about k / interval.

What it is not:
  * an error that the reads share is supported and invisible (ONT homopolymer lengths are the main case);
  * a true k-mer in a coverage hole is counted as an error;
  * with noisy reads and --min_count 1 an error k-mer can be carried by a chance read error: the figure is an upper bound of
    the true QV, and <o>_kmer_qv.hist.tsv is the evidence for a larger --min_count;
  * it compares assemblies on the same reads; it does not replace `assess` where a truth exists;
  * no value of --min_count is recommended.

--completeness asks the other question: which of the reads' k-mers the assembly lacks (Merqury's completeness; the rule: the
second k-mer section of include/pepper_hip.h). The same reads, the same clipping; a read k-mer the assembly does not hold goes
into a reads-only hash table on the device (--read_table_mb), part by part where the table cannot hold all of them (--passes,
the reads streamed again for every part). With noisy reads the error k-mers dominate the reads-only side at low counts: the
whole curve over the threshold is written, and it is read past them.
"""
import concurrent.futures
import math
import os
import sys
import time
from typing import List, Sequence, Tuple

import numpy as np

from .assess import log, read_fasta, upper, write_text

MAX_ASSEMBLY = 1 << 31
MAX_BATCH_BASES = 1 << 31
CAP = 1 << 30
READ_LIMIT = 1 << 40        # the reader's read limit per interval: never reached, so no read is dropped
CONTIG_HEADER = "#name\tlength\tkmers\tsupported\tunsupported\tno_key\terror_rate\tQV\n"
SEGMENT_HEADER = "#name\tstart\tend\tunsupported\n"
RUNS_HEADER = "#name\tstart\tend\tkmers\tcore_start\tcore_end\n"
HIST_HEADER = "#count\tkmers\n"
SPECTRUM_HEADER = "#count\treads_only\tasm_x1\tasm_x2\tasm_x3\tasm_x4plus\n"
COMPLETENESS_HEADER = "#solid\tread_kmers\tin_assembly\tcompleteness\n"
READS_HEAD_BYTES, READS_SLOT_BYTES, READS_MIN_SLOTS, MAX_PASSES = 256, 12, 1024, 4096
MAX_READ_TABLE_MB = float(1 << 20)


class KmerQvError(ValueError):
    """what the command refuses (exit status 2)"""


def check_options(k: int, min_count: int, segment: int, interval: int) -> None:
    if not (11 <= k <= 31 and k % 2 == 1):
        raise KmerQvError("-k %d: must be odd in [11, 31]" % k)
    if not 1 <= min_count <= CAP:
        raise KmerQvError("--min_count %d: must lie in [1, 2^30]" % min_count)
    if not (32 <= segment <= 65536 and segment % 32 == 0):
        raise KmerQvError("--segment %d: must be a multiple of 32 in [32, 65536]" % segment)
    if interval < 1000:
        raise KmerQvError("--interval %d: must be at least 1000" % interval)


def read_slots(read_table_mb: float) -> int:
    """the largest power of two of slots whose reads-only table (a 256-byte head, 12 bytes per slot) fits in --read_table_mb"""
    mb = float(read_table_mb)
    if not (mb == mb and 0 < mb <= MAX_READ_TABLE_MB):
        raise KmerQvError("--read_table_mb %s: must lie in (0, 2^20]" % read_table_mb)
    fit = (int(mb * (1 << 20)) - READS_HEAD_BYTES) // READS_SLOT_BYTES
    if fit < READS_MIN_SLOTS:
        raise KmerQvError("--read_table_mb %s: the smallest table, %d slots, needs %d bytes" % (
            read_table_mb, READS_MIN_SLOTS, READS_HEAD_BYTES + READS_SLOT_BYTES * READS_MIN_SLOTS))
    return 1 << (fit.bit_length() - 1)


def check_completeness_options(completeness: bool, read_table_mb, passes, solid) -> Tuple[int, int, int]:
    """-> (slots, passes, solid), the defaults 1024 MB, 1 pass, solid 2 filled in; the three options belong to --completeness"""
    if not completeness:
        for name, v in (("--read_table_mb", read_table_mb), ("--passes", passes), ("--solid", solid)):
            if v is not None:
                raise KmerQvError("%s is an option of --completeness" % name)
        return 0, 1, 2
    passes = 1 if passes is None else int(passes)
    solid = 2 if solid is None else int(solid)
    if not 1 <= passes <= MAX_PASSES:
        raise KmerQvError("--passes %d: must lie in [1, %d]" % (passes, MAX_PASSES))
    if not 1 <= solid <= 255:
        raise KmerQvError("--solid %d: must lie in [1, 255]" % solid)
    return read_slots(1024 if read_table_mb is None else read_table_mb), passes, solid


def error_qv(kmers: int, supported: int, k: int) -> Tuple[str, str]:
    """error_rate = 1 - (supported / kmers)^(1/k), QV = -10 log10(error_rate): `.` without a k-mer, `inf` without an
    unsupported one; the QV formatted as assess.identity_qv formats its own"""
    if kmers == 0:
        return ".", "."
    if supported == kmers:
        return "%.3e" % 0.0, "inf"
    e = 1.0 - (supported / kmers) ** (1.0 / k)
    return "%.3e" % e, "%.2f" % (-10.0 * math.log10(e) + 0.0)


def run_core(first: int, last: int, k: int):
    """the bases every k-mer of the run [first, last] covers: [last, first + k), or None where that is empty (a run longer
    than k). A lone substitution at p gives the run [p - k + 1, p] and the core [p, p + 1)."""
    return (last, first + k) if last < first + k else None


def contig_text(names: Sequence[str], lengths: Sequence[int], ctg: np.ndarray, k: int) -> Tuple[str, Tuple[int, int]]:
    """-> (<o>_kmer_qv.tsv, (unsupported k-mers, k-mers) of TOTAL)"""
    out = [CONTIG_HEADER]
    rows = [(n, ln, int(c[0]), int(c[1]), int(c[2])) for n, ln, c in zip(names, lengths, ctg)]
    rows.append(("TOTAL", sum(lengths), int(ctg[:, 0].sum()), int(ctg[:, 1].sum()), int(ctg[:, 2].sum())))
    for name, ln, keyed, unsup, no_key in rows:
        out.append("\t".join([name, str(ln), str(keyed), str(keyed - unsup), str(unsup), str(no_key)]
                             + list(error_qv(keyed, keyed - unsup, k))) + "\n")
    return "".join(out), (rows[-1][3], rows[-1][2])


def segment_text(names, lengths, seg_off, segs, segment: int) -> str:
    out = [SEGMENT_HEADER]
    for p, (name, ln) in enumerate(zip(names, lengths)):
        for j, v in enumerate(segs[int(seg_off[p]):int(seg_off[p + 1])]):
            out.append("%s\t%d\t%d\t%d\n" % (name, j * segment, min(ln, (j + 1) * segment), int(v)))
    return "".join(out)


def runs_text(names, runs, k: int) -> str:
    out = [RUNS_HEADER]
    for p, first, last in ((int(a), int(b), int(c)) for a, b, c in runs):
        core = run_core(first, last, k)
        out.append("\t".join([names[p], str(first), str(last + k), str(last - first + 1)]
                             + ([str(core[0]), str(core[1])] if core else [".", "."])) + "\n")
    return "".join(out)


def hist_text(hist) -> str:
    """count, number of assembly k-mers with that count (the last line: that count or more)"""
    last = len(hist) - 1
    return HIST_HEADER + "".join("%s\t%d\n" % (c if c < last else "%d+" % last, int(v)) for c, v in enumerate(hist))


def completeness_at(ro_hist, spectrum, s: int) -> Tuple[int, int, str]:
    """-> (read k-mers seen s times or more, those of them in the assembly, their share or `.` without any)"""
    found = int(np.asarray(spectrum)[:, s:].sum())
    total = found + int(np.asarray(ro_hist)[s:].sum())
    return total, found, ("%.6f" % (found / total)) if total else "."


def spectrum_text(ro_hist, spectrum) -> str:
    """count, the distinct read k-mers the assembly lacks with that count, the assembly's distinct k-mers with that count that
    it holds once, twice, three times, four times or more (the last line: that count or more)"""
    last = len(ro_hist) - 1
    return SPECTRUM_HEADER + "".join("%s\t%d\t%s\n" % (c if c < last else "%d+" % last, int(ro_hist[c]),
                                                      "\t".join(str(int(row[c])) for row in spectrum)) for c in range(last + 1))


def completeness_text(ro_hist, spectrum) -> str:
    """the whole curve: one line for every threshold that leaves a read k-mer"""
    out = [COMPLETENESS_HEADER]
    for s in range(1, len(ro_hist)):
        total, found, share = completeness_at(ro_hist, spectrum, s)
        if total > 0:
            out.append("%d\t%d\t%d\t%s\n" % (s, total, found, share))
    return "".join(out)


def read_intervals(contigs: Sequence[Tuple[str, int]], interval: int) -> List[Tuple[str, int, int]]:
    """every contig cut into pieces of `interval` bases: [(name, start, end)]"""
    return [(name, s, min(s + interval, ln)) for name, ln in contigs for s in range(0, ln, interval)]


class Scorer:
    """one assembly's table on the device: built once, counted into batch by batch, summarised at the end"""

    def __init__(self, ctx, label: str, seqs: Sequence[Tuple[str, bytes]], k: int, segment: int, slots: int = 0):
        """slots > 0: a reads-only table of that many slots beside the assembly's (--completeness)"""
        import torch
        self.torch, self.ctx, self.label, self.k, self.segment = torch, ctx, label, int(k), int(segment)
        self.names, self.lengths = [n for n, _ in seqs], [len(s) for _, s in seqs]
        if sum(self.lengths) >= MAX_ASSEMBLY:
            raise KmerQvError("the %s holds %d bases: at most 2^31 - 1" % (label, sum(self.lengths)))
        a_off = np.zeros(len(seqs) + 1, np.int64)
        a_off[1:] = np.cumsum(self.lengths)
        self.n, self.N = len(seqs), int(a_off[-1])
        self.table_bytes = ctx.kmer_table_bytes(a_off)
        self.A = torch.from_numpy(np.frombuffer(b"".join(upper(s) for _, s in seqs) + b"\0", np.uint8).copy()).cuda()
        self.ao = torch.from_numpy(a_off).cuda()
        self.table = torch.empty(self.table_bytes, dtype=torch.uint8, device="cuda")
        self.bcnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.kmer_table_build_dev(self.A.data_ptr(), self.ao.data_ptr(), self.n, self.k, CAP, self.table.data_ptr(), self.table_bytes,
                                 self.bcnt.data_ptr())
        self.slots = int(slots)
        if self.slots:
            self.rtable_bytes = ctx.kmer_reads_table_bytes(self.slots)
            self.rtable = torch.empty(self.rtable_bytes, dtype=torch.uint8, device="cuda")
            self.ro_hist = torch.zeros(256, dtype=torch.int64, device="cuda")
            self.fcnt = torch.zeros(4, dtype=torch.int64, device="cuda")
            self.ro_keys = self.dropped = 0
            torch.cuda.synchronize()
            ctx.kmer_reads_table_init_dev(self.rtable.data_ptr(), self.rtable_bytes, self.slots, CAP)

    def count(self, d_bases: int, d_base_off: int, n_reads: int, n_bases: int) -> None:
        self.ctx.kmer_count_reads_dev(self.table.data_ptr(), self.table_bytes, d_bases, d_base_off, n_reads, n_bases)

    def count_all(self, d_bases: int, d_base_off: int, n_reads: int, n_bases: int, part: int, n_parts: int) -> None:
        self.ctx.kmer_count_reads_all_dev(self.table.data_ptr(), self.table_bytes, self.rtable.data_ptr(), self.rtable_bytes, d_bases,
                                          d_base_off, n_reads, n_bases, part, n_parts)

    def flush(self) -> None:
        """after a pass: the reads-only table into ro_hist, emptied for the next part; a full table is refused"""
        from . import _ffi
        self.ctx.kmer_reads_flush_dev(self.rtable.data_ptr(), self.rtable_bytes, self.ro_hist.data_ptr(), self.fcnt.data_ptr())
        self.ctx.synchronize()
        keys, status, dropped, _ = (int(v) for v in self.fcnt.cpu().numpy())
        self.ro_keys, self.dropped = self.ro_keys + keys, self.dropped + dropped
        if status == _ffi.PV_ERR_CAPACITY:
            raise KmerQvError("the %s's table of read k-mers is full (%d slots, %d read k-mers dropped): choose a larger "
                              "--read_table_mb or more --passes" % (self.label, self.slots, dropped))
        if status != _ffi.PV_OK:
            raise RuntimeError("kmer_qv: the %s's flush ended with device status %d" % (self.label, status))

    def spectrum(self):
        """-> (ro_hist [256], spectrum [4][256]) as numpy arrays, after the last flush"""
        from . import _ffi
        torch = self.torch
        spec, cnt = torch.zeros((4, 256), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        self.ctx.kmer_spectrum_dev(self.table.data_ptr(), self.table_bytes, spec.data_ptr(), cnt.data_ptr())
        self.ctx.synchronize()
        if int(cnt.cpu().numpy()[1]) != _ffi.PV_OK:
            raise RuntimeError("kmer_qv: the %s's spectrum ended with device status %d" % (self.label, int(cnt.cpu().numpy()[1])))
        return self.ro_hist.cpu().numpy(), spec.cpu().numpy()

    def summary(self, min_count: int):
        """-> (contig counts [n][3], seg_off, segs, runs [r][3], hist [256]) as numpy arrays"""
        from . import _ffi
        torch = self.torch
        S = sum((ln + self.segment - 1) // self.segment for ln in self.lengths)
        z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")  # noqa: E731
        ctg, seg_off, segs, hist, cnt = z(max(self.n, 1), 3), z(self.n + 1), z(max(S, 1)), z(_ffi.PV_KMER_HIST), z(8)
        capacity = 1 << 16
        for _ in (0, 1):
            runs = z(max(capacity, 1), 3)
            torch.cuda.synchronize()
            self.ctx.kmer_support_dev(self.table.data_ptr(), self.table_bytes, self.ao.data_ptr(), self.n, min_count, self.segment,
                                      ctg.data_ptr(), seg_off.data_ptr(), S, segs.data_ptr(), capacity, runs.data_ptr(), hist.data_ptr(),
                                      0, cnt.data_ptr())
            self.ctx.synchronize()
            c = cnt.cpu().numpy()
            if int(c[1]) != _ffi.PV_ERR_CAPACITY:
                break
            capacity = int(c[2])   # the one sized second call
        if int(c[1]) != _ffi.PV_OK:
            raise RuntimeError("kmer_qv: the %s's summary ended with device status %d (table status %d)"
                               % (self.label, int(c[1]), int(self.bcnt.cpu().numpy()[1])))
        return (ctg.cpu().numpy()[:self.n], seg_off.cpu().numpy(), segs.cpu().numpy()[:S], runs.cpu().numpy()[:int(c[0])],
                hist.cpu().numpy())

    def texts(self, min_count: int):
        """-> ({file suffix: text}, (unsupported k-mers, k-mers, QV) of TOTAL)"""
        ctg, seg_off, segs, runs, hist = self.summary(min_count)
        contig_txt, (unsup, kmers) = contig_text(self.names, self.lengths, ctg, self.k)
        files = {".tsv": contig_txt, ".segments.tsv": segment_text(self.names, self.lengths, seg_off, segs, self.segment),
                 ".runs.bed": runs_text(self.names, runs, self.k), ".hist.tsv": hist_text(hist)}
        return files, (unsup, kmers, error_qv(kmers, kmers - unsup, self.k)[1])

    def completeness_texts(self, solid: int):
        """-> ({file suffix: text}, completeness at `solid` or `.`)"""
        ro_hist, spec = self.spectrum()
        return ({".spectrum.tsv": spectrum_text(ro_hist, spec), ".completeness.tsv": completeness_text(ro_hist, spec)},
                completeness_at(ro_hist, spec, solid)[2])


def stream_reads(ctx, bam: str, fasta: str, intervals, scorers: Sequence[Scorer], threads: int, timers: dict = None,
                 part: Tuple[int, int] = None) -> None:
    """every interval's reads through the host reader on `threads` reader threads, a few intervals ahead of the device; each
    batch goes up with the polisher's upload call and past every scorer's table. The counts are integer sums, so neither the
    number of threads nor the order of the batches changes them. part = (p, P), with --completeness: the k-mers of part p of P
    alone, and those the assembly lacks into the scorer's reads-only table."""
    from . import bamio
    from .polish import _read_ahead, _thread_handles
    T = timers if timers is not None else {}
    for key in ("read_s", "device_s", "reads", "read_bases", "batches"):
        T.setdefault(key, 0)
    handles = _thread_handles(bam, fasta)

    def read(iv):
        t0 = time.perf_counter()
        fb = bamio.fill_batch(*handles(), [iv], 0, False, 1.0, 0, max_reads=READ_LIMIT)
        return iv, fb, time.perf_counter() - t0

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
        t0 = time.perf_counter()
        for iv, fb, _ in _read_ahead(ex, read, intervals, max(2, int(threads))):
            T["read_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            b = fb.batch
            if b.n_regions:
                n_reads, n_bases = int(b.read_off[b.n_regions]), int(b.base_off[int(b.read_off[b.n_regions])])
                if int(fb.reads_seen.sum()) != n_reads:
                    raise KmerQvError("interval %s:%d-%d: the reader dropped reads" % iv)
                if n_bases >= MAX_BATCH_BASES:
                    raise KmerQvError("interval %s:%d-%d holds %d read bases: choose a smaller --interval" % (iv + (n_bases,)))
                dev, totals, keep = ctx.upload_batch(b)
                for s in scorers:
                    if part is None:
                        s.count(dev.bases, dev.base_off, totals[0], totals[1])
                    else:
                        s.count_all(dev.bases, dev.base_off, totals[0], totals[1], part[0], part[1])
                ctx.synchronize()   # the copies out of the host batch are done: it may go, and the next may come
                del keep
                T["reads"] += n_reads
                T["read_bases"] += n_bases
                T["batches"] += 1
            fb.close()
            T["device_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
        T["read_s"] += time.perf_counter() - t0


def run(args) -> int:
    try:
        k, min_count = int(args.kmer), int(args.min_count)
        check_options(k, min_count, int(args.segment), int(args.interval))
        complete = bool(args.completeness)
        slots, passes, solid = check_completeness_options(complete, args.read_table_mb, args.passes, args.solid)
        for what, p in (("assembly FASTA", args.assembly), ("BAM", args.bam), ("draft FASTA", args.fasta)):
            if not os.path.isfile(p):
                raise KmerQvError("cannot find the %s %s" % (what, p))
        from . import bamio
        asm = read_fasta(args.assembly)
        draft = read_fasta(args.fasta) if args.draft else None
        try:
            fa, bm = bamio.FastaHandler(args.fasta), bamio.BamHandler(args.bam)
        except IOError as e:
            raise KmerQvError(str(e))
        known = set(fa.get_chromosome_names())
        contigs = [(n, fa.get_chromosome_sequence_length(n)) for n in bm.get_chromosome_sequence_names() if n in known]
        fa.close()
        bm.close()
        if not contigs:
            raise KmerQvError("no contig of the BAM is in the draft FASTA")
        from . import runtime
        ctx = runtime.Context(int(args.device_id))
        try:
            scorers = [Scorer(ctx, "assembly", asm, k, int(args.segment), slots)]
            if draft is not None:
                scorers.append(Scorer(ctx, "draft", draft, k, int(args.segment), slots))
            T = {}
            intervals = read_intervals(contigs, int(args.interval))
            if not complete:
                stream_reads(ctx, args.bam, args.fasta, intervals, scorers, int(args.threads), T)
            else:   # the passes are the outer loop: the reads are streamed again for every part
                for p in range(passes):
                    Tp = {}
                    stream_reads(ctx, args.bam, args.fasta, intervals, scorers, int(args.threads), Tp, part=(p, passes))
                    for s in scorers:
                        s.flush()
                    for key, v in Tp.items():   # the reads are the same in every pass: counted once, the times summed
                        T[key] = T.get(key, 0) + v if key.endswith("_s") else v
            results = [s.texts(min_count) for s in scorers]
            if complete:
                shares = []
                for s, (files, _) in zip(scorers, results):
                    more, share = s.completeness_texts(solid)
                    files.update(more)
                    shares.append(share)
        finally:
            ctx.close()
    except KmerQvError as e:
        sys.stderr.write("ERROR: kmer_qv: %s\n" % e)
        return 2
    d = os.path.dirname(args.output)
    if d:
        os.makedirs(d, exist_ok=True)
    for stem, (files, _) in zip(("_kmer_qv", "_kmer_qv_draft"), results):
        for suffix, text in files.items():
            write_text(args.output + stem + suffix, text)
    log("kmer_qv: %d reads, %d read bases in %d batches; reader %.2f s, device %.2f s" % (
        T["reads"], T["read_bases"], T["batches"], T["read_s"], T["device_s"]))
    unsup, kmers, qv = results[0][1]
    if draft is not None:
        dunsup, _, dqv = results[1][1]
        log("kmer_qv: unsupported k-mers %d -> %d, QV %s -> %s (draft -> assembly), k = %d, min_count = %d" % (
            dunsup, unsup, dqv, qv, k, min_count))
    else:
        log("kmer_qv: unsupported k-mers %d of %d, QV %s, k = %d, min_count = %d" % (unsup, kmers, qv, k, min_count))
    if complete:
        keys = "%d distinct read k-mers the assembly lacks in %d slots, %d pass%s" % (
            scorers[0].ro_keys, slots, passes, "" if passes == 1 else "es")
        if draft is not None:
            log("kmer_qv: completeness %s -> %s (draft -> assembly) at --solid %d; %s" % (shares[1], shares[0], solid, keys))
        else:
            log("kmer_qv: completeness %s at --solid %d; %s" % (shares[0], solid, keys))
    return 0
