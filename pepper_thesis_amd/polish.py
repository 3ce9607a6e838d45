"""`polish`: BAM + draft FASTA -> polished FASTA, with every stage on the device.

The reference's product (pepper/modules/python/polish.py:14-117) runs make_images -> call_consensus -> stitch through image and
prediction HDF5 files. Here each batch of regions goes through

  region_from_files (reader threads) [-> pv_polish_realign_dev] -> pv_polish_summarize_regions_dev -> pv_rnn_forward_p2_dev
  -> pv_polish_stitch_dev

without leaving HBM; only the region offsets and the polished bases (one byte per base) come back to the host.

  python -m pepper_thesis_amd polish -b reads.bam -f draft.fa -m model.pkl -o out/polished [-t 5] [-r ctg:start-end] [--bf16]
      [--realign] [--gpu_decode] [--qualities] [--edits [--evidence]] [--min_depth N] [--min_qual Q] [--min_support K] [-hp]
  python -m pepper_thesis_amd polish -b reads.bam -f draft.fa --vote [--runs [--min_run N]] -o out/polished [the same flags but -m and --bf16]

--gpu_decode (opt-in) replaces the first stage: reader threads only plan blocks and fetch draft bytes, and the BAM is inflated,
decoded and clipped on the device (gpu_decode.py; _decoded_pieces below). Same FASTA.

--qualities (opt-in, one device) also writes `<o>/_pepper_polished.fq`: the same contigs and sequences with one Phred byte
per base. The chain then keeps P2's accumulated softmax, turns it into row qualities (pv_polish_row_qual_dev, the rule in
include/pepper_hip.h: what predict_distributed_gpu.py:96-105 means to store, and Stitch.py:39-91 means to string up with
`+33` and `base != 0`, both commented out there) and stitches them beside the bases (pv_polish_stitch_qual_dev); one more
byte per base comes back. The FASTA is byte for byte the one of a run without the flag.

--edits (opt-in, one device) also writes `<o>/_pepper_polished.edits.vcf.gz` and its tabix index: what the polisher changed
in the draft. Behind the stitch, on the same stream, pv_polish_edits_dev compares the labels of the columns the stitch
consults with the draft bytes of the batch and leaves one 16-byte record per substitution, deletion or inserted base (with
--qualities: with the column's row quality); the region offsets and the records come back, and polish_edits.py joins them
into VCF records per contig. The FASTA (and FASTQ) are byte for byte those of a run without the flag.

--evidence (opt-in, one device, needs --edits) gives every VCF record its read support. The builder also hands out the depth and
the ten raw counts of every chunk row (pv_polish_out.depth, .counts), pv_polish_edits_evidence_dev runs in place of the edits
call and leaves one 8-byte record beside every edit record (depth, reads that spell the draft, reads that spell the edit on
either strand; the rule is in include/pepper_hip.h), 8 more bytes per edit come back, and polish_edits.py writes the numbers
of each record's weakest column as INFO (DP, AD, SAF, SAR). FASTA, FASTQ and the other VCF columns are byte for byte those of
a run without the flag.

--min_depth N (opt-in, one device; 0 = off) keeps the draft wherever fewer than N reads stand behind a column. The builder
also hands out the read depth of every chunk row (pv_polish_out.depth), and between the network (and the row qualities) and
the stitch pv_polish_mask_low_depth_dev rewrites, in place, the labels of the rows below N to the ones that spell the draft
(insert rows: no base) and their qualities to 0; a draft byte other than ACGT cannot be spelled and keeps the network's
label. Stitch, qualities and edits then agree without knowing of it. A region without reads gives no chunks, so with N >= 1
it gets a piece of its own: the upper-cased draft of its kept range, quality 0, no edits; the FASTA then keeps the draft's
coordinates wherever nothing was polished, and the edits VCF carries one ##pepper_min_depth=N line in place of the
##pepper_no_reads lines. Without the flag no output changes by a byte. The reference has no counterpart.

--min_qual Q (opt-in, one device; 0 = off, 0..94) changes the draft only where the network is sure. The row qualities are
computed whether or not --qualities is given, and behind the mask and before the stitch pv_polish_filter_low_qual_dev takes
back, in place, every run of adjacent edited columns whose lowest quality is below Q: an edit is applied whole or not at all
(the rule is in include/pepper_hip.h). A run over a draft byte other than ACGT cannot be spelled and stays. Stitch, qualities
and edits then agree without knowing of it, every VCF record has QUAL >= Q, and the VCF carries one ##pepper_min_qual=Q line.
Without the flag no output changes by a byte. The reference has no counterpart, and no Q is recommended.

--min_support K (opt-in, one device; 0 = off, 0..65535) never changes the draft to something fewer than K reads show. The
builder also hands out the depth and the ten raw counts of every chunk row (as for --evidence), and behind the quality filter
and before the stitch pv_polish_filter_low_support_dev takes back, in place, every run of adjacent edited columns whose
weakest column is spelled by fewer than K reads (alt_fwd + alt_rev of the evidence rule; include/pepper_hip.h). A run over a
draft byte other than ACGT cannot be spelled and stays. Stitch, qualities and edits then agree without knowing of it, every
VCF record written with --evidence has AD's second number >= K, and the VCF carries one ##pepper_min_support=K line. It needs
none of --edits, --qualities and --evidence. --min_support 1 means "no edit without a read behind it"; no larger K is
recommended. Without the flag no output changes by a byte. The reference has no counterpart.

-hp / --use_hp_info (opt-in, one device) writes one polished sequence per haplotype, `<o>/_pepper_polished_hp1.fa` and
`_hp2.fa` (with --qualities / --edits their `_hp1` / `_hp2` forms; the un-suffixed files are not written). A launch is read,
decoded and uploaded once; then for h in (1, 2) pv_batch_select_hp_dev compacts the batch on the device to the reads whose HP
tag is 0 or h (the rule is in include/pepper_hip.h) and the chain above runs on that batch, from the realigner on, with its
kernels unchanged and its buffers reused. The selection's counters and read_off come back: a region left without reads for h
gives no piece for h (with --min_depth it is filled from the draft), as a region without reads gives none. A launch in which
no read is tagged runs the chain once for both. Each haplotype's files are those of a plain run on a BAM holding only the
untagged reads and those of the haplotype. The edits VCF carries one ##pepper_haplotype=h line.

--vote (opt-in, one device; in place of -m and --bf16) polishes without a model. The builder also hands out the depth and the
ten raw counts of every chunk row (as for --evidence), and where pv_rnn_forward_p2_dev stands pv_polish_vote_dev writes the
same two planes from them: the label most reads of the row spell (ties go to the draft; a deletion must be strictly ahead;
the rule is in include/pepper_hip.h) and, where qualities are wanted, the fraction of the reads behind each label, so that
a row's quality is the Phred value of the fraction of reads that disagree with the winner. Everything behind it runs
unchanged, so every other flag works with it, and under -hp each haplotype votes with its own reads. A column without reads
keeps the draft; over a draft byte other than ACGT it leaves the sequence, since no label spells it. The log counts the rows
changed and the rows without reads, and the edits VCF carries one ##pepper_consensus=vote line. It is the floor a trained
model is compared with, not a replacement: a majority cannot mend systematic read errors such as homopolymer lengths.
Without the flag no output changes by a byte. The reference has no counterpart.

--vote --runs [--min_run N] (opt-in, one device, behind --vote only; N in 2..48, default 3; not with --min_support, whose
promise is per column) also votes the length of every homopolymer run of the draft read by read: directly behind the column
vote pv_polish_vote_runs_dev takes the batch the builder was given (realigned under --realign, one haplotype's under -hp),
lets every read that spans a run and holds nothing but its letter between the flanks vote its length, and where more than
half of the spanning reads vote rewrites the run's rows to the most frequent length (ties keep the draft's; the rule is in
include/pepper_hip.h). It mends what a column vote cannot: left-aligned deletions piling up in a correct run's first column,
an inserted base spread over several anchors. A miscall most reads share stays wrong; runs above 48 bases and adjacent runs
are left alone. The --evidence numbers stay the column's own counts. The log counts the runs seen, decided, changed and
skipped, and the edits VCF carries ##pepper_consensus=vote+runs and ##pepper_min_run=N. Without the flag no output changes by
a byte.

Semantics kept from the reference:
  * regions: ImageGenerationUI.py:257-273 - for pos in range(start, end, 1000): [max(start, pos-100), min(end, pos+1100)],
    the interval clamped to [0, contig_len-1] (polish_intervals);
  * reads per region: polish_summary.region_from_files (a region without reads gives no chunks);
  * --realign: every read realigned to draft [start, end + 20) first (AlignmentSummarizer.py:159-177, 327-331; the
    reference always does it; off by default here for now);
  * stitch: Stitch.py:37-128 (pv_polish_stitch_dev, include/pepper_hip.h);
  * output: perform_stitch.py:43-84 - one record per contig with a non-empty sequence, contigs in natural-key order, each
    sequence on one line, at handle_output_directory(-o) + '_pepper_polished.fa' (ImageGenerationUI.py:68-80: -o is made a
    directory, so `-o out/polished` writes `out/polished/_pepper_polished.fa`).
-g and -w are accepted and ignored (there is no CPU path; no DataLoader; -g alone means one device). -d_ids with one id picks
the device. -d_ids with several ids (up to 16, repeats allowed) starts one rank per id in fresh child processes
(polish_rank.py, as the reference's call_consensus starts one caller per device id): rank r polishes regions i % world == r
on device ids[r] and rank 0 writes the one FASTA; -t is the total of reader threads over the ranks. A bare WORLD_SIZE > 1
launch of `polish` (torchrun without this parent) is refused.
"""
import collections
import concurrent.futures
import dataclasses
import itertools
import os
import re
import sys
import time
from datetime import datetime
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _ffi

MAX_SIZE = 1000            # ImageGenerationUI.py:249-252 (inference and training alike)
MIN_IMAGE_OVERLAP = 100    # ImageSizeOptions.MIN_IMAGE_OVERLAP (pepper/modules/python/Options.py:10)
HIDDEN_SIZE = 128          # the only polisher shape the kernels implement (TrainOptions, Options.py:19-20)
GRU_LAYERS = 1


def log(msg):
    sys.stderr.write("[" + datetime.now().strftime("%m-%d-%Y %H:%M:%S") + "] INFO: " + msg + "\n")
    sys.stderr.flush()


def natural_key(s: str):
    """perform_stitch.py:11-13"""
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]


def polish_intervals(contig_len: int, start: Optional[int] = None, end: Optional[int] = None) -> List[Tuple[int, int]]:
    """the regions of one contig (ImageGenerationUI.py:257-273); inclusive [start, end] pairs"""
    if start is None:
        a, b = 0, contig_len - 1
    else:
        a, b = max(0, int(start)), min(int(end), contig_len - 1)
    return [(max(a, p - MIN_IMAGE_OVERLAP), min(b, p + MAX_SIZE + MIN_IMAGE_OVERLAP)) for p in range(a, b, MAX_SIZE)]


def output_fasta_path(output_prefix: str) -> str:
    """handle_output_directory (ImageGenerationUI.py:68-80) then perform_stitch.py:53; creates the directory"""
    d = output_prefix if output_prefix.endswith("/") else output_prefix + "/"
    os.makedirs(d, exist_ok=True)
    return d + "_pepper_polished.fa"


def load_polish_model(model_path: str) -> dict:
    """the polisher checkpoint (ModelHander.py:80-110: torch.save dict with model_state_dict, hidden_size, gru_layers, keys
    possibly 'module.'-prefixed) or an .npz of the state dict -> numpy state dict for Context.load_p2"""
    if model_path.endswith(".npz"):
        with np.load(model_path, allow_pickle=False) as z:
            sd = {k: z[k] for k in z.files}
        hidden, layers = HIDDEN_SIZE, GRU_LAYERS
    else:
        import torch
        ckpt = torch.load(model_path, map_location="cpu", weights_only=True)
        if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
            hidden, layers = int(ckpt.get("hidden_size", HIDDEN_SIZE)), int(ckpt.get("gru_layers", GRU_LAYERS))
            sd = ckpt["model_state_dict"]
        else:
            hidden, layers, sd = HIDDEN_SIZE, GRU_LAYERS, ckpt
        sd = {k: v.detach().cpu().numpy() for k, v in sd.items()}
    if hidden != HIDDEN_SIZE or layers != GRU_LAYERS:
        raise ValueError("polisher model with hidden_size=%d, gru_layers=%d: the kernels implement hidden_size=%d, gru_layers=%d only"
                         % (hidden, layers, HIDDEN_SIZE, GRU_LAYERS))
    sd = {(k[7:] if k.startswith("module.") else k): np.asarray(v, dtype=np.float32) for k, v in sd.items()}
    shape = sd.get("gru_encoder.weight_hh_l0", np.zeros(0)).shape
    if shape != (3 * HIDDEN_SIZE, HIDDEN_SIZE):
        raise ValueError("polisher model: gru_encoder.weight_hh_l0 has shape %s, expected (%d, %d)" % (shape, 3 * HIDDEN_SIZE, HIDDEN_SIZE))
    return sd


def output_fastq_path(fasta_path: str) -> str:
    """the FASTQ of --qualities lies beside the FASTA: ..._pepper_polished.fa -> ..._pepper_polished.fq"""
    assert fasta_path.endswith(".fa"), fasta_path
    return fasta_path[:-3] + ".fq"


def write_fastq(path: str, seqs: Dict[str, bytes], quals: Dict[str, bytes]) -> None:
    """one four-line record `@name / seq / + / qual+33` per contig with a non-empty sequence, in write_fasta's order; quals
    hold raw Phred bytes 0..93. Written under a temporary name and renamed."""
    tmp = path + ".partial"
    try:
        with open(tmp, "wb") as fh:
            for contig in sorted(seqs, key=natural_key):
                if seqs[contig]:
                    q = np.frombuffer(quals[contig], np.uint8)
                    if len(q) != len(seqs[contig]) or (len(q) and int(q.max()) > 93):
                        raise ValueError("contig %s: %d qualities (max %d) for %d bases" % (contig, len(q), int(q.max(initial=0)),
                                                                                            len(seqs[contig])))
                    fh.write(b"@" + contig.encode() + b"\n" + seqs[contig] + b"\n+\n" + (q + 33).astype(np.uint8).tobytes() + b"\n")
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except FileNotFoundError:
            pass
        raise


def write_fasta(path: str, seqs: Dict[str, bytes]) -> None:
    with open(path, "w") as fh:
        for contig in sorted(seqs, key=natural_key):
            if seqs[contig]:
                fh.write(">" + contig + "\n" + seqs[contig].decode() + "\n")


class Work(NamedTuple):
    """one region of a run: its place in the run's region list, the -r / contig entry it belongs to, the inclusive interval"""
    index: int
    contig_index: int
    contig: str
    start: int
    end: int


def polish_work(fasta, bam, region: Optional[str]) -> Tuple[List[Work], int]:
    """the regions of a run in contig order (the list every rank derives alike) and the draft bases they cover"""
    work, bases_in = [], 0
    for ci, (contig, s, e) in enumerate(_contig_list(fasta, bam, region)):
        ivs = polish_intervals(fasta.get_chromosome_sequence_length(contig), s, e)
        work += [Work(len(work) + k, ci, contig, a, b) for k, (a, b) in enumerate(ivs)]
        bases_in += ivs[-1][1] - ivs[0][0] + 1 if ivs else 0   # draft bases covered (the regions overlap)
    return work, bases_in


@dataclasses.dataclass(frozen=True)
class ChainOptions:
    """the opt-in stages a chain is made for: the one place that lists them (False / 0: off; the module docstring has each
    flag's rule). A set no chain is made for is refused here."""
    qualities: bool = False   # --qualities: the result's qual
    edits: bool = False       # --edits: the result's edit_off and edits
    evidence: bool = False    # --evidence (needs edits): the result's evidence
    min_depth: int = 0        # --min_depth N: the result's masked
    min_qual: int = 0         # --min_qual Q: the result's filtered
    min_support: int = 0      # --min_support K: the result's supported
    use_hp: bool = False      # -hp: run / run_decoded give a HapChainResult
    vote: bool = False        # --vote: the result's voted; the context needs no weights
    vote_runs: int = 0        # --vote --runs: min_run >= 2 (needs vote, takes no min_support); the result's runs
    checked: dataclasses.InitVar[bool] = True   # False: from_args, whose caller refuses a bad set in the command's words first

    def __post_init__(self, checked):
        for f in dataclasses.fields(self):
            object.__setattr__(self, f.name, type(f.default)(getattr(self, f.name)))
        if checked:
            self.check()

    def check(self) -> None:
        if self.vote_runs and not self.vote:
            raise ValueError("a chain with vote_runs needs vote: the run vote rewrites the rows the column vote left")
        if self.vote_runs and self.min_support:
            raise ValueError("a chain with vote_runs takes no min_support: that filter's promise is per column")
        if self.evidence and not self.edits:
            raise ValueError("a chain with evidence needs edits: the evidence records stand beside the edit records")

    @classmethod
    def from_args(cls, args) -> "ChainOptions":
        """the set a `polish` namespace asks for (one not made by cli.polish_parser may lack any flag), not yet checked"""
        def flag(name, default=False):
            return getattr(args, name, default) or default
        return cls(flag("qualities"), flag("edits"), flag("evidence"), flag("min_depth", 0), flag("min_qual", 0),
                   flag("min_support", 0), flag("use_hp_info"), flag("vote"), flag("min_run", 3) if flag("runs") else 0, checked=False)

    def keywords(self) -> dict:
        """only the options that are set: what open_chain, a chain's constructor and polish_fused are called with, so that a
        stub chain keeps its narrow signature"""
        return {k: v for k, v in dataclasses.asdict(self).items() if v}

    @property
    def want_counts(self) -> bool:
        """the builder also hands out the ten raw counts of every chunk row (and then their depth)"""
        return self.evidence or self.min_support > 0 or self.vote

    @property
    def want_depth(self) -> bool:
        return self.min_depth > 0 or self.want_counts

    @property
    def want_row_qual(self) -> bool:
        """the row qualities are computed: for the outputs, or (min_qual alone) for the quality filter only"""
        return self.qualities or self.min_qual > 0


class Pass(NamedTuple):
    """one pass of the chain that leaves counters on the device and counts in the result"""
    attr: str                   # the ChainResult attribute that carries its counts; with_<attr>() sets it
    option: str                 # the ChainOptions field that switches it on (> 0)
    timers: Tuple[str, ...]     # the timer key of every entry of the counts
    counters: str               # the chain's int64 device tensor: {., status, first bad chunk, ...}
    n_counters: int
    pick: Tuple[int, ...]       # where every entry of the counts stands in the counters
    noun: str                   # "polisher <noun>: device status ..."
    in_place: Optional[str]     # the context's call, for a pass that rewrites the labels in place before the stitch
    report: str                 # the command's log line, filled from the options and the timers

    @property
    def empty(self) -> tuple:
        """the counts of a launch without chunks"""
        return (0,) * len(self.timers)


# The count-carrying passes, in the order their status is read back (the first bad one is reported); the in-place ones are
# launched in this order too, behind the votes, which stand in the network's place. Timers, the no-chunk result, the status
# read-back, the log lines and ChainResult's extra planes all follow from here: a new pass is one row.
PASSES = (
    # (rows that kept the draft, rows that could not: draft byte not ACGT)
    Pass("masked", "min_depth", ("masked_rows", "unmaskable_rows"), "mask_counts", 4, (0, 3), "minimum depth",
         "polish_mask_low_depth_dev",
         "MIN DEPTH %(min_depth)d: %(masked_rows)d CHUNK ROWS KEPT THE DRAFT, %(unmaskable_rows)d COULD NOT (DRAFT BYTE NOT ACGT), "
         "%(draft_regions)d REGIONS WITHOUT READS FILLED FROM THE DRAFT"),
    # (rows of edits taken back, rows of pinned runs below the threshold: draft byte not ACGT)
    Pass("filtered", "min_qual", ("reverted_rows", "pinned_rows"), "filter_counts", 4, (0, 3), "minimum quality",
         "polish_filter_low_qual_dev",
         "MIN QUAL %(min_qual)d: %(reverted_rows)d CHUNK ROWS OF EDITS TAKEN BACK, %(pinned_rows)d ROWS OF LOW RUNS KEPT (DRAFT BYTE "
         "NOT ACGT)"),
    # (rows of edits taken back, rows of pinned runs below the minimum)
    Pass("supported", "min_support", ("unsupported_rows", "pinned_unsupported_rows"), "support_counts", 4, (0, 3),
         "minimum support", "polish_filter_low_support_dev",
         "MIN SUPPORT %(min_support)d: %(unsupported_rows)d CHUNK ROWS OF EDITS TAKEN BACK, %(pinned_unsupported_rows)d ROWS OF WEAK "
         "RUNS KEPT (DRAFT BYTE NOT ACGT)"),
    # (rows whose winner is not what the draft holds, base rows without reads)
    Pass("voted", "vote", ("voted_rows", "no_read_rows"), "vote_counts", 4, (0, 3), "vote", None,
         "VOTE: %(voted_rows)d CHUNK ROWS WHERE THE READS' MAJORITY IS NOT THE DRAFT, %(no_read_rows)d BASE ROWS WITHOUT READS (THE "
         "DRAFT IS KEPT, OR DROPPED WHERE ITS BYTE IS NOT ACGT)"),
    # (candidate runs seen, runs decided, decided runs whose length changes, candidates skipped as adjacent)
    Pass("runs", "vote_runs", ("runs_seen", "runs_decided", "runs_changed", "runs_skipped"), "runs_counts", 6, (4, 0, 3, 5),
         "run vote", None,
         "RUNS (MIN RUN %(vote_runs)d): %(runs_seen)d CANDIDATE RUNS SEEN, %(runs_decided)d DECIDED BY THEIR READS, %(runs_changed)d "
         "OF THEM WITH A LENGTH THAT IS NOT THE DRAFT'S, %(runs_skipped)d SKIPPED AS ADJACENT"),
)
PASS_TIMERS = tuple(k for p in PASSES for k in p.timers)
# what a ChainResult may carry beside its five planes: every pass's counts, and --evidence's polish_edits.EVIDENCE_DTYPE
# records, evidence[i] beside edits[i]
RESULT_EXTRAS = tuple(p.attr for p in PASSES) + ("evidence",)


class ChainResult(NamedTuple):
    """what a chain's run / run_decoded give for one batch of regions. A plane the chain was not made for is None. The
    RESULT_EXTRAS are attributes (None here), not tuple fields, so the record keeps its five planes for everything that
    unpacks it; with_masked() and its kin give a result that carries one."""
    region_off: np.ndarray                 # int64 [n_regions+1] into bases and qual
    bases: object                          # anything sliceable by region_off: polished bases, or make_images' chunk list
    qual: Optional[bytes] = None           # --qualities: one raw Phred byte per base
    edit_off: Optional[np.ndarray] = None  # --edits: int64 [n_regions+1] into edits
    edits: Optional[np.ndarray] = None     # --edits: polish_edits.EDIT_DTYPE records

    def region(self, g: int) -> tuple:
        """region g's share: (bases, qual or None, edits or None), and behind them its evidence records where the result
        carries any"""
        a, b = self.region_off[g], self.region_off[g + 1]
        share = (self.bases[a:b], None if self.qual is None else self.qual[a:b],
                 None if self.edits is None else self.edits[self.edit_off[g]:self.edit_off[g + 1]])
        return share if self.evidence is None else share + (self.evidence[self.edit_off[g]:self.edit_off[g + 1]],)


for _name in RESULT_EXTRAS:
    setattr(ChainResult, _name, None)


class HapChainResult(NamedTuple):
    """what a chain made with use_hp gives for one batch of regions: a ChainResult per haplotype, 1 then 2"""
    results: tuple     # (ChainResult of haplotype 1, of haplotype 2)
    has_reads: tuple   # per haplotype: bool [n_regions], False where the selection left the region without reads
    tags: tuple        # (reads, untagged, HP1, HP2, other values) of the batch: batch_select.tag_counts
    payload: int = 0   # bytes of bases, qualities and cigar words the two selections read and wrote (0: nothing was selected)


HP_TIMERS = ("hp_reads", "hp_untagged", "hp_1", "hp_2", "hp_other")   # and hp_payload_bytes


def hp_path(path: str, haplotype: int) -> str:
    """..._pepper_polished.fa -> ..._pepper_polished_hp<h>.fa"""
    assert path.endswith(".fa"), path
    return "%s_hp%d.fa" % (path[:-3], haplotype)


class _MaskedChainResult(ChainResult):
    """a ChainResult with the RESULT_EXTRAS as instance attributes"""


def _with(res: ChainResult, name: str, value) -> ChainResult:
    """res, carrying `value` in its attribute `name` and every other extra it carried"""
    out = _MaskedChainResult(*res)
    for k in RESULT_EXTRAS:
        setattr(out, k, value if k == name else getattr(res, k))
    return out


def with_masked(res: ChainResult, masked: Tuple[int, int]) -> ChainResult:
    """res, carrying the counts of a minimum-depth chain in its attribute `masked`"""
    return _with(res, "masked", (int(masked[0]), int(masked[1])))


def with_filtered(res: ChainResult, filtered: Tuple[int, int]) -> ChainResult:
    """res, carrying the counts of a minimum-quality chain in its attribute `filtered`"""
    return _with(res, "filtered", (int(filtered[0]), int(filtered[1])))


def with_supported(res: ChainResult, supported: Tuple[int, int]) -> ChainResult:
    """res, carrying the counts of a minimum-support chain in its attribute `supported`"""
    return _with(res, "supported", (int(supported[0]), int(supported[1])))


def with_voted(res: ChainResult, voted: Tuple[int, int]) -> ChainResult:
    """res, carrying the counts of a vote chain in its attribute `voted`"""
    return _with(res, "voted", (int(voted[0]), int(voted[1])))


def with_runs(res: ChainResult, runs: Tuple[int, int, int, int]) -> ChainResult:
    """res, carrying the counts of a run-vote chain in its attribute `runs`"""
    return _with(res, "runs", tuple(int(v) for v in runs))


def with_evidence(res: ChainResult, evidence: np.ndarray) -> ChainResult:
    """res, carrying the evidence records of an evidence chain (one per edit record) in its attribute `evidence`"""
    assert res.edits is not None and len(evidence) == len(res.edits), (len(evidence), res.edits is None)
    return _with(res, "evidence", evidence)


class Piece(NamedTuple):
    """one region with reads after the chain: its Work's contig, start and index, and its share of the ChainResult"""
    contig: str
    start: int
    index: int
    bases: object
    qual: Optional[bytes] = None
    edits: Optional[np.ndarray] = None
    # --evidence: one polish_edits.EVIDENCE_DTYPE record beside every edit record. Not a tuple field, as ChainResult's
    # counts are none: the piece keeps its six for everything that builds or unpacks it; piece_of() attaches it
    evidence = None


class _EvidencePiece(Piece):
    """a Piece with the instance attribute `evidence`"""


def piece_of(w, share: tuple) -> Piece:
    """the Piece of Work w from its share of a ChainResult (ChainResult.region): (bases, qual, edits[, evidence])"""
    if len(share) == 3:
        return Piece(w.contig, w.start, w.index, *share)
    out = _EvidencePiece(w.contig, w.start, w.index, *share[:3])
    out.evidence = share[3]
    return out


def merge_pieces(pieces, part: int = 3) -> Dict[str, bytes]:
    """pieces (Piece, or plain (contig, region start, region index, bytes) tuples), in any order -> one string per contig
    of their entry `part` (3: the bases, 4: the qualities): the regions in start order (create_consensus_sequence; their
    kept ranges are disjoint, so this is the reference's string), equal starts (a region listed twice by -r) in
    region-list order"""
    by: Dict[str, list] = {}
    for p in pieces:
        contig, start, index = p[:3]
        by.setdefault(contig, []).append((start, index, p[part]))
    return {c: b"".join(s for _, _, s in sorted(v, key=lambda t: (t[0], t[1]))) for c, v in by.items()}


def write_polished_fasta(path: str, pieces) -> Dict[str, bytes]:
    """merge_pieces, then the FASTA (perform_stitch.py:43-84); -> the sequences"""
    seqs = merge_pieces(pieces)
    write_fasta(path, seqs)
    for c in sorted(seqs, key=natural_key):
        log("FINISHED PROCESSING %s, POLISHED SEQUENCE LENGTH: %d." % (c, len(seqs[c])))
    return seqs


def _contig_list(fasta, bam, region: Optional[str]):
    """[(contig, start|None, end|None)]: -r as make_images parses it, else the contigs common to the FASTA and the BAM"""
    from .make_images import expand_region_names, parse_region
    if region:
        return [parse_region(p) for p in expand_region_names(region)]
    in_bam = set(bam.get_chromosome_sequence_names())
    common = [n for n in fasta.get_chromosome_names() if n in in_bam]
    if not common:
        raise ValueError("no contigs common to the BAM file and the FASTA file")
    return [(n, None, None) for n in sorted(common, key=natural_key)]


class _DeviceChain:
    """device buffers of the builder -> GRU -> stitch chain, grown on demand; run / run_decoded return a ChainResult.
    qualities: P2's accumulated softmax is kept, turned into row qualities and stitched beside the bases (the result's
    qual). edits: the edit pass runs behind the stitch, with the row qualities when there are any (the result's edit_off
    and edits). min_depth >= 1: the builder also fills the depth plane and, before the stitch, the labels (and row
    qualities) of the rows below min_depth are rewritten in place to spell the draft (the result's masked). min_qual >= 1:
    the row qualities are computed whether or not the chain was made for qualities and, behind the mask and before the
    stitch, every run of adjacent edits whose lowest quality is below min_qual is taken back in place (the result's
    filtered). use_hp: run / run_decoded return a HapChainResult: the batch is selected on the device by haplotype
    (pv_batch_select_hp_dev) and everything from the realigner on runs once per haplotype on the selected reads.
    evidence (needs edits): the builder also fills the depth and the counts plane, and pv_polish_edits_evidence_dev runs in
    place of the edits call, so every edit record gets its read support (the result's evidence). min_support >= 1: the
    builder also fills the depth and the counts plane and, behind the quality filter and before the stitch, every run of
    adjacent edits whose weakest column fewer than min_support reads spell is taken back in place (the result's supported);
    it needs neither edits nor qualities nor evidence. vote: the builder also fills the depth and the counts plane and
    pv_polish_vote_dev stands where the network stands: the labels (and, where row qualities are needed, the read fractions
    in the place of the softmax sums) come from the majority of the reads of every row, and the context needs no weights (the
    result's voted). vote_runs = min_run >= 2 (needs vote): pv_polish_vote_runs_dev runs directly behind the vote with the
    batch the builder was given (realigned under --realign, one haplotype's under -hp) and rewrites the rows of every
    homopolymer run whose length the reads decide (the result's runs)."""

    def __init__(self, ctx, own_ctx: bool = False, **options):
        self.options = ChainOptions(**options)   # (refuses a bad set before the context is touched)
        for k, v in dataclasses.asdict(self.options).items():   # the chain's public attributes: qualities, edits, ...
            setattr(self, k, v)
        import torch
        self.ctx, self.dev, self.own_ctx = ctx, "cuda:%d" % ctx.device_id, own_ctx
        for p in PASSES:
            setattr(self, p.counters, torch.zeros(p.n_counters, dtype=torch.int64, device=self.dev))
        self.edit_buf = self.ev_buf = self.sel = None
        self.edit_counts = torch.zeros(4, dtype=torch.int64, device=self.dev)
        self.dout = self.labels = self.seq = None
        self.acc = self.row_qual = self.qual = None
        self.rout = None
        self.counts = torch.zeros(4, dtype=torch.int64, device=self.dev)

    def close(self):
        if self.own_ctx:
            self.ctx.close()

    def _ensure(self, chunks: int):
        import torch
        from .device import DevicePolishOut
        if self.dout is None or self.dout.capacity < chunks:
            self.dout = DevicePolishOut(chunks, device=self.dev, depth=self.options.want_depth, counts=self.options.want_counts)
            self.labels = torch.zeros((chunks, 1000), dtype=torch.uint8, device=self.dev)
            self.seq = torch.zeros(chunks * 1000, dtype=torch.uint8, device=self.dev)
            if self.options.want_row_qual:
                self.acc = torch.zeros((chunks, 1000, 5), dtype=torch.float32, device=self.dev)
                self.row_qual = torch.zeros((chunks, 1000), dtype=torch.uint8, device=self.dev)
            if self.qualities:
                self.qual = torch.zeros(chunks * 1000, dtype=torch.uint8, device=self.dev)
            if self.edits:   # one record per chunk row: capacity cannot run short
                self.edit_buf = torch.zeros((chunks * 1000, 16), dtype=torch.uint8, device=self.dev)
            if self.evidence:
                self.ev_buf = torch.zeros((chunks * 1000, 8), dtype=torch.uint8, device=self.dev)
            torch.cuda.synchronize()   # the fills ran on torch's stream; the chain runs on the context's

    def _summarize(self, db, sizes, host_batch) -> int:
        """builder on the device; -> n_chunks. sizes: (columns of all regions, regions), for the chunk estimate. A batch
        beyond the device form's workspace heuristics (PV_ERR_LIMIT: e.g. a very long insert) runs the host form on
        host_batch(), which retries with measured bounds, and its chunks are uploaded."""
        from .polish_summary import polish_summarize
        cols, n_regions = sizes
        want = (cols + cols // 2 + 1024) // 950 + 2 * n_regions + 2
        for _ in range(2):
            self._ensure(want)
            self.ctx.polish_summarize_dev(db, self.dout)
            self.ctx.synchronize()
            n, status = self.dout.n_chunks(), self.dout.status()
            if status == _ffi.PV_ERR_LIMIT:
                break
            if status != _ffi.PV_OK:
                raise _ffi.PepperHipError(status, "polisher image builder: device status %d" % status)
            if n <= self.dout.capacity:
                return n
            want = n
        import torch
        want_depth, want_counts = self.options.want_depth, self.options.want_counts
        planes = dict(want_depth=want_depth, want_counts=True) if want_counts else dict(want_depth=want_depth)
        out = polish_summarize(self.ctx, host_batch(), **planes)
        n = len(out.chunk_id)
        self._ensure(n)
        for name in ("images", "position", "index", "region", "chunk_id"):
            getattr(self.dout, name)[:n].copy_(torch.from_numpy(getattr(out, name)))
        if want_depth:
            self.dout.set_depth(out.depth)
        if want_counts:
            self.dout.set_row_counts(out.counts)
        return n

    def _realign(self, db, host_batch, qmax: int, windows):
        """reads of at most qmax bases realigned to the draft on the device -> (maker of the realigned host batch, device
        batch for the builder). The only read-back is the counters (cigar total and status); the host batch is made only
        if the builder needs its host form."""
        import torch
        from .realign import DeviceRealignOut, RealignResult, device_windows, pack_windows, realigned_batch
        woff, win = pack_windows(windows)
        d_woff, d_win = device_windows(woff, win, self.dev)
        n_reads = db.n_reads
        want = db.n_cigar + 4 * n_reads + db.n_bases // 8 + 16
        for _ in range(2):
            if self.rout is None or self.rout.n_reads < n_reads or self.rout.capacity < want:
                self.rout = DeviceRealignOut(max(n_reads, self.rout.n_reads if self.rout else 0), want, self.dev)
                torch.cuda.synchronize()   # the fills ran on torch's stream; the chain runs on the context's
            self.ctx.polish_realign_dev(db, d_woff.data_ptr(), d_win.data_ptr(), qmax, self.rout)
            self.ctx.synchronize()
            total, status, _, _ = (int(v) for v in self.rout.counts.tolist())
            if status == _ffi.PV_ERR_CAPACITY:
                want = total
                continue
            if status != _ffi.PV_OK:
                raise _ffi.PepperHipError(status, "polisher realignment: device status %d" % status)
            break
        ro = self.rout
        c = _ffi.pv_batch_in()
        for f, _ in _ffi.pv_batch_in._fields_:
            setattr(c, f, getattr(db.c, f))
        c.read_pos, c.cigar_off, c.cigar = ro.read_pos.data_ptr(), ro.cigar_off.data_ptr(), ro.cigar.data_ptr()
        rdb = _RealignedDeviceBatch(c, db, total, (d_woff, d_win))
        n = n_reads

        def host():
            res = RealignResult(ro.read_pos[:n].cpu().numpy(), ro.cigar_off[:n + 1].cpu().numpy(),
                                ro.cigar[:total].cpu().numpy().view(np.uint32), None, None, None, 0, 0)
            return realigned_batch(host_batch(), res)
        return host, rdb

    def p2_labels(self, images: np.ndarray) -> np.ndarray:
        """P2 labels uint8 [B,1000] of host images uint8 [B,1000,10] (pv_rnn_forward_p2: PV_ERR_STATE if the call was
        poisoned); the chain of `call_consensus`"""
        return self.ctx.forward_p2(images)

    def p2_labels_and_qualities(self, images: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """p2_labels plus the row qualities uint8 [B,1000] of every row (pv_polish_row_qual on the labels and the accumulated
        softmax of the same call); the chain of `call_consensus --qualities`"""
        labels, acc = self.ctx.forward_p2(images, want_acc=True)
        return labels, self.ctx.polish_row_qual(labels, acc, seq_overlap=50)

    def _build(self, db, sizes, host_batch, qmax: int, windows):
        """[realignment ->] builder -> (device batch, n_chunks); the chunks are in self.dout. sizes, host_batch: see
        _summarize; qmax: the longest read, for the realigner; windows: the realignment window of every region (--realign), else None."""
        if windows is not None:
            host_batch, db = self._realign(db, host_batch, qmax, windows)
        return db, self._summarize(db, sizes, host_batch)

    def _host_inputs(self, batch, windows):
        """_build's first four arguments for one host batch of regions, uploaded here"""
        from .device import DeviceBatch
        sizes = int((batch.ref_end - batch.ref_start + 1).sum()), batch.n_regions
        qmax = int(np.diff(batch.base_off).max()) if windows is not None and batch.n_reads else 0   # (the realigner's alone)
        return DeviceBatch(batch, self.dev), sizes, lambda: batch, qmax

    def _decoded_inputs(self, dec):
        """_build's first four arguments for a gpu_decode.DecodedBatch: the reads are on the device already, the decode is
        ordered before the chain with its event, the longest read comes from the decode, the region sizes from its plan
        (the polisher's reference bytes are one per column of the region)"""
        dec.wait_on(self.ctx)
        if not self.use_hp:
            return dec, (dec.n_ref_bytes, dec.n_regions), lambda: dec.to_host()[0], dec.qmax

        def host():   # the host copy with its tags, for the host form of the selection
            b, hp = dec.to_host()
            b.read_hp = np.ascontiguousarray(hp, np.int32)
            return b
        return dec, (dec.n_ref_bytes, dec.n_regions), host, dec.qmax

    def build(self, batch, windows=None):
        """_build for one host batch of regions"""
        return self._build(*self._host_inputs(batch, windows), windows)

    def build_decoded(self, dec, windows=None):
        """_build for a gpu_decode.DecodedBatch"""
        return self._build(*self._decoded_inputs(dec), windows)

    def run(self, batch, windows=None) -> ChainResult:
        """one batch of regions -> its ChainResult: region_off [n_regions+1], the polished bases of all its regions,
        concatenated, and the planes this chain was made for (a chain made with use_hp: a HapChainResult)"""
        if self.use_hp:
            return self._run_hp(*self._host_inputs(batch, windows), windows, batch.n_regions)
        db, n = self.build(batch, windows)
        return self._labels_and_stitch(db, n, batch.n_regions)

    def run_decoded(self, dec, windows=None) -> ChainResult:
        """run for a gpu_decode.DecodedBatch"""
        if self.use_hp:
            return self._run_hp(*self._decoded_inputs(dec), windows, dec.n_regions)
        db, n = self.build_decoded(dec, windows)
        return self._labels_and_stitch(db, n, dec.n_regions)

    def _select(self, db, haplotype: int, n_regions: int):
        """the reads of one haplotype of a device batch, compacted into the chain's selection buffers -> (device batch of
        the kept reads, its read_off on the host). The counters and read_off are read back: the builder takes the totals as
        arguments, and the regions left without reads give no piece."""
        import torch
        from .device import DeviceSelectOut, SelectedDeviceBatch
        if self.sel is None or not self.sel.fits(n_regions, db.n_reads, db.n_bases, db.n_cigar):
            old = self.sel
            self.sel = DeviceSelectOut(*(max(a, b) for a, b in zip(
                (n_regions, db.n_reads, db.n_bases, db.n_cigar),
                (old.n_regions, old.read_capacity, old.base_capacity, old.cigar_capacity) if old else (0, 0, 0, 0))),
                device=self.dev, want_src=False)
            torch.cuda.synchronize()
        self.ctx.batch_select_hp_dev(db, haplotype, self.sel)
        self.ctx.synchronize()
        kept, n_bases, n_cigar, status = (int(v) for v in self.sel.counts.tolist())
        if status != _ffi.PV_OK:   # capacity cannot run short: the buffers hold the whole batch
            raise _ffi.PepperHipError(status, "polisher haplotype selection: device status %d" % status)
        read_off = self.sel.t["read_off"][:n_regions + 1].cpu().numpy()
        return SelectedDeviceBatch(db, self.sel, kept, n_bases, n_cigar), read_off

    def _run_hp(self, db, sizes, host_batch, qmax: int, windows, n_regions: int) -> HapChainResult:
        """one uploaded (or decoded) batch -> a ChainResult per haplotype: select, [realign], builder, then the rest of the
        chain, for h = 1, 2 in turn on the chain's buffers. A host batch without tags (read_hp None) keeps every read for
        both, so the chain runs once."""
        from .batch_select import tag_counts
        tags = tag_counts(db.read_hp, db.n_reads)
        if db.read_hp is None:
            has = np.diff(host_batch().read_off) > 0
            b, n = self._build(db, sizes, host_batch, qmax, windows)
            res = self._labels_and_stitch(b, n, n_regions)
            return HapChainResult((res, res), (has, has), tags)
        results, has_reads, payload = [], [], 0
        for h in (1, 2):
            sdb, read_off = self._select(db, h, n_regions)
            has_reads.append(np.diff(read_off) > 0)
            payload += 2 * (2 * sdb.n_bases + 4 * sdb.n_cigar)
            if sdb.n_reads == 0:   # nothing to build from
                results.append(self._labels_and_stitch(sdb, 0, n_regions))
                continue
            b, n = self._build(sdb, sizes, lambda h=h: self.ctx.batch_select_hp(host_batch(), h)[0], qmax, windows)
            results.append(self._labels_and_stitch(b, n, n_regions))
        return HapChainResult(tuple(results), tuple(has_reads), tags, payload)

    def _labels_and_stitch(self, db, n: int, n_regions: int) -> ChainResult:
        """P2 (a vote chain: the majority vote [-> the run vote]) [-> row qualities] [-> minimum-depth mask] [-> minimum-quality
        filter] [-> minimum-support filter] -> stitch [-> edits] over the first n chunks of self.dout on the context's stream,
        one synchronize, then the read-back"""
        from .polish_edits import EDIT_DTYPE, EVIDENCE_DTYPE
        o = self.options
        on = [p for p in PASSES if getattr(o, p.option) > 0]
        if n == 0:   # nothing to launch: every plane this chain was made for, empty
            zero = np.zeros(n_regions + 1, np.int64)
            res = ChainResult(zero, b"", b"" if o.qualities else None)
            res = res._replace(edit_off=zero.copy(), edits=np.zeros(0, EDIT_DTYPE)) if o.edits else res
            res = with_evidence(res, np.zeros(0, EVIDENCE_DTYPE)) if o.evidence else res
            for p in on:
                res = _with(res, p.attr, p.empty)
            return res
        import torch
        # --min_qual without --qualities computes the row qualities for the filter alone: the mask, the support filter, the
        # stitch and the edits get 0 and run as in a chain without qualities
        d_filter_acc, d_filter_qual = (self.acc.data_ptr(), self.row_qual.data_ptr()) if o.want_row_qual else (0, 0)
        d_row_qual, d_qual = (d_filter_qual, self.qual.data_ptr()) if o.qualities else (0, 0)
        d_labels = self.labels.data_ptr()
        draft = (db.t["ref_start"].data_ptr(), db.t["ref_off"].data_ptr(), db.t["ref"].data_ptr(), n_regions)
        roff = torch.empty(n_regions + 1, dtype=torch.int64, device=self.dev)   # every entry is written
        if o.vote:   # the reads' majority in the network's place: the same two planes, from the counts of this batch
            self.ctx.polish_vote_dev(self.dout, n, *draft, d_labels, d_filter_acc, self.vote_counts.data_ptr())
            if o.vote_runs:   # and every homopolymer run's length read by read, in place, from the reads the builder had
                self.ctx.polish_vote_runs_dev(self.dout, n, db, *draft, o.vote_runs, d_labels, d_filter_acc,
                                              self.runs_counts.data_ptr())
        else:
            self.ctx.forward_p2_dev(self.dout.images.data_ptr(), n, d_labels, d_filter_acc)
        if d_filter_qual:
            # (a label above 4 is reported by the stitch where it is on a kept column, as without qualities: the counts of
            # the row kernel are overwritten)
            self.ctx.polish_row_qual_dev(d_labels, d_filter_acc, n, d_filter_qual, self.counts.data_ptr(), self.dout.seq_length,
                                         self.dout.seq_overlap)
        for p in on:
            if p.in_place:   # what follows sees the draft's labels wherever the pass took the network's back; the row qualities
                # it zeroes are those the stitch and the edits read (the quality filter: its own, see above)
                d_q = d_filter_qual if p.option == "min_qual" else d_row_qual
                getattr(self.ctx, p.in_place)(self.dout, n, d_labels, d_q, *draft, getattr(o, p.option), d_labels, d_q,
                                              getattr(self, p.counters).data_ptr())
        self.ctx.polish_stitch_dev(self.dout, n, d_labels, draft[0], n_regions, roff.data_ptr(), self.seq.data_ptr(),
                                   self.seq.numel(), self.counts.data_ptr(), d_row_qual=d_row_qual, d_qual=d_qual)
        if o.edits:
            eoff = torch.empty(n_regions + 1, dtype=torch.int64, device=self.dev)   # every entry is written
            if o.evidence:   # the edits call's twin: the same records, and each one's read support beside it
                self.ctx.polish_edits_evidence_dev(self.dout, n, d_labels, d_row_qual, *draft, eoff.data_ptr(),
                                                   self.edit_buf.data_ptr(), self.ev_buf.data_ptr(), self.edit_buf.shape[0],
                                                   self.edit_counts.data_ptr())
            else:
                self.ctx.polish_edits_dev(self.dout, n, d_labels, d_row_qual, *draft, eoff.data_ptr(), self.edit_buf.data_ptr(),
                                          self.edit_buf.shape[0], self.edit_counts.data_ptr())
        self.ctx.synchronize()   # raises if a split GRU form timed out (its labels are then poisoned)
        extras = {}
        for p in on:
            c = [int(v) for v in getattr(self, p.counters).tolist()]
            if c[1] != _ffi.PV_OK:
                raise _ffi.PepperHipError(c[1], "polisher %s: device status %d (chunk %d)" % (p.noun, c[1], c[2]))
            extras[p.attr] = tuple(c[i] for i in p.pick)
        total, status, bad = (int(v) for v in self.counts[:3].tolist())
        if status != _ffi.PV_OK:   # capacity cannot run short: seq holds a byte for every column
            raise _ffi.PepperHipError(status, "polisher stitch: device status %d (chunk %d)" % (status, bad))
        res = ChainResult(roff.cpu().numpy(), self.seq[:total].cpu().numpy().tobytes(),
                          self.qual[:total].cpu().numpy().tobytes() if o.qualities else None)
        if o.edits:
            total, status, bad = (int(v) for v in self.edit_counts[:3].tolist())
            if status != _ffi.PV_OK:   # capacity cannot run short: a record for every chunk row
                raise _ffi.PepperHipError(status, "polisher edits: device status %d (chunk %d)" % (status, bad))
            res = res._replace(edit_off=eoff.cpu().numpy(), edits=self.edit_buf[:total].cpu().numpy().view(EDIT_DTYPE).reshape(-1))
            if o.evidence:
                res = with_evidence(res, self.ev_buf[:total].cpu().numpy().view(EVIDENCE_DTYPE).reshape(-1))
        for attr, counts in extras.items():
            res = _with(res, attr, counts)
        return res




def open_device_chain(device: int, shared_device: bool, state_dict: dict, dtype: int, **options) -> _DeviceChain:
    """a context on `device` with the polisher weights loaded, and the chain on it (closing the chain closes the context).
    shared_device: other ranks use this GPU too, so the option is set before the first device call (the split GRU forms need
    co-resident workgroups and would time out, poisoning the labels). False leaves the create-time default (PV_SHARED_DEVICE).
    This is the default `open_chain` of run and polish_rank.run; CPU tests pass a stub with the same signature, whose result
    has run(batch, windows) -> ChainResult and close(). options: the ChainOptions the chain is made for, each passed only
    when set (ChainOptions.keywords); its results carry the planes and counts of those. With vote no weights are loaded and
    state_dict may be None."""
    from .runtime import Context
    ctx = Context(device)
    try:
        if shared_device:
            ctx.set_option("shared_device", 1)
        if not options.get("vote"):
            ctx.load_p2(state_dict, dtype)
        return _DeviceChain(ctx, own_ctx=True, **options)
    except BaseException:
        ctx.close()
        raise




class _RealignedDeviceBatch:
    """a DeviceBatch whose positions and cigars are the realigner's output (same bases, quals, flags, mapq, regions)"""

    def __init__(self, c, db, n_cigar, keep):
        self.c, self._keep = c, (db, keep)
        self.n_reads, self.n_bases, self.n_cigar, self.n_ref_bytes = db.n_reads, db.n_bases, int(n_cigar), db.n_ref_bytes
        self.max_region_len = db.max_region_len
        self.t = db.t


def _read_ahead(ex, fn, items, depth):
    """fn(item) for every item on the executor's threads, results in order, at most `depth` in flight (bounded memory)"""
    it = iter(items)
    q = collections.deque(ex.submit(fn, x) for x in itertools.islice(it, depth))
    while q:
        f = q.popleft()
        for x in itertools.islice(it, 1):
            q.append(ex.submit(fn, x))
        yield f.result()


def _timers(timers: Optional[dict], more=()) -> dict:
    """the caller's timer dict (or a fresh one) with the keys of polish_pieces, and `more`, present"""
    T = timers if timers is not None else {}
    for k in ("read_s", "device_s", "regions", "batches") + PASS_TIMERS + tuple(more):
        T.setdefault(k, 0)
    return T




def _thread_handles(bam: str, fasta: str):
    """-> handles(): the calling thread's own (BamHandler, FastaHandler); the native handles are not shared between threads"""
    import threading
    from .bamio import BamHandler, FastaHandler
    local = threading.local()

    def handles():
        if not hasattr(local, "h"):
            local.h = (BamHandler(bam), FastaHandler(fasta))
        return local.h
    return handles


def _count_masked(T: dict, res) -> None:
    """the counts a result carries of every pass of PASSES (one launch's) into the timers"""
    for p in PASSES:
        for k, v in zip(p.timers, getattr(res, p.attr, None) or ()):
            T[k] += v




def kept_range(w: Work) -> Tuple[int, int]:
    """the positions of a region the stitch keeps, inclusive: (start + 200, end], or [start, end] for start 0"""
    return (w.start + 2 * MIN_IMAGE_OVERLAP + 1 if w.start > 0 else w.start), w.end


def draft_pieces(fa, work: List[Work], pieces, qualities: bool, edits: bool, evidence: bool = False) -> List[Piece]:
    """`--min_depth N` with N >= 1: a region of the run that gave no piece has no reads, so all of it is below N and it keeps
    the draft: a piece of the upper-cased draft bytes of its kept range (N and IUPAC bytes as they are), quality 0 for each
    base when the run carries qualities, no edits and therefore (evidence: an empty plane of) no evidence"""
    from .polish_edits import EDIT_DTYPE, EVIDENCE_DTYPE
    done = {p.index for p in pieces}
    out = []
    for w in work:
        first, last = kept_range(w)
        if w.index in done or last < first:
            continue
        bases = fa.get_reference_sequence(w.contig, first, last + 1).upper().encode()
        out.append(piece_of(w, (bases, bytes(len(bases)) if qualities else None, np.zeros(0, EDIT_DTYPE) if edits else None)
                            + ((np.zeros(0, EVIDENCE_DTYPE),) if evidence else ())))
    return out


def _hap_pieces(T: dict, hres: HapChainResult, works) -> list:
    """a launch's HapChainResult -> [(haplotype, Piece)]: haplotype 1's regions, then haplotype 2's, each without the regions
    its selection left without reads; the tag counts and the row counts go into the timers"""
    for k, v in zip(HP_TIMERS + ("hp_payload_bytes",), tuple(hres.tags) + (hres.payload,)):
        T[k] = T.get(k, 0) + int(v)
    out = []
    for h, (res, has) in enumerate(zip(hres.results, hres.has_reads), 1):
        _count_masked(T, res)
        out += [(h, piece_of(w, res.region(g))) for g, w in enumerate(works) if has[g]]
    return out


def polish_pieces(bam: str, fasta: str, work: List[Work], chain, batch_size: int = 2048, threads: int = 5, realign: bool = False,
                  timers: Optional[dict] = None, gpu_decode: bool = False, open_decoder=None, use_hp: bool = False):
    """the regions of `work` through the chain -> a Piece for every region with reads, in `work` order. This is the whole
    device part of a run: the single-rank run passes every region, a rank of a multi-device run its share.
    chain.run(batch, windows) -> ChainResult (_DeviceChain or a CPU test's stub); a piece carries the planes that result
    carried (qual with a chain made for --qualities, edits with one made for --edits, else None).
    timers (optional) accumulates read_s, device_s, regions, batches, and masked_rows / unmaskable_rows of the results that
    carry the counts of a minimum-depth chain, reverted_rows / pinned_rows of those of a minimum-quality chain.
    gpu_decode: the device read path (_decoded_pieces): the reader threads only plan, the BAM is inflated, decoded and clipped
    on chain.ctx's device, and the chain takes the batches where they are (chain.run_decoded). open_decoder(T): the decoder,
    by default a gpu_decode.GpuDecoder with the polisher's settings (CPU tests pass a stub with its scan_groups, realize,
    iterate and close).
    use_hp: the chain was made with use_hp and gives a HapChainResult per launch; (haplotype, Piece) pairs are yielded, per
    launch haplotype 1's then haplotype 2's, and the timers also count the tags (HP_TIMERS)."""
    if gpu_decode:
        yield from _decoded_pieces(bam, fasta, work, chain, batch_size, threads, realign, timers, open_decoder, use_hp)
        return
    from .batch import pack_regions
    from .polish_summary import region_from_files
    T = _timers(timers)
    handles = _thread_handles(bam, fasta)

    def read(w):
        return w, region_from_files(*handles(), w.contig, w.start, w.end, realign=realign)

    per_launch = max(1, int(batch_size) // 2)

    def flush(items):
        t0 = time.perf_counter()
        regs = [r for _, r in items]
        res = chain.run(pack_regions(regs), [r.window for r in regs] if realign else None)
        if use_hp:
            out = _hap_pieces(T, res, [w for w, _ in items])
        else:
            _count_masked(T, res)
            out = [piece_of(w, res.region(g)) for g, (w, _) in enumerate(items)]
        T["device_s"] += time.perf_counter() - t0
        T["batches"] += 1
        return out

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
        pending = []
        t0 = time.perf_counter()
        for w, reg in _read_ahead(ex, read, work, 2 * per_launch):
            if reg is None:
                continue
            pending.append((w, reg))
            T["regions"] += 1
            if len(pending) == per_launch:
                T["read_s"] += time.perf_counter() - t0
                yield from flush(pending)
                pending = []
                t0 = time.perf_counter()
        T["read_s"] += time.perf_counter() - t0
        if pending:
            yield from flush(pending)


def _decoded_pieces(bam, fasta, work, chain, batch_size, threads, realign, timers, open_decoder, use_hp=False):
    """polish_pieces' device read path. Reader threads plan reader groups (gpu_decode.region_groups: blocks, interval table,
    draft bytes, realign windows); the decoder's service thread scans them, cuts the regions with reads into the launches
    the host path makes (per_launch regions each) and fills them on its own stream; this thread runs the chain on every
    part of a launch: a decoded batch as it lies on the device, a host-route group (reads longer than the plan's look-ahead,
    or a group over the workspace budget) as the host path's packed batch. Adds the timers plan_s, decode_s, chain_runs
    (chain runs: one per part of a launch) and the decoder's own (gpu_decode_groups_host, gpu_decode_slot_retries, gpu_decode_ws_peak_bytes, ...)."""
    from . import gpu_decode as gd
    from .polish_summary import MAX_READS_IN_REGION
    T = _timers(timers, ("chain_runs", "plan_s", "decode_s", "gpu_decode_groups", "gpu_decode_groups_host"))
    per_launch = max(1, int(batch_size) // 2)
    if open_decoder is None:
        def open_decoder(T):
            return gd.GpuDecoder(chain.ctx, bam, fasta, 0, False, 1.0, 0, T, max_reads=MAX_READS_IN_REGION, adaptive_slots=True,
                                 realign=realign)
    handles = _thread_handles(bam, fasta)

    def plan(ws):
        return gd.PlannedGroup(*handles(), [(w.contig, w.start, w.end) for w in ws], 0, pad_ref=True, windows=realign, works=ws)

    groups = gd.region_groups(work)
    dec = open_decoder(T)
    try:
        with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
            def planned():
                for g in _read_ahead(ex, plan, groups, max(2 * per_launch // gd.GROUP_REGIONS, 2 * int(threads), 2)):
                    T["plan_s"] += g.t_plan
                    yield g
            gen = gd.decoded_launches(dec, planned(), per_launch)
            launches = dec.iterate(gen)
            t0 = time.perf_counter()
            for parts in launches:
                T["read_s"] += time.perf_counter() - t0
                t0 = time.perf_counter()
                for kind, b, windows, ws in parts:
                    res = chain.run_decoded(b, windows) if kind == "dev" else chain.run(b, windows)
                    T["chain_runs"] += 1
                    T["regions"] += len(ws)
                    if use_hp:
                        yield from _hap_pieces(T, res, ws)
                        continue
                    _count_masked(T, res)
                    for g, w in enumerate(ws):
                        yield piece_of(w, res.region(g))
                T["device_s"] += time.perf_counter() - t0
                T["batches"] += 1
                del parts
                t0 = time.perf_counter()
            T["read_s"] += time.perf_counter() - t0
    finally:
        dec.close()


def decode_report(T: dict) -> str:
    """one line on what the device read path did, for the log (empty without --gpu_decode)"""
    if "gpu_decode_groups" not in T:
        return ""
    return ("GPU DECODE: %d GROUPS IN %d SCANS, %d ON THE HOST ROUTE, %d SLOT RETRIES, %d CHAIN RUNS IN %d LAUNCHES"
            % (T["gpu_decode_groups"], T.get("gpu_inflate_launches", 0), T["gpu_decode_groups_host"],
               T.get("gpu_decode_slot_retries", 0), T.get("chain_runs", 0), T["batches"]))


# What polish_fused asks of a chain passed in, in the order it asks: (option = the chain's attribute, the value of a chain
# without the attribute, refused when (run's value, chain's value), what the chain does: %r the chain's value, %d the run's)
_MADE_FOR = (
    ("min_depth", None, lambda want, have: want >= 1 and have != want, "masks below depth %r, not %d"),
    ("min_qual", None, lambda want, have: want >= 1 and have != want, "filters below quality %r, not %d"),
    ("min_support", None, lambda want, have: want >= 1 and have != want, "filters below support %r, not %d"),
    ("vote", False, lambda want, have: want and not have, "does not vote"),
    ("vote", False, lambda want, have: have and not want, "votes in the network's place"),
    ("vote_runs", 0, lambda want, have: want != int(have or 0), "votes runs from length %r, not %d"),
    ("use_hp", False, lambda want, have: want and not have, "does not select reads by haplotype"),
)
_NOT_MADE = "polish_fused: the chain%s: it was not made for this run"


def polish_fused(bam: str, fasta: str, model_path: str, out_prefix: str, region: Optional[str] = None, batch_size: int = 2048,
                 threads: int = 5, dtype: int = _ffi.PV_DTYPE_F32, ctx=None, timers: Optional[dict] = None,
                 realign: bool = False, chain=None, gpu_decode: bool = False, **options) -> str:
    """-> path of the polished FASTA (use_hp: of haplotype 1's). batch_size: chunks per device launch (a region of up to 1201 columns gives about two).
    realign: realign every read to the draft on the device before the builder, as the reference always does.
    chain: a chain with the weights already loaded (open_device_chain; the caller closes it), else one is made on `ctx`
    (default: a context on device 0) from model_path. gpu_decode: polish_pieces' device read path.
    options: the ChainOptions of the run. They make this function's own chain and pick the files and the VCF's header
    lines; a chain passed in must have been made for them (_MADE_FOR), and one whose results lack a plane they need is
    refused too (ValueError), before any file is written.
    qualities: also write the FASTQ beside the FASTA (output_fastq_path).
    edits: also write the edits VCF and its index beside the FASTA (polish_edits.output_vcf_path). The VCF is composed
    before any file is written, so a run it refuses (overlapping -r ranges of one contig) leaves nothing.
    evidence (with edits): every VCF record carries DP, AD, SAF and SAR of its weakest column (polish_edits.compose_records).
    min_depth >= 1: the rows below it are masked, the regions without reads are filled from the draft (draft_pieces), and
    the VCF names the threshold. min_qual >= 1, min_support >= 1: the runs of edits below them are taken back, and the VCF
    names the threshold.
    use_hp: one set of files per haplotype (hp_path) in place of the un-suffixed ones.
    vote: the labels come from the reads' majority: model_path is not read (it may be None), and the VCF names the consensus.
    vote_runs = min_run >= 2 (with vote): every homopolymer run's length is voted read by read too (a chain passed in must
    have been made with the same min_run), and the VCF names the consensus vote+runs and min_run."""
    from .bamio import BamHandler, FastaHandler
    from .runtime import Context
    t_start = time.perf_counter()
    if chain is not None and options.get("evidence") and not options.get("edits"):
        raise ValueError("polish_fused: evidence needs edits: the numbers go into the edits VCF")
    o = ChainOptions(**options)
    T = dict(read_s=0.0, device_s=0.0, regions=0, batches=0, bases_in=0, bases_out=0, draft_regions=0, **dict.fromkeys(PASS_TIMERS, 0))
    own = None
    if chain is None:
        state_dict = None if o.vote else load_polish_model(model_path)
        if ctx is None:
            ctx = own = Context(0)
        if not o.vote:
            ctx.load_p2(state_dict, dtype)
        chain = _DeviceChain(ctx, **o.keywords())
    try:
        fa, bm = FastaHandler(fasta), BamHandler(bam)
        work, T["bases_in"] = polish_work(fa, bm, region)
        out_path = output_fasta_path(out_prefix)
        log("POLISHING %d REGIONS, OUTPUT: %s" % (len(work), out_path))
        for option, default, refused, does in _MADE_FOR:
            want, have = getattr(o, option), getattr(chain, option, default)
            if refused(want, have):
                raise ValueError(_NOT_MADE % (" " + (does % (have, want) if "%" in does else does)))
        if o.use_hp:
            pairs = list(polish_pieces(bam, fasta, work, chain, batch_size, threads, realign, T, gpu_decode=gpu_decode, use_hp=True))
            outputs = [(h, hp_path(out_path, h), [p for k, p in pairs if k == h]) for h in (1, 2)]
        else:
            outputs = [(0, out_path, list(polish_pieces(bam, fasta, work, chain, batch_size, threads, realign, T, gpu_decode=gpu_decode)))]
        vcfs = []
        for _, _, pieces in outputs:
            for want, plane in ((o.qualities, "qual"), (o.edits, "edits"), (o.evidence, "evidence")):
                if want and pieces and getattr(pieces[0], plane) is None:
                    raise ValueError(_NOT_MADE % ("'s results have no %s plane" % plane))
            if o.min_depth >= 1:
                filled = draft_pieces(fa, work, pieces, o.qualities, o.edits, o.evidence)
                T["draft_regions"] += len(filled)
                pieces += filled
            vcfs.append(_edits_vcf(fa, fasta, work, pieces, o.qualities, o.min_depth, o.min_qual, o.evidence) if o.edits else None)
    finally:
        if own is not None:
            own.close()
    for (h, path, pieces), vcf in zip(outputs, vcfs):
        seqs = write_polished_fasta(path, pieces)
        if o.qualities:
            write_fastq(output_fastq_path(path), seqs, merge_pieces(pieces, part=4))
        if o.edits:
            from . import polish_edits
            polish_edits.write_edits_vcf(polish_edits.output_vcf_path(path), *vcf, haplotype=h, evidence=o.evidence,
                                         min_support=o.min_support, min_run=o.vote_runs,
                                         consensus=("vote+runs" if o.vote_runs else "vote") if o.vote else "")
            if o.evidence:   # records whose alt support (of their weakest column) stands on one strand only
                T["one_strand_records"] = T.get("one_strand_records", 0) + sum(
                    (r.evidence[2] == 0) != (r.evidence[3] == 0) for recs in vcf[4].values() for r in recs)
            T["edit_records"] = T.get("edit_records", 0) + sum(len(p.edits) for p in pieces)
            T["vcf_records"] = T.get("vcf_records", 0) + sum(len(r) for r in vcf[4].values())
        T["bases_out"] += sum(len(s) for s in seqs.values())
    T["wall_s"] = time.perf_counter() - t_start
    if timers is not None:
        timers.update(T)
    return outputs[0][1]


def _edits_vcf(fa, fasta_path: str, work: List[Work], pieces, qualities: bool, min_depth: int = 0, min_qual: int = 0,
               evidence: bool = False) -> tuple:
    """the pieces' edit records -> write_edits_vcf's arguments behind the path: (source, reference, contigs of the run with
    their lengths, read-free runs, VCF records per contig, min_depth, min_qual). Pieces of a contig are joined in region-start order,
    as merge_pieces joins the bases. A region without a piece gave no chunks: the FASTA omits its kept range
    (kept_range) and a pepper_no_reads header line names it. With min_depth >= 1 every region has a piece (draft_pieces).
    evidence: the pieces' evidence records are joined alike and the VCF records carry their weakest column's."""
    from . import polish_edits
    names = list(dict.fromkeys(w.contig for w in work))
    contigs = [(c, fa.get_chromosome_sequence_length(c)) for c in names]
    done = {p.index for p in pieces}
    no_reads = polish_edits.no_read_runs(
        (w.contig,) + kept_range(w) for w in work if w.index not in done)
    by: Dict[str, list] = {}
    for p in pieces:
        by.setdefault(p.contig, []).append((p.start, p.index, p.edits, p.evidence if evidence else None))
    records = {}
    for c, length in contigs:
        if c in by:
            parts = sorted(by[c], key=lambda t: (t[0], t[1]))
            recs = np.concatenate([e for _, _, e, _ in parts])
            draft = fa.get_reference_sequence(c, 0, length).encode() if len(recs) else b""
            ev = {"evidence": np.concatenate([v for _, _, _, v in parts])} if evidence else {}
            records[c] = polish_edits.compose_records(c, recs, draft, qualities, warn=log, **ev)
    return "pepper_thesis_amd polish", os.path.abspath(fasta_path), contigs, no_reads, records, int(min_depth), int(min_qual)


def _one_device(option: str, flag: str, what: str) -> tuple:
    """a refusal of the command: `option` is set and -d_ids lists several devices, between which `what` holds"""
    return (lambda o, args, devices: getattr(o, option) and devices > 1,
            "polish %s runs on one device (-d_ids %%(device_ids)s lists %%(devices)d): %s.\n" % (flag, what))


# What the command refuses about its options, in the order it looks (the first that holds is reported): (refused when (the
# unchecked ChainOptions, the namespace, the devices of -d_ids), the text behind "ERROR: ", filled from the options)
_REFUSALS = (
    _one_device("qualities", "--qualities", "the quality plane is not carried through the rank exchange yet"),
    _one_device("edits", "--edits", "the edit records are not carried through the rank exchange yet"),
    (lambda o, args, devices: o.evidence and not o.edits,
     "polish --evidence needs --edits: the read support goes into the INFO column of the edits VCF.\n"),
    (lambda o, args, devices: not 0 <= o.min_depth <= 65535,
     "polish --min_depth %(min_depth)d: the minimum depth is a number of reads from 0 (off) to 65535.\n"),
    _one_device("min_depth", "--min_depth", "the depth plane is not carried through the rank exchange yet"),
    (lambda o, args, devices: not 0 <= o.min_qual <= 94,
     "polish --min_qual %(min_qual)d: the minimum quality is a Phred value from 0 (off) to 94 (qualities stop at 93, so 94 takes "
     "back every edit).\n"),
    _one_device("min_qual", "--min_qual", "the row qualities are not carried through the rank exchange yet"),
    (lambda o, args, devices: not 0 <= o.min_support <= 65535,
     "polish --min_support %(min_support)d: the minimum support is a number of reads from 0 (off) to 65535.\n"),
    _one_device("min_support", "--min_support", "the counts plane is not carried through the rank exchange yet"),
    (lambda o, args, devices: getattr(args, "min_run", None) is not None and not o.vote_runs,
     "polish --min_run needs --runs: it is the shortest homopolymer run the run vote looks at.\n"),
    (lambda o, args, devices: o.vote_runs and not o.vote,
     "polish --runs needs --vote: the run vote rewrites the rows the reads' column vote left; behind a model it has no meaning.\n"),
    (lambda o, args, devices: o.vote_runs and not 2 <= o.vote_runs <= 48,
     "polish --min_run %(vote_runs)d: the shortest run voted on is a length from 2 to 48.\n"),
    _one_device("vote_runs", "--runs", "the reads are not carried through the rank exchange"),
    (lambda o, args, devices: o.vote_runs and o.min_support,
     "polish --runs takes no --min_support: that filter promises that at least K reads spell an edit in its own column, and a "
     "run-voted column can be one that few reads delete there.\n"),
    _one_device("vote", "--vote", "the counts plane is not carried through the rank exchange yet"),
    _one_device("use_hp", "-hp", "the haplotypes are not carried through the rank exchange yet"),
)


def run(args, open_chain=open_device_chain) -> int:
    """the `polish` command. With several -d_ids: check the inputs here (no GPU API is touched), then start one rank per id
    and wait for them (polish_rank.launch). open_chain: see open_device_chain (CPU tests pass a stub)."""
    from . import cli, polish_rank
    vote = bool(getattr(args, "vote", False))
    if not vote and getattr(args, "model_path", None) is None:   # (a namespace not made by cli.polish_parser, which refuses this itself)
        sys.stderr.write("ERROR: polish: the following arguments are required: -m/--model_path (or --vote, which needs no model)\n")
        return 2
    if vote and (getattr(args, "model_path", None) is not None or getattr(args, "bf16", False)):
        sys.stderr.write("ERROR: polish --vote takes no %s: the vote stands in the network's place, so no model is read and none "
                         "may be named.\n" % ("-m" if getattr(args, "model_path", None) is not None else "--bf16"))
        return 2
    _, world, device = cli.rank_world_device(args)
    if world > 1:
        sys.stderr.write("ERROR: polish runs on one process (WORLD_SIZE=%d): multi-rank polishing is not part of this build.\n" % world)
        return 2
    try:
        plan = polish_rank.plan_ranks(args.device_ids, args.threads)
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        return 2
    o = ChainOptions.from_args(args)
    said = dict(dataclasses.asdict(o), device_ids=args.device_ids, devices=len(plan))
    for refused, text in _REFUSALS:
        if refused(o, args, len(plan)):
            sys.stderr.write("ERROR: " + text % said)
            return 2
    for what, path in (("BAM", args.bam), ("FASTA", args.fasta)) + (() if vote else (("MODEL", args.model_path),)):
        if not os.path.isfile(path):
            sys.stderr.write("ERROR: CAN NOT LOCATE %s FILE.\n" % what)
            return 1
    if args.threads <= 0 or args.batch_size <= 0:
        sys.stderr.write("ERROR: THREADS AND batch_size NEED TO BE > 0.\n")
        return 1
    try:
        state_dict = None if vote else load_polish_model(args.model_path)
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        return 2
    if len(plan) > 1:
        return polish_rank.launch(args, plan)
    dtype = _ffi.PV_DTYPE_BF16_INPUT_GEMM if args.bf16 else _ffi.PV_DTYPE_F32
    chain = open_chain(device, False, state_dict, dtype, **o.keywords())   # (only those that are set: stub chains keep their signatures)
    try:
        T = {}
        path = polish_fused(args.bam, args.fasta, args.model_path, args.output_file, args.region, args.batch_size, args.threads,
                            timers=T, realign=bool(getattr(args, "realign", False)), chain=chain,
                            gpu_decode=bool(getattr(args, "gpu_decode", False)), **o.keywords())
    except ValueError as e:
        if not o.edits:
            raise
        sys.stderr.write("ERROR: %s\n" % e)
        return 2
    finally:
        chain.close()
    if decode_report(T):
        log(decode_report(T))
    log("POLISHED FASTA: %s (%d REGIONS, %d BASES IN %.2f SEC)" % (path, T["regions"], T["bases_out"], T["wall_s"]))
    paths = [path]
    if o.use_hp:
        paths.append(hp_path(path[:-len("_hp1.fa")] + ".fa", 2))
        log("POLISHED FASTA: " + paths[1])
        log("HAPLOTYPES: %d READS SEEN, %d UNTAGGED, %d HP1, %d HP2, %d WITH OTHER TAG VALUES (IN NEITHER HAPLOTYPE)"
            % tuple(T.get(k, 0) for k in HP_TIMERS))
        if T.get("hp_reads", 0) == T.get("hp_untagged", 0):
            sys.stderr.write("WARNING: polish -hp: no read carries an HP tag; both haplotypes are the plain polish of all reads.\n")
    for p in sorted(PASSES, key=lambda p: p.in_place is not None):   # in launch order: the votes, then the in-place passes
        if getattr(o, p.option):
            log(p.report % dict(dataclasses.asdict(o), **T))
    if o.qualities:
        log("POLISHED FASTQ: " + ", ".join(output_fastq_path(p) for p in paths))
    if o.edits:
        from .polish_edits import output_vcf_path
        log("EDITS VCF: %s (%d RECORDS FROM %d EDITED COLUMNS)" % (", ".join(output_vcf_path(p) for p in paths), T["vcf_records"],
                                                                   T["edit_records"]))
    if o.evidence:
        log("EVIDENCE: %d OF %d RECORDS HAVE THEIR ALT SUPPORT ON ONE STRAND ONLY" % (T.get("one_strand_records", 0), T["vcf_records"]))
    return 0
