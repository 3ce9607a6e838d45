"""The polisher's command line (pepper/pepper.py:24-260): `python -m pepper_thesis_amd.pepper <sub-command> ...`.

  polish          BAM + draft -> polished FASTA, every stage on the device (polish.py; the parser of `python -m
                  pepper_thesis_amd polish`, unchanged)
  make_images     BAM + draft -> image HDF5 files              (polish_steps.make_images_run)
  call_consensus  image files -> prediction HDF5 files         (polish_steps.call_consensus_run)
  stitch          prediction files -> polished FASTA           (polish_steps.stitch_run)
  assess          polished FASTA + truth FASTA -> identity, QV and error tables, on the device (assess.run)
  kmer_qv         polished FASTA + BAM + draft -> reference-free k-mer QV and where the unsupported k-mers lie (kmer_qv.run)

A program of its own, as in the reference: its `make_images` is the polisher's, not the variant caller's sub-command of the
same name (`python -m pepper_thesis_amd make_images`). download_models and torch_stat are not part of this build.
"""
import argparse
import sys

from . import cli


def make_images_parser(ap=None):
    """add_make_images_arguments (pepper/pepper.py:104-147), plus --realign as in polish"""
    ap = ap or argparse.ArgumentParser(prog="make_images")
    ap.add_argument("-b", "--bam", type=str, required=True, help="BAM file of the reads aligned to the draft assembly")
    ap.add_argument("-f", "--fasta", type=str, required=True, help="FASTA file of the draft assembly")
    ap.add_argument("-r", "--region", type=str, default=None, help="contig[:start-end]")
    ap.add_argument("-o", "--output_dir", type=str, required=True, default="make_image_output/",
                    help="output directory, created if missing")
    ap.add_argument("-t", "--threads", type=int, default=5,
                    help="reader threads, and the number of image files (region i goes to file i %% threads)")
    ap.add_argument("--realign", action="store_true", default=False,
                    help="realign every read to the draft (Smith-Waterman on the device) before the images are built, as "
                         "polish --realign; the reference always does this. Off by default")
    cli.polish_gpu_decode_flag(ap)
    return ap


def call_consensus_parser(ap=None):
    """add_call_consensus_arguments (pepper/pepper.py:150-218), plus --bf16 as in polish"""
    ap = ap or argparse.ArgumentParser(prog="call_consensus")
    ap.add_argument("-i", "--image_dir", type=str, required=True, help="directory of the image HDF5 files")
    ap.add_argument("-m", "--model_path", type=str, required=True, help="the polisher model")
    ap.add_argument("-o", "--output_dir", type=str, required=True, default="output", help="output directory")
    ap.add_argument("-bs", "--batch_size", type=int, default=2048,
                    help="chunks (1000 columns) per device launch; default 2048 as in polish (the reference's is 128)")
    ap.add_argument("-g", "--gpu", action="store_true", default=False, help="accepted; this build has no CPU path")
    ap.add_argument("-d_ids", "--device_ids", type=str, default=None,
                    help="comma list of device ids: one id picks the device; several ids (at most 16, repeats allowed) start "
                         "one caller per id, caller r on the r-th id writing pepper_prediction_<id>.hdf (<id>_<r> for a "
                         "repeated id)")
    ap.add_argument("-w", "--num_workers", type=int, default=4, help="accepted and ignored")
    ap.add_argument("-t", "--threads", type=int, default=8, help="accepted and ignored (there is no CPU path)")
    ap.add_argument("--bf16", action="store_true", default=False,
                    help="PV_DTYPE_BF16_INPUT_GEMM: matrix products on the bf16 MFMA with 3-term split operands")
    ap.add_argument("--qualities", action="store_true", default=False,
                    help="write every chunk's phred_score as the per-row Phred quality of its label (0..93, from P2's "
                         "accumulated softmax; the rule in include/pepper_hip.h) instead of the reference's label table, for "
                         "stitch --qualities")
    return ap


def stitch_parser(ap=None):
    """add_stitch_arguments (pepper/pepper.py:221-253)"""
    ap = ap or argparse.ArgumentParser(prog="stitch")
    ap.add_argument("-i", "--input_dir", type=str, required=True, help="directory of the prediction HDF5 files")
    ap.add_argument("-o", "--output_file", type=str, required=True,
                    help="output prefix: the FASTA is <output_file>_pepper_polished.fa (parent directories are created)")
    ap.add_argument("-t", "--threads", type=int, default=5, help="accepted and ignored (the stitch runs on the device)")
    ap.add_argument("--qualities", action="store_true", default=False,
                    help="also write <output_file>_pepper_polished.fq with one Phred byte per base, from the phred_score that "
                         "call_consensus --qualities wrote")
    return ap


def assess_parser(ap=None):
    """`assess`: the reference has no counterpart (it leaves assessment to outside tools)"""
    ap = ap or argparse.ArgumentParser(prog="assess")
    ap.add_argument("-a", "--assembly", type=str, required=True, help="FASTA of the assembly to score (the polished one)")
    ap.add_argument("-t", "--truth", type=str, required=True,
                    help="FASTA of the true sequence. Contigs are paired by name, in the same orientation, and taken to be "
                         "colinear: no reverse complement and no rearrangement is looked for (--place drops the names and "
                         "finds contig, strand and interval by content)")
    ap.add_argument("-o", "--output", type=str, required=True,
                    help="output prefix: <output>_assess.tsv (one line per contig and TOTAL) and <output>_assess.segments.tsv "
                         "(one line per segment); parent directories are created")
    ap.add_argument("-d", "--draft", type=str, default=None,
                    help="FASTA of the draft: scored the same way into <output>_assess_draft.tsv; the log gives errors and QV "
                         "before -> after")
    ap.add_argument("--errors", action="store_true", default=False,
                    help="also write <output>_assess.errors.tsv: every substitution, insertion and deletion of the alignment, in "
                         "assembly and truth coordinates (0-based); with -d the draft's list goes to "
                         "<output>_assess_draft.errors.tsv")
    ap.add_argument("-q", "--fastq", type=str, default=None,
                    help="the FASTQ `polish --qualities` wrote for the -a assembly: every error is charged to the quality of its "
                         "base, and <output>_assess.calibration.tsv gives, per contig and quality value, bases, errors and the "
                         "observed QV")
    ap.add_argument("--segment", type=int, default=1024,
                    help="bases between anchors, a multiple of 32 in [256, 65536]; the windowed error track has this resolution")
    ap.add_argument("--max_shift", type=int, default=8192,
                    help="how far from its proportional place an anchor is searched in the truth, in [32, 1048576]")
    ap.add_argument("--place", action="store_true", default=False,
                    help="do not pair contigs by name: place every assembly contig on the truth by content (which truth contig, "
                         "which strand, which interval, from 32-mers that occur once in the truth), reverse-complement it if "
                         "need be and score it against that interval; <output>_assess.placement.tsv lists the placements. One "
                         "interval per contig, no rearrangement search")
    ap.add_argument("--place_step", type=int, default=None,
                    help="with --place: bases between the sampled 32-mers, a multiple of 32 in [32, 65536] (default 1024)")
    ap.add_argument("--min_hits", type=int, default=None,
                    help="with --place: the fewest agreeing unique 32-mers that place a contig, in [1, 65535] (default 3)")
    ap.add_argument("-d_id", "--device_id", type=int, default=0, help="the device")
    return ap


KMER_QV_IS_NOT = ("What it is not: an error that the reads share is supported and invisible (ONT homopolymer lengths are the main "
                  "case); a true k-mer in a coverage hole is counted as an error; with noisy reads and --min_count 1 an error "
                  "k-mer can be carried by a chance read error, so the figure is an upper bound of the true QV and the "
                  "histogram is the evidence for a larger --min_count; it compares assemblies on the same reads and does not "
                  "replace `assess` where a truth exists; no value of --min_count is recommended.")


COMPLETENESS_IS_NOT = ("The same reads and the same interval clipping as the QV side. What it is not: with noisy reads the error "
                       "k-mers dominate reads_only at low counts, and that is what the curve is read past; a k-mer the reads "
                       "cover thinly is lost at a high threshold whether or not the assembly holds it.")


def kmer_qv_parser(ap=None):
    """`kmer_qv`: the reference has no counterpart"""
    ap = ap or argparse.ArgumentParser(prog="kmer_qv")
    ap.description = ("Reference-free QV of an assembly: a k-mer of the assembly that fewer than --min_count read k-mers contain "
                      "is taken to be an error (the rule of Merqury and yak, on the device). The reads are the aligned part of "
                      "the BAM's primary reads as the polisher sees them, soft clips and leading insertions gone, clipped at "
                      "the --interval edges (a read k-mer across an edge is not counted: about k / interval of them).")
    ap.epilog = KMER_QV_IS_NOT
    ap.add_argument("-a", "--assembly", type=str, required=True, help="FASTA of the assembly to score (the polished one)")
    ap.add_argument("-b", "--bam", type=str, required=True, help="BAM of the reads, as given to polish")
    ap.add_argument("-f", "--fasta", type=str, required=True,
                    help="FASTA the BAM was aligned to (the draft): the reader wants its bytes; with -d it is scored too")
    ap.add_argument("-o", "--output", type=str, required=True,
                    help="output prefix: <output>_kmer_qv.tsv (one line per contig and TOTAL), .segments.tsv (unsupported k-mers "
                         "per --segment bases), .runs.bed (stretches of unsupported k-mers and the bases all of them cover) and "
                         ".hist.tsv (assembly k-mers by read count); parent directories are created")
    ap.add_argument("-d", "--draft", action="store_true", default=False,
                    help="score the -f FASTA the same way into <output>_kmer_qv_draft.*, in the same pass over the reads; the log "
                         "gives unsupported k-mers and QV before -> after")
    ap.add_argument("-k", "--kmer", type=int, default=21, help="k-mer length, odd, in [11, 31]")
    ap.add_argument("--min_count", type=int, default=1,
                    help="a k-mer with fewer read occurrences is unsupported; choose it by <output>_kmer_qv.hist.tsv, no value is "
                         "recommended")
    ap.add_argument("--segment", type=int, default=1024, help="bases per line of the segment track, a multiple of 32 in [32, 65536]")
    ap.add_argument("--interval", type=int, default=1000000, help="bases of a contig read at a time, at least 1000")
    ap.add_argument("-t", "--threads", type=int, default=5, help="reader threads; the output does not depend on them")
    ap.add_argument("--completeness", action="store_true", default=False,
                    help="also count the reads' k-mers that the assembly lacks, in a table of their own on the device: "
                         "<output>_kmer_qv.spectrum.tsv (by read count: the distinct read k-mers the assembly lacks, and its own "
                         "distinct k-mers that it holds once, twice, three times, four times or more) and .completeness.tsv (for "
                         "every threshold s: the distinct read k-mers seen s times or more, those of them in the assembly, their "
                         "share). " + COMPLETENESS_IS_NOT)
    ap.add_argument("--read_table_mb", type=float, default=None,
                    help="with --completeness: megabytes of device memory for each scored FASTA's table of read k-mers (default "
                         "1024); the largest power of two of 12-byte slots that fits is used. A full table ends the run with "
                         "status 2")
    ap.add_argument("--passes", type=int, default=None,
                    help="with --completeness: read the BAM this many times, in [1, 4096] (default 1), each time counting one part "
                         "of the k-mers, so that the table need only hold that part; the result does not depend on it")
    ap.add_argument("--solid", type=int, default=None,
                    help="with --completeness: the threshold, in [1, 255], of the completeness the log gives (default 2, a "
                         "convention: a read k-mer seen twice is rarely a read error at low depth; the file holds every threshold)")
    ap.add_argument("-d_id", "--device_id", type=int, default=0, help="the device")
    return ap


def parser():
    ap = argparse.ArgumentParser(prog="pepper", description="PEPPER polisher on the MI355X-native hot path: polish, or its three "
                                                            "steps make_images -> call_consensus -> stitch through files")
    ap.add_argument("--version", action="store_true", default=False)
    sub = ap.add_subparsers(dest="sub_command")
    cli.polish_parser(sub.add_parser("polish", help="make_images -> call_consensus -> stitch on the device, without files"))
    make_images_parser(sub.add_parser("make_images", help="image HDF5 files of the reads aligned to the draft"))
    call_consensus_parser(sub.add_parser("call_consensus", help="prediction HDF5 files from the image files and a model"))
    stitch_parser(sub.add_parser("stitch", help="the polished FASTA from the prediction files"))
    assess_parser(sub.add_parser("assess", help="identity, QV and error breakdown of an assembly against a truth FASTA"))
    kmer_qv_parser(sub.add_parser("kmer_qv", help="reference-free QV of an assembly from its k-mers' support in the reads"))
    return ap


def main(argv=None) -> int:
    ap = parser()
    args = ap.parse_args(argv)
    if args.version:
        print("PEPPER VERSION: ", cli.__version__)
        return 0
    if args.sub_command == "polish":
        from . import polish
        return polish.run(args)
    if args.sub_command == "assess":
        from . import assess
        return assess.run(args)
    if args.sub_command == "kmer_qv":
        from . import kmer_qv
        return kmer_qv.run(args)
    from . import polish_steps
    if args.sub_command == "make_images":
        return polish_steps.make_images_run(args)
    if args.sub_command == "call_consensus":
        return polish_steps.call_consensus_run(args)
    if args.sub_command == "stitch":
        return polish_steps.stitch_run(args)
    sys.stderr.write("ERROR: NO SUBCOMMAND SELECTED. PLEASE SELECT ONE OF THE AVAIABLE SUB-COMMANDS.\n")
    ap.print_help()
    return 2


if __name__ == "__main__":
    rc = main()
    sys.exit(rc if isinstance(rc, int) else 0)
