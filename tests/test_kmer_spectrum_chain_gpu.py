"""GPU: `pepper kmer_qv -d --completeness` on a truth of two 20 kb contigs with 20x error-free reads aligned to it: the draft
(the truth) is complete at every threshold, the assembly (the truth without one 2 kb stretch) is not, the curve is the rule's
restatement fed with what the host reader returns, neither --passes nor the reader threads change a byte, a table too small
ends with status 2, and without the flag the command writes what it wrote before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_writer as bw  # noqa: E402
import kmer_qv_ref as R  # noqa: E402
import kmer_spectrum_ref as S  # noqa: E402

from pepper_thesis_amd import bamio, build, pepper  # noqa: E402
from pepper_thesis_amd import kmer_qv as kq  # noqa: E402

pytestmark = pytest.mark.gpu
K, LENGTH, DEPTH, INTERVAL = 21, 20_000, 20, 6000
CUT = (9000, 11000)   # the stretch of the first contig that the assembly lacks
QV_FILES = [".hist.tsv", ".runs.bed", ".segments.tsv", ".tsv"]
MORE_FILES = [".completeness.tsv", ".spectrum.tsv"]


def records(rng, truth):
    recs = []
    for tid, (_, t) in enumerate(truth):
        for p in range(DEPTH):
            s = 0 if p == 0 else -int(rng.integers(0, 1500))
            while s < LENGTH - 60:
                e = LENGTH if LENGTH - (s + 3000) < 500 else s + int(rng.integers(1500, 3001))
                a, b = max(s, 0), min(e, LENGTH)
                recs.append(dict(tid=tid, pos=a, mapq=60, flag=16 * (len(recs) % 2), cigar=[(0, b - a)], seq=t[a:b], qual=[30] * (b - a),
                                 name="r%d" % len(recs), hp=None))
                s = e
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


def run(tmp, name, more, expect=0):
    d = str(tmp / ("run_%s" % name))
    argv = ["kmer_qv", "-a", str(tmp / "asm.fa"), "-b", str(tmp / "reads.bam"), "-f", str(tmp / "truth.fa"), "-o", os.path.join(d, "x"),
            "-d", "-k", str(K), "--interval", str(INTERVAL)] + more
    assert pepper.main(argv) == expect
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


@pytest.fixture(scope="module")
def chain(tmp_path_factory, hip_ctx):
    build.build_io()
    tmp = tmp_path_factory.mktemp("kmer_spectrum_chain")
    rng = np.random.default_rng(81)
    truth = [("ctgA", "".join(rng.choice(list("ACGT"), LENGTH))), ("ctgB", "".join(rng.choice(list("ACGT"), LENGTH)))]
    asm = [("ctgA", truth[0][1][:CUT[0]] + truth[0][1][CUT[1]:]), truth[1]]
    bw.write_fasta(str(tmp / "truth.fa"), truth)
    bw.write_fasta(str(tmp / "asm.fa"), asm)
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(t)) for n, t in truth], records(rng, truth))
    runs = {"plain": run(tmp, "plain", ["-t", "2"]),
            "flag": run(tmp, "flag", ["-t", "2", "--completeness", "--read_table_mb", "1"]),
            "passes": run(tmp, "passes", ["-t", "1", "--completeness", "--read_table_mb", "1", "--passes", "3"]),
            "threads": run(tmp, "threads", ["-t", "4", "--completeness", "--read_table_mb", "1", "--solid", "5"])}
    # the reader's own reads, and their k-mers
    bam, fa = bamio.BamHandler(str(tmp / "reads.bam")), bamio.FastaHandler(str(tmp / "truth.fa"))
    reads = []
    for iv in kq.read_intervals([(n, len(t)) for n, t in truth], INTERVAL):
        fb = bamio.fill_batch(bam, fa, [iv], 0, False, 1.0, 0, max_reads=kq.READ_LIMIT)
        b = fb.batch
        reads += [b.bases[int(b.base_off[r]):int(b.base_off[r + 1])].tobytes() for r in range(int(b.read_off[b.n_regions]))]
        fb.close()
    assert len(reads) > 8 * DEPTH
    return tmp, truth, asm, runs, R.read_counts(reads, K)


def _curve(text):
    return [(int(f[0]), int(f[1]), int(f[2]), f[3]) for f in (l.split("\t") for l in text.split("\n")[1:] if l)]


def test_without_the_flag_the_files_are_those_of_before(chain):
    _, truth, asm, runs, counts = chain
    names = ["x_kmer_qv" + s for s in QV_FILES] + ["x_kmer_qv_draft" + s for s in QV_FILES]
    assert sorted(runs["plain"]) == sorted(names)
    for stem, seqs in (("x_kmer_qv", asm), ("x_kmer_qv_draft", truth)):
        contigs, nm, ln = [t.encode() for _, t in seqs], [n for n, _ in seqs], [len(t) for _, t in seqs]
        ctg, seg_off, segs, rr, hist, _ = R.support(contigs, None, K, kq.CAP, 1, 1024, counts=counts)
        assert runs["plain"][stem + ".tsv"] == kq.contig_text(nm, ln, ctg, K)[0]
        assert runs["plain"][stem + ".segments.tsv"] == kq.segment_text(nm, ln, seg_off, segs, 1024)
        assert runs["plain"][stem + ".runs.bed"] == kq.runs_text(nm, rr, K)
        assert runs["plain"][stem + ".hist.tsv"] == kq.hist_text(hist)
    # and the flag adds its two files per FASTA and changes none of the others
    assert sorted(runs["flag"]) == sorted(names + ["x_kmer_qv" + s for s in MORE_FILES] + ["x_kmer_qv_draft" + s for s in MORE_FILES])
    assert all(runs["flag"][f] == runs["plain"][f] for f in names)


def test_passes_and_reader_threads_write_the_same_bytes(chain):
    runs = chain[3]
    assert runs["flag"] == runs["passes"] == runs["threads"]


def test_the_draft_is_complete_and_the_assembly_is_not(chain):
    runs = chain[3]
    draft = _curve(runs["flag"]["x_kmer_qv_draft.completeness.tsv"])
    assert len(draft) > 10 and [s for s, _, _, _ in draft] == list(range(1, len(draft) + 1))
    assert all(total == found > 0 and share == "1.000000" for _, total, found, share in draft)
    got = _curve(runs["flag"]["x_kmer_qv.completeness.tsv"])
    s2 = got[1]
    assert s2[0] == 2 and s2[2] < s2[1] and float(s2[3]) < 1.0
    # about 2 kb of 40 are missing, less the k-mers across the interval edges, which no read holds
    assert 1900 <= s2[1] - s2[2] <= 2000 + K and 0.94 < float(s2[3]) < 0.96
    spectrum = runs["flag"]["x_kmer_qv_draft.spectrum.tsv"].split("\n")
    assert spectrum[0] == kq.SPECTRUM_HEADER[:-1] and len(spectrum) == 258
    assert all(l.split("\t")[1] == "0" for l in spectrum[1:257])   # the reads hold nothing the truth lacks


def test_the_curve_is_the_restatements_on_the_readers_reads(chain):
    _, truth, asm, runs, counts = chain
    for stem, seqs in (("x_kmer_qv", asm), ("x_kmer_qv_draft", truth)):
        ro, sp = S.spectrum([t.encode() for _, t in seqs], None, K, kq.CAP, counts=counts)
        assert runs["flag"][stem + ".spectrum.tsv"] == kq.spectrum_text(ro, sp)
        assert runs["flag"][stem + ".completeness.tsv"] == kq.completeness_text(ro, sp)
        held = S.asm_keys([t.encode() for _, t in seqs], K)
        lost = sorted(c for x, c in counts.items() if x not in held)   # the counts of the read k-mers this FASTA lacks
        curve = _curve(runs["flag"][stem + ".completeness.tsv"])
        assert len(curve) == max(counts.values())
        for s, total, found, _ in curve:
            assert total - found == sum(1 for c in lost if c >= s), s


def test_a_table_too_small_ends_with_status_2(chain, capsys):
    tmp = chain[0]
    capsys.readouterr()
    files = run(tmp, "small", ["-t", "2", "--completeness", "--read_table_mb", "0.012"], expect=2)
    err = capsys.readouterr().err
    assert "--read_table_mb" in err and "--passes" in err and "dropped" in err and "1024 slots" in err
    assert not [f for f in files if "completeness" in f]
    # more passes make the same table do: a tenth of the 2 k lost k-mers at a time fits
    assert run(tmp, "small10", ["-t", "2", "--completeness", "--read_table_mb", "0.012", "--passes", "10"]) == chain[3]["flag"]
