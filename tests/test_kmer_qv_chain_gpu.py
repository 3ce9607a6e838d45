"""GPU: `polish --vote` then `pepper kmer_qv -d` on a 20 kb truth with a draft of planted substitutions, one inserted base
and two deleted bases, and 30x clean reads: the draft's runs point at every planted error, the polished assembly has no
unsupported k-mer, the tables are those of the rule's restatement fed with what the host reader returns, and the number of
reader threads changes no byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_writer as bw  # noqa: E402
import kmer_qv_ref as R  # noqa: E402

from pepper_thesis_amd import bamio, build, cli, pepper, polish  # noqa: E402
from pepper_thesis_amd import kmer_qv as kq  # noqa: E402

pytestmark = pytest.mark.gpu
K, LENGTH, DEPTH = 21, 20_000, 30


def _other(rng, b):
    return str(rng.choice([c for c in "ACGT" if c != b]))


class Planted:
    """a truth T and a draft D as alignment columns (t, d): substitutions, one base only the draft holds, two bases it lacks,
    none of them in or beside a homopolymer"""

    def __init__(self, rng):
        self.T = "".join(rng.choice(list("ACGT"), LENGTH))

        def quiet(i):   # no two equal neighbours around i
            return all(self.T[j] != self.T[j + 1] for j in range(i - 3, i + 5))
        free = [next(i for i in range(at, at + 1000) if quiet(i)) for at in range(300, LENGTH - 1500, 1500)]
        assert len(free) == 13
        self.sub_t, ins_t, del_t = free[:10], free[10], free[11]
        self.aln = []
        for i, t in enumerate(self.T):
            if i in (del_t, del_t + 1):
                self.aln.append((t, None))                    # the draft lacks these two bases
                continue
            self.aln.append((t, _other(rng, t) if i in self.sub_t else t))
            if i == ins_t:
                extra = next(c for c in "ACGT" if c not in (t, self.T[i + 1]))
                self.aln.append((None, extra))                # a base only the draft holds
        self.D = "".join(d for _, d in self.aln if d is not None)
        d_at = np.cumsum([d is not None for _, d in self.aln]) - 1
        a_of_t = np.flatnonzero([t is not None for t, _ in self.aln])
        self.d_at, self.a_of_t = d_at, a_of_t
        self.subs = [int(d_at[a_of_t[i]]) for i in self.sub_t]      # draft columns
        self.inserted = int(d_at[a_of_t[ins_t]]) + 1                 # the draft column of the extra base
        self.junction = int(d_at[a_of_t[del_t - 1]])                 # the draft column before the missing bases

    def records(self, rng):
        recs, n = [], len(self.T)
        for p in range(DEPTH):
            s = 0 if p == 0 else -int(rng.integers(0, 1500))
            while s < n - 60:
                e = n if n - (s + 3000) < 500 else s + int(rng.integers(1500, 3001))
                a, b = max(s, 0), min(e, n)
                cols = self.aln[int(self.a_of_t[a]):int(self.a_of_t[b - 1]) + 1]
                while cols and None in cols[0]:
                    a, cols = a + (cols[0][0] is not None), cols[1:]
                while cols and None in cols[-1]:
                    cols = cols[:-1]
                cigar = []
                for t, d in cols:
                    op = 0 if t is not None and d is not None else 1 if d is None else 2
                    if cigar and cigar[-1][0] == op:
                        cigar[-1][1] += 1
                    else:
                        cigar.append([op, 1])
                seq = "".join(t for t, _ in cols if t is not None)
                first = next(i for i in range(int(self.a_of_t[a]), len(self.aln)) if self.aln[i][1] is not None)
                recs.append(dict(tid=0, pos=int(self.d_at[first]), mapq=60, flag=16 * (len(recs) % 2), cigar=[(o, l) for o, l in cigar],
                                 seq=seq, qual=[30] * len(seq), name="r%d" % len(recs), hp=None))
                s = e
        recs.sort(key=lambda r: r["pos"])
        return recs


@pytest.fixture(scope="module")
def chain(tmp_path_factory, hip_ctx):
    """the files, the polished FASTA of `polish --vote`, and two kmer_qv runs with different reader threads"""
    build.build_io()
    tmp = tmp_path_factory.mktemp("kmer_qv_chain")
    rng = np.random.default_rng(71)
    pl = Planted(rng)
    bw.write_fasta(str(tmp / "draft.fa"), [("ctg", pl.D)])
    bw.write_bam(str(tmp / "reads.bam"), [("ctg", len(pl.D))], pl.records(rng))

    def open_chain(device, shared, state_dict, dtype, **k):
        return polish._DeviceChain(hip_ctx, **k)
    out_dir = str(tmp / "vote")
    argv = ["-b", str(tmp / "reads.bam"), "-f", str(tmp / "draft.fa"), "-t", "3", "-bs", "8", "-o", out_dir, "--vote"]
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=open_chain) == 0
    polished = os.path.join(out_dir, "_pepper_polished.fa")
    # "one": the contig read as one interval; 1 and 4: cut into intervals of 6000 bases (the read k-mers across their edges are
    # not counted), with one and with four reader threads
    runs = {}
    for name, more in (("one", ["-t", "2"]), (1, ["--interval", "6000", "-t", "1"]), (4, ["--interval", "6000", "-t", "4"])):
        d = str(tmp / ("run_%s" % name))
        argv = ["kmer_qv", "-a", polished, "-b", str(tmp / "reads.bam"), "-f", str(tmp / "draft.fa"), "-o", os.path.join(d, "x"), "-d",
                "-k", str(K)] + more
        assert pepper.main(argv) == 0
        runs[name] = {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}
    return tmp, pl, polished, runs


def _bed(text):
    return [(f[0], int(f[1]), int(f[2]), int(f[3]), f[4], f[5]) for f in (l.split("\t") for l in text.split("\n")[1:] if l)]


def test_the_files_and_the_reader_threads(chain):
    _, _, _, runs = chain
    stems = ["x_kmer_qv" + s for s in (".hist.tsv", ".runs.bed", ".segments.tsv", ".tsv")]
    assert sorted(runs[1]) == sorted(runs["one"]) == sorted(stems + [s.replace("x_kmer_qv", "x_kmer_qv_draft") for s in stems])
    assert runs[1] == runs[4]


def test_the_drafts_runs_point_at_every_planted_error(chain):
    _, pl, _, runs = chain
    bed = _bed(runs["one"]["x_kmer_qv_draft.runs.bed"])
    cores = [(int(c0), int(c1)) for _, _, _, _, c0, c1 in bed if c0 != "."]
    for p in pl.subs:
        assert any(c0 <= p < c1 for c0, c1 in cores), p
    for p in (pl.inserted, pl.junction, pl.junction + 1):
        assert any(s <= p < e for _, s, e, _, _, _ in bed), p
    assert len(bed) == 12 and ("ctg", pl.subs[0] - K + 1, pl.subs[0] + K, K, str(pl.subs[0]), str(pl.subs[0] + 1)) in bed
    total = runs["one"]["x_kmer_qv_draft.tsv"].split("\n")[2].split("\t")
    assert total[0] == "TOTAL" and int(total[4]) == sum(b[3] for b in bed) == 10 * K + K + (K - 1)


def test_the_polished_assembly_has_no_unsupported_kmer(chain):
    _, pl, polished, runs = chain
    assert dict(kq.read_fasta(polished)) == {"ctg": pl.T.encode()}
    lines = runs["one"]["x_kmer_qv.tsv"].split("\n")
    assert lines[1].split("\t") == ["ctg", str(LENGTH), str(LENGTH - K + 1), str(LENGTH - K + 1), "0", "0", "0.000e+00", "inf"]
    assert _bed(runs["one"]["x_kmer_qv.runs.bed"]) == []
    # cut into intervals, the k-mers across the three interval edges have no read k-mer: what the documentation says
    cut = _bed(runs[1]["x_kmer_qv.runs.bed"])
    assert 1 <= len(cut) <= 3 and all(any(s < edge < e for edge in (6000, 12000, 18000)) for _, s, e, _, _, _ in cut)


def test_the_tables_are_the_restatements_on_the_readers_reads(chain):
    tmp, pl, polished, runs = chain
    bam, fa = bamio.BamHandler(str(tmp / "reads.bam")), bamio.FastaHandler(str(tmp / "draft.fa"))
    reads = []
    for iv in kq.read_intervals([("ctg", len(pl.D))], 6000):
        fb = bamio.fill_batch(bam, fa, [iv], 0, False, 1.0, 0, max_reads=kq.READ_LIMIT)
        b = fb.batch
        reads += [b.bases[int(b.base_off[r]):int(b.base_off[r + 1])].tobytes() for r in range(int(b.read_off[b.n_regions]))]
        fb.close()
    assert len(reads) > 4 * DEPTH and max(len(r) for r in reads) <= 6010
    counts = R.read_counts(reads, K)
    for stem, seq in (("x_kmer_qv", pl.T), ("x_kmer_qv_draft", pl.D)):
        ctg, seg_off, segs, rr, hist, _ = R.support([seq.encode()], None, K, kq.CAP, 1, 1024, counts=counts)
        assert runs[1][stem + ".tsv"] == kq.contig_text(["ctg"], [len(seq)], ctg, K)[0]
        assert runs[1][stem + ".segments.tsv"] == kq.segment_text(["ctg"], [len(seq)], seg_off, segs, 1024)
        assert runs[1][stem + ".runs.bed"] == kq.runs_text(["ctg"], rr, K)
        assert runs[1][stem + ".hist.tsv"] == kq.hist_text(hist)
