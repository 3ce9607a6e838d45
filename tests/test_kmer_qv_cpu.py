"""CPU: the restatement of the k-mer support rule (tests/kmer_qv_ref.py) against a brute-force quadratic count on tiny inputs;
the QV and core arithmetic, the writers, the parser and every refusal of `pepper kmer_qv`."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmer_qv_ref as R  # noqa: E402

from pepper_thesis_amd import kmer_qv as kq  # noqa: E402
from pepper_thesis_amd import pepper  # noqa: E402

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def acgt(s):
    return all(c in b"ACGT" for c in s)


def brute(contigs, reads, k, cap, min_count, segment):
    """every assembly k-mer against every read k-mer, as strings"""
    planes = []
    for a in contigs:
        v = np.full(len(a), R.NO_KEY, np.uint32)
        for i in range(len(a) - k + 1):
            x = a[i:i + k]
            if not acgt(x):
                continue
            c = sum(1 for r in reads for j in range(len(r) - k + 1) if r[j:j + k] in (x, rc(x)))
            v[i] = min(cap, c)
        planes.append(v)
    return planes


@pytest.mark.parametrize("k", [11, 13, 31])
def test_the_restatement_equals_a_brute_force_count(k):
    rng = np.random.default_rng(k)
    s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4 * k + 9).tobytes())
    contigs = [s[:2 * k + 4], b"", s[k:3 * k] + b"N" + s[3 * k:], rc(s[5:5 + k + 2]), s[:k - 1], s[:k].lower(), b"A" * (k + 2) + b"T" * k]
    reads = [s, rc(s[3:3 * k]), s[:k], s[:k - 1], b"", s[7:7 + k] + b"n" + s[7:7 + k], b"A" * (k + 1), s[:k]]
    for cap, min_count, segment in ((1 << 30, 1, 32), (3, 3, 32), (2, 1, 64)):
        planes = brute(contigs, reads, k, cap, min_count, segment)
        got = R.support(contigs, reads, k, cap, min_count, segment)
        assert np.array_equal(got[5], np.concatenate(planes))
        # the summary, straight from the definition
        for p, (a, v) in enumerate(zip(contigs, planes)):
            pos = v[:max(0, len(a) - k + 1)]
            keyed, bad = pos != R.NO_KEY, (pos != R.NO_KEY) & (pos < min_count)
            assert got[0][p].tolist() == [int(keyed.sum()), int(bad.sum()), int((~keyed).sum())]
            segs = got[2][got[1][p]:got[1][p + 1]]
            assert len(segs) == -(-len(a) // segment) and [int(x) for x in segs] == [int(bad[j:j + segment].sum()) for j in range(0, len(a), segment)]
            flags = "".join("x" if b else "." for b in bad)
            want_runs = [(p, i, i + len(m) - 1) for i, m in _runs(flags)]
            assert [tuple(r) for r in got[3].tolist() if r[0] == p] == want_runs
        every = np.concatenate([v[:max(0, len(a) - k + 1)] for a, v in zip(contigs, planes)])
        every = every[every != R.NO_KEY]
        assert got[4].tolist() == np.bincount(np.minimum(every, 255), minlength=256).tolist()
    assert R.canon(s[:k]) == R.canon(rc(s[:k])) and R.key_of(b"ACGT") == 0b00011011 and R.key_of(b"ACgT") is None
    assert [x for _, x in R.canon_keys(s, k)] == [R.canon(s[i:i + k]) for i in range(len(s) - k + 1)]


def _runs(flags):
    import re
    return [(m.start(), m.group()) for m in re.finditer("x+", flags)]


def test_error_rate_qv_and_core():
    assert kq.error_qv(0, 0, 21) == (".", ".")
    assert kq.error_qv(1000, 1000, 21) == ("0.000e+00", "inf")
    e = 1.0 - (979 / 1000) ** (1 / 21)
    assert kq.error_qv(1000, 979, 21) == ("%.3e" % e, "%.2f" % (-10 * math.log10(e)))
    assert kq.error_qv(5, 0, 11) == ("1.000e+00", "0.00")
    k = 21
    assert kq.run_core(100 - k + 1, 100, k) == (100, 101)          # a lone substitution at 100
    assert kq.run_core(50, 50 + k - 1, k) == (50 + k - 1, 50 + k)   # k k-mers: one base
    assert kq.run_core(50, 50 + k, k) is None                      # longer than k: no base is in every k-mer
    assert kq.run_core(7, 7, k) == (7, 7 + k)


def test_the_writers():
    names, lengths, k = ["a", "b", "c"], [100, 40, 0], 21
    ctg = np.array([[80, 21, 0], [15, 0, 5], [0, 0, 0]], np.int64)
    text, total = kq.contig_text(names, lengths, ctg, k)
    lines = text.split("\n")
    assert lines[0] == "#name\tlength\tkmers\tsupported\tunsupported\tno_key\terror_rate\tQV" and total == (21, 95)
    e = 1.0 - (59 / 80) ** (1 / 21)
    assert lines[1] == "a\t100\t80\t59\t21\t0\t%.3e\t%.2f" % (e, -10 * math.log10(e))
    assert lines[2] == "b\t40\t15\t15\t0\t5\t0.000e+00\tinf" and lines[3] == "c\t0\t0\t0\t0\t0\t.\t."
    assert lines[4].startswith("TOTAL\t140\t95\t74\t21\t5\t") and lines[5] == ""
    seg = kq.segment_text(names, lengths, np.array([0, 4, 6, 6]), np.array([0, 21, 0, 0, 0, 0]), 32)
    assert seg.split("\n")[1:8] == ["a\t0\t32\t0", "a\t32\t64\t21", "a\t64\t96\t0", "a\t96\t100\t0", "b\t0\t32\t0", "b\t32\t40\t0", ""]
    bed = kq.runs_text(names, np.array([[0, 40, 60], [0, 70, 95], [1, 3, 3]]), k)
    assert bed.split("\n") == ["#name\tstart\tend\tkmers\tcore_start\tcore_end", "a\t40\t81\t21\t60\t61", "a\t70\t116\t26\t.\t.",
                               "b\t3\t24\t1\t3\t24", ""]
    hist = np.zeros(256, np.int64)
    hist[[0, 30, 255]] = [21, 70, 4]
    h = kq.hist_text(hist).split("\n")
    assert h[0] == "#count\tkmers" and h[1] == "0\t21" and h[31] == "30\t70" and h[256] == "255+\t4" and len(h) == 258
    assert kq.read_intervals([("x", 2500), ("y", 0), ("z", 1000)], 1000) == [("x", 0, 1000), ("x", 1000, 2000), ("x", 2000, 2500),
                                                                             ("z", 0, 1000)]


def test_the_parser():
    ap = pepper.parser()
    a = ap.parse_args(["kmer_qv", "-a", "p.fa", "-b", "r.bam", "-f", "d.fa", "-o", "out/x"])
    assert (a.sub_command, a.assembly, a.bam, a.fasta, a.output) == ("kmer_qv", "p.fa", "r.bam", "d.fa", "out/x")
    assert (a.draft, a.kmer, a.min_count, a.segment, a.interval, a.threads, a.device_id) == (False, 21, 1, 1024, 1000000, 5, 0)
    a = ap.parse_args(["kmer_qv", "-a", "p.fa", "-b", "r.bam", "-f", "d.fa", "-o", "x", "-d", "-k", "31", "--min_count", "3", "--segment",
                       "256", "--interval", "50000", "-t", "2", "-d_id", "1"])
    assert (a.draft, a.kmer, a.min_count, a.segment, a.interval, a.threads, a.device_id) == (True, 31, 3, 256, 50000, 2, 1)
    text = pepper.kmer_qv_parser().format_help()
    for word in ("homopolymer", "coverage hole", "upper bound", "does not replace", "no value of --min_count is recommended"):
        assert word in " ".join(text.split()), word


def test_every_refusal_is_exit_status_2(tmp_path, capsys):
    fa = tmp_path / "d.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    base = ["kmer_qv", "-a", str(fa), "-b", str(fa), "-f", str(fa), "-o", str(tmp_path / "o")]
    for extra, word in ((["-k", "20"], "-k 20"), (["-k", "9"], "-k 9"), (["-k", "33"], "-k 33"), (["--min_count", "0"], "--min_count 0"),
                        (["--segment", "48"], "--segment 48"), (["--interval", "10"], "--interval 10")):
        assert pepper.main(base + extra) == 2
        assert word in capsys.readouterr().err
    for flag in ("-a", "-b", "-f"):
        argv = list(base)
        argv[argv.index(flag) + 1] = str(tmp_path / "missing")
        assert pepper.main(argv) == 2
        assert "cannot find" in capsys.readouterr().err
    assert not list(tmp_path.glob("o_*"))
    for bad in ((0, 1, 32, 1000), (21, 1 << 31, 32, 1000)):
        with pytest.raises(kq.KmerQvError):
            kq.check_options(*bad)
    kq.check_options(11, 1 << 30, 65536, 1000)


def test_no_common_contig_is_refused_before_the_device_is_opened(tmp_path, capsys):
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    seq = "ACGTTGCAAGCT" * 10
    bw.write_fasta(str(tmp_path / "d.fa"), [("ctgA", seq)])
    rec = dict(tid=0, pos=0, mapq=60, flag=0, cigar=[(0, 60)], seq=seq[:60], qual=[30] * 60, name="r", hp=None)
    bw.write_bam(str(tmp_path / "r.bam"), [("other", 120)], [rec])
    argv = ["kmer_qv", "-a", str(tmp_path / "d.fa"), "-b", str(tmp_path / "r.bam"), "-f", str(tmp_path / "d.fa"), "-o", str(tmp_path / "o")]
    assert pepper.main(argv) == 2
    assert "no contig of the BAM is in the draft FASTA" in capsys.readouterr().err


class _NoDevice:
    def kmer_table_bytes(self, a_off):
        raise AssertionError("the limit is checked before the device is asked")


def test_an_assembly_above_the_limit_is_refused():
    class Long(bytes):
        def __len__(self):
            return 1 << 30
    with pytest.raises(kq.KmerQvError) as e:
        kq.Scorer(_NoDevice(), "assembly", [("a", Long()), ("b", Long())], 21, 1024)
    assert "2^31" in str(e.value)
