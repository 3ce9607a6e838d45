"""CPU: the hash of the completeness rule at its vectors, the slot sizing of --read_table_mb, the refusals of the options, the
two texts and the completeness curve from hand-made tables, and the rule's restatement (tests/kmer_spectrum_ref.py) on a worked
example."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmer_qv_ref as R  # noqa: E402
import kmer_spectrum_ref as S  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402
from pepper_thesis_amd import kmer_qv as kq  # noqa: E402
from pepper_thesis_amd import pepper  # noqa: E402

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def test_the_mix_vectors():
    assert S.mix(0) == 0
    assert S.mix(1) == 0x5692161d100b05e5
    assert S.mix(0x3fffff) == 0x4262be0542100624
    assert S.mix((1 << 62) - 1) == 0xad34157e3cb2ef5e
    assert S.part_of(1, 1) == 0 and S.part_of(1, 7) == 0x5692161d % 7 and S.home_of(1, 1024) == 0x5e5 & 1023


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pepper_hip.h")).read()
    for name in ("PV_KMER_READS_MIN_SLOTS", "PV_KMER_READS_PROBES", "PV_KMER_MAX_PARTS"):
        assert "#define %s %d\n" % (name, getattr(_ffi, name)) in hdr, name
    assert "#define PV_KMER_READS_MAX_SLOTS (1ll << 34)\n" in hdr and _ffi.PV_KMER_READS_MAX_SLOTS == 1 << 34
    assert (kq.READS_MIN_SLOTS, kq.MAX_PASSES) == (_ffi.PV_KMER_READS_MIN_SLOTS, _ffi.PV_KMER_MAX_PARTS)
    for word in ("0xbf58476d1ce4e5b9", "0x94d049bb133111eb"):
        assert word in hdr


def test_the_slots_of_read_table_mb():
    # a table is a 256-byte head and 12 bytes per slot: the largest power of two of slots that fits
    assert kq.read_slots(1024) == 1 << 26          # 2^30 / 12 = 89.5 M
    assert kq.read_slots(1) == 1 << 16             # 87 359 slots fit
    assert kq.read_slots(768.001) == 1 << 26 and kq.read_slots(768) == 1 << 25   # 2^26 slots need 768 MB and the head
    least = (256 + 12 * 1024) / (1 << 20)
    assert kq.read_slots(least) == 1024 and kq.read_slots(0.012) == 1024
    assert kq.read_slots(1.9 * least) == 1024 and kq.read_slots((256 + 12 * 2048) / (1 << 20)) == 2048
    for bad in (0, -1, 0.0117, float("nan"), float(1 << 21)):
        with pytest.raises(kq.KmerQvError):
            kq.read_slots(bad)


def test_the_options_and_their_refusals():
    assert kq.check_completeness_options(False, None, None, None) == (0, 1, 2)
    assert kq.check_completeness_options(True, None, None, None) == (1 << 26, 1, 2)
    assert kq.check_completeness_options(True, 1, 4096, 255) == (1 << 16, 4096, 255)
    for bad in ((False, 64, None, None), (False, None, 2, None), (False, None, None, 3), (True, None, 0, None), (True, None, 4097, None),
                (True, None, None, 0), (True, None, None, 256), (True, 0.001, None, None)):
        with pytest.raises(kq.KmerQvError):
            kq.check_completeness_options(*bad)


def test_the_parser_and_exit_status_2(tmp_path, capsys):
    ap = pepper.parser()
    base = ["kmer_qv", "-a", "p.fa", "-b", "r.bam", "-f", "d.fa", "-o", "out/x"]
    a = ap.parse_args(base)
    assert (a.completeness, a.read_table_mb, a.passes, a.solid) == (False, None, None, None)
    a = ap.parse_args(base + ["--completeness", "--read_table_mb", "0.5", "--passes", "3", "--solid", "4"])
    assert (a.completeness, a.read_table_mb, a.passes, a.solid) == (True, 0.5, 3, 4)
    text = " ".join(pepper.kmer_qv_parser().format_help().split())
    for word in ("error k-mers dominate reads_only at low counts", "a convention", "same interval clipping"):
        assert word in text, word
    fa = tmp_path / "d.fa"
    fa.write_text(">c\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    base = ["kmer_qv", "-a", str(fa), "-b", str(fa), "-f", str(fa), "-o", str(tmp_path / "o")]
    for extra, word in ((["--read_table_mb", "64"], "--read_table_mb is an option of --completeness"),
                        (["--passes", "2"], "--passes is an option of --completeness"),
                        (["--completeness", "--passes", "0"], "--passes 0"), (["--completeness", "--passes", "4097"], "--passes 4097"),
                        (["--completeness", "--solid", "0"], "--solid 0"), (["--completeness", "--solid", "256"], "--solid 256"),
                        (["--completeness", "--read_table_mb", "0.001"], "--read_table_mb 0.001"),
                        (["--completeness", "--read_table_mb", "-3"], "--read_table_mb -3")):
        assert pepper.main(base + extra) == 2, extra
        assert word in capsys.readouterr().err
    assert not list(tmp_path.glob("o_*"))


def test_the_texts_and_the_curve():
    ro, sp = np.zeros(256, np.int64), np.zeros((4, 256), np.int64)
    ro[[1, 2, 30, 255]] = [900, 40, 5, 1]
    sp[0, [0, 1, 29, 30]] = [7, 2, 50, 100]
    sp[1, 60], sp[3, 255] = 10, 3
    assert kq.completeness_at(ro, sp, 1) == (165 + 946, 165, "%.6f" % (165 / 1111))
    assert kq.completeness_at(ro, sp, 2) == (163 + 46, 163, "%.6f" % (163 / 209))
    assert kq.completeness_at(ro, sp, 31) == (13 + 1, 13, "%.6f" % (13 / 14))
    assert kq.completeness_at(ro, sp, 255) == (4, 3, "0.750000")
    for s in range(1, 256):
        assert kq.completeness_at(ro, sp, s)[:2] == S.completeness(ro, sp, s)
    t = kq.spectrum_text(ro, sp).split("\n")
    assert t[0] == "#count\treads_only\tasm_x1\tasm_x2\tasm_x3\tasm_x4plus" and len(t) == 258 and t[257] == ""
    assert t[1] == "0\t0\t7\t0\t0\t0" and t[2] == "1\t900\t2\t0\t0\t0" and t[31] == "30\t5\t100\t0\t0\t0"
    assert t[61] == "60\t0\t0\t10\t0\t0" and t[256] == "255+\t1\t0\t0\t0\t3"
    c = kq.completeness_text(ro, sp).split("\n")
    assert c[0] == "#solid\tread_kmers\tin_assembly\tcompleteness" and len(c) == 257
    assert c[1] == "1\t1111\t165\t%.6f" % (165 / 1111) and c[255] == "255\t4\t3\t0.750000"
    # no read k-mer at a threshold: `.`, and no line
    ro[255], sp[3, 255] = 0, 0
    assert kq.completeness_at(ro, sp, 61) == (0, 0, ".") and kq.completeness_at(ro, sp, 60) == (10, 10, "1.000000")
    c = kq.completeness_text(ro, sp).split("\n")
    assert len(c) == 62 and c[60].startswith("60\t10\t10\t")
    assert kq.completeness_text(np.zeros(256, np.int64), np.zeros((4, 256), np.int64)) == kq.COMPLETENESS_HEADER


def test_the_restatement_on_a_worked_example():
    k = 11
    u, v, w, x = b"ACGGTCATTGA", b"GGATCCTTACA", b"TTGACCAGTAG", b"CATCGGAATCT"
    assert len({R.canon(s) for s in (u, v, w, x)}) == 4
    # the assembly holds u three times (once as its reverse complement), v once; the reads hold u twice, v never, w five times
    # on both strands, x once, and a k-mer with an N, which has no key
    contigs = [u + b"N" + rc(u), v + b"N" + u]
    reads = [u, rc(u), w, rc(w), w, w, rc(w), x, b"ACGTNACGTAC", w[:k - 1]]
    ro, sp = S.spectrum(contigs, reads, k)
    assert {int(c): int(n) for c, n in enumerate(ro) if n} == {1: 1, 5: 1}
    assert {(m, c): int(sp[m, c]) for m in range(4) for c in range(256) if sp[m, c]} == {(2, 2): 1, (0, 0): 1}
    assert S.asm_keys(contigs, k) == {R.canon(u): 3, R.canon(v): 1}
    assert S.completeness(ro, sp, 1) == (3, 1) and S.completeness(ro, sp, 2) == (2, 1) and S.completeness(ro, sp, 3) == (1, 0)
    assert S.completeness(ro, sp, 6) == (0, 0)
    ro3, sp3 = S.spectrum(contigs, reads, k, cap=3)
    assert {int(c): int(n) for c, n in enumerate(ro3) if n} == {1: 1, 3: 1} and int(sp3[2, 2]) == 1
    # five copies of u in the assembly land in the row "four times or more"; a count above 255 in the last column
    ro, sp = S.spectrum([b"N".join([u] * 5)], [w] * 300 + [u] * 256, k)
    assert int(sp[3, 255]) == 1 and int(sp.sum()) == 1 and int(ro[255]) == 1 and int(ro.sum()) == 1
    # the parts split the keys, not the instances: every key's count lies in exactly one part
    whole = R.read_counts(reads, k)
    for n_parts in (1, 3, 7):
        parts = [S.part_counts(reads, k, p, n_parts) for p in range(n_parts)]
        assert sum(len(p) for p in parts) == len(whole) and all(whole[x_] == c for p in parts for x_, c in p.items())
