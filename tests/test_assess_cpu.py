"""`pepper assess` without a device: the rule's restatement (tests/assess_ref.py) against a full-matrix Levenshtein distance,
the parser and what the command refuses, the text of the tables, the FASTA reader and the launch packing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import assess, pepper  # noqa: E402

L, SHIFT = 256, 64


def planted(seed, n):
    """a truth of n random bases with a homopolymer run every 150, and an assembly with sparse planted edits (about 1.2 %):
    substitutions, deletions and insertions at least 40 apart, every third indel inside a homopolymer run. -> (assembly,
    truth, planted homopolymer insertions, planted homopolymer deletions)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n)
    for p in range(100, n - 10, 150):
        t[p:p + 5] = t[p]
    truth = bytes(b"ACGT"[x] for x in t)
    out, pos, k, hp_i, hp_d = [], 0, 0, 0, 0
    while pos < n:
        step = int(rng.integers(40, 130))
        nxt = min(n, pos + step)
        out.append(truth[pos:nxt])
        pos = nxt
        if pos >= n - 40:
            out.append(truth[pos:])
            break
        kind = k % 3
        k += 1
        if kind == 0:      # substitution
            out.append(bytes([b"ACGT"[(b"ACGT".index(truth[pos]) + 1 + int(rng.integers(0, 3))) % 4]]))
            pos += 1
        elif kind == 1:    # the assembly lacks a truth base
            if k % 2 == 0:
                run = 100 + 150 * ((pos - 100) // 150 + 1)
                if run + 5 < n - 40:
                    out.append(truth[pos:run + 2])
                    pos = run + 2
                    hp_d += 1
            pos += 1
        else:              # the assembly holds a base the truth lacks
            if k % 2 == 0:
                run = 100 + 150 * ((pos - 100) // 150 + 1)
                if run + 5 < n - 40:
                    out.append(truth[pos:run + 2])
                    pos = run + 2
                    out.append(truth[pos:pos + 1])
                    hp_i += 1
                    continue
            out.append(bytes([b"ACGT"[(b"ACGT".index(truth[pos]) + 2) % 4]]))
    return b"".join(out), truth, hp_i, hp_d


SEEDS = [(1, 1000), (2, 1500), (3, 2000), (4, 2600), (5, 3000), (6, 1234), (7, 2999), (8, 777 + 1024)]


@pytest.mark.parametrize("seed,n", SEEDS)
def test_sparse_edits_give_the_edit_distance(seed, n):
    a, t, hp_i, hp_d = planted(seed, n)
    segs, tot = R.assess_pair(a, t, L, SHIFT)
    lev = R.levenshtein(a, t)
    print("seed %d: n_A %d n_B %d segments %d S+I+D %d levenshtein %d hp_ins %d/%d hp_del %d/%d" % (
        seed, len(a), len(t), tot["segments"], tot["sub"] + tot["ins"] + tot["del"], lev, tot["hp_ins"], hp_i, tot["hp_del"], hp_d))
    assert lev > 0
    assert tot["sub"] + tot["ins"] + tot["del"] == lev
    assert tot["unaligned"] == 0 and tot["edge"] == 0 and tot["aligned"] == tot["segments"] >= n // L
    assert tot["match"] + tot["sub"] + tot["ins"] == len(a) and tot["match"] + tot["sub"] + tot["del"] == len(t)
    assert tot["hp_ins"] >= hp_i and tot["hp_del"] >= hp_d and hp_i + hp_d > 0
    assert tot["hp_ins"] <= tot["ins"] and tot["hp_del"] <= tot["del"]


def test_levenshtein_itself():
    assert R.levenshtein(b"kitten", b"sitting") == 3
    assert R.levenshtein(b"", b"ACG") == 3 and R.levenshtein(b"ACG", b"") == 3 and R.levenshtein(b"", b"") == 0
    assert R.levenshtein(b"ACGT", b"ACGT") == 0 and R.levenshtein(b"AAAA", b"TTTT") == 4


def test_homopolymer_rule():
    # one A too many in a run of the truth's: an insertion that equals a neighbour; one C too few: a deletion that does
    t = b"GATTACAGGCTAAAAACGTCCCCCGTAGCATCGACTAGCTAGGCTA"
    a = t.replace(b"AAAAA", b"AAAAAA").replace(b"CCCCC", b"CCCC")
    r = R.align_segment(a, t, 0, 0, len(a), len(t))
    assert (r["ins"], r["hp_ins"], r["del"], r["hp_del"], r["sub"]) == (1, 1, 1, 1, 0)
    # an inserted base that equals neither neighbour, a deleted one that differs from both
    a = t.replace(b"GATTACA", b"GATGTACA").replace(b"CGTAGC", b"CGAGC")
    r = R.align_segment(a, t, 0, 0, len(a), len(t))
    assert (r["ins"], r["hp_ins"], r["del"], r["hp_del"], r["sub"]) == (1, 0, 1, 0, 0)


def test_band_limits_in_the_rule():
    rng = np.random.default_rng(11)
    a = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 200))
    extra = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 97))
    assert R.align_segment(a, a + extra[:96], 0, 0, 200, 296)["status"] == R.SEG_ALIGNED
    assert R.align_segment(a, a + extra, 0, 0, 200, 297)["status"] == R.SEG_UNALIGNED
    assert R.align_segment(a + extra[:96], a, 0, 0, 296, 200)["status"] == R.SEG_ALIGNED
    assert R.align_segment(a + extra, a, 0, 0, 297, 200)["status"] == R.SEG_UNALIGNED


# ---- the command ---------------------------------------------------------------------------------------------------------

def test_parser_defaults_and_flags():
    ap = pepper.parser()
    a = ap.parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "out/x"])
    assert (a.sub_command, a.assembly, a.truth, a.output, a.draft) == ("assess", "p.fa", "t.fa", "out/x", None)
    assert (a.segment, a.max_shift, a.device_id) == (1024, 8192, 0)
    a = ap.parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x", "-d", "d.fa", "--segment", "512", "--max_shift", "100",
                       "-d_id", "3"])
    assert (a.draft, a.segment, a.max_shift, a.device_id) == ("d.fa", 512, 100, 3)
    with pytest.raises(SystemExit) as e:
        ap.parse_args(["assess", "-a", "p.fa", "-o", "x"])
    assert e.value.code == 2
    help_text = pepper.assess_parser().format_help()
    assert "colinear" in help_text and "reverse complement" in help_text


def _fa(path, recs):
    with open(path, "w") as fh:
        for n, s in recs:
            fh.write(">%s\n%s\n" % (n, s))
    return str(path)


@pytest.mark.parametrize("extra", [["--segment", "250"], ["--segment", "128"], ["--segment", "65568"], ["--segment", "1000"],
                                   ["--max_shift", "31"], ["--max_shift", "1048577"]])
def test_refused_options_exit_2(tmp_path, capsys, extra):
    p = _fa(tmp_path / "p.fa", [("c", "ACGT")])
    rc = pepper.main(["assess", "-a", p, "-t", p, "-o", str(tmp_path / "o")] + extra)
    assert rc == 2
    assert "ERROR: assess" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "o") + "_assess.tsv")


def test_missing_file_and_no_pair_exit_2(tmp_path, capsys):
    p = _fa(tmp_path / "p.fa", [("c1", "ACGT")])
    t = _fa(tmp_path / "t.fa", [("c2", "ACGT")])
    assert pepper.main(["assess", "-a", str(tmp_path / "none.fa"), "-t", t, "-o", str(tmp_path / "o")]) == 2
    assert "cannot find" in capsys.readouterr().err

    class NoDevice:   # pairing is decided before anything is asked of the device
        def assess(self, *a, **k):
            raise AssertionError("no launch expected")
    with pytest.raises(assess.AssessError, match="no contig name"):
        assess.tables(NoDevice(), assess.read_fasta(p), assess.read_fasta(t), 1024, 8192)


def test_contig_of_2_31_bytes_is_refused():
    class Long(bytes):
        def __len__(self):
            return 1 << 31

    class NoDevice:
        pass
    with pytest.raises(assess.AssessError, match="2\\^31"):
        assess.tables(NoDevice(), [("c", Long(b"A"))], [("c", b"A")], 1024, 8192)


class RefDevice:
    """stands where runtime.Context stands: Context.assess by the rule's restatement"""

    def assess(self, pairs, segment, max_shift):
        from pepper_thesis_amd import _ffi
        rows, off, totals = R.assess_batch(pairs, segment, max_shift)
        segs = np.zeros(len(rows), np.dtype(_ffi.pv_assess_seg))
        for k, f in enumerate(R.SEG_FIELDS):
            segs[f] = rows[:, k]
        return segs, off, totals


def test_table_text_inf_dot_and_unpaired():
    rng = np.random.default_rng(5)
    s = "".join("ACGT"[x] for x in rng.integers(0, 4, 700))
    asm = [("same", s.encode()), ("onlyA", b"ACGTACGT"), ("empty", b""), ("err", (s[:300] + "T" + s[300:]).lower().encode())]
    truth = [("err", s.encode()), ("same", s.lower().encode()), ("empty", b""), ("onlyT", b"ACG")]
    contig, seg, total = assess.tables(RefDevice(), asm, truth, 256, 64)
    exp_contig, exp_seg = R.tables(asm, truth, 256, 64)
    assert contig == exp_contig and seg == exp_seg
    lines = {ln.split("\t")[0]: ln.rstrip("\n").split("\t") for ln in contig.splitlines()}
    assert contig.splitlines()[0].startswith("#name\tstatus") and contig.splitlines()[-1].startswith("TOTAL\ttotal")
    assert [ln.split("\t")[0] for ln in contig.splitlines()[1:]] == ["same", "onlyA", "empty", "err", "onlyT", "TOTAL"]
    assert lines["same"][1] == "paired" and lines["same"][-2:] == ["1.000000", "inf"] and lines["same"][4:9] == ["700", "700", "0", "0", "0"]
    assert lines["empty"][1] == "paired" and lines["empty"][-2:] == [".", "."] and lines["empty"][4] == "0"
    assert lines["onlyA"][1:4] == ["unpaired", "8", "0"] and lines["onlyA"][-2:] == [".", "."]
    assert lines["onlyT"][1:4] == ["unpaired", "0", "3"]
    assert lines["err"][6:9] == ["0", "1", "0"] and lines["err"][-1] == "%.2f" % (-10 * np.log10(1 / 701))
    assert lines["TOTAL"][2:4] == ["1401", "1400"] and lines["TOTAL"][7] == "1"
    assert total["ins"] == 1 and total["segments"] == 3 + 1 + 3
    assert len(seg.splitlines()) == 1 + 7 and seg.splitlines()[1].split("\t")[:6] == ["same", "0", "0", "256", "0", "256"]


def test_read_fasta(tmp_path):
    p = tmp_path / "x.fa"
    p.write_bytes(b">c1 some words\nACGT\nacgtn\n\n>empty\n>c3\tdesc\r\nNNNN\r\nAC\n>last")
    recs = assess.read_fasta(str(p))
    assert recs == [("c1", b"ACGTacgtn"), ("empty", b""), ("c3", b"NNNNAC"), ("last", b"")]
    assert assess.upper(recs[0][1]) == b"ACGTACGTN" and assess.upper(b"a[z{`@") == b"A[Z{`@"
    dup = tmp_path / "dup.fa"
    dup.write_bytes(b">a\nAC\n>a\nGT\n")
    with pytest.raises(assess.AssessError, match="twice"):
        assess.read_fasta(str(dup))
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n>a\nAC\n")
    with pytest.raises(assess.AssessError, match="before the first"):
        assess.read_fasta(str(bad))


def test_write_is_renamed_into_place(tmp_path):
    p = str(tmp_path / "t.tsv")
    assess.write_text(p, "x\n")
    assert open(p).read() == "x\n" and os.listdir(str(tmp_path)) == ["t.tsv"]


def test_pack_launches():
    need = assess.direction_bytes
    assert need(1000, 256) == 32 * 1000 + 256 * 4 and need(0, 256) == 256
    assert assess.pack_launches([], 256, 1000) == []
    sizes = [1000, 1000, 5000, 10, 0, 3000]
    b = need(1000, 256) * 2
    assert assess.pack_launches(sizes, 256, b) == [[0, 1], [2], [3, 4], [5]]           # 5000 and 3000 alone exceed it
    assert assess.pack_launches(sizes, 256, b - 1) == [[0], [1], [2], [3, 4], [5]]     # one byte short of two
    assert assess.pack_launches(sizes, 256, 1 << 40) == [[0, 1, 2, 3, 4, 5]]
    assert assess.pack_launches(sizes, 256, 0) == [[i] for i in range(6)]
    assert assess.pack_launches([1 << 30], 1024) == [[0]]                                # beyond the default budget: alone
    for launch in assess.pack_launches(sizes, 256, b):
        assert len(launch) == 1 or sum(need(sizes[i], 256) for i in launch) <= b


def test_scratch_helper_matches_the_packing_estimate():
    from pepper_thesis_amd import _ffi
    lib = _ffi.load()
    for sizes in ([0], [255], [256], [1000, 0, 70000], [5_000_000]):
        off = np.zeros(len(sizes) + 1, np.int64)
        off[1:] = np.cumsum(sizes)
        got = int(lib.pv_assess_scratch_bytes(len(sizes), off.ctypes.data, 256))
        dirs = sum(assess.direction_bytes(n, 256) for n in sizes)
        slots = sum(n // 256 + 1 for n in sizes)
        assert dirs <= got <= dirs + 48 * slots + 24 * len(sizes) + 5 * 256 + 8, (sizes, got, dirs)
    assert lib.pv_assess_scratch_bytes(-1, None, 256) < 0 and lib.pv_assess_scratch_bytes(1, None, 256) < 0
