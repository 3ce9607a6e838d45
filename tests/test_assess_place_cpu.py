"""CPU: the placement rule's restatement (tests/assess_place_ref.py) on cases whose answer is written out, the options and the
parser of `assess --place`, and the composing of pairs and tables with the rule's restatements in the context's place."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_errors_ref as E  # noqa: E402
import assess_place_cases as X  # noqa: E402
import assess_place_ref as P  # noqa: E402
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import _ffi, assess, pepper  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule -----------------------------------------------------------------------------------------------------------------

def test_keys_by_hand():
    assert P.key_of(b"A" * 32) == 0 and P.key_of(b"A" * 31 + b"C") == 1 and P.key_of(b"T" * 32) == (1 << 64) - 1
    assert P.key_of(b"C" + b"A" * 31) == 1 << 62 and P.key_of(b"A" * 31 + b"N") is None and P.key_of(b"a" * 32) is None
    assert P.rc_key(P.key_of(b"A" * 31 + b"C")) == P.key_of(b"G" + b"T" * 31)
    k = X.rnd(5, 32)
    assert P.rc_key(P.key_of(k)) == P.key_of(P.revcomp(k)) and P.rc_key(P.rc_key(P.key_of(k))) == P.key_of(k)
    pal = b"ACGTTGCAACGTTGCA"
    assert P.key_of(pal + P.revcomp(pal)) == P.rc_key(P.key_of(pal + P.revcomp(pal)))
    assert P.revcomp(b"AACGTN") == b"NACGTT"


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_the_rule_on_cases_with_written_answers(name):
    """every case carries its answer (its check); expected() runs it"""
    asm, truth, step, min_hits, recs = X.expected(name)
    assert recs.shape == (len(asm), 8)
    unplaced = recs[:, X.STATUS] == P.UNPLACED
    assert (recs[unplaced, :4] == -1).all() and (recs[~unplaced, X.TRUTH] >= 0).all()
    assert (recs[:, X.AGREE] <= recs[:, X.HITS]).all() and (recs[:, X.HITS] <= recs[:, X.TRIED]).all()


def test_one_contig_by_hand():
    """truth t of 200 bases; the contig is t[40:140] with step 32: samples at 0, 32, 64 -> j = 40, 72, 104; its reverse
    complement has the same three hits on the other strand, a' = 68 - a"""
    t = X.rnd(7, 200)
    index = P.truth_index([t])
    assert P.place_one(t[40:140], [t], index, 32, 3) == (40, 140, 0, 0, P.PLACED, 3, 3, 3)
    assert P.place_one(P.revcomp(t[40:140]), [t], index, 32, 3) == (40, 140, 0, 1, P.PLACED, 3, 3, 3)
    assert P.place_one(t[40:140], [t], index, 32, 4) == (-1, -1, -1, -1, P.UNPLACED, 3, 3, 3)
    # equal counts on (0, forward) and (1, forward): whichever wins the tie, 2 H > N fails
    u = X.rnd(8, 200)
    assert P.place_one(t[:64] + u[:64], [t, u], P.truth_index([t, u]), 32, 1) == (-1, -1, -1, -1, P.UNPLACED, 4, 4, 2)
    # a second copy of the truth makes every 32-mer occur twice: tried, no hit
    assert P.place_one(t[40:140], [t, t], P.truth_index([t, t]), 32, 1) == (-1, -1, -1, -1, P.UNPLACED, 3, 0, 0)


# ---- constants, record, options, parser ---------------------------------------------------------------------------------------

def test_constants_and_record_layout_follow_the_header():
    hdr = open(os.path.join(ROOT, "include", "pepper_hip.h")).read()
    for name in ("PV_ASSESS_PLACE_TILE", "PV_ASSESS_PLACE_MAX_TRUTH", "PV_ASSESS_PLACED", "PV_ASSESS_UNPLACED", "PV_ASSESS_MISPLACED"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_ffi, name), name
    assert _ffi.PV_ASSESS_PLACE_TILE == X.TILE and _ffi.PV_ASSESS_PLACE_MAX_TRUTH >= 8192
    assert (_ffi.PV_ASSESS_PLACED, _ffi.PV_ASSESS_UNPLACED, _ffi.PV_ASSESS_MISPLACED) == (P.PLACED, P.UNPLACED, P.MISPLACED)
    dt = np.dtype(_ffi.pv_assess_placement)
    assert dt.itemsize == 40 and dt.names == P.REC_FIELDS
    assert [dt.fields[f][1] for f in dt.names] == [0, 8, 16, 20, 24, 28, 32, 36]


def test_option_checks():
    for step in (32, 64, 1024, 65536):
        assess.check_place_options(step, 3)
    for step in (0, 31, 48, 65568, -32):
        with pytest.raises(assess.AssessError, match="--place_step"):
            assess.check_place_options(step, 3)
    for hits in (1, 65535):
        assess.check_place_options(1024, hits)
    for hits in (0, -1, 65536):
        with pytest.raises(assess.AssessError, match="--min_hits"):
            assess.check_place_options(1024, hits)


def test_parser():
    ap = pepper.parser()
    a = ap.parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x"])
    assert (a.place, a.place_step, a.min_hits) == (False, None, None)
    a = ap.parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x", "--place"])
    assert (a.place, a.place_step, a.min_hits) == (True, None, None)
    assert (assess.DEFAULT_PLACE_STEP, assess.DEFAULT_MIN_HITS) == (1024, 3)
    a = ap.parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x", "--place", "--place_step", "64", "--min_hits", "7"])
    assert (a.place, a.place_step, a.min_hits) == (True, 64, 7)
    assert "rearrangement" in pepper.assess_parser().format_help()


@pytest.mark.parametrize("extra", [["--place_step", "64"], ["--min_hits", "2"], ["--place", "--place_step", "48"],
                                   ["--place", "--min_hits", "0"], ["--place", "--place_step", "65568"]])
def test_refused_flags_exit_2_before_a_context_is_opened(tmp_path, capsys, monkeypatch, extra):
    from pepper_thesis_amd import runtime

    def no_context(*a, **k):
        raise AssertionError("no context expected")
    monkeypatch.setattr(runtime, "Context", no_context)
    p = X.write_fasta(tmp_path / "p.fa", [("c", b"ACGT")])
    assert pepper.main(["assess", "-a", p, "-t", p, "-o", str(tmp_path / "o")] + extra) == 2
    assert "ERROR: assess" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "o") + "_assess.tsv")


# ---- pairs and tables, with the restatements where the context stands ---------------------------------------------------------

class RefDevice:
    """stands where runtime.Context stands: every call by its rule's restatement"""

    def __init__(self, *a):
        self.placed = []

    def close(self):
        pass

    def assess(self, pairs, segment, max_shift):
        rows, off, totals = R.assess_batch(pairs, segment, max_shift)
        segs = np.zeros(len(rows), np.dtype(_ffi.pv_assess_seg))
        for k, f in enumerate(R.SEG_FIELDS):
            segs[f] = rows[:, k]
        return segs, off, totals

    def assess_errors(self, pairs, quals, segment, max_shift):
        segs, off, totals = self.assess(pairs, segment, max_shift)
        rows, eoff, hist = E.errors_batch(pairs, segment, max_shift, quals)
        errs = np.zeros(len(rows), np.dtype(_ffi.pv_assess_error))
        for k, f in enumerate(E.ERR_FIELDS):
            errs[f] = rows[:, k]
        return segs, off, totals, errs, eoff, hist

    def assess_place(self, asm, truth, step, min_hits):
        self.placed.append((len(asm), len(truth), step, min_hits))
        rows = P.place(asm, truth, step, min_hits)
        recs = np.zeros(len(rows), np.dtype(_ffi.pv_assess_placement))
        for k, f in enumerate(P.REC_FIELDS):
            recs[f] = rows[:, k]
        return recs


def test_rows_are_oriented_sliced_and_keep_their_qualities():
    s = X.command_scenario()
    dev = RefDevice()
    rows, recs = assess.place_rows(dev, s["asm"], s["truth"], 64, 3, s["quals"])
    assert dev.placed == [(5, 2, 64, 3)]   # one call: the whole assembly against the whole truth
    hand_a, hand_t = dict(s["hand_asm"]), dict(s["hand_truth"])
    for name, status, a, b, shift, q in rows:
        if name == "junk":
            assert (status, b, shift, q) == ("unplaced", None, 0, None) and a == hand_a["junk"]
            continue
        assert (status, a, b, shift) == ("paired", hand_a[name], hand_t[name], s["where"][name][2]), name
        assert np.array_equal(q, s["hand_quals"][name]) and q.flags.c_contiguous
    want = {n: (tn, "+-"[strand], lo, hi) for n, (tn, strand, lo, hi) in s["where"].items()}
    text = assess.placement_text(s["asm"], s["truth"], recs)
    assert text == X.placement_table(s["asm"], s["truth"], P.place([R.upper(a) for _, a in s["asm"]], [R.upper(b) for _, b in s["truth"]], 64, 3))
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert lines[0] == ["#name", "status", "truth", "strand", "truth_start", "truth_end", "samples", "hits", "agreeing"]
    for f in lines[1:]:
        if f[0] == "junk":
            assert f[1:6] == ["unplaced", ".", ".", ".", "."] and f[7:] == ["0", "0"]
        else:
            assert (f[1], (f[2], f[3], int(f[4]), int(f[5]))) == ("placed", want[f[0]])
    assert assess.truth_cover(s["truth"], recs) == (500, 100)   # chrB [0, 500) bare, chrB [2400, 2500) twice


def test_truth_cover_interval_arithmetic():
    recs = np.zeros(5, np.dtype(_ffi.pv_assess_placement))
    for k, (t, lo, hi, st) in enumerate([(0, 10, 50, 0), (0, 40, 60, 0), (0, 45, 48, 0), (1, 0, 30, 0), (1, 0, 30, 2)]):
        recs[k] = (lo, hi, t, 0, st, 0, 0, 0)
    assert assess.truth_cover([("a", b"A" * 100), ("b", b"C" * 30), ("c", b"G" * 7)], recs) == (50 + 0 + 7, 10)


def test_command_with_place_gives_the_hand_paired_tables(tmp_path, capsys, monkeypatch):
    """`assess --place --errors -q` on the assembler's contigs = plain `assess --errors -q` on the same contigs oriented and
    paired by hand with their exact truth slices, line for line after the name and offset mapping"""
    from pepper_thesis_amd import runtime
    monkeypatch.setattr(runtime, "Context", RefDevice)
    s = X.command_scenario()
    fa, fq = X.write_fasta, X.write_fastq
    up = lambda recs: [(n, R.upper(x)) for n, x in recs]   # noqa: E731
    common = ["--segment", "256", "--max_shift", "64", "--errors"]
    placed, hand = str(tmp_path / "placed"), str(tmp_path / "hand")
    assert pepper.main(["assess", "-a", fa(tmp_path / "asm.fa", s["asm"]), "-t", fa(tmp_path / "truth.fa", s["truth"]), "-o", placed,
                        "-q", fq(tmp_path / "asm.fq", up(s["asm"]), s["quals"]), "-d", fa(tmp_path / "draft.fa", s["asm"][:3]),
                        "--place", "--place_step", "64"] + common) == 0
    err = capsys.readouterr().err
    assert "contig junk of the assembly is unplaced" in err and "contig junk of the draft is unplaced" in err
    assert "truth: 500 bases lie in no placed interval of the assembly, 100 in more than one" in err
    assert pepper.main(["assess", "-a", fa(tmp_path / "hand.fa", s["hand_asm"]), "-t", fa(tmp_path / "hand_truth.fa", s["hand_truth"]),
                        "-o", hand, "-q", fq(tmp_path / "hand.fq", up(s["hand_asm"]), s["hand_quals"])] + common) == 0
    read = lambda p: open(p).read()   # noqa: E731
    where = s["where"]
    assert read(placed + "_assess.tsv") == X.shift_column(read(hand + "_assess.tsv"), (), where, "unplaced")
    assert read(placed + "_assess.segments.tsv") == X.shift_column(read(hand + "_assess.segments.tsv"), (4, 5), where)
    assert read(placed + "_assess.errors.tsv") == X.shift_column(read(hand + "_assess.errors.tsv"), 3, where)
    assert read(placed + "_assess.calibration.tsv") == read(hand + "_assess.calibration.tsv")
    assert len(read(placed + "_assess.errors.tsv").splitlines()) > 20
    # TOTAL is the sum of the contigs' lines
    rows = [ln.split("\t") for ln in read(placed + "_assess.tsv").splitlines()[1:]]
    assert rows[-1][:2] == ["TOTAL", "total"] and [r[1] for r in rows[:-1]] == ["paired", "paired", "unplaced", "paired", "paired"]
    for c in range(2, 16):
        assert int(rows[-1][c]) == sum(int(r[c]) for r in rows[:-1] if r[1] == "paired"), c
    truth_up = [R.upper(b) for _, b in s["truth"]]
    assert read(placed + "_assess.placement.tsv") == X.placement_table(s["asm"], s["truth"], P.place([a for _, a in up(s["asm"])], truth_up, 64, 3))
    assert read(placed + "_assess_draft.placement.tsv") == X.placement_table(s["asm"][:3], s["truth"],
                                                                             P.place([a for _, a in up(s["asm"][:3])], truth_up, 64, 3))
    assert sorted(os.listdir(str(tmp_path))) == sorted(
        ["asm.fa", "asm.fq", "draft.fa", "hand.fa", "hand.fq", "hand_truth.fa", "truth.fa"] +
        ["hand_assess" + x for x in (".tsv", ".segments.tsv", ".errors.tsv", ".calibration.tsv")] +
        ["placed_assess" + x for x in (".tsv", ".segments.tsv", ".errors.tsv", ".calibration.tsv", ".placement.tsv", "_draft.tsv",
                                       "_draft.errors.tsv", "_draft.placement.tsv")])
    # without --place the assembler's names pair with nothing: status 2, as before
    assert pepper.main(["assess", "-a", str(tmp_path / "asm.fa"), "-t", str(tmp_path / "truth.fa"), "-o", str(tmp_path / "plain")]) == 2
    assert "no contig name occurs in both files" in capsys.readouterr().err


def test_no_contig_placed_is_status_2(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import runtime
    monkeypatch.setattr(runtime, "Context", RefDevice)
    a = X.write_fasta(tmp_path / "a.fa", [("c1", X.rnd(1, 300)), ("c2", b"ACGT")])
    t = X.write_fasta(tmp_path / "t.fa", [("c1", X.rnd(2, 300))])
    assert pepper.main(["assess", "-a", a, "-t", t, "-o", str(tmp_path / "o"), "--place", "--place_step", "32"]) == 2
    err = capsys.readouterr().err
    assert "contig c1 of the assembly is unplaced" in err and "no contig of the assembly could be placed" in err
    assert not os.path.exists(str(tmp_path / "o") + "_assess.tsv")


def test_too_many_truth_contigs_and_long_contigs_are_refused():
    class NoDevice:
        pass

    class Long(bytes):
        def __len__(self):
            return 1 << 31
    with pytest.raises(assess.AssessError, match="at most 8192"):
        assess.place_rows(NoDevice(), [("c", b"A")], [("t%d" % k, b"A") for k in range(8193)], 1024, 3)
    with pytest.raises(assess.AssessError, match="2\\^31"):
        assess.place_rows(NoDevice(), [("c", b"A")], [("t", Long(b"A"))], 1024, 3)
