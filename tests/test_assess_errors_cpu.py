"""assess --errors / -q without a device: the restatement of the error list and the calibration table
(tests/assess_errors_ref.py) against hand-worked answers, the patch property, the count identities, the FASTQ reader's refusals,
the text of the two tables, and what the command refuses before it opens a context."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assess_errors_cases as X  # noqa: E402
import assess_errors_ref as E  # noqa: E402
import assess_ref as R  # noqa: E402

from pepper_thesis_amd import assess, pepper  # noqa: E402

L, SHIFT = 256, 64
SMALL = [n for n in sorted(X.CASES) if n != "many_segments"]


def rec_tuple(r):
    return tuple(int(r[f]) for f in E.ERR_FIELDS)


def test_hand_worked_single_errors():
    t = b"GA" + X.rnd(1, 196) + b"CT"
    q = ((np.arange(200) * 7) % 94).astype(np.uint8)
    # one substitution at 50
    a = bytearray(t)
    a[50] = X.other(t[50])[0]
    recs, hist, tot, _ = E.errors_pair(bytes(a), t, L, SHIFT, q)
    assert [rec_tuple(r) for r in recs] == [(50, 50, 0, 0, E.SUB, a[50], t[50], 0, int(q[50]))]
    assert hist[:, 0].sum() == 200 and hist[int(q[50]), 1] == 1 and hist[:, 1:].sum() == 1
    # one insertion at 70, of a base that differs from both neighbours
    x = X.other(t[69], t[70])
    recs, hist, _, _ = E.errors_pair(t[:70] + x + t[70:], t, L, SHIFT, np.append(q, 9).astype(np.uint8))
    assert [rec_tuple(r) for r in recs] == [(70, 70, 0, 0, E.INS, x[0], 0, 0, int(q[70]))]
    assert hist[:, 0].sum() == 201 and hist[int(q[70]), 2] == 1
    # the first base missing: a_pos = 0, only Q[0] exists beside it
    recs, hist, _, _ = E.errors_pair(t[1:], t, L, SHIFT, q[:199])
    assert [rec_tuple(r) for r in recs] == [(0, 0, 0, 0, E.DEL, 0, ord("G"), 0, int(q[0]))]
    # the last base missing: a_pos = n_A, only Q[n_A - 1] exists beside it
    recs, hist, _, _ = E.errors_pair(t[:-1], t, L, SHIFT, q[:199])
    assert [rec_tuple(r) for r in recs] == [(199, 199, 0, 0, E.DEL, 0, ord("T"), 0, int(q[198]))]
    assert hist[:, 0].sum() == 199 and hist[int(q[198]), 3] == 1
    # a deletion inside: the weaker neighbour is charged
    while t[100] in (t[99], t[101]):
        t = t[:100] + X.other(t[99], t[101]) + t[101:]
    recs, _, _, _ = E.errors_pair(t[:100] + t[101:], t, L, SHIFT, q[:199])
    assert [rec_tuple(r) for r in recs] == [(100, 100, 0, 0, E.DEL, 0, t[100], 0, int(min(q[99], q[100])))]
    # without qualities: 255 and no table
    recs, hist, _, _ = E.errors_pair(t[:100] + t[101:], t, L, SHIFT, None)
    assert hist is None and [r["qual"] for r in recs] == [255]
    # an empty assembly: quality 0 for every deletion
    recs, hist, _, _ = E.errors_pair(b"", b"ACGT", L, SHIFT, np.zeros(0, np.uint8))
    assert [(r["a_pos"], r["b_pos"], r["qual"]) for r in recs] == [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0)] and hist[0, 3] == 4


def test_hand_worked_errors_next_to_an_anchor():
    t = X.rnd(31, 600)
    assert R.chain(R.find_anchors(t, t, L, SHIFT)) == [(256, 256), (512, 512)]
    q = ((np.arange(600) * 7) % 94).astype(np.uint8)
    a = bytearray(t)
    a[255], a[288] = X.other(t[255])[0], X.other(t[288])[0]   # the last base before the anchor and the first one behind it
    recs, hist, tot, _ = E.errors_pair(bytes(a), t, L, SHIFT, q)
    assert [rec_tuple(r) for r in recs] == [(255, 255, 0, 0, E.SUB, a[255], t[255], 0, int(q[255])),
                                            (288, 288, 0, 1, E.SUB, a[288], t[288], 0, int(q[288]))]
    assert hist[:, 0].sum() == 600   # the anchors' 64 bytes are counted
    # the base before the anchor missing: the anchor is found one column further, the deletion stands before assembly 255
    while t[255] in (t[254], t[256]):
        t = t[:255] + X.other(t[254], t[256]) + t[256:]
    recs, _, _, _ = E.errors_pair(t[:255] + t[256:], t, L, SHIFT, q[:599])
    assert [rec_tuple(r) for r in recs] == [(255, 255, 0, 0, E.DEL, 0, t[255], 0, int(min(q[254], q[255])))]


@pytest.mark.parametrize("name", SMALL)
def test_patch_property_and_identities(name):
    pairs, quals, shift, rows, off, hist = X.expected(name)
    _, _, totals = X.totals_of(pairs, shift)
    assert len(rows) == totals[:, 5:8].sum()
    for p, (A, B) in enumerate(pairs):
        r = rows[off[p]:off[p + 1]]
        recs = [dict(zip(E.ERR_FIELDS, (int(v) for v in x))) for x in r]
        if totals[p, 2] == 0:
            assert E.apply_errors(A, recs) == B, (name, p)
        # the counts of assess_ref, walked independently
        assert [(r[:, 4] == k).sum() for k in (E.SUB, E.INS, E.DEL)] == list(totals[p, 5:8]), (name, p)
        assert hist[p, :, 0].sum() == totals[p, 4] + totals[p, 5] + totals[p, 6]
        assert list(hist[p, :, 1:].sum(axis=0)) == list(totals[p, 5:8])
        for k in (E.SUB, E.INS, E.DEL):
            assert np.array_equal(np.bincount(r[r[:, 4] == k, 8], minlength=E.QBINS), hist[p, :, k])
        assert (r[:, 2] == p).all()


def test_quality_above_93_counts_as_93():
    t = X.rnd(3, 100)
    a = bytearray(t)
    a[10] = X.other(t[10])[0]
    recs, hist, _, _ = E.errors_pair(bytes(a), t, L, SHIFT, np.full(100, 200, np.uint8))
    assert recs[0]["qual"] == 93 and hist[93, 0] == 100 and hist[93, 1] == 1


# ---- the FASTQ reader ----------------------------------------------------------------------------------------------------

ASM = [("c1", b"ACGTAC"), ("c2", b"ggT"), ("empty", b"")]
GOOD = b"@c1 words\nACGTAC\n+\n!~5555\n@c2\nGGt\n+c2\nIII\n"


@pytest.mark.parametrize("reader,err", [(E.read_fastq, E.FastqError), (assess.read_fastq, assess.AssessError)])
def test_fastq_reader_and_its_refusals(tmp_path, reader, err):
    p = tmp_path / "x.fq"
    p.write_bytes(GOOD)
    got = reader(str(p), ASM)
    assert sorted(got) == ["c1", "c2"] and got["c1"].tolist() == [0, 93, 20, 20, 20, 20] and got["c2"].tolist() == [40, 40, 40]
    assert got["c1"].dtype == np.uint8
    p.write_bytes(GOOD + b"@empty\n\n+\n\n")
    assert sorted(reader(str(p), ASM)) == ["c1", "c2", "empty"]
    bad = {"four lines": (GOOD[:-4], "c2"),                                       # the last record has no quality line
           "plus": (GOOD.replace(b"+c2", b"-c2"), "c2"),
           "length": (GOOD.replace(b"III", b"II"), "c2"),
           "byte": (GOOD.replace(b"III", b"I I"), "c2"),                          # a blank is below '!'
           "byte above": (GOOD.replace(b"III", b"I\x7fI"), "c2"),
           "twice": (GOOD + b"@c1\nACGTAC\n+\nIIIIII\n", "c1"),
           "differs": (GOOD.replace(b"ACGTAC", b"ACGTAA"), "c1"),
           "missing": (GOOD[:GOOD.index(b"@c2")], "c2")}
    for what, (text, name) in bad.items():
        p.write_bytes(text)
        with pytest.raises(err) as e:
            reader(str(p), ASM)
        assert name in str(e.value), (what, str(e.value))


# ---- the text of the tables ----------------------------------------------------------------------------------------------

def test_table_text_from_fixed_records():
    recs = [dict(a_pos=5, b_pos=6, pair=0, segment=0, kind=E.SUB, a_base=ord("A"), b_base=ord("C"), hp=0, qual=12),
            dict(a_pos=9, b_pos=10, pair=0, segment=1, kind=E.INS, a_base=ord("T"), b_base=0, hp=1, qual=255),
            dict(a_pos=30, b_pos=30, pair=0, segment=2, kind=E.DEL, a_base=0, b_base=ord("G"), hp=0, qual=0)]
    want = ["ctg\tsub\t5\t6\tA\tC\t0\t12\t0\n", "ctg\tins\t9\t10\tT\t.\t1\t.\t1\n", "ctg\tdel\t30\t30\t.\tG\t0\t0\t2\n"]
    assert [E.error_line("ctg", r) for r in recs] == want and [assess.error_line("ctg", r) for r in recs] == want
    assert E.ERRORS_HEADER == assess.ERRORS_HEADER == "#name\tkind\tassembly_pos\ttruth_pos\tassembly_base\ttruth_base\thp\tqual\tsegment\n"
    assert E.CALIBRATION_HEADER == assess.CALIBRATION_HEADER == ("#name\tqual\tbases\tsubstitutions\tinsertions\tdeletions\terrors\t"
                                                                 "columns\tobserved_QV\n")
    hist = np.zeros((E.QBINS, 4), np.int64)
    hist[5] = [90, 4, 3, 10]      # 17 errors in 100 columns: QV 7.70
    hist[40] = [100000, 0, 0, 0]
    hist[93] = [0, 0, 0, 1]       # a deletion charged to a quality no base carries
    want = "c\t5\t90\t4\t3\t10\t17\t100\t7.70\nc\t40\t100000\t0\t0\t0\t0\t100000\tinf\nc\t93\t0\t0\t0\t1\t1\t1\t0.00\n"
    assert E.calibration_lines("c", hist) == want and assess.calibration_lines("c", hist) == want
    # from 5 up: 18 errors in 100101 columns, QV 37.45 >= 5
    assert E.calibrated_from(hist) == 5 and assess.calibrated_from(hist) == 5
    hist[5] = [1, 1, 0, 0]
    hist[40] = [10, 5, 0, 0]      # QV 3 at every threshold, and QV 0 at 93
    assert E.calibrated_from(hist) is None and assess.calibrated_from(hist) is None
    assert E.calibrated_from(np.zeros((E.QBINS, 4), np.int64)) is None


def test_parser_has_the_new_options():
    a = pepper.parser().parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x"])
    assert a.errors is False and a.fastq is None
    a = pepper.parser().parse_args(["assess", "-a", "p.fa", "-t", "t.fa", "-o", "x", "--errors", "-q", "p.fq"])
    assert a.errors is True and a.fastq == "p.fq"
    assert pepper.parser().parse_args(["assess", "-a", "p", "-t", "t", "-o", "x", "--fastq", "y"]).fastq == "y"


def test_pack_launches_counts_the_error_scratch():
    sizes = [1000, 1000, 5000, 10, 0, 3000]
    need = lambda n: assess.direction_bytes(n, 256) + assess.error_bytes(n, 256)  # noqa: E731
    assert assess.error_bytes(1000, 256) == 4 * (8 + 8 + 94 * 16) and assess.error_bytes(0, 256) == 1520
    b = need(1000) * 2
    assert assess.pack_launches(sizes, 256, b, errors=True) == [[0, 1], [2], [3, 4], [5]]
    assert assess.pack_launches(sizes, 256, b - 1, errors=True) == [[0], [1], [2], [3, 4], [5]]
    # the same budget packs two pairs without the error pass, and no longer with it
    b0 = assess.direction_bytes(1000, 256) * 2
    assert assess.pack_launches(sizes[:2], 256, b0) == [[0, 1]] and assess.pack_launches(sizes[:2], 256, b0, errors=True) == [[0], [1]]


def test_error_scratch_helper_covers_the_packing_estimate():
    from pepper_thesis_amd import _ffi
    lib = _ffi.load()
    for sizes in ([0], [255], [256], [1000, 0, 70000], [5_000_000]):
        off = np.zeros(len(sizes) + 1, np.int64)
        off[1:] = np.cumsum(sizes)
        got = int(lib.pv_assess_errors_scratch_bytes(len(sizes), off.ctypes.data, 256))
        plain = int(lib.pv_assess_scratch_bytes(len(sizes), off.ctypes.data, 256))
        extra = sum(assess.error_bytes(n, 256) for n in sizes)
        assert plain + extra <= got <= plain + extra + 8 + 3 * 256, (sizes, got, plain, extra)
    assert lib.pv_assess_errors_scratch_bytes(-1, None, 256) < 0 and lib.pv_assess_errors_scratch_bytes(1, None, 256) < 0


def test_record_layout():
    from pepper_thesis_amd import _ffi
    dt = np.dtype(_ffi.pv_assess_error)
    assert dt.itemsize == 32 and [dt.fields[f][1] for f in ("a_pos", "b_pos", "pair", "segment", "kind", "a_base", "b_base", "hp",
                                                            "qual", "pad")] == [0, 8, 16, 20, 24, 25, 26, 27, 28, 29]
    assert (_ffi.PV_ASSESS_ERR_SUB, _ffi.PV_ASSESS_ERR_INS, _ffi.PV_ASSESS_ERR_DEL, _ffi.PV_ASSESS_QBINS) == (1, 2, 3, 94)


# ---- the command ---------------------------------------------------------------------------------------------------------

def _fa(path, recs):
    with open(path, "w") as fh:
        for n, s in recs:
            fh.write(">%s\n%s\n" % (n, s))
    return str(path)


def test_fastq_problems_exit_2_before_a_context_is_opened(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import runtime

    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(runtime, "Context", no_context)
    p = _fa(tmp_path / "p.fa", [("c1", "ACGTACGT")])
    out = str(tmp_path / "o")
    assert pepper.main(["assess", "-a", p, "-t", p, "-o", out, "-q", str(tmp_path / "none.fq")]) == 2
    assert "cannot find the FASTQ" in capsys.readouterr().err
    fq = tmp_path / "p.fq"
    fq.write_text("@c1\nACGTACGA\n+\nIIIIIIII\n")
    assert pepper.main(["assess", "-a", p, "-t", p, "-o", out, "-q", str(fq), "--errors"]) == 2
    err = capsys.readouterr().err
    assert "ERROR: assess" in err and "c1" in err and "differs" in err
    assert not any(f.startswith("o_") for f in os.listdir(str(tmp_path)))
