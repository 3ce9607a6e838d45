"""CPU: the polisher's per-base quality without a device: the library's threshold table against numpy, the host checker
(tests/qual_ref.py) on hand-worked rows, the --qualities option on every command that takes it, the multi-device refusal,
the FASTQ writer, and the prediction files `stitch --qualities` refuses."""
import os

import numpy as np
import pytest

import qual_ref as qr
import stitch_ref as sr
from pepper_thesis_amd import _ffi, build, cli, pepper, polish, polish_steps
from pepper_thesis_amd.hdf5io import H5File, PolishImageStore, PolishPredictionStore

L = 1000
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _ffi.load()


def test_library_thresholds_equal_numpy_bit_for_bit(lib):
    want = np.float32(10.0 ** (-np.arange(1, 94) / 10.0))
    got = np.array([lib.pv_polish_qual_threshold(k) for k in range(1, 94)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(qr.T.view(np.uint32), want.view(np.uint32))
    assert (np.diff(got) < 0).all()                      # strictly decreasing: the count is the largest k that passes
    assert lib.pv_polish_qual_threshold(0) == 1.0 and lib.pv_polish_qual_threshold(94) == 0.0
    assert lib.pv_polish_qual_threshold(-1) == 0.0


def _one_row(label, value, row):
    """a [1, L] chunk whose row `row` has `value` under `label`; -> its quality"""
    labels = np.zeros((1, L), np.uint8)
    acc = np.zeros((1, L, 5), np.float32)
    labels[0, row] = label
    acc[0, row, label] = value
    return int(qr.row_qual(labels, acc)[0, row])


def test_checker_on_hand_worked_values():
    # cnt = 2 (row 500): err = 1 - acc / 2
    assert _one_row(1, f32(1.0), 500) == 3        # err 0.5: T[3] = 0.5012 >= 0.5 > T[4] = 0.3981
    assert _one_row(2, f32(1.8), 500) == 9        # float32(0.9) = 0.89999998, err = 0.10000002 > T[10] = 0.100000001
    assert _one_row(3, f32(2.0), 500) == 93       # err 0
    assert _one_row(4, f32(0.0), 500) == 0        # err 1 > T[1]
    # cnt = 1 (row 10): err = 1 - acc
    assert _one_row(1, f32(0.5), 10) == 3
    assert _one_row(1, f32(0.9), 10) == 9
    assert _one_row(1, f32(0.99), 10) == 20       # float32(0.99) = 0.99000001, err = 0.0099999905 <= T[20] = 0.0099999998
    assert _one_row(0, f32(1.0), 10) == 93
    assert _one_row(0, f32(1.0) - f32(2.0 ** -24), 10) == 72   # the smallest err > 0: 5.96e-8, T[72] = 6.31e-8, T[73] = 5.01e-8
    assert _one_row(2, np.nextafter(f32(1.0), f32(2.0)), 10) == 93   # acc a hair over cnt: err < 0
    assert _one_row(2, f32(np.nan), 10) == 0
    assert _one_row(2, f32(np.nan), 500) == 0


def test_checker_on_threshold_boundaries():
    """acc exactly on the T[k] * cnt boundaries for k = 1, 10, 20, 93 and one float32 ulp to either side, err = 0, err < 0 and
    NaN, under both counts: the vectorised checker against the definition worked with Python floats, and what must hold at
    a boundary whatever the rounding"""
    rows = qr.threshold_rows()
    assert len(rows) == 2 * (4 * 3 + 4)
    for cnt, row in ((1.0, 20), (2.0, 300)):
        mine = [r for r in rows if r[2] == cnt]
        got = [_one_row(lb, v, row) for lb, v, _, _ in mine]
        assert got == [q for _, _, _, q in mine], cnt
        for i, k in enumerate((1, 10, 20)):
            lo, mid, hi = got[3 * i:3 * i + 3]     # acc one ulp below, on, one ulp above (1 - T[k]) * cnt
            assert lo <= mid <= hi and k - 1 <= lo and hi <= k + 1 and mid in (k - 1, k), (cnt, k, lo, mid, hi)
        lo, mid, hi = got[9:12]                    # k = 93: T[93] = 5e-10 is below float32's spacing at 1, so acc rounds to cnt
        assert (mid, hi) == (93, 93) and lo == 72   # one ulp below cnt: err = 2^-24 under either count
    # err is exactly T[k] where 1 - T[k] is a float32 (k = 10 is not; build one from a power of two instead)
    assert _one_row(1, f32(0.75), 20) == 6 and qr.T[5] >= 0.25 > qr.T[6]   # err 0.25: T[6] = 0.2512 >= 0.25 > T[7] = 0.1995


def test_checker_count_boundaries():
    """acc = 1 under the label on every row: err = 0 where one window covers the row, 0.5 where two do"""
    labels = np.tile(np.arange(5, dtype=np.uint8), L // 5)[None]
    acc = np.zeros((1, L, 5), np.float32)
    acc[0, np.arange(L), labels[0]] = 1.0
    q = qr.row_qual(labels, acc)[0]
    assert q[[0, 49, 50, 949, 950, 999]].tolist() == [93, 93, 3, 3, 93, 93]
    assert (q[:50] == 93).all() and (q[50:950] == 3).all() and (q[950:] == 93).all()
    assert qr.row_counts().tolist() == [1.0] * 50 + [2.0] * 900 + [1.0] * 50
    labels[0, 7] = 255                                    # a poisoned label: quality 0
    assert qr.row_qual(labels, acc)[0, 7] == 0


def test_checker_stitch_of_a_quality_plane():
    """two chunks sharing 50 columns, different qualities on them: chunk "1" (last in string order) wins; label 0 gives no
    byte; the sequence is stitch_ref's"""
    pos = np.stack([np.arange(0, 1000), np.arange(950, 1950)])
    idx = np.zeros((2, L), np.int64)
    lab = np.ones((2, L), np.uint8)
    lab[0, 100] = 0
    lab[1, 10] = 0           # position 960: dropped although chunk 0 calls a base there
    rq = np.stack([np.full(L, 10, np.uint8), np.full(L, 20, np.uint8)])
    seq, q = qr.create_consensus_qual(qr.regions_with_qual(pos, idx, [0, 0], [0, 1], lab, rq, [(0, 2000)]))
    assert seq == sr.create_consensus_sequence(sr.regions_from_chunks(pos, idx, [0, 0], [0, 1], lab, [(0, 2000)]))
    assert len(seq) == 1950 - 2 and q == bytes([10] * 949 + [20] * 999)
    assert qr.fastq_text({"c2": ("AC", bytes([0, 93])), "c10": ("", b""), "c1": ("G", bytes([40]))}) == b"@c1\nG\n+\nI\n@c2\nAC\n+\n!~\n"


def test_qualities_option_parses_on_every_command():
    base = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]
    assert cli.polish_parser().parse_args(base + ["--qualities"]).qualities is True
    assert cli.polish_parser().parse_args(base).qualities is False
    ap = pepper.parser()
    assert ap.parse_args(["polish"] + base + ["--qualities", "--bf16", "--realign", "--gpu_decode"]).qualities is True
    assert ap.parse_args(["call_consensus", "-i", "i", "-m", "m", "-o", "o", "--qualities"]).qualities is True
    assert ap.parse_args(["call_consensus", "-i", "i", "-m", "m", "-o", "o"]).qualities is False
    assert ap.parse_args(["stitch", "-i", "i", "-o", "o", "--qualities"]).qualities is True
    assert ap.parse_args(["stitch", "-i", "i", "-o", "o"]).qualities is False
    args = ap.parse_args(["call_consensus", "-i", "i", "-m", "m", "-o", "o", "--qualities", "-d_ids", "0,0"])
    assert "--qualities" in polish_steps.consensus_argv(args)    # the ranks of a multi-device call_consensus get it too


def test_polish_qualities_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)

    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "--qualities", "-d_ids", "0,1"])
    assert polish.run(args, open_chain=open_chain) == 2
    err = capsys.readouterr().err
    assert "--qualities runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_fastq_writer_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    seqs = {c: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for c, n in (("ctg10", 70), ("ctg2", 1), ("ctg1", 0), ("x", 300))}
    quals = {c: bytes(rng.integers(0, 94, len(s), dtype=np.uint8)) for c, s in seqs.items()}
    quals["x"] = bytes([0, 93]) + quals["x"][2:]
    path = str(tmp_path / "d" / "_pepper_polished.fq")
    os.makedirs(os.path.dirname(path))
    assert polish.output_fastq_path(str(tmp_path / "d" / "_pepper_polished.fa")) == path
    polish.write_fastq(path, seqs, quals)
    assert os.listdir(os.path.dirname(path)) == ["_pepper_polished.fq"]        # the temporary name is gone
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4 * 3 + 1
    got = {}
    for i in range(0, 12, 4):
        assert lines[i][:1] == b"@" and lines[i + 2] == b"+"
        got[lines[i][1:].decode()] = (lines[i + 1], bytes(v - 33 for v in lines[i + 3]))
    assert list(got) == ["ctg2", "ctg10", "x"]                                 # natural order, the empty contig left out
    assert got == {c: (seqs[c], quals[c]) for c in got}
    assert got["x"][1][:2] == bytes([0, 93]) and lines[11][:2] == b"!~"
    # the same contigs and sequences as the FASTA
    polish.write_fasta(str(tmp_path / "d" / "p.fa"), seqs)
    fa = open(str(tmp_path / "d" / "p.fa"), "rb").read().split(b"\n")
    assert [l[1:] for l in fa[0:-1:2]] == [l[1:] for l in lines[0:-1:4]] and fa[1:-1:2] == lines[1:-1:4]
    assert open(path, "rb").read() == qr.fastq_text({c: (seqs[c].decode(), quals[c]) for c in seqs})
    # qualities that do not fit the bases: nothing is left behind
    bad = str(tmp_path / "d" / "bad.fq")
    for q in (quals["ctg10"][:-1], bytes([94]) + quals["ctg10"][1:]):
        with pytest.raises(ValueError):
            polish.write_fastq(bad, seqs, dict(quals, ctg10=q))
        assert not os.path.exists(bad) and not os.path.exists(bad + ".partial")


class _QualCaller:
    """labels and row qualities from the image alone"""

    def p2_labels(self, images):
        return (images[:, :, 0].astype(np.int64) * 7 + images[:, :, 9]) % 5

    def p2_labels_and_qualities(self, images):
        return self.p2_labels(images), (images[:, :, 1] % 94).astype(np.uint8)

    def close(self):
        pass


def test_call_consensus_qualities_writes_row_qualities_as_phred_score(tmp_path):
    rng = np.random.default_rng(2)
    img = str(tmp_path / "img.hdf")
    images = rng.integers(0, 255, (3, L, 10), dtype=np.uint8)
    with PolishImageStore(img, "w") as s:
        for cid in range(3):
            s.write_chunk("c", 0, 2900, cid, images[cid], np.arange(950 * cid, 950 * cid + L), np.zeros(L))
    for flag, out in ((True, str(tmp_path / "q.hdf")), (False, str(tmp_path / "t.hdf"))):
        assert polish_steps.call_share([img], out, _QualCaller(), 2, flag) == 3
        with PolishPredictionStore(out) as s:
            for cid in range(3):
                lab = s.read_chunk("c", "c-0-2900", str(cid))["bases"]
                ph = s.read_phred("c", "c-0-2900", str(cid))
                assert ph.dtype == np.uint8 and ph.shape == (L,)
                assert np.array_equal(lab, _QualCaller().p2_labels(images[cid:cid + 1])[0])
                want = (images[cid, :, 1] % 94) if flag else polish_steps.phred_scores(lab[None])[0]
                assert np.array_equal(ph, want), (flag, cid)


def _prediction_dir(tmp_path, name, phred0, phred1):
    """two chunks of one region; phred None: the dataset is left out"""
    pred = str(tmp_path / name)
    os.makedirs(pred)
    with H5File(os.path.join(pred, "p.hdf"), "w") as f:
        base = "predictions/c/c-0-1900/"
        f.write(base + "contig_start", 0)
        f.write(base + "contig_end", 1900)
        for cid, ph in ((0, phred0), (1, phred1)):
            f.write(base + "%d/position" % cid, np.arange(950 * cid, 950 * cid + L, dtype=np.int64))
            f.write(base + "%d/index" % cid, np.zeros(L, np.int64))
            f.write(base + "%d/bases" % cid, np.ones(L, np.uint8))
            if ph is not None:
                f.write(base + "%d/phred_score" % cid, ph)
    return pred


@pytest.mark.parametrize("case,phred,what", [("missing", None, "no phred_score"), ("short", np.zeros(999, np.uint8), "[999]"),
                                             ("wide", np.zeros(L, np.int32), "int32"), ("2d", np.zeros((L, 1), np.uint8), "[1000, 1]")])
def test_stitch_qualities_refuses_unusable_phred_score(tmp_path, capsys, case, phred, what):
    pred = _prediction_dir(tmp_path, case, np.zeros(L, np.uint8), phred)
    out = str(tmp_path / ("out_" + case))

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the device is not reached")
    args = pepper.parser().parse_args(["stitch", "-i", pred, "-o", out, "--qualities"])
    assert polish_steps.stitch_run(args, NoDevice()) == 1
    err = capsys.readouterr().err
    assert "p.hdf" in err and "c/c-0-1900/1" in err and what in err and "phred_score" in err
    assert not os.path.exists(out + "_pepper_polished.fa") and not os.path.exists(out + "_pepper_polished.fq")


def test_stitch_layout_carries_row_qualities(tmp_path):
    ph = [np.arange(L, dtype=np.int64).astype(np.uint8) % 94, np.full(L, 7, np.uint8)]
    pred = _prediction_dir(tmp_path, "ok", ph[0], ph[1])
    by = polish_steps.gather_regions(polish_steps.hdf_files(pred))
    (lay,) = list(polish_steps.stitch_layouts(by["c"], qualities=True))
    assert lay.row_qual.dtype == np.uint8 and np.array_equal(lay.row_qual, np.stack(ph))
    (plain,) = list(polish_steps.stitch_layouts(by["c"]))
    assert plain.row_qual is None and np.array_equal(plain.labels, lay.labels)
