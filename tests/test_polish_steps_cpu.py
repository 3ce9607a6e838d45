"""CPU: the polisher's step-by-step commands (polish_steps.py, pepper.py) without a device - the two HDF5 formats, the
phred_score table, the file -> chunk layout of `stitch` against tests/stitch_ref.py, the rejected stitch inputs, the command
line, and the multi-caller plumbing of `call_consensus -d_ids` with a stub caller. The device runs are in
test_polish_steps_gpu.py."""
import os
import sys
import time

import numpy as np
import pytest

import stitch_ref as sr
from pepper_thesis_amd import cli, pepper, polish_rank, polish_steps
from pepper_thesis_amd.hdf5io import H5S_SCALAR, H5S_SIMPLE, H5File, PolishImageStore, PolishPredictionStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 1000


def _chunk_rows(rng, start, end, inserts=0.3):
    """(position, index) rows of a region [start, end] with random insert rows, as the builder orders them"""
    pos, idx = [], []
    for p in range(start, end + 1):
        pos.append(p)
        idx.append(0)
        for k in range(int(rng.random() < inserts) * int(rng.integers(1, 4))):
            pos.append(p)
            idx.append(k + 1)
    return np.array(pos, np.int64), np.array(idx, np.int64)


def _chunks(pos, idx):
    """cut rows into chunks of L overlapping by 50; the last padded with -1 (chunk_images)"""
    out, s = [], 0
    while True:
        p, x = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
        n = min(L, len(pos) - s)
        p[:n], x[:n] = pos[s:s + n], idx[s:s + n]
        out.append((p, x))
        if s + L >= len(pos):
            return out
        s += L - 50


# ---- formats -----------------------------------------------------------------------------------------------------------

def test_image_file_layout_and_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    path = str(tmp_path / "img.hdf")
    img = rng.integers(0, 255, (L, 10), dtype=np.uint8)
    pos, idx = np.arange(100, 1100, dtype=np.int64), np.arange(L, dtype=np.int64)
    pos[-7:] = idx[-7:] = -1
    with PolishImageStore(path, "w") as s:
        s.write_chunk("ctg_1", 900, 2100, 3, img, pos, idx)
        s.write_chunk("ctg_1", 900, 2100, 3, img * 0, pos, idx)   # a name once written is kept (DataStore.write_summary)
    with H5File(path) as f:
        assert f.keys("/") == ["summaries"] and f.keys("/summaries") == ["ctg_1_900_2100_3"]
        base = "summaries/ctg_1_900_2100_3/"
        assert sorted(f.keys(base)) == ["chunk_id", "contig", "image", "index", "label", "position", "region_end", "region_start"]
        want = {"image": (np.uint8, (L, 10)), "label": (np.uint8, (L,)), "position": (np.int64, (L,)), "index": (np.int64, (L,))}
        for k, (dt, shape) in want.items():
            a = f.read(base + k)
            assert a.dtype == dt and a.shape == shape, k
            assert f.space_class(base + k) == H5S_SIMPLE, k
        for k, v in (("contig", "ctg_1"), ("region_start", 900), ("region_end", 2100), ("chunk_id", 3)):
            assert f.space_class(base + k) == H5S_SCALAR, k
            got = f.read(base + k)
            assert got == v and type(got) is (str if k == "contig" else np.int64), (k, got)   # vlen UTF-8 str / int64
        assert not f.read(base + "label").any()
    with PolishImageStore(path) as s:
        c = s.read_chunk("ctg_1_900_2100_3")
    assert (c["contig"], c["region_start"], c["region_end"], c["chunk_id"]) == ("ctg_1", 900, 2100, 3)
    assert np.array_equal(c["image"], img) and np.array_equal(c["position"], pos) and np.array_equal(c["index"], idx)


def test_prediction_file_layout_and_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    path = str(tmp_path / "pred.hdf")
    rows = {}
    with PolishPredictionStore(path, "w") as s:
        for cid in (0, 1, 10, 2):
            p, x = rng.integers(-1, 5000, L), rng.integers(-1, 3, L)
            b = rng.integers(0, 5, L, dtype=np.uint8)
            rows[cid] = (p, x, b)
            s.write_prediction("chr1", 0, 1100, cid, p, x, b, polish_steps.phred_scores(b[None])[0])
    with H5File(path) as f:
        assert f.keys("/predictions") == ["chr1"] and f.keys("/predictions/chr1") == ["chr1-0-1100"]
        base = "predictions/chr1/chr1-0-1100/"
        assert sorted(f.keys(base)) == ["0", "1", "10", "2", "contig_end", "contig_start"]
        for k, v in (("contig_start", 0), ("contig_end", 1100)):
            assert f.space_class(base + k) == H5S_SCALAR and f.read(base + k) == v and f.read(base + k).dtype == np.int64
        for cid in rows:
            assert sorted(f.keys(base + str(cid))) == ["bases", "index", "phred_score", "position"]
            for k, dt in (("position", np.int64), ("index", np.int64), ("bases", np.uint8), ("phred_score", np.uint8)):
                a = f.read(base + "%d/%s" % (cid, k))
                assert a.dtype == dt and a.shape == (L,) and f.space_class(base + "%d/%s" % (cid, k)) == H5S_SIMPLE
    with PolishPredictionStore(path) as s:
        assert s.contigs() == ["chr1"] and s.regions("chr1") == ["chr1-0-1100"]
        assert s.region_span("chr1", "chr1-0-1100") == (0, 1100)
        assert sorted(s.chunk_names("chr1", "chr1-0-1100")) == ["0", "1", "10", "2"]
        for cid, (p, x, b) in rows.items():
            c = s.read_chunk("chr1", "chr1-0-1100", str(cid))
            assert np.array_equal(c["position"], p) and np.array_equal(c["index"], x) and np.array_equal(c["bases"], b)


def test_reader_accepts_fixed_length_contig_and_int32_index(tmp_path):
    """what other h5py writers may produce: a fixed-length byte string for contig, int32 index"""
    path = str(tmp_path / "other.hdf")
    with H5File(path, "w") as f:
        base = "summaries/chrX_5_1200_0/"
        f.write(base + "image", np.ones((L, 10), np.uint8))
        f.write(base + "label", np.zeros(L, np.uint8))
        f.write(base + "position", np.arange(L, dtype=np.int64))
        f.write(base + "index", np.arange(L, dtype=np.int32))
        f.write(base + "contig", np.array(b"chrX", dtype="S4"))
        f.write(base + "region_start", 5)
        f.write(base + "region_end", 1200)
        f.write(base + "chunk_id", 0)
    with PolishImageStore(path) as s:
        c = s.read_chunk("chrX_5_1200_0")
    assert c["contig"] == "chrX" and c["index"].dtype == np.int64 and np.array_equal(c["index"], np.arange(L))
    assert (c["region_start"], c["region_end"], c["chunk_id"]) == (5, 1200, 0)


def test_phred_table_is_pinned():
    # predict_distributed_gpu.py:96-104 on labels 0..4: -10 log10(1 - label / count), inf -> 100, NaN -> 0, truncated
    assert polish_steps.PHRED_TABLE.tolist() == [[0, 100, 0, 0, 0], [0, 3, 100, 0, 0]]
    labels = np.tile(np.arange(5, dtype=np.uint8), 200)[None]
    ph = polish_steps.phred_scores(labels)[0]
    for c in range(L):
        count = 1 if c < 50 or c >= L - 50 else 2
        assert ph[c] == polish_steps.PHRED_TABLE[count - 1, labels[0, c]], c
    with np.errstate(divide="ignore", invalid="ignore"):   # the formula itself, as float32 then astype(uint8) on x86
        for count in (1, 2):
            for lab in range(5):
                v = np.float32(-10) * np.log10(np.float32(1) - np.float32(lab) / np.float32(count))
                v = 100 if np.isinf(v) else (0 if np.isnan(v) or v < 0 else int(v))
                assert polish_steps.PHRED_TABLE[count - 1, lab] == v, (count, lab)


# ---- stitch: file -> chunk layout ------------------------------------------------------------------------------------

def _write_predictions(tmp, rng, n_files=3, S=11_000):
    """regions of two contigs, each of more than 10 chunks, dealt at random over n_files files and written in shuffled
    order; -> {contig: [(start, end)]}"""
    regions = []
    for contig, n in (("ctg10", 3), ("ctg2", 4)):
        for k in range(n):
            start = 0 if k == 0 else k * S - 100
            regions.append((contig, start, (k + 1) * S + 100))
    order = rng.permutation(len(regions))
    stores = [PolishPredictionStore(os.path.join(tmp, "pepper_prediction_%d.hdf" % i), "w") for i in range(n_files)]
    for j in order:
        contig, s, e = regions[j]
        chunks = _chunks(*_chunk_rows(rng, s, e))
        assert len(chunks) > 10
        st = stores[int(rng.integers(0, n_files))]
        for cid in rng.permutation(len(chunks)):
            p, x = chunks[cid]
            b = rng.integers(0, 5, L).astype(np.uint8)
            st.write_prediction(contig, s, e, int(cid), p, x, b, polish_steps.phred_scores(b[None])[0])
    for st in stores:
        st.close()
    return regions


def _ref_regions(tmp):
    """RegionChunks of every contig, read with the generic H5File reader"""
    by = {}
    for name in sorted(os.listdir(tmp)):
        with H5File(os.path.join(tmp, name)) as f:
            for contig in f.keys("/predictions"):
                for reg in f.keys("/predictions/" + contig):
                    base = "predictions/%s/%s/" % (contig, reg)
                    rc = sr.RegionChunks(f.read(base + "contig_start"), f.read(base + "contig_end"))
                    for ch in f.keys(base):
                        if ch not in ("contig_start", "contig_end"):
                            rc.chunks[int(ch)] = tuple(f.read(base + ch + "/" + k) for k in ("position", "index", "bases"))
                    by.setdefault(contig, []).append(rc)
    return by


def test_stitch_layout_equals_host_stitch(tmp_path):
    tmp = str(tmp_path / "pred")
    os.makedirs(tmp)
    regions = _write_predictions(tmp, np.random.default_rng(5))
    by = polish_steps.gather_regions(polish_steps.hdf_files(tmp))
    assert sorted(by) == ["ctg10", "ctg2"]
    ref = _ref_regions(tmp)
    for contig, refs in by.items():
        assert [(r.start, r.end) for r in refs] == sorted((s, e) for c, s, e in regions if c == contig)
        lays = list(polish_steps.stitch_layouts(refs))
        assert len(lays) == 1
        lay = lays[0]
        # the layout pv_polish_stitch requires
        assert np.all(np.diff(lay.region) >= 0) and lay.region[0] == 0 and lay.region[-1] == len(refs) - 1
        for g in range(len(refs)):
            assert lay.chunk_id[lay.region == g].tolist() == list(range(int((lay.region == g).sum())))
        assert lay.region_start.tolist() == [r.start for r in refs]
        assert lay.position.dtype == np.int64 and lay.index.dtype == np.int32 and lay.labels.dtype == np.uint8
        assert (lay.position == -1).any()   # padding rows travel as they are
        got = sr.stitch_contigs(lay.position, lay.index, lay.region, lay.chunk_id, lay.labels,
                                [(contig, r.start, r.end) for r in refs])[contig]
        want = sr.create_consensus_sequence(ref[contig], threads=3)
        assert got == want and len(want) > 20_000
        # split launches give the same regions, at region boundaries
        small = list(polish_steps.stitch_layouts(refs, max_chunks=20))
        assert len(small) > 1 and sum(len(s.regions) for s in small) == len(refs)
        assert np.array_equal(np.concatenate([s.labels for s in small]), lay.labels)


def _stitch_args(tmp, out):
    return pepper.parser().parse_args(["stitch", "-i", tmp, "-o", out])


def test_stitch_rejects_region_in_two_files(tmp_path, capsys):
    tmp = str(tmp_path / "pred")
    os.makedirs(tmp)
    for i in range(2):
        with PolishPredictionStore(os.path.join(tmp, "p%d.hdf" % i), "w") as s:
            s.write_prediction("c", 0, 1100, 0, np.arange(L), np.zeros(L), np.ones(L), np.zeros(L))
    out = str(tmp_path / "out" / "x")
    assert polish_steps.stitch_run(_stitch_args(tmp, out)) == 1
    err = capsys.readouterr().err
    assert "c-0-1100" in err and "p0.hdf" in err and "p1.hdf" in err
    assert not os.path.exists(out + "_pepper_polished.fa") and not os.path.exists(out + "_pepper_polished.fa.partial")


def test_stitch_rejects_gap_in_chunk_ids(tmp_path, capsys):
    tmp = str(tmp_path / "pred")
    os.makedirs(tmp)
    with PolishPredictionStore(os.path.join(tmp, "p.hdf"), "w") as s:
        for cid in (0, 1, 3):
            s.write_prediction("c", 0, 3000, cid, np.arange(L), np.zeros(L), np.ones(L), np.zeros(L))
    out = str(tmp_path / "x")
    assert polish_steps.stitch_run(_stitch_args(tmp, out)) == 1
    err = capsys.readouterr().err
    assert "p.hdf" in err and "c-0-3000" in err and "gap at 2" in err
    assert not os.path.exists(out + "_pepper_polished.fa")


def test_stitch_rejects_index_beyond_int32(tmp_path, capsys):
    tmp = str(tmp_path / "pred")
    os.makedirs(tmp)
    idx = np.zeros(L, np.int64)
    idx[5] = 1 << 31
    with PolishPredictionStore(os.path.join(tmp, "p.hdf"), "w") as s:
        s.write_prediction("c", 0, 1100, 0, np.arange(L), idx, np.ones(L), np.zeros(L))
    out = str(tmp_path / "x")
    assert polish_steps.stitch_run(_stitch_args(tmp, out)) == 1
    err = capsys.readouterr().err
    assert "c-0-1100" in err and "chunk 0" in err and "int32" in err
    assert not os.path.exists(out + "_pepper_polished.fa")


# ---- the command line --------------------------------------------------------------------------------------------------

def test_every_reference_option_parses():
    p = pepper.parser()
    a = p.parse_args(["make_images", "--bam", "r.bam", "--fasta", "d.fa", "--region", "c:1-9", "--output_dir", "o", "--threads", "3"])
    assert (a.bam, a.fasta, a.region, a.output_dir, a.threads, a.realign) == ("r.bam", "d.fa", "c:1-9", "o", 3, False)
    a = p.parse_args(["make_images", "-b", "r.bam", "-f", "d.fa", "-r", "c", "-o", "o", "-t", "2", "--realign"])
    assert (a.threads, a.realign) == (2, True)
    assert p.parse_args(["make_images", "-b", "r", "-f", "f", "-o", "o"]).threads == 5
    a = p.parse_args(["call_consensus", "--image_dir", "i", "--model_path", "m", "--output_dir", "o", "--batch_size", "64", "--gpu",
                      "--device_ids", "0,1", "--num_workers", "2", "--threads", "4"])
    assert (a.image_dir, a.model_path, a.output_dir, a.batch_size, a.gpu, a.device_ids, a.num_workers, a.threads, a.bf16) == \
        ("i", "m", "o", 64, True, "0,1", 2, 4, False)
    a = p.parse_args(["call_consensus", "-i", "i", "-m", "m", "-o", "o", "-bs", "8", "-g", "-d_ids", "0", "-w", "0", "-t", "1", "--bf16"])
    assert (a.batch_size, a.device_ids, a.bf16) == (8, "0", True)
    a = p.parse_args(["call_consensus", "-i", "i", "-m", "m", "-o", "o"])
    assert (a.batch_size, a.num_workers, a.threads, a.device_ids) == (2048, 4, 8, None)
    a = p.parse_args(["stitch", "--input_dir", "i", "--output_file", "o/x", "--threads", "2"])
    assert (a.input_dir, a.output_file, a.threads) == ("i", "o/x", 2)
    assert p.parse_args(["stitch", "-i", "i", "-o", "x"]).threads == 5
    help_text = pepper.call_consensus_parser().format_help()
    assert "128" in help_text and "ignored" in help_text


def test_pepper_polish_is_the_polish_parser():
    argv = ["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl", "-o", "out", "-t", "3", "-r", "c:1-5", "-bs", "64", "-g", "-d_ids", "0,0",
            "-w", "1", "--bf16", "--realign"]
    a = vars(pepper.parser().parse_args(["polish"] + argv))
    assert a.pop("sub_command") == "polish" and a.pop("version") is False
    assert a == vars(cli.polish_parser().parse_args(argv))
    b = vars(pepper.parser().parse_args(["polish", "-b", "r", "-f", "f", "-m", "m", "-o", "o"]))
    b.pop("sub_command"), b.pop("version")
    assert b == vars(cli.polish_parser().parse_args(["-b", "r", "-f", "f", "-m", "m", "-o", "o"]))


# ---- call_consensus on several callers, with a stub caller -------------------------------------------------------------

class _StubCaller:
    """labels from the image alone (so a chunk's labels do not depend on its launch); records device and shared flag"""

    def __init__(self, log, device, shared):
        self.log, self.device, self.shared = log, device, shared

    def p2_labels(self, images):
        self.log.append((self.device, self.shared, len(images)))
        return (images[:, :, 0].astype(np.int64) * 7 + images[:, :, 9]) % 5

    def close(self):
        pass


def _write_images(tmp, n_files=5, seed=9):
    rng = np.random.default_rng(seed)
    os.makedirs(tmp)
    for i in range(n_files):
        with PolishImageStore(os.path.join(tmp, "pepper_hp_images_thread_%d_x.hdf" % i), "w") as s:
            for r in range(int(rng.integers(1, 4))):
                start = 1000 * (10 * i + r)
                for cid in range(int(rng.integers(1, 4))):
                    s.write_chunk("ctg%d" % (i % 2), start, start + 1100, cid, rng.integers(0, 255, (L, 10), dtype=np.uint8),
                                  np.arange(start, start + L), np.zeros(L))
    open(os.path.join(tmp, "notes.txt"), "w").write("not an image file")
    H5File(os.path.join(tmp, "empty.hdf"), "w").close()   # no summaries group: skipped


def _predictions(out_dir):
    got = {}
    for name in sorted(os.listdir(out_dir)):
        with PolishPredictionStore(os.path.join(out_dir, name)) as s:
            for c in s.contigs():
                for reg in s.regions(c):
                    for ch in s.chunk_names(c, reg):
                        base = "predictions/%s/%s/%s/" % (c, reg, ch)
                        key = (c, reg, ch)
                        assert key not in got
                        got[key] = (s.region_span(c, reg),) + tuple(s.f.read(base + k).tobytes()
                                                                     for k in ("position", "index", "bases", "phred_score"))
    return got


def _cc_args(img, out, extra=()):
    model = os.path.join(os.path.dirname(img), "m.npz")
    if not os.path.exists(model):
        from pepper_thesis_amd import synth
        np.savez(model, **synth.make_weights_p2(3))
    return pepper.parser().parse_args(["call_consensus", "-i", img, "-m", model, "-o", out, "-bs", "4"] + list(extra))


def test_two_callers_equal_one_caller(tmp_path, monkeypatch):
    img = str(tmp_path / "img")
    _write_images(img)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    log1 = []
    rc = polish_steps.call_consensus_run(_cc_args(img, str(tmp_path / "one")),
                                         open_caller=lambda d, sh, sd, dt: _StubCaller(log1, d, sh))
    assert rc == 0 and os.listdir(str(tmp_path / "one")) == ["pepper_prediction_0.hdf"]
    assert log1 and all(d == 0 and not sh and n <= 4 for d, sh, n in log1)
    one = _predictions(str(tmp_path / "one"))
    # world 2 on one device: each rank as the launcher would start it
    args = _cc_args(img, str(tmp_path / "two"), ["-d_ids", "0,0"])
    plan = polish_rank.plan_ranks(args.device_ids, args.threads)
    log2 = []
    for r in range(2):
        assert polish_steps.call_consensus_rank(args, plan, r, lambda d, sh, sd, dt: _StubCaller(log2, d, sh)) == 0
    assert sorted(os.listdir(str(tmp_path / "two"))) == ["pepper_prediction_0.hdf", "pepper_prediction_0_1.hdf"]
    assert all(d == 0 and sh for d, sh, _ in log2)
    two = _predictions(str(tmp_path / "two"))
    assert two == one and len(one) > 10
    for key, (span, p, x, b, ph) in one.items():   # bases are the caller's labels, phred_score from the table
        bases = np.frombuffer(b, np.uint8)
        assert bases.max() <= 4 and np.array_equal(np.frombuffer(ph, np.uint8), polish_steps.phred_scores(bases[None])[0])


_RANK_CODE = r"""
import os, sys, time
sys.path.insert(0, %r)
from pepper_thesis_amd import pepper, polish_rank, polish_steps
class C:
    def p2_labels(self, images):
        if os.environ["RANK"] == "1":
            raise RuntimeError("stub caller: failing on purpose")
        time.sleep(120)
    def close(self):
        pass
sys.exit(polish_steps.call_consensus_rank(pepper.call_consensus_parser().parse_args(sys.argv[1:]),
                                          polish_rank.plan_ranks("0,0", 1), int(os.environ["RANK"]), lambda d, sh, sd, dt: C()))
"""


@pytest.mark.timeout(120)
def test_failing_caller_fails_the_command(tmp_path, capsys):
    img = str(tmp_path / "img")
    _write_images(img)
    out = str(tmp_path / "out")
    args = _cc_args(img, out, ["-d_ids", "0,0"])
    t0 = time.time()
    rc = polish_steps.call_consensus_run(args, rank_cmd=[sys.executable, "-c", _RANK_CODE % ROOT])
    dt = time.time() - t0
    assert rc != 0 and dt < 60, (rc, dt)
    assert "call_consensus: rank 1 ended with exit status 1" in capsys.readouterr().err
    assert not [n for n in os.listdir(out) if n.endswith("hdf")]
