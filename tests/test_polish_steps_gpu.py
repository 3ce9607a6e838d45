"""GPU: the polisher step by step (`python -m pepper_thesis_amd.pepper make_images / call_consensus / stitch`) against the
fused `polish`, the P2 labels and the host stitch checker. Every command runs in a fresh process under its own time limit.

The three steps equal `polish` byte for byte where a chunk's P2 labels do not depend on the other chunks of its launch:
shared_device = 1 (PV_SHARED_DEVICE=1 for a single caller; ranks sharing a device set it themselves), launches below the size
where the one-workgroup GRU forms stop being picked (test_p2_rows_independent_of_the_batch_with_shared_device).
call_consensus batches chunks in file order, polish in region order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stitch_ref as sr
from pepper_thesis_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 600


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """three contigs (ctg1 without reads), 60 reads of ~1.5 kb per contig with reads, seeded P2 weights"""
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    tmp = tmp_path_factory.mktemp("steps")
    rng = np.random.default_rng(21)
    contigs = [("ctg2", "".join(rng.choice(list("ACGT"), size=9_500))), ("ctg10", "".join(rng.choice(list("ACGT"), size=6_200))),
               ("ctg1", "".join(rng.choice(list("ACGT"), size=3_000)))]
    bw.write_fasta(str(tmp / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs[:2]):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1500)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    return tmp


def _run(argv, shared_env):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PV_SHARED_DEVICE", None)
    if shared_env:
        env["PV_SHARED_DEVICE"] = "1"
    r = subprocess.run([sys.executable, "-m", "pepper_thesis_amd.pepper"] + argv, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=STEP_TIMEOUT_S)
    assert r.returncode == 0, (argv, r.stderr[-3000:])
    return r.stderr


@pytest.mark.parametrize("realign", [False, True])
def test_three_steps_equal_polish(inputs, realign):
    t = inputs
    extra = ["--realign"] if realign else []
    tag = "r" if realign else "n"
    _run(["polish", "-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-m", str(t / "model.npz"), "-o", str(t / ("fused_" + tag)),
          "-t", "4", "-d_ids", "0"] + extra, shared_env=True)
    fused = open(str(t / ("fused_" + tag) / "_pepper_polished.fa"), "rb").read()
    assert fused.startswith(b">ctg2\n") and b"\n>ctg10\n" in fused and b">ctg1\n" not in fused
    for threads, d_ids in ((1, "0"), (3, "0,0")):
        img, pred, out = (str(t / ("%s_%s_%d" % (k, tag, threads))) for k in ("img", "pred", "out"))
        _run(["make_images", "-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-o", img, "-t", str(threads)] + extra, False)
        names = sorted(os.listdir(img))
        assert len(names) == threads and all(n.startswith("pepper_hp_images_thread_") and n.endswith(".hdf") for n in names)
        err = _run(["call_consensus", "-i", img, "-m", str(t / "model.npz"), "-o", pred, "-d_ids", d_ids, "-bs", "512"],
                   shared_env=(d_ids == "0"))
        want = ["pepper_prediction_0.hdf"] + (["pepper_prediction_0_1.hdf"] if d_ids == "0,0" else [])
        assert sorted(os.listdir(pred)) == want, err[-2000:]
        _run(["stitch", "-i", pred, "-o", out + "/polished"], False)
        got = open(out + "/polished_pepper_polished.fa", "rb").read()
        assert got == fused, (realign, threads, d_ids)


def _ref_fasta(pred_dir):
    """stitch_ref's FASTA from the prediction files, read with the generic H5File reader"""
    from pepper_thesis_amd.hdf5io import H5File
    by = {}
    for name in sorted(os.listdir(pred_dir)):
        with H5File(os.path.join(pred_dir, name)) as f:
            for contig in f.keys("/predictions"):
                for reg in f.keys("/predictions/" + contig):
                    base = "predictions/%s/%s/" % (contig, reg)
                    rc = sr.RegionChunks(f.read(base + "contig_start"), f.read(base + "contig_end"))
                    for ch in f.keys(base):
                        if ch not in ("contig_start", "contig_end"):
                            rc.chunks[int(ch)] = tuple(f.read(base + ch + "/" + k) for k in ("position", "index", "bases"))
                    by.setdefault(contig, []).append(rc)
    return sr.fasta_text({c: sr.create_consensus_sequence(r, threads=4) for c, r in by.items()})


@pytest.mark.parametrize("bf16", [False, True])
def test_bases_are_p2_labels_and_stitch_equals_checker(inputs, hip_ctx, opts, bf16):
    from pepper_thesis_amd import _ffi, polish
    from pepper_thesis_amd.hdf5io import PolishImageStore, PolishPredictionStore
    t = inputs
    tag = "b" if bf16 else "f"
    img, pred, out = (str(t / ("%s_%s" % (k, tag))) for k in ("img", "pred", "out"))
    _run(["make_images", "-b", str(t / "reads.bam"), "-f", str(t / "ref.fa"), "-o", img, "-t", "2"], False)
    _run(["call_consensus", "-i", img, "-m", str(t / "model.npz"), "-o", pred, "-bs", "64"] + (["--bf16"] if bf16 else []),
         shared_env=True)
    keys, images = [], []
    for name in sorted(os.listdir(img)):
        with PolishImageStore(os.path.join(img, name)) as s:
            for nm in s.summaries():
                c = s.read_chunk(nm)
                keys.append((c["contig"], "%s-%d-%d" % (c["contig"], c["region_start"], c["region_end"]), str(c["chunk_id"]),
                             c["position"], c["index"]))
                images.append(c["image"])
    assert len(images) > 20
    opts(shared_device=1)
    hip_ctx.load_p2(polish.load_polish_model(str(t / "model.npz")), _ffi.PV_DTYPE_BF16_INPUT_GEMM if bf16 else _ffi.PV_DTYPE_F32)
    labels = hip_ctx.forward_p2(np.stack(images))
    with PolishPredictionStore(os.path.join(pred, "pepper_prediction_0.hdf")) as s:
        n = 0
        for k, (contig, reg, ch, pos, idx) in enumerate(keys):
            c = s.read_chunk(contig, reg, ch)
            assert np.array_equal(c["bases"], labels[k]), k
            assert np.array_equal(c["position"], pos) and np.array_equal(c["index"], idx)
            n += 1
        assert n == sum(len(s.chunk_names(c, r)) for c in s.contigs() for r in s.regions(c))
    _run(["stitch", "-i", pred, "-o", out + "/p"], False)
    got = open(out + "/p_pepper_polished.fa").read()
    assert got == _ref_fasta(pred) and got.startswith(">ctg2\n")


def test_stitch_refuses_a_label_above_4(tmp_path, capsys):
    from pepper_thesis_amd import pepper, polish_steps
    from pepper_thesis_amd.hdf5io import PolishPredictionStore
    pred = str(tmp_path / "pred")
    os.makedirs(pred)
    bases = np.ones(1000, np.uint8)
    bases[500] = 255   # a poisoned label on a kept column
    with PolishPredictionStore(os.path.join(pred, "p.hdf"), "w") as s:
        s.write_prediction("c", 0, 1100, 0, np.arange(1000), np.zeros(1000), np.ones(1000), np.zeros(1000))
        s.write_prediction("c", 0, 1100, 1, np.arange(950, 1950), np.zeros(1000), bases, np.zeros(1000))
    out = str(tmp_path / "x")
    assert polish_steps.stitch_run(pepper.parser().parse_args(["stitch", "-i", pred, "-o", out])) == 1
    err = capsys.readouterr().err
    assert "p.hdf" in err and "c/c-0-1100/1" in err and "above 4" in err
    assert not os.path.exists(out + "_pepper_polished.fa")
