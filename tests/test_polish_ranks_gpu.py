"""GPU: `polish -d_ids 0,0` (two ranks on one device, polish_rank.py) gives the FASTA of the single-rank run with
PV_SHARED_DEVICE=1, byte for byte, with and without --realign; and the premise of that identity: with shared_device = 1 the P2
labels of a chunk do not depend on the other chunks of its launch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pepper_thesis_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(tmp_path):
    """the inputs of test_polish_stitch_gpu.py::test_polish_command_end_to_end: three contigs, ctg1 without reads"""
    import torch
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    rng = np.random.default_rng(21)
    contigs = [("ctg2", "".join(rng.choice(list("ACGT"), size=9_500))), ("ctg10", "".join(rng.choice(list("ACGT"), size=6_200))),
               ("ctg1", "".join(rng.choice(list("ACGT"), size=3_000)))]
    bw.write_fasta(str(tmp_path / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs[:2]):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1500)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    for r in recs:
        r["mapq"] = int(rng.integers(0, 61))
    bw.write_bam(str(tmp_path / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)
    w = synth.make_weights_p2(31, 3.0)
    torch.save({"model_state_dict": {"module." + k: torch.from_numpy(v) for k, v in w.items()}, "hidden_size": 128,
                "gru_layers": 1, "epochs": 1}, str(tmp_path / "model.pkl"))


def _polish(tmp_path, out, d_ids, extra, shared_env):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PV_SHARED_DEVICE", None)
    if shared_env:
        env["PV_SHARED_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "pepper_thesis_amd", "polish", "-b", str(tmp_path / "reads.bam"), "-f", str(tmp_path / "ref.fa"),
           "-m", str(tmp_path / "model.pkl"), "-o", str(tmp_path / out), "-t", "4", "-d_ids", d_ids] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(str(tmp_path / out / "_pepper_polished.fa"), "rb").read(), r.stderr


@pytest.mark.parametrize("realign", [False, True])
def test_two_ranks_on_one_device_equal_one_rank(tmp_path, realign):
    _inputs(tmp_path)
    extra = ["--realign"] if realign else []
    one, err1 = _polish(tmp_path, "one", "0", extra, shared_env=True)
    two, err2 = _polish(tmp_path, "two", "0,0", extra, shared_env=False)   # the ranks set shared_device themselves
    assert two == one and one.startswith(b">ctg2\n") and b"\n>ctg10\n" in one
    per_rank = dict((int(r), int(n)) for r, n in re.findall(r"\[RANK (\d)/2\] POLISHED (\d+) REGIONS", err2))
    assert sorted(per_rank) == [0, 1] and min(per_rank.values()) > 0, err2[-3000:]
    assert "(shared)" in err2
    total = int(re.search(r"POLISHED FASTA: \S+ \((\d+) REGIONS", err1).group(1))
    assert sum(per_rank.values()) == total
    assert os.listdir(str(tmp_path / "two")) == ["_pepper_polished.fa"]


def test_p2_rows_independent_of_the_batch_with_shared_device(hip_ctx, opts):
    """shared_device = 1: the labels (and the accumulated softmax, bit for bit) of any subset of a launch's chunks, run alone,
    equal those chunks' rows inside the full launch - the premise of the two-rank byte identity (a rank's launches hold other
    regions than the single-rank launches). 2121 chunks is the size of a 1024-region polish launch."""
    opts(shared_device=1)
    hip_ctx.load_p2(synth.make_weights_p2(31, 3.0))
    y = synth.synth_p2_images(4242, 2121)
    labels, acc = hip_ctx.forward_p2(y, want_acc=True)
    for rows in (np.arange(1060), np.arange(1, 2121, 2), np.array([7]), np.r_[3, 17, 18, 1500:1531, 2120]):
        l_sub, a_sub = hip_ctx.forward_p2(y[rows], want_acc=True)
        assert np.array_equal(l_sub, labels[rows]), len(rows)
        assert np.array_equal(a_sub.view(np.uint32), acc[rows].view(np.uint32)), len(rows)
