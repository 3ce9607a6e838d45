"""CPU: the stitch semantics of the polisher (host checker, tests/stitch_ref.py), the region tiling, the `polish` command line,
its refusals and the checkpoint loader. The device stitch is checked against the same checker in test_polish_stitch_gpu.py."""
import os

import numpy as np
import pytest

import stitch_ref as sr
from pepper_thesis_amd import cli, polish, synth


def _chunk(pos, labels, idx=None):
    pos = np.asarray(pos, np.int64)
    return pos, np.zeros(len(pos), np.int32) if idx is None else np.asarray(idx, np.int32), np.asarray(labels, np.uint8)


def _overlap_pair(a, b):
    """chunks a and b of one region share positions 3 and 4; a labels them A, b labels them T"""
    r = sr.RegionChunks(0, 10)
    r.chunks[a] = _chunk([0, 1, 2, 3, 4], [2, 2, 2, 1, 1])
    r.chunks[b] = _chunk([3, 4, 5, 6, 7], [4, 4, 3, 3, 3])
    return sr.create_consensus_sequence([r])


@pytest.mark.parametrize("a,b,expect", [(0, 1, "CCCTTGGG"), (9, 10, "CCCAAGGG"), (10, 11, "CCCTTGGG")])
def test_overlap_winner_is_last_in_string_order(a, b, expect):
    assert _overlap_pair(a, b) == expect


def test_region_start_buffer_padding_and_label_zero():
    r = sr.RegionChunks(500, 1600)
    r.chunks[0] = _chunk([699, 700, 701, 702, 703, -1, -1], [1, 1, 2, 0, 3, 4, 4], [0, 0, 0, 0, 0, -1, -1])
    assert sr.create_consensus_sequence([r]) == "CG"    # <= start + 200 dropped, label 0 and padding give nothing
    r0 = sr.RegionChunks(0, 1100)
    r0.chunks[0] = _chunk([0, 1, 1, 2], [1, 2, 3, 4], [0, 0, 1, 0])
    assert sr.create_consensus_sequence([r0]) == "ACGT"   # a region at 0 keeps everything; insert rows sort after their base


def test_empty_regions_and_natural_contig_order():
    empty = sr.RegionChunks(900, 2100)
    assert sr.small_chunk_stitch([empty]) == (-1, -1, "")
    assert sr.create_consensus_sequence([empty]) == ""
    seqs = {"ctg10": "A", "ctg2": "C", "ctg1": "G", "ctg3": ""}
    assert sr.fasta_text(seqs) == ">ctg1\nG\n>ctg2\nC\n>ctg10\nA\n"
    assert [c for c in sorted(seqs, key=polish.natural_key)] == ["ctg1", "ctg2", "ctg3", "ctg10"]


def test_worker_grouping_does_not_change_the_string():
    """the reference deals regions to workers; with its tiling the kept ranges are disjoint, so any grouping agrees"""
    rng = np.random.default_rng(5)
    regs = []
    for a, b in polish.polish_intervals(5000):
        r = sr.RegionChunks(a, b)
        pos = np.arange(a, b + 1)
        r.chunks[0] = _chunk(pos, rng.integers(0, 5, len(pos)))
        regs.append(r)
    one = sr.create_consensus_sequence(regs, 1)
    assert one == sr.create_consensus_sequence(regs[::-1], 4) == "".join(sr.create_consensus_sequence([r]) for r in regs)
    assert len(one) == sum(int((r.chunks[0][2][r.chunks[0][0] > (r.start + 200 if r.start else -1)] != 0).sum()) for r in regs)


def test_region_tiling():
    assert polish.polish_intervals(5000) == [(0, 1100), (900, 2100), (1900, 3100), (2900, 4100), (3900, 4999)]
    assert polish.polish_intervals(10_000, 2500, 4700) == [(2500, 3600), (3400, 4600), (4400, 4700)]
    assert polish.polish_intervals(3000, 1000, 9999) == [(1000, 2100), (1900, 2999)]   # clamped at the contig end
    assert polish.polish_intervals(3000, -50, 800) == [(0, 800)]


def test_output_path_rule(tmp_path):
    p = polish.output_fasta_path(str(tmp_path / "out" / "polished"))
    assert p == str(tmp_path / "out" / "polished") + "/_pepper_polished.fa"
    assert os.path.isdir(tmp_path / "out" / "polished")
    assert polish.output_fasta_path(str(tmp_path) + "/o/") == str(tmp_path) + "/o/_pepper_polished.fa"


def test_polish_arguments_reference_names():
    ap = cli.polish_parser()
    a = ap.parse_args(["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl", "-o", "out/p", "-t", "7", "-r", "ctg1:100-200", "-bs", "256",
                       "-g", "-d_ids", "0", "-w", "2", "--bf16"])
    assert (a.bam, a.fasta, a.model_path, a.output_file, a.threads, a.region, a.batch_size, a.gpu, a.device_ids, a.num_workers,
            a.bf16) == ("r.bam", "d.fa", "m.pkl", "out/p", 7, "ctg1:100-200", 256, True, "0", 2, True)
    a = ap.parse_args(["--bam", "r.bam", "--fasta", "d.fa", "--model_path", "m.pkl", "--output_file", "o", "--threads", "3",
                       "--region", "ctg2", "--batch_size", "64", "--gpu", "--device_ids", "1", "--num_workers", "0"])
    assert (a.threads, a.region, a.batch_size, a.gpu, a.device_ids, a.num_workers, a.bf16) == (3, "ctg2", 64, True, "1", 0, False)
    with pytest.raises(SystemExit):
        ap.parse_args(["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl"])   # -o is required


def _files(tmp_path):
    for n in ("r.bam", "d.fa"):
        (tmp_path / n).write_bytes(b"")
    return ["-b", str(tmp_path / "r.bam"), "-f", str(tmp_path / "d.fa"), "-o", str(tmp_path / "out")]


def test_multi_rank_is_refused(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["polish", "-m", str(tmp_path / "m.pkl")] + _files(tmp_path)) == 2
    assert "multi-rank" in capsys.readouterr().err


def _save_ckpt(path, sd, **kw):
    import torch
    ck = {"model_state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}, "hidden_size": 128, "gru_layers": 1,
          "epochs": 3}
    ck.update(kw)
    torch.save(ck, path)


def test_checkpoint_with_module_prefix_loads(tmp_path):
    w = synth.make_weights_p2(17)
    _save_ckpt(str(tmp_path / "m.pkl"), w)
    got = polish.load_polish_model(str(tmp_path / "m.pkl"))
    assert set(got) == set(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    np.savez(str(tmp_path / "m.npz"), **w)
    got = polish.load_polish_model(str(tmp_path / "m.npz"))
    assert all(np.array_equal(got[k], w[k]) for k in w)


@pytest.mark.parametrize("kw", [{"hidden_size": 256}, {"gru_layers": 2}])
def test_unsupported_checkpoint_shapes_are_refused(tmp_path, capsys, kw, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    m = str(tmp_path / "m.pkl")
    _save_ckpt(m, synth.make_weights_p2(17), **kw)
    with pytest.raises(ValueError, match="kernels implement hidden_size=128, gru_layers=1"):
        polish.load_polish_model(m)
    assert cli.main(["polish", "-m", m] + _files(tmp_path)) == 2
    assert "hidden_size" in capsys.readouterr().err


def test_wrong_tensor_shape_is_refused(tmp_path):
    w = synth.make_weights_p2(17)
    w["gru_encoder.weight_hh_l0"] = np.zeros((3 * 64, 64), np.float32)
    np.savez(str(tmp_path / "m.npz"), **w)
    with pytest.raises(ValueError, match="gru_encoder.weight_hh_l0"):
        polish.load_polish_model(str(tmp_path / "m.npz"))
