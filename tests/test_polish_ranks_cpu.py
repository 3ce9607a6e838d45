"""CPU, world_size 2 over gloo: the multi-rank plumbing of `polish -d_ids a,b,...` (polish_rank.py). The device chain is replaced
by a stub that returns, for every region, the draft bases the stitch would keep (pos > start + 200, all of a region at 0), so
the merged FASTA is checkable by hand; the GPU test of the real chain on two ranks is in test_polish_ranks_gpu.py."""
import functools
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from pepper_thesis_amd import cli, polish, polish_rank, synth

CONTIGS = (("ctg2", 9_500), ("ctg10", 6_200), ("ctg1", 3_000))   # ctg1 has no reads


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _StubChain:
    """the chain's contract (run(batch, windows) -> ChainResult, close()) without a device; records every region"""

    def __init__(self, log_path, device, shared, fail):
        self.log_path, self.device, self.shared, self.fail = log_path, device, shared, fail

    def run(self, batch, windows=None):
        if self.fail:
            raise RuntimeError("stub chain: failing on purpose")
        out, roff = [], [0]
        with open(self.log_path, "a") as fh:
            for g in range(batch.n_regions):
                a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
                draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1]
                out.append(draft[201:] if a > 0 else draft)
                roff.append(roff[-1] + len(out[-1]))
                fh.write("%s %d %d %d %d\n" % (batch.contigs[g], a, b, self.device, int(self.shared)))
        return polish.ChainResult(np.asarray(roff, np.int64), b"".join(out))

    def close(self):
        pass


def _stub_open(tmp, fail_rank, device, shared_device, state_dict, dtype):
    rank = int(os.environ.get("RANK", "0")) if os.environ.get("WORLD_SIZE", "1") != "1" else -1
    return _StubChain(os.path.join(tmp, "regions_%d.txt" % rank), device, shared_device, rank == fail_rank)


def _argv(tmp, out, extra=()):
    return ["-b", os.path.join(tmp, "r.bam"), "-f", os.path.join(tmp, "r.fa"), "-m", os.path.join(tmp, "m.npz"), "-o",
            os.path.join(tmp, out), "-t", "4", "-bs", "8"] + list(extra)


def _worker(rank, world, port, tmp, fail_rank, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from pepper_thesis_amd import cli, polish_rank
    args = cli.polish_parser().parse_args(_argv(tmp, "out2", ["-d_ids", "3,3"]))
    t0 = time.time()
    rc = polish_rank.run(args, open_chain=functools.partial(_stub_open, tmp, fail_rank), timeout_s=60)
    q.put((rank, rc, time.time() - t0))


def _make_inputs(tmp):
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    rng = np.random.default_rng(21)
    contigs = [(n, "".join(rng.choice(list("ACGT"), size=L))) for n, L in CONTIGS]
    bw.write_fasta(os.path.join(tmp, "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs[:2]):
        recs += bw.random_records(rng, 40, len(seq), tid=tid, mean_len=1500)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(os.path.join(tmp, "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(os.path.join(tmp, "m.npz"), **synth.make_weights_p2(3))
    return dict(contigs)


def _run_world(tmp, world, fail_rank=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, tmp, fail_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, rc, dt = q.get(timeout=150)
        got[r] = (rc, dt)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def _logged(tmp, rank):
    path = os.path.join(tmp, "regions_%d.txt" % rank)
    if not os.path.exists(path):
        return []
    return [tuple(int(t) if t.isdigit() else t for t in line.split()) for line in open(path).read().splitlines()]


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_rank(tmp_path, monkeypatch):
    tmp = str(tmp_path)
    seqs = _make_inputs(tmp)
    # world 1: polish.run with the stub chain (no -d_ids: today's single-rank path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args1 = cli.polish_parser().parse_args(_argv(tmp, "out1"))
    assert polish.run(args1, open_chain=functools.partial(_stub_open, tmp, None)) == 0
    one = open(os.path.join(tmp, "out1", "_pepper_polished.fa")).read()
    # the regions with reads, in order, and the string the stitch rule gives from the draft
    from pepper_thesis_amd import bamio, polish_summary
    b, f = bamio.BamHandler(os.path.join(tmp, "r.bam")), bamio.FastaHandler(os.path.join(tmp, "r.fa"))
    regions, expect = [], {}
    for c in sorted(seqs, key=polish.natural_key):
        for s, e in polish.polish_intervals(len(seqs[c])):
            if polish_summary.region_from_files(b, f, c, s, e) is not None:
                regions.append((c, s, e))
                expect[c] = expect.get(c, "") + seqs[c][s + 201 if s else 0:e + 1]
    assert {c for c, _, _ in regions} == {"ctg2", "ctg10"} and len(regions) > 8
    assert one == "".join(">%s\n%s\n" % (c, expect[c]) for c in sorted(expect, key=polish.natural_key))
    assert [(c, s, e) for c, s, e, _, _ in _logged(tmp, -1)] == regions
    # world 2, both ranks on device 3: rank 0's FASTA is the world-1 FASTA byte for byte
    got = _run_world(tmp, 2)
    assert got[0][0] == 0 and got[1][0] == 0, got
    assert open(os.path.join(tmp, "out2", "_pepper_polished.fa"), "rb").read() == one.encode()
    assert os.listdir(os.path.join(tmp, "out2")) == ["_pepper_polished.fa"]
    ranks = [_logged(tmp, r) for r in range(2)]
    assert all(dev == 3 and shared == 1 for rk in ranks for _, _, _, dev, shared in rk)   # two ranks on one device: shared
    seen = [(c, s, e) for rk in ranks for c, s, e, _, _ in rk]
    assert len(seen) == len(set(seen)) and set(seen) == set(regions)   # every region once, on one rank
    order = {r: i for i, r in enumerate((c, s, e) for c in sorted(seqs, key=polish.natural_key)
                                        for s, e in polish.polish_intervals(len(seqs[c])))}
    for r in range(2):
        assert ranks[r] and all(order[(c, s, e)] % 2 == r for c, s, e, _, _ in ranks[r])   # region i on rank i % 2


@pytest.mark.timeout(300)
def test_failing_rank_fails_every_rank(tmp_path):
    tmp = str(tmp_path)
    _make_inputs(tmp)
    got = _run_world(tmp, 2, fail_rank=1)
    assert got[0][0] != 0 and got[1][0] != 0, got
    assert max(dt for _, dt in got.values()) < 30, got   # no rank waits for a peer that is gone
    assert not os.path.exists(os.path.join(tmp, "out2", "_pepper_polished.fa"))


def test_launcher_plan():
    import torch
    plan = polish_rank.plan_ranks("3,5,3", 8)
    assert [(p.rank, p.device, p.shared_device) for p in plan] == [(0, 3, True), (1, 5, False), (2, 3, True)]
    assert [p.threads for p in plan] == [2, 2, 2]                          # -t is the total: 8 // 3
    assert [p.threads for p in polish_rank.plan_ranks("0,1", 1)] == [1, 1]
    assert polish_rank.plan_ranks(None, 5) == [polish_rank.RankPlan(0, 0, False, 5)]
    assert polish_rank.plan_ranks("2", 5) == [polish_rank.RankPlan(0, 2, False, 5)]
    assert len(polish_rank.plan_ranks(",".join(["0"] * 16), 16)) == 16
    with pytest.raises(ValueError, match="at most 16"):
        polish_rank.plan_ranks(",".join(str(i) for i in range(17)), 16)
    with pytest.raises(ValueError, match="comma list"):
        polish_rank.plan_ranks("0,x", 4)
    assert not torch.cuda.is_initialized()


def test_too_many_ids_refused_before_anything_starts(tmp_path, monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ids = ",".join(["0"] * 17)
    assert cli.main(["polish", "-b", "none.bam", "-f", "none.fa", "-m", "none.pkl", "-o", str(tmp_path / "o"), "-d_ids", ids]) == 2
    assert "at most 16" in capsys.readouterr().err and not os.path.exists(tmp_path / "o")


def test_rank_argv_round_trips():
    a = cli.polish_parser().parse_args(["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl", "-o", "out/p", "-t", "7", "-r", "ctg1:100-200",
                                        "-bs", "256", "-g", "-d_ids", "0,0", "-w", "2", "--bf16", "--realign"])
    plan = polish_rank.plan_ranks(a.device_ids, a.threads)
    b = cli.polish_parser().parse_args(polish_rank.rank_argv(a, plan))
    for k in ("bam", "fasta", "model_path", "output_file", "threads", "region", "batch_size", "device_ids", "bf16", "realign"):
        assert getattr(a, k) == getattr(b, k), k


def test_supervisor_stops_the_other_ranks():
    """a rank that fails ends the run: the parent stops the rank still running and returns non-zero; nothing is restarted"""
    py = sys.executable
    ok = [py, "-c", "pass"]
    slow = [py, "-c", "import time; time.sleep(120)"]
    bad = [py, "-c", "import sys; sys.exit(3)"]
    env = dict(os.environ)
    t0 = time.time()
    assert polish_rank.supervise([slow, bad], [env, env]) == 3
    assert time.time() - t0 < 60
    assert polish_rank.supervise([ok, ok, ok], [env] * 3) == 0
    killed = [py, "-c", "import os, signal; os.kill(os.getpid(), signal.SIGKILL)"]
    assert polish_rank.supervise([slow, killed], [env, env]) == 1


def test_merge_is_order_free():
    pieces = [("c1", 900, 1, b"GG"), ("c2", 0, 3, b"T"), ("c1", 0, 0, b"AA"), ("c1", 900, 2, b"CC")]
    want = {"c1": b"AAGGCC", "c2": b"T"}
    assert polish.merge_pieces(pieces) == want
    assert polish.merge_pieces(pieces[::-1]) == want
