"""GPU: pv_polish_realign[_dev] against the reference fixture and the host checker (tests/realign_ref.py), the builder on
realigned reads, and `polish --realign` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import realign_cases as rc
import realign_ref as rr
from pepper_thesis_amd import _ffi, polish, polish_summary, realign, synth
from pepper_thesis_amd.batch import pack_regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _regions_and_windows(cases):
    regs, wins = [], []
    for start, end, win, reads in cases:
        regs.append(rc.as_region(start, end, win, reads))
        wins.append(win)
    return regs, wins


def _run(ctx, regs, wins, **kw):
    b = pack_regions(regs)
    woff, win = realign.pack_windows(wins)
    return b, ctx.polish_realign(b, woff, win, **kw)


def _read_cigar(res, k):
    return res.cigar[res.cigar_off[k]:res.cigar_off[k + 1]]


def _check_read(res, k, rec, read, tag):
    assert (int(res.state[k]), int(res.score[k])) == (rec.state, rec.score), tag
    if rec.state == rr.REALIGNED:
        assert tuple(int(v) for v in res.ends[k]) == (rec.ref_begin, rec.ref_end, rec.query_begin, rec.query_end), tag
        assert int(res.read_pos[k]) == rec.new_pos, tag
        assert np.array_equal(_read_cigar(res, k), rec.cigar), tag
    elif rec.state == rr.UNCHANGED:
        assert int(res.read_pos[k]) == read.pos and np.array_equal(_read_cigar(res, k), read.cigar), tag
    else:
        assert len(_read_cigar(res, k)) == 0, tag


def test_fixture_parity(hip_ctx):
    g = np.load(os.path.join(ROOT, "tests", "golden", "realign_golden.npz"), allow_pickle=False)
    from test_polish_realign_cpu import golden_cases
    cases = golden_cases(g)
    regs, wins = _regions_and_windows([(s, int(g[n + "/end"]), w, reads) for n, s, w, reads, _, _ in cases])
    b, res = _run(hip_ctx, regs, wins)
    k = 0
    for name, start, win, reads, recs, cigars in cases:
        for j, (exp, ecig) in enumerate(zip(recs.tolist(), cigars)):
            tag = "%s read %d" % (name, j)
            rec = rr.Record(exp[0], exp[1], *exp[2:7], cigar=ecig)
            _check_read(res, k, rec, reads[j], tag)
            k += 1
    assert k == b.n_reads
    assert res.n_dropped == int(sum((c[4][:, 0] == 2).sum() for c in cases))


def _check_vs_checker(res, regs, wins, sample=None):
    k0 = 0
    for g, (reg, win) in enumerate(zip(regs, wins)):
        idx = range(len(reg.reads)) if sample is None else [j for j in range(len(reg.reads)) if k0 + j in sample]
        reads = [reg.reads[j] for j in idx]
        recs = rr.realign_reads(reg.ref_start, win, reads)
        for j, rec, read in zip(idx, recs, reads):
            _check_read(res, k0 + j, rec, read, "region %d read %d" % (g, j))
        k0 += len(reg.reads)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_parity_with_checker(hip_ctx, seed):
    cases = [rc.random_region(1000 * seed + k, start=5000 + 1000 * k, n_reads=40, long_ins=0.002) for k in range(4)]
    cases.append(rc.random_region(77 + seed, start=0, n_reads=30, contig_len=900, alphabet=b"NnacgtUuRY\xc8\xff"))
    if seed == 1:
        cases.append(rc.random_region(99, start=20_000, n_reads=1500, long_ins=0.0005))
    regs, wins = _regions_and_windows(cases)
    b, res = _run(hip_ctx, regs, wins)
    _check_vs_checker(res, regs, wins)
    assert res.n_realigned > 0.9 * b.n_reads


def test_edge_cases_with_high_bytes(hip_ctx):
    cases = [(s, e, w, reads) for _, s, e, w, reads in rc.edge_regions(high=True)]
    regs, wins = _regions_and_windows(cases)
    b, res = _run(hip_ctx, regs, wins)
    _check_vs_checker(res, regs, wins)


@pytest.fixture(scope="module")
def large_batch():
    rng = np.random.default_rng(5)
    regs = [rc.fast_region(rng, 10_000 + 1000 * g, n_reads=int(rng.integers(25, 40))) for g in range(1000)]
    return regs, [r.window for r in regs]


def test_large_batch(hip_ctx, large_batch):
    regs, wins = large_batch
    b, res = _run(hip_ctx, regs, wins)
    n = b.n_reads
    assert n >= 30_000 and res.n_realigned == n
    rng = np.random.default_rng(0)
    sample = set(rng.choice(n, 250, replace=False).tolist()) | {0, n - 1}
    _check_vs_checker(res, regs, wins, sample)
    # every read: the emitted cigar rescored with the matrix gives the score, consumes the query and spans the ends
    k = 0
    for reg, win in zip(regs, wins):
        for rd in reg.reads:
            off = rd.pos - reg.ref_start
            s, qn, span = rr.rescore(win[off:], rd.bases, _read_cigar(res, k), int(res.ends[k, 0]))
            assert (s, qn, span) == (int(res.score[k]), len(rd.bases), int(res.ends[k, 1] - res.ends[k, 0] + 1)), k
            k += 1


def test_scratch_slicing_and_limit(hip_ctx):
    cases = [rc.random_region(300 + k, start=1000 * k, n_reads=12, long_ins=0.01) for k in range(3)]
    regs, wins = _regions_and_windows(cases)
    b, ref = _run(hip_ctx, regs, wins)
    old = hip_ctx.get_option("realign_scratch_kb")
    try:
        hip_ctx.set_option("realign_scratch_kb", 4096)  # 21 workers of 192 KB, 4 of 1 MB, then single 4 MB workers
        _, got = _run(hip_ctx, regs, wins)
        for f in ("read_pos", "cigar_off", "cigar", "score", "ends", "state"):
            assert np.array_equal(getattr(got, f), getattr(ref, f)), f
        hip_ctx.set_option("realign_scratch_kb", 1)     # no full-size read fits 1 KB of direction bytes
        with pytest.raises(_ffi.PepperHipError) as e:
            _run(hip_ctx, regs, wins)
        assert e.value.code == _ffi.PV_ERR_LIMIT and "realign_scratch_kb" in str(e.value)
    finally:
        hip_ctx.set_option("realign_scratch_kb", old)
    _, again = _run(hip_ctx, regs, wins)
    assert np.array_equal(again.cigar, ref.cigar)


def test_capacity_then_retry(hip_ctx):
    regs, wins = _regions_and_windows([rc.random_region(400, n_reads=20)])
    b, ref = _run(hip_ctx, regs, wins)
    need = len(ref.cigar)
    with pytest.raises(_ffi.PepperHipError) as e:
        _run(hip_ctx, regs, wins, cigar_capacity=need - 1)
    assert e.value.code == _ffi.PV_ERR_CAPACITY and ("need %d words" % need) in str(e.value)
    _, got = _run(hip_ctx, regs, wins, cigar_capacity=need)
    assert np.array_equal(got.cigar, ref.cigar) and np.array_equal(got.cigar_off, ref.cigar_off)


def test_device_form_equals_host_form(hip_ctx, large_batch):
    import torch
    from pepper_thesis_amd.device import DeviceBatch
    regs, wins = large_batch[0][:200], large_batch[1][:200]
    b, ref = _run(hip_ctx, regs, wins)
    dev = "cuda:%d" % hip_ctx.device_id
    db = DeviceBatch(b, dev)
    woff, win = realign.pack_windows(wins)
    d_woff, d_win = realign.device_windows(woff, win, dev)
    out = realign.DeviceRealignOut(b.n_reads, len(ref.cigar), dev)
    torch.cuda.synchronize()
    hip_ctx.polish_realign_dev(db, d_woff.data_ptr(), d_win.data_ptr(), int(np.diff(b.base_off).max()), out)
    hip_ctx.synchronize()
    total, status, nre, ndr = out.counts.tolist()
    assert (total, status, nre, ndr) == (len(ref.cigar), 0, ref.n_realigned, ref.n_dropped)
    assert np.array_equal(out.cigar[:total].cpu().numpy().view(np.uint32), ref.cigar)
    assert np.array_equal(out.cigar_off.cpu().numpy(), ref.cigar_off)
    assert np.array_equal(out.read_pos.cpu().numpy(), ref.read_pos)
    assert np.array_equal(out.ends.cpu().numpy(), ref.ends) and np.array_equal(out.score.cpu().numpy(), ref.score)


def test_builder_on_realigned_reads(hip_ctx, oracle_lib):
    from test_polish_gpu import assert_polish_equal
    cases = [rc.random_region(500 + k, start=3000 * k, n_reads=30, long_ins=0.003) for k in range(6)]
    cases += [(s, e, w, reads) for _, s, e, w, reads in rc.edge_regions()]
    s, e, w, reads = cases[0]
    reads.append(rc._read(e - 60, w[e - 60 - s:e - s + 15]))   # runs 15 bases past the region end
    regs, wins = _regions_and_windows(cases)
    b, res = _run(hip_ctx, regs, wins)
    rb = realign.realigned_batch(b, res)
    # some alignments now run past the region end into the safe bases, which the clipped reads never did
    past = [k for k in range(b.n_reads) if res.state[k] == 1 and
            res.read_pos[k] - res.ends[k, 0] + res.ends[k, 1] > rb.ref_end[np.searchsorted(rb.read_off, k, "right") - 1]]
    assert past
    assert_polish_equal(hip_ctx.polish_summarize(rb, want_flat=True), oracle_lib.polish_summarize(rb, 1000, 50), "realigned")
    # dropped reads in place with no cigar words build what the reference builds without them
    host = pack_regions([rr.realigned_region(r, w) for r, w in zip(regs, wins)])
    assert_polish_equal(hip_ctx.polish_summarize(host, want_flat=True), oracle_lib.polish_summarize(rb, 1000, 50), "dropped")


def _bam_and_draft(tmp_path, seed):
    import bam_writer as bw
    from pepper_thesis_amd import build
    build.build_io()
    rng = np.random.default_rng(seed)
    contigs = [("ctg2", rc.ACGT[rng.integers(0, 4, 7_500)].tobytes().decode()),
               ("ctg10", rc.ACGT[rng.integers(0, 4, 4_200)].tobytes().decode())]
    bw.write_fasta(str(tmp_path / "ref.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        for i in range(70):
            a = int(rng.integers(0, len(seq) - 300))
            b = min(len(seq), a + int(rng.integers(300, 3000)))
            q = rc._mutate(rng, np.frombuffer(seq[a:b].encode(), np.uint8), long_ins=0.0005)
            recs.append(dict(tid=tid, pos=a, mapq=60, flag=int(rng.choice([0, 16])), cigar=[(0, len(q))], seq=q.tobytes().decode(),
                             qual=[30] * len(q), name="r%d_%d" % (tid, i), hp=None))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp_path / "reads.bam"), [(n, len(s)) for n, s in contigs], recs)


def test_polish_realign_end_to_end(hip_ctx, tmp_path):
    """`polish --realign` in a fresh process = region_from_files -> realign_ref -> builder -> forward_p2 -> stitch on the
    host; without --realign the output is what polish_fused wrote before this option existed"""
    import torch
    import stitch_ref as sr
    from pepper_thesis_amd import bamio
    _bam_and_draft(tmp_path, 33)
    w = synth.make_weights_p2(31, 3.0)
    torch.save({"model_state_dict": {"module." + k: torch.from_numpy(v) for k, v in w.items()}, "hidden_size": 128,
                "gru_layers": 1, "epochs": 1}, str(tmp_path / "model.pkl"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = {}
    for flag in ("--realign", None):
        cmd = [sys.executable, "-m", "pepper_thesis_amd", "polish", "-b", str(tmp_path / "reads.bam"), "-f",
               str(tmp_path / "ref.fa"), "-m", str(tmp_path / "model.pkl"), "-o", str(tmp_path / ("out%s" % bool(flag))), "-t", "3"]
        r = subprocess.run(cmd + ([flag] if flag else []), cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[flag] = open(str(tmp_path / ("out%s" % bool(flag)) / "_pepper_polished.fa")).read()

    b, f = bamio.BamHandler(str(tmp_path / "reads.bam")), bamio.FastaHandler(str(tmp_path / "ref.fa"))
    hip_ctx.load_p2(w)
    exp = {}
    for realigned in (True, False):
        names, regs = [], []
        for c in ("ctg2", "ctg10"):
            for s, e in polish.polish_intervals(f.get_chromosome_sequence_length(c)):
                reg = polish_summary.region_from_files(b, f, c, s, e, realign=realigned)
                if reg is not None:
                    names.append((c, s, e))
                    regs.append(rr.realigned_region(reg, reg.window) if realigned else reg)
        out, labels = polish_summary.polish_regions(hip_ctx, regs)
        exp[realigned] = sr.fasta_text(sr.stitch_contigs(out.position, out.index, out.region, out.chunk_id, labels, names,
                                                         threads=5))
    assert outs["--realign"] == exp[True]
    assert outs[None] == exp[False]
    assert exp[True] != exp[False]
    # the same in-process through polish_fused (the bench path), and the default stays off
    p = polish.polish_fused(str(tmp_path / "reads.bam"), str(tmp_path / "ref.fa"), str(tmp_path / "model.pkl"),
                            str(tmp_path / "fused"), ctx=hip_ctx, realign=True)
    assert open(p).read() == exp[True]


def _golden_chain(g, name):
    from test_oracle_polish_ref import case_batch
    key = "chain/" + name
    return case_batch(g, key), g[key + "/win_off"], g[key + "/win"]


def _check_chain_realign(g, name, res, k0, n):
    key = "chain/" + name
    st, pos = g[key + "/realign_state"], g[key + "/realign_pos"]
    coff, cig = g[key + "/realign_cigar_off"], g[key + "/realign_cigar"]
    for j in range(n):
        k = k0 + j
        assert (int(res.state[k]) == rr.DROPPED) == (int(st[j]) == 2), (name, j)
        if st[j] == 1:
            assert int(res.read_pos[k]) == int(pos[j]), (name, j)
            assert np.array_equal(res.cigar[res.cigar_off[k]:res.cigar_off[k + 1]], cig[coff[j]:coff[j + 1]]), (name, j)


def test_golden_chain_realign_build_chunk(hip_ctx):
    """realign -> realigned_batch -> pv_polish_summarize_regions equals the reference's ReadAligner -> SummaryGenerator ->
    chunk_images(1000, 50) (create_summary with realignment_flag=True, from the reads onward); each case alone, then all
    cases in one batch"""
    from pepper_thesis_amd.batch import merge_batches
    from test_oracle_polish_ref import assert_matches_golden, expected, expected_all, load_golden, names
    g = load_golden()
    chain = names(g, "chain_names")
    for name in chain:
        b, woff, win = _golden_chain(g, name)
        res = realign.realign(hip_ctx, b, woff, win)
        _check_chain_realign(g, name, res, 0, b.n_reads)
        out = hip_ctx.polish_summarize(realign.realigned_batch(b, res), 1000, 50, want_flat=True)
        assert_matches_golden(out, expected(g, "chain/" + name, 1000, 50), name)
    parts = [_golden_chain(g, n) for n in chain]
    b = merge_batches([p[0] for p in parts])
    woff, win = realign.pack_windows([p[2][:int(p[1][-1])].tobytes() for p in parts])
    res = realign.realign(hip_ctx, b, woff, win)
    k0 = 0
    for name, p in zip(chain, parts):
        _check_chain_realign(g, name, res, k0, p[0].n_reads)
        k0 += p[0].n_reads
    out = hip_ctx.polish_summarize(realign.realigned_batch(b, res), 1000, 50, want_flat=True)
    assert_matches_golden(out, expected_all(g, ["chain/" + n for n in chain], 1000, 50), "all chains")
