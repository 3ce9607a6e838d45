"""GPU: the polisher's `--gpu_decode` read path against its host reader, byte for byte - the batches of every launch
(DecodedBatch.to_host() == pack_regions of region_from_files), the host route, the slot retry, the workspace budget, and the
commands end to end (`polish`, `pepper make_images`) against the same commands without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_writer as bw  # noqa: E402
from pepper_thesis_amd import bamio, build, gpu_decode as gd, polish, synth  # noqa: E402
from pepper_thesis_amd.batch import RegionBatch, pack_regions  # noqa: E402
from pepper_thesis_amd.polish_summary import MAX_READS_IN_REGION, region_from_files  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 600


def _reads(rng, n, L, tid, lo=50, hi=800):
    """reads of lo..hi bases with inserts, deletions and soft clips; flags and MAPQ as they come: forward / reverse, secondary
    (0x100) and supplementary (0x800, both dropped by the polisher), MAPQ 0 (kept)"""
    recs = bw.random_records(rng, n, L, tid=tid, mean_len=(lo + hi) // 2, allow_skip=False)
    return [r for r in recs if lo <= len(r["seq"]) <= hi]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """c1: 6000 bases, reads at both ends and none over [1900, 3100]; one read of 800 bases with deletions that spans three
    regions; c2: 3500 bases; c3: 1000 bases under 1501 reads of 8 bases. Seeded P2 weights."""
    build.build_io()
    tmp = tmp_path_factory.mktemp("pdec")
    rng = np.random.default_rng(77)
    contigs = [("c1", 6000), ("c2", 3500), ("c3", 1000)]
    bw.write_fasta(str(tmp / "d.fa"), [(n, "".join(rng.choice(list("ACGT"), size=L))) for n, L in contigs])
    recs = [r for r in _reads(rng, 260, 6000, 0) if r["pos"] + bw.ref_len(r["cigar"]) < 1850 or r["pos"] > 3150]
    span = dict(tid=0, pos=3980, mapq=0, flag=16, cigar=[(0, 400), (2, 140), (0, 400)], seq="".join(rng.choice(list("ACGT"), size=800)),
                qual=[int(q) for q in rng.integers(1, 50, size=800)], name="span3")   # [3980, 4920): regions at 2900, 3900 and 4900
    recs += [span] + _reads(rng, 120, 3500, 1)
    recs += [dict(tid=2, pos=100 + (i % 700), mapq=60, flag=0, cigar=[(0, 8)], seq="ACGTTGCA", qual=[10 + i % 40] * 8, name="s%d" % i)
             for i in range(1501)]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    assert any(r["mapq"] == 0 and not r["flag"] & 0x900 for r in recs) and any(r["flag"] & 0x100 for r in recs)
    assert any(r["flag"] & 0x800 for r in recs)
    bw.write_bam(str(tmp / "r.bam"), contigs, recs, block_records=23)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    return tmp


def _work(bam, fa, region=None, extra=()):
    work, _ = polish.polish_work(bamio.FastaHandler(fa), bamio.BamHandler(bam), region)
    for contig, s, e in extra:
        work.append(polish.Work(len(work), 0, contig, s, e))
    return work


def _launches(ctx, bam, fa, work, per_launch, realign=True, **kw):
    """the launches of polish_pieces' device read path, made on this thread -> ([parts], timers)"""
    T = {}
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    dec = gd.GpuDecoder(ctx, bam, fa, 0, False, 1.0, 0, T, max_reads=MAX_READS_IN_REGION, realign=realign, **kw)
    try:
        planned = [gd.PlannedGroup(b, f, [(w.contig, w.start, w.end) for w in g], 0, pad_ref=True, windows=realign, works=g)
                   for g in gd.region_groups(work)]
        return list(gd.decoded_launches(dec, iter(planned), per_launch)), T
    finally:
        dec.close()


def _same_as_host(launches, bam, fa, work, per_launch, realign=True):
    """every part equals the host reader's batch of the same regions; the launches hold what the host path's flush holds"""
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    host = {w.index: region_from_files(b, f, w.contig, w.start, w.end, realign=realign) for w in work}
    with_reads = [w for w in work if host[w.index] is not None]
    flushes = [with_reads[i:i + per_launch] for i in range(0, len(with_reads), per_launch)]
    assert [[w for _, _, _, ws in parts for w in ws] for parts in launches] == flushes
    n_reads = 0
    for parts in launches:
        for kind, batch, windows, ws in parts:
            regs = [host[w.index] for w in ws]
            want = pack_regions(regs)
            if kind == "dev":
                got, hp = batch.to_host()
                assert batch.n_regions == len(ws) and batch.qmax == (int(np.diff(want.base_off).max()) if realign else 0)
                np.testing.assert_array_equal(hp, want.read_hp if want.read_hp is not None else np.zeros(want.n_reads, np.int32))
            else:
                got = batch
            for fld in RegionBatch.FIELDS:
                np.testing.assert_array_equal(getattr(got, fld), getattr(want, fld), err_msg="%s of %s" % (fld, ws[0]))
            assert got.contigs == want.contigs
            assert (windows is None and not realign) or [bytes(x) for x in windows] == [r.window for r in regs]
            n_reads += want.n_reads
    return n_reads


# ---- 1. batch identity ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_launch", [3, 1024])
def test_batches_equal_the_host_readers(hip_ctx, files, per_launch):
    bam, fa = str(files / "r.bam"), str(files / "d.fa")
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    # every region of the three contigs, and one that ends past the end of c1 (N padding), behind the others
    work = _work(bam, fa, extra=[("c1", 5400, 6600)])
    assert (work[0].contig, work[0].start) == ("c1", 0)
    assert region_from_files(b, f, "c1", 1900, 3100) is None                      # no reads, between two regions with reads
    assert region_from_files(b, f, "c1", 900, 2100) and region_from_files(b, f, "c1", 2900, 4100)
    assert region_from_files(b, f, "c1", 5400, 6600).ref.endswith(b"N" * 601)
    for s, e in ((2900, 4100), (3900, 5100), (4900, 5999)):   # the reverse-strand MAPQ 0 read over [3980, 4920): three regions
        assert s <= 4919 and e >= 3980 and any(r.mapq == 0 and r.is_reverse for r in region_from_files(b, f, "c1", s, e).reads)
    assert len(region_from_files(b, f, "c3", 0, 999).reads) == MAX_READS_IN_REGION   # the reservoir ran (1501 reads)
    launches, T = _launches(hip_ctx, bam, fa, work, per_launch)
    n = _same_as_host(launches, bam, fa, work, per_launch)
    assert n > 1500 + 300 and T["gpu_decode_groups_host"] == 0 and T["gpu_decode_slot_retries"] == 0
    if per_launch == 1024:   # two contigs (three) in one launch, one decoded batch
        assert len(launches) == 1 and [k for k, _, _, _ in launches[0]] == ["dev"]
        assert len(set(launches[0][0][1].to_host()[0].contigs)) == 3


def test_without_realign_no_windows_and_no_qmax(hip_ctx, files):
    bam, fa = str(files / "r.bam"), str(files / "d.fa")
    work = _work(bam, fa, "c2")
    launches, _ = _launches(hip_ctx, bam, fa, work, 2, realign=False)
    assert _same_as_host(launches, bam, fa, work, 2, realign=False) > 100


# ---- 2. host route -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_files(tmp_path_factory):
    """one contig of 60 kb in BGZF blocks of 256 bytes. A read of 600 bases at 500 skips 50 kb of the draft (an N operation):
    it is the first record over the index window three past region 0's, so the plan of the regions of window 0 ends two blocks
    past the block the read starts in, while its record (about 950 bytes) and the records behind it lie further on."""
    build.build_io()
    tmp = tmp_path_factory.mktemp("plong")
    rng = np.random.default_rng(78)
    L = 60_000
    bw.write_fasta(str(tmp / "d.fa"), [("c1", "".join(rng.choice(list("ACGT"), size=L)))])
    recs = [r for r in _reads(rng, 500, L, 0, 50, 600)]
    for r in recs:
        r["flag"], r["hp"], r["aux"] = r["flag"] & 0x10, None, b""
    long = dict(tid=0, pos=500, mapq=60, flag=0, cigar=[(0, 300), (3, 50_000), (0, 300)], seq="".join(rng.choice(list("ACGT"), size=600)),
                qual=[30] * 600, name="skip50k", aux=b"")
    recs = sorted(recs + [long], key=lambda r: r["pos"])
    assert sum(1 for r in recs if 500 < r["pos"] < 1000) >= 2   # records behind the long one that region 0's walk has to reach
    bw.write_bam(str(tmp / "r.bam"), [("c1", L)], recs, block_bytes=256)
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    return tmp


def test_a_read_past_the_plan_sends_its_group_the_host_route(hip_ctx, long_files):
    bam, fa = str(long_files / "r.bam"), str(long_files / "d.fa")
    work = _work(bam, fa, "c1:0-24000")
    launches, T = _launches(hip_ctx, bam, fa, work, 7)
    assert [len(g) for g in gd.region_groups(work)] == [16, 1, 7]
    assert T["gpu_decode_groups_host"] == 1 and T["gpu_decode_groups"] == 3
    kinds = [k for parts in launches for k, _, _, _ in parts]
    assert "host" in kinds and "dev" in kinds
    host_regions = [w.index for parts in launches for k, _, _, ws in parts if k == "host" for w in ws]
    assert len(host_regions) >= 10 and max(host_regions) < 16   # the first group: the regions of index window 0, in their places
    assert _same_as_host(launches, bam, fa, work, 7) > 100


# ---- 3. slot retry, 4. workspace -----------------------------------------------------------------------------------------

def test_too_few_slots_are_retried_once_with_the_safe_rule(hip_ctx, files):
    bam, fa = str(files / "r.bam"), str(files / "d.fa")
    work = _work(bam, fa, "c2")
    assert len(gd.region_groups(work)) == 1
    want, T0 = _launches(hip_ctx, bam, fa, work, 1024)
    got, T1 = _launches(hip_ctx, bam, fa, work, 1024, min_record_bytes=1 << 20)   # one slot per interval
    assert T0["gpu_decode_slot_retries"] == 0 and T1["gpu_decode_slot_retries"] == 1
    assert T1["gpu_inflate_launches"] == T0["gpu_inflate_launches"] + 1 == 2
    assert _same_as_host(got, bam, fa, work, 1024) == _same_as_host(want, bam, fa, work, 1024) > 100
    a, b = want[0][0][1].to_host()[0], got[0][0][1].to_host()[0]
    for fld in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(a, fld), getattr(b, fld), err_msg=fld)


def test_the_workspace_stays_under_a_small_budget(hip_ctx, files):
    bam, fa = str(files / "r.bam"), str(files / "d.fa")
    work = _work(bam, fa)
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    sizes = [(len(g), bamio.plan_blocks(b, [(w.contig, w.start, w.end) for w in g], 0, gd.MARGIN_BLOCKS).out_bytes) for g in gd.region_groups(work)]
    alone = [gd.decode_ws_bytes(n, n * gd.safe_slots(ob)) for n, ob in sizes]
    budget = max(alone) + 64          # every group fits on its own, no two of the larger ones together
    assert len(sizes) == 3 and budget < sum(alone)
    free, T0 = _launches(hip_ctx, bam, fa, work, 1024)
    tight, T1 = _launches(hip_ctx, bam, fa, work, 1024, ws_budget=budget)
    assert T0["gpu_inflate_launches"] == 1 and T0["gpu_decode_ws_peak_bytes"] > budget
    assert T1["gpu_inflate_launches"] >= 2 and 0 < T1["gpu_decode_ws_peak_bytes"] <= budget
    assert T1["gpu_decode_groups_host"] == 0 and T1["gpu_decode_groups_over_budget"] == 0
    # what is live at any one time - every scan whose buffers have not been let go - stays under the budget too: a scan's
    # regions are filled and its workspace released before the next scan runs
    assert T0["gpu_decode_ws_live_peak_bytes"] == T0["gpu_decode_ws_peak_bytes"]
    assert T1["gpu_decode_ws_peak_bytes"] <= T1["gpu_decode_ws_live_peak_bytes"] <= budget < sum(alone)
    assert T1["gpu_decode_buffers_live_peak_bytes"] > T1["gpu_decode_ws_live_peak_bytes"]
    assert T1["gpu_decode_buffers_live_peak_bytes"] < T0["gpu_decode_buffers_live_peak_bytes"]
    assert _same_as_host(tight, bam, fa, work, 1024) == _same_as_host(free, bam, fa, work, 1024)
    # a budget below the largest group's own need: that group is read on the host, the output stays the same
    small, T2 = _launches(hip_ctx, bam, fa, work, 1024, ws_budget=max(alone) - 8)
    assert T2["gpu_decode_groups_over_budget"] == T2["gpu_decode_groups_host"] == alone.count(max(alone))
    assert T2["gpu_decode_ws_peak_bytes"] <= T2["gpu_decode_ws_live_peak_bytes"] <= max(alone) - 8
    assert _same_as_host(small, bam, fa, work, 1024) == _same_as_host(free, bam, fa, work, 1024)


# ---- the builder's host form behind a decoded batch ----------------------------------------------------------------------------

def test_a_long_insert_takes_the_builders_host_form_with_the_decoded_batchs_host_copy(hip_ctx, tmp_path, monkeypatch):
    """one 9000-base insert in a 400-column region: more insert rows than the device form's workspace heuristic allows for
    (tests/test_polish_gpu.py), so the chain reports PV_ERR_LIMIT and builds from DecodedBatch.to_host()"""
    from pepper_thesis_amd import polish_summary
    build.build_io()
    rng = np.random.default_rng(3)
    bam, fa = str(tmp_path / "r.bam"), str(tmp_path / "d.fa")
    bw.write_fasta(fa, [("li", "".join(rng.choice(list("ACGT"), size=400)))])
    ins = "".join(rng.choice(list("ACGTN"), size=9000))
    recs = [dict(tid=0, pos=10, mapq=60, flag=0, cigar=[(0, 100)], seq="A" * 100, qual=[20] * 100, name="a"),
            dict(tid=0, pos=20, mapq=60, flag=16, cigar=[(0, 5), (1, 9000), (0, 60)], seq="C" * 5 + ins + "G" * 60, qual=[20] * 9065, name="b"),
            dict(tid=0, pos=20, mapq=60, flag=0, cigar=[(0, 5), (1, 2), (0, 60)], seq="T" * 67, qual=[20] * 67, name="c")]
    bw.write_bam(bam, [("li", 400)], recs)
    work = _work(bam, fa)
    launches, _ = _launches(hip_ctx, bam, fa, work, 4, realign=False)
    assert _same_as_host(launches, bam, fa, work, 4, realign=False) == 3
    (kind, db, _, ws), = launches[0]
    assert kind == "dev" and len(ws) == 1
    host_form, real = [], polish_summary.polish_summarize   # the batches the builder's host form was given

    def recording(ctx, batch, *a, **kw):
        host_form.append(batch)
        return real(ctx, batch, *a, **kw)

    monkeypatch.setattr(polish_summary, "polish_summarize", recording)
    chain = polish._DeviceChain(hip_ctx)
    _, n = chain.build_decoded(db)
    monkeypatch.undo()
    assert len(host_form) == 1 and n >= 10     # the device form gave up (PV_ERR_LIMIT); the chunks are the host form's
    copy = db.to_host()[0]
    for fld in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(host_form[0], fld), getattr(copy, fld), err_msg=fld)
    got = {k: getattr(chain.dout, k)[:n].cpu().numpy().copy() for k in ("images", "position", "index", "region", "chunk_id")}
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    want = hip_ctx.polish_summarize(pack_regions([region_from_files(b, f, "li", ws[0].start, ws[0].end)]))
    assert len(want.chunk_id) == n and int(want.index.max()) == 9000
    for k in got:
        np.testing.assert_array_equal(got[k], getattr(want, k), err_msg=k)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------

def _run(argv):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PV_SHARED_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "pepper_thesis_amd.pepper"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=STEP_TIMEOUT_S)
    assert r.returncode == 0, (argv, r.stderr[-3000:])
    return r.stderr


def _decode_lines(err):
    """the groups every `GPU DECODE:` log line reports (one line per process that read through the device path)"""
    import re
    return [int(n) for n in re.findall(r"GPU DECODE: (\d+) GROUPS", err)]


def _polish(t, tag, extra, processes=1):
    """-> the FASTA; the run's log says that it took the device path exactly where --gpu_decode was given"""
    out = str(t / tag)
    err = _run(["polish", "-b", str(t / "r.bam"), "-f", str(t / "d.fa"), "-m", str(t / "model.npz"), "-o", out, "-t", "3", "-bs", "8"] + extra)
    groups = _decode_lines(err)
    if "--gpu_decode" in extra:
        assert len(groups) == processes and min(groups) > 0, err[-2000:]
    else:
        assert groups == [], err[-2000:]
    return open(os.path.join(out, "_pepper_polished.fa"), "rb").read()


@pytest.mark.parametrize("realign", [False, True])
def test_polish_gpu_decode_writes_the_same_fasta(files, realign):
    extra = ["--realign"] if realign else []
    tag = "r" if realign else "n"
    want = _polish(files, "host_" + tag, ["-d_ids", "0"] + extra)
    assert want.startswith(b">c1\n") and b"\n>c2\n" in want and b"\n>c3\n" in want
    assert _polish(files, "dev_" + tag, ["-d_ids", "0", "--gpu_decode"] + extra) == want
    assert _polish(files, "dev2_" + tag, ["-d_ids", "0,0", "--gpu_decode"] + extra, processes=2) == want   # both ranks


def test_polish_gpu_decode_with_a_host_route_group_writes_the_same_fasta(long_files):
    want = _polish(long_files, "host", ["-d_ids", "0", "-r", "c1:0-24000", "--realign"])
    assert _polish(long_files, "dev", ["-d_ids", "0", "-r", "c1:0-24000", "--realign", "--gpu_decode"]) == want


def test_make_images_gpu_decode_writes_the_same_files(files):
    from pepper_thesis_amd.hdf5io import PolishImageStore
    t = files
    dirs = {}
    for tag, extra in (("host", []), ("dev", ["--gpu_decode"])):
        dirs[tag] = str(t / ("img_" + tag))
        err = _run(["make_images", "-b", str(t / "r.bam"), "-f", str(t / "d.fa"), "-o", dirs[tag], "-t", "3", "--realign"] + extra)
        assert [n > 0 for n in _decode_lines(err)] == ([True] if extra else []), err[-2000:]
    names = {tag: sorted(os.listdir(d)) for tag, d in dirs.items()}
    assert len(names["host"]) == len(names["dev"]) == 3
    n_chunks = 0
    for a, b in zip(names["host"], names["dev"]):
        assert a.rsplit("_", 2)[0] == b.rsplit("_", 2)[0]   # the same thread number; the time stamp differs
        with PolishImageStore(os.path.join(dirs["host"], a)) as sa, PolishImageStore(os.path.join(dirs["dev"], b)) as sb:
            assert sa.summaries() == sb.summaries()
            for name in sa.summaries():
                ca, cb = sa.read_chunk(name), sb.read_chunk(name)
                assert sorted(ca) == sorted(cb)
                for k in ca:
                    assert np.array_equal(ca[k], cb[k]), (name, k)
                n_chunks += 1
    assert n_chunks >= 10
