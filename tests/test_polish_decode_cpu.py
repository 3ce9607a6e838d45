"""CPU: everything around the kernels of the polisher's `--gpu_decode` read path - the flags, the read limit keyword of the
native fill, the grouping / workspace policy (pure functions of the plan sizes) and polish_pieces' launch composition with a
stub chain and a stub decoder."""
import argparse
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_writer as bw  # noqa: E402
from pepper_thesis_amd import bamio, build, cli, gpu_decode as gd, pepper, polish  # noqa: E402
from pepper_thesis_amd.batch import RegionBatch, pack_regions  # noqa: E402
from pepper_thesis_amd.polish_summary import MAX_READS_IN_REGION, region_from_files  # noqa: E402


# ---- flags ------------------------------------------------------------------------------------------------------------

def test_flags():
    base = ["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl", "-o", "out"]
    assert cli.polish_parser().parse_args(base).gpu_decode is False
    assert cli.polish_parser().parse_args(base + ["--gpu_decode"]).gpu_decode is True
    ap = pepper.parser()
    assert ap.parse_args(["polish"] + base).gpu_decode is False
    assert ap.parse_args(["polish"] + base + ["--gpu_decode", "--realign"]).gpu_decode is True
    mi = ["make_images", "-b", "r.bam", "-f", "d.fa", "-o", "img"]
    assert ap.parse_args(mi).gpu_decode is False
    assert ap.parse_args(mi + ["--gpu_decode"]).gpu_decode is True
    assert not hasattr(ap.parse_args(["call_consensus", "-i", "img", "-m", "m.pkl", "-o", "pred"]), "gpu_decode")
    assert not hasattr(ap.parse_args(["stitch", "-i", "pred", "-o", "out"]), "gpu_decode")
    for argv in (["call_consensus", "-i", "img", "-m", "m.pkl", "-o", "pred", "--gpu_decode"],
                 ["stitch", "-i", "pred", "-o", "out", "--gpu_decode"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)


def test_the_flag_travels_to_every_rank():
    from pepper_thesis_amd import polish_rank
    base = ["-b", "r.bam", "-f", "d.fa", "-m", "m.pkl", "-o", "out", "-d_ids", "0,0"]
    for extra in ([], ["--gpu_decode"], ["--gpu_decode", "--realign"]):
        args = cli.polish_parser().parse_args(base + extra)
        argv = polish_rank.rank_argv(args, polish_rank.plan_ranks(args.device_ids, args.threads))
        again = cli.polish_parser(argparse.ArgumentParser()).parse_args(argv)
        assert again.gpu_decode is bool(extra) and again.realign is ("--realign" in extra)


# ---- the read limit ---------------------------------------------------------------------------------------------------

def _short_reads(n, tid=0, pos0=100, length=8):
    return [dict(tid=tid, pos=pos0 + (i % 700), mapq=60, flag=0, cigar=[(0, length)], seq="ACGTACGT"[:length],
                 qual=[10 + i % 40] * length, name="s%d" % i) for i in range(n)]


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """one 1000-base contig with 1501 reads of 8 bases: the smallest input at which the polisher's reservoir runs"""
    build.build_io()
    tmp = tmp_path_factory.mktemp("many")
    rng = np.random.default_rng(5)
    bw.write_fasta(str(tmp / "d.fa"), [("m1", "".join(rng.choice(list("ACGT"), size=1000)))])
    recs = sorted(_short_reads(1501), key=lambda r: r["pos"])
    bw.write_bam(str(tmp / "r.bam"), [("m1", 1000)], recs, block_records=200)
    return str(tmp / "r.bam"), str(tmp / "d.fa")


class _Recorder:
    """the native library with the read limit of every fill recorded"""

    def __init__(self, lib):
        self._lib, self.limits = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in ("pvio_fill_batch", "pvio_fill_batch_blocks"):
            def call(*a):
                self.limits.append((name, int(a[10])))
                return fn(*a)
            return call
        return fn


def test_read_limit_default_and_keyword(many, monkeypatch):
    bam, fa = many
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    rec = _Recorder(bamio.load())
    monkeypatch.setattr(bamio, "_lib", rec)
    iv = [("m1", 0, 999)]
    everything = bamio.fill_batch(b, f, iv, 0, False, 1.0, 0)
    p = bamio.plan_blocks(b, iv, 0, 2)
    bamio.fill_batch_blocks(b, f, iv, p.coffset[:0], p.next_coffset[:0], p.isize[:0], p.out_off[:0], np.zeros(1, np.uint8), 0, False, 1.0, 0)
    assert rec.limits == [("pvio_fill_batch", 5000), ("pvio_fill_batch_blocks", 5000)]   # existing callers: today's value
    assert everything.batch.n_reads == 1501
    some = bamio.fill_batch(b, f, iv, 0, False, 1.0, 0, max_reads=1500)
    blocks = bamio.fill_batch_blocks(b, f, iv, p.coffset[:0], p.next_coffset[:0], p.isize[:0], p.out_off[:0], np.zeros(1, np.uint8), 0,
                                     False, 1.0, 0, max_reads=1500)
    assert rec.limits[2:] == [("pvio_fill_batch", 1500), ("pvio_fill_batch_blocks", 1500)]
    keep = bamio.reservoir_indices(1501, 1.0, 1500)
    assert len(keep) == 1500 and sorted(keep.tolist()) != keep.tolist()   # the reservoir replaced a read: not the first 1500
    for got in (some.batch, blocks.batch):
        assert got.n_reads == 1500
        np.testing.assert_array_equal(got.read_pos, everything.batch.read_pos[keep])
        np.testing.assert_array_equal(got.quals.reshape(1500, 8), everything.batch.quals.reshape(1501, 8)[keep])


def test_region_from_files_keeps_1500_in_reservoir_order(many):
    bam, fa = many
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    assert MAX_READS_IN_REGION == 1500
    reg = region_from_files(b, f, "m1", 0, 999)
    assert len(reg.reads) == 1500
    filled = bamio.fill_batch(b, f, [("m1", 0, 999)], 0, False, 1.0, 0, max_reads=MAX_READS_IN_REGION)
    ref = filled.batch   # (views of the native batch: `filled` owns them)
    got = pack_regions([reg])
    for fld in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(got, fld), getattr(ref, fld), err_msg=fld)


# ---- grouping and workspace policy ------------------------------------------------------------------------------------

def test_region_groups_cover_the_work_once_and_in_order():
    work = []
    for ci, (contig, n) in enumerate((("a", 40), ("b", 1), ("c", 17))):
        for a, e in polish.polish_intervals(n * 1000):
            work.append(polish.Work(len(work), ci, contig, a, e))
    for sub in (work, work[0::2], work[1::2], work[:1], []):
        groups = gd.region_groups(sub)
        assert [w for g in groups for w in g] == list(sub)
        for g in groups:
            assert 1 <= len(g) <= gd.GROUP_REGIONS and len({w.contig for w in g}) == 1
            assert len({w.start >> 14 for w in g}) == 1 and [w.start for w in g] == sorted(w.start for w in g)
    assert len(gd.region_groups(work)) < len(work) / 4   # the regions of one index window do share a group


def _check_plan(sizes, budget, mrb):
    plan = gd.plan_launches(sizes, budget, mrb)
    assert [gi for _, gis, _ in plan for gi in gis] == list(range(len(sizes)))   # every group once, in order
    for kind, gis, per in plan:
        if kind == "host":
            n, ob = sizes[gis[0]]
            assert len(gis) == 1 and gd.decode_ws_bytes(n, n * gd.safe_slots(ob)) > budget
            continue
        assert kind == "dev" and len(per) == len(gis)
        slots = 0
        for gi, p in zip(gis, per):
            n, ob = sizes[gi]
            assert 1 <= p <= gd.safe_slots(ob) and p == gd.interval_slots(ob, mrb)
            assert gd.decode_ws_bytes(n, n * gd.safe_slots(ob)) <= budget   # a retry with the safe rule fits
            slots += n * p
        assert gd.decode_ws_bytes(sum(sizes[gi][0] for gi in gis), slots) <= budget
    return plan


def test_plan_launches_policy():
    rng = np.random.default_rng(3)
    sizes = [(int(rng.integers(1, 17)), int(rng.integers(0, 3_000_000))) for _ in range(60)] + [(16, 40_000_000), (1, 0), (3, 35)]
    for budget in (1 << 20, 8 << 20, 64 << 20, 1 << 34):
        for mrb in (36, 200, 4096):
            _check_plan(sizes, budget, mrb)
    # the safe rule is the issue's: bytes / 36 + 1 slots per interval, 60 bytes of workspace each
    assert gd.safe_slots(3600) == 101 and gd.interval_slots(3600) == 101 and gd.interval_slots(3600, 360) == 11
    assert gd.interval_slots(3600, 1) == 101   # never more than the safe rule
    assert 60 * 1000 <= gd.decode_ws_bytes(1, 1000) <= 60 * 1000 + 256
    plan = _check_plan([(16, 41_000_000)] * 3 + [(4, 100_000)], 1 << 30, 36)   # 16 x 1.139 M slots x 60 bytes = 1.093e9 > 2^30
    assert [k for k, _, _ in plan] == ["host", "host", "host", "dev"]
    plan = _check_plan([(4, 1_000_000)] * 5, 16 << 20, 36)   # 4 x 27778 slots x 60 bytes = 6.7 MB per group: two per scan
    assert [len(g) for _, g, _ in plan] == [2, 2, 1]
    assert gd.plan_launches([(4, 1_000_000)] * 5) == [("dev", [0, 1, 2, 3, 4], [27778] * 5)]   # no budget: one scan
    # a retry is a plan of the groups that ran out, with the safe rule
    retry = gd.plan_launches([(4, 1_000_000)] * 2, 16 << 20, gd.REC_MIN_BYTES)
    assert retry == [("dev", [0, 1], [gd.safe_slots(1_000_000)] * 2)]


# ---- polish_pieces: launch composition ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """three contigs: `a` (6 regions, reads at both ends only: the regions between have none), `b` and `c` (full cover)"""
    build.build_io()
    tmp = tmp_path_factory.mktemp("small")
    rng = np.random.default_rng(11)
    contigs = [("a", 6000), ("b", 4000), ("c", 2500)]
    bw.write_fasta(str(tmp / "d.fa"), [(n, "".join(rng.choice(list("ACGT"), size=L))) for n, L in contigs])
    recs = []
    for tid, (_, L) in enumerate(contigs):
        for i in range(40):
            pos = int(rng.integers(0, L - 400))
            if tid == 0 and 1300 < pos + 300 and pos < 3700:
                continue
            n = int(rng.integers(50, 300))
            recs.append(dict(tid=tid, pos=pos, mapq=int(rng.choice([0, 20, 60])), flag=int(rng.choice([0, 16])), cigar=[(0, n)],
                             seq="".join(rng.choice(list("ACGT"), size=n)), qual=[30] * n, name="r%d_%d" % (tid, i)))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), contigs, recs, block_records=7)
    return str(tmp / "r.bam"), str(tmp / "d.fa")


class _Chain:
    """stub chain: records the regions of every call together with the launch counter at that moment"""
    ctx = None

    def __init__(self, T):
        self.T, self.calls = T, []

    def run(self, batch, windows=None):
        starts = [int(s) for s in batch.ref_start]
        self.calls.append((self.T.get("batches", 0), "host", list(zip(batch.contigs, starts)), windows))
        return polish.ChainResult(np.arange(len(starts) + 1), b"".join(b"%d" % (s % 10) for s in starts))

    def run_decoded(self, dec, windows=None):
        self.calls.append((self.T.get("batches", 0), "dev", list(dec), windows))
        return polish.ChainResult(np.arange(len(dec) + 1), b"".join(b"%d" % (s % 10) for _, s in dec))


class _Decoder:
    """stub decoder: scan_groups counts reads with the host reader and sends the groups of `host_contig` the host route;
    realize hands out the regions' names in place of a decoded batch"""

    def __init__(self, bam, fa, T, host_contig, realign):
        self.T, self.host_contig, self.realign = T, host_contig, realign
        self.h = (bamio.BamHandler(bam), bamio.FastaHandler(fa))
        self.scans = 0

    def scan_groups(self, planned):
        self.scans += 1
        key, out = object(), []
        for gi, g in enumerate(planned):
            regions = [region_from_files(self.h[0], self.h[1], c, s, e, realign=self.realign) for c, s, e in g.ivs]
            reads = [0 if r is None else len(r.reads) for r in regions]
            if g.ivs[0][0] == self.host_contig:
                self.T["gpu_decode_groups_host"] += 1
                out.append(gd.GroupScan(g, "host", reads, g, regions=regions))
            else:
                out.append(gd.GroupScan(g, "dev", reads, key, gi))
        return out

    def realize(self, launch):
        parts = []
        for kind, key, regs in launch:
            works = [gs.group.works[k] for gs, k in regs]
            if kind == "host":
                rs = [gs.regions[k] for gs, k in regs]
                parts.append(("host", pack_regions(rs), [r.window for r in rs] if self.realign else None, works))
            else:
                win = [gs.group.windows[k] for gs, k in regs] if self.realign else None
                parts.append(("dev", [(w.contig, w.start) for w in works], win, works))
        return parts

    def iterate(self, gen, depth=2):
        return gen   # (the real decoder runs it on its service thread)

    def close(self):
        self.closed = True


@pytest.mark.parametrize("realign", [False, True])
@pytest.mark.parametrize("batch_size", [2, 6, 7, 64])
def test_polish_pieces_launches_equal_the_host_paths(small, batch_size, realign):
    bam, fa = small
    work, _ = polish.polish_work(bamio.FastaHandler(fa), bamio.BamHandler(bam), None)
    assert [w.contig for w in work].count("a") == 6
    T0 = {}
    host = _Chain(T0)
    want = list(polish.polish_pieces(bam, fa, work, host, batch_size, 3, realign, T0))
    with_reads = [(c, s) for _, _, regs, _ in host.calls for c, s in regs]
    assert 0 < len(with_reads) < len(work)    # some regions of `a` have no reads
    T1 = {}
    chain = _Chain(T1)
    decs = []

    def open_decoder(T):
        decs.append(_Decoder(bam, fa, T, "b", realign))
        return decs[0]

    got = list(polish.polish_pieces(bam, fa, work, chain, batch_size, 3, realign, T1, gpu_decode=True, open_decoder=open_decoder))
    assert got == want
    assert decs[0].closed and T1["gpu_decode_groups_host"] == 1 and T1["plan_s"] > 0 and "decode_s" in T1
    assert T1["batches"] == T0["batches"] and T1["regions"] == T0["regions"] == len(with_reads)
    assert T1["chain_runs"] == len(chain.calls) >= T1["batches"]
    launches = {}
    for n, kind, regs, windows in chain.calls:
        launches.setdefault(n, []).extend(regs)
        assert (kind == "host") == all(c == "b" for c, _ in regs) and (windows is None) != realign
        assert windows is None or len(windows) == len(regs)
    # the same regions in the same launches, in the same order
    assert [launches[n] for n in sorted(launches)] == [regs for _, _, regs, _ in host.calls]
    if realign:   # the planner's windows are the host reader's
        w_host = [w for _, _, _, ws in host.calls for w in ws]
        w_dev = [bytes(w) for _, _, _, ws in chain.calls for w in ws]
        assert w_dev == w_host


def test_planned_group_pads_the_draft_and_fetches_windows(small):
    bam, fa = small
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    ivs = [("c", 0, 1100), ("c", 1900, 2499), ("c", 2000, 3200)]   # the last one ends past the contig end (2500 bases)
    g = gd.PlannedGroup(b, f, ivs, 0, pad_ref=True, windows=True)
    for k, (c, s, e) in enumerate(ivs):
        reg = region_from_files(b, f, c, s, e, realign=True)
        assert g.refs[k].tobytes() == reg.ref and len(reg.ref) == e - s + 1 and g.windows[k] == reg.window
    assert g.refs[2].tobytes().endswith(b"N" * 701) and len(g.windows[2]) == 500
    plain = gd.PlannedGroup(b, f, ivs, 0)   # today's planner: what the FASTA returns, no windows
    assert plain.refs[2].size == 500 and plain.windows is None


def test_compose_launches_hands_over_every_part_once_and_as_soon_as_it_is_complete():
    class G:
        def __init__(self, n):
            self.ivs = [("x", i, i) for i in range(n)]
    k1, k2 = object(), object()
    a, b, c = gd.GroupScan(G(3), "dev", [1, 1, 1], k1), gd.GroupScan(G(2), "dev", [1, 0], k1), gd.GroupScan(G(2), "dev", [2, 2], k2)
    seen = []   # (what the scans had handed out when the part was closed, the part)

    def scans():
        for x in (a, b, None, c, None):
            seen.append(("scan", x))
            yield x

    def on_part(part):
        seen.append(("part", part[1], [(gs, k) for gs, k in part[2]]))
        return ("done", len(part[2]))

    assert list(gd.compose_launches(scans(), 2, on_part)) == [[("done", 2)], [("done", 2)], [("done", 2)]]
    parts = [x for x in seen if x[0] == "part"]
    assert [p[2] for p in parts] == [[(a, 0), (a, 1)], [(a, 2), (b, 0)], [(c, 0), (c, 1)]]   # every region once, in order
    # the last part of the first scan is closed at the scan's None: before the next scan is asked for
    assert seen.index(parts[1]) < seen.index(("scan", c))
    # without on_part the parts come as they are
    plain = list(gd.compose_launches([a, b, None, c], 3))
    assert [[(k, key is k1, len(regs)) for k, key, regs in launch] for launch in plain] == [[("dev", True, 3)], [("dev", True, 1), ("dev", False, 2)]]


def test_compose_launches_raises_a_groups_error_in_its_place():
    class G:
        def __init__(self, n):
            self.ivs = [("x", i, i) for i in range(n)]
    a = gd.GroupScan(G(3), "dev", [1, 0, 2], "k")
    bad = gd.GroupScan(G(1), IOError("corrupt"), [0], "k")
    it = gd.compose_launches([a, bad], 2)
    assert [(k, [i for _, i in regs]) for k, _, regs in next(it)] == [("dev", [0, 2])]
    with pytest.raises(IOError, match="corrupt"):
        next(it)
