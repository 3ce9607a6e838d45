"""CPU: the host side of the `--gpu_decode` reader mode. pvio_plan_intervals' interval / chunk table together with
pvio_plan_blocks' block table must lead a plain walker - a Python restatement of the device's record walk (k_bam_walk in
csrc/bam_decode.hip) over blocks inflated with zlib - to exactly the records the host reader parses for the interval; and the
flag parses, implies gpu_inflate and refuses helper threads."""
import struct
import zlib

import numpy as np
import pytest

import bam_writer as bw
from pepper_thesis_amd import bamio, build, cli

SAFE = 100


def walk_interval(plan, data, ivp, k):
    """-> (records as (tid, pos, body bytes), status) of interval k: 'ok', or 'past_plan' when the walk needs a block the
    plan does not hold. The device's rules: start at every chunk's begin, continue while tell() < chunk end (a block consumed
    to its end reports offset 0 of the next one), the stream is contiguous only where next_coffset[i] == coffset[i + 1], skip
    lower tids, end the interval at the first record of a higher tid or with pos >= re."""
    co, nx, isz, oo = plan.coffset, plan.next_coffset, plan.isize, plan.out_off
    tid, qend = int(ivp.tid[k]), int(ivp.re[k])
    out = []

    def advance(b, target):
        while target > oo[b] + isz[b]:
            if b + 1 >= plan.n_blocks or co[b + 1] != nx[b]:
                return None
            b += 1
        return b

    for ci in range(int(ivp.chunk_off[k]), int(ivp.chunk_off[k + 1])):
        cbeg, cend = int(ivp.chunk_beg[ci]), int(ivp.chunk_end[ci])
        b = int(np.searchsorted(co, cbeg >> 16))
        if b >= plan.n_blocks or co[b] != cbeg >> 16:
            return out, "past_plan"
        p = int(oo[b]) + (cbeg & 0xFFFF)
        while True:
            bend = int(oo[b] + isz[b])
            tell = (int(nx[b]) << 16) if (isz[b] > 0 and p >= bend) else ((int(co[b]) << 16) | ((p - int(oo[b])) & 0xFFFF))
            if tell >= cend:
                break
            b = advance(b, p + 4)
            if b is None:
                return out, "past_plan"
            bs = struct.unpack_from("<I", data, p)[0]
            assert 32 <= bs <= 1 << 30
            p += 4
            b = advance(b, p + bs)
            if b is None:
                return out, "past_plan"
            rtid, rpos = struct.unpack_from("<ii", data, p)
            if rtid != tid:
                if rtid > tid:
                    return out, "ok"
            else:
                if rpos >= qend:
                    return out, "ok"
                out.append((rtid, rpos, bytes(data[p:p + bs])))
            p += bs
    return out, ("past_plan" if ivp.dropped[k] else "ok")


def inflate_plan(plan):
    data = bytearray(plan.out_bytes)
    for i in range(plan.n_blocks):
        raw = zlib.decompress(plan.payload[plan.in_off[i]:plan.in_off[i] + plan.clen[i]].tobytes(), -15)
        assert len(raw) == plan.isize[i] and zlib.crc32(raw) == plan.crc[i]
        data[plan.out_off[i]:plan.out_off[i] + len(raw)] = raw
    return data


def body_key(rec):
    """what identifies a bam_writer record inside its encoded body: (tid, pos, name)"""
    return rec["tid"], rec["pos"], rec.get("name", "r")


def walked_key(w):
    l_name = w[2][8]
    return w[0], w[1], w[2][32:32 + l_name - 1].decode()


def check_file(bam, recs, groups, contigs, expect_ok=True, min_checked=None):
    """-> intervals checked. expect_ok=False: an interval whose walk leaves the plan is not compared (the device hands it to the
    host reader), but at least min_checked (default: all but one) must have been"""
    h = bamio.BamHandler(bam)
    n_checked, n_all = 0, sum(len(g) for g in groups)
    for ivs in groups:
        plan = bamio.plan_blocks(h, ivs, SAFE, 1)
        ivp = bamio.plan_intervals(h, ivs, SAFE)
        data = inflate_plan(plan)
        assert ivp.n_intervals == len(ivs) and len(ivp.chunk_off) == len(ivs) + 1
        for k, (contig, start, end) in enumerate(ivs):
            tid = contigs.index(contig)
            rs, re_ = max(0, start - SAFE), end + SAFE
            assert (int(ivp.tid[k]), int(ivp.rs[k]), int(ivp.re[k])) == (tid, rs, re_)
            got, status = walk_interval(plan, data, ivp, k)
            if expect_ok:
                assert status == "ok", (ivs, k)
            elif status != "ok":
                continue
            # before clipping: every record of the contig that starts before `re` and that the index can reach is visited in
            # file order; the visited ones that overlap the window are exactly the writer's overlapping records
            over = [r for r in recs if r["tid"] == tid and r["pos"] < re_ and r["pos"] + max(bw.ref_len(r["cigar"]), 1) > rs]
            seen = [walked_key(w) for w in got]
            pos_in = [i for i, r in enumerate(recs) if body_key(r) in set(seen)]
            assert seen == [body_key(recs[i]) for i in pos_in]                       # file order, no record twice
            assert [body_key(r) for r in over] == [x for x in seen if x in {body_key(r) for r in over}]
            assert {body_key(r) for r in over} <= set(seen)
            # after clipping: the walked records through the restated rules == the host reader's get_reads
            walked = [recs[i] for i in pos_in]
            for supp, mq in ((False, 5), (True, 0)):
                exp = bw.expected_reads(walked, tid, rs, re_, supp, mq)
                host = h.get_reads(contig, rs, re_, supp, mq, 0)
                assert [(e["pos"], e["seq"], e["name"]) for e in exp] == [(g.pos, g.bases.decode(), g.query_name) for g in host]
            n_checked += 1
    assert n_checked >= (n_all if expect_ok else (max(1, n_all - 1) if min_checked is None else min_checked)), (n_checked, n_all)
    return n_checked


@pytest.fixture(scope="module")
def fixture_files(tmp_path_factory):
    """the test_bamio module fixture, rebuilt"""
    build.build_io()
    d = tmp_path_factory.mktemp("dec")
    rng = np.random.default_rng(5)
    seqs = [("chr20", "".join(rng.choice(list("ACGTacgtN"), size=130_000, p=[.22, .22, .22, .22, .02, .02, .02, .02, .04]))),
            ("chrM", "".join(rng.choice(list("ACGT"), size=16_500)))]
    bw.write_fasta(str(d / "ref.fa"), seqs, width=70)
    recs = bw.random_records(rng, 900, 130_000, tid=0) + bw.random_records(rng, 60, 16_500, tid=1, mean_len=800)
    bw.write_bam(str(d / "reads.bam"), [(n, len(s)) for n, s in seqs], recs)
    return dict(bam=str(d / "reads.bam"), fa=str(d / "ref.fa"), recs=recs)


def test_walker_on_the_bamio_fixture_and_two_contigs(fixture_files):
    groups = [[("chr20", 0, 1000)], [("chr20", 16_300, 16_500), ("chr20", 49_900, 60_100)], [("chr20", 100_000, 129_999)],
              [("chr20", 65_535, 65_537), ("chrM", 100, 16_400)], [("chrM", 0, 16_499), ("chr20", 129_000, 129_999)]]
    check_file(fixture_files["bam"], fixture_files["recs"], groups, ["chr20", "chrM"])


def _records(seed, n, length, mean_len):
    rng = np.random.default_rng(seed)
    recs = bw.random_records(rng, n, length, tid=0, mean_len=mean_len, allow_skip=False)
    for i, r in enumerate(recs):
        r["name"] = "q%d" % i
    return recs


def test_walker_on_full_64k_blocks(tmp_path):
    """the native writer fills every block to the limit: records straddle block boundaries all the time"""
    from pepper_thesis_amd.batch import Read, Region, pack_regions
    build.build_io()
    recs = _records(8, 400, 50_000, 3000)
    for i, r in enumerate(recs):
        r["flag"], r["mapq"], r["hp"], r["name"] = r["flag"] & 0x10, 60, None, "r%d" % i   # (the native writer's names)
        r["seq"] = r["seq"].replace("N", "A")
    reads = [Read.make(r["pos"], np.asarray([(l << 4) | op for op, l in r["cigar"]], np.uint32), r["seq"], r["qual"],
                       bool(r["flag"] & 0x10), r["mapq"]) for r in recs]
    b = pack_regions([Region(0, 49_999, b"A" * 50_000, reads)])
    path = str(tmp_path / "native.bam")
    bamio.write_bam(path, [("c1", 50_000)], np.zeros(len(reads), np.int32), b, level=1)
    check_file(path, recs, [[("c1", 10_000, 40_000)], [("c1", 0, 5000), ("c1", 45_000, 49_999)]], ["c1"])


def test_walker_when_chunks_end_on_block_ends_and_intervals_have_several_chunks(tmp_path):
    """one record per block: every chunk of the index ends exactly where a block ends (tell() then reports the next block);
    long and short reads land in bins of different levels, so an interval has several chunks"""
    build.build_io()
    recs = _records(21, 300, 200_000, 2500) + _records(22, 40, 200_000, 30_000)
    for i, r in enumerate(recs):
        r["name"] = "m%d" % i
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    path = str(tmp_path / "one.bam")
    bw.write_bam(path, [("c1", 200_000)], recs, block_records=1)
    h = bamio.BamHandler(path)
    ivp = bamio.plan_intervals(h, [("c1", 60_000, 90_000)], SAFE)
    assert ivp.n_chunks >= 2
    check_file(path, recs, [[("c1", 60_000, 90_000)], [("c1", 0, 20_000), ("c1", 150_000, 199_999)]], ["c1"], expect_ok=False)
    path2 = str(tmp_path / "few.bam")
    bw.write_bam(path2, [("c1", 200_000)], recs, block_records=3)
    check_file(path2, recs, [[("c1", 100_000, 120_000)]], ["c1"], expect_ok=False)


def test_interval_chunks_are_the_chunks_the_block_plan_covers(fixture_files):
    h = bamio.BamHandler(fixture_files["bam"])
    ivs = [("chr20", 20_000, 30_000), ("chr20", 90_000, 100_000), ("chrM", 0, 5000)]
    plan, ivp = bamio.plan_blocks(h, ivs, SAFE, 1), bamio.plan_intervals(h, ivs, SAFE)
    cos = set(int(c) for c in plan.coffset)
    assert ivp.n_chunks > 0 and all(int(b) >> 16 in cos for b in ivp.chunk_beg)
    assert all(int(b) < int(e) for b, e in zip(ivp.chunk_beg, ivp.chunk_end))
    for k in range(len(ivs)):
        cb = ivp.chunk_beg[ivp.chunk_off[k]:ivp.chunk_off[k + 1]]
        assert list(cb) == sorted(cb)
    with pytest.raises(IOError):
        bamio.plan_intervals(h, [("nope", 0, 10)], SAFE)


# ---- the flag ------------------------------------------------------------------------------------------------------------

def test_gpu_decode_flag_parses_and_implies_gpu_inflate():
    cv = cli.call_variant_parser().parse_args(["-b", "a.bam", "-f", "a.fa", "-m", "m.pkl", "-o", "out", "--ont_r9_guppy5_sup", "--gpu_decode"])
    assert cv.gpu_decode is True and cv.gpu_inflate is True
    mi = cli.make_images_parser().parse_args(["-b", "a.bam", "-f", "a.fa", "-o", "out", "--ont_r9_guppy5_sup", "--gpu_decode"])
    assert mi.gpu_decode is True and mi.gpu_inflate is True
    off = cli.make_images_parser().parse_args(["-b", "a.bam", "-f", "a.fa", "-o", "out", "--ont_r9_guppy5_sup"])
    assert off.gpu_decode is False and off.gpu_inflate is False
    only = cli.call_variant_parser().parse_args(["-b", "a.bam", "-f", "a.fa", "-m", "m.pkl", "-o", "out", "--ont_r9_guppy5_sup", "--gpu_inflate"])
    assert only.gpu_inflate is True and only.gpu_decode is False


def test_gpu_decode_refuses_helper_threads_and_a_missing_context(fixture_files):
    from pepper_thesis_amd.make_images import region_batches
    with pytest.raises(ValueError, match="gpu_decode"):
        region_batches(fixture_files["bam"], fixture_files["fa"], "chr20:0-20000", 10_000, gpu_decode=True, inflate_helpers=2, ctx=object())
    with pytest.raises(ValueError, match="gpu_decode"):
        region_batches(fixture_files["bam"], fixture_files["fa"], "chr20:0-20000", 10_000, gpu_decode=True, ctx=None)
