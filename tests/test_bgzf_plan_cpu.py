"""CPU: the block planner of the GPU-inflate reader mode (pvio_plan_blocks) and the record parse from a table of inflated
blocks (pvio_fill_batch_blocks). The blocks are inflated here with Python's zlib: fill_batch_blocks must give exactly the
arrays of fill_batch, and a block missing from the table must be read and inflated on the host (and counted)."""
import struct
import zlib

import numpy as np
import pytest

import bam_writer as bw
from pepper_thesis_amd import bamio, build
from pepper_thesis_amd.batch import Read, Region, RegionBatch, pack_regions

SAFE = 100


def _inflate(plan):
    """the planned blocks inflated with zlib, end to end at plan.out_off"""
    data = np.zeros(max(plan.out_bytes, 1), np.uint8)
    for i in range(plan.n_blocks):
        a = int(plan.in_off[i])
        raw = zlib.decompress(plan.payload[a:a + int(plan.clen[i])].tobytes(), -15)
        assert len(raw) == plan.isize[i] and zlib.crc32(raw) & 0xFFFFFFFF == plan.crc[i]
        o = int(plan.out_off[i])
        data[o:o + len(raw)] = np.frombuffer(raw, np.uint8)
    return data


def _native_bam(path, level, n_reads=300, length=60_000, mean_len=3000, seed=8):
    rng = np.random.default_rng(seed)
    recs = bw.random_records(rng, n_reads, length, tid=0, mean_len=mean_len, allow_skip=False)
    for r in recs:
        r["seq"] = r["seq"].replace("N", "A")
    reads = [Read.make(r["pos"], np.asarray([(l << 4) | op for op, l in r["cigar"]], np.uint32), r["seq"], r["qual"],
                       bool(r["flag"] & 0x10), r["mapq"]) for r in recs]
    b = pack_regions([Region(0, length - 1, b"A" * length, reads)])
    b.read_flags = np.asarray([r["flag"] & 0x10 and 1 or 0 for r in recs], np.uint8)
    b.read_mapq = np.asarray([r["mapq"] for r in recs], np.uint8)
    bamio.write_bam(path, [("c1", length)], np.zeros(len(reads), np.int32), b, level=level)
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    build.build_io()
    d = tmp_path_factory.mktemp("plan")
    rng = np.random.default_rng(21)
    n = 60_000
    seq = "".join(rng.choice(list("ACGT"), size=n))
    fa = str(d / "ref.fa")
    bw.write_fasta(fa, [("c1", seq)])
    out = dict(fa=fa)
    recs = bw.random_records(rng, 1500, n, tid=0, mean_len=900, allow_skip=False)
    bw.write_bam(str(d / "py.bam"), [("c1", n)], recs)               # the test-side writer: zlib level 6, 40 records a block
    out["py"] = str(d / "py.bam")
    out["native1"] = _native_bam(str(d / "n1.bam"), 1)                 # the native writer: full 64 KiB blocks
    out["native6"] = _native_bam(str(d / "n6.bam"), 6)
    out["long"] = _native_bam(str(d / "long.bam"), 1, n_reads=40, mean_len=45_000, seed=3)   # records longer than a block
    return out


INTERVALS = [[("c1", 0, 5000)], [("c1", 20_000, 30_000), ("c1", 25_000, 35_000), ("c1", 50_000, 59_999)],
             [("c1", 10_000, 10_100), ("c1", 40_000, 52_000)]]


@pytest.mark.parametrize("which", ["py", "native1", "native6", "long"])
def test_planned_blocks_match_the_file(files, which):
    raw = open(files[which], "rb").read()
    b = bamio.BamHandler(files[which])
    for ivs in INTERVALS:
        plan = bamio.plan_blocks(b, ivs, SAFE, 2)
        assert plan.n_blocks > 0
        assert np.all(np.diff(plan.coffset) > 0)                          # deduplicated, in file order
        assert plan.out_off[0] == 0 and np.array_equal(np.diff(plan.out_off), plan.isize[:-1])
        assert plan.out_bytes == int(plan.isize.sum())
        for i in range(plan.n_blocks):
            co = int(plan.coffset[i])
            assert raw[co:co + 4] == b"\x1f\x8b\x08\x04"
            xlen = struct.unpack_from("<H", raw, co + 10)[0]
            bsize = struct.unpack_from("<H", raw, co + 16)[0] + 1
            clen = bsize - 12 - xlen - 8
            crc, isize = struct.unpack_from("<II", raw, co + bsize - 8)
            assert (plan.next_coffset[i], plan.clen[i], plan.isize[i], plan.crc[i]) == (co + bsize, clen, isize, crc)
            a = int(plan.in_off[i])
            assert plan.payload[a:a + clen].tobytes() == raw[co + 12 + xlen:co + 12 + xlen + clen]


def _assert_same(fa_, fb_):
    assert fa_.interval_index.tolist() == fb_.interval_index.tolist()
    assert fa_.reads_seen.tolist() == fb_.reads_seen.tolist()
    for fld in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(fa_.batch, fld), getattr(fb_.batch, fld), err_msg=fld)
    ha, hb = fa_.batch.read_hp, fb_.batch.read_hp
    assert (ha is None) == (hb is None) and (ha is None or np.array_equal(ha, hb))


@pytest.mark.parametrize("which", ["py", "native1", "native6", "long"])
def test_fill_batch_blocks_equals_fill_batch(files, which):
    b, f = bamio.BamHandler(files[which]), bamio.FastaHandler(files["fa"])
    for ivs in INTERVALS:
        plan = bamio.plan_blocks(b, ivs, SAFE, 2)
        data = _inflate(plan)
        for supp, mapq, rate in ((False, 5, 1.0), (True, 0, 1.0), (False, 20, 0.4)):
            ref = bamio.fill_batch(b, f, ivs, mapq, supp, rate, SAFE)
            got = bamio.fill_batch_blocks(b, f, ivs, plan.coffset, plan.next_coffset, plan.isize, plan.out_off, data, mapq, supp,
                                          rate, SAFE)
            _assert_same(ref, got)
            # reads longer than the planner's 32 kb look-ahead may need a block past the plan, inflated on the host
            assert got.blocks_host == 0 or which == "long"
            assert ref.batch.n_reads > 0 or which == "long"
            ref.close()
            got.close()


def test_missing_blocks_fall_back_to_the_host(files):
    """a zero-block margin, and a table with blocks taken out: the missing blocks are read and inflated on the host,
    counted in blocks_host, and the arrays stay those of fill_batch"""
    b, f = bamio.BamHandler(files["native1"]), bamio.FastaHandler(files["fa"])
    ivs = INTERVALS[1]
    ref = bamio.fill_batch(b, f, ivs, 5, False, 1.0, SAFE)
    plan0 = bamio.plan_blocks(b, ivs, SAFE, 0)
    plan2 = bamio.plan_blocks(b, ivs, SAFE, 2)
    assert plan0.n_blocks < plan2.n_blocks and set(plan0.coffset.tolist()) <= set(plan2.coffset.tolist())
    got = bamio.fill_batch_blocks(b, f, ivs, plan0.coffset, plan0.next_coffset, plan0.isize, plan0.out_off, _inflate(plan0))
    _assert_same(ref, got)
    # 0 here: the reader parses only records that start before a chunk's end (BAI chunk ends are record ends) or the first record
    # past the region, and with reads this short those lie inside the planned blocks; the long-read case below needs the fallback
    assert got.blocks_host == 0
    data = _inflate(plan2)
    keep = np.arange(plan2.n_blocks) % 3 != 1                          # every third block missing
    got = bamio.fill_batch_blocks(b, f, ivs, plan2.coffset[keep], plan2.next_coffset[keep], plan2.isize[keep],
                                  plan2.out_off[keep], data)
    _assert_same(ref, got)
    assert got.blocks_host > 0
    empty = bamio.fill_batch_blocks(b, f, ivs, plan2.coffset[:0], plan2.next_coffset[:0], plan2.isize[:0], plan2.out_off[:0],
                                    data)
    _assert_same(ref, empty)
    assert empty.blocks_host >= plan0.n_blocks - 1


@pytest.mark.parametrize("which", ["native1", "py", "long"])
def test_zero_margin_plan_counts_every_host_inflate(files, which):
    """a zero-block margin: blocks_host counts exactly the block loads the table could not serve. Removing one table block at
    a time counts the loads it served; their sum + blocks_host(plan) == blocks_host(empty table). Reads
    longer than the planner's 32 kb look-ahead (`long`) make the fallback run."""
    b, f = bamio.BamHandler(files[which]), bamio.FastaHandler(files["fa"])
    for ivs in INTERVALS:
        ref = bamio.fill_batch(b, f, ivs, 5, False, 1.0, SAFE)
        p = bamio.plan_blocks(b, ivs, SAFE, 0)
        data = _inflate(p)
        got = bamio.fill_batch_blocks(b, f, ivs, p.coffset, p.next_coffset, p.isize, p.out_off, data)
        _assert_same(ref, got)
        none = bamio.fill_batch_blocks(b, f, ivs, p.coffset[:0], p.next_coffset[:0], p.isize[:0], p.out_off[:0], data)
        _assert_same(ref, none)
        used = 0
        for i in range(p.n_blocks):
            k = np.arange(p.n_blocks) != i
            g = bamio.fill_batch_blocks(b, f, ivs, p.coffset[k], p.next_coffset[k], p.isize[k], p.out_off[k], data)
            assert g.blocks_host >= got.blocks_host   # (a block that several intervals read is loaded once per interval)
            used += g.blocks_host - got.blocks_host
        assert used + got.blocks_host == none.blocks_host > 0
        if which != "long":
            assert got.blocks_host == 0
    if which == "long":
        p = bamio.plan_blocks(b, INTERVALS[0], SAFE, 0)
        got = bamio.fill_batch_blocks(b, f, INTERVALS[0], p.coffset, p.next_coffset, p.isize, p.out_off, _inflate(p))
        assert got.blocks_host > 0
        _assert_same(bamio.fill_batch(b, f, INTERVALS[0], 5, False, 1.0, SAFE), got)


def test_helper_threads_and_block_tables_are_exclusive(files):
    b = bamio.BamHandler(files["py"])
    b.set_threads(2)
    with pytest.raises(IOError) as ei:
        bamio.plan_blocks(b, INTERVALS[0], SAFE, 2)
    assert "helper threads" in str(ei.value)
    b.set_threads(0)
    assert bamio.plan_blocks(b, INTERVALS[0], SAFE, 2).n_blocks > 0


def _block_offsets(raw):
    offs, p = [], 0
    while p < len(raw):
        offs.append(p)
        p += struct.unpack_from("<H", raw, p + 16)[0] + 1
    return offs


def test_truncated_file_and_corrupt_header_are_clean_errors(files, tmp_path):
    raw = open(files["py"], "rb").read()
    bai = open(files["py"] + ".bai", "rb").read()
    offs = _block_offsets(raw)
    ivs = [("c1", 0, 59_999)]
    b = bamio.BamHandler(files["py"])
    plan = bamio.plan_blocks(b, ivs, SAFE, 2)
    assert plan.n_blocks >= len(offs) - 2
    victim = offs[len(offs) // 2]
    cases = {
        "trunc": (raw[:victim + 30], "truncated"),                                                     # cut inside a payload
        "magic": (raw[:victim] + b"\x00" + raw[victim + 1:], "not a BGZF block"),
        "isize": (raw[:offs[len(offs) // 2 + 1] - 4] + struct.pack("<I", 70_000) + raw[offs[len(offs) // 2 + 1]:], "ISIZE"),
    }
    for name, (bad, msg) in cases.items():
        p = str(tmp_path / ("%s.bam" % name))
        open(p, "wb").write(bad)
        open(p + ".bai", "wb").write(bai)
        h = bamio.BamHandler(p)
        with pytest.raises(IOError) as ei:
            bamio.plan_blocks(h, ivs, SAFE, 2)
        assert msg in str(ei.value), (name, str(ei.value))
        with pytest.raises(IOError):                                                             # the host path agrees
            bamio.fill_batch(h, bamio.FastaHandler(files["fa"]), ivs)
