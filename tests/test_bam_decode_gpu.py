"""GPU: BAM record decode and region clipping on the device (pv_bam_scan_dev / pv_bam_fill_dev, the `gpu_decode` reader mode)
against the host reader bamio.fill_batch on the same files: every pv_batch_in field, read_hp, interval_index, reads_seen, the
totals and max_region_len, byte for byte."""
import copy
import gzip
import struct

import numpy as np
import pytest

import bam_writer as bw
from pepper_thesis_amd import bamio, build
from pepper_thesis_amd.batch import RegionBatch

pytestmark = pytest.mark.gpu


def same_as_host(hip_ctx, bam, fa, ivs, mq=5, supp=False, rate=1.0, T=None, expect_host=0):
    """decode `ivs` as ONE reader group on the device and compare with fill_batch; -> the number of reads compared"""
    from pepper_thesis_amd.gpu_decode import decode_groups
    T = {} if T is None else T
    items = decode_groups(hip_ctx, bam, fa, [ivs], mq, supp, rate, 100, T)
    fb = bamio.fill_batch(bamio.BamHandler(bam), bamio.FastaHandler(fa), ivs, mq, supp, rate, 100)
    assert T["gpu_decode_groups_host"] == expect_host, T
    if fb.batch.n_regions == 0:
        assert items == [], items   # no region: the device path hands over nothing
        return 0
    assert len(items) == 1 and items[0][0] == ("host" if expect_host else "dev"), items
    if expect_host:
        hb, hp, ii, seen = items[0][1].batch, items[0][1].batch.read_hp, items[0][1].interval_index, items[0][1].reads_seen
        hp = np.zeros(hb.n_reads, np.int32) if hp is None else hp
    else:
        db = items[0][1]
        hb, hp = db.to_host()
        ii, seen = db.interval_index, db.reads_seen
        assert (db.n_reads, db.n_bases, db.n_cigar, db.n_ref_bytes, db.max_region_len, db.n_regions) == \
               (fb.batch.n_reads, fb.batch.n_bases, fb.batch.n_cigar, int(fb.batch.ref.shape[0]), fb.batch.max_region_len, fb.batch.n_regions)
    for f in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(hb, f), getattr(fb.batch, f), err_msg=f)
    np.testing.assert_array_equal(hp, np.zeros(fb.batch.n_reads, np.int32) if fb.batch.read_hp is None else fb.batch.read_hp)
    np.testing.assert_array_equal(ii, fb.interval_index)
    np.testing.assert_array_equal(seen, fb.reads_seen)
    return fb.batch.n_reads


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the test_bamio module fixture, rebuilt"""
    build.build_io()
    d = tmp_path_factory.mktemp("dec")
    rng = np.random.default_rng(5)
    seqs = [("chr20", "".join(rng.choice(list("ACGTacgtN"), size=130_000, p=[.22, .22, .22, .22, .02, .02, .02, .02, .04]))),
            ("chrM", "".join(rng.choice(list("ACGT"), size=16_500)))]
    bw.write_fasta(str(d / "ref.fa"), seqs, width=70)
    recs = bw.random_records(rng, 900, 130_000, tid=0) + bw.random_records(rng, 60, 16_500, tid=1, mean_len=800)
    bw.write_bam(str(d / "reads.bam"), [(n, len(s)) for n, s in seqs], recs)
    return dict(bam=str(d / "reads.bam"), fa=str(d / "ref.fa"))


@pytest.mark.parametrize("region", [("chr20", 0, 1000), ("chr20", 16_300, 16_500), ("chr20", 49_900, 60_100),
                                    ("chr20", 100_000, 129_999), ("chr20", 65_535, 65_537), ("chrM", 100, 16_400)])
@pytest.mark.parametrize("supp,min_mapq", [(False, 5), (True, 0)])
def test_bamio_fixture_regions(hip_ctx, files, region, supp, min_mapq):
    assert same_as_host(hip_ctx, files["bam"], files["fa"], [region], min_mapq, supp) > 0


def test_contig_end_start_at_zero_several_intervals_and_empty_ones(hip_ctx, files):
    ivs = [("chr20", 0, 4000), ("chr20", 120_000, 129_999), ("chrM", 16_000, 16_499), ("chr20", 30_000, 42_000), ("chrM", 0, 3000)]
    assert same_as_host(hip_ctx, files["bam"], files["fa"], ivs, 5, False) > 0
    # intervals without reads drop out; a group of nothing else gives no batch at all
    build.build_io()
    assert same_as_host(hip_ctx, files["bam"], files["fa"], [("chr20", 129_990, 129_999), ("chr20", 60_000, 61_000)], 61, False) == 0


# ---- hand-made records ---------------------------------------------------------------------------------------------------

def _rec(pos, cigar, seq=None, **kw):
    qn = sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    seq = seq if seq is not None else ("ACGTTGCA" * (qn // 8 + 1))[:qn]
    r = dict(tid=0, pos=pos, mapq=60, flag=0, cigar=cigar, seq=seq, qual=[(7 * i + 3) % 60 for i in range(len(seq))], name="h%d" % pos,
             aux=b"")
    r.update(kw)
    return r


def _fasta(tmp_path, n=6000, name="c1"):
    rng = np.random.default_rng(1)
    fa = str(tmp_path / "ref.fa")
    bw.write_fasta(fa, [(name, "".join(rng.choice(list("ACGT"), size=n)))])
    return fa


def test_hand_made_records(hip_ctx, tmp_path):
    """window [900, 2100] (interval 1000-2000): clip edges, op kinds, SEQ parities, IUPAC codes, HP tag forms, flags, mapq"""
    build.build_io()
    hp = lambda ty, fmt, v: b"HP" + ty + struct.pack(fmt, v)   # noqa: E731
    recs = [
        _rec(100, [(0, 3000)]),                                                # starts before the window and ends after it
        _rec(850, [(0, 50), (1, 6), (0, 40)]),                                 # first in-window operation: I
        _rec(860, [(0, 40), (4, 5), (0, 40)]),                                 # ... S
        _rec(870, [(0, 30), (2, 12), (0, 40)]),                                # ... D
        _rec(880, [(0, 20), (3, 15), (0, 40)]),                                # ... N
        _rec(890, [(4, 9), (0, 11), (1, 3), (0, 50)]),                         # an odd first kept SEQ index
        _rec(891, [(0, 10), (1, 2), (0, 50)]),                                 # an even one behind an insert
        _rec(1000, [(5, 4), (7, 30), (8, 2), (6, 3), (0, 30), (5, 2)]),        # = X H P
        _rec(1100, [(0, 15)], seq="=ACMGRSVTWYHKDBN"[:15]),                    # every IUPAC code, odd l_seq
        _rec(1101, [(0, 16)], seq="=ACMGRSVTWYHKDBN"),
        _rec(1200, [], seq=""),                                                # l_seq 0, no CIGAR
        _rec(1300, [(0, 40)], aux=hp(b"c", "<b", -1)), _rec(1301, [(0, 40)], aux=hp(b"C", "<B", 2)),
        _rec(1302, [(0, 40)], aux=hp(b"s", "<h", -1)), _rec(1303, [(0, 40)], aux=hp(b"S", "<H", 3)),
        _rec(1304, [(0, 40)], aux=hp(b"i", "<i", 1)), _rec(1305, [(0, 40)], aux=hp(b"I", "<I", 2)),
        _rec(1306, [(0, 40)], aux=hp(b"C", "<B", 0)),
        _rec(1310, [(0, 40)], aux=b"RGZ" + b"g" * 150 + b"\x00" + b"MLBC" + struct.pack("<I", 70) + bytes(70) + hp(b"C", "<B", 1)),
        _rec(1311, [(0, 40)], aux=hp(b"C", "<B", 1) + b"NMi" + struct.pack("<i", 3) + hp(b"s", "<h", 2)),   # two HP fields: the last wins
        _rec(1312, [(0, 40)], aux=b"HPZab\x00" + b"XXq"),                      # HP of a non-integer type; then a field that does not fit
        _rec(1400, [(0, 40)], flag=4), _rec(1401, [(0, 40)], flag=0x100), _rec(1402, [(0, 40)], flag=0x200),
        _rec(1403, [(0, 40)], flag=0x400), _rec(1404, [(0, 40)], flag=0x800), _rec(1405, [(0, 40)], flag=0x810), _rec(1406, [(0, 40)], flag=16),
        _rec(1500, [(0, 40)], mapq=4), _rec(1501, [(0, 40)], mapq=5), _rec(1502, [(0, 40)], mapq=0),
        _rec(2050, [(0, 30), (2, 100), (0, 30)]),                              # a deletion across `re`
        _rec(2080, [(0, 10), (1, 4), (0, 30)]),                                # M cut at `re`, the walk ends there
        _rec(2100, [(0, 10)]), _rec(2101, [(0, 10)]),                          # the last position of the window, and the first outside
    ]
    fa = _fasta(tmp_path)
    for blk, nm in ((0xFF00, "a"), (97, "tiny")):   # tiny blocks: every record straddles several block boundaries
        bam = str(tmp_path / (nm + ".bam"))
        bw.write_bam(bam, [("c1", 6000)], recs, block_bytes=blk)
        for supp, mq in ((False, 5), (True, 0)):
            assert same_as_host(hip_ctx, bam, fa, [("c1", 1000, 2000)], mq, supp) >= 20
        assert same_as_host(hip_ctx, bam, fa, [("c1", 0, 500), ("c1", 1290, 1295), ("c1", 2100, 2300)], 0, True) > 3


def test_cg_tag_long_cigar(hip_ctx, tmp_path):
    """more than 65 535 operations: the real CIGAR is in CG:B,I behind the <l_seq>S<rlen>N placeholder"""
    build.build_io()
    cig = [(0, 1), (1, 1)] * 33_000 + [(0, 5)]
    long_rec = _rec(500, cig, cg=True)
    recs = bw.random_records(np.random.default_rng(2), 30, 4000, tid=0, mean_len=600, allow_skip=False)
    for r in recs[::2]:
        r["cg"] = True
    recs = sorted(recs + [long_rec], key=lambda r: r["pos"])
    fa, bam = _fasta(tmp_path, 40_000), str(tmp_path / "cg.bam")
    bw.write_bam(bam, [("c1", 40_000)], recs)
    assert same_as_host(hip_ctx, bam, fa, [("c1", 600, 3500)], 0, True) > 10
    assert same_as_host(hip_ctx, bam, fa, [("c1", 10_000, 20_000), ("c1", 33_000, 34_000)], 0, True) > 0


# ---- block geometry, packing, down-sampling -------------------------------------------------------------------------------

def _native_bam(path, recs, length):
    from pepper_thesis_amd.batch import Read, Region, pack_regions
    reads = [Read.make(r["pos"], np.asarray([(l << 4) | op for op, l in r["cigar"]], np.uint32), r["seq"].replace("N", "A"), r["qual"],
                       bool(r["flag"] & 0x10), r["mapq"]) for r in recs]
    b = pack_regions([Region(0, length - 1, b"A" * length, reads)])
    bamio.write_bam(path, [("c1", length)], np.zeros(len(reads), np.int32), b, level=1)


def test_block_geometry_and_several_groups_in_one_launch(hip_ctx, tmp_path):
    from pepper_thesis_amd.gpu_decode import decode_groups
    build.build_io()
    rng = np.random.default_rng(8)
    recs = bw.random_records(rng, 400, 50_000, tid=0, mean_len=3000, allow_skip=False)
    fa = _fasta(tmp_path, 50_000)
    full = str(tmp_path / "full.bam")          # full 64 KiB blocks: records straddle their boundaries
    _native_bam(full, recs, 50_000)
    assert same_as_host(hip_ctx, full, fa, [("c1", 10_000, 40_000)], 5, False) > 50
    one = str(tmp_path / "one.bam")            # one record per block: every chunk ends exactly on a block end
    bw.write_bam(one, [("c1", 50_000)], recs, block_records=1)
    assert same_as_host(hip_ctx, one, fa, [("c1", 20_000, 30_000), ("c1", 0, 3000)], 0, True) > 50
    # a plan with a gap between two chunks (two far-apart intervals in one group), and several groups in one launch
    assert same_as_host(hip_ctx, full, fa, [("c1", 1000, 2000), ("c1", 45_000, 46_000)], 5, False) > 10
    groups = [[("c1", 0, 9000)], [("c1", 9000, 18_000), ("c1", 18_000, 27_000)], [("c1", 40_000, 49_999)]]
    T = {}
    items = decode_groups(hip_ctx, full, fa, groups, 5, False, 1.0, 100, T)
    assert [k for k, _ in items] == ["dev"] and T["gpu_decode_groups"] == 3 and T["gpu_decode_groups_host"] == 0
    hb, hp = items[0][1].to_host()
    h = (bamio.BamHandler(full), bamio.FastaHandler(fa))
    from pepper_thesis_amd.batch import merge_batches
    fbs = [bamio.fill_batch(h[0], h[1], g, 5, False, 1.0, 100) for g in groups]
    ref = merge_batches([f.batch for f in fbs])
    for f in RegionBatch.FIELDS:
        np.testing.assert_array_equal(getattr(hb, f), getattr(ref, f), err_msg=f)
    assert items[0][1].interval_index.tolist() == [0, 1, 2, 3]


def test_downsampling_takes_the_reservoir_order(hip_ctx, files, monkeypatch):
    assert same_as_host(hip_ctx, files["bam"], files["fa"], [("chr20", 20_000, 40_000), ("chrM", 0, 16_000)], 0, True, rate=0.4) > 20
    monkeypatch.setattr(bamio, "MAX_READS_IN_REGION", 37)   # read at call time by fill_batch and by the device path
    n = same_as_host(hip_ctx, files["bam"], files["fa"], [("chr20", 20_000, 40_000), ("chr20", 129_000, 129_999), ("chrM", 0, 16_000)], 0, True)
    assert 37 < n <= 3 * 37


# ---- seeded fuzz, long reads -----------------------------------------------------------------------------------------------

def test_seeded_fuzz(hip_ctx, tmp_path):
    """6 files x 4 windows x 2 filter settings = 48 comparisons, reads all shorter than 32 kb: no group may take the host route"""
    build.build_io()
    n_cmp = 0
    for seed in range(6):
        rng = np.random.default_rng(1000 + seed)
        L = 30_000
        recs = bw.random_records(rng, 250, L, tid=0, mean_len=int(rng.integers(300, 3000)), allow_skip=bool(seed % 2))
        fa, bam = _fasta(tmp_path, L), str(tmp_path / ("f%d.bam" % seed))
        bw.write_bam(bam, [("c1", L)], recs, block_records=int(rng.integers(1, 60)))
        for _ in range(4):
            a = int(rng.integers(0, L - 2000))
            b_ = a + int(rng.integers(1, 9000))
            for supp, mq in ((False, 5), (True, 0)):
                same_as_host(hip_ctx, bam, fa, [("c1", a, min(b_, L - 1))], mq, supp, expect_host=0)
                n_cmp += 1
    assert n_cmp == 48


def test_long_reads_take_the_host_route_and_are_counted(hip_ctx, tmp_path):
    """the `long` file of test_bgzf_plan_cpu (40 reads, mean length 45 000): reads run past the plan's 32 kb look-ahead"""
    build.build_io()
    rng = np.random.default_rng(8)
    L = 300_000
    recs = bw.random_records(rng, 40, L, tid=0, mean_len=45_000, allow_skip=False)
    for r in recs:
        r["flag"], r["mapq"], r["hp"] = r["flag"] & 0x10, 60, None
    fa, bam = _fasta(tmp_path, L), str(tmp_path / "long.bam")
    _native_bam(bam, recs, L)
    T, n_host = {}, 0
    for ivs in ([("c1", 0, 5000)], [("c1", 20_000, 30_000), ("c1", 25_000, 35_000)], [("c1", 100_000, 140_000)], [("c1", 200_000, 299_999)]):
        from pepper_thesis_amd.gpu_decode import decode_groups
        Tk = {}
        items = decode_groups(hip_ctx, bam, fa, [ivs], 5, False, 1.0, 100, Tk)
        n_host += Tk["gpu_decode_groups_host"]
        same_as_host(hip_ctx, bam, fa, ivs, 5, False, expect_host=Tk["gpu_decode_groups_host"])
        assert len(items) <= 1
    assert n_host > 0


# ---- corrupt inputs: a status, an IOError, and the process goes on ------------------------------------------------------------

def _first_record_offset(body):
    l_text = struct.unpack_from("<I", body, 4)[0]
    off = 8 + l_text
    n_ref = struct.unpack_from("<I", body, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 4 + struct.unpack_from("<I", body, off)[0] + 4
    return off


def _plain(raw):
    import zlib
    out, p = bytearray(), 0
    while p < len(raw):
        bsize = int.from_bytes(raw[p + 16:p + 18], "little") + 1
        out += zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        p += bsize
    return out


def test_corrupt_records_and_blocks_raise_and_a_good_file_decodes_afterwards(hip_ctx, tmp_path, files):
    from pepper_thesis_amd.gpu_decode import decode_groups
    build.build_io()
    rng = np.random.default_rng(4)
    recs = bw.random_records(rng, 5, 4000, tid=0, mean_len=500, allow_skip=False)
    for r in recs:
        r["flag"], r["mapq"] = 0, 60
    fa, good = _fasta(tmp_path, 4000), str(tmp_path / "good.bam")
    bw.write_bam(good, [("c1", 4000)], recs)
    body = _plain(open(good, "rb").read())
    off = _first_record_offset(body)
    bs0 = struct.unpack_from("<I", body, off)[0]

    def variant(name, edit, cut=None):
        b = bytearray(body)
        edit(b)
        p = str(tmp_path / (name + ".bam"))
        tail = bytes(b[off:cut]) if cut else bytes(b[off:])
        open(p, "wb").write(bw._bgzf_block(bytes(b[:off])) + bw._bgzf_block(tail) + bw.BGZF_EOF)
        open(p + ".bai", "wb").write(open(good + ".bai", "rb").read())
        return p

    def cigar_longer(b):   # the first M operation of the first record grows past l_seq
        l_name = b[off + 4 + 8]
        at = off + 4 + 32 + l_name
        struct.pack_into("<I", b, at, ((len(recs[0]["seq"]) + 3000) << 4) | (struct.unpack_from("<I", b, at)[0] & 0xF))
        struct.pack_into("<H", b, off + 4 + 12, 1)

    cases = [
        ("bs_small", lambda b: struct.pack_into("<I", b, off, 20), None, "block_size 20"),
        ("fields", lambda b: struct.pack_into("<I", b, off + 4 + 16, 0x00FFFFFF), None, "corrupt BAM record (fields need"),
        ("neg_lseq", lambda b: struct.pack_into("<i", b, off + 4 + 16, -5), None, "negative l_seq"),
        ("cigar", cigar_longer, None, "CIGAR longer than SEQ"),
        ("trunc", lambda b: None, len(body) - 40, "truncated BAM record"),
    ]
    for name, edit, cut, text in cases:
        p = variant(name, edit, cut)
        with pytest.raises(IOError) as eh:
            bamio.fill_batch(bamio.BamHandler(p), bamio.FastaHandler(fa), [("c1", 0, 3999)], 0, True, 1.0, 100)
        assert text in str(eh.value), (name, str(eh.value))
        T = {}
        items = decode_groups(hip_ctx, p, fa, [[("c1", 0, 3999)]], 0, True, 1.0, 100, T)
        assert [k for k, _ in items] == ["error"], (name, items)
        assert isinstance(items[0][1], IOError) and text in str(items[0][1]), (name, str(items[0][1]))
        assert T["gpu_decode_groups_host"] == (1 if name == "trunc" else 0)
    # a block with a bad CRC under a walked record
    raw = bytearray(open(files["bam"], "rb").read())
    offs, p = [], 0
    while p < len(raw):
        offs.append(p)
        p += int.from_bytes(raw[p + 16:p + 18], "little") + 1
    victim = offs[len(offs) // 3]
    raw[victim + 18 + 60] ^= 0x5A
    bad = str(tmp_path / "crc.bam")
    open(bad, "wb").write(bytes(raw))
    open(bad + ".bai", "wb").write(open(files["bam"] + ".bai", "rb").read())
    items = decode_groups(hip_ctx, bad, files["fa"], [[("chr20", 0, 129_999)]], 0, True, 1.0, 100, {})
    assert [k for k, _ in items] == ["error"] and "offset %d" % victim in str(items[0][1])
    # the same process and context decode good files afterwards
    assert same_as_host(hip_ctx, good, fa, [("c1", 0, 3999)], 0, True) == 5
    assert same_as_host(hip_ctx, files["bam"], files["fa"], [("chr20", 0, 129_999)], 0, True) > 500


# ---- into the builders, end to end -------------------------------------------------------------------------------------------

def _reads_bam(tmp_path, seed=17, length=40_000, n_reads=500):
    build.build_io()
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), size=length))
    bw.write_fasta(str(tmp_path / "ref.fa"), [("chr20", ref)])
    recs = bw.random_records(rng, n_reads, length, tid=0, mean_len=2500, allow_skip=False)
    for r in recs:
        seq, qi, rp = list(r["seq"]), 0, r["pos"]
        for op, ln in r["cigar"]:
            if op in (0, 7, 8):
                for i in range(ln):
                    if rp + i < len(ref) and rng.random() > 0.04:
                        seq[qi + i] = ref[rp + i]
                qi += ln; rp += ln
            elif op in (1, 4):
                qi += ln
            elif op in (2, 3):
                rp += ln
        r["seq"], r["mapq"] = "".join(seq), 60
        r["flag"] &= 0x10
    bw.write_bam(str(tmp_path / "reads.bam"), [("chr20", len(ref))], recs)
    return str(tmp_path / "reads.bam"), str(tmp_path / "ref.fa")


def test_decoded_batch_into_the_three_builders(hip_ctx, tmp_path):
    import torch
    from pepper_thesis_amd.batch import PRESETS, hp_params
    from pepper_thesis_amd.device import DeviceBatch, DeviceOut, DevicePolishOut
    from pepper_thesis_amd.gpu_decode import decode_groups, summarize_decoded
    bam, fa = _reads_bam(tmp_path)
    ivs = [("chr20", 2000, 14_000), ("chr20", 14_000, 26_000)]
    (kind, db), = decode_groups(hip_ctx, bam, fa, [ivs], 5, False, 1.0, 100, {})
    assert kind == "dev"
    fb = bamio.fill_batch(bamio.BamHandler(bam), bamio.FastaHandler(fa), ivs, 5, False, 1.0, 100)
    assert fb.batch.read_hp is not None
    P = PRESETS["ont_r9_guppy5_sup"]
    dev = "cuda:%d" % hip_ctx.device_id
    host_dev = DeviceBatch(fb.batch, dev)   # the host-read batch, uploaded: both go through the same *_dev call
    db.wait_on(hip_ctx)
    CAP = 65536
    for hp in (False, True):
        p = hp_params(P) if hp else P
        outs = []
        for b in (db, host_dev):
            images = torch.zeros((CAP, 21, 48), dtype=torch.int8, device=dev) if hp else None
            do = DeviceOut(CAP, 16 * CAP, dev, images)
            torch.cuda.synchronize()
            (hip_ctx.summarize_hp_dev if hp else hip_ctx.summarize_dev)(b, p, do)
            hip_ctx.synchronize()
            n, sb, st = (int(v) for v in do.counts[:3].tolist())
            assert st == 0 and 50 < n <= CAP and sb <= 16 * CAP
            outs.append([t_.cpu().numpy() for t_ in (do.region[:n], do.position[:n], do.depth[:n], do.cand_freq[:n], do.images[:n],
                                                     do.cand_off[:n + 1], do.cand_str[:sb])])
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x, y)
        got = summarize_decoded(hip_ctx, db, p, hp)   # the read-back form make_images uses
        assert len(got) == len(outs[1][0])
        np.testing.assert_array_equal(got.images, outs[1][4])
    outs = []
    for b in (db, DeviceBatch(fb.batch, "cuda:%d" % hip_ctx.device_id)):
        po = DevicePolishOut(64, 1000, 50, "cuda:%d" % hip_ctx.device_id)
        hip_ctx.polish_summarize_dev(b, po)
        hip_ctx.synchronize()
        n = po.n_chunks()
        assert po.status() == 0 and 0 < n <= 64
        outs.append([t[:n].cpu().numpy() for t in (po.images, po.position, po.index, po.region, po.chunk_id)])
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


def _pred_records(path):
    from pepper_thesis_amd import hdf5io
    with hdf5io.PredictionStore(path, "r") as st:
        return [(k, {f: v.tolist() for f, v in bt.items()}) for k, bt in st.batches()]


def test_call_variant_fused_gpu_decode_gives_identical_predictions(hip_ctx, tmp_path):
    from pepper_thesis_amd import pipeline, synth
    from pepper_thesis_amd.batch import PRESETS
    bam, fa = _reads_bam(tmp_path)
    w = synth.make_weights_p1(3, 3.0)
    P = PRESETS["ont_r9_guppy5_sup"]
    T0, T1 = {}, {}
    n0 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "host.hdf"), P, "chr20:1000-39000", 6000,
                                     intervals_per_call=4, timers=T0)
    n1 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "gpu.hdf"), P, "chr20:1000-39000", 6000,
                                     intervals_per_call=4, timers=T1, gpu_decode=True)
    assert n0 == n1 > 100
    assert _pred_records(str(tmp_path / "host.hdf")) == _pred_records(str(tmp_path / "gpu.hdf"))
    assert T1["gpu_decode_groups"] == T1["intervals"] >= 6 and T1["gpu_decode_groups_host"] == 0 and "gpu_decode_groups" not in T0
    assert T1["gpu_decode_scan_ms"] > 0 and T1["gpu_decode_fill_ms"] > 0 and T1["reads"] == T0["reads"] and T1["bases"] == T0["bases"]


def test_make_images_and_call_variant_cli_gpu_decode(tmp_path):
    from pepper_thesis_amd import call_variant, hdf5io, make_images, synth
    bam, fa = _reads_bam(tmp_path, seed=5)
    base = ["-b", bam, "-f", fa, "-r", "chr20:2000-38000", "--region_size", "12000", "--ont_r9_guppy5_sup"]
    for hp, name in (([], "pepper_variants_images_thread_0.hdf5"), (["-hp"], "pepper_variants_images_thread_0_hp.hdf5")):
        tag = "hp" if hp else "p"
        make_images.main(base + hp + ["-o", str(tmp_path / ("img_host_" + tag))])
        make_images.main(base + hp + ["-o", str(tmp_path / ("img_gpu_" + tag)), "--gpu_decode"])
        with hdf5io.ImageStore(str(tmp_path / ("img_host_" + tag) / name), "r") as a, \
                hdf5io.ImageStore(str(tmp_path / ("img_gpu_" + tag) / name), "r") as b:
            assert a.summaries() == b.summaries() and len(a.summaries()) == 3
            for nm in a.summaries():
                x, y = a.read_summary(nm), b.read_summary(nm)
                assert sorted(x) == sorted(y)
                for key in x:
                    assert np.asarray(x[key]).tolist() == np.asarray(y[key]).tolist(), (nm, key)
    w = synth.make_weights_p1(3, 3.0)
    np.savez(str(tmp_path / "model.npz"), **w)
    cv = base + ["-m", str(tmp_path / "model.npz"), "-s", "HG003"]
    c0 = call_variant.main(cv + ["-o", str(tmp_path / "cv_host")])
    c1 = call_variant.main(cv + ["-o", str(tmp_path / "cv_gpu"), "--gpu_decode"])
    assert c0 == c1 and c0["total"] > 0
    for fn in ("PEPPER_VARIANT_FULL.vcf.gz", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING.vcf.gz"):
        body = [[ln for ln in gzip.open(str(d / fn), "rt").read().splitlines() if not ln.startswith("#")]
                for d in (tmp_path / "cv_host", tmp_path / "cv_gpu")]
        assert body[0] == body[1], fn
