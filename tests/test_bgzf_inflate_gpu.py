"""GPU: the batched BGZF/DEFLATE inflate kernel (pv_bgzf_inflate[_dev]) against Python's zlib, its per-block statuses on
crafted streams, and the opt-in `gpu_inflate` reader mode end to end against the default host inflate."""
import gzip
import os
import zlib

import numpy as np
import pytest

from deflate_writer import DBASE, DEXT, LBASE, LEXT, Bits  # noqa: F401
from pepper_thesis_amd import _ffi

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def flushed(data: bytes) -> bytes:
    """mid-stream sync and full flushes: empty stored blocks inside the BFINAL chain"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    k = len(data) // 3
    return (co.compress(data[:k]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[k:2 * k]) + co.flush(zlib.Z_FULL_FLUSH) +
            co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[2 * k:]) + co.flush())


def far_matches(rng):
    """matches reaching 32767 and 32768 bytes back, which zlib's compressor never emits (its limit is 32768 - 262): a stored
    block of random bytes, then fixed-Huffman pairs; the expected bytes come from copying byte by byte here"""
    out = []
    for nm, n_prefix, pairs in (
            ("far_32768", 32768, [(3, 32768), (64, 32768), (65, 32768), (258, 32768)]),
            ("far_32767", 32768, [(3, 32767), (64, 32767), (65, 32767), (258, 32767), (258, 32768)]),
            ("far_wrap", 40000, [(258, 32768), (65, 32767), (3, 32768), (258, 32500), (64, 32768), (7, 1), (258, 32768),
                                 (130, 32767), (258, 2), (200, 32768)])):
        raw = bytearray(rng.integers(0, 256, n_prefix, dtype=np.uint8).tobytes())
        b = Bits().stored(bytes(raw)).put(1, 1).put(1, 2)
        for k, (ln, d) in enumerate(pairs):
            for _ in range(ln):
                raw.append(raw[-d])
            b.match_fixed(ln, d)
            if k % 3 == 2:                    # a literal between some of the pairs
                raw.append(0x41 + k)
                b.lit_fixed(0x41 + k)
        b.lit_fixed(256)
        out.append((nm, bytes(raw), b.bytes()))
    return out


def _bam_like_bytes():
    import bam_writer as bw
    rng = np.random.default_rng(4)
    recs = bw.random_records(rng, 120, 30_000, tid=0, mean_len=1500, allow_skip=False)
    import tempfile
    from pepper_thesis_amd import bamio, build
    build.build_io()
    with tempfile.TemporaryDirectory() as d:
        bw.write_bam(os.path.join(d, "r.bam"), [("c1", 30_000)], recs)
        return bamio.bgzf_read_all(os.path.join(d, "r.bam"))


def corpus():
    """(name, raw, payload): every kind of stream the decoder must handle"""
    rng = np.random.default_rng(7)
    text = b"".join(b"read_%d\tchr20\t%d\t60\t%dM\tACGTTGCA%s\n" % (i, 1000 + 37 * i, 100 + i % 50, b"ACGT"[i % 4:i % 4 + 1] * (i % 23))
                    for i in range(2000))[:65536]
    bam = _bam_like_bytes()
    rnd = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    half = rng.integers(0, 4, 32768, dtype=np.uint8).tobytes()
    out = []
    for lv in range(10):
        out.append(("level%d" % lv, text, deflate(text, lv)))
        out.append(("bam_level%d" % lv, bam[:65536], deflate(bam[:65536], lv)))
    for nm, stg in (("filtered", zlib.Z_FILTERED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE),
                    ("fixed", zlib.Z_FIXED)):
        out.append((nm, text, deflate(text, 6, stg)))
        out.append(("bam_" + nm, bam[5000:60000], deflate(bam[5000:60000], 6, stg)))
    out.append(("flushes", text, flushed(text)))
    out.append(("bam_flushes", bam[:40000], flushed(bam[:40000])))
    for sz in (0, 1, 65536):
        out.append(("size%d" % sz, text[:sz], deflate(text[:sz])))
        out.append(("size%d_l0" % sz, rnd[:sz], deflate(rnd[:sz], 0)))
    out.append(("random", rnd, deflate(rnd, 9)))
    out.append(("dist1_run", b"a" * 65536, deflate(b"a" * 65536, 9)))
    out.append(("dist1_rle", b"\x00" * 30000 + b"xy" * 100, deflate(b"\x00" * 30000 + b"xy" * 100, 6, zlib.Z_RLE)))
    out.append(("dist32768", half + half, deflate(half + half, 9)))
    out.append(("short_period", b"abc" * 20000, deflate(b"abc" * 20000, 1)))
    out.append(("eof_block", b"", bytes.fromhex("0300")))
    for i in range(8):
        a = int(rng.integers(0, len(bam) - 20000))
        chunk = bam[a:a + int(rng.integers(1, 20000))]
        out.append(("bam_slice%d" % i, chunk, deflate(chunk, int(rng.integers(1, 10)))))
    out += far_matches(rng)
    for nm, raw, pay in out:
        assert zlib.decompress(pay, -15) == raw, nm
    return out


def crafted():
    """(name, payload, isize, crc, expected status): one stream per failure status"""
    good = b"GATTACA" * 20
    gp = deflate(good)
    crc = zlib.crc32(good) & 0xFFFFFFFF
    stored = deflate(good, 0)
    cases = [
        ("btype3", Bits().put(1, 1).put(3, 2).bytes(), 10, 0, _ffi.PV_BGZF_BAD_BTYPE),
        ("stored_nlen", bytes([1, 5, 0, 0, 0]) + b"hello", 5, zlib.crc32(b"hello"), _ffi.PV_BGZF_STORED_LEN),
        ("cl_oversubscribed", Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4).put(0x1249249249249249, 57).bytes(),
         10, 0, _ffi.PV_BGZF_BAD_CODE_LENGTHS),
        ("cl_incomplete", Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(2, 3).put(0, 9).put(0, 16).bytes(),
         10, 0, _ffi.PV_BGZF_BAD_CODE_LENGTHS),
        ("litlen_286", Bits().put(1, 1).put(1, 2).lit_fixed(286).bytes(), 10, 0, _ffi.PV_BGZF_BAD_SYMBOL),
        ("litlen_287", Bits().put(1, 1).put(1, 2).lit_fixed(97).lit_fixed(287).bytes(), 10, 0, _ffi.PV_BGZF_BAD_SYMBOL),
        ("dist_30", Bits().put(1, 1).put(1, 2).lit_fixed(97).lit_fixed(257).code(30, 5).bytes(), 10, 0, _ffi.PV_BGZF_BAD_SYMBOL),
        ("dist_31", Bits().put(1, 1).put(1, 2).lit_fixed(97).lit_fixed(257).code(31, 5).bytes(), 10, 0, _ffi.PV_BGZF_BAD_SYMBOL),
        ("dist_too_far", Bits().put(1, 1).put(1, 2).lit_fixed(97).lit_fixed(257).code(1, 5).lit_fixed(256).bytes(), 4, 0,
         _ffi.PV_BGZF_DIST_TOO_FAR),
        ("overflow", gp, len(good) - 7, crc, _ffi.PV_BGZF_OUTPUT_OVERFLOW),
        ("short", gp, len(good) + 7, crc, _ffi.PV_BGZF_OUTPUT_SHORT),
        ("overrun_stored", stored[:len(stored) // 2], len(good), crc, _ffi.PV_BGZF_INPUT_OVERRUN),
        ("overrun_fixed", Bits().put(1, 1).put(1, 2).lit_fixed(97).bytes()[:1], 1, 0, _ffi.PV_BGZF_INPUT_OVERRUN),
        ("crc", gp, len(good), crc ^ 1, _ffi.PV_BGZF_CRC_MISMATCH),
        ("isize_too_big", gp, 70_000, crc, _ffi.PV_BGZF_BAD_ARGS),
    ]
    for nm, pay, isize, c, st in cases:   # zlib (or the trailer check) rejects every one of them too
        if st in (_ffi.PV_BGZF_OUTPUT_OVERFLOW, _ffi.PV_BGZF_OUTPUT_SHORT, _ffi.PV_BGZF_CRC_MISMATCH, _ffi.PV_BGZF_BAD_ARGS):
            continue
        d = zlib.decompressobj(-15)
        try:
            raw = d.decompress(pay)
            ok = d.eof and len(raw) == isize
        except zlib.error:
            ok = False
        assert not ok, nm
    return cases


def layout(sizes, rng, gap=16):
    """output offsets in shuffled order with guard gaps between the ranges -> (out_off, total bytes)"""
    order = rng.permutation(len(sizes))
    out_off = np.zeros(len(sizes), np.int64)
    o = gap
    for i in order:
        out_off[i] = o
        o += int(sizes[i]) + gap
    return out_off, o


def table(payloads, isizes, crcs, rng):
    in_off = np.zeros(len(payloads), np.int64)
    buf, o = [], 0
    for i, p in enumerate(payloads):   # payloads at odd, unaligned offsets
        pad = int(rng.integers(0, 4))
        buf.append(b"\x00" * pad)
        o += pad
        in_off[i] = o
        buf.append(p)
        o += len(p)
    payload = np.frombuffer(b"".join(buf) + b"\x00", np.uint8).copy()
    out_off, total = layout(isizes, rng)
    return payload, in_off, np.array([len(p) for p in payloads], np.int32), np.asarray(isizes, np.int32), \
        np.asarray(crcs, np.uint32), out_off, total


def test_corpus_is_byte_identical_to_zlib(hip_ctx):
    rng = np.random.default_rng(1)
    cs = corpus()
    raws = [r for _, r, _ in cs]
    payload, in_off, clen, isize, crc, out_off, total = table([p for _, _, p in cs], [len(r) for r in raws],
                                                              [zlib.crc32(r) & 0xFFFFFFFF for r in raws], rng)
    out = np.full(total, GUARD, np.uint8)
    out, status, counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off, out)
    bad = {cs[i][0]: int(status[i]) for i in np.flatnonzero(status)}
    assert not bad, bad
    assert counts == (sum(len(r) for r in raws), _ffi.PV_OK, -1, 0)
    mask = np.ones(total, bool)
    for (nm, raw, _), o in zip(cs, out_off):
        assert out[o:o + len(raw)].tobytes() == raw, nm
        mask[o:o + len(raw)] = False
    assert np.all(out[mask] == GUARD)


def test_matches_32767_and_32768_back(hip_ctx):
    """the largest distances DEFLATE allows: at 32768 a copy reads and writes the same slot of the 32 KiB history ring"""
    rng = np.random.default_rng(11)
    cs = far_matches(np.random.default_rng(5))
    for nm, raw, pay in cs:
        assert zlib.decompress(pay, -15) == raw, nm
        d = zlib.decompressobj(-15)
        assert d.decompress(pay) == raw and d.eof
    raws = [r for _, r, _ in cs]
    payload, in_off, clen, isize, crc, out_off, total = table([p for _, _, p in cs], [len(r) for r in raws],
                                                              [zlib.crc32(r) & 0xFFFFFFFF for r in raws], rng)
    out, status, counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off, np.full(total, GUARD, np.uint8))
    assert status.tolist() == [0] * len(cs), status
    for (nm, raw, _), o in zip(cs, out_off):
        assert out[o:o + len(raw)].tobytes() == raw, nm


def test_big_mixed_batch_with_bad_blocks(hip_ctx):
    """8192+ blocks, outputs shuffled and apart; every crafted failure is reported at its own index, every other block of
    the same batch decodes, and no byte outside a block's range changes"""
    rng = np.random.default_rng(2)
    cs = corpus()
    bads = crafted()
    n = 8192 + len(bads)
    pick = rng.integers(0, len(cs), n)
    bad_at = rng.choice(n, len(bads), replace=False)
    pays, isz, crcs, want = [], [], [], []
    for i in range(n):
        nm, raw, pay = cs[pick[i]]
        pays.append(pay); isz.append(len(raw)); crcs.append(zlib.crc32(raw) & 0xFFFFFFFF); want.append(raw)
    for k, i in enumerate(bad_at):
        nm, pay, s, c, st = bads[k]
        pays[i], isz[i], crcs[i], want[i] = pay, s, c, None
    payload, in_off, clen, isize, crc, out_off, total = table(pays, [min(s, 65536) for s in isz], crcs, rng)
    isize = np.asarray(isz, np.int32)
    out = np.full(total + 65536, GUARD, np.uint8)
    out, status, counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off, out)
    exp_status = np.zeros(n, np.int32)
    for k, i in enumerate(bad_at):
        exp_status[i] = bads[k][4]
    mism = {bads[k][0]: (int(status[i]), bads[k][4]) for k, i in enumerate(bad_at) if status[i] != bads[k][4]}
    assert not mism, mism
    np.testing.assert_array_equal(status, exp_status)
    first = int(np.sort(bad_at)[0])
    assert counts == (sum(len(w) for w in want if w is not None), _ffi.PV_ERR_INVALID, first, int(exp_status[first]))
    mask = np.ones(out.size, bool)
    for i in range(n):
        o = int(out_off[i])
        s = min(int(isz[i]), 65536)
        if want[i] is not None:
            assert out[o:o + s].tobytes() == want[i], i
        mask[o:o + s] = False   # a failed block may have written inside its own range, never outside
    assert np.all(out[mask] == GUARD)


def test_device_form_on_a_second_stream_agrees(hip_ctx):
    import torch
    rng = np.random.default_rng(3)
    cs = corpus() * 40
    raws = [r for _, r, _ in cs]
    payload, in_off, clen, isize, crc, out_off, total = table([p for _, _, p in cs], [len(r) for r in raws],
                                                              [zlib.crc32(r) & 0xFFFFFFFF for r in raws], rng)
    crc[5] ^= 0xFFFF
    host_out, host_status, host_counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off,
                                                              np.full(total, GUARD, np.uint8))
    dev = "cuda:%d" % hip_ctx.device_id
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(payload=payload, in_off=in_off, clen=clen, isize=isize, crc=crc.view(np.int32), out_off=out_off).items()}
    d_out = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    d_status = torch.empty(len(cs), dtype=torch.int32, device=dev)
    d_counts = torch.empty(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    hip_ctx.bgzf_inflate_dev(t["payload"].data_ptr(), payload.size, len(cs), t["in_off"].data_ptr(), t["clen"].data_ptr(),
                             t["isize"].data_ptr(), t["crc"].data_ptr(), t["out_off"].data_ptr(), d_out.data_ptr(), total,
                             d_status.data_ptr(), d_counts.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert tuple(d_counts.cpu().tolist()) == host_counts
    assert host_counts[1] == _ffi.PV_ERR_INVALID and host_counts[2] == 5 and host_counts[3] == _ffi.PV_BGZF_CRC_MISMATCH
    np.testing.assert_array_equal(d_status.cpu().numpy(), host_status)
    np.testing.assert_array_equal(d_out.cpu().numpy(), host_out)


# ---- the reader mode end to end ----------------------------------------------------------------------------------------

def _reads_bam(tmp_path, seed=17, length=40_000, n_reads=500, **bam_kw):
    import bam_writer as bw
    from pepper_thesis_amd import build
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
    bw.write_bam(str(tmp_path / "reads.bam"), [("chr20", len(ref))], recs, **bam_kw)
    return str(tmp_path / "reads.bam"), str(tmp_path / "ref.fa")


def _pred_records(path):
    from pepper_thesis_amd import hdf5io
    with hdf5io.PredictionStore(path, "r") as st:
        return [(k, {f: v.tolist() for f, v in bt.items()}) for k, bt in st.batches()]


def test_call_variant_fused_gpu_inflate_gives_identical_predictions(hip_ctx, tmp_path):
    from pepper_thesis_amd import pipeline, synth
    from pepper_thesis_amd.batch import PRESETS
    bam, fa = _reads_bam(tmp_path)
    w = synth.make_weights_p1(3, 3.0)
    P = PRESETS["ont_r9_guppy5_sup"]
    T0, T1 = {}, {}
    n0 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "host.hdf"), P, "chr20:1000-39000", 6000,
                                     intervals_per_call=4, timers=T0)
    n1 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "gpu.hdf"), P, "chr20:1000-39000", 6000,
                                     intervals_per_call=4, timers=T1, gpu_inflate=True)
    assert n0 == n1 > 100
    assert _pred_records(str(tmp_path / "host.hdf")) == _pred_records(str(tmp_path / "gpu.hdf"))
    assert T1["gpu_inflate_blocks"] > 0 and T1["gpu_inflate_launches"] >= 1 and "gpu_inflate_blocks" not in T0
    assert T1["gpu_inflate_bytes"] > 0 and T1["gpu_inflate_kernel_ms"] > 0


def test_make_images_and_call_variant_cli_gpu_inflate(tmp_path):
    from pepper_thesis_amd import call_variant, hdf5io, make_images, synth
    bam, fa = _reads_bam(tmp_path, seed=5)
    base = ["-b", bam, "-f", fa, "-r", "chr20:2000-38000", "--region_size", "12000", "--ont_r9_guppy5_sup"]
    make_images.main(base + ["-o", str(tmp_path / "img_host")])
    make_images.main(base + ["-o", str(tmp_path / "img_gpu"), "--gpu_inflate"])
    name = "pepper_variants_images_thread_0.hdf5"
    with hdf5io.ImageStore(str(tmp_path / "img_host" / name), "r") as a, hdf5io.ImageStore(str(tmp_path / "img_gpu" / name), "r") as b:
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
    c1 = call_variant.main(cv + ["-o", str(tmp_path / "cv_gpu"), "--gpu_inflate"])
    assert c0 == c1 and c0["total"] > 0
    for fn in ("PEPPER_VARIANT_FULL.vcf.gz", "PEPPER_VARIANT_OUTPUT_VARIANT_CALLING.vcf.gz"):
        body = [[ln for ln in gzip.open(str(d / fn), "rt").read().splitlines() if not ln.startswith("#")]
                for d in (tmp_path / "cv_host", tmp_path / "cv_gpu")]
        assert body[0] == body[1], fn


def test_corrupt_block_in_a_query_raises_in_gpu_mode(hip_ctx, tmp_path):
    from pepper_thesis_amd import pipeline, synth
    from pepper_thesis_amd.batch import PRESETS
    bam, fa = _reads_bam(tmp_path, seed=9)
    raw = bytearray(open(bam, "rb").read())
    offs, p = [], 0
    while p < len(raw):
        offs.append(p)
        p += int.from_bytes(raw[p + 16:p + 18], "little") + 1
    assert len(offs) >= 8
    victim = offs[len(offs) // 2]
    raw[victim + 18 + 60] ^= 0x5A
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(raw))
    open(bad + ".bai", "wb").write(open(bam + ".bai", "rb").read())
    w = synth.make_weights_p1(3, 3.0)
    with pytest.raises(IOError) as ei:
        pipeline.call_variant_fused(hip_ctx, w, bad, fa, str(tmp_path / "p.hdf"), PRESETS["ont_r9_guppy5_sup"],
                                    "chr20:1000-39000", 6000, intervals_per_call=4, gpu_inflate=True)
    assert "offset %d" % victim in str(ei.value)
    # the context and the reader mode still work afterwards
    n = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "ok.hdf"), PRESETS["ont_r9_guppy5_sup"],
                                    "chr20:1000-39000", 6000, intervals_per_call=4, gpu_inflate=True)
    assert n > 100
