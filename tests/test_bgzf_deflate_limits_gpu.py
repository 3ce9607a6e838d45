"""GPU: the BGZF inflate kernel (pv_bgzf_inflate[_dev]) at DEFLATE's own format limits: the named streams of deflate_cases,
which no compressor emits, a seeded differential run against the token writer, a seeded mutation run judged by zlib, the
device form, and a BAM whose blocks come from the writer read end to end. test_deflate_cases_cpu.py shows on the CPU that
zlib agrees with every expectation used here. Every comparison is exact."""
import collections
import random
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_writer as dw
from pepper_thesis_amd import _ffi
from test_bgzf_inflate_gpu import GUARD, _pred_records, _reads_bam, table

pytestmark = pytest.mark.gpu


def launch(hip_ctx, entries, seed):
    """entries [(payload, isize, crc)] at unaligned input offsets, outputs shuffled with guard gaps between them"""
    rng = np.random.default_rng(seed)
    payload, in_off, clen, isize, crc, out_off, total = table([e[0] for e in entries], [e[1] for e in entries],
                                                              [e[2] for e in entries], rng)
    out, status, counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off, np.full(total, GUARD, np.uint8))
    return out, status, counts, out_off


def guards_intact(out, out_off, sizes):
    mask = np.ones(out.size, bool)
    for o, s in zip(out_off, sizes):
        mask[int(o):int(o) + int(s)] = False
    return bool(np.all(out[mask] == GUARD))


def good(raw, payload):
    return payload, len(raw), dc.crc32(raw)


def libdeflate_streams():
    """streams of libdeflate's own compressor at levels 1, 6 and 12, where the library loads"""
    compress = dc.libdeflate_compress()
    if compress is None:
        return []
    rng = random.Random(12)
    data = {"tokens": dw.expand(dc.random_tokens(rng, 65536, 0, 0.6, list(range(48, 112)))),
            "skewed": bytes(min(255, int(rng.expovariate(0.05))) for _ in range(40000)),
            "random": bytes(rng.randrange(256) for _ in range(20000))}
    out = []
    for nm, raw in data.items():
        for level in (1, 6, 12):
            pay = compress(raw, level)
            assert zlib.decompress(pay, -15) == raw
            out.append(("libdeflate_%s_level_%d" % (nm, level), raw, pay))
    return out


def test_named_cases_are_byte_identical(hip_ctx):
    cs = dc.named()
    extra = libdeflate_streams()
    print("libdeflate's compressor: %s" % ("%d streams added" % len(extra) if extra else "not loaded"))
    cs = cs + extra
    out, status, counts, out_off = launch(hip_ctx, [good(raw, pay) for _, raw, pay in cs], 1)
    bad = {cs[i][0]: int(status[i]) for i in np.flatnonzero(status)}
    assert not bad, bad
    assert counts == (sum(len(raw) for _, raw, _ in cs), _ffi.PV_OK, -1, 0)
    for (nm, raw, _), o in zip(cs, out_off):
        assert out[o:o + len(raw)].tobytes() == raw, nm
    assert guards_intact(out, out_off, [len(raw) for _, raw, _ in cs])


def test_refused_cases_each_report_their_status_beside_good_blocks(hip_ctx):
    rng = random.Random(6)
    cs = dc.named()[::16]
    bads = dc.refused()
    entries = [good(raw, pay) for _, raw, pay in cs]
    want = [raw for _, raw, _ in cs]
    names = [nm for nm, _, _ in cs]
    for nm, pay, isize, crc, st in bads:
        i = rng.randint(0, len(entries))
        entries.insert(i, (pay, isize, crc))
        want.insert(i, None)
        names.insert(i, nm)
    exp = np.zeros(len(entries), np.int32)
    for nm, _, _, _, st in bads:
        exp[names.index(nm)] = getattr(_ffi, st)
    out, status, counts, out_off = launch(hip_ctx, entries, 2)
    mism = {nm: (int(s), int(e)) for nm, s, e in zip(names, status, exp) if s != e}
    assert not mism, mism
    first = int(np.flatnonzero(exp)[0])
    assert counts == (sum(len(w) for w in want if w is not None), _ffi.PV_ERR_INVALID, first, int(exp[first]))
    for nm, w, o in zip(names, want, out_off):
        if w is not None:
            assert out[o:o + len(w)].tobytes() == w, nm
    assert guards_intact(out, out_off, [e[1] for e in entries])


def test_seeded_streams_from_the_writer(hip_ctx):
    streams = dc.seeded_streams()
    agg = dw.aggregate_stats(dw.stream_stats(p) for _, p, _ in streams)
    print("seeded run:", agg)
    assert len(streams) == 2000
    assert agg["lit_used"] == 15 and agg["dist_used"] == 15 and agg["cross_runs"] >= 1 and agg["max_pair_bits"] >= 45, agg
    out, status, counts, out_off = launch(hip_ctx, [good(raw, pay) for raw, pay, _ in streams], 3)
    bad = {int(i): int(status[i]) for i in np.flatnonzero(status)}
    assert not bad, bad
    assert counts == (sum(len(raw) for raw, _, _ in streams), _ffi.PV_OK, -1, 0)
    for k, ((raw, _, _), o) in enumerate(zip(streams, out_off)):
        assert out[o:o + len(raw)].tobytes() == raw, k
    assert guards_intact(out, out_off, [len(raw) for raw, _, _ in streams])


def test_bit_flipped_streams_agree_with_zlib(hip_ctx):
    """zlib is the judge of a stream with flipped bits: where it reaches the end of the stream the kernel gives the same
    bytes, everywhere else the kernel refuses with the unharmed stream's length and CRC"""
    inputs = dc.mutation_inputs()
    entries, want = [], []
    n_drop = 0
    for raw, pay in inputs:
        verdict, got = dc.judge(pay)
        if verdict == "drop":
            n_drop += 1
        elif verdict == "accept":
            entries.append(good(got, pay))
            want.append(got)
        else:
            entries.append(good(raw, pay))
            want.append(None)
    n_acc, n_ref = sum(w is not None for w in want), sum(w is None for w in want)
    print("mutation run: %d accepted, %d refused, %d dropped" % (n_acc, n_ref, n_drop))
    n = len(inputs)
    assert n == 3000 and n_acc >= n // 4 and n_ref >= n // 4 and n_drop <= n // 50       # conditions on the inputs
    out, status, counts, out_off = launch(hip_ctx, entries, 4)
    wrong = collections.OrderedDict()
    for k, (w, o, s) in enumerate(zip(want, out_off, status)):
        if w is None:
            if s == 0:
                wrong[k] = "zlib refuses, the kernel accepts"
        elif s != 0:
            wrong[k] = "zlib accepts %d bytes, the kernel says %d" % (len(w), int(s))
        elif out[o:o + len(w)].tobytes() != w:
            wrong[k] = "bytes differ"
    assert not wrong, (len(wrong), list(wrong.items())[:10])
    assert counts[0] == sum(len(w) for w in want if w is not None)
    assert guards_intact(out, out_off, [e[1] for e in entries])


def test_device_form_on_a_second_stream_agrees_on_the_named_cases(hip_ctx):
    import torch
    cs = dc.named()
    bads = dc.refused()
    entries = [good(raw, pay) for _, raw, pay in cs]
    for k, (nm, pay, isize, crc, st) in enumerate(bads):
        entries.insert(50 + 90 * k, (pay, isize, crc))
    rng = np.random.default_rng(5)
    payload, in_off, clen, isize, crc, out_off, total = table([e[0] for e in entries], [e[1] for e in entries],
                                                              [e[2] for e in entries], rng)
    host_out, host_status, host_counts = hip_ctx.bgzf_inflate(payload, in_off, clen, isize, crc, out_off,
                                                              np.full(total, GUARD, np.uint8))
    dev = "cuda:%d" % hip_ctx.device_id
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(payload=payload, in_off=in_off, clen=clen, isize=isize, crc=crc.view(np.int32), out_off=out_off).items()}
    d_out = torch.full((total,), GUARD, dtype=torch.uint8, device=dev)
    d_status = torch.empty(len(entries), dtype=torch.int32, device=dev)
    d_counts = torch.empty(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    hip_ctx.bgzf_inflate_dev(t["payload"].data_ptr(), payload.size, len(entries), t["in_off"].data_ptr(), t["clen"].data_ptr(),
                             t["isize"].data_ptr(), t["crc"].data_ptr(), t["out_off"].data_ptr(), d_out.data_ptr(), total,
                             d_status.data_ptr(), d_counts.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert tuple(d_counts.cpu().tolist()) == host_counts
    assert host_counts[1:] == (_ffi.PV_ERR_INVALID, 50, getattr(_ffi, bads[0][4]))
    assert int(np.count_nonzero(host_status)) == len(bads)
    np.testing.assert_array_equal(d_status.cpu().numpy(), host_status)
    np.testing.assert_array_equal(d_out.cpu().numpy(), host_out)


def test_call_variant_fused_reads_a_bam_of_writer_blocks(hip_ctx, tmp_path):
    """every block of the BAM is one dynamic block with random complete codes of up to 15 bits and a run-length-encoded
    header, from a greedy tokeniser: the GPU inflate reader gives the prediction records of the host inflate"""
    from pepper_thesis_amd import pipeline, synth
    from pepper_thesis_amd.batch import PRESETS
    bam, fa = _reads_bam(tmp_path, seed=23, length=12_000, n_reads=100, block_records=4,
                         deflate=dc.writer_deflate(random.Random(5)))
    w = synth.make_weights_p1(3, 3.0)
    P = PRESETS["ont_r9_guppy5_sup"]
    T0, T1 = {}, {}
    n0 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "host.hdf"), P, "chr20:1000-9000", 4000,
                                     intervals_per_call=4, timers=T0)
    n1 = pipeline.call_variant_fused(hip_ctx, w, bam, fa, str(tmp_path / "gpu.hdf"), P, "chr20:1000-9000", 4000,
                                     intervals_per_call=4, timers=T1, gpu_inflate=True)
    assert n0 == n1 > 0
    assert _pred_records(str(tmp_path / "host.hdf")) == _pred_records(str(tmp_path / "gpu.hdf"))
    assert T1["gpu_inflate_blocks"] > 0 and "gpu_inflate_blocks" not in T0
