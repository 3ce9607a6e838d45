"""CPU: the DEFLATE streams of deflate_cases against zlib, so that what the GPU test expects of the inflate kernel does not
depend on the kernel: zlib decodes every accepted case and every seeded stream to the bytes the tokens expand to, refuses
every refused case, and every named case carries the feature it is named for (deflate_writer.stream_stats)."""
import random
import zlib

import pytest

import deflate_cases as dc
import deflate_writer as dw


def inflate(payload):
    d = zlib.decompressobj(-15)
    return d.decompress(payload), d.eof, d.unused_data


def test_bits_writes_lsb_first_and_codes_msb_first():
    assert dw.Bits().put(1, 1).put(2, 2).put(0x15, 5).tobytes() == bytes([0xAD])
    assert dw.Bits().code(0b110, 3).tobytes() == bytes([0b011])
    assert dw.Bits().put(1, 1).bytes() == b"\x01\x00"
    assert dw.Bits().stored(b"hi", 1).tobytes() == bytes([1, 2, 0, 0xFD, 0xFF]) + b"hi"
    assert dw.canonical_codes([2, 1, 3, 3]) == [(0b01, 2), (0b0, 1), (0b011, 3), (0b111, 3)]    # RFC 1951 3.2.2, bits reversed
    assert dw.length_symbols(258) == [284, 285] and dw.length_symbols(3) == [257] and dw.length_symbols(227) == [284]
    assert [dw.dist_symbol(d) for d in (1, 4, 5, 6, 24576, 24577, 32768)] == [0, 3, 4, 4, 28, 29, 29]


def test_run_length_header_round_trips_and_is_greedy():
    rng = random.Random(9)
    assert dw.rle_lengths([0] * 139 + [5] * 8 + [0] * 3 + [4, 4], "runs") == \
        [(18, 127), (0, 0), (5, 0), (16, 3), (5, 0), (17, 0), (4, 0), (4, 0)]
    for _ in range(300):
        lens = []
        while len(lens) < 300:
            lens += [rng.choice((0, 0, 3, 7, 15))] * rng.choice((1, 2, 3, 6, 7, 11, 140))
        for style in ("plain", "runs"):
            assert dw.expand_header(dw.rle_lengths(lens, style)) == lens


@pytest.mark.parametrize("max_len", [7, 9, 12, 15])
def test_complete_lengths_are_complete_and_bounded(max_len):
    rng = random.Random(max_len)
    for n in (2, 3, 19, 30, 100, 128):
        for force in (False, True):
            lens = dw.complete_lengths(rng, n, max_len, force)
            assert len(lens) == n and dw.kraft(lens) == 32768 and 1 <= min(lens) and max(lens) <= max_len
            if force and n > max_len:
                assert max(lens) == max_len
    assert dw.complete_lengths(rng, 1, max_len) == [1]


def test_stream_stats_decodes_what_zlib_compressed():
    """the inspector is a decoder of its own: it agrees with zlib on zlib's own streams of every block type"""
    rng = random.Random(4)
    data = dw.expand(dc.random_tokens(rng, 30000, 0, 0.6, list(range(64))))
    for level in (0, 1, 6, 9):
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            pay = co.compress(data) + co.flush()
            st = dw.stream_stats(pay)
            assert st["out"] == data and (st["end_bit"] + 7) // 8 == len(pay)


def test_accepted_cases_decode_with_zlib_to_what_the_tokens_expand_to():
    cases = dc.accepted()
    for c in cases:
        out, eof, unused = inflate(c.payload)
        assert out == c.raw and eof and unused == b"", c.name
        assert dw.expand(c.tokens) == c.raw, c.name
        assert len(c.raw) <= 65536, c.name
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    assert sum(n.startswith("pair_48_bits_at_bit_") for n in names) == 32
    assert sum(n.startswith("copy_dist_") for n in names) == len(dc.COPY_DISTS) * len(dc.COPY_LENS) == 552
    assert {"isize_%d" % s for s in dc.ISIZES} <= names


def test_every_named_case_carries_its_feature():
    for c in dc.accepted():
        st = dw.stream_stats(c.payload)
        assert c.check(st), c.name
        assert st["out"] == c.raw, c.name
        assert (st["end_bit"] + 7) // 8 == len(c.payload), c.name      # the stream ends in the payload's last byte


def test_refused_cases_are_refused_by_zlib_and_by_the_inspector():
    names = [r[0] for r in dc.refused()]
    assert len(set(names)) == len(names) == 6
    for name, payload, isize, crc, status in dc.refused():
        assert dc.judge(payload) == ("refuse", None), name
        with pytest.raises(zlib.error):
            zlib.decompress(payload, -15)
        with pytest.raises(ValueError):
            dw.stream_stats(payload)
        assert status in ("PV_BGZF_BAD_CODE_LENGTHS", "PV_BGZF_BAD_SYMBOL")


def test_seeded_streams_decode_with_zlib_to_what_the_tokens_expand_to():
    streams = dc.seeded_streams()
    assert len(streams) == 2000
    for k, (raw, payload, tokens) in enumerate(streams):
        out, eof, unused = inflate(payload)
        assert out == raw and eof and unused == b"", k
        assert dw.expand(tokens) == raw and 1 <= len(raw) <= 8192, k
    agg = dw.aggregate_stats(dw.stream_stats(p) for _, p, _ in streams)
    assert agg["lit_used"] == 15 and agg["dist_used"] == 15 and agg["cross_runs"] > 0 and agg["max_pair_bits"] >= 45, agg


def test_mutation_inputs_fall_in_both_classes():
    """conditions on the inputs of the mutation run: a quarter at least accepted and refused by zlib, 2 % at most dropped"""
    inputs = dc.mutation_inputs()
    verdicts = [dc.judge(p)[0] for _, p in inputs]
    n = len(inputs)
    assert n == 3000
    assert verdicts.count("accept") >= n // 4 and verdicts.count("refuse") >= n // 4 and verdicts.count("drop") <= n // 50
    for (raw, p), v in zip(inputs, verdicts):
        assert 1 <= len(raw) <= 8192


def test_writer_deflate_makes_blocks_that_zlib_reads():
    rng = random.Random(2)
    deflate = dc.writer_deflate(rng)
    data = dw.expand(dc.random_tokens(rng, 20000, 0, 0.5, list(range(16))))
    for piece in (data, data[:1], b"", b"abcabcabcabc" * 50):
        pay = deflate(piece)
        assert inflate(pay) == (piece, True, b"")
        st = dw.stream_stats(pay)
        assert st["lit_declared"] == 15 and st["blocks"][0]["hlit"] == 286 and st["blocks"][0]["hdist"] == 30
    assert dw.stream_stats(deflate(data))["n_matches"] > 100


def test_write_bam_takes_a_deflate_callable(tmp_path):
    import numpy as np

    import bam_writer as bw
    recs = bw.random_records(np.random.default_rng(3), 12, 5000, tid=0, mean_len=400, allow_skip=False)
    calls = []

    def deflate(data):
        calls.append(len(data))
        return dc.writer_deflate(random.Random(len(calls)))(data)

    bw.write_bam(str(tmp_path / "z.bam"), [("c1", 5000)], recs, block_records=5)
    bw.write_bam(str(tmp_path / "w.bam"), [("c1", 5000)], recs, block_records=5, deflate=deflate)
    assert len(calls) == 4                  # the header and three blocks of records

    def members(path):
        raw, p, out = open(path, "rb").read(), 0, []
        while p < len(raw):
            bsize = int.from_bytes(raw[p + 16:p + 18], "little") + 1
            out.append(zlib.decompress(raw[p + 18:p + bsize - 8], -15))
            assert zlib.crc32(out[-1]) == int.from_bytes(raw[p + bsize - 8:p + bsize - 4], "little")
            p += bsize
        return out
    assert members(str(tmp_path / "z.bam")) == members(str(tmp_path / "w.bam"))
    assert open(str(tmp_path / "z.bam.bai"), "rb").read() != b""
