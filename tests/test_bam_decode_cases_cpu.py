"""CPU: the cases of bam_decode_cases hold what they were built to hold, and every record stream of theirs that is a valid
BAM, written as a real file (BGZF, BAI) and read by the host reader (bamio, csrc/pv_io.cpp), gives what the restatement
(bam_decode_ref) gives: the host reader, the restatement and the device (test_bam_decode_limits_gpu) stay in agreement."""
import numpy as np
import pytest

import bam_decode_cases as cases
import bam_decode_ref as ref
import bam_writer as bw
from pepper_thesis_amd import bamio, build

REFS = [("c0", cases.BIG), ("c1", cases.BIG), ("c2", cases.BIG)]


@pytest.fixture(scope="module", autouse=True)
def _io():
    build.build_io()


@pytest.mark.parametrize("name", sorted(cases.ALL_LAUNCHES))
def test_every_case_holds_what_it_was_built_to_hold(name):
    L = cases.ALL_LAUNCHES[name]()
    L.checks()
    assert sum(iv["check"] is not None for iv in L.ivs) == len(L.ivs)


def test_pass_size_cases_hold():
    for n in (255, 256, 257, 513):
        cases.intervals_launch(n).checks()
    for n in (1023, 1024, 1025, 2049):
        cases.fill_launch(n).checks()
    for c in cases.status_cases():
        c["launch"].checks()
        assert len(c["launch"].ivs) == 3 and 0 < c["bad"] < 3, c["name"]


def same_as_host(records, queries, block_bytes, tmp_path, supp=False, mq=0):
    """queries: {(tid, rs, re)}; -> reads compared"""
    assert all(r.get("raw") is None for r in records)
    key = lambda r: (r["tid"] if r["tid"] >= 0 else 1 << 31, r["pos"])   # noqa: E731
    assert [key(r) for r in records] == sorted(key(r) for r in records), "a BAM is sorted"
    path = str(tmp_path / "c.bam")
    bw.write_bam(path, REFS, records, block_bytes=block_bytes)
    bam = bamio.BamHandler(path)
    n = 0
    for tid, rs, re in sorted(queries):
        assert rs < re, "the index query [rs, re) of such a window is empty: no restatement comparison"
        e = ref.decode_interval([records], tid, rs, re, supp, mq)
        if e["status"] != ref.OK:
            with pytest.raises(IOError) as eh:
                bam.get_reads("c%d" % tid, rs, re, supp, mq)
            assert e["status"] == ref.CIGAR_LONGER and "CIGAR longer than SEQ" in str(eh.value)
            continue
        got = bam.get_reads("c%d" % tid, rs, re, supp, mq)
        assert len(got) == len(e["reads"]), (tid, rs, re)
        for g, x in zip(got, e["reads"]):
            assert (g.pos, g.bases, bytes(g.quals), g.cigar.tolist(), int(g.is_reverse), g.mapq, g.hp_tag) == \
                   (x["pos"], x["seq"], x["qual"], x["cigar"], x["rev"], x["mapq"], x["hp"]), (tid, rs, re, x["listed"])
        n += len(got)
    bam.close()
    return n


@pytest.mark.parametrize("name", ["clip", "aux", "geometry", "intervals_257", "records", "fill_1025", "fill_limits"])
@pytest.mark.parametrize("block_bytes", [None, 97])
def test_host_reader_agrees_with_the_restatement(name, block_bytes, tmp_path):
    L = cases.ALL_LAUNCHES[name]()
    by_records = {}
    for iv in L.ivs:
        st = L.groups[iv["gi"]][0]
        recs, q = by_records.setdefault(tuple(id(r) for r in st.records), (st.records, set()))
        q.add((iv["tid"], iv["rs"], iv["re"]))
    if name == "intervals_257":   # (every interval is a query of the one file: keep a spread of them)
        (recs, q), = by_records.values()
        by_records = {0: (recs, set(sorted(q)[::7]))}
    n = 0
    for k, (recs, q) in enumerate(by_records.values()):
        if len(recs) > 1000 and block_bytes:   # (tiny blocks under the long streams add time and nothing else)
            continue
        d = tmp_path / ("g%d" % k)
        d.mkdir()
        n += same_as_host(recs, q, block_bytes, d, L.supp, L.mq)
    assert n > 0


def test_a_record_that_ends_with_a_full_block(tmp_path):
    recs = cases.full_block_records()
    assert cases.Stream(recs, (65536,)).end(3) == 65536
    # reads of four bases at 100, 101, 102, 110, 120, 121: all six; those over [105, 111]; those over [111, 1000]
    assert same_as_host(recs, {(0, 0, 1000), (0, 105, 111), (0, 111, 1000)}, 65536, tmp_path) == 6 + 2 + 3


def test_write_bam_options():
    """block_bytes cuts records anywhere; aux bytes are written as given"""
    r = cases.rec(5, [(0, 4)], aux=b"XYZab\x00")
    assert bw.record_bytes(r).endswith(b"XYZab\x00") and bw.record_bytes(dict(r, aux=None)).endswith(b"RGZgrp1\x00")
    assert np.frombuffer(bw.record_bytes(r)[:4], "<u4")[0] == len(bw.record_bytes(r)) - 4
