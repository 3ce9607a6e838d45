"""Realignment (polish --realign) on the host: the checker against the reference fixture, the read-loop rules and the CLI."""
import os

import numpy as np
import pytest

import realign_cases
import realign_ref
from pepper_thesis_amd.batch import Read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "realign_golden.npz"), allow_pickle=False)


def golden_cases(g):
    """-> [(name, start, window, reads, records [n, 7], cigars [list of uint32 arrays])]"""
    out = []
    for name in (n.decode() for n in g["names"]):
        bo, co, ico = g[name + "/base_off"], g[name + "/cigar_off"], g[name + "/in_cigar_off"]
        bases, cig, icig = g[name + "/bases"].tobytes(), g[name + "/cigar"], g[name + "/in_cigar"]
        reads = [Read(int(p), icig[ico[k]:ico[k + 1]], bases[bo[k]:bo[k + 1]], np.full(bo[k + 1] - bo[k], 20, np.uint8))
                 for k, p in enumerate(g[name + "/read_pos"].tolist())]
        cigars = [cig[co[k]:co[k + 1]] for k in range(len(reads))]
        out.append((name, int(g[name + "/start"]), g[name + "/window"].tobytes(), reads, g[name + "/record"], cigars))
    return out


def test_fixture_covers_the_issue_cases(golden):
    recs = np.concatenate([c[4] for c in golden_cases(golden)])
    assert (recs[:, 0] == realign_ref.DROPPED).any()
    assert ((recs[:, 0] == realign_ref.UNCHANGED) & (recs[:, 1] <= 1)).any()
    assert (recs[:, 1] > 255).any()
    assert (recs[:, 0] == realign_ref.REALIGNED).sum() > 200


def test_checker_reproduces_the_reference(golden):
    n = 0
    for name, start, win, reads, recs, cigars in golden_cases(golden):
        got = realign_ref.realign_reads(start, win, reads)
        for k, (r, exp, ecig) in enumerate(zip(got, recs.tolist(), cigars)):
            tag = "%s read %d" % (name, k)
            assert (r.state, r.score) == (exp[0], exp[1]), tag
            if exp[0] == realign_ref.REALIGNED:
                assert (r.ref_begin, r.ref_end, r.query_begin, r.query_end, r.new_pos) == tuple(exp[2:7]), tag
                assert np.array_equal(r.cigar, ecig), tag
                n += 1
            elif exp[0] == realign_ref.UNCHANGED:
                assert np.array_equal(r.cigar, reads[k].cigar) and r.new_pos == reads[k].pos, tag
    assert n > 200


def limit_golden_cases(g):
    """the fixture's cases at the realigner's limits, their inputs rebuilt from the seeds of realign_cases (the fixture holds
    a digest of them and the reference's outputs) -> [(name, start, window, read, record [7], cigar)]"""
    out = []
    for (group, region, read), name in zip(realign_cases.FIXTURE_CASES, (n.decode() for n in g["limit_names"])):
        fname, start, win, rd = realign_cases.fixture_case(group, region, read)
        assert fname == name
        assert np.array_equal(realign_cases.input_digest(start, win, [rd]), g[name + "/input_sha1"]), \
            "%s: the seeded inputs are not the ones the fixture was made from" % name
        assert g[name + "/cigar_off"].tolist() == [0, len(g[name + "/cigar"])]
        out.append((name, start, win, rd, g[name + "/record"][0].tolist(), g[name + "/cigar"]))
    return out


def test_checker_reproduces_the_reference_at_the_limits(golden):
    """the reference's striped Smith-Waterman on the largest legal score (alone, inside a 16384-base query, on a
    homopolymer), a period-2 repeat, a band over the whole window and a dense cigar: the checker gives every field"""
    cases = limit_golden_cases(golden)
    assert len(cases) == 6
    by_name = {}
    for name, start, win, rd, exp, ecig in cases:
        r, = realign_ref.realign_reads(start, win, [rd])
        assert exp[0] == realign_ref.REALIGNED
        assert (r.state, r.score, r.ref_begin, r.ref_end, r.query_begin, r.query_end, r.new_pos) == tuple(exp), name
        assert np.array_equal(r.cigar, ecig), name
        by_name[name.split("/", 1)[1]] = (r, rd)
    # the reference's own figures are the ones these cases were chosen for
    for k in ("saturation/full/0", "saturation/full/1", "saturation/homopolymer/0"):
        assert by_name[k][0].score == 8188, k
    r, rd = by_name["saturation/full/1"]
    assert (r.ref_begin, r.ref_end, r.query_begin, r.query_end) == (0, 2046, 7000, 9046) and len(rd.bases) == 16384
    r = by_name["saturation/full/0"][0]
    assert (r.ref_begin, r.ref_end, r.query_begin, r.query_end) == (0, 2046, 0, 2046)
    assert by_name["saturation/period2/0"][0].score == 2400
    r = by_name["bands/bands/4"][0]
    assert 2 * r.band + 1 >= r.ref_end - r.ref_begin + 1 == 2047
    assert len(by_name["dense/dense/0"][0].cigar) > 1000


def test_window_drop_keep_and_op_mapping():
    win = b"ACGTACGTTTGCA" + b"GGGGCCCC" + b"A" * 19
    start = 100
    reads = [Read.make(99, "4M", b"ACGT"),            # starts before the region: dropped
             Read.make(104, "4M", b"ACGT"),           # realigned against window[4:]
             Read.make(100, "3M", b"NNN"),            # score 0: kept as it was
             Read.make(100 + len(win), "2M", b"AC"),  # at the end of the window: nothing to align to, kept
             Read.make(102, "5M", b"GTAAGTTT")]       # an insertion in the middle
    recs = realign_ref.realign_reads(start, win, reads)
    assert [r.state for r in recs] == [2, 1, 0, 0, 1]
    assert recs[1].new_pos == 104 and recs[1].cigar.tolist() == [(4 << 4) | 0]
    assert recs[2].cigar.tolist() == reads[2].cigar.tolist() and recs[2].new_pos == 100
    ops = [(int(w) & 15, int(w) >> 4) for w in recs[4].cigar]
    assert sum(n for op, n in ops if op in (0, 1, 4)) == 8
    assert all(op in (0, 1, 2, 4) for op, _ in ops)


def test_equal_and_mismatch_runs_stay_apart_and_n_is_equal():
    sc, rb, re_, qb, qe, cig = realign_ref.align(b"AAAANAAAA", b"AAAANAAAA")
    assert [(int(w) & 15, int(w) >> 4) for w in cig] == [(7, 9)]           # N vs N is '=' (scored -6)
    assert sc == 8 * 4 - 6 and (rb, re_, qb, qe) == (0, 8, 0, 8)
    sc, rb, re_, qb, qe, cig = realign_ref.align(b"ACGTACGTACGT", b"ACGTAGGTACGT")
    assert [(int(w) & 15, int(w) >> 4) for w in cig] == [(7, 5), (8, 1), (7, 6)]
    assert realign_ref.to_read_cigar(cig).tolist() == [5 << 4, 1 << 4, 6 << 4]


def test_high_bytes_are_code_4():
    a = realign_ref.align(b"ACGTNACGT", b"ACGTNACGT")
    b = realign_ref.align(b"ACGT\xc8ACGT", b"ACGT\xffACGT")
    assert a[:5] == b[:5]


def test_window_is_region_plus_19():
    contig = bytes(range(65, 65 + 60))
    assert realign_ref.window(contig, 10, 20) == contig[10:40]
    assert realign_ref.window(contig, 40, 59) == contig[40:60]


def test_cli_realign_flag_parses_and_defaults_off():
    from pepper_thesis_amd import cli
    p = cli.polish_parser()
    a = p.parse_args(["-b", "x.bam", "-f", "x.fa", "-m", "m.pkl", "-o", "out"])
    assert a.realign is False
    a = p.parse_args(["-b", "x.bam", "-f", "x.fa", "-m", "m.pkl", "-o", "out", "--realign"])
    assert a.realign is True
