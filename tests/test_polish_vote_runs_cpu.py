"""CPU: `polish --vote --runs`: the host checker of the run vote (tests/vote_runs_ref.py) on hand-worked cases, behind the host
checkers of the builder's planes and of the column vote; the flag on the parsers, its refusals, the VCF header lines, the
result's counters, and a stub chain through the command."""
import os
import re

import numpy as np
import pytest

import vote_runs_cases as rc
import vote_runs_ref as rr
from pepper_thesis_amd import bamio, cli, pepper, polish, polish_edits as pe
from test_polish_vote_cpu import _StubChain, _args, _no_chain, inputs  # noqa: F401  (the module's BAM and FASTA)

L, O = 64, 8


def _case(draft, s, n, lengths, anchors=None, start=100, extra=()):
    """reads over the whole draft that show lengths[i] letters for the run [s, s + n) -> host_chain's result and the batch"""
    b = draft[s]
    reads = [rc.read_over(draft, start, 0, len(draft), rc.run_edits(s, n, b, ln, None if anchors is None else anchors[i]),
                          is_reverse=bool(i % 2)) for i, ln in enumerate(lengths)]
    batch = rc.one_region(draft, reads + list(extra), start)
    return batch, rc.host_chain(batch, L, O)


def _runs(batch, lay, lab, acc, min_run=3):
    return rr.vote_runs(batch, lay.position, lay.index, lay.region, lay.chunk_id, lab, acc, O, min_run)


def test_a_wrong_deletion_in_a_correct_run():
    """A^8 is right; 9 reads show 8, 6 show 7, 5 show 6, deletions left-aligned: the first column is deleted in 11 of 20 and the
    column vote deletes it; the reads' most frequent length is 8"""
    rng = np.random.default_rng(1)
    draft = rc.draft_with_runs(rng, 90, {40: ("A", 8)})
    batch, (lay, counts, depth, lab, acc) = _case(draft, 40, 8, [8] * 9 + [7] * 6 + [6] * 5)
    voted = rc.spelled(lay, lab)
    assert voted == draft[:40] + "A" * 7 + draft[48:]                      # the column vote breaks the draft
    at = lay.where(0, lay.rows[0].index((140, 0)))
    c = counts[at][0]
    assert lab[at].tolist() == [0] and int(c[8]) + int(c[9]) == 11 and int(c[0]) + int(c[4]) == 9
    lab2, acc2, cnt, runs = _runs(batch, lay, lab, acc)
    assert cnt == [1, 0, -1, 0, 1, 0]
    (r,) = runs
    assert (r.s, r.n, r.b, r.S, r.V, r.L) == (140, 8, "A", 20, 20, 8) and r.h[6:9] == (5, 6, 9)
    assert rc.spelled(lay, lab2) == draft
    # the rows of the span carry 9 / 20 in the label's slot and nothing else; every other row is the column vote's
    span = (lay.position >= 140) & (lay.position <= 147)
    assert (lab2[span] == 1).all() and np.array_equal(lab2[~span], lab[~span]) and np.array_equal(acc2[~span], acc[~span])
    for k, j in zip(*np.nonzero(span)):
        w = np.float32(1 if j < O or j >= L - O else 2)
        assert acc2[k, j].tolist() == [0, w * (np.float32(9) / np.float32(20)), 0, 0, 0]
    assert lab.tolist() != lab2.tolist()


def test_a_missed_insertion():
    """the draft holds A^5 and the truth A^6; 12 of 20 reads show 6 with the inserted base at three anchors, 4 reads each: every
    insert row holds 4 reads for the base and 16 for nothing, so the column vote inserts nothing"""
    rng = np.random.default_rng(2)
    draft = rc.draft_with_runs(rng, 90, {50: ("A", 5)})
    anchors = [49] * 4 + [51] * 4 + [53] * 4 + [None] * 8
    batch, (lay, counts, depth, lab, acc) = _case(draft, 50, 5, [6] * 12 + [5] * 8, anchors)
    assert rc.spelled(lay, lab) == draft
    ins = (lay.index > 0) & (lay.position >= 0)
    assert sorted(set(zip(lay.position[ins].tolist(), lay.index[ins].tolist()))) == [(149, 1), (151, 1), (153, 1)]
    assert (counts[ins].sum(-1) == 4).all() and (depth[ins] == 20).all()
    lab2, acc2, cnt, runs = _runs(batch, lay, lab, acc)
    assert cnt == [1, 0, -1, 1, 1, 0] and (runs[0].S, runs[0].V, runs[0].L) == (20, 20, 6) and runs[0].h[5:7] == (8, 12)
    assert rc.spelled(lay, lab2) == draft[:50] + "A" * 6 + draft[55:]
    first = (lay.position == 149) & (lay.index == 1)
    assert (lab2[first] == 1).all() and (lab2[ins & ~first] == 0).all()
    assert np.array_equal(lab2[~ins], lab[~ins])


@pytest.mark.parametrize("lengths,want", [
    ([5] * 6 + [4] * 6 + [6] * 6, 5),              # n among the most frequent
    ([4] * 6 + [7] * 6 + [5] * 2, 4),              # else the closest to n
    ([4] * 6 + [6] * 6 + [5] * 2, 4),              # at the same distance the smaller
    ([6] * 6 + [7] * 6 + [3] * 6, 6),              # the closest, above n
    ([0] * 9 + [5] * 2, 0),                        # a run most reads delete altogether
])
def test_ties(lengths, want):
    rng = np.random.default_rng(3)
    draft = rc.draft_with_runs(rng, 80, {30: ("G", 5)})
    batch, (lay, counts, depth, lab, acc) = _case(draft, 30, 5, lengths)
    assert rr.winner([lengths.count(l) for l in range(64)], 5) == want
    lab2, _, cnt, runs = _runs(batch, lay, lab, acc)
    assert runs[0].L == want and cnt[:4] == [1, 0, -1, int(want != 5)]
    assert rc.spelled(lay, lab2) == draft[:30] + "G" * want + draft[35:]


def test_half_of_the_spanning_reads_is_not_a_majority():
    """10 pure reads of 20: 2 * V == S, undecided, and the column vote's rows stay; one more pure read decides"""
    rng = np.random.default_rng(4)
    draft = rc.draft_with_runs(rng, 80, {30: ("C", 6)})
    other = next(b for b in "ACGT" if b not in (draft[29], "C", draft[33]))

    def reads(n_pure):
        out = []
        for i in range(20):
            ed = rc.run_edits(30, 6, "C", 5) if i < n_pure else {32: ("sub", other)}
            out.append(rc.read_over(draft, 100, 0, 80, ed, is_reverse=bool(i % 2)))
        return out
    batch = rc.one_region(draft, reads(10), 100)
    lay, counts, depth, lab, acc = rc.host_chain(batch, L, O)
    lab2, acc2, cnt, runs = _runs(batch, lay, lab, acc)
    assert (runs[0].S, runs[0].V, runs[0].L) == (20, 10, None) and cnt == [0, 0, -1, 0, 1, 0]
    assert np.array_equal(lab2, lab) and np.array_equal(acc2, acc)
    batch = rc.one_region(draft, reads(11), 100)
    lay, counts, depth, lab, acc = rc.host_chain(batch, L, O)
    _, _, cnt, runs = _runs(batch, lay, lab, acc)
    assert (runs[0].S, runs[0].V, runs[0].L) == (20, 11, 5) and cnt[:4] == [1, 0, -1, 1]


def test_candidates():
    c = rr.candidates
    assert c(b"CAAAG", 3) == ([(1, 3, "A")], 1, 0)
    assert c(b"AAAG", 3) == ([], 0, 0) and c(b"CAAA", 3) == ([], 0, 0)        # a flank outside the draft
    assert c(b"CaAaG", 3) == ([(1, 3, "A")], 1, 0)                            # lower case is upper-cased
    assert c(b"CAANAAG", 2) == ([(1, 2, "A"), (4, 2, "A")], 2, 0)             # any other byte ends a run
    assert c(b"CAAATTTG", 3) == ([], 2, 2)                                    # adjacent: both skipped
    assert c(b"CAAATTG", 3) == ([(1, 3, "A")], 1, 0)                          # TT is no candidate at min_run 3 ...
    assert c(b"CAAATTG", 2) == ([], 2, 2)                                     # ... and is one at 2
    assert c(b"C" + b"A" * 48 + b"G", 3)[1:] == (1, 0) and c(b"C" + b"A" * 49 + b"G", 3) == ([], 0, 0)
    assert c(b"GAAACTTTG", 3) == ([(1, 3, "A"), (5, 3, "T")], 2, 0)           # a shared flank is not adjacency
    with pytest.raises(ValueError):
        rr.vote_runs(None, np.zeros((0, L)), np.zeros((0, L)), [], [], np.zeros((0, L)), None, O, 1)
    with pytest.raises(ValueError):
        rr.vote_runs(None, np.zeros((0, L)), np.zeros((0, L)), [], [], np.zeros((0, L)), None, O, 49)


# ---- the flag ---------------------------------------------------------------------------------------------------------------------

NO_MODEL = ["-b", "r", "-f", "f", "-o", "o"]


def test_runs_parses_with_and_without_min_run(monkeypatch):
    a = cli.polish_parser().parse_args(NO_MODEL + ["--vote", "--runs"])
    assert a.runs and a.min_run is None
    b = cli.polish_parser().parse_args(NO_MODEL + ["--vote", "--runs", "--min_run", "5"])
    assert b.runs and b.min_run == 5
    c = cli.polish_parser().parse_args(NO_MODEL + ["--vote"])
    assert not c.runs and c.min_run is None
    args = pepper.parser().parse_args(["polish"] + NO_MODEL + ["--vote", "--runs", "--min_run", "4", "--realign", "--gpu_decode",
                                                               "--qualities", "--edits", "--evidence", "--min_depth", "3",
                                                               "--min_qual", "20", "-hp"])
    assert args.runs and args.min_run == 4 and args.use_hp_info
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--runs"])
        assert e.value.code == 2


@pytest.mark.parametrize("more,words", [
    (["-m", "some.pkl", "--runs"], ["--runs needs --vote"]),
    (["--vote", "--runs", "-d_ids", "0,1"], ["--runs runs on one device", "0,1"]),
    (["--vote", "--runs", "--min_support", "2"], ["--runs takes no --min_support", "in its own column"]),
    (["--vote", "--runs", "--min_run", "1"], ["--min_run 1", "from 2 to 48"]),
    (["--vote", "--runs", "--min_run", "49"], ["--min_run 49", "from 2 to 48"]),
    (["--vote", "--min_run", "4"], ["--min_run needs --runs"]),
])
def test_refusals(tmp_path, capsys, monkeypatch, more, words):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    assert polish.run(_args(tmp_path, *more), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert err.startswith("ERROR: polish") and all(w in err for w in words), err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_vcf_header_lines():
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20, haplotype=1, consensus="vote+runs", min_run=3).split("\n")
    assert text[4:10] == ["##pepper_consensus=vote+runs", "##pepper_min_run=3", "##pepper_min_depth=3", "##pepper_min_qual=20",
                          "##pepper_haplotype=1", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, consensus="vote") == pe.vcf_text("s", "r", [("c", 10)], [], recs,
                                                                                          consensus="vote", min_run=0)
    assert "pepper_min_run" not in pe.vcf_text("s", "r", [("c", 10)], [], recs, consensus="vote")


def test_result_carries_the_run_counts():
    res = polish.ChainResult(np.array([0, 2]), b"AC")
    assert res.runs is None
    got = polish.with_runs(polish.with_voted(res, (7, 1)), (9, 6, 2, 1))
    assert got.runs == (9, 6, 2, 1) and got.voted == (7, 1) and tuple(got) == tuple(res)
    every = polish.with_supported(polish.with_filtered(polish.with_masked(got, (3, 2)), (5, 4)), (9, 8))
    assert every.runs == (9, 6, 2, 1) and polish.with_voted(every, (1, 1)).runs == (9, 6, 2, 1)
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    T = polish._timers(None)
    for r in (res, got, every):
        polish._count_masked(T, r)
    assert (T["runs_seen"], T["runs_decided"], T["runs_changed"], T["runs_skipped"]) == (18, 12, 4, 2)


class _RunsStub(_StubChain):
    def __init__(self, vote_runs=0, **kw):
        super().__init__(**kw)
        self.vote_runs = vote_runs

    def run(self, batch, windows=None):
        res = super().run(batch, windows)
        return polish.with_runs(res, (7, 5, 2, 1)) if self.vote_runs else res


def test_the_command_opens_a_run_vote_chain(inputs, capsys, monkeypatch):  # noqa: F811
    t, drafts = inputs
    monkeypatch.setattr(polish, "load_polish_model", lambda path: pytest.fail("no model may be loaded (%r)" % (path,)))
    made = []

    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append((state_dict, kw))
        return _RunsStub(**kw)
    for name, more, min_run in (("runs", [], 3), ("runs4", ["--min_run", "4"], 4)):
        argv = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-t", "3", "-bs", "8", "--edits", "--vote", "--runs", "-o", str(t / name)]
        assert polish.run(cli.polish_parser().parse_args(argv + more), open_chain=open_chain) == 0
        assert made[-1] == (None, {"edits": True, "vote": True, "vote_runs": min_run})
        text = bamio.bgzf_read_all(str(t / name / "_pepper_polished.edits.vcf.gz")).decode()
        header = [l[2:] for l in text.split("\n") if l.startswith("##pepper_")]
        assert header == ["pepper_consensus=vote+runs", "pepper_min_run=%d" % min_run]
        m = re.search(r"RUNS \(MIN RUN (\d+)\): (\d+) CANDIDATE RUNS SEEN, (\d+) DECIDED BY THEIR READS, (\d+) OF THEM WITH A LENGTH THAT "
                      r"IS NOT THE DRAFT'S, (\d+) SKIPPED AS ADJACENT", capsys.readouterr().err)
        assert m and int(m.group(1)) == min_run
        launches = int(m.group(2)) // 7
        assert launches >= 2 and [int(m.group(i)) for i in (2, 3, 4, 5)] == [7 * launches, 5 * launches, 2 * launches, launches]
    # a chain made for another min_run, or for none, is refused before it runs
    for chain, kw in ((_RunsStub(vote=True), {"vote_runs": 3}), (_RunsStub(vote=True, vote_runs=4), {"vote_runs": 3}),
                      (_RunsStub(vote=True, vote_runs=3), {})):
        with pytest.raises(ValueError) as e:
            polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), None, str(t / "other_runs"), chain=chain, vote=True, **kw)
        assert "not made for this run" in str(e.value)


def test_a_chain_with_runs_needs_the_vote_and_no_support_filter():
    """refused by the chain's constructor before it touches its context"""
    for kw in (dict(vote_runs=3), dict(vote=True, vote_runs=3, min_support=2)):
        with pytest.raises(ValueError):
            polish._DeviceChain(None, **kw)
