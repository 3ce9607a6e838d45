"""CPU: `polish --vote`: the host checker (tests/vote_ref.py) on hand-computed rows, the option on both entry points and its
refusals, the VCF header line, the result's counters, and a stub chain through the command: no model is loaded and the chain
is opened with vote=True."""
import os
import re

import numpy as np
import pytest

import edits_ref as er
import min_qual_cases as mc
import vote_cases as vc
import vote_ref as vr
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe


# ---- the checker on hand-computed rows -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,ten,draft,label,n", vc.BASE_ROWS, ids=[r[0] for r in vc.BASE_ROWS])
def test_base_rows(name, ten, draft, label, n):
    got = vr.base_row(ten, vr.draft_label(draft[0]))
    assert got == (label, n), name


@pytest.mark.parametrize("name,ten,depth,label,n", vc.INSERT_ROWS, ids=[r[0] for r in vc.INSERT_ROWS])
def test_insert_rows(name, ten, depth, label, n):
    assert vr.insert_row(ten, depth) == (label, n), name


def test_draft_labels():
    assert [vr.draft_label(b) for b in b"ACGTacgt"] == [1, 2, 3, 4, 1, 2, 3, 4]
    assert [vr.draft_label(b) for b in b"NnRy-*@["] == [None] * 8


def test_a_base_row_does_not_look_at_its_depth_and_every_tie_pattern_is_listed():
    seen = set()
    for _, ten, draft, label, n in vc.BASE_ROWS:
        top = max(n[1:])
        seen.add((tuple(b for b in (1, 2, 3, 4) if n[b] == top and top > 0), vr.draft_label(draft[0]) in
                  [b for b in (1, 2, 3, 4) if n[b] == top]))
    ties = {t for t, _ in seen if len(t) >= 2}
    assert {(1, 2), (2, 4), (3, 4), (1, 2, 3), (2, 3, 4), (1, 2, 3, 4)} <= ties
    assert all((t, inside) in seen for t in ((1, 2), (1, 2, 3, 4), (2, 3, 4)) for inside in (True, False))


def test_whole_layout_counters_weights_and_padding():
    """one region of 70 columns with an insert row, L = 40, O = 10: three chunks, the last one padded"""
    L, O = 40, 10
    draft = bytearray(b"ACGT" * 17 + b"AC")
    draft[3], draft[20], draft[33] = ord("N"), ord("c"), ord("g")
    lay = mc.Layout([(0, bytes(draft), {7: 2})], L, O)
    counts = np.zeros(lay.position.shape + (10,), np.uint16)
    depth = np.zeros(lay.position.shape, np.uint16)
    for r, (p, x) in enumerate(lay.rows[0]):          # ten reads spell the draft everywhere, nothing is inserted
        if x == 0:
            dl = vr.draft_label(draft[p])
            vc.plant(lay, counts, depth, 0, r, vc.row(**{"acgt"[dl - 1]: 10}) if dl else vc.row(a=4, c=6))
        else:
            vc.plant(lay, counts, depth, 0, r, vc.row(), 10)
    lab, acc, changed, no_reads = vr.vote(counts, depth, *lay.args()[:4], lay.ref_start, lay.ref_off, lay.ref, O)
    assert (changed, no_reads) == (1, 0)                                  # the N column: C wins, and that is not the draft
    assert np.array_equal(lab, np.where(lay.position == 3, 2, lay.spelled()[0]))
    pad = lay.position < 0
    assert pad.any() and (lab[pad] == 0).all() and (acc[pad] == 0).all()
    # w(j) at its edges: 1 for j = O - 1 and j = L - O, 2 for j = O and j = L - O - 1, on the winner's plane
    for j, w in ((O - 1, 1.0), (O, 2.0), (L - O - 1, 2.0), (L - O, 1.0)):
        assert acc[0, j, lab[0, j]] == np.float32(w) and acc[0, j].sum() == np.float32(w), j
        assert vr.weight(j, L, O) == np.float32(w)
    assert acc[lay.where(0, 3)][0].tolist() == [0.0, np.float32(4) / np.float32(10), np.float32(6) / np.float32(10), 0.0, 0.0]   # (row 3 < O)
    # no reads: the draft where a label spells it (lower case too), label 0 over the N; all three count as rows without reads
    for p in (3, 20, 33, 50):
        vc.plant(lay, counts, depth, 0, lay.rows[0].index((p, 0)), vc.row())
    lab, acc, changed, no_reads = vr.vote(counts, depth, *lay.args()[:4], lay.ref_start, lay.ref_off, lay.ref, O)
    assert (changed, no_reads) == (len(lay.where(0, 3)[0]), sum(len(lay.where(0, lay.rows[0].index((p, 0)))[0]) for p in (3, 20, 33, 50)))
    assert lab[lay.where(0, 3)].tolist() == [0] * len(lay.where(0, 3)[0])
    assert [int(lab[lay.where(0, lay.rows[0].index((p, 0)))][0]) for p in (20, 33, 50)] == [2, 3, vr.draft_label(draft[50])]
    assert (acc[lay.where(0, lay.rows[0].index((20, 0)))] == 0).all()
    # an insert row most reads fill; its copies in two chunks agree
    r = lay.rows[0].index((7, 1))
    vc.plant(lay, counts, depth, 0, r, vc.row(t=7), 10)
    lab, acc, changed2, _ = vr.vote(counts, depth, *lay.args()[:4], lay.ref_start, lay.ref_off, lay.ref, O)
    assert lab[lay.where(0, r)].tolist() == [4] * len(lay.where(0, r)[0]) and changed2 == changed + len(lay.where(0, r)[0])
    # a base position outside the draft, and a broken chunk order
    pos = lay.position.copy()
    pos[1, 5] = 70
    with pytest.raises(vr.BadChunk) as e:
        vr.vote(counts, depth, pos, lay.index, lay.region, lay.chunk_id, lay.ref_start, lay.ref_off, lay.ref, O)
    assert e.value.chunk == 1
    with pytest.raises(vr.BadChunk) as e:
        vr.vote(counts, depth, lay.position, lay.index, lay.region, np.array([0, 2, 3], np.int32), lay.ref_start, lay.ref_off, lay.ref, O)
    assert e.value.chunk == 1


# ---- the option ---------------------------------------------------------------------------------------------------------

NO_MODEL = ["-b", "r", "-f", "f", "-o", "o"]


def test_vote_parses_without_a_model_on_both_entry_points(monkeypatch):
    a = cli.polish_parser().parse_args(NO_MODEL + ["--vote"])
    assert a.vote and a.model_path is None
    b = cli.polish_parser().parse_args(NO_MODEL + ["-m", "m"])
    assert not b.vote and b.model_path == "m"
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append((args.vote, args.model_path)) or 0)
    assert cli.main(["polish"] + NO_MODEL + ["--vote"]) == 0 and cli.main(["polish"] + NO_MODEL + ["-m", "m"]) == 0
    assert pepper.main(["polish"] + NO_MODEL + ["--vote"]) == 0
    assert seen == [(True, None), (False, "m"), (True, None)]
    args = pepper.parser().parse_args(["polish"] + NO_MODEL + ["--vote", "--realign", "--gpu_decode", "--qualities", "--edits",
                                                               "--evidence", "--min_depth", "3", "--min_qual", "20", "--min_support", "2", "-hp"])
    assert args.vote and args.min_support == 2 and args.use_hp_info and args.evidence


@pytest.mark.parametrize("entry", ["parser", "cli", "pepper"])
def test_neither_model_nor_vote_is_argparses_own_error(entry, capsys, monkeypatch, tmp_path):
    monkeypatch.setattr(polish, "run", lambda args: pytest.fail("the command may not start"))
    argv = ["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-o", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        if entry == "parser":
            cli.polish_parser().parse_args(argv)
        else:
            (cli if entry == "cli" else pepper).main(["polish"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "the following arguments are required: -m/--model_path" in err and "usage:" in err
    assert not os.path.exists(str(tmp_path / "out"))


def test_a_namespace_made_by_hand_is_refused_too(tmp_path, capsys):
    import argparse
    started = []
    ns = argparse.Namespace(bam="b", fasta="f", model_path=None, output_file=str(tmp_path / "out"), device_ids=None, threads=1)
    assert polish.run(ns, open_chain=_no_chain(started)) == 2
    assert "the following arguments are required: -m/--model_path" in capsys.readouterr().err and started == []


def test_the_step_commands_do_not_take_the_flag():
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--vote"])
        assert e.value.code == 2


def _no_chain(started):
    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    return open_chain


def _args(tmp_path, *more):
    return cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-o", str(tmp_path / "out")]
                                          + list(more))


@pytest.mark.parametrize("more,word", [(["-m", "some.pkl"], "-m"), (["--bf16"], "--bf16"), (["-m", "some.pkl", "--bf16"], "-m")])
def test_vote_with_a_model_or_bf16_is_refused(tmp_path, capsys, more, word):
    started = []
    assert polish.run(_args(tmp_path, "--vote", *more), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--vote takes no " + word in err and "no model is read" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_vote_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    assert polish.run(_args(tmp_path, "--vote", "-d_ids", "0,1"), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--vote runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))
    # one id is one device: that check passes (the inputs are checked next: none here, and no model file is looked for)
    assert polish.run(_args(tmp_path, "--vote", "-d_ids", "0"), open_chain=_no_chain(started)) == 1
    err = capsys.readouterr().err
    assert "CAN NOT LOCATE BAM FILE" in err and "MODEL" not in err


def test_vcf_header_line_is_the_first_of_the_pepper_lines():
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20, min_support=2, haplotype=1, consensus="vote").split("\n")
    assert text[4:10] == ["##pepper_consensus=vote", "##pepper_min_depth=3", "##pepper_min_qual=20", "##pepper_min_support=2",
                          "##pepper_haplotype=1", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    ev = pe.vcf_text("s", "r", [("c", 10)], [("c", 5, 6)], recs, evidence=True, consensus="vote").split("\n")
    at = ev.index("##pepper_consensus=vote")
    assert ev[at - 1].startswith("##INFO=") and ev[at + 1] == "##pepper_no_reads=c:5-6"
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs) == pe.vcf_text("s", "r", [("c", 10)], [], recs, consensus="")
    assert "pepper_consensus" not in pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20)


def test_result_carries_the_counts_beside_its_planes():
    res = polish.ChainResult(np.array([0, 2]), b"AC")
    assert res.voted is None
    got = polish.with_voted(res, (7, 1))
    assert got.voted == (7, 1) and got.masked is None and got.supported is None and tuple(got) == tuple(res)
    every = polish.with_supported(polish.with_filtered(polish.with_masked(got, (3, 2)), (5, 4)), (9, 8))
    assert (every.voted, every.masked, every.filtered, every.supported) == ((7, 1), (3, 2), (5, 4), (9, 8))
    assert polish.with_voted(every, (1, 1)).supported == (9, 8)
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    T = polish._timers(None)
    for r in (res, got, every):
        polish._count_masked(T, r)
    assert (T["voted_rows"], T["no_read_rows"], T["masked_rows"]) == (14, 2, 3)


# ---- a stub chain through the command -----------------------------------------------------------------------------------

class _StubChain:
    """the chain's contract without a device: every region gives the upper-cased draft bases the stitch would keep, with a
    substitution at every 97th position, and the planes it was made for. What the command itself adds for --vote is what
    these tests are about."""

    def __init__(self, qualities=False, edits=False, vote=False):
        self.qualities, self.edits, self.vote = qualities, edits, vote

    def run(self, batch, windows=None):
        out, quals, recs, roff, eoff = [], [], [], [0], [0]
        for g in range(batch.n_regions):
            a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
            draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1].decode()
            s = []
            for p in range(a + 201 if a > 0 else a, b + 1):
                d = draft[p - a].upper()
                if p % 97 == 5:
                    new = "ACGT"[("ACGT".index(d) + 1) % 4]
                    recs.append((p, 0, pe.KIND_SUB, ord(draft[p - a]), ord(new), 30 + p % 60))
                    d = new
                s.append(d)
                quals.append(30 + p % 60)
            out.append("".join(s).encode())
            roff.append(roff[-1] + len(s))
            eoff.append(len(recs))
        res = polish.ChainResult(np.asarray(roff, np.int64), b"".join(out), bytes(quals) if self.qualities else None)
        if self.edits:
            res = res._replace(edit_off=np.asarray(eoff, np.int64), edits=np.array(recs, pe.EDIT_DTYPE))
        return polish.with_voted(res, (5, 2)) if self.vote else res

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two covered contigs with ACGT / acgt drafts; no model file anywhere"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("vote_cpu")
    rng = np.random.default_rng(55)
    contigs = [("ctg1", "".join(rng.choice(list("ACGTacgt"), size=3_300))), ("ctg2", "".join(rng.choice(list("ACGTacgt"), size=2_450)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    return tmp, dict(contigs)


def test_the_command_opens_a_vote_chain_and_loads_no_model(inputs, capsys, monkeypatch):
    t, drafts = inputs
    monkeypatch.setattr(polish, "load_polish_model", lambda path: pytest.fail("no model may be loaded (%r)" % (path,)))
    made = []

    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append((state_dict, kw))
        return _StubChain(**kw)
    argv = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-t", "3", "-bs", "8", "--qualities", "--edits", "--vote", "-o", str(t / "out")]
    assert polish.run(cli.polish_parser().parse_args(argv), open_chain=open_chain) == 0
    assert made == [(None, {"qualities": True, "edits": True, "vote": True})]
    names = sorted(os.listdir(str(t / "out")))
    assert names == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa", "_pepper_polished.fq"]
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(str(t / "out" / names[0])).decode())
    assert header[3:] == ["contig=<ID=ctg1,length=3300>", "contig=<ID=ctg2,length=2450>", "pepper_consensus=vote"] and recs
    m = re.search(r"VOTE: (\d+) CHUNK ROWS WHERE THE READS' MAJORITY IS NOT THE DRAFT, (\d+) BASE ROWS WITHOUT READS", capsys.readouterr().err)
    assert m and int(m.group(1)) * 2 == int(m.group(2)) * 5 and int(m.group(2)) >= 4      # (5, 2) per launch, two launches at least


def test_a_chain_that_was_not_made_for_the_run_is_refused_before_it_runs(inputs):
    t, _ = inputs

    class _Unused(_StubChain):
        def run(self, batch, windows=None):
            raise AssertionError("the chain may not run")
    for chain, vote in ((_Unused(), True), (_Unused(vote=True), False)):
        with pytest.raises(ValueError) as e:
            polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), None, str(t / "other"), chain=chain, **({"vote": True} if vote else {}))
        assert "not made for this run" in str(e.value)
    assert os.listdir(str(t / "other")) == []
