"""CPU: `polish --min_qual` without a device: the checker (tests/min_qual_ref.py) on hand-worked runs with the expected labels
written out, the option and its refusals, and a stub chain through the command: the VCF header line, the log line, and
byte-identical files with `--min_qual 0` and without the flag."""
import os
import re

import numpy as np
import pytest

import edits_ref as er
import min_qual_ref as mq
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, synth
from pepper_thesis_amd.polish import with_filtered


# ---- the checker on hand-worked runs --------------------------------------------------------------------------------------

def _one_chunk(draft: bytes, inserts=()):
    """one region at 0 in one chunk: a base row per draft byte, an insert row behind the positions of `inserts`, two padding
    rows -> (position, index, region, chunk_id, ref_start, ref_off, ref)"""
    pos, idx = [], []
    for p in range(len(draft)):
        pos.append(p); idx.append(0)
        if p in inserts:
            pos.append(p); idx.append(1)
    pos, idx = pos + [-1, -1], idx + [-1, -1]
    return np.array([pos]), np.array([idx]), [0], [0], [0], [0, len(draft)], np.frombuffer(draft, np.uint8)


def _lab(s: str):
    """'1234 0' -> labels; blanks are ignored"""
    return np.array([[int(c) for c in s.replace(" ", "")]], np.uint8)


def test_minimum_on_the_first_middle_and_last_record():
    #   position   0 1 2 3 4  5 6 7 8 9  10 11 12 13 14  15 16 17 18 19
    #   draft      A C G T A  C G T A C   G  T  A  C  G   T  A  C  G  T
    #   labels     1 3 4 1 1  2 4 1 2 2   3  1  2  3  3   4  2  3  3  4   pad pad
    #   run          a a a      b b b        c  c  c         d  d
    #   quality      5 . .      . 5 .        .  .  5         40 41            (.: 40)
    args = _one_chunk(b"ACGTACGTACGTACGTACGT")
    lab = _lab("1341 1241 2231 2334 2334 00")
    rq = np.full(lab.shape, 40, np.uint8)
    rq[0, [1, 7, 13, 17]] = 5, 5, 5, 41
    runs = mq.region_runs(lab, rq, *args)
    assert [(len(r.records), r.minimum, r.pinned) for r in runs] == [(3, 5, False)] * 3 + [(2, 40, False)]
    assert [[rec[0] for rec in r.records] for r in runs] == [[1, 2, 3], [6, 7, 8], [11, 12, 13], [16, 17]]
    for q in (0, 1, 5):                                 # nothing is below the threshold: the identity
        l, r, n, p, gone = mq.filter_low_qual(lab, rq, *args, q)
        assert np.array_equal(l, lab) and np.array_equal(r, rq) and (n, p, gone) == (0, 0, [])
    l, r, n, p, gone = mq.filter_low_qual(lab, rq, *args, 6)
    #                  position  0123 4567 8901 2345 6789
    assert l.tolist() == _lab("1234 1234 1234 1234 2334 00").tolist()       # a, b, c spell the draft again, whole; d stays
    assert r.tolist() == [[40, 0, 0, 0, 40, 40, 0, 0, 0, 40, 40, 0, 0, 0, 40, 40, 40, 41, 40, 40, 40, 40]]
    assert (n, p, len(gone)) == (9, 0, 3)
    assert mq.filter_low_qual(lab, rq, *args, 40)[2] == 9 and mq.filter_low_qual(lab, rq, *args, 41)[2] == 11
    l, r, n, p, gone = mq.filter_low_qual(lab, rq, *args, 94)
    assert l.tolist() == _lab("1234 1234 1234 1234 1234 00").tolist() and n == 11 and r[0, 16:18].tolist() == [0, 0]
    assert lab[0, 1] == 3 and rq[0, 1] == 5                                 # the inputs are never altered


def test_a_run_goes_whole_substitution_with_insert_and_two_deletions():
    #   position   0 1 2 3 4  5 5' 6 7 8  9 10 11 12 12' 13
    #   draft      A C G T A  C    G T A  C  G  T  A      C
    #   labels     1 2 3 4 1  4 2  3 4 1  0  0  4  1 3    2
    #   quality    . . . . .  30 3 . . .  20 2  .  . 50   .       (.: 60)
    args = _one_chunk(b"ACGTACGTACGTAC", inserts=(5, 12))
    lab = _lab("12341 42 341 00 4 13 2 00")
    rq = np.full(lab.shape, 60, np.uint8)
    rq[0, [5, 6, 10, 11, 14]] = 30, 3, 20, 2, 50
    runs = mq.region_runs(lab, rq, *args)
    assert [[(rec[0], rec[1], rec[2]) for rec in r.records] for r in runs] == [
        [(5, 0, er.SUB), (5, 1, er.INS)], [(9, 0, er.DEL), (10, 0, er.DEL)], [(12, 1, er.INS)]]
    assert [r.minimum for r in runs] == [3, 2, 50]
    # 3: only the deletions go, both of them, though one column alone is below: reverting one would leave another frameshift
    l, r, n, p, _ = mq.filter_low_qual(lab, rq, *args, 3)
    assert l.tolist() == _lab("12341 42 341 23 4 13 2 00").tolist() and (n, p) == (2, 0)
    assert r[0, 10:12].tolist() == [0, 0] and r[0, 5:7].tolist() == [30, 3]
    # 4: the substitution goes with its low insert: the base row spells C again, the insert row holds no base
    l, r, n, p, _ = mq.filter_low_qual(lab, rq, *args, 4)
    assert l.tolist() == _lab("12341 20 341 23 4 13 2 00").tolist() and (n, p) == (4, 0) and r[0, 5:7].tolist() == [0, 0]
    # 51: the lone insert too
    l, r, n, p, _ = mq.filter_low_qual(lab, rq, *args, 51)
    assert l.tolist() == _lab("12341 20 341 23 4 10 2 00").tolist() and (n, p) == (5, 0) and r[0, 14] == 0


def test_pinned_runs_stay_and_a_lower_case_draft_is_reverted():
    #   position   0 1 2 3 4  5 6 7 8 9  10 11 12 13 14  15 16 17
    #   draft      A C G T N  A C G T R   A  C  G  a  c   g  t  A
    #   labels     1 2 3 1 1  1 2 3 4 1   1  2  3  1  3   0  4  1
    #   quality    . . . 2 .  . . . . .   .  .  .  .  1   50 .  .      (.: 60)
    #   3 and 4: a substitution beside the N, which any label edits: one run, pinned. 9: the R alone, pinned.
    #   13: 'a' under label A is no edit. 14, 15: a substitution and a deletion over lower-case bytes.
    args = _one_chunk(b"ACGTNACGTRACGacgtA")
    lab = _lab("12311 12341 12313 041 00")
    rq = np.full(lab.shape, 60, np.uint8)
    rq[0, [3, 14, 15]] = 2, 1, 50
    runs = mq.region_runs(lab, rq, *args)
    assert [([rec[0] for rec in r.records], r.minimum, r.pinned) for r in runs] == [([3, 4], 2, True), ([9], 60, True),
                                                                                  ([14, 15], 1, False)]
    l, r, n, p, gone = mq.filter_low_qual(lab, rq, *args, 3)
    assert l.tolist() == _lab("12311 12341 12312 341 00").tolist()          # c and g come back as C and G; 3 and 4 stay
    assert (n, p, len(gone)) == (2, 2, 1) and r[0, [3, 4, 14, 15]].tolist() == [2, 60, 0, 0]
    l, r, n, p, gone = mq.filter_low_qual(lab, rq, *args, 94)
    assert l.tolist() == _lab("12311 12341 12312 341 00").tolist() and (n, p) == (2, 3)
    assert mq.filter_low_qual(lab, rq, *args, 1)[2:4] == (0, 0) and mq.filter_low_qual(lab, rq, *args, 2)[2:4] == (2, 0)


def test_runs_end_at_a_region_boundary_and_owners_follow_the_string_order():
    import min_qual_cases as mc
    lay = mc.Layout([(0, b"ACGT" * 3, {}), (0, b"ACGT" * 100, {})], L=40, O=10)
    assert lay.n == 1 + 13 and lay.chunk_id.tolist() == [0] + list(range(13))
    own = mq.owned_mask(lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, lay.position.shape)
    k9, k10, k4 = 1 + 9, 1 + 10, 1 + 4
    assert own[k9, 30:].all() and not own[k10, :10].any()                   # "9" is behind "10": the earlier chunk owns
    assert own[k4, :10].all() and not own[k4 - 1, 30:].any()                # the ordinary hand-off: the later chunk owns
    assert own.sum() == 12 + 400


# ---- the option ---------------------------------------------------------------------------------------------------------

BASE = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]


def test_min_qual_option_parses_on_both_entry_points(monkeypatch):
    assert cli.polish_parser().parse_args(BASE + ["--min_qual", "20"]).min_qual == 20
    assert cli.polish_parser().parse_args(BASE).min_qual == 0
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.min_qual) or 0)
    assert cli.main(["polish"] + BASE + ["--min_qual", "3"]) == 0 and cli.main(["polish"] + BASE) == 0
    assert pepper.main(["polish"] + BASE + ["--min_qual", "94"]) == 0
    assert seen == [3, 0, 94]
    args = pepper.parser().parse_args(["polish"] + BASE + ["--min_qual", "2", "--bf16", "--realign", "--gpu_decode", "--qualities",
                                                            "--edits", "--min_depth", "3"])
    assert args.min_qual == 2 and args.min_depth == 3 and args.edits and args.qualities
    with pytest.raises(SystemExit) as e:
        cli.polish_parser().parse_args(BASE + ["--min_qual", "high"])
    assert e.value.code == 2


def test_the_step_commands_do_not_take_the_flag():
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--min_qual", "20"])
        assert e.value.code == 2


def _no_chain(started):
    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    return open_chain


def _args(tmp_path, *more):
    return cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out")] + list(more))


@pytest.mark.parametrize("value", ["-1", "95", "1000"])
def test_values_outside_the_range_are_refused(tmp_path, capsys, value):
    started = []
    assert polish.run(_args(tmp_path, "--min_qual", value), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_qual" in err and value in err and "94" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_polish_min_qual_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    assert polish.run(_args(tmp_path, "--min_qual", "20", "-d_ids", "0,1"), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_qual runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))
    # --min_qual 0 is off: several devices start their ranks as ever (the inputs are checked first: none here)
    assert polish.run(_args(tmp_path, "--min_qual", "0", "-d_ids", "0,1"), open_chain=_no_chain(started)) == 1
    assert "--min_qual" not in capsys.readouterr().err


def test_vcf_header_names_the_threshold_once():
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [("c", 5, 6)], recs, min_qual=20)
    assert text.split("\n")[:7] == ["##fileformat=VCFv4.2", "##source=s", "##reference=r", "##contig=<ID=c,length=10>",
                                    "##pepper_no_reads=c:5-6", "##pepper_min_qual=20", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    assert text.count("pepper_min_qual") == 1
    both = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20).split("\n")
    assert both[4:6] == ["##pepper_min_depth=3", "##pepper_min_qual=20"]
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, 0, 0) == pe.vcf_text("s", "r", [("c", 10)], [], recs)
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 0) == pe.vcf_text("s", "r", [("c", 10)], [], recs, 3)
    assert "pepper_min_qual" not in pe.vcf_text("s", "r", [("c", 10)], [("c", 1, 4)], recs)


def test_result_carries_the_counts_beside_its_planes():
    res = polish.ChainResult(np.array([0, 2]), b"AC")
    assert res.filtered is None and res.masked is None
    got = with_filtered(res, (7, 1))
    assert got.filtered == (7, 1) and got.masked is None and tuple(got) == tuple(res) and got.region(0) == (b"AC", None, None)
    both = with_filtered(polish.with_masked(res, (3, 2)), (7, 1))
    assert (both.masked, both.filtered) == ((3, 2), (7, 1)) and tuple(both) == tuple(res)
    assert polish.with_masked(got, (3, 2)).filtered == (7, 1)
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    assert polish.Piece._fields == ("contig", "start", "index", "bases", "qual", "edits")
    T = polish._timers(None)
    for r in (res, got, both):
        polish._count_masked(T, r)
    assert (T["reverted_rows"], T["pinned_rows"], T["masked_rows"], T["unmaskable_rows"]) == (14, 2, 3, 2)


# ---- a stub chain through the command -----------------------------------------------------------------------------------

class _StubChain:
    """the chain's contract without a device: every region gives the upper-cased draft bases the stitch would keep, with a
    substitution at every 97th position, and the planes it was made for. It filters nothing: what the command itself adds
    for --min_qual is what these tests are about."""

    def __init__(self, qualities=False, edits=False, min_qual=0):
        self.qualities, self.edits, self.min_qual = qualities, edits, min_qual

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
        return with_filtered(res, (5, 2)) if self.min_qual else res

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two covered contigs with ACGT / acgt drafts"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("min_qual_cpu")
    rng = np.random.default_rng(53)
    contigs = [("ctg1", "".join(rng.choice(list("ACGTacgt"), size=3_300))), ("ctg2", "".join(rng.choice(list("ACGTacgt"), size=2_450)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    return tmp, dict(contigs)


def _run(t, name, flags, made):
    base = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "3", "-bs", "8", "--qualities", "--edits"]

    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append(kw)
        return _StubChain(**kw)
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / name)] + flags), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(str(t / name))):
        out[f] = bamio.bgzf_read_all(str(t / name / f)) if f.endswith(".vcf.gz") else open(str(t / name / f), "rb").read()
    return out


NAMES = ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa", "_pepper_polished.fq"]


def test_without_the_flag_nothing_changes(inputs, capsys):
    t, _ = inputs
    made = []
    plain, zero = _run(t, "plain", [], made), _run(t, "zero", ["--min_qual", "0"], made)
    assert made == [{"qualities": True, "edits": True}] * 2          # the keyword reaches the opener only when set
    assert list(plain) == NAMES and plain == zero
    assert b"pepper_min_qual" not in plain[NAMES[0]] and "MIN QUAL" not in capsys.readouterr().err


def test_header_line_and_log_line(inputs, capsys):
    t, drafts = inputs
    made = []
    plain, got = _run(t, "plain2", [], made), _run(t, "twenty", ["--min_qual", "20"], made)
    assert made[1] == {"qualities": True, "edits": True, "min_qual": 20} and list(got) == NAMES
    err = capsys.readouterr().err
    header, cols, recs = er.parse_vcf(got[NAMES[0]].decode())
    assert header[3:] == ["contig=<ID=ctg1,length=3300>", "contig=<ID=ctg2,length=2450>", "pepper_min_qual=20"]
    # the stub filters nothing, so everything else is the plain run's
    assert got[NAMES[2]] == plain[NAMES[2]] and got[NAMES[3]] == plain[NAMES[3]]
    assert [l for l in got[NAMES[0]].split(b"\n") if b"pepper_min_qual" not in l] == plain[NAMES[0]].split(b"\n")
    m = re.search(r"MIN QUAL 20: (\d+) CHUNK ROWS OF EDITS TAKEN BACK, (\d+) ROWS OF LOW RUNS KEPT \(DRAFT BYTE NOT ACGT\)", err)
    assert m and int(m.group(1)) * 2 == int(m.group(2)) * 5 and int(m.group(2)) >= 4      # (5, 2) per launch, two launches at least
    for c in drafts:
        mine = [r[1:] for r in recs if r[0] == c]
        assert len(mine) > 10 and all(r[3] >= 20 for r in mine)


def test_a_chain_made_for_another_threshold_is_refused_before_it_runs(inputs):
    t, _ = inputs

    class _Unused(_StubChain):
        def run(self, batch, windows=None):
            raise AssertionError("the chain may not run")
    for chain in (_Unused(), _Unused(min_qual=30)):
        with pytest.raises(ValueError) as e:
            polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), str(t / "other"), chain=chain, min_qual=20)
        assert "not made for this run" in str(e.value)
    assert os.listdir(str(t / "other")) == []
