"""CPU: `polish --min_support` without a device: the checker (tests/min_support_ref.py) on hand-worked counts rows and runs with
the expected labels written out, the option and its refusals, and a stub chain through the command: the keyword, the VCF
header line, the log line, and byte-identical files with `--min_support 0` and without the flag."""
import os
import re

import numpy as np
import pytest

import edits_ref as er
import min_qual_cases as mc
import min_support_ref as ms
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, synth
from pepper_thesis_amd.polish import with_supported

A, C_, G, T = (ord(c) for c in "ACGT")


# ---- the support of one column, from a written-out counts row --------------------------------------------------------------

#        reverse strand    forward strand   other / deleted
#        A   C   G   T     A   C   G   T    rev  fwd
ROW = [  3,  0, 11,  1,    2,  0,  7, 40,    5,   6]


def test_support_of_a_substitution_a_deletion_and_an_inserted_base():
    assert ms.support_of(er.SUB, A, G, ROW, 80) == 11 + 7           # to G: c[2] + c[6]
    assert ms.support_of(er.SUB, ord("a"), T, ROW, 80) == 1 + 40    # to T: c[3] + c[7]; the draft byte plays no part
    assert ms.support_of(er.DEL, G, 0, ROW, 80) == 5 + 6            # c[8] + c[9]
    assert ms.support_of(er.INS, 0, A, ROW, 80) == 3 + 2            # of the insert row's own counts: c[0] + c[4]
    assert ms.support_of(er.INS, 0, A, ROW, 0) == 5                 # the depth plays no part


def test_a_base_no_read_holds_has_support_0_whatever_else_the_reads_show():
    assert ms.support_of(er.SUB, A, C_, ROW, 80) == 0               # 40 forward reads show T, none shows C
    assert ms.support_of(er.INS, 0, C_, ROW, 80) == 0


def test_support_on_one_strand_counts_fully_and_the_sum_is_not_clamped():
    assert ms.support_of(er.SUB, A, T, [0, 0, 0, 0, 0, 0, 0, 9, 0, 0], 9) == 9
    assert ms.support_of(er.DEL, A, 0, [0] * 8 + [4, 0], 4) == 4
    assert ms.support_of(er.SUB, A, T, [0, 0, 0, 65535, 0, 0, 0, 65535, 0, 0], 65535) == 131070


# ---- the checker on hand-worked runs ---------------------------------------------------------------------------------------

def _one_chunk(draft: bytes, inserts=()):
    pos, idx = [], []
    for p in range(len(draft)):
        pos.append(p); idx.append(0)
        if p in inserts:
            pos.append(p); idx.append(1)
    pos, idx = pos + [-1, -1], idx + [-1, -1]
    return np.array([pos]), np.array([idx]), [0], [0], [0], [0, len(draft)], np.frombuffer(draft, np.uint8)


def _lab(s: str):
    return np.array([[int(c) for c in s.replace(" ", "")]], np.uint8)


def _counts(lab, fwd, rev=None):
    """a counts plane in which the reads that spell each row's own label are fwd[j] forward and rev[j] reverse reads (label
    0: in the deleted planes), and 40 forward reads hold the next base round"""
    n = lab.shape[1]
    c = np.zeros((1, n, 10), np.uint16)
    rev = [0] * n if rev is None else rev
    for j in range(n):
        b = int(lab[0, j])
        if b == 0:
            c[0, j, 9], c[0, j, 8] = fwd[j], rev[j]
        else:
            c[0, j, 4 + b - 1], c[0, j, b - 1] = fwd[j], rev[j]
            c[0, j, 4 + b % 4] = 40
    return c


def test_five_records_whose_minimum_is_on_the_third_column():
    #   position   0 1 2 3 4  5 6 7 8 9  10 11
    #   draft      A C G T A  C G T A C   G  T
    #   labels     1 2 4 1 2  0 4 4 1 1   3  4    pad pad
    #   run            a a a  a a     b
    #   support        9 9 2  9 9     1             (fwd + rev)
    args = _one_chunk(b"ACGTACGTACGT")
    lab = _lab("1241 2044 11 34 00")
    fwd = [7] * 14
    rev = [2] * 14
    fwd[4], rev[4] = 2, 0
    fwd[9], rev[9] = 0, 1
    counts, depth = _counts(lab, fwd, rev), np.full(lab.shape, 50, np.uint16)
    rq = np.full(lab.shape, 60, np.uint8)
    runs = ms.region_runs(lab, counts, depth, *args)
    assert [[rec[0] for rec in r.records] for r in runs] == [[2, 3, 4, 5, 6], [9]]
    assert [(r.supports, r.minimum, r.pinned) for r in runs] == [((9, 9, 2, 9, 9), 2, False), ((1,), 1, False)]
    assert [rec[2] for rec in runs[0].records] == [er.SUB, er.SUB, er.SUB, er.DEL, er.SUB]
    for k in (0, 1):                                               # the identity
        l, q, n, p, gone = ms.filter_low_support(lab, rq, counts, depth, *args, k)
        assert np.array_equal(l, lab) and np.array_equal(q, rq) and (n, p, gone) == (0, 0, [])
    l, q, n, p, gone = ms.filter_low_support(lab, rq, counts, depth, *args, 2)
    assert l.tolist() == _lab("1241 2044 12 34 00").tolist() and (n, p, len(gone)) == (1, 0, 1) and q[0, 9] == 0
    l, q, n, p, gone = ms.filter_low_support(lab, rq, counts, depth, *args, 3)       # run a goes whole for its third column
    assert l.tolist() == _lab("1234 1234 12 34 00").tolist() and (n, p, len(gone)) == (6, 0, 2)
    assert q.tolist() == [[60, 60, 0, 0, 0, 0, 0, 60, 60, 0, 60, 60, 60, 60]]
    l, q, n, p, gone = ms.filter_low_support(lab, None, counts, depth, *args, 65535)  # without a quality plane
    assert l.tolist() == _lab("1234 1234 12 34 00").tolist() and q is None and n == 6
    assert lab[0, 2] == 4 and rq[0, 2] == 60                       # the inputs are never altered


def test_an_inserted_base_is_judged_by_its_own_row():
    #   position   0 1 1' 2 3
    #   draft      A C    G T
    #   labels     1 2 3  3 4     pad pad            an inserted G behind position 1
    args = _one_chunk(b"ACGT", inserts=(1,))
    lab = _lab("12334 00")
    counts = np.zeros((1, 7, 10), np.uint16)
    counts[0, 1, [1, 5]] = 20, 20                                  # the anchor: 40 reads show C; nobody asks
    counts[0, 2, 6] = 3                                            # the insert row: 3 forward reads hold G
    counts[0, 2, 7] = 30                                           # and 30 hold T
    depth = np.full(lab.shape, 40, np.uint16)
    runs = ms.region_runs(lab, counts, depth, *args)
    assert [(r.records[0][:3], r.supports) for r in runs] == [((1, 1, er.INS), (3,))]
    assert ms.filter_low_support(lab, None, counts, depth, *args, 3)[2] == 0
    l, _, n, p, _ = ms.filter_low_support(lab, None, counts, depth, *args, 4)
    assert l.tolist() == _lab("12034 00").tolist() and (n, p) == (1, 0)


def test_a_pinned_run_stays_and_is_counted():
    #   position   0 1 2 3 4  5 6 7
    #   draft      A C N T A  c G T
    #   labels     1 3 1 4 1  0 3 4   pad pad      1 and 2: a substitution beside the N, which any label edits: one run, pinned
    args = _one_chunk(b"ACNTAcGT")
    lab = _lab("13141 034 00")
    counts = _counts(lab, [0] * 10)                                # no read spells any label
    depth = np.full(lab.shape, 40, np.uint16)
    rq = np.full(lab.shape, 33, np.uint8)
    runs = ms.region_runs(lab, counts, depth, *args)
    assert [([rec[0] for rec in r.records], r.minimum, r.pinned) for r in runs] == [([1, 2], 0, True), ([5], 0, False)]
    l, q, n, p, gone = ms.filter_low_support(lab, rq, counts, depth, *args, 1)
    assert l.tolist() == _lab("13141 234 00").tolist() and (n, p, len(gone)) == (1, 2, 1)   # the deleted c comes back as C
    assert q[0].tolist() == [33] * 5 + [0] + [33] * 4


def test_two_regions_meeting_at_a_boundary_are_two_runs_and_a_duplicate_is_untouched():
    lay = mc.Layout([(0, b"ACGT" * 15, {}), (0, b"ACGT" * 10, {})], L=40, O=10)
    assert lay.n == 2 + 1 and lay.region.tolist() == [0, 0, 1]
    lab, _ = lay.spelled()
    rq = np.full(lab.shape, 60, np.uint8)
    for g, r in ((0, 58), (0, 59), (1, 0), (1, 1), (0, 33)):
        lay.plant(lab, rq, g, r, "sub", 60)
    # region 0's last two positions and region 1's first two: adjacent rows of the batch, one VCF block where the regions
    # abut, but two runs. Row 33 of region 0 is in chunks 0 and 1; chunk 1 owns it.
    counts = np.zeros(lab.shape + (10,), np.uint16)
    counts[..., 4:8] = 6                                           # six forward reads for every base: support 6 everywhere
    for at in (lay.where(0, 59), lay.where(0, 33)):
        counts[at] = 0                                             # but nobody behind two of the edits
    depth = np.full(lab.shape, 24, np.uint16)
    runs = ms.region_runs(lab, counts, depth, *lay.args())
    assert [(r.region, [rec[0] for rec in r.records], r.minimum) for r in runs] == [(0, [33], 0), (0, [58, 59], 0), (1, [0, 1], 6)]
    assert runs[0].rows == ((1, 3),)
    l, q, n, p, gone = ms.filter_low_support(lab, rq, counts, depth, *lay.args(), 1)
    assert (n, p, len(gone)) == (3, 0, 2)
    spelled = lay.spelled()[0]
    assert l[1, 3] == spelled[1, 3] and q[1, 3] == 0               # the owner spells the draft again ...
    assert l[0, 33] == lab[0, 33] != spelled[0, 33] and q[0, 33] == 60   # ... its copy in chunk 0, which owns nothing, is as it was
    assert np.array_equal(l[2], lab[2])                            # region 1's run is judged apart and stays
    assert ms.filter_low_support(lab, rq, counts, depth, *lay.args(), 7)[2] == 5


# ---- the option ---------------------------------------------------------------------------------------------------------

BASE = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]


def test_min_support_option_parses_on_both_entry_points(monkeypatch):
    assert cli.polish_parser().parse_args(BASE + ["--min_support", "3"]).min_support == 3
    assert cli.polish_parser().parse_args(BASE).min_support == 0
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.min_support) or 0)
    assert cli.main(["polish"] + BASE + ["--min_support", "1"]) == 0 and cli.main(["polish"] + BASE) == 0
    assert pepper.main(["polish"] + BASE + ["--min_support", "65535"]) == 0
    assert seen == [1, 0, 65535]
    args = pepper.parser().parse_args(["polish"] + BASE + ["--min_support", "2", "--bf16", "--realign", "--gpu_decode", "--qualities",
                                                            "--edits", "--evidence", "--min_depth", "3", "--min_qual", "20", "-hp"])
    assert args.min_support == 2 and args.min_depth == 3 and args.min_qual == 20 and args.evidence and args.use_hp_info
    with pytest.raises(SystemExit) as e:
        cli.polish_parser().parse_args(BASE + ["--min_support", "many"])
    assert e.value.code == 2


def test_the_step_commands_do_not_take_the_flag():
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--min_support", "2"])
        assert e.value.code == 2


def _no_chain(started):
    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    return open_chain


def _args(tmp_path, *more):
    return cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out")] + list(more))


@pytest.mark.parametrize("value", ["-1", "65536"])
def test_values_outside_the_range_are_refused(tmp_path, capsys, value):
    started = []
    assert polish.run(_args(tmp_path, "--min_support", value), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_support" in err and value in err and "65535" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_polish_min_support_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    assert polish.run(_args(tmp_path, "--min_support", "2", "-d_ids", "0,1"), open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_support runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))
    # --min_support 0 is off: several devices pass that check (the inputs are checked next: none here)
    assert polish.run(_args(tmp_path, "--min_support", "0", "-d_ids", "0,1"), open_chain=_no_chain(started)) == 1
    assert "--min_support" not in capsys.readouterr().err


def test_vcf_header_lines_stand_in_order():
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20, min_support=2)
    assert text.split("\n")[:8] == ["##fileformat=VCFv4.2", "##source=s", "##reference=r", "##contig=<ID=c,length=10>",
                                    "##pepper_min_depth=3", "##pepper_min_qual=20", "##pepper_min_support=2",
                                    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    assert text.count("pepper_min_support") == 1
    hp = pe.vcf_text("s", "r", [("c", 10)], [("c", 5, 6)], recs, haplotype=2, min_support=1).split("\n")
    assert hp[4:7] == ["##pepper_no_reads=c:5-6", "##pepper_min_support=1", "##pepper_haplotype=2"]
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, min_support=0) == pe.vcf_text("s", "r", [("c", 10)], [], recs)
    assert "pepper_min_support" not in pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20)


def test_result_carries_the_counts_beside_its_planes():
    res = polish.ChainResult(np.array([0, 2]), b"AC")
    assert res.supported is None
    got = with_supported(res, (7, 1))
    assert got.supported == (7, 1) and got.masked is None and got.filtered is None and tuple(got) == tuple(res)
    assert got.region(0) == (b"AC", None, None)
    every = with_supported(polish.with_filtered(polish.with_masked(res, (3, 2)), (5, 4)), (7, 1))
    assert (every.masked, every.filtered, every.supported) == ((3, 2), (5, 4), (7, 1)) and tuple(every) == tuple(res)
    assert polish.with_masked(got, (3, 2)).supported == (7, 1) and polish.with_filtered(got, (3, 2)).supported == (7, 1)
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    T = polish._timers(None)
    for r in (res, got, every):
        polish._count_masked(T, r)
    assert (T["unsupported_rows"], T["pinned_unsupported_rows"], T["reverted_rows"], T["pinned_rows"], T["masked_rows"]) == (14, 2, 5, 4, 3)


# ---- a stub chain through the command -----------------------------------------------------------------------------------

class _StubChain:
    """the chain's contract without a device: every region gives the upper-cased draft bases the stitch would keep, with a
    substitution at every 97th position, and the planes it was made for. It filters nothing: what the command itself adds
    for --min_support is what these tests are about."""

    def __init__(self, qualities=False, edits=False, min_support=0):
        self.qualities, self.edits, self.min_support = qualities, edits, min_support

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
        return with_supported(res, (5, 2)) if self.min_support else res

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two covered contigs with ACGT / acgt drafts"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("min_support_cpu")
    rng = np.random.default_rng(54)
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
    plain, zero = _run(t, "plain", [], made), _run(t, "zero", ["--min_support", "0"], made)
    assert made == [{"qualities": True, "edits": True}] * 2          # exactly today's keywords: the new one only when set
    assert list(plain) == NAMES and plain == zero
    assert b"pepper_min_support" not in plain[NAMES[0]] and "MIN SUPPORT" not in capsys.readouterr().err


def test_header_line_and_log_line(inputs, capsys):
    t, drafts = inputs
    made = []
    plain, got = _run(t, "plain2", [], made), _run(t, "two", ["--min_support", "2"], made)
    assert made[1] == {"qualities": True, "edits": True, "min_support": 2} and list(got) == NAMES
    err = capsys.readouterr().err
    header, cols, recs = er.parse_vcf(got[NAMES[0]].decode())
    assert header[3:] == ["contig=<ID=ctg1,length=3300>", "contig=<ID=ctg2,length=2450>", "pepper_min_support=2"]
    # the stub filters nothing, so everything else is the plain run's
    assert got[NAMES[2]] == plain[NAMES[2]] and got[NAMES[3]] == plain[NAMES[3]]
    assert [l for l in got[NAMES[0]].split(b"\n") if b"pepper_min_support" not in l] == plain[NAMES[0]].split(b"\n")
    m = re.search(r"MIN SUPPORT 2: (\d+) CHUNK ROWS OF EDITS TAKEN BACK, (\d+) ROWS OF WEAK RUNS KEPT \(DRAFT BYTE NOT ACGT\)", err)
    assert m and int(m.group(1)) * 2 == int(m.group(2)) * 5 and int(m.group(2)) >= 4      # (5, 2) per launch, two launches at least


def test_a_chain_made_for_another_minimum_is_refused_before_it_runs(inputs):
    t, _ = inputs

    class _Unused(_StubChain):
        def run(self, batch, windows=None):
            raise AssertionError("the chain may not run")
    for chain in (_Unused(), _Unused(min_support=3)):
        with pytest.raises(ValueError) as e:
            polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), str(t / "other"), chain=chain, min_support=2)
        assert "not made for this run" in str(e.value)
    assert os.listdir(str(t / "other")) == []
