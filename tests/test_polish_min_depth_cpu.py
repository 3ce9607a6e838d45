"""CPU: `polish --min_depth` without a device: the checker (tests/depth_ref.py) on hand-worked cases, the option and its
refusals, and a stub chain through the command: read-free regions and a read-free contig filled from the draft, the VCF
header, and byte-identical files without the flag."""
import os

import numpy as np
import pytest

import depth_ref as dr
import edits_ref as er
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, polish_summary, synth
from pepper_thesis_amd.batch import Read, Region, pack_regions


# ---- the checker on hand-worked cases -------------------------------------------------------------------------------------

def test_depth_of_hand_worked_reads():
    #  position           10 11 12 13 14 15 16 17 18 19
    #  a  10  3M2D2M        M  M  M  D  D  M  M
    #  b   8  4M3I3N2M      M  M  N  N  N  M  M            two bases before the region; the insert hangs on 11
    #  c  16  1M1P9M                          M  P  M  M   P takes a position; the read runs past the region's end
    #  d  10  10M, mapping quality 0: not counted
    #  e   5  3S5M2D1M      D  D  M                        soft clip, five bases before the region
    reads = [Read.make(10, "3M2D2M", "ACGTA"), Read.make(8, "4M3I3N2M", "ACGTTTTAC"), Read.make(16, "1M1P9M", "A" * 10),
             Read.make(10, "10M", "A" * 10, mapq=0), Read.make(5, "3S5M2D1M", "TTTACGTAC"), ]
    b = pack_regions([Region(10, 19, b"ACGTNacgtA", reads)])
    #                                   10 11 12 13 14 15 16 17 18 19
    assert dr.region_depth(b, 0).tolist() == [3, 3, 3, 2, 2, 2, 3, 1, 1, 1]
    # a column no read covers, and one only deletions cover
    b = pack_regions([Region(0, 7, b"ACGTACGT", [Read.make(0, "2M", "AC"), Read.make(1, "1M3D1M", "CC"), Read.make(1, "1M3D1M", "CC")])])
    assert dr.region_depth(b, 0).tolist() == [1, 3, 2, 2, 2, 2, 0, 0]
    pos = np.array([[0, 1, 1, 2, 6, 7, -1, -1]])
    idx = np.array([[0, 0, 1, 0, 0, 0, -1, -1]])
    assert dr.row_depth(b, pos, idx, [0]).tolist() == [[1, 3, 3, 2, 0, 0, 0, 0]]     # the insert row takes its anchor's, padding 0


def test_mask_rule_on_hand_worked_rows():
    #        region 0 starts at 100 with draft "aCNTr", region 1 at 7 with "GGG"
    ref = np.frombuffer(b"aCNTrGGG", np.uint8)
    ref_off, ref_start = [0, 5, 8], [100, 7]
    pos = np.array([[100, 101, 101, 102, 103, 104, -1], [7, 8, 8, 8, 9, -1, -1]])
    idx = np.array([[0, 0, 1, 0, 0, 0, -1], [0, 0, 1, 2, 0, -1, -1]])
    depth = np.array([[0, 2, 2, 1, 3, 1, 0], [2, 1, 1, 1, 9, 0, 0]], np.uint16)
    lab = np.array([[3, 0, 4, 1, 255, 2, 4], [0, 4, 3, 0, 255, 1, 2]], np.uint8)
    rq = np.array([[10, 20, 30, 40, 50, 60, 70], [11, 21, 31, 41, 51, 61, 71]], np.uint8)
    args = (pos, idx, [0, 1], ref_start, ref_off, ref)
    # min_depth 0 is the identity; the inputs are never altered
    l0, q0, m, u = dr.mask(lab, rq, depth, *args, 0)
    assert np.array_equal(l0, lab) and np.array_equal(q0, rq) and (m, u) == (0, 0)
    # 2: a column no read covers (depth 0 over 'a' -> A), an N and an IUPAC r that cannot be spelled (kept and counted), a label
    # 255 above the threshold (copied), an insert behind a thin column (-> no base), padding untouched
    l2, q2, m, u = dr.mask(lab, rq, depth, *args, 2)
    assert l2.tolist() == [[1, 0, 4, 1, 255, 2, 4], [0, 3, 0, 0, 255, 1, 2]]
    assert q2.tolist() == [[0, 20, 30, 40, 50, 60, 70], [11, 0, 0, 0, 51, 61, 71]]
    assert (m, u) == (4, 2)
    # 3: the deletion label over C is replaced by C too, and its insert row goes
    l3, q3, m, u = dr.mask(lab, None, depth, *args, 3)
    assert q3 is None and l3.tolist() == [[1, 2, 0, 1, 255, 2, 4], [3, 3, 0, 0, 255, 1, 2]] and (m, u) == (7, 2)
    # 65535: every row that is no padding, the poisoned labels included
    l9, _, m, u = dr.mask(lab, rq, depth, *args, 65535)
    assert l9.tolist() == [[1, 2, 0, 1, 4, 2, 4], [3, 3, 0, 0, 3, 1, 2]] and (m, u) == (9, 2)
    assert lab[0, 0] == 3 and rq[0, 0] == 10


# ---- the option ---------------------------------------------------------------------------------------------------------

BASE = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]


def test_min_depth_option_parses_on_both_entry_points(monkeypatch):
    assert cli.polish_parser().parse_args(BASE + ["--min_depth", "4"]).min_depth == 4
    assert cli.polish_parser().parse_args(BASE).min_depth == 0
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.min_depth) or 0)
    assert cli.main(["polish"] + BASE + ["--min_depth", "3"]) == 0 and cli.main(["polish"] + BASE) == 0
    assert pepper.main(["polish"] + BASE + ["--min_depth", "65535"]) == 0
    assert seen == [3, 0, 65535]
    ap = pepper.parser()
    args = ap.parse_args(["polish"] + BASE + ["--min_depth", "2", "--bf16", "--realign", "--gpu_decode", "--qualities", "--edits"])
    assert args.min_depth == 2 and args.edits and args.qualities
    with pytest.raises(SystemExit) as e:
        cli.polish_parser().parse_args(BASE + ["--min_depth", "few"])
    assert e.value.code == 2


def _no_chain(started):
    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    return open_chain


@pytest.mark.parametrize("value", ["-1", "65536", "1000000"])
def test_values_outside_the_range_are_refused(tmp_path, capsys, value):
    started = []
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "--min_depth", value])
    assert polish.run(args, open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_depth" in err and value in err and "65535" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_polish_min_depth_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "--min_depth", "2", "-d_ids", "0,1"])
    assert polish.run(args, open_chain=_no_chain(started)) == 2
    err = capsys.readouterr().err
    assert "--min_depth runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))
    # --min_depth 0 is off: several devices start their ranks as ever (the inputs are checked first: none here)
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "--min_depth", "0", "-d_ids", "0,1"])
    assert polish.run(args, open_chain=_no_chain(started)) == 1 and "--min_depth" not in capsys.readouterr().err


def test_vcf_header_names_the_threshold_once():
    recs = {"c": [pe.VcfRecord(2, "C", "T", None)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3)
    assert text.split("\n")[:5] == ["##fileformat=VCFv4.2", "##source=s", "##reference=r", "##contig=<ID=c,length=10>",
                                    "##pepper_min_depth=3"]
    assert text.count("pepper_min_depth") == 1 and "pepper_no_reads" not in text
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, 0) == pe.vcf_text("s", "r", [("c", 10)], [], recs)
    assert "pepper_min_depth" not in pe.vcf_text("s", "r", [("c", 10)], [("c", 1, 4)], recs)


def test_result_carries_the_counts_beside_its_planes():
    res = polish.ChainResult(np.array([0, 2]), b"AC")
    assert res.masked is None
    got = polish.with_masked(res, (7, 1))
    assert got.masked == (7, 1) and tuple(got) == tuple(res) and got.region(0) == (b"AC", None, None)
    T = polish._timers(None)
    polish._count_masked(T, res)
    polish._count_masked(T, got)
    polish._count_masked(T, got)
    assert (T["masked_rows"], T["unmaskable_rows"]) == (14, 2)


# ---- a stub chain through the command -----------------------------------------------------------------------------------

class _StubChain:
    """the chain's contract without a device: every region gives the upper-cased draft bases the stitch would keep, with a
    substitution at every 97th position whose draft byte is a base, and the planes it was made for. It looks at no depth: what
    the command itself adds for --min_depth is what these tests are about."""

    def __init__(self, qualities=False, edits=False, min_depth=0):
        self.qualities, self.edits, self.min_depth = qualities, edits, min_depth

    def run(self, batch, windows=None):
        out, quals, recs, roff, eoff = [], [], [], [0], [0]
        for g in range(batch.n_regions):
            a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
            draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1].decode()
            s = []
            for p in range(a + 201 if a > 0 else a, b + 1):
                d = draft[p - a].upper()
                if p % 97 == 5 and d in "ACGT":
                    new = "ACGT"[("ACGT".index(d) + 1) % 4]
                    recs.append((p, 0, pe.KIND_SUB, ord(draft[p - a]), ord(new), p % 60))
                    d = new
                s.append(d)
                quals.append(p % 60)
            out.append("".join(s).encode())
            roff.append(roff[-1] + len(s))
            eoff.append(len(recs))
        res = polish.ChainResult(np.asarray(roff, np.int64), b"".join(out), bytes(quals) if self.qualities else None)
        if self.edits:
            res = res._replace(edit_off=np.asarray(eoff, np.int64), edits=np.array(recs, pe.EDIT_DTYPE))
        return polish.with_masked(res, (3, 1)) if self.min_depth else res

    def close(self):
        pass


GAP = (2_300, 5_900)      # no read of ctg2 touches these positions: two regions in a row get no reads


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """ctg2 with a read-free stretch longer than a region, ctg10 covered, ctg30 without a read; drafts with lower-case, N and
    IUPAC bytes"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("min_depth_cpu")
    rng = np.random.default_rng(31)
    letters, p = list("ACGTacgtNRy"), [.2, .2, .2, .2, .04, .04, .04, .04, .02, .01, .01]
    contigs = [("ctg2", "".join(rng.choice(letters, size=9_500, p=p))), ("ctg10", "".join(rng.choice(letters, size=3_300, p=p))),
               ("ctg30", "".join(rng.choice(letters, size=2_450, p=p)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs[:2]):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
    recs = [r for r in recs if r["tid"] != 0 or r["pos"] + bw.ref_len(r["cigar"]) <= GAP[0] or r["pos"] > GAP[1]]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    return tmp, dict(contigs)


def _open(made):
    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append(kw)
        return _StubChain(**kw)
    return open_chain


def _run(t, name, flags, made):
    base = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "3", "-bs", "8", "--qualities", "--edits"]
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / name)] + flags), open_chain=_open(made)) == 0
    out = {}
    for f in sorted(os.listdir(str(t / name))):
        raw = open(str(t / name / f), "rb").read()
        out[f] = bamio.bgzf_read_all(str(t / name / f)) if f.endswith(".vcf.gz") else raw
    return out


NAMES = ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa", "_pepper_polished.fq"]


def _records(text):
    """the lines of a text file that ends with a newline"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    return lines[:-1]


def test_without_the_flag_nothing_changes(inputs):
    t, drafts = inputs
    made = []
    plain, zero = _run(t, "plain", [], made), _run(t, "zero", ["--min_depth", "0"], made)
    assert made == [{"qualities": True, "edits": True}] * 2          # the keyword reaches the opener only when set
    assert list(plain) == NAMES and plain == zero
    # and they are what the chain's pieces give: the read-free regions left out, the read-free contig absent
    fa = _records(plain[NAMES[2]])
    assert fa[0::2] == [">ctg2", ">ctg10"] and len(fa[1]) < len(drafts["ctg2"]) - 1_900 and len(fa[3]) == len(drafts["ctg10"])
    header = er.parse_vcf(plain[NAMES[0]].decode())[0]
    assert sum(h.startswith("pepper_no_reads=ctg2:") for h in header) == 1 and "pepper_no_reads=ctg30:1-2450" in header
    assert not any(h.startswith("pepper_min_depth") for h in header)


def test_read_free_regions_and_contigs_keep_the_draft(inputs, capsys):
    t, drafts = inputs
    made = []
    got = _run(t, "one", ["--min_depth", "1"], made)
    assert made == [{"qualities": True, "edits": True, "min_depth": 1}] and list(got) == NAMES
    err = capsys.readouterr().err
    # what every region gives: the stub's bases where it has reads, else the upper-cased draft of its kept range
    bh, fh = bamio.BamHandler(str(t / "r.bam")), bamio.FastaHandler(str(t / "r.fa"))
    want, want_q, free = {}, {}, []
    for c in ("ctg2", "ctg10", "ctg30"):
        seq, q = [], []
        for s, e in polish.polish_intervals(len(drafts[c])):
            has_reads = polish_summary.region_from_files(bh, fh, c, s, e) is not None
            free += [] if has_reads else [(c, s, e)]
            for p in range(s + 201 if s > 0 else s, e + 1):
                d = drafts[c][p].upper()
                if has_reads and p % 97 == 5 and d in "ACGT":
                    d = "ACGT"[("ACGT".index(d) + 1) % 4]
                seq.append(d)
                q.append(chr(33 + p % 60) if has_reads else "!")
        want[c], want_q[c] = "".join(seq), "".join(q)
        assert len(want[c]) == len(drafts[c])                         # the draft's coordinates are kept
    assert ("ctg2", 2900, 4100) in free and ("ctg2", 3900, 5100) in free and [c for c, _, _ in free].count("ctg30") == 3
    fa, fq = _records(got[NAMES[2]]), _records(got[NAMES[3]])
    assert fa == [x for c in ("ctg2", "ctg10", "ctg30") for x in (">" + c, want[c])]
    assert fq == [x for c in ("ctg2", "ctg10", "ctg30") for x in ("@" + c, want[c], "+", want_q[c])]
    assert want["ctg30"] == drafts["ctg30"].upper() and set(want_q["ctg30"]) == {"!"} and set("NRY") <= set(want["ctg30"])
    # the VCF: one pepper_min_depth line where the pepper_no_reads lines stood; the draft with the records applied is the FASTA
    header, cols, recs = er.parse_vcf(got[NAMES[0]].decode())
    assert header[3:] == ["contig=<ID=ctg2,length=9500>", "contig=<ID=ctg10,length=3300>", "contig=<ID=ctg30,length=2450>",
                          "pepper_min_depth=1"]
    for c in ("ctg2", "ctg10", "ctg30"):
        mine = [r[1:] for r in recs if r[0] == c]
        assert er.apply(mine, drafts[c].encode()) == want[c], c
        assert (len(mine) > 10) == (c != "ctg30")
        assert not [r for r in mine if c == "ctg2" and GAP[0] + 1_000 < r[0] < GAP[1] - 1_000]
    assert ("MIN DEPTH 1: %d CHUNK ROWS KEPT THE DRAFT, %d COULD NOT" % (3 * made_launches(err), made_launches(err))) in err
    assert ("%d REGIONS WITHOUT READS FILLED FROM THE DRAFT" % len(free)) in err


def made_launches(err: str) -> int:
    """launches of the run, from its own log line (the stub reports 3 masked rows and 1 unmaskable row per launch)"""
    import re
    m = re.search(r"MIN DEPTH 1: (\d+) CHUNK ROWS KEPT THE DRAFT, (\d+) COULD NOT", err)
    assert m and int(m.group(1)) == 3 * int(m.group(2)) and int(m.group(2)) >= 2
    return int(m.group(2))


def test_a_chain_made_for_another_threshold_is_refused_before_it_runs(inputs):
    t, _ = inputs

    class _Unused(_StubChain):
        def run(self, batch, windows=None):
            raise AssertionError("the chain may not run")
    for chain in (_Unused(), _Unused(min_depth=3)):
        with pytest.raises(ValueError) as e:
            polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), str(t / "other"), chain=chain, min_depth=2)
        assert "not made for this run" in str(e.value)
    assert os.listdir(str(t / "other")) == []
