"""CPU: `polish -hp` without a device: the option and its refusal, and a stub chain through the command: the two sets of files
and no un-suffixed one, the ##pepper_haplotype line, a region whose selection is empty for one haplotype, the draft fill with
--min_depth, the log line and the warning, and a run without the flag that writes exactly what it wrote before."""
import os
import re

import numpy as np
import pytest

import edits_ref as er
import select_ref as sel
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, synth

BASE = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]


def test_option_parses_on_both_entry_points(monkeypatch):
    assert cli.polish_parser().parse_args(BASE + ["-hp"]).use_hp_info is True
    assert cli.polish_parser().parse_args(BASE + ["--use_hp_info"]).use_hp_info is True
    assert cli.polish_parser().parse_args(BASE).use_hp_info is False
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.use_hp_info) or 0)
    assert cli.main(["polish"] + BASE + ["-hp"]) == 0 and cli.main(["polish"] + BASE) == 0
    assert pepper.main(["polish"] + BASE + ["--use_hp_info"]) == 0
    assert seen == [True, False, True]
    args = pepper.parser().parse_args(["polish"] + BASE + ["-hp", "--bf16", "--realign", "--gpu_decode", "--qualities", "--edits",
                                                            "--min_depth", "3", "--min_qual", "20"])
    assert args.use_hp_info and args.min_qual == 20 and args.min_depth == 3 and args.edits and args.qualities and args.gpu_decode


def test_the_step_commands_do_not_take_the_flag():
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--use_hp_info"])
        assert e.value.code == 2


def test_polish_hp_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []

    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "-hp", "-d_ids", "0,1"])
    assert polish.run(args, open_chain=open_chain) == 2
    err = capsys.readouterr().err
    assert "-hp runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_vcf_header_names_the_haplotype_once():
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20, haplotype=2).split("\n")
    assert text[4:8] == ["##pepper_min_depth=3", "##pepper_min_qual=20", "##pepper_haplotype=2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs, haplotype=0) == pe.vcf_text("s", "r", [("c", 10)], [], recs)
    assert "pepper_haplotype" not in pe.vcf_text("s", "r", [("c", 10)], [("c", 1, 4)], recs)


def test_hp_path():
    assert polish.hp_path("o/_pepper_polished.fa", 1) == "o/_pepper_polished_hp1.fa"
    assert polish.output_fastq_path(polish.hp_path("o/_pepper_polished.fa", 2)) == "o/_pepper_polished_hp2.fq"
    assert pe.output_vcf_path(polish.hp_path("o/_pepper_polished.fa", 2)) == "o/_pepper_polished_hp2.edits.vcf.gz"
    assert polish.HapChainResult._fields == ("results", "has_reads", "tags", "payload")
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    assert polish.Piece._fields == ("contig", "start", "index", "bases", "qual", "edits")


# ---- a stub chain through the command ------------------------------------------------------------------------------------

class _StubChain:
    """the chain's contract without a device: every region gives the upper-cased draft bases the stitch would keep, with a
    substitution at every position p with p % 97 == 5 * haplotype (haplotype 0: a chain made without use_hp), and the planes it
    was made for. Made with use_hp it answers with a HapChainResult: which regions keep reads comes from the batch's tags."""

    def __init__(self, qualities=False, edits=False, min_depth=0, use_hp=False):
        self.qualities, self.edits, self.min_depth, self.use_hp = qualities, edits, min_depth, use_hp
        self.batches = 0

    def _result(self, batch, h):
        out, quals, recs, roff, eoff = [], [], [], [0], [0]
        for g in range(batch.n_regions):
            a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
            draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1].decode()
            s = []
            for p in range(a + 201 if a > 0 else a, b + 1):
                d = draft[p - a].upper()
                if p % 97 == 5 * h:
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
        return polish.with_masked(res, (1, 0)) if self.min_depth else res

    def run(self, batch, windows=None):
        self.batches += 1
        if not self.use_hp:
            return self._result(batch, 0)
        from pepper_thesis_amd.batch_select import tag_counts
        has = [np.diff(sel.select(batch, h)[0].read_off) > 0 for h in (1, 2)]
        return polish.HapChainResult((self._result(batch, 1), self._result(batch, 2)), tuple(has), tag_counts(batch.read_hp, batch.n_reads))

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """ctg1: reads of both haplotypes, untagged ones and a few with HP:3; ctg2: HP:2 reads only; untagged.bam: no tags"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("hp_cpu")
    rng = np.random.default_rng(61)
    contigs = [("ctg1", "".join(rng.choice(list("ACGTacgt"), size=3_300))), ("ctg2", "".join(rng.choice(list("ACGTacgt"), size=1_500)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        mine = bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
        for k, r in enumerate(mine):
            r["hp"] = 2 if tid == 1 else (None, 1, 2, 1, 2, 3)[k % 6]
        recs += mine
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    refs = [(n, len(s)) for n, s in contigs]
    bw.write_bam(str(tmp / "r.bam"), refs, recs)
    bw.write_bam(str(tmp / "untagged.bam"), refs, [dict(r, hp=None) for r in recs])
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    tags = [r["hp"] for r in recs]
    return tmp, dict(contigs), tags


def _run(t, name, flags, made, bam="r.bam"):
    base = ["-b", str(t / bam), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "3", "-bs", "8"]

    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append(kw)
        return _StubChain(**kw)
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / name)] + flags), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(str(t / name))):
        out[f] = bamio.bgzf_read_all(str(t / name / f)) if f.endswith(".vcf.gz") else open(str(t / name / f), "rb").read()
    return out


def _fasta(data: bytes):
    lines = data.decode().split("\n")
    return dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))


def _expected(draft: str, h: int, first: int = 0) -> str:
    s = list(draft.upper())
    for p in range(first, len(s)):
        if p % 97 == 5 * h:
            s[p] = "ACGT"[("ACGT".index(s[p]) + 1) % 4]
    return "".join(s)


def test_without_the_flag_nothing_changes(inputs, capsys):
    t, drafts, _ = inputs
    made = []
    got = _run(t, "plain", ["--qualities", "--edits"], made)
    assert made == [{"qualities": True, "edits": True}]                 # the keyword reaches the opener only when set
    assert list(got) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa", "_pepper_polished.fq"]
    assert _fasta(got["_pepper_polished.fa"]) == {c: _expected(d, 0) for c, d in drafts.items()}
    err = capsys.readouterr().err
    assert b"pepper_haplotype" not in got["_pepper_polished.edits.vcf.gz"] and "HAPLOTYPES" not in err and "_hp" not in err


def test_two_fastas_and_no_unsuffixed_file(inputs, capsys):
    t, drafts, tags = inputs
    made = []
    got = _run(t, "hp", ["-hp"], made)
    assert made == [{"use_hp": True}]
    assert list(got) == ["_pepper_polished_hp1.fa", "_pepper_polished_hp2.fa"]
    # ctg2 holds HP:2 reads only: haplotype 1 has no reads there, so its FASTA is without the contig
    assert _fasta(got["_pepper_polished_hp1.fa"]) == {"ctg1": _expected(drafts["ctg1"], 1)}
    assert _fasta(got["_pepper_polished_hp2.fa"]) == {c: _expected(d, 2) for c, d in drafts.items()}
    err = capsys.readouterr().err
    m = re.search(r"HAPLOTYPES: (\d+) READS SEEN, (\d+) UNTAGGED, (\d+) HP1, (\d+) HP2, (\d+) WITH OTHER TAG VALUES", err)
    assert m and "WARNING" not in err
    seen, untagged, hp1, hp2, other = (int(v) for v in m.groups())
    # a read is seen once per region it reaches, so the counts are at least the file's and keep its proportions' order
    assert seen == untagged + hp1 + hp2 + other and untagged >= tags.count(None) and hp1 >= tags.count(1)
    assert hp2 >= tags.count(2) and other >= tags.count(3) > 0 and hp2 > hp1 > 0
    assert "_pepper_polished_hp1.fa" in err and "_pepper_polished_hp2.fa" in err


def test_fastq_and_vcf_names_and_the_header_line(inputs):
    t, drafts, _ = inputs
    made = []
    got = _run(t, "hp_all", ["-hp", "--qualities", "--edits"], made)
    assert made == [{"qualities": True, "edits": True, "use_hp": True}]
    assert list(got) == ["_pepper_polished_hp%d%s" % (h, x) for h in (1, 2) for x in (".edits.vcf.gz", ".edits.vcf.gz.tbi", ".fa", ".fq")]
    for h in (1, 2):
        fa = _fasta(got["_pepper_polished_hp%d.fa" % h])
        fq = got["_pepper_polished_hp%d.fq" % h].decode().split("\n")
        assert fq[0::4][:-1] == ["@" + c for c in fa] and fq[1::4] == list(fa.values())
        header, cols, recs = er.parse_vcf(got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode())
        assert header[-1] == "pepper_haplotype=%d" % h and sum(l.startswith("pepper_haplotype") for l in header) == 1
        assert ("pepper_no_reads=ctg2:1-1500" in header) == (h == 1)       # haplotype 1 polished nothing of ctg2
        for c in fa:
            mine = [r[1:] for r in recs if r[0] == c]
            assert er.apply(mine, drafts[c].encode()) == fa[c] and len(mine) > 10
        assert not [r for r in recs if r[0] not in fa]


def test_min_depth_fills_the_emptied_regions_from_the_draft(inputs, capsys):
    t, drafts, _ = inputs
    made = []
    got = _run(t, "hp_depth", ["-hp", "--min_depth", "1", "--edits"], made)
    assert made == [{"edits": True, "min_depth": 1, "use_hp": True}]
    assert _fasta(got["_pepper_polished_hp1.fa"]) == {"ctg1": _expected(drafts["ctg1"], 1), "ctg2": drafts["ctg2"].upper()}
    assert _fasta(got["_pepper_polished_hp2.fa"]) == {c: _expected(d, 2) for c, d in drafts.items()}
    for h in (1, 2):
        header, cols, recs = er.parse_vcf(got["_pepper_polished_hp%d.edits.vcf.gz" % h].decode())
        assert header[-2:] == ["pepper_min_depth=1", "pepper_haplotype=%d" % h] and not any("no_reads" in l for l in header)
        assert (h == 2) == any(r[0] == "ctg2" for r in recs)
    assert re.search(r"MIN DEPTH 1: \d+ CHUNK ROWS KEPT THE DRAFT, 0 COULD NOT \(DRAFT BYTE NOT ACGT\), 2 REGIONS", capsys.readouterr().err)


def test_untagged_file_gives_the_plain_run_twice_and_a_warning(inputs, capsys):
    t, drafts, _ = inputs
    made = []
    got = _run(t, "hp_untagged", ["-hp"], made, bam="untagged.bam")
    assert list(got) == ["_pepper_polished_hp1.fa", "_pepper_polished_hp2.fa"]
    for h in (1, 2):                                            # (the stub marks the haplotype; the contigs are all there)
        assert _fasta(got["_pepper_polished_hp%d.fa" % h]) == {c: _expected(d, h) for c, d in drafts.items()}
    err = capsys.readouterr().err
    assert "WARNING: polish -hp: no read carries an HP tag" in err
    m = re.search(r"HAPLOTYPES: (\d+) READS SEEN, (\d+) UNTAGGED, 0 HP1, 0 HP2, 0 WITH OTHER", err)
    assert m and m.group(1) == m.group(2) != "0"


def test_a_chain_made_without_use_hp_is_refused_before_it_runs(inputs):
    t, _, _ = inputs

    class _Unused(_StubChain):
        def run(self, batch, windows=None):
            raise AssertionError("the chain may not run")
    with pytest.raises(ValueError) as e:
        polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), str(t / "other"), chain=_Unused(), use_hp=True)
    assert "not made for this run" in str(e.value)
    assert os.listdir(str(t / "other")) == []
