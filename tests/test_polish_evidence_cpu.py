"""CPU: `polish --edits --evidence` without a device: the checker (tests/counts_ref.py) on hand-worked regions, the evidence
rule per edit kind, the composer's weakest column, the INFO text and header lines, the option and its refusals, and a stub
chain through the command, plain and under -hp."""
import os

import numpy as np
import pytest

import counts_ref as cr
import depth_ref as dr
import edits_ref as er
import select_ref as sel
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, synth
from pepper_thesis_amd.batch import Read, Region, pack_regions

BASE = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]


# ---- the checker on a hand-worked region ----------------------------------------------------------------------------------

def _hand_region():
    """positions 100..105. Forward and reverse reads, a lower-case base (g at 102), a read N (104), a deletion over 102-103, a
    3-base insert behind 102 shared by two reads and a 1-base insert there by a third, and a read of mapping quality 0"""
    reads = [Read.make(100, "6M", b"ACgTNC"),
             Read.make(100, "2M2D2M", b"ACAC", is_reverse=True),
             Read.make(101, "2M3I2M", b"CGTTATA"),
             Read.make(101, "2M3I1M", b"CGTTAT", is_reverse=True),
             Read.make(102, "1M1I1M", b"GcT"),
             Read.make(100, "6M", b"TTTTTT", mapq=0)]
    return Region(100, 105, b"ACGTAC", reads)


#              A- C- G- T- A+ C+ G+ T+ o- o+      (- reverse, + forward; o: other or deleted)
HAND = {(100, 0): [1, 0, 0, 0, 1, 0, 0, 0, 0, 0],
        (101, 0): [0, 2, 0, 0, 0, 2, 0, 0, 0, 0],
        (102, 0): [0, 0, 1, 0, 0, 0, 3, 0, 1, 0],
        (103, 0): [0, 0, 0, 1, 0, 0, 0, 3, 1, 0],
        (104, 0): [1, 0, 0, 0, 1, 0, 0, 0, 0, 1],
        (105, 0): [0, 1, 0, 0, 0, 1, 0, 0, 0, 0],
        (102, 1): [0, 0, 0, 1, 0, 1, 0, 1, 0, 0],
        (102, 2): [0, 0, 0, 1, 0, 0, 0, 1, 0, 0],
        (102, 3): [1, 0, 0, 0, 1, 0, 0, 0, 0, 0]}
HAND_DEPTH = [2, 4, 5, 5, 3, 2]


def test_hand_worked_counts():
    batch = pack_regions([_hand_region()])
    got = cr.region_counts(batch, 0)
    assert sorted(got) == sorted(HAND)
    for key, want in HAND.items():
        assert got[key].tolist() == want, key
    assert dr.region_depth(batch, 0).tolist() == HAND_DEPTH


def test_reads_that_leave_the_region():
    """a read that begins before the region and one that ends behind it count inside only; an insert whose anchor lies before
    the region or that begins behind its end is dropped"""
    reads = [Read.make(98, "4M", b"ACGT"),                       # 100, 101 <- G, T
             Read.make(100, "2I2M", b"TTAC", is_reverse=True),   # the insert's anchor is 99: dropped; 100, 101 <- A, C
             Read.make(104, "2M2I1M", b"ACGGT"),                 # 104, 105 <- A, C; the insert begins on 106 > end: dropped
             Read.make(105, "1M3D", b"A", is_reverse=True)]      # 105 <- A; the deletion begins behind the end
    batch = pack_regions([Region(100, 105, b"ACGTAC", reads)])
    got = cr.region_counts(batch, 0)
    assert sorted(got) == [(p, 0) for p in range(100, 106)]
    assert got[(100, 0)].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert got[(101, 0)].tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    assert got[(104, 0)].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert got[(105, 0)].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0]


def test_base_rows_sum_to_the_depth():
    import polish_cases as pc
    for regions in (pc.tile_edges(512), pc.tile_edges(1023, bare=True, tail=2), pc.all_bytes(), pc.many_regions()[:200]):
        batch = pack_regions(regions)
        for g in range(batch.n_regions):
            counts, depth = cr.region_counts(batch, g), dr.region_depth(batch, g)
            start = int(batch.ref_start[g])
            assert [int(counts[(start + c, 0)].sum()) for c in range(len(depth))] == depth.tolist(), g


def test_row_counts_follow_the_chunk_rows():
    batch = pack_regions([_hand_region()])
    position = np.array([[100, 101, 102, 102, 102], [102, 102, 103, -1, -1]], np.int64)
    index = np.array([[0, 0, 0, 1, 2], [2, 3, 0, -1, -1]], np.int32)
    got = cr.row_counts(batch, position, index, np.zeros(2, np.int32))
    assert got.dtype == np.uint16 and got.shape == (2, 5, 10)
    assert got[0].tolist() == [HAND[(100, 0)], HAND[(101, 0)], HAND[(102, 0)], HAND[(102, 1)], HAND[(102, 2)]]
    assert got[1].tolist() == [HAND[(102, 2)], HAND[(102, 3)], HAND[(103, 0)], [0] * 10, [0] * 10]


# ---- the evidence rule ------------------------------------------------------------------------------------------------------

def test_evidence_rule_per_kind():
    # (depth, ref, alt_fwd, alt_rev)
    assert cr.evidence_of(pe.KIND_SUB, ord("a"), ord("C"), HAND[(101, 0)], 4) == (4, 0, 2, 2)
    assert cr.evidence_of(pe.KIND_SUB, ord("C"), ord("A"), HAND[(101, 0)], 4) == (4, 4, 0, 0)
    assert cr.evidence_of(pe.KIND_SUB, ord("g"), ord("T"), HAND[(103, 0)], 5) == (5, 0, 3, 1)
    assert cr.evidence_of(pe.KIND_DEL, ord("G"), 0, HAND[(102, 0)], 5) == (5, 4, 0, 1)
    assert cr.evidence_of(pe.KIND_DEL, ord("a"), 0, HAND[(104, 0)], 3) == (3, 2, 1, 0)   # plane 9 holds the read's N
    # an inserted base: ref counts the reads over the anchor that hold nothing in this insert row
    assert cr.evidence_of(pe.KIND_INS, 0, ord("T"), HAND[(102, 1)], 5) == (5, 2, 1, 1)
    assert cr.evidence_of(pe.KIND_INS, 0, ord("A"), HAND[(102, 3)], 5) == (5, 3, 1, 1)
    assert cr.evidence_of(pe.KIND_INS, 0, ord("G"), HAND[(102, 2)], 5) == (5, 3, 0, 0)
    assert cr.evidence_of(pe.KIND_INS, 0, ord("G"), HAND[(102, 2)], 1) == (1, 0, 0, 0)   # never below 0


def test_a_draft_n_under_a_substitution_has_no_ref_reads():
    assert cr.evidence_of(pe.KIND_SUB, ord("N"), ord("G"), HAND[(102, 0)], 5) == (5, 0, 3, 1)
    assert cr.evidence_of(pe.KIND_SUB, ord("y"), ord("G"), HAND[(102, 0)], 5) == (5, 0, 3, 1)
    assert cr.evidence_of(pe.KIND_DEL, ord("N"), 0, HAND[(102, 0)], 5) == (5, 0, 0, 1)


def test_ref_is_clamped():
    c = [0, 40000, 0, 0, 0, 40000, 0, 0, 0, 0]
    assert cr.evidence_of(pe.KIND_SUB, ord("C"), ord("A"), c, 65535) == (65535, 65535, 0, 0)


# ---- the composer -----------------------------------------------------------------------------------------------------------

DRAFT = b"ACGTACGTAC"


def _recs(*rows):
    return np.array([r + (255,) for r in rows], pe.EDIT_DTYPE)


def _ev(*rows):
    return np.array(list(rows), pe.EVIDENCE_DTYPE)


def _composed(edits, evidence, draft=DRAFT):
    got = pe.compose_records("c", edits, draft, False, evidence=evidence)
    want = cr.record_evidence(list(edits), [tuple(int(v) for v in e) for e in evidence])
    assert [r.evidence for r in got] == want          # the product's composer against the checker's
    # and the records themselves are those of a run without evidence
    assert [tuple(r)[:4] for r in got] == [tuple(r) for r in pe.compose_records("c", edits, draft, False)]
    return got


def test_weakest_column_is_the_second():
    edits = _recs((3, 0, pe.KIND_SUB, ord("T"), ord("A")), (4, 0, pe.KIND_DEL, ord("A"), 0), (5, 0, pe.KIND_SUB, ord("C"), ord("G")))
    ev = _ev((30, 2, 14, 13), (31, 20, 1, 2), (29, 1, 9, 9))
    got = _composed(edits, ev)
    assert len(got) == 1 and got[0].evidence == (31, 20, 1, 2)      # all four numbers are that one column's


def test_tie_takes_the_first():
    edits = _recs((3, 0, pe.KIND_SUB, ord("T"), ord("A")), (3, 1, pe.KIND_INS, 0, ord("G")), (4, 0, pe.KIND_SUB, ord("A"), ord("C")),
                  (7, 0, pe.KIND_SUB, ord("T"), ord("C")))
    ev = _ev((30, 2, 5, 5), (30, 26, 3, 1), (28, 9, 0, 4), (27, 3, 12, 12))
    got = _composed(edits, ev)
    assert [r.evidence for r in got] == [(30, 26, 3, 1), (27, 3, 12, 12)]


def test_record_at_the_contig_start():
    edits = _recs((0, 0, pe.KIND_DEL, ord("A"), 0), (1, 0, pe.KIND_DEL, ord("C"), 0))
    got = _composed(edits, _ev((12, 9, 2, 1), (13, 10, 1, 1)))
    assert [tuple(r) for r in got] == [(1, "ACG", "G", None, (13, 10, 1, 1))]       # anchored behind; the weaker column is the second


def test_evidence_must_match_the_records():
    with pytest.raises(ValueError, match="evidence"):
        pe.compose_records("c", _recs((3, 0, pe.KIND_DEL, ord("T"), 0)), DRAFT, False, evidence=_ev((1, 1, 1, 1), (2, 2, 2, 2)))
    assert pe.compose_records("c", _recs(), DRAFT, False, evidence=_ev()) == []


def test_checker_on_the_reference_records():
    """the weakest-column rule on the blocks tests/edits_ref.py cuts: its vcf_records and the checker's blocks agree in number
    and the product's composer gives each the checker's evidence"""
    rng = np.random.default_rng(5)
    draft = bytes(rng.choice(list(b"ACGT"), 400).astype(np.uint8))
    pred = {}
    for p in range(400):
        d = "ACGT".index(chr(draft[p]))
        r = rng.random()
        pred[(p, 0)] = ((0 if r < .1 else 1 + (d + 1) % 4 if r < .25 else 1 + d), 255)
        if rng.random() < .1:
            pred[(p, 1)] = (int(rng.integers(1, 5)), 255)
    prim = er.primitive_edits(pred, draft, 0)
    edits = np.array(prim, pe.EDIT_DTYPE)
    ev = np.zeros(len(edits), pe.EVIDENCE_DTYPE)
    for f in ev.dtype.names:
        ev[f] = rng.integers(0, 6, len(edits))
    got = _composed(edits, ev, draft)
    ref_records = er.vcf_records(er.replacements(pred, draft, 0), draft, False)
    assert [tuple(r)[:3] for r in got] == [tuple(r)[:3] for r in ref_records]
    assert len(cr.blocks_of(prim)) == len(ref_records)


# ---- the text ----------------------------------------------------------------------------------------------------------------

INFO_LINES = [
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads over the weakest edited column of the record">',
    '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads that spell the draft, reads that spell the edit, at that column">',
    '##INFO=<ID=SAF,Number=A,Type=Integer,Description="Forward-strand reads that spell the edit at that column">',
    '##INFO=<ID=SAR,Number=A,Type=Integer,Description="Reverse-strand reads that spell the edit at that column">']


def test_info_text_and_header_lines():
    recs = {"c": [pe.EvidenceVcfRecord(2, "C", "T", 30, (31, 20, 1, 2)), pe.EvidenceVcfRecord(5, "AC", "A", None, (7, 0, 0, 3))]}
    text = pe.vcf_text("s", "r", [("c", 10)], [], recs, 3, 20, haplotype=2, evidence=True).split("\n")
    assert text[:4] == ["##fileformat=VCFv4.2", "##source=s", "##reference=r", "##contig=<ID=c,length=10>"]
    assert text[4:8] == INFO_LINES                                            # in front of the pepper_* lines
    assert text[8:12] == ["##pepper_min_depth=3", "##pepper_min_qual=20", "##pepper_haplotype=2",
                          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    assert text[12:] == ["c\t2\t.\tC\tT\t30\tPASS\tDP=31;AD=20,3;SAF=1;SAR=2", "c\t5\t.\tAC\tA\t.\tPASS\tDP=7;AD=0,3;SAF=0;SAR=3", ""]
    assert pe.info_text((31, 20, 1, 2)) == cr.info_text((31, 20, 1, 2)) == "DP=31;AD=20,3;SAF=1;SAR=2"
    # without the keyword the text is the one of a build without the feature, whatever the records carry
    plain = {"c": [pe.VcfRecord(*r[:4]) for r in recs["c"]]}
    assert pe.vcf_text("s", "r", [("c", 10)], [], recs) == pe.vcf_text("s", "r", [("c", 10)], [], plain)
    assert "INFO=" not in pe.vcf_text("s", "r", [("c", 10)], [], plain) and pe.vcf_text("s", "r", [("c", 10)], [], plain).endswith("PASS\t.\n")


def test_dtype_is_the_header_struct():
    from pepper_thesis_amd import _ffi
    import ctypes as C
    assert C.sizeof(_ffi.pv_polish_evidence) == pe.EVIDENCE_DTYPE.itemsize == 8
    assert [n for n, _ in _ffi.pv_polish_evidence._fields_] == list(pe.EVIDENCE_DTYPE.names) == ["depth", "ref", "alt_fwd", "alt_rev"]
    assert _ffi.pv_polish_out._fields_[-2:] == [("depth", C.c_void_p), ("counts", C.c_void_p)]   # behind the earlier members


# ---- the option ---------------------------------------------------------------------------------------------------------------

def test_option_parses_on_both_entry_points(monkeypatch):
    assert cli.polish_parser().parse_args(BASE + ["--edits", "--evidence"]).evidence is True
    assert cli.polish_parser().parse_args(BASE + ["--edits"]).evidence is False
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.evidence) or 0)
    assert cli.main(["polish"] + BASE + ["--edits", "--evidence"]) == 0 and cli.main(["polish"] + BASE) == 0
    assert pepper.main(["polish"] + BASE + ["--edits", "--evidence"]) == 0
    assert seen == [True, False, True]
    args = pepper.parser().parse_args(["polish"] + BASE + ["-hp", "--bf16", "--realign", "--gpu_decode", "--qualities", "--edits",
                                                            "--evidence", "--min_depth", "3", "--min_qual", "20"])
    assert args.evidence and args.use_hp_info and args.min_qual == 20 and args.min_depth == 3 and args.edits


def test_the_step_commands_do_not_take_the_flag():
    for cmd in ("make_images", "call_consensus", "stitch"):
        with pytest.raises(SystemExit) as e:
            pepper.parser().parse_args([cmd, "--evidence"])
        assert e.value.code == 2


def _refused(tmp_path, monkeypatch, flags):
    from pepper_thesis_amd import polish_rank
    started = []

    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out")] + flags)
    assert polish.run(args, open_chain=open_chain) == 2
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


def test_evidence_without_edits_is_refused(tmp_path, capsys, monkeypatch):
    _refused(tmp_path, monkeypatch, ["--evidence"])
    assert "--evidence needs --edits" in capsys.readouterr().err


def test_evidence_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    _refused(tmp_path, monkeypatch, ["--edits", "--evidence", "-d_ids", "0,1"])
    err = capsys.readouterr().err
    assert "runs on one device" in err and "0,1" in err


def test_chain_and_command_refuse_evidence_without_edits():
    with pytest.raises(ValueError, match="needs edits"):
        polish._DeviceChain(None, evidence=True)
    with pytest.raises(ValueError, match="needs edits"):
        polish.polish_fused("b", "f", "m", "o", evidence=True, chain=object())


def test_results_and_pieces_keep_their_fields():
    res = polish.ChainResult(np.array([0, 2]), b"AC", None, np.array([0, 1]), np.zeros(1, pe.EDIT_DTYPE))
    assert res.evidence is None and res.region(0) == (b"AC", None, res.edits[0:1])
    ev = np.array([(9, 1, 5, 1)], pe.EVIDENCE_DTYPE)
    got = polish.with_evidence(res, ev)
    assert tuple(got)[:3] == tuple(res)[:3] and got.evidence is ev and len(got.region(0)) == 4 and got.region(0)[3].tolist() == ev.tolist()
    both = polish.with_filtered(polish.with_masked(got, (3, 2)), (7, 1))
    assert (both.masked, both.filtered) == ((3, 2), (7, 1)) and both.evidence is ev
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    w = polish.Work(4, 0, "c", 10, 20)
    p = polish.piece_of(w, got.region(0))
    assert tuple(p)[:5] == ("c", 10, 4, b"AC", None) and p.evidence.tolist() == ev.tolist()
    assert polish.piece_of(w, res.region(0)).evidence is None and polish.Piece("c", 0, 0, b"").evidence is None


# ---- a stub chain through the command -------------------------------------------------------------------------------------

def _stub_evidence(p: int, h: int):
    """(depth, ref, alt_fwd, alt_rev) the stub gives the edit at p in haplotype h's pass; every third has one strand only"""
    return (40 + p % 7 + h, p % 5, 0 if p % 3 == 0 else 1 + p % 11, 2 + (p + h) % 9)


class _StubChain:
    """the chain's contract without a device (as in test_polish_hp_cpu.py): every region gives the upper-cased draft the stitch
    would keep with a substitution at every p with p % 97 == 5 * haplotype, and, made for evidence, _stub_evidence beside each"""

    def __init__(self, qualities=False, edits=False, use_hp=False, evidence=False):
        self.qualities, self.edits, self.use_hp, self.evidence = qualities, edits, use_hp, evidence

    def _result(self, batch, h):
        out, recs, evs, roff, eoff = [], [], [], [0], [0]
        for g in range(batch.n_regions):
            a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
            draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1].decode()
            s = []
            for p in range(a + 201 if a > 0 else a, b + 1):
                d = draft[p - a].upper()
                if p % 97 == 5 * h:
                    new = "ACGT"[("ACGT".index(d) + 1) % 4]
                    recs.append((p, 0, pe.KIND_SUB, ord(draft[p - a]), ord(new), 255))
                    evs.append(_stub_evidence(p, h))
                    d = new
                s.append(d)
            out.append("".join(s).encode())
            roff.append(roff[-1] + len(s))
            eoff.append(len(recs))
        res = polish.ChainResult(np.asarray(roff, np.int64), b"".join(out), None)
        if self.edits:
            res = res._replace(edit_off=np.asarray(eoff, np.int64), edits=np.array(recs, pe.EDIT_DTYPE))
        return polish.with_evidence(res, np.array(evs, pe.EVIDENCE_DTYPE)) if self.evidence else res

    def run(self, batch, windows=None):
        if not self.use_hp:
            return self._result(batch, 0)
        from pepper_thesis_amd.batch_select import tag_counts
        has = [np.diff(sel.select(batch, h)[0].read_off) > 0 for h in (1, 2)]
        return polish.HapChainResult((self._result(batch, 1), self._result(batch, 2)), tuple(has), tag_counts(batch.read_hp, batch.n_reads))

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("evidence_cpu")
    rng = np.random.default_rng(71)
    contigs = [("ctg1", "".join(rng.choice(list("ACGTacgt"), size=3_300))), ("ctg2", "".join(rng.choice(list("ACGTacgt"), size=1_500)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        mine = bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
        for k, r in enumerate(mine):
            r["hp"] = (None, 1, 2)[k % 3]
        recs += mine
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    return tmp, dict(contigs)


def _run(t, name, flags, made):
    base = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "3", "-bs", "8"]

    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append(kw)
        return _StubChain(**kw)
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / name)] + flags), open_chain=open_chain) == 0
    out = {}
    for f in sorted(os.listdir(str(t / name))):
        out[f] = bamio.bgzf_read_all(str(t / name / f)) if f.endswith(".vcf.gz") else open(str(t / name / f), "rb").read()
    return out


def _split(vcf: bytes):
    """-> (header lines, record lines as column lists)"""
    lines = vcf.decode().split("\n")
    assert lines[-1] == ""
    return [l for l in lines[:-1] if l.startswith("#")], [l.split("\t") for l in lines[:-1] if not l.startswith("#")]


def _check_vcf(with_flag: bytes, without: bytes, h: int):
    head, recs = _split(with_flag)
    head0, recs0 = _split(without)
    assert [l for l in head if not l.startswith("##INFO=")] == head0 and [l for l in head if l.startswith("##INFO=")] == INFO_LINES
    assert [r[:7] + ["."] for r in recs] == recs0 and len(recs) > 20
    for r in recs:          # a substitution alone: the record's position is the edit's
        assert r[7] == cr.info_text(_stub_evidence(int(r[1]) - 1, h)), r
    return sum((ev[2] == 0) != (ev[3] == 0) for ev in (_stub_evidence(int(r[1]) - 1, h) for r in recs)), len(recs)


def test_command_writes_the_evidence_and_leaves_the_rest(inputs, capsys):
    t, _ = inputs
    made = []
    plain = _run(t, "plain", ["--edits"], made)
    capsys.readouterr()
    got = _run(t, "ev", ["--edits", "--evidence"], made)
    err = capsys.readouterr().err
    assert made == [{"edits": True}, {"edits": True, "evidence": True}]       # the keyword reaches the opener only when set
    names = ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi", "_pepper_polished.fa"]
    assert list(plain) == list(got) == names and plain[names[2]] == got[names[2]]
    # the run without the flag: no INFO header line, `.` in every INFO column
    head0, recs0 = _split(plain[names[0]])
    assert not any(l.startswith("##INFO") for l in head0) and {r[7] for r in recs0} == {"."}
    one_strand, n = _check_vcf(got[names[0]], plain[names[0]], 0)
    assert one_strand > 0 and "EVIDENCE: %d OF %d RECORDS HAVE THEIR ALT SUPPORT ON ONE STRAND ONLY" % (one_strand, n) in err


def test_each_haplotype_carries_its_own_evidence(inputs, capsys):
    t, _ = inputs
    made = []
    plain = _run(t, "hp_plain", ["--edits", "-hp"], made)
    got = _run(t, "hp_ev", ["--edits", "--evidence", "-hp"], made)
    assert made[1] == {"edits": True, "use_hp": True, "evidence": True}
    assert list(plain) == list(got) and len(got) == 6
    total = 0
    for h in (1, 2):
        assert got["_pepper_polished_hp%d.fa" % h] == plain["_pepper_polished_hp%d.fa" % h]
        name = "_pepper_polished_hp%d.edits.vcf.gz" % h
        assert ("##pepper_haplotype=%d" % h).encode() in got[name]
        total += _check_vcf(got[name], plain[name], h)[0]
    assert "EVIDENCE: %d OF" % total in capsys.readouterr().err
