"""CPU: `polish --edits` without a device: the composer on hand-worked blocks, QUAL, the header, the refusal of records that
are not increasing, the option on both entry points, the multi-device refusal, and a stub chain through the command whose
VCF applies back to the FASTA (tests/edits_ref.py)."""
import os

import numpy as np
import pytest

import edits_ref as er
from pepper_thesis_amd import bamio, build, cli, pepper, polish, polish_edits as pe, synth

#        0123456789
DRAFT = b"ACgTNACGTA"


def _recs(*rows):
    """(position, index, kind, base, qual) rows -> EDIT_DTYPE records; the draft byte is DRAFT's for index 0"""
    a = np.zeros(len(rows), pe.EDIT_DTYPE)
    for i, (p, x, kind, base, q) in enumerate(rows):
        a[i] = (p, x, kind, DRAFT[p] if x == 0 else 0, ord(base) if base else 0, q)
    return a


def _compose(*rows, qualities=True, draft=DRAFT, warn=None):
    return [tuple(r) for r in pe.compose_records("c", _recs(*rows), draft, qualities, warn=warn)]


def test_record_type_is_the_c_struct():
    import ctypes as C
    from pepper_thesis_amd import _ffi
    assert pe.EDIT_DTYPE.itemsize == C.sizeof(_ffi.pv_polish_edit) == 16
    for name, _ in _ffi.pv_polish_edit._fields_:
        assert pe.EDIT_DTYPE.fields[name][1] == getattr(_ffi.pv_polish_edit, name).offset
    assert (pe.KIND_SUB, pe.KIND_DEL, pe.KIND_INS) == (er.SUB, er.DEL, er.INS) == (1, 2, 3)


def test_composer_on_hand_worked_blocks():
    assert _compose((1, 0, 1, "T", 30)) == [(2, "C", "T", 30)]                                     # a SNP
    assert _compose((1, 0, 1, "T", 30), (2, 0, 1, "A", 20), (3, 0, 1, "C", 25)) == [(2, "CGT", "TAC", 20)]   # an MNP; g -> G
    assert _compose((5, 1, 3, "G", 9), (5, 2, 3, "T", 8)) == [(6, "A", "AGT", 8)]                  # an insertion behind an unchanged base
    assert _compose((6, 0, 2, None, 12), (7, 0, 2, None, 11)) == [(6, "ACG", "A", 11)]              # a deletion: the left anchor
    assert _compose((0, 0, 2, None, 5), (1, 0, 2, None, 6)) == [(1, "ACG", "G", 5)]                 # at position 0: the right anchor
    assert _compose((2, 0, 1, "A", 40), (3, 0, 2, None, 7)) == [(2, "CGT", "CA", 7)]                # a substitution, then a deletion
    assert _compose((8, 0, 2, None, 3), (9, 0, 2, None, 4)) == [(8, "GTA", "G", 3)]                 # a block that ends at the contig end
    assert _compose((9, 0, 1, "C", 3), (9, 1, 3, "C", 2)) == [(9, "TA", "TCC", 2)]                  # longer and another first base: anchored
    assert _compose((9, 0, 1, "C", 3)) == [(10, "A", "C", 3)]
    assert _compose((4, 0, 1, "A", 50)) == [(5, "N", "A", 50)]                                      # a draft N under a base label
    # a deletion with an insertion behind it keeps no base of its own: anchored; a substitution with one is not
    assert _compose((3, 0, 2, None, 9), (3, 1, 3, "C", 9)) == [(4, "T", "C", 9)]
    assert _compose((3, 0, 2, None, 9), (3, 1, 3, "C", 9), (3, 2, 3, "C", 9)) == [(3, "GT", "GCC", 9)]
    # two blocks: an unchanged position between them; POS strictly increasing
    got = _compose((1, 0, 2, None, 1), (3, 0, 2, None, 2), (4, 0, 1, "T", 3), (6, 1, 3, "A", 4))
    assert got == [(1, "AC", "A", 1), (4, "TN", "T", 2), (7, "C", "CA", 4)]   # T N -> T: shorter, same first base: no anchor
    # every block equals the checker's walk over the same edits
    rep = {p: (er.upper(DRAFT[p]), None) for p in range(len(DRAFT))}
    rep.update({1: ("", 1), 3: ("", 2), 4: ("T", 3), 6: ("CA", 4)})
    assert got == er.vcf_records(rep, DRAFT, True)
    assert er.apply(got, DRAFT) == "AGTACAGTA"


def test_whole_contig_deleted_gives_a_warning_and_no_record():
    said = []
    assert _compose((0, 0, 2, None, 1), (1, 0, 2, None, 1), draft=b"AC", warn=said.append) == []
    assert len(said) == 1 and "contig c" in said[0]
    # the whole contig replaced by something: nothing to anchor on, and nothing needed
    assert _compose((0, 0, 2, None, 1), (1, 0, 2, None, 1), (1, 1, 3, "T", 1), draft=b"AC", warn=said.append) == [(1, "AC", "T", 1)]
    assert len(said) == 1


def test_qual_is_the_block_minimum_or_a_dot():
    rows = ((1, 0, 1, "T", 30), (2, 0, 2, None, 0), (2, 1, 3, "A", 93), (7, 0, 1, "A", 255))
    assert [r[3] for r in _compose(*rows)] == [0, 255]
    assert [r[3] for r in _compose(*rows, qualities=False)] == [None, None]
    text = pe.vcf_text("s", "r", [("c", 10)], [], {"c": pe.compose_records("c", _recs(*rows), DRAFT, False)})
    assert text.endswith("c\t2\t.\tCG\tTA\t.\tPASS\t.\nc\t8\t.\tG\tA\t.\tPASS\t.\n")
    text = pe.vcf_text("s", "r", [("c", 10)], [], {"c": pe.compose_records("c", _recs(*rows), DRAFT, True)})
    assert text.endswith("c\t2\t.\tCG\tTA\t0\tPASS\t.\nc\t8\t.\tG\tA\t255\tPASS\t.\n")


def test_header_order_and_no_read_lines():
    runs = pe.no_read_runs([("ctg2", 3101, 4100), ("ctg2", 4101, 5100), ("ctg2", 7101, 8100), ("ctg10", 0, 1100), ("ctg10", 1101, 1150),
                            ("ctg10", 1301, 1200)])
    assert runs == [("ctg2", 3102, 5101), ("ctg2", 7102, 8101), ("ctg10", 1, 1151)]      # adjacent ranges merged, an empty one left out
    recs = {"ctg10": [pe.VcfRecord(5, "A", "C", None)], "ctg2": [pe.VcfRecord(1, "AC", "A", 7), pe.VcfRecord(9, "T", "TG", 0)]}
    text = pe.vcf_text("pepper_thesis_amd polish", "/d/draft.fa", [("ctg10", 2000), ("ctg2", 9500), ("ctg1", 30)], runs, recs)
    assert text.split("\n") == [
        "##fileformat=VCFv4.2", "##source=pepper_thesis_amd polish", "##reference=/d/draft.fa",
        "##contig=<ID=ctg1,length=30>", "##contig=<ID=ctg2,length=9500>", "##contig=<ID=ctg10,length=2000>",
        "##pepper_no_reads=ctg2:3102-5101", "##pepper_no_reads=ctg2:7102-8101", "##pepper_no_reads=ctg10:1-1151",
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
        "ctg2\t1\t.\tAC\tA\t7\tPASS\t.", "ctg2\t9\t.\tT\tTG\t0\tPASS\t.", "ctg10\t5\t.\tA\tC\t.\tPASS\t.", ""]
    header, cols, parsed = er.parse_vcf(text)
    assert er.no_read_ranges(header, "ctg2") == [(3101, 5100), (7101, 8100)] and len(parsed) == 3 and cols.count("\t") == 7


def test_vcf_is_written_bgzipped_with_an_index_under_its_final_names_only(tmp_path):
    build.build_io()
    path = str(tmp_path / "_pepper_polished.edits.vcf.gz")
    assert pe.output_vcf_path(str(tmp_path / "_pepper_polished.fa")) == path
    recs = {"c": [pe.VcfRecord(2, "C", "T", 30)]}
    pe.write_edits_vcf(path, "s", "r", [("c", 10)], [], recs)
    assert sorted(os.listdir(str(tmp_path))) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi"]
    assert bamio.bgzf_read_all(path).decode() == pe.vcf_text("s", "r", [("c", 10)], [], recs)
    assert bamio.bgzf_read_all(path + ".tbi")[:4] == b"TBI\x01"


@pytest.mark.parametrize("rows", [((3, 0, 1, "A", 1), (3, 0, 1, "C", 1)), ((3, 1, 3, "A", 1), (3, 0, 2, None, 1)),
                                  ((5, 0, 2, None, 1), (4, 0, 2, None, 1)), ((3, 0, 2, None, 1), (12, 0, 2, None, 1))])
def test_records_that_do_not_increase_or_leave_the_draft_are_refused(rows):
    with pytest.raises(ValueError) as e:
        pe.compose_records("ctg7", _bad(rows), DRAFT, True)
    assert "ctg7" in str(e.value)


def _bad(rows):
    a = np.zeros(len(rows), pe.EDIT_DTYPE)
    for i, (p, x, kind, base, q) in enumerate(rows):
        a[i] = (p, x, kind, 0, ord(base) if base else 0, q)
    return a


def test_edits_option_parses_on_both_entry_points(monkeypatch):
    base = ["-b", "r", "-f", "f", "-m", "m", "-o", "o"]
    assert cli.polish_parser().parse_args(base + ["--edits"]).edits is True
    assert cli.polish_parser().parse_args(base).edits is False
    seen = []
    monkeypatch.setattr(polish, "run", lambda args: seen.append(args.edits) or 0)
    assert cli.main(["polish"] + base + ["--edits"]) == 0 and cli.main(["polish"] + base) == 0     # python -m pepper_thesis_amd
    assert pepper.main(["polish"] + base + ["--edits"]) == 0                                        # python -m pepper_thesis_amd.pepper
    assert seen == [True, False, True]
    ap = pepper.parser()
    assert ap.parse_args(["polish"] + base + ["--edits", "--bf16", "--realign", "--gpu_decode", "--qualities"]).edits is True
    assert ap.parse_args(["polish"] + base).edits is False


def test_polish_edits_on_several_devices_is_refused(tmp_path, capsys, monkeypatch):
    from pepper_thesis_amd import polish_rank
    started = []
    monkeypatch.setattr(polish_rank, "launch", lambda *a, **k: started.append("launch") or 0)

    def open_chain(*a, **k):
        started.append("chain")
        raise AssertionError("no chain may be opened")
    args = cli.polish_parser().parse_args(["-b", str(tmp_path / "no.bam"), "-f", str(tmp_path / "no.fa"), "-m", str(tmp_path / "no.pkl"),
                                           "-o", str(tmp_path / "out"), "--edits", "-d_ids", "0,1"])
    assert polish.run(args, open_chain=open_chain) == 2
    err = capsys.readouterr().err
    assert "--edits runs on one device" in err and "0,1" in err
    assert started == [] and not os.path.exists(str(tmp_path / "out"))


# ---- a stub chain through the command -----------------------------------------------------------------------------------

class _EditingChain:
    """the chain's contract without a device: every region gives the draft bases the stitch would keep, changed by a rule on
    the position alone (a substitution, a deletion, two inserted bases, and around every 500th position all three at once),
    and, when made for it, the records of those changes"""

    def __init__(self, edits=False):
        self.edits = edits

    @staticmethod
    def _at(p, d):
        """-> (what stands for draft byte d at position p, inserted bases)"""
        other = "ACGT"[("ACGT".index(d) + 1 + p % 3) % 4] if d in "ACGT" else "A"
        m = p % 101
        if m == 7 or p % 500 == 250:
            return other, "GT" if p % 500 == 250 else ""
        if m == 40 or p % 500 in (251, 252):
            return "", ""
        if m == 70:
            return d, "TC"
        return d, ""

    def run(self, batch, windows=None):
        out, recs, roff, eoff = [], [], [0], [0]
        for g in range(batch.n_regions):
            a, b = int(batch.ref_start[g]), int(batch.ref_end[g])
            draft = batch.ref[batch.ref_off[g]:batch.ref_off[g + 1]].tobytes()[:b - a + 1].decode()
            s = ""
            for p in range(a + 201 if a > 0 else a, b + 1):
                d = draft[p - a]
                own, tail = self._at(p, d)
                s += own + tail
                if own != d:
                    recs.append((p, 0, pe.KIND_SUB if own else pe.KIND_DEL, ord(d), ord(own) if own else 0, p % 60))
                recs += [(p, i + 1, pe.KIND_INS, 0, ord(c), (p + i) % 50) for i, c in enumerate(tail)]
            out.append(s.encode())
            roff.append(roff[-1] + len(s))
            eoff.append(len(recs))
        res = polish.ChainResult(np.asarray(roff, np.int64), b"".join(out))
        return res._replace(edit_off=np.asarray(eoff, np.int64), edits=np.array(recs, pe.EDIT_DTYPE)) if self.edits else res

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """two contigs; no read of ctg2 touches 2300..5900, so two of its regions get none"""
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("edits_cpu")
    rng = np.random.default_rng(29)
    contigs = [("ctg2", "".join(rng.choice(list("ACGTN"), size=9_500, p=[.245, .245, .245, .245, .02]))),
               ("ctg10", "".join(rng.choice(list("ACGT"), size=3_300)))]
    bw.write_fasta(str(tmp / "r.fa"), contigs)
    recs = []
    for tid, (_, seq) in enumerate(contigs):
        recs += bw.random_records(rng, 60, len(seq), tid=tid, mean_len=1200)
    recs = [r for r in recs if r["tid"] != 0 or r["pos"] + bw.ref_len(r["cigar"]) <= 2_300 or r["pos"] > 5_900]
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    bw.write_bam(str(tmp / "r.bam"), [(n, len(s)) for n, s in contigs], recs)
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    return tmp, dict(contigs)


def _open(made):
    def open_chain(device, shared, state_dict, dtype, **kw):
        made.append(kw)
        return _EditingChain(**kw)
    return open_chain


def test_stub_chain_through_the_command(inputs):
    t, drafts = inputs
    base = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "3", "-bs", "8"]
    made = []
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "plain")]), open_chain=_open(made)) == 0
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "edits"), "--edits"]), open_chain=_open(made)) == 0
    assert made == [{}, {"edits": True}]                     # the keyword reaches the opener only when set
    assert os.listdir(str(t / "plain")) == ["_pepper_polished.fa"]
    assert sorted(os.listdir(str(t / "edits"))) == ["_pepper_polished.edits.vcf.gz", "_pepper_polished.edits.vcf.gz.tbi",
                                                    "_pepper_polished.fa"]
    fasta = open(str(t / "edits" / "_pepper_polished.fa")).read()
    assert fasta == open(str(t / "plain" / "_pepper_polished.fa")).read()
    header, cols, recs = er.parse_vcf(bamio.bgzf_read_all(str(t / "edits" / "_pepper_polished.edits.vcf.gz")).decode())
    assert header[:5] == ["fileformat=VCFv4.2", "source=pepper_thesis_amd polish", "reference=" + str(t / "r.fa"),
                          "contig=<ID=ctg2,length=9500>", "contig=<ID=ctg10,length=3300>"]
    # the regions without reads, found the reader's way: their kept ranges, adjacent ones as one line
    from pepper_thesis_amd import polish_summary
    bh, fh = bamio.BamHandler(str(t / "r.bam")), bamio.FastaHandler(str(t / "r.fa"))
    free = [(c, s, e) for c in ("ctg2", "ctg10") for s, e in polish.polish_intervals(len(drafts[c]))
            if polish_summary.region_from_files(bh, fh, c, s, e) is None]
    assert ("ctg2", 2900, 4100) in free and ("ctg2", 3900, 5100) in free and all(c == "ctg2" and s > 0 for c, s, _ in free)
    assert [s for _, s, _ in free] == list(range(free[0][1], free[-1][1] + 1, 1000))       # they are in a row: one run
    assert header[5:] == ["pepper_no_reads=ctg2:%d-%d" % (free[0][1] + 201 + 1, free[-1][2] + 1)]
    lines = fasta.split("\n")
    seqs = dict(zip((l[1:] for l in lines[0:-1:2]), lines[1:-1:2]))
    for c in ("ctg2", "ctg10"):
        mine = [r[1:] for r in recs if r[0] == c]
        assert len(mine) > 50 and all(r[3] is None for r in mine)
        assert er.apply(mine, drafts[c].encode(), er.no_read_ranges(header, c)) == seqs[c], c
        assert any(len(r[1]) > 2 and len(r[2]) > 2 for r in mine)     # the blocks around every 500th position


def test_overlapping_ranges_of_one_contig_are_refused_before_anything_is_written(inputs, capsys):
    t, _ = inputs
    base = ["-b", str(t / "r.bam"), "-f", str(t / "r.fa"), "-m", str(t / "m.npz"), "-t", "2", "-r", "ctg10:0-2000,ctg10:1000-3000"]
    made = []
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "twice"), "--edits"]), open_chain=_open(made)) == 2
    assert "ctg10" in capsys.readouterr().err and "--edits" not in made
    assert os.listdir(str(t / "twice")) == []
    assert polish.run(cli.polish_parser().parse_args(base + ["-o", str(t / "twice_plain")]), open_chain=_open(made)) == 0
