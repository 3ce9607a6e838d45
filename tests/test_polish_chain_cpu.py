"""CPU: the polish chain's result records (polish.ChainResult, polish.Piece), merge_pieces over either plane, and
polish_fused's refusal of a chain whose results lack a plane the run needs."""
import itertools
import os

import numpy as np
import pytest

from pepper_thesis_amd import build, polish, polish_edits as pe, synth

OFF = np.array([0, 3, 3, 7], np.int64)            # three regions, the middle one empty
BASES, QUAL = b"ACGTTGA", bytes([10, 20, 30, 40, 50, 60, 70])
EDIT_OFF = np.array([0, 2, 2, 3], np.int64)
EDITS = np.array([(5, 0, pe.KIND_SUB, 65, 67, 9), (6, 1, pe.KIND_INS, 0, 71, 255), (900, 0, pe.KIND_DEL, 84, 0, 3)], pe.EDIT_DTYPE)


def _result(off, bases, qual, edit_off, edits, with_qual, with_edits):
    return polish.ChainResult(off, bases, qual if with_qual else None, *((edit_off, edits) if with_edits else ()))


@pytest.mark.parametrize("with_qual,with_edits", list(itertools.product([False, True], repeat=2)))
def test_region_slices_every_present_plane(with_qual, with_edits):
    res = _result(OFF, BASES, QUAL, EDIT_OFF, EDITS, with_qual, with_edits)
    assert res.region_off is OFF and res.bases is BASES
    assert (res.qual is None) != with_qual and (res.edit_off is None) != with_edits and (res.edits is None) != with_edits
    want = [(b"ACG", QUAL[:3], EDITS[:2]), (b"", b"", EDITS[:0]), (b"TTGA", QUAL[3:], EDITS[2:])]
    for g, (b, q, e) in enumerate(want):
        got = res.region(g)
        assert len(got) == 3 and got[0] == b
        assert got[1] == (q if with_qual else None)
        assert (got[2] is None) if not with_edits else (got[2].dtype == pe.EDIT_DTYPE and got[2].tolist() == e.tolist())
        p = polish.Piece("ctg", 1000 * g, g, *got)
        assert (p.contig, p.start, p.index, p.bases) == ("ctg", 1000 * g, g, b) == tuple(p[:4])
        assert p.qual == got[1] and (p.edits is None) != with_edits
    with pytest.raises(IndexError):
        res.region(3)


def test_piece_and_result_defaults():
    assert polish.Piece("c", 0, 0, b"A") == ("c", 0, 0, b"A", None, None)
    assert polish.ChainResult(OFF, BASES)[2:] == (None, None, None)
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    assert polish.Piece._fields == ("contig", "start", "index", "bases", "qual", "edits")


def test_bases_is_anything_sliceable():
    chunks = [("img%d" % k, k) for k in range(5)]           # make_images keeps its chunk tuples in `bases`
    res = polish.ChainResult(np.array([0, 2, 2, 5]), chunks)
    assert [res.region(g)[0] for g in range(3)] == [chunks[:2], [], chunks[2:]]
    assert all(res.region(g)[1:] == (None, None) for g in range(3))


@pytest.mark.parametrize("with_qual,with_edits", list(itertools.product([False, True], repeat=2)))
def test_zero_region_result(with_qual, with_edits):
    zero = np.zeros(1, np.int64)
    res = _result(zero, b"", b"", zero.copy(), np.zeros(0, pe.EDIT_DTYPE), with_qual, with_edits)
    assert len(res.region_off) == 1 and res.bases == b""
    assert res.qual == (b"" if with_qual else None) and (res.edits is None) != with_edits
    with pytest.raises(IndexError):
        res.region(0)


def test_merge_pieces_over_the_quality_plane():
    pieces = [polish.Piece("c1", 900, 1, b"GG", b"\x01\x02"), polish.Piece("c2", 0, 3, b"T", b"\x09"),
              polish.Piece("c1", 0, 0, b"AA", b"\x03\x04"), polish.Piece("c1", 900, 2, b"CC", b"\x05\x06")]
    for ps in (pieces, pieces[::-1]):
        assert polish.merge_pieces(ps) == polish.merge_pieces(ps, part=3) == {"c1": b"AAGGCC", "c2": b"T"}
        assert polish.merge_pieces(ps, part=4) == {"c1": b"\x03\x04\x01\x02\x05\x06", "c2": b"\x09"}
    assert polish.merge_pieces(p[:4] for p in pieces) == {"c1": b"AAGGCC", "c2": b"T"}      # plain tuples still do
    assert polish.merge_pieces([]) == polish.merge_pieces([], part=4) == {}


class _PlainChain:
    """a chain made without planes: every region gives one base per draft column"""
    ctx = None

    def run(self, batch, windows=None):
        n = (batch.ref_end - batch.ref_start + 1).astype(np.int64)
        return polish.ChainResult(np.concatenate([[0], np.cumsum(n)]), b"A" * int(n.sum()))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import bam_writer as bw
    build.build_io()
    tmp = tmp_path_factory.mktemp("chain_cpu")
    rng = np.random.default_rng(3)
    seq = "".join(rng.choice(list("ACGT"), size=2_400))
    bw.write_fasta(str(tmp / "r.fa"), [("ctg", seq)])
    bw.write_bam(str(tmp / "r.bam"), [("ctg", len(seq))], sorted(bw.random_records(rng, 20, len(seq), tid=0, mean_len=600),
                                                                key=lambda r: r["pos"]))
    np.savez(str(tmp / "m.npz"), **synth.make_weights_p2(3))
    return tmp


@pytest.mark.parametrize("flags,plane", [(dict(qualities=True), "qual"), (dict(edits=True), "edits"),
                                         (dict(qualities=True, edits=True), "qual")])
def test_polish_fused_refuses_a_chain_without_the_plane(inputs, flags, plane):
    t = inputs
    out = str(t / ("out_" + "_".join(flags)))
    with pytest.raises(ValueError, match="no %s plane" % plane):
        polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), out, threads=2, chain=_PlainChain(), **flags)
    assert not os.path.exists(out) or os.listdir(out) == []
    # the same chain serves the run it was made for
    plain = str(t / "plain")
    path = polish.polish_fused(str(t / "r.bam"), str(t / "r.fa"), str(t / "m.npz"), plain, threads=2, chain=_PlainChain())
    assert os.listdir(plain) == ["_pepper_polished.fa"] and open(path).read().startswith(">ctg\nAAAA")
