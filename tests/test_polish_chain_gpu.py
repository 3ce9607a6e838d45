"""GPU: the device chain's one launch path (polish._DeviceChain._labels_and_stitch) for every combination of --qualities
and --edits on the same small batch: the planes a chain was not made for are absent, and the ones it shares with another
chain are the same bytes. What the planes must hold is checked against the host checkers in test_polish_qual_gpu.py and
test_polish_edits_gpu.py; nothing here has a tolerance."""
import numpy as np
import pytest

from pepper_thesis_amd import _ffi, polish, polish_edits as pe, synth
from pepper_thesis_amd.batch import Region, pack_regions

pytestmark = pytest.mark.gpu
COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (qualities, edits)
READLESS = 1


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """one contig of 3,300 bases, so four overlapping regions (two of them interior: the overlap drop and chunk seams are
    active), about 40 reads of ~400 bases, none touching region 1 ([900, 2100]); seeded P2 weights.
    The reader leaves a region without reads out of a launch. Here it is packed into the batch, between regions that have
    reads: the builder gives it chunks of zero rows, the launch path sees them like any others."""
    import bam_writer as bw
    from pepper_thesis_amd import build
    from pepper_thesis_amd.bamio import BamHandler, FastaHandler
    from pepper_thesis_amd.polish_summary import region_from_files
    build.build_io()
    tmp = tmp_path_factory.mktemp("chain")
    rng = np.random.default_rng(41)
    seq = "".join(rng.choice(list("ACGT"), size=3_300))
    bw.write_fasta(str(tmp / "ref.fa"), [("ctg", seq)])
    recs = [r for r in bw.random_records(rng, 90, len(seq), tid=0, mean_len=400)
            if r["pos"] + bw.ref_len(r["cigar"]) <= 900 or r["pos"] > 2_100]
    assert 30 <= len(recs) <= 50
    bw.write_bam(str(tmp / "reads.bam"), [("ctg", len(seq))], sorted(recs, key=lambda r: r["pos"]))
    np.savez(str(tmp / "model.npz"), **synth.make_weights_p2(31, 3.0))
    b, f = BamHandler(str(tmp / "reads.bam")), FastaHandler(str(tmp / "ref.fa"))
    ivs = polish.polish_intervals(len(seq))
    assert ivs == [(0, 1100), (900, 2100), (1900, 3100), (2900, 3299)]
    regs = [region_from_files(b, f, "ctg", s, e) for s, e in ivs]
    assert [r is None for r in regs] == [g == READLESS for g in range(4)]
    s, e = ivs[READLESS]
    regs[READLESS] = Region(s, e, seq[s:e + 1].encode(), [], contig="ctg")
    return pack_regions(regs), polish.load_polish_model(str(tmp / "model.npz"))


def test_every_combination_through_the_one_launch_path(batch, hip_ctx, opts):
    """The launch without chunks (n == 0) is entered at _labels_and_stitch itself: the builder gives every region of a batch
    chunks, with or without reads, so no batch size brings run() there."""
    b, state = batch
    opts(shared_device=1)
    hip_ctx.load_p2(state, _ffi.PV_DTYPE_F32)
    res, empty = {}, {}
    for q, e in COMBOS:
        chain = polish._DeviceChain(hip_ctx, qualities=q, edits=e)
        res[q, e] = chain.run(b)                                  # all four regions in one launch
        empty[q, e] = chain._labels_and_stitch(None, 0, 3)
    plain = res[False, False]
    assert isinstance(plain, polish.ChainResult) and plain.region_off.dtype == np.int64 and len(plain.region_off) == 5
    assert plain.region_off[0] == 0 and (np.diff(plain.region_off) >= 0).all() and plain.region_off[-1] == len(plain.bases) > 0
    assert set(plain.bases) <= set(b"ACGT")
    for (q, e), r in res.items():
        assert np.array_equal(r.region_off, plain.region_off) and r.bases == plain.bases, (q, e)
        assert (r.qual is None) != q and (r.edit_off is None) != e and (r.edits is None) != e, (q, e)
        for g in range(4):                                        # a region's share holds the planes the result holds
            part = r.region(g)
            assert part[0] == plain.bases[plain.region_off[g]:plain.region_off[g + 1]]
            assert (part[1] is None) != q and (part[2] is None) != e
            assert not q or len(part[1]) == len(part[0])
    qual = res[True, False].qual
    assert qual == res[True, True].qual and len(qual) == len(plain.bases) and max(qual) <= 93 and len(set(qual)) > 1
    ed, edq = res[False, True], res[True, True]
    assert np.array_equal(ed.edit_off, edq.edit_off) and len(ed.edit_off) == 5 and ed.edit_off[0] == 0
    assert (np.diff(ed.edit_off) >= 0).all() and ed.edit_off[-1] == len(ed.edits) == len(edq.edits) > 0
    assert ed.edits.dtype == edq.edits.dtype == pe.EDIT_DTYPE
    for name in ("position", "index", "kind", "draft", "base"):
        assert np.array_equal(ed.edits[name], edq.edits[name]), name
    assert (ed.edits["qual"] == 255).all() and (edq.edits["qual"] <= 93).all()
    for (q, e), r in empty.items():
        assert isinstance(r, polish.ChainResult) and r.region_off.tolist() == [0, 0, 0, 0] and r.bases == b"", (q, e)
        assert r.qual == (b"" if q else None)
        assert (r.edit_off.tolist() == [0, 0, 0, 0] and r.edits.dtype == pe.EDIT_DTYPE and len(r.edits) == 0) if e else (
            r.edit_off is None and r.edits is None)
        part = r.region(1)
        assert part[:2] == (b"", b"" if q else None) and ((len(part[2]) == 0) if e else part[2] is None)
