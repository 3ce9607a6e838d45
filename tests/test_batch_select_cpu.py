"""CPU: the host checker of the haplotype selection (tests/select_ref.py) on hand-worked batches with the expected arrays
written out, and against RegionBatch.region() / pack_regions of the kept reads. The device forms are compared with this checker
in test_batch_select_gpu.py."""
import numpy as np
import pytest

import select_ref as sel
from pepper_thesis_amd import _ffi
from pepper_thesis_amd.batch import Read, Region, pack_regions


def _batch():
    """3 regions, 4 + 2 + 3 reads; read i has i + 1 bases (the byte 10 * i + k at place k) and 1 + i % 2 cigar words
    (100 * i + k); tags
        region 0: 0  1  2  3      region 1: 2  2      region 2: 0 -1  1
    so haplotype 1 empties region 1, haplotype 2 keeps it whole, and nothing is dropped from region 2 but the -1."""
    n = 9
    lens, clens = np.arange(1, n + 1), 1 + np.arange(n) % 2
    b = sel.make_batch(lens, clens, [4, 2, 3], [0, 1, 2, 3, 2, 2, 0, -1, 1])
    b.bases = np.concatenate([10 * i + np.arange(i + 1) for i in range(n)]).astype(np.uint8)
    b.quals = (b.bases + 1).astype(np.uint8)
    b.cigar = np.concatenate([100 * i + np.arange(1 + i % 2) for i in range(n)]).astype(np.uint32)
    b.read_pos = np.arange(1000, 1000 + n, dtype=np.int64)
    b.read_flags = (np.arange(n) % 2).astype(np.uint8)
    b.read_mapq = (np.arange(n) + 20).astype(np.uint8)
    return b


def test_haplotype_1_written_out():
    b = _batch()
    out, src = sel.select(b, 1)
    assert src.tolist() == [0, 1, 6, 8]
    assert out.read_off.tolist() == [0, 2, 2, 4]                     # region 1 is emptied
    assert out.read_pos.tolist() == [1000, 1001, 1006, 1008]
    assert out.read_flags.tolist() == [0, 1, 0, 0] and out.read_mapq.tolist() == [20, 21, 26, 28]
    assert out.read_hp.tolist() == [0, 1, 0, 1]
    assert out.base_off.tolist() == [0, 1, 3, 10, 19]
    assert out.bases.tolist() == [0, 10, 11] + list(range(60, 67)) + list(range(80, 89))
    assert out.quals.tolist() == [v + 1 for v in out.bases.tolist()]
    assert out.cigar_off.tolist() == [0, 1, 3, 4, 5]
    assert out.cigar.tolist() == [0, 100, 101, 600, 800]
    for f in ("ref_start", "ref_end", "cand_start", "cand_end", "ref_off", "ref"):      # the input's own arrays
        assert getattr(out, f) is getattr(b, f)
    assert b.n_reads == 9 and b.read_off.tolist() == [0, 4, 6, 9]    # the input is not altered


def test_haplotype_2_written_out():
    b = _batch()
    out, src = sel.select(b, 2)
    assert src.tolist() == [0, 2, 4, 5, 6]
    assert out.read_off.tolist() == [0, 2, 4, 5]                     # region 1 is untouched: both of its reads
    assert out.read_hp.tolist() == [0, 2, 2, 2, 0]
    assert out.base_off.tolist() == [0, 1, 4, 9, 15, 22]
    assert out.bases.tolist() == [0, 20, 21, 22] + list(range(40, 45)) + list(range(50, 56)) + list(range(60, 67))
    assert out.cigar_off.tolist() == [0, 1, 2, 3, 5, 6]
    assert out.cigar.tolist() == [0, 200, 400, 500, 501, 600]
    g1_in, g1_out = b.region(1), out.region(1)
    assert [(r.pos, r.bases, r.cigar.tolist(), r.hp_tag) for r in g1_in.reads] == [(r.pos, r.bases, r.cigar.tolist(), r.hp_tag) for r in g1_out.reads]


def test_other_values_are_in_no_haplotype():
    b = _batch()
    out, src = sel.select(b, 3)                                      # a third haplotype exists by the rule
    assert src.tolist() == [0, 3, 6]
    b.read_hp = np.array([2**31 - 1, -1, 3, 4, 5, 6, 7, 8, 9], np.int32)
    for h in (1, 2):
        out, src = sel.select(b, h)
        assert len(src) == 0 and out.read_off.tolist() == [0, 0, 0, 0] and out.base_off.tolist() == [0] and out.cigar_off.tolist() == [0]
        assert out.n_reads == 0 and out.n_bases == 0 and out.n_cigar == 0
    with pytest.raises(AssertionError):
        sel.select(b, 0)


def test_untagged_batches_are_the_identity():
    b = _batch()
    for hp in (None, np.zeros(9, np.int32), np.full(9, 2, np.int32)):
        b.read_hp = hp
        out, src = sel.select(b, 2)
        assert src.tolist() == list(range(9))
        for f in sel.READ_FIELDS:
            got, want = getattr(out, f), getattr(b, f)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f
        assert (out.read_hp is None) == (hp is None)


@pytest.mark.parametrize("haplotype", [1, 2])
def test_checker_against_pack_regions_of_the_kept_reads(haplotype):
    rng = np.random.default_rng(5)
    per = rng.integers(0, 6, 40)
    per[[0, 7, 39]] = [3, 0, 2]
    n = int(per.sum())
    lens = rng.choice([0, 1, 2, 15, 16, 17, 40], n)
    b = sel.make_batch(lens, rng.integers(0, 4, n), per, rng.choice([0, 1, 2, 3, -1], n), seed=6)
    out, src = sel.select(b, haplotype)
    regions = []
    for g in range(b.n_regions):
        reg = b.region(g)
        reads = [r for r in reg.reads if r.hp_tag in (0, haplotype)]
        regions.append(Region(reg.ref_start, reg.ref_end, reg.ref, reads, reg.cand_start, reg.cand_end, reg.contig))
    want = pack_regions(regions)
    assert 0 < want.n_reads < n and (np.diff(want.read_off) == 0).any()
    for f in sel.READ_FIELDS + ("ref_start", "ref_end", "ref_off", "ref"):
        assert getattr(out, f).tobytes() == getattr(want, f).tobytes(), f
    assert want.read_hp is not None and out.read_hp.tolist() == want.read_hp.tolist()
    assert np.array_equal(b.read_pos[src], out.read_pos)


def test_the_binding_and_its_struct_are_declared():
    names = [s[0] for s in _ffi.SYMBOLS]
    assert "pv_batch_select_hp" in names and "pv_batch_select_hp_dev" in names
    fields = [f for f, _ in _ffi.pv_select_out._fields_]
    assert fields[:3] == ["read_capacity", "base_capacity", "cigar_capacity"] and fields[-5:] == ["read_hp", "src_read", "n_reads",
                                                                                                  "n_bases", "n_cigar"]
