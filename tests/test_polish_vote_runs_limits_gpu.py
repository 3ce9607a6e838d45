"""GPU: pv_polish_vote_runs[_dev] at the limits of its own kernels, on the cases of tests/vote_runs_limits_cases.py (what each
reaches is asserted on the CPU in test_polish_vote_runs_limits_cpu.py): read rounds of 256, up to 86 runs in the 88 slots of a tile,
runs and flanks on either side of a tile edge, regions that meet inside a tile, every CIGAR word, every chunk geometry,
PV_ERR_STATE, and the workspace from one batch to the next. Every case goes builder -> column vote -> run vote on the device
(the PV_ERR_STATE layouts are uploaded by hand), and labels, acc as bits and the six counters equal the host checker's
(tests/vote_runs_ref.py) in the device form and the host form, with and without acc. Nothing here has a tolerance.

No read had to be dropped for the builder: it takes N, P, H, = and X words, a CIGAR that ends in I and regions that overlap on
the draft as they are."""
import ctypes as C

import numpy as np
import pytest
import torch

import chunk_geometry_cases as cg
import min_qual_cases as mc
import vote_runs_limits_cases as Z
import vote_runs_ref as rr
from pepper_thesis_amd import _ffi
from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut
from test_polish_vote_runs_gpu import _Chain, _bits, _check

pytestmark = pytest.mark.gpu


def _case(ctx, c):
    ch, lab, cnt, runs = _check(ctx, c.batch, c.L, c.O, c.min_run)
    assert cnt[1:3] == [0, -1]
    return ch, lab, cnt, runs


# ---- 1. read rounds -----------------------------------------------------------------------------------------------------------------

def test_rounds_of_256_reads(hip_ctx):
    """600 reads: a round of which tile 1 keeps none, a round both tiles keep whole, a last round of 88; the winners need all three"""
    c = Z.rounds()
    ch, lab, cnt, runs = _case(hip_ctx, c)
    assert cnt == [3, 0, -1, 2, 3, 0] and [r.L for r in runs] == [5, 9, 3] and max(r.S for r in runs) > Z.ROUND
    assert not np.array_equal(lab, ch.lab0)


def test_255_256_and_257_voters(hip_ctx):
    ch, lab, cnt, runs = _case(hip_ctx, Z.round_counts())
    assert cnt == [3, 0, -1, 2, 3, 0] and [(r.V, r.L) for r in runs] == [(255, 5), (256, 6), (257, 5)]


# ---- 2. slots -----------------------------------------------------------------------------------------------------------------------

def test_86_runs_start_in_one_tile(hip_ctx):
    ch, lab, cnt, runs = _case(hip_ctx, Z.slots())
    assert cnt[0] == cnt[4] == 233 and cnt[3] >= 40 and cnt[5] == 0
    # at min_run 3 the same batch has no candidate: nothing is written
    ch, lab, cnt, runs = _case(hip_ctx, Z.slots(3))
    assert cnt == [0, 0, -1, 0, 0, 0] and np.array_equal(lab, ch.lab0)
    lab, acc, cnt = ch.run(3)
    assert np.array_equal(lab, ch.lab0) and np.array_equal(_bits(acc), _bits(ch.acc0))


def test_the_workspace_from_a_large_batch_to_a_small_one_and_back(hip_ctx):
    """the runs.* buffers of the 700-byte batch serve the 90-byte batch behind it: what the first left there (cover, dec_L,
    row_of) is not the second's"""
    want = None
    for c in (Z.slots(), Z.small(), Z.slots()):
        ch, lab, cnt, runs = _case(hip_ctx, c)
        if c is Z.small():
            assert cnt == [2, 0, -1, 2, 2, 0]
        elif want is None:
            want = (lab.tobytes(), cnt)
        else:
            assert (lab.tobytes(), cnt) == want


# ---- 3. tile edges and region edges ------------------------------------------------------------------------------------------------

def test_runs_and_flanks_on_either_side_of_a_tile_edge(hip_ctx):
    ch, lab, cnt, runs = _case(hip_ctx, Z.tile_edges())
    assert cnt == [5, 0, -1, 4, 7, 2] and [(r.s, r.L) for r in runs] == [(208, 50), (511, 5), (768, 7), (1000, 48), (1301, 2)]


@pytest.mark.parametrize("across", [False, True], ids=["region_5_starts_tile_1", "region_5_across_byte_256"])
def test_regions_that_meet_inside_a_tile(hip_ctx, across):
    ch, lab, cnt, runs = _case(hip_ctx, Z.regions_in_a_tile(across))
    assert cnt == [4, 0, -1, 4, 6, 0] and [(r.region, r.L) for r in runs if r.L is not None] == [(0, 39), (4, 3), (5, 4), (6, 7)]


# ---- 4. CIGAR words -----------------------------------------------------------------------------------------------------------------

def test_every_cigar_word(hip_ctx):
    ch, lab, cnt, runs = _case(hip_ctx, Z.cigar_words())
    assert cnt == [3, 0, -1, 2, 3, 0] and [(r.L, r.S - r.V) for r in runs] == [(7, 1), (4, 0), (4, 0)]


# ---- 5. chunk geometries ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo", cg.GEOMETRIES, ids=cg.geo_id)
def test_runs_on_the_chunk_boundaries_of_every_geometry(hip_ctx, geo):
    c = Z.geometry(*geo)
    ch, lab, cnt, runs = _case(hip_ctx, c)                               # (_check: both copies of a shared row agree)
    assert cnt == [3, 0, -1, 2, 3, 0]
    grow = c.where["grow"]
    lay = mc.Layout([(0, c.batch.ref.tobytes(), {grow - 1: 2, grow + 1: 2})], *geo)
    assert np.array_equal(ch.position, lay.position) and np.array_equal(ch.index, lay.index)   # the layout the CPU test looked at


# ---- 6. PV_ERR_STATE ------------------------------------------------------------------------------------------------------------------

class _Uploaded(_Chain):
    """_Chain over a hand-made layout: the chunk arrays uploaded as they are, arbitrary labels 0..4 and floats as the planes"""

    def __init__(self, ctx, batch, lay):
        self.ctx, self.batch, self.L, self.O, self.n = ctx, batch, lay.L, lay.O, lay.n
        self.db = DeviceBatch(batch)
        self.do = DevicePolishOut(lay.n, lay.L, lay.O)
        for name in ("position", "index", "region", "chunk_id"):
            getattr(self.do, name)[:lay.n].copy_(torch.from_numpy(np.array(getattr(lay, name))))
        rng = np.random.default_rng(lay.n)
        self.lab0 = rng.integers(0, 5, (lay.n, lay.L)).astype(np.uint8)
        self.acc0 = (rng.random((lay.n, lay.L, 5), dtype=np.float32) * np.float32(2.0)).astype(np.float32)
        self.lab, self.acc = torch.from_numpy(self.lab0).cuda(), torch.from_numpy(self.acc0).cuda()
        self.cnt = torch.full((6,), -7, dtype=torch.int64, device="cuda")
        self.common = (self.db.t["ref_start"].data_ptr(), self.db.t["ref_off"].data_ptr(), self.db.t["ref"].data_ptr(), batch.n_regions)
        self.position, self.index, self.region, self.chunk_id = lay.position, lay.index, lay.region, lay.chunk_id
        self.out = lay.out
        torch.cuda.synchronize()


def test_a_layout_one_insert_row_short_is_pv_err_state(hip_ctx):
    c = Z.state()
    seen, skipped = c.runs[1:]
    # with the two insert rows the winner needs, the hand-made layout is voted like any other: every row outside the two runs
    # comes back bit for bit
    ch = _Uploaded(hip_ctx, c.batch, mc.Layout(c.enough, c.L, c.O))
    w_lab, w_acc, w_cnt, _ = ch.want()
    assert w_cnt == [2, 0, -1, 2, seen, skipped]
    for acc in (True, False):
        lab, a, cnt = ch.run(acc=acc)
        assert cnt == w_cnt and np.array_equal(lab, w_lab) and np.array_equal(_bits(a), _bits(w_acc if acc else ch.acc0))
        lab, a, cnt = ch.host(acc=acc)
        assert cnt == w_cnt and np.array_equal(lab, w_lab) and (a is None or np.array_equal(_bits(a), _bits(w_acc)))
    # one row short
    ch = _Uploaded(hip_ctx, c.batch, mc.Layout(c.short, c.L, c.O))
    with pytest.raises(rr.BadState):
        ch.want()
    want = [0, _ffi.PV_ERR_STATE, -1, 0, seen, skipped]
    for acc in (True, False):
        lab, a, cnt = ch.run(acc=acc)
        assert cnt == want and np.array_equal(lab, ch.lab0) and np.array_equal(_bits(a), _bits(ch.acc0))
        h_lab, h_acc, cnt6 = ch.lab0.copy(), ch.acc0.copy() if acc else None, (C.c_int64 * 6)()
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.polish_vote_runs(ch.out, ch.batch, h_lab, h_acc, 3, c.L, c.O, counts=cnt6)
        assert e.value.code == _ffi.PV_ERR_STATE and "more insert rows" in str(e.value) and list(cnt6) == want
        assert np.array_equal(h_lab, ch.lab0) and (h_acc is None or np.array_equal(_bits(h_acc), _bits(ch.acc0)))
    # a broken chunk id as well: the layout's verdict comes first
    bad = ch.n - 1
    cid = np.array(ch.chunk_id)
    cid[bad] += 5
    ch.do.chunk_id[:ch.n].copy_(torch.from_numpy(cid))
    with pytest.raises(rr.BadChunk) as e:
        rr.vote_runs(c.batch, ch.position, ch.index, ch.region, cid, ch.lab0, ch.acc0, c.O, 3)
    assert e.value.chunk == bad
    lab, a, cnt = ch.run()
    assert cnt == [0, _ffi.PV_ERR_INVALID, bad, 0, seen, skipped]
    assert np.array_equal(lab, ch.lab0) and np.array_equal(_bits(a), _bits(ch.acc0))
