"""GPU: the BAM record decode kernels (csrc/bam_decode.hip) at their own limits, through direct calls of Context.bam_scan_dev
and Context.bam_fill_dev on plain bytes and tables (bam_decode_cases), integer for integer and byte for byte against the
restatement (bam_decode_ref): the CIGAR clip at its 64-operation turn seams, the aux walk at its 64-byte turns, block
geometry, every per-interval status and both calls' refusals, the pass sizes of the block-wide scans, the fill's capacities.

The harness does what a caller must: scan, counts to the host, outputs sized from them, fill. `data`, the workspace and every
output lie between guard bands filled with a canary, and every test ends by checking them. A malformed table is made by
passing a size or an offset too small for the table, never by allocating less: no case here is meant to fault."""
import numpy as np
import pytest

import bam_decode_cases as cases
import bam_decode_ref as ref
from pepper_thesis_amd import _ffi

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD, DATA_GUARD, WS_GUARD = 4096, 128 * 1024, 64 * 1024
TABLES = ("data", "coffset", "next_coffset", "out_off", "isize", "blk_status", "iv_tid", "iv_rs", "iv_re", "iv_blk0", "iv_blk1",
          "iv_chunk_off", "chunk_beg", "chunk_end", "iv_dropped", "iv_rec_off")
OUT_ITEM = dict(read_pos=8, read_flags=1, read_mapq=1, read_hp=4, base_off=8, cigar_off=8, bases=1, quals=1, cigar=4)
OUT_DTYPE = dict(read_pos=np.int64, read_flags=np.uint8, read_mapq=np.uint8, read_hp=np.int32, base_off=np.int64, cigar_off=np.int64,
                 bases=np.uint8, quals=np.uint8, cigar=np.uint32)


class Buf:
    """n bytes of device memory between two guard bands, canary everywhere but under `init`"""

    def __init__(self, n, dev, init=None, guard=GUARD):
        import torch
        self.n, self.g = int(n), guard
        self.t = torch.full((guard + self.n + (-self.n) % 8 + guard,), CANARY, dtype=torch.uint8, device=dev)
        if init is not None and self.n:
            self.t[guard:guard + self.n] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1).copy())
        self.ptr = self.t.data_ptr() + guard

    def host(self, dtype=np.uint8):
        return self.t[self.g:self.g + self.n].cpu().numpy().view(dtype)

    def intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:self.g] == CANARY).all() and (h[self.g + self.n:] == CANARY).all())


class Run:
    """one scan and its fills: the tables on the device, the workspace, the counts, the outputs"""

    def __init__(self, ctx, t, stream=None):
        import torch
        self.ctx, self.t, self.dev = ctx, t, "cuda:%d" % ctx.device_id
        self.stream = stream
        self.bufs = {k: Buf(t[k].nbytes, self.dev, t[k], DATA_GUARD if k == "data" else GUARD) for k in TABLES}
        self.N = int(t["n_intervals"])
        slots = max(int(t["iv_rec_off"].max()), int(t["rec_slots"]), 0)     # the workspace is never smaller than any table asks
        self.ws_need = int(ctx.lib.pv_bam_decode_ws_bytes(self.N, int(t["rec_slots"])))
        self.bufs["ws"] = Buf(int(ctx.lib.pv_bam_decode_ws_bytes(max(self.N, 0), slots)) + 16, self.dev, guard=WS_GUARD)
        self.bufs["counts"] = Buf(64 * max(self.N, 1), self.dev)
        cin = self.cin = _ffi.pv_bam_decode_in()
        for k in TABLES:
            setattr(cin, k, self.bufs[k].ptr)
        for k in ("data_bytes", "n_blocks", "n_intervals", "include_supplementary", "min_mapq", "rec_slots", "n_chunks"):
            setattr(cin, k, int(t[k]))
        torch.cuda.synchronize()

    def _sync(self):
        import torch
        torch.cuda.synchronize()

    def scan(self, cin=None, ws=None, ws_bytes=None):
        b = self.bufs
        self.ctx.bam_scan_dev(self.cin if cin is None else cin, b["ws"].ptr if ws is None else ws, b["ws"].n if ws_bytes is None else ws_bytes,
                              b["counts"].ptr, self.stream.cuda_stream if self.stream else 0)
        self._sync()
        return b["counts"].host(np.int64).reshape(-1, 8)[:self.N]

    def fill(self, reg_iv, read_off, sel_off, sel, base_cap, cigar_cap, alloc_bases=None, alloc_cigar=None, n_reads=None, n_sel=None):
        """-> the output arrays (their whole allocation) and the totals"""
        n = int(read_off[-1])
        alloc_bases = base_cap if alloc_bases is None else alloc_bases
        alloc_cigar = cigar_cap if alloc_cigar is None else alloc_cigar
        count = dict(read_pos=n, read_flags=n, read_mapq=n, read_hp=n, base_off=n + 1, cigar_off=n + 1, bases=alloc_bases, quals=alloc_bases, cigar=alloc_cigar)
        o = {k: Buf(OUT_ITEM[k] * count[k], self.dev) for k in OUT_ITEM}
        o["totals"] = Buf(32, self.dev)
        n_sel = len(sel) if n_sel is None else n_sel
        sel = np.asarray(sel if len(sel) else [0], np.int64)
        args = dict(reg_iv=np.asarray(reg_iv, np.int32), read_off=np.asarray(read_off, np.int64), sel_off=np.asarray(sel_off, np.int64), sel=sel)
        for k, v in args.items():
            o["_" + k] = Buf(v.nbytes, self.dev, v)
        out = _ffi.pv_batch_in()
        for k in OUT_ITEM:
            if k != "read_hp":
                setattr(out, k, o[k].ptr)
        self.outs = o
        self._sync()
        self.ctx.bam_fill_dev(self.cin, self.bufs["ws"].ptr, self.bufs["ws"].n, len(reg_iv), o["_reg_iv"].ptr, o["_read_off"].ptr, o["_sel_off"].ptr,
                              o["_sel"].ptr, n_sel, n if n_reads is None else n_reads, base_cap, cigar_cap, out, o["read_hp"].ptr, o["totals"].ptr,
                              self.stream.cuda_stream if self.stream else 0)
        self._sync()
        return {k: o[k].host(OUT_DTYPE[k]) for k in OUT_ITEM}, o["totals"].host(np.int64)

    def intact(self):
        bad = [k for k, b in list(self.bufs.items()) + list(getattr(self, "outs", {}).items()) if not b.intact()]
        assert not bad, "written outside: %s" % bad


def canary_of(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, CANARY, np.uint8).view(dtype)


def check_scan(L, t, counts, special=()):
    for i, iv in enumerate(L.ivs):
        if i not in special:
            assert counts[i].tolist() == L.expected_counts(t, i), (i, iv["name"], counts[i].tolist())


def check_fill(got, totals, exp, base_cap, cigar_cap, status):
    """every array, whole: what the restatement holds where a read is written, the canary everywhere else"""
    n = len(exp["written"])
    nb, nc = np.diff(exp["base_off"]), np.diff(exp["cigar_off"])
    assert totals.tolist() == [n, int(exp["base_off"][-1]), int(exp["cigar_off"][-1]), status], totals.tolist()
    np.testing.assert_array_equal(got["base_off"], exp["base_off"])
    np.testing.assert_array_equal(got["cigar_off"], exp["cigar_off"])
    w = exp["written"] & (exp["base_off"][1:] <= base_cap) & (exp["cigar_off"][1:] <= cigar_cap)
    for k in ("read_pos", "read_flags", "read_mapq", "read_hp"):
        np.testing.assert_array_equal(got[k], np.where(w, exp[k], canary_of(OUT_DTYPE[k], n)), err_msg=k)
    for k, per, src in (("bases", nb, exp["bases"]), ("quals", nb, exp["quals"]), ("cigar", nc, exp["cigar"])):
        want = canary_of(OUT_DTYPE[k], len(got[k]))
        m = np.repeat(w, per)
        assert len(m) == len(src) <= len(want), k
        want[:len(src)][m] = src[m]
        np.testing.assert_array_equal(got[k], want, err_msg=k)
    return int(w.sum())


def regions_of(L, pick=None):
    """[(interval, None)] for every interval the restatement decodes without a status (or those of `pick`)"""
    return [(i, None) for i, iv in enumerate(L.ivs) if iv["exp"]["status"] == ref.OK and (pick is None or i in pick)]


def fill_and_check(run, L, regions, base_cap=None, cigar_cap=None, status=_ffi.PV_OK, reg_iv=None):
    exp = cases.expected_fill(L, regions)
    sel_off, sel = [], []
    for i, s in regions:
        sel_off.append(-1 if s is None else len(sel))
        sel += [] if s is None else list(s)
    full_b, full_c = int(exp["base_off"][-1]), int(exp["cigar_off"][-1])
    base_cap = full_b if base_cap is None else base_cap
    cigar_cap = full_c if cigar_cap is None else cigar_cap
    reg_iv = [i for i, _ in regions] if reg_iv is None else reg_iv
    got, totals = run.fill(reg_iv, exp["read_off"], sel_off, sel, base_cap, cigar_cap, full_b + 8, full_c + 8)
    n = check_fill(got, totals, exp, base_cap, cigar_cap, status)
    run.intact()
    return n


def decode(ctx, L, stream=None):
    """the whole contract on one launch: checks of the cases, scan, counts, fill of every good interval, canaries"""
    L.checks()
    t = L.tables()
    run = Run(ctx, t, stream)
    counts = run.scan()
    check_scan(L, t, counts)
    regions = regions_of(L)
    assert fill_and_check(run, L, regions) == sum(len(L.ivs[i]["exp"]["reads"]) for i, _ in regions) > 0
    return run, counts


# ---- a, b, c -------------------------------------------------------------------------------------------------------------------

def test_cigar_clip_at_the_turn_seams(hip_ctx):
    L = cases.clip_launch()
    run, counts = decode(hip_ctx, L)
    st = [iv["exp"]["status"] for iv in L.ivs]
    assert st.count(ref.CIGAR_LONGER) == 4 and counts[:, 3].tolist() == st


def test_aux_fields_at_the_turn_seams(hip_ctx):
    decode(hip_ctx, cases.aux_launch())


def test_block_geometry(hip_ctx):
    L = cases.geometry_launch()
    assert len(L.ivs) > 450
    run, counts = decode(hip_ctx, L)
    assert counts[:, 3].tolist().count(ref.PAST_PLAN) == 2


# ---- d. statuses ------------------------------------------------------------------------------------------------------------------

def test_statuses_from_the_tables(hip_ctx):
    all_cases = cases.status_cases()
    assert len(all_cases) == 18
    for c in all_cases:
        L, bad = c["launch"], c["bad"]
        L.checks()
        t = L.tables()
        st, blk0, off = L.groups[c["g"]]
        if c["tamper"]:
            c["tamper"](t, blk0)
        run = Run(hip_ctx, t)
        counts = run.scan()
        check_scan(L, t, counts, special=(bad,))
        assert counts[bad, 3] == c["status"], (c["name"], counts[bad].tolist())
        for col, v in c["detail"].items():
            v = L.reported_voff(t, off + st.starts[1]) if v == "record 1" else v
            assert counts[bad, col] == v, (c["name"], col, counts[bad].tolist())
        good = [i for i in range(3) if i != bad]
        assert fill_and_check(run, L, [(i, None) for i in good]) == 6, c["name"]


def _refused(code, fn):
    with pytest.raises(_ffi.PepperHipError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_the_calls_own_refusals(hip_ctx):
    L, _ = cases.status_launch(cases.good_records(400))
    t = L.tables()
    run = Run(hip_ctx, t)

    def with_(**kw):
        c = type(run.cin).from_buffer_copy(run.cin)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for k in ("iv_tid", "iv_rec_off", "iv_dropped", "coffset", "blk_status", "data", "chunk_beg", "chunk_end"):
        _refused(_ffi.PV_ERR_INVALID, lambda: run.scan(cin=with_(**{k: None})))
    for k in ("n_intervals", "n_blocks", "data_bytes", "rec_slots", "n_chunks"):
        _refused(_ffi.PV_ERR_INVALID, lambda: run.scan(cin=with_(**{k: -1})))
    _refused(_ffi.PV_ERR_CAPACITY, lambda: run.scan(ws_bytes=run.ws_need - 1))
    _refused(_ffi.PV_ERR_INVALID, lambda: run.scan(ws=run.bufs["ws"].ptr + 4, ws_bytes=run.ws_need))
    _refused(_ffi.PV_ERR_INVALID, lambda: run.scan(ws=0, ws_bytes=run.ws_need))
    assert (run.bufs["counts"].host() == CANARY).all() and (run.bufs["ws"].host() == CANARY).all()   # refused: nothing ran
    run.intact()
    counts = run.scan(ws_bytes=run.ws_need)      # exactly enough is enough
    check_scan(L, t, counts)
    exp = cases.expected_fill(L, regions_of(L))
    for n_reads in (0, int(t["rec_slots"]) + 1):
        _refused(_ffi.PV_ERR_INVALID, lambda: run.fill([0, 1, 2], exp["read_off"], [-1, -1, -1], [], 64, 64, n_reads=n_reads))
        assert all((run.outs[k].host() == CANARY).all() for k in OUT_ITEM) and (run.outs["totals"].host() == CANARY).all()
    assert fill_and_check(run, L, regions_of(L)) == 9


# ---- e. pass sizes of the scans ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_interval_numbering_across_passes(hip_ctx, n):
    L = cases.intervals_launch(n)
    assert len(L.ivs) == n and [L.ivs[i]["exp"]["n_rec"] for i in (0, n // 2, n - 1)] == [0, 0, 0]
    decode(hip_ctx, L)


def test_kept_numbering_across_passes(hip_ctx):
    L = cases.records_launch()
    assert [iv["exp"]["n_rec"] for iv in L.ivs] == [255, 256, 257, 600]
    run, _ = decode(hip_ctx, L)
    rng = np.random.default_rng(3)
    # every kept read by its number, backwards and shuffled: kept[] must hold the right record behind every number
    regions = [(i, rng.permutation(len(iv["exp"]["reads"])).tolist()) for i, iv in enumerate(L.ivs)]
    fill_and_check(run, L, regions)
    fill_and_check(run, L, [(i, list(range(len(iv["exp"]["reads"])))[::-1]) for i, iv in enumerate(L.ivs)])


@pytest.mark.parametrize("total", [1023, 1024, 1025, 2049])
def test_fill_offsets_across_passes(hip_ctx, total):
    L = cases.fill_launch(total)
    kept = [len(iv["exp"]["reads"]) for iv in L.ivs]
    assert sum(kept) == total and kept[1] == 0
    run, _ = decode(hip_ctx, L)                                   # record order, the empty region included
    rng = np.random.default_rng(total)
    assert fill_and_check(run, L, [(i, rng.permutation(k).tolist()) for i, k in enumerate(kept)]) == total
    L2 = cases.fill_launch(total + 50)                            # a reservoir subset of `total` reads out of total + 50
    kept2 = [len(iv["exp"]["reads"]) for iv in L2.ivs]
    take = [kept2[0] - 30, 0, kept2[2] - 18, 5]
    assert sum(take) == total
    run2, _ = decode(hip_ctx, L2)
    assert fill_and_check(run2, L2, [(i, rng.choice(k, m, replace=False).tolist()) for i, (k, m) in enumerate(zip(kept2, take))]) == total


def test_capped_grids_take_a_second_turn(hip_ctx):
    L = cases.capped_launch(16390)
    t = L.tables()
    assert t["rec_slots"] == 16390 > 16384 and len(L.ivs[0]["exp"]["reads"]) == 16390   # both grids are capped at 16384 waves
    decode(hip_ctx, L)


# ---- f. the fill's limits ----------------------------------------------------------------------------------------------------------

def test_fill_lengths_parities_codes_and_qualities(hip_ctx):
    decode(hip_ctx, cases.fill_limits_launch())


def test_fill_capacity_one_short(hip_ctx):
    L = cases.fill_launch(1025)
    L.checks()
    run = Run(hip_ctx, L.tables())
    run.scan()
    regions = regions_of(L)
    exp = cases.expected_fill(L, regions)
    nb, nc = int(exp["base_off"][-1]), int(exp["cigar_off"][-1])
    assert fill_and_check(run, L, regions, base_cap=nb - 1, status=_ffi.PV_ERR_CAPACITY) == 1024
    assert fill_and_check(run, L, regions, cigar_cap=nc - 1, status=_ffi.PV_ERR_CAPACITY) == 1024
    assert fill_and_check(run, L, regions, base_cap=nb // 2, cigar_cap=nc // 3, status=_ffi.PV_ERR_CAPACITY) < 600
    assert fill_and_check(run, L, regions) == 1025


def test_fill_indices_outside_the_kept_reads(hip_ctx):
    L = cases.fill_launch(1025)
    run = Run(hip_ctx, L.tables())
    run.scan()
    kept = [len(iv["exp"]["reads"]) for iv in L.ivs]
    bad = _ffi.PV_ERR_INVALID
    assert fill_and_check(run, L, [(0, None), (2, [3, kept[2], 5]), (3, None)], status=bad) == kept[0] + 2 + 7
    assert fill_and_check(run, L, [(0, None), (2, [3, -1, 5]), (3, None)], status=bad) == kept[0] + 2 + 7
    assert fill_and_check(run, L, [(3, [0, 1]), (1, [0])], status=bad) == 2                       # an interval that keeps nothing has no read 0
    # sel_off + k past n_sel: the last region's indices run out
    exp = cases.expected_fill(L, [(0, None), (3, [6, 5, None, None])])
    got, totals = run.fill([0, 3], exp["read_off"], [-1, 0], [6, 5], int(exp["base_off"][-1]) + 8, int(exp["cigar_off"][-1]) + 8, n_sel=2)
    assert check_fill(got, totals, exp, 1 << 40, 1 << 40, bad) == kept[0] + 2
    run.intact()
    for iv in (-1, len(L.ivs)):
        assert fill_and_check(run, L, [(0, None), (None, [0] * 9), (3, None)], status=bad, reg_iv=[0, iv, 3]) == kept[0] + 7
    assert fill_and_check(run, L, regions_of(L)) == 1025


# ---- g. another stream, twice ------------------------------------------------------------------------------------------------------------

def test_on_a_stream_of_its_own_twice(hip_ctx):
    import torch
    L = cases.fill_launch(1025)
    stream = torch.cuda.Stream(device="cuda:%d" % hip_ctx.device_id)
    seen = []
    for _ in range(2):
        run, counts = decode(hip_ctx, L, stream)   # (the counts come to the host between the two calls: that step is the contract)
        seen.append([counts.tobytes()] + [run.outs[k].host().tobytes() for k in list(OUT_ITEM) + ["totals"]])
    assert seen[0] == seen[1]
