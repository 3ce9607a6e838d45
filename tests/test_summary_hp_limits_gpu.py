"""GPU: the haplotag-aware image builder (pv_summarize_regions_hp[_dev], 48 planes x 21 rows) at every limit its kernels have,
the HP-only edges (overlay clamp and byte packing, failing inserts at depth, the small / large allele-table switch) and the
device-resident form, against the CPU oracle (pinned to the reference at these shapes by
test_oracle_summary_hp.py::test_oracle_vs_live_reference_deep_shapes). Integer work: bit-exact."""
import functools

import numpy as np
import pytest

import cases
from golden_io import assert_summary_equal, summary_as_expected
from pepper_thesis_amd import synth
from pepper_thesis_amd.batch import PRESETS, Read, Region, hp_params, pack_regions

pytestmark = pytest.mark.gpu

P_HP = hp_params(PRESETS["ont_r9_guppy5_sup"])
GUARD = 0x5A


def _exact(hip_ctx, oracle_lib, b, P, what, want_i32=True):
    o = hip_ctx.summarize_hp(b, P, want_i32)
    assert_summary_equal(o, summary_as_expected(oracle_lib.summarize_hp(b, P, want_i32)), what)
    return o


def _shift(regions, step):
    """regions laid `step` columns apart (one batch, distinct positions)"""
    out = []
    for k, r in enumerate(regions):
        off = k * step
        out.append(Region(off + r.ref_start, off + r.ref_end, r.ref,
                          [Read.make(off + x.pos, x.cigar, x.bases, x.quals, x.is_reverse, x.mapq, x.hp_tag) for x in r.reads],
                          None if r.cand_start is None else off + r.cand_start, None if r.cand_end is None else off + r.cand_end))
    return out


@functools.lru_cache(maxsize=None)
def _batch(name):
    """the module's larger batches, built once"""
    if name == "dense":
        return pack_regions([cases.hp_every_column_a_site()])
    if name == "many_32768":
        return pack_regions([cases.hp_many_reads(32768)])
    if name == "bench4":
        from tools import bench_hp
        return pack_regions(bench_hp.tag_regions(bench_hp.workload_regions(4)))
    raise KeyError(name)


# ---- 1. the 26-plane limit tests (test_summary_gpu.py) in haplotag form -------------------------------------------------

def test_depth_5000_max_reads(hip_ctx, oracle_lib):
    """MAX_READS_IN_REGION = 5000 (Options.py:98), every tag: several pair batches per tile, depth clipped to 125"""
    b = pack_regions([cases.hp_depth_5000()])
    assert b.n_reads > 4000
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "depth 5000")
    assert len(o) > 10 and int(o.depth.max()) == 125


def test_region_read_limit_of_the_16_bit_planes(hip_ctx, oracle_lib):
    """32767 reads over the same 120 columns (every tag, both strands) are exact. Hand-worked: the six reads of
    cases.HP_MANY_DEL_READS delete column 65, which is row 15 of the window at the SNP column 60; the '*' symbol planes
    (14 + 11 * group) count a deleted column in the read's symbol sets (tag 0 both, 1 set 1, any other value set 2):
    forward set 1 = tags 0, 1 forward = 2; reverse set 1 = tag 1 reverse = 1; forward set 2 = tags 0, 2, -1 forward = 3;
    reverse set 2 = tag 3 reverse = 1. Every other plane of the window is at the +-125 clamp."""
    b = pack_regions([cases.hp_many_reads(32767)])
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "32767 reads")
    assert len(o) == 1 and int(o.position[0]) == 1060 and int(o.depth[0]) == 125
    assert o.images_i32[0, 15, [14, 25, 36, 47]].tolist() == [2, 1, 3, 1]


def test_region_read_limit_split_between_set_1_and_both(hip_ctx, oracle_lib):
    """32767 forward reads, tag 0 or 1 alternately: every read joins haplotype set 1, so the set-1 forward REF-count plane is
    the sum of two count-set classes (set 1 only: 16383 reads, both: 16384) = -32767 before the clamp, the int16 limit;
    a class counted twice or a wrapped sum would turn it positive. The window holds the clamped -125 (every HP plane is
    clamped), and the set-2 plane (the tag-0 reads) is -125 as well."""
    b = pack_regions([cases.hp_many_reads(32767, tags=lambda i: i & 1, all_forward=True)])
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "32767 reads, tags 0 / 1")
    assert len(o) == 1
    assert int(o.images_i32[0, 0, 4]) == -125 and int(o.images_i32[0, 0, 26]) == -125
    # the only reverse reads are two deleting ones: tag 1 (set 1) and tag 3 (no REF-count set)
    assert int(o.images_i32[0, 0, 15]) == -1 and int(o.images_i32[0, 0, 37]) == 0


def test_region_read_limit_32768_is_refused(hip_ctx):
    """one read more than the 16-bit planes count: PV_ERR_LIMIT from the host form, status PV_ERR_LIMIT from the device form"""
    import torch
    from pepper_thesis_amd import _ffi
    from pepper_thesis_amd.device import DeviceBatch, DeviceOut
    big = _batch("many_32768")
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.summarize_hp(big, P_HP)
    assert e.value.code == _ffi.PV_ERR_LIMIT and "32767" in str(e.value)
    img = torch.zeros((64, _ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES), dtype=torch.int8, device="cuda:0")
    dout = DeviceOut(64, 1024, images=img)
    hip_ctx.summarize_hp_dev(DeviceBatch(big), P_HP, dout)
    hip_ctx.synchronize()
    assert dout.status() == _ffi.PV_ERR_LIMIT


def _events_at(batch_region, positions):
    """SNP observations (mismatching bases, all at quality 20) at the given columns of a region of full-length reads"""
    ref = np.frombuffer(batch_region.ref, np.uint8)
    n = 0
    cols = np.unique(np.asarray(positions) - batch_region.ref_start)
    for rd in batch_region.reads:
        n += int((np.frombuffer(rd.bases, np.uint8)[cols] != ref[cols]).sum())
    return n


def test_every_column_a_site_triggers_workspace_retry(hip_ctx, oracle_lib):
    """six reads over 40 000 columns, each differing from the reference on half of them: over 30 000 sites against the
    heuristic's n_cols / 8 + 1024 = 6024, and every mismatch at a site is an event in this form (over 90 000) against the
    heuristic's n_cigar + n_bases / 64 + 4096 + n_bases / 16 = 6 + 3750 + 4096 + 15 000 = 22 852. The first launch must
    overflow; the host entry point retries with exact bounds."""
    b = _batch("dense")
    reg = cases.hp_every_column_a_site()
    o = hip_ctx.summarize_hp(b, P_HP, False)
    e = oracle_lib.summarize_hp(b, P_HP, False)
    assert len(o) == len(e) > 30_000
    n_sites = len(np.unique(e.position))
    n_events = _events_at(reg, e.position)
    assert n_sites > b.ref.shape[0] // 8 + 1024
    assert n_events > b.n_cigar + b.n_bases // 64 + 4096 + b.n_bases // 16
    np.testing.assert_array_equal(o.images, e.images)
    np.testing.assert_array_equal(o.position, e.position)
    np.testing.assert_array_equal(o.depth, e.depth)
    assert o.candidates == e.candidates


def test_1024_alleles_at_one_site_fit_the_table(hip_ctx, oracle_lib):
    """the HP allele table has no pre-seeded A/C/G/T slots (s_nU = 0): in this form only mismatching bases and inserts /
    deletes are allele keys. The site (anchor column 14; every read matches there, so no SNP key) holds 1023 distinct
    six-base inserts and one three-base insert seen 200 times: 1024 keys = UMAX, exactly full. Exact, with the 200-read
    insert as a candidate."""
    b = pack_regions([cases.hp_many_alleles(1024)])
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "1024 alleles")
    assert o.candidates == ["2GGTT"]


def test_more_than_1024_alleles_at_one_site_is_reported(hip_ctx):
    """the same site with 1024 distinct six-base inserts next to the three-base one: 1025 keys, one over the table:
    PV_ERR_LIMIT, not a crash or a wrong answer"""
    from pepper_thesis_amd import _ffi
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.summarize_hp(pack_regions([cases.hp_many_alleles(1025)]), P_HP)
    assert e.value.code == _ffi.PV_ERR_LIMIT


def test_long_indels_and_padded_reference(hip_ctx, oracle_lib):
    """a 3000-base insertion (quality sum over the inserted bases), a deletion longer than the region remainder, a reference
    buffer longer than the region (ref_len > R), SNPs beside both so that windows cover them; two presets"""
    b = pack_regions([cases.hp_long_indels()])
    for preset in ("ont_r9_guppy5_sup", "hifi"):
        o = _exact(hip_ctx, oracle_lib, b, hp_params(PRESETS[preset]), preset)
        assert len(o) == 2


def test_read_over_more_than_256_tiles_takes_the_search_path(hip_ctx, oracle_lib):
    """reads over 270 tiles (a 140 kb region): op ranges by binary search, no sub-tile index"""
    rng = np.random.default_rng(41)
    R = 140_000
    ref = cases._acgt(rng, R)
    reads = []
    for i in range(8):
        if i < 4:   # one op over 270 tiles
            reads.append(Read.make(200, "%dM" % (R - 1000), cases.mutated(ref[200:R - 800], rng, 0.002).tobytes(), 25, i % 2 == 0))
        else:       # many ops over 270 tiles: 900M 1I 900M 2D ...
            cig, seq, pos = [], [], 300
            while pos + 2000 < R - 500:
                cig.append("900M1I900M2D")
                seq.append(cases.mutated(ref[pos:pos + 900], rng, 0.002).tobytes() + b"A"
                           + cases.mutated(ref[pos + 900:pos + 1800], rng, 0.002).tobytes())
                pos += 1802
            reads.append(Read.make(300, "".join(cig), b"".join(seq), 25, i % 2 == 0))
    b = pack_regions(cases.tag_reads([Region(0, R - 1, ref.tobytes(), reads)], 41))
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "270 tiles")
    assert len(o) > 100


def test_read_with_more_than_65535_ops(hip_ctx, oracle_lib):
    """1M1D x 34 000 = 68 000 ops: more than the 16-bit op offsets of the tile-boundary table"""
    rng = np.random.default_rng(43)
    n_units = 34_000
    R = 2 * n_units + 400
    ref = cases._acgt(rng, R)
    reads = []
    for i in range(5):
        seq = cases.mutated(ref[100:100 + 2 * n_units:2].copy(), rng, 0.01)
        reads.append(Read.make(100, "1M1D" * n_units, seq.tobytes(), 25, i % 2 == 0))
    for i in range(5):
        reads.append(Read.make(50, "%dM" % (R - 100), cases.mutated(ref[50:R - 50], rng, 0.01).tobytes(), 25, i % 2 == 1))
    b = pack_regions(cases.tag_reads([Region(0, R - 1, ref.tobytes(), reads)], 43))
    o = _exact(hip_ctx, oracle_lib, b, P_HP, "68 k ops")
    assert len(o) > 100


def test_op_batches_beyond_the_lookup_tables(hip_ctx, oracle_lib):
    """(a) 140 reads that are one long match each (512 slots per op), (b) 140 reads with an op on nearly every column (over
    100 k ops in a pair batch) and reads with 300 one-base inserts in a row (saturated sub-tile index)"""
    rng = np.random.default_rng(47)
    R = 1500
    ref = cases._acgt(rng, R)
    alt = cases.mutated(ref, rng, 0.02)
    reads = [Read.make(0, "%dM" % R, cases.mutated(alt, rng, 0.01).tobytes(), 25, i % 2 == 0) for i in range(140)]
    b = pack_regions(cases.tag_reads([Region(0, R - 1, ref.tobytes(), reads)], 47))
    assert len(_exact(hip_ctx, oracle_lib, b, P_HP, "long matches")) > 10
    reads = []
    for i in range(140):
        n_units = (R - 20) // 2
        seq = bytearray()
        for u in range(n_units):
            seq += bytes([int(alt[10 + 2 * u]), ord("ACGT"[(u + (i & 1)) % 4]), int(alt[11 + 2 * u])])
        reads.append(Read.make(10, "1M1I1M" * n_units, bytes(seq), 25, i % 2 == 0))
    for i in range(6):
        seq = alt[40:340].tobytes() + b"ACGT" * 75 + alt[340:900].tobytes()
        reads.append(Read.make(40, "300M" + "1I" * 300 + "560M", seq, 25, i % 2 == 0))
    b = pack_regions(cases.tag_reads([Region(0, R - 1, ref.tobytes(), reads)], 48))
    assert len(_exact(hip_ctx, oracle_lib, b, P_HP, "dense ops")) > 10


def test_more_than_8192_tiles_in_a_batch(hip_ctx, oracle_lib):
    """4.4 M columns are 8 594 tiles: two passes of the one-workgroup tile scan"""
    rng = np.random.default_rng(53)
    regs = []
    for g in range(44):
        R = 100_000
        ref = cases._acgt(rng, R)
        start = int(rng.integers(1000, R - 3000))
        alt = cases.mutated(ref[start:start + 1500], rng, 0.02)
        reads = [Read.make(g * 1_000_000 + start, "1500M", cases.mutated(alt, rng, 0.005).tobytes(), 25, i % 2 == 0)
                 for i in range(6)]
        regs.append(Region(g * 1_000_000, g * 1_000_000 + R - 1, ref.tobytes(), reads))
    b = pack_regions(cases.tag_reads(regs, 53))
    assert (b.ref.shape[0] + 511) // 512 > 8192
    o = hip_ctx.summarize_hp(b, P_HP, False)
    e = oracle_lib.summarize_hp(b, P_HP, False)
    assert len(o) > 100
    assert_summary_equal(o, summary_as_expected(e), "8594 tiles")


def test_full_size_region_properties(hip_ctx, oracle_lib):
    """a BASELINE-size region (100 200 columns, 60x, 10 kb reads, every tag): exact, positions in order, the same region twice
    in one batch is the single result twice, and run to run byte-identical"""
    reg = cases.tag_reads([synth.synth_region(2024)], 2024)[0]
    b1 = pack_regions([reg])
    o1 = _exact(hip_ctx, oracle_lib, b1, P_HP, "full size")
    assert len(o1) > 300
    assert (np.diff(o1.position) >= 0).all()
    reg2 = cases.tag_reads([synth.synth_region(2024, ref_start=reg.ref_start)], 2024)[0]
    o2 = hip_ctx.summarize_hp(pack_regions([reg, reg2]), P_HP, False)
    n = len(o1)
    assert len(o2) == 2 * n
    np.testing.assert_array_equal(o2.images[:n], o1.images)
    np.testing.assert_array_equal(o2.images[n:], o1.images)
    np.testing.assert_array_equal(o2.depth[n:], o1.depth)
    assert o2.candidates[:n] == o1.candidates and o2.candidates[n:] == o1.candidates
    o3 = hip_ctx.summarize_hp(b1, P_HP, False)
    assert o3.images.tobytes() == o1.images.tobytes() and o3.candidates == o1.candidates


# ---- 2. edges of the haplotag form only -----------------------------------------------------------------------------------

def test_overlay_counts_clamped_and_packed_per_group(hip_ctx, oracle_lib):
    """one candidate per region (SNP, insert, delete: t = 1, 2, 3) whose observations in one (strand x set) group are 124,
    125, 126, 255, 256 or 300, the other groups 3, 5 and 7 plus the untagged reads of the big group (they join both sets),
    and reads tagged 3 / -1 (no group). k_site_alleles clamps each group count to 125 and packs the four into one int32;
    k_write_windows<true> unpacks them onto planes 4+t, 26+t (forward set 1 / 2) and 15+t, 37+t (reverse set 1 / 2) of the
    middle row"""
    regs, counts = cases.hp_overlay_batch_regions()
    o = _exact(hip_ctx, oracle_lib, pack_regions(regs), P_HP, "overlay clamp")
    for g, ((t, n, big), c) in enumerate(zip(cases.HP_OVERLAY_CASES, counts)):
        k = [i for i in range(len(o)) if o.region[i] == g and o.candidates[i][0] == str(t)]
        assert len(k) == 1, (g, t)
        row = o.images_i32[k[0], 10]
        assert c[big] == n
        assert row[[4 + t, 26 + t, 15 + t, 37 + t]].tolist() == [min(v, 125) for v in c], (t, n, big, c)


def test_failing_inserts_at_depth_take_the_anchor_coverage_back(hip_ctx, oracle_lib):
    """200 inserts whose inserted bases fail the quality bar on an anchor that passes it, 40 passing inserts, 30 matches, every
    tag: each failing insert removes its anchor's coverage (more than 125 of them), so the anchor's depth is 270 - 200 = 70"""
    for preset in ("ont_r9_guppy5_sup", "hifi"):
        o = _exact(hip_ctx, oracle_lib, pack_regions([cases.hp_failing_inserts()]), hp_params(PRESETS[preset]), preset)
        assert len(o) == 1 and int(o.position[0]) == 30 and int(o.depth[0]) == 70 and o.candidates == ["2GCA"]


def test_allele_table_switch_hp(hip_ctx, oracle_lib):
    """k_site_rank: a haplotag-form site receives every SNP observation as an event (nev = the SNP counter), and goes to the
    large-table launch k_site_alleles<true, UMAX, true> when nev + 4 > UM_SMALL = 96. Regions of depth 88..97 whose reads all
    mismatch at column 40: depths 88-92 run in the small-table instantiation, 93-97 in the large one"""
    regs = cases.switch_regions("snp")
    o = _exact(hip_ctx, oracle_lib, pack_regions(regs), P_HP, "allele-table switch (HP)")
    for g, d in enumerate(cases.SWITCH_DEPTHS):
        mine = [i for i in range(len(o)) if o.region[i] == g]
        assert sorted(o.candidates[i] for i in mine) == ["1G", "1T"], d
        assert {int(o.depth[i]) for i in mine} == {d}


def test_allele_table_switch_26_planes(hip_ctx, oracle_lib):
    """the 26-plane form's events are insert + delete + rare SNP observations: regions with 88..97 insert observations at
    one anchor (and no other event there) put nev = 88..92 in the small-table instantiation and 93..97 in the large one"""
    regs = cases.switch_regions("ins")
    b = pack_regions(regs)
    P = PRESETS["ont_r9_guppy5_sup"]
    o = hip_ctx.summarize(b, P, True)
    assert_summary_equal(o, summary_as_expected(oracle_lib.summarize(b, P, True)), "allele-table switch (26 planes)")
    for g, d in enumerate(cases.SWITCH_DEPTHS):
        mine = [i for i in range(len(o)) if o.region[i] == g]
        assert [o.candidates[i] for i in mine] == ["2AAC"] and int(o.cand_freq[mine[0]]) == d, d


# ---- 3. the device-resident form -------------------------------------------------------------------------------------------

def _dev_out(capacity, str_capacity, room=0):
    """a DeviceOut for the HP form whose tensors have `room` spare entries past the capacities, all filled with GUARD"""
    import torch
    from pepper_thesis_amd import _ffi
    from pepper_thesis_amd.device import DeviceOut
    img = torch.empty((capacity + room, _ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES), dtype=torch.int8, device="cuda:0")
    dout = DeviceOut(capacity + room, str_capacity + room, images=img)
    dout.c.capacity, dout.c.str_capacity = capacity, str_capacity
    for t in (dout.region, dout.position, dout.depth, dout.cand_freq, dout.images, dout.cand_str, dout.cand_off):
        t.view(torch.uint8).fill_(GUARD)
    return dout


def _run_dev(hip_ctx, batch, P, dout):
    """the device form on a side stream; -> counts [n_out, str_bytes, status, n_sites]"""
    import torch
    from pepper_thesis_amd.device import DeviceBatch
    db = DeviceBatch(batch)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    hip_ctx.summarize_hp_dev(db, P, dout, stream=s.cuda_stream)
    s.synchronize()
    return dout.counts.cpu().tolist()


def _guard_after(t, n):
    import torch
    rest = t.view(torch.uint8).reshape(t.shape[0], -1)[n:] if t.dim() > 1 or t.dtype != torch.uint8 else t[n:]
    return bool((rest.cpu().numpy() == GUARD).all())


def _assert_dev_equals_host(dout, counts, host, what):
    import torch
    n = len(host)
    assert counts[0] == n and counts[2] == 0, (what, counts)
    np.testing.assert_array_equal(dout.region[:n].cpu().numpy(), host.region, err_msg=what)
    np.testing.assert_array_equal(dout.position[:n].cpu().numpy(), host.position, err_msg=what)
    np.testing.assert_array_equal(dout.depth[:n].cpu().numpy(), host.depth, err_msg=what)
    np.testing.assert_array_equal(dout.cand_freq[:n].cpu().numpy(), host.cand_freq, err_msg=what)
    np.testing.assert_array_equal(dout.images[:n].cpu().numpy(), host.images, err_msg=what)
    off = dout.cand_off[:n + 1].cpu().numpy()
    raw = dout.cand_str[:int(off[-1]) if n else 0].cpu().numpy().tobytes()
    assert int(off[0]) == 0 and counts[1] == int(off[-1]), what
    assert [raw[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(n)] == host.candidates, what
    # nothing written past the windows, the offsets and the key bytes the call reports
    for t, m in ((dout.region, n), (dout.position, n), (dout.depth, n), (dout.cand_freq, n), (dout.images, n),
                 (dout.cand_off, n + 1), (dout.cand_str, counts[1])):
        assert _guard_after(t, m), what
    assert dout.images.dtype == torch.int8


def _golden_case_regions():
    regs = []
    for name in cases.EDGE_CASES:
        regs.extend(cases.EDGE_CASES[name]())
    regs.extend(synth.synth_region(seed, **kw) for seed, kw, _ in cases.GOLDEN_RANDOM)
    return _shift(cases.tag_reads(regs, 5), 100_000)


def _random_regions(seed=3):
    rng = np.random.default_rng(seed)
    # (depth 40x or more: at 5x with 6 % noise a third of the columns are sites, beyond the device form's workspace
    # heuristic - it reports PV_ERR_LIMIT then, see test_device_form_dense_sites_report_the_limit)
    regs = [synth.synth_region(900 + k, region_len=int(rng.integers(300, 6000)), depth=int(rng.integers(40, 90)),
                               read_len=int(rng.integers(200, 3000)), site_every=int(rng.integers(15, 200)),
                               ref_start=100_000 * (k + 1))
            for k in range(6)]
    return cases.tag_reads(regs, seed)


@pytest.mark.parametrize("which", ["golden_cases", "random", "untagged"])
def test_device_form_matches_host_form(hip_ctx, oracle_lib, which):
    """pv_summarize_regions_hp_dev on a side stream == pv_summarize_regions_hp == the oracle: int8 images, region, position,
    depth, cand_freq and candidate strings; guard bytes past what the call reports stay untouched. 'untagged' passes a null
    read_hp pointer."""
    if which == "golden_cases":
        b = pack_regions(_golden_case_regions())
    elif which == "random":
        b = pack_regions(_random_regions())
    else:
        b = cases.random_batch(16, cases.GOLDEN_RANDOM[5][1])
        assert b.read_hp is None
    host = _exact(hip_ctx, oracle_lib, b, P_HP, which, want_i32=False)
    assert len(host) > 20
    dout = _dev_out(4096, 8 * 4096, room=32)   # (the site bound of the workspace heuristic grows with the capacity too)
    counts = _run_dev(hip_ctx, b, P_HP, dout)
    _assert_dev_equals_host(dout, counts, host, which)


def test_device_form_on_the_benchmark_workload(hip_ctx, oracle_lib):
    """the hp_builder figure's workload (tools/bench_hp.py: bench.py's 100 kb regions at 60x, its tag mix), first 4 regions:
    device form == host form window for window, host form == oracle"""
    b = _batch("bench4")
    host = _exact(hip_ctx, oracle_lib, b, P_HP, "bench_hp workload", want_i32=False)
    assert len(host) > 1000
    dout = _dev_out(16384, 16384 * 16, room=16)
    counts = _run_dev(hip_ctx, b, P_HP, dout)
    _assert_dev_equals_host(dout, counts, host, "bench_hp workload (device)")


def test_device_form_dense_sites_report_the_limit(hip_ctx):
    """the every-column-a-site batch overflows the device form's workspace heuristic; it cannot retry, so it must end with
    status PV_ERR_LIMIT and no windows"""
    from pepper_thesis_amd import _ffi
    dout = _dev_out(4096, 4096 * 8, room=16)
    counts = _run_dev(hip_ctx, _batch("dense"), P_HP, dout)
    assert counts[2] == _ffi.PV_ERR_LIMIT, counts
    assert _guard_after(dout.images, 0) and _guard_after(dout.region, 0)


def test_device_form_output_capacity(hip_ctx):
    """capacity below the number of windows: the counts report what is needed, the windows that fit are the host form's first
    ones, and no byte lands past `capacity` windows"""
    b = cases.hp_random_batch(11, cases.GOLDEN_RANDOM[0][1])
    host = hip_ctx.summarize_hp(b, P_HP)
    n = len(host)
    assert n == 74
    cap = 10
    need = int(sum(len(c) for c in host.candidates))   # (a candidate string starts with its type digit)
    dout = _dev_out(cap, need, room=80)
    counts = _run_dev(hip_ctx, b, P_HP, dout)
    assert counts[0] == n and counts[1] == need and counts[2] == 0, counts
    np.testing.assert_array_equal(dout.images[:cap].cpu().numpy(), host.images[:cap])
    np.testing.assert_array_equal(dout.position[:cap].cpu().numpy(), host.position[:cap])
    np.testing.assert_array_equal(dout.region[:cap].cpu().numpy(), host.region[:cap])
    first = int(sum(len(c) for c in host.candidates[:cap]))
    for t, m in ((dout.region, cap), (dout.position, cap), (dout.depth, cap), (dout.cand_freq, cap), (dout.images, cap),
                 (dout.cand_off, cap + 1), (dout.cand_str, first)):
        assert _guard_after(t, m)
