"""CPU: every case of vote_runs_limits_cases reaches the limit it is named for, shown from the checker (vote_runs_ref.py) and
plain arithmetic on the kernel's constants: read rounds that keep none, all and some of their 256 reads, 86 runs in a tile of 88
slots, runs and flanks on either side of a tile edge, regions that meet inside a tile, every CIGAR word with a CIGAR of more
than 128 words, runs on the chunk boundaries of every chunk geometry, and a layout that is short of insert rows. A case that is
edited so that it stops reaching its kernel path fails here."""
import numpy as np
import pytest

import chunk_geometry_cases as cg
import min_qual_cases as mc
import vote_runs_cases as rc
import vote_runs_limits_cases as Z
import vote_runs_ref as rr


def test_the_constants_fit_together():
    # a run takes its bytes and a byte that is not a candidate's, min_run >= 2: at most 86 start in a tile, under the 88 slots
    assert -(-Z.TILE // 3) == 86 <= Z.SLOTS and (Z.MAX_RUN, Z.MAX_LEN) == (rr.MAX_RUN, rr.MAX_LEN)


def test_rounds_keep_none_all_and_some_of_their_reads():
    c = Z.rounds()
    b = c.batch
    assert b.n_regions == 1 and int(b.ref_off[1]) == 300 and b.n_reads == 600
    kept = [Z.kept_per_round(b, 0, t) for t in (0, 1)]
    assert all(len(k) == 3 for k in kept)                             # rounds of 256, 256 and 88
    assert kept[1][0] == 0 and kept[0][1] == kept[1][1] == Z.ROUND and 0 < kept[0][0] < Z.ROUND and 0 < kept[1][2] < 88
    for lo, hi in ((0, 256), (256, 512), (512, 600)):                 # mapping quality 0 in the rounds that may have it
        q0 = int((b.read_mapq[lo:hi] == 0).sum())
        assert q0 == 0 if lo == 256 else 0.2 * (hi - lo) <= q0 <= 0.3 * (hi - lo), (lo, q0)
    runs, seen, skipped = c.runs
    assert [(r.s - Z.ROUNDS_START, r.n, r.b) for r in runs] == [(s, n, x) for s, (x, n) in sorted(Z.ROUNDS_RUNS.items())]
    assert [Z.tile_of(b, r) for r in runs] == [0, 0, 1] and runs[1].s + runs[1].n - 1 - Z.ROUNDS_START > 256   # C x 8 crosses into tile 1
    assert max(r.S for r in runs) > Z.ROUND and all(r.L is not None for r in runs) and (seen, skipped) == (3, 0)
    assert [r.L - r.n for r in runs] == [0, 1, -1]
    first = Z.all_runs(Z.first_reads(b, Z.ROUND))[0]                   # only the first round counted
    assert [r.L for r in first] == [4, None, None] and first[0].L != runs[0].L
    # every round's own lengths vary, and several anchors hold the inserted letters
    for r in runs:
        assert sum(v > 0 for v in r.h) >= 2, r
    cig = [b.cigar[int(b.cigar_off[r]):int(b.cigar_off[r + 1])] for r in range(600)]
    assert len({tuple(int(w) for w in cg_) for cg_ in cig}) >= 20


def test_round_counts_are_255_256_and_257_voters():
    c = Z.round_counts()
    runs = c.runs[0]
    assert [(r.S, r.V) for r in runs] == [(n, n) for n in Z.ROUND_COUNTS] and [r.L for r in runs] == [5, 6, 5]
    assert [r.L for r in Z.all_runs(Z.first_reads(c.batch, int(np.diff(c.batch.read_off)[2]) - 1))[0]][2] == 6   # the last read decides
    kept = [Z.kept_per_round(c.batch, g, 0) for g in range(3)]
    assert [len(k) for k in kept] == [2, 2, 2] and all(0 < k[0] < Z.ROUND and k[1] > 0 for k in kept)
    assert [sum(k) for k in kept] == list(Z.ROUND_COUNTS)


def test_slots_86_runs_start_in_one_tile():
    c = Z.slots()
    assert c.draft == ("T" + "AACGGTCCATTG" * 60)[:700] and c.min_run == 2 and c.batch.n_reads == 12
    runs, seen, skipped = c.runs
    per = Z.runs_per_tile(c.batch, 2)
    assert tuple(per[t] for t in range(3)) == Z.SLOTS_PER_TILE == (85, 86, 62) and max(per.values()) <= Z.SLOTS
    assert (seen, skipped) == (233, 0) and len(runs) == 233
    mine = [r for r in runs if Z.tile_of(c.batch, r) == 1]
    assert mine[0].s == 256 and mine[-1].s == 511 and mine[-1].s + mine[-1].n - 1 == 512     # tile 1's bytes 0 and 255
    assert all(r.L is not None for r in runs) and sum(r.L != r.n for r in runs) >= 40
    assert {r.L for r in runs} == {0, 1, 2, 3, 4} and len({r.h for r in mine}) >= 10
    assert Z.slots(3).runs == ([], 0, 0)                                                      # runs of two are no candidates at 3


def test_tile_edges_owners_and_flanks():
    c = Z.tile_edges()
    runs, seen, skipped = c.runs
    assert (seen, skipped) == (7, 2) and c.batch.n_reads == 10 and int(c.batch.ref_off[1]) == 1600
    got = {r.s: (r.n, Z.tile_of(c.batch, r), r.L) for r in runs}
    assert got == {208: (48, 0, 50), 511: (6, 1, 5), 768: (5, 3, 7), 1000: (48, 3, 48), 1301: (3, 5, 2)}
    tile = lambda p: p // Z.TILE
    assert tile(208 + 47) == 0 and tile(208 + 48) == 1                 # the last byte is the tile's last, the right flank the next tile's
    assert tile(511) == 1 and tile(510) == 1 and tile(512) == 2        # the first byte is the tile's last
    assert tile(768) == 3 and tile(767) == 2                           # the left flank is the tile's before
    assert tile(1000) == 3 and tile(1047) == 4 and tile(1048) == 4     # the run crosses byte 1024
    st = {s: n for s, n, _ in rr.stretches(c.draft.encode()) if n > 1}
    assert {n for n in st.values() if n > Z.MAX_RUN} == {49, 96, 97, 200}
    assert st[1100] == 200 and tile(1100) != tile(1299) and st[1301] == 3 and c.draft[1300] not in "TC"
    assert st[1532] == st[1536] == 4 and tile(1535) != tile(1536)      # the skipped pair touches on a tile edge
    # the grown runs' insert rows: two anchors each, so the rank of a row counts rows of two anchors behind the left flank
    lay = rc.host_chain(c.batch, c.L, c.O)[0]
    for s in (208, 768):
        anchors = {p for p, x in lay.rows[0] if x > 0 and s - 1 <= p < s + got[s][0]}
        assert anchors == set(Z.EDGE_ANCHORS[s]), s


@pytest.mark.parametrize("across", [False, True], ids=["region_5_starts_tile_1", "region_5_across_byte_256"])
def test_regions_meet_inside_a_tile(across):
    c = Z.regions_in_a_tile(across)
    b = c.batch
    sizes = np.diff(b.ref_off)
    assert b.n_regions == 7 and sizes.min() >= 30 and sizes.max() <= 70
    lo5, hi5 = int(b.ref_off[5]), int(b.ref_off[6])
    assert (lo5 < 256 < hi5) if across else lo5 == 256
    per = [rr.region_runs(b, g, 3) for g in range(7)]
    assert [p[1] for p in per] == c.seen and [sum(r.L is not None for r in p[0]) for p in per] == c.decided and all(p[2] == 0 for p in per)
    reads = np.diff(b.read_off)
    assert reads[1] == 0 and reads[2] > 0 and (b.read_mapq[int(b.read_off[2]):int(b.read_off[3])] == 0).all() and reads[3] > 0
    # the joined pair: six A's in a row in the flat draft, and no candidate on either side
    flat = b.ref.tobytes()
    assert flat[lo5 - 4:lo5 + 4] == b"CAAAAAAT"
    d4, d5 = flat[int(b.ref_off[4]):lo5], flat[lo5:hi5]
    assert not [s for s, n, _ in rr.candidates(d4, 3)[0] if s + n > 56] and not [s for s, n, _ in rr.candidates(d5, 3)[0] if s < 4]
    assert (len(d4) - 3, 3, "A") in rr.stretches(d4) and (0, 3, "A") in rr.stretches(d5)
    # the run both flanks of which are the region's ends
    assert (per[0][0][0].s, per[0][0][0].n) == (101, 40) and sizes[0] == 42 and per[0][0][0].L == 39
    # the overlapping pair holds one run twice, and their reads decide differently
    r5, r6 = per[5][0][0], per[6][0][0]
    assert b.ref_start[6] < b.ref_end[5] and (r5.s, r5.n, r5.b) == (r6.s, r6.n, r6.b) and (r5.L, r6.L) == (4, 7)


def test_cigar_words_every_code_and_a_deep_search():
    c = Z.cigar_words()
    b = c.batch
    assert set(int(w) & 0xF for w in b.cigar) == set(range(9))
    assert int(np.diff(b.cigar_off).max()) >= 128
    runs = c.runs[0]
    assert [(r.s - Z.WORDS_START, r.n, r.b) for r in runs] == [(s, n, x) for s, (x, n) in sorted(Z.WORDS_RUNS.items())]
    for kind, reads in c.kinds.items():
        pairs = [(Z.spans(rd, r.s, r.n), Z.overlaps(rd, r.s, r.n)) for rd in reads for r in runs]
        assert (True, True) in pairs and (False, True) in pairs, kind
        # what the kind's first read alone shows for the first run
        one = rr.region_runs(rc.one_region(c.draft, [reads[0]], Z.WORDS_START), 0, 3)[0][0]
        shown = Z.WORDS_SHOWN[kind]
        want = (0, 0, None) if shown is None else (1, 0, None) if shown == "impure" else (1, 1, shown)
        assert (one.S, one.V, one.L) == want, (kind, one)
    assert set(Z.WORDS_SHOWN) == set(c.kinds) == set(Z.WORDS_KINDS)
    assert all(r.L is not None for r in runs) and [r.L - r.n for r in runs] == [1, -1, 0] and runs[0].S > runs[0].V


@pytest.mark.parametrize("geo", cg.GEOMETRIES, ids=cg.geo_id)
def test_geometries_put_runs_on_the_chunk_boundaries(geo):
    L, O = geo
    step = L - O
    c = Z.geometry(L, O)
    assert (c.L, c.O) == geo and int(c.batch.ref_off[1]) == max(3 * L, 200) and c.batch.n_reads == 8
    runs = {r.b: r for r in c.runs[0]}
    assert {k: runs[Z.GEOMETRY_LETTERS[k]].L - 3 for k in ("shrink", "keep", "grow")} == {"shrink": -1, "keep": 0, "grow": 2}
    assert c.runs[1:] == (3, 0)
    lay = mc.Layout([(0, c.batch.ref.tobytes(), {p: 2 for p in (c.where["grow"] - 1, c.where["grow"] + 1)})], L, O)
    got = rc.host_chain(c.batch, L, O)[0]                              # the reads ask for exactly these insert rows
    assert np.array_equal(got.position, lay.position) and np.array_equal(got.index, lay.index)
    rows = {k: Z.span_rows(lay, runs[Z.GEOMETRY_LETTERS[k]]) for k in c.where}
    assert len(rows["grow"]) == 7 and len(rows["shrink"]) == len(rows["keep"]) == 3
    chunks_of = lambda r: {m for m in range(lay.n) if m * step <= r < m * step + L}
    if L < 16:
        assert all(len(chunks_of(v[0]) | chunks_of(v[-1])) >= 2 for v in rows.values())
        return
    assert rows["grow"][-1] == L - 1 and 0 not in chunks_of(L)          # chunk 0 ends with the run; its right flank is chunk 1's
    m = rows["shrink"][1] // step                                      # the shrinking run lies on either side of chunk m's first row
    assert m >= 1 and rows["shrink"][0] == m * step - 1 and rows["shrink"][1] == m * step
    if O >= 19:
        assert step <= rows["keep"][0] and rows["keep"][-1] < L        # inside the rows chunks 0 and 1 share


def test_state_one_insert_row_short():
    c = Z.state()
    runs = c.runs[0]
    assert [(r.n, r.L) for r in runs] == [(4, 3), (5, 7)]
    for regs, ok in ((c.short, False), (c.enough, True)):
        lay = mc.Layout(regs, c.L, c.O)
        lab, _ = lay.spelled()
        have = sum(1 for p, x in lay.rows[0] if x > 0)
        assert have == (2 if ok else 1)
        if ok:
            assert rr.vote_runs(c.batch, lay.position, lay.index, lay.region, lay.chunk_id, lab, None, c.O, 3)[2] == [2, 0, -1, 2, 2, 0]
        else:
            with pytest.raises(rr.BadState):
                rr.vote_runs(c.batch, lay.position, lay.index, lay.region, lay.chunk_id, lab, None, c.O, 3)
