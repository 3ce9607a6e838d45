"""CPU: the cases of tests/chunk_geometry_cases.py discriminate, and the host checkers agree with each other on them, at every
chunk geometry of the table: the shared columns carry labels that tell the two copies apart in every way the stitch can get
wrong, every region has a chunk with both neighbours, the geometries that stand for a ragged thread layout have one, and the
decade case tells the decimal string order of chunk ids from the numeric one on exactly the pairs where they differ."""
import numpy as np
import pytest

import chunk_geometry_cases as cg
import edits_ref as er
import min_qual_ref as mq
import qual_ref as qr
import stitch_ref as sr

GEO = pytest.mark.parametrize("geo", cg.GEOMETRIES, ids=cg.geo_id)


def _kept(lay):
    """bool [n, L]: the rows the stitch keeps (no padding, not in the buffer of a late region)"""
    rs = lay.ref_start[lay.region][:, None]
    return (lay.position >= 0) & (lay.index >= 0) & ~((rs > 0) & (lay.position <= rs + sr.BUFFER_POSITIONS))


def test_the_table():
    assert len(cg.GEOMETRIES) == 20 == len(set(cg.GEOMETRIES))
    for L, O in cg.GEOMETRIES:
        assert 1 <= L <= cg.THREADS * cg.MAX_CPT and 0 <= 2 * O <= L and 1 <= cg.cpt(L) <= cg.MAX_CPT
    assert {cg.cpt(L) for L, _ in cg.GEOMETRIES} == {1, 2, 3, 4, 9, 15, 16}
    assert any(O == 0 for _, O in cg.GEOMETRIES) and any(2 * O == L for L, O in cg.GEOMETRIES)
    for L, O in cg.RAGGED:
        assert (L, O) in cg.GEOMETRIES and (L % cg.cpt(L) != 0 or L < cg.THREADS * cg.cpt(L))
    for L, O in cg.CUT_SHORT:                        # the last thread with columns holds fewer than cpt
        assert L % cg.cpt(L) != 0
    for L, O in cg.FULL:
        assert (L, O) in cg.GEOMETRIES and L == cg.THREADS * cg.cpt(L)
    assert (3841 // 16, 3841 % 16, cg.THREADS - 241) == (240, 1, 15) and -(-257 // 2) == 129 and -(-513 // 3) == 171


@GEO
def test_case_discriminates(geo):
    L, O = geo
    case = cg.geometry_case(L, O)
    lay = case.lay
    assert lay.n_regions == 3 and lay.ref_start.tolist() == [0, 700, 9_000] and lay.n * L <= 70_000
    assert (lay.index > 0).any() and (lay.index[lay.region != 1] <= 0).all()            # inserts, in one region
    assert (lay.position < 0).any() or L - O == 1                                        # padding rows (a step of 1 leaves none)
    assert any(chr(b) in "Nn" for b in lay.ref.tolist()) and any(chr(b) in "acgt" for b in lay.ref.tolist())
    for g in range(3):
        mine = np.flatnonzero(lay.region == g)
        assert len(lay.rows[g]) >= 3 * L and len(mine) >= 3                              # a chunk with both neighbours
        assert (lay.position[mine[1]] >= 0).all()
    kept = _kept(lay)
    assert kept[lay.region == 1].any() and kept[lay.region == 2].any() and not kept.all()
    k, j, k2, j2 = cg.shared_columns(lay)
    if O == 0:
        assert len(k) == 0
        return
    own = case.owned
    both = kept[k, j]
    assert np.array_equal(both, kept[k2, j2]) and both.any()
    assert (own[k, j][both] != own[k2, j2][both]).all()                                   # one copy owns a kept key
    assert not own[k, j][~both].any() and not own[k2, j2][~both].any()
    a, b = case.labels[k, j], case.labels[k2, j2]
    win = np.where(own[k, j], a, b)
    lose = np.where(own[k, j], b, a)
    for g in range(3):
        mine = both & (lay.region[k] == g)
        assert int((mine & (a != b) & (a > 0) & (b > 0)).sum()) >= min(O, 8), g
    assert (both & (win == 0) & (lose > 0)).any() and (both & (win > 0) & (lose == 0)).any()
    assert (case.rq[k, j] != case.rq[k2, j2]).all()
    # the depth plane: the copies agree, and the median is a threshold with rows on either side
    assert np.array_equal(case.depth[k, j], case.depth[k2, j2])
    real = case.depth[lay.position >= 0]
    assert (real < case.min_depth).any() and (real >= case.min_depth).any()


@GEO
def test_checkers_agree(geo):
    L, O = geo
    case = cg.geometry_case(L, O)
    lay = case.lay
    seqs = case.stitch_seq
    assert [s for s, _ in case.stitch_qual] == seqs and all(len(s) == len(q) for s, q in case.stitch_qual)
    assert all(len(s) > 0 for s in seqs)
    assert sum(len(s) for s in seqs) == sr.kept_nonzero_count(lay.position, lay.index, case.labels, lay.region, lay.chunk_id, lay.ref_start)
    records, off = case.edits(True)
    kinds = [r[2] for r in records]
    assert all(kinds.count(x) > 0 for x in (er.SUB, er.DEL, er.INS)) and off[-1] == len(records)
    assert [r[:5] for r in case.edits(False)[0]] == [r[:5] for r in records] and {r[5] for r in case.edits(False)[0]} == {255}
    for g, pred in enumerate(case.dicts):
        draft = case.contig_draft(g)
        vcf = er.vcf_records(er.replacements(pred, draft, 0), draft, True)
        assert er.apply(vcf, draft, case.cut(g)) == seqs[g].decode(), g
        assert er.polished(pred, draft, 0) == seqs[g].decode(), g
    # owned_mask marks exactly one copy of every kept key
    own = case.owned
    gg = np.broadcast_to(lay.region[:, None], own.shape)
    keys = set(zip(gg[own].tolist(), lay.position[own].tolist(), lay.index[own].tolist()))
    assert len(keys) == int(own.sum()) == sum(len(d) for d in case.dicts)
    assert keys == {(g, p, x) for g, d in enumerate(case.dicts) for p, x in d}
    assert not own[~_kept(lay)].any()
    # mask and filter change something and leave something
    m_lab, m_q, masked, unmaskable = case.masked
    assert masked > 0 and unmaskable > 0 and (m_lab == case.labels).any() and int((m_q != case.rq).sum()) <= masked
    f_lab, f_q, reverted, pinned, gone = case.filtered
    assert reverted > 0 and pinned > 0 and int((f_lab != case.labels).sum()) == reverted
    assert np.array_equal(f_lab[~own], case.labels[~own]) and np.array_equal(f_q[~own], case.rq[~own])
    # row qualities: the planted rows hold what the hand-worked cases say, for each count the geometry has
    want = qr.row_qual(case.labels, case.acc, O).reshape(-1)
    cnt = np.tile(qr.row_counts(L, O), lay.n)
    assert {float(cnt[t]) for t in case.planted} == ({1.0} if 2 * O == L else {2.0} if O == 0 else {1.0, 2.0})
    assert len(case.planted) == 16 * (1 + (0 < 2 * O < L)) and all(want[t] == q for t, q in case.planted.items())


@pytest.mark.parametrize("n_chunks", cg.N_CHUNKS)
def test_count_cases(n_chunks):
    case = cg.count_case(n_chunks)
    lay = case.lay
    assert lay.n == n_chunks and (lay.L, lay.O) == (8, 4)
    per = -(-n_chunks // cg.FOLD_THREADS)
    assert per == (1 if n_chunks <= 1024 else 2 if n_chunks <= 2048 else 3)
    assert sum(len(s) for s in case.stitch_seq) == sr.kept_nonzero_count(lay.position, lay.index, case.labels, lay.region,
                                                                          lay.chunk_id, lay.ref_start)
    for k in {0, n_chunks - 1, min(per - 1, n_chunks - 1), min(per, n_chunks - 1)}:      # where the poisoned labels go
        assert case.owned[k].any(), k
    assert cg.N_CHUNKS == (1, 2, 1023, 1024, 1025, 2047, 2048, 2049)


def test_decade_case_tells_string_order_from_numeric_order():
    lay = cg.decade_layout()
    spans = list(zip(lay.ref_start.tolist(), lay.ref_end.tolist()))

    def numeric_stitch(reg):
        """stitch_ref.small_chunk_stitch for one region, the chunk ids walked as numbers"""
        pred = {}
        for c in sorted(reg.chunks):
            for pos, indx, base in zip(*(a.tolist() for a in reg.chunks[c])):
                if not (reg.start > 0 and pos <= reg.start + sr.BUFFER_POSITIONS) and indx >= 0 and pos >= 0:
                    pred[(pos, indx)] = base
        return "".join(sr.LABEL_DECODER[pred[k]] for k in sorted(pred))

    # every pair of adjacent chunks disagrees on what it shares: the two orders differ on the decade steps and nowhere else
    labels = np.broadcast_to((1 + lay.chunk_id % 4).astype(np.uint8)[:, None], lay.position.shape)
    reg = sr.regions_from_chunks(lay.position, lay.index, lay.region, lay.chunk_id, labels, spans)[0]
    by_string, by_number = sr.create_consensus_sequence([reg]), numeric_stitch(reg)
    assert len(by_string) == len(by_number) == 4_100
    differ = [p for p in range(4_100) if by_string[p] != by_number[p]]
    assert differ == [4 * (c + 1) + i for c in cg.DECADE_STRING_OWNER for i in range(4)]
    assert all(str(c) > str(c + 1) for c in cg.DECADE_STRING_OWNER)
    assert [c for c in range(1023) if str(c) > str(c + 1)] == list(cg.DECADE_STRING_OWNER)
    # the case's own labels: C where the earlier chunk owns, G where the later one does, on the nine planted pairs
    labels = cg.decade_labels(lay)
    reg = sr.regions_from_chunks(lay.position, lay.index, lay.region, lay.chunk_id, labels, spans)[0]
    by_string, by_number = sr.create_consensus_sequence([reg]), numeric_stitch(reg)
    for c in cg.DECADE_C:
        at = slice(4 * (c + 1), 4 * (c + 1) + 4)
        assert by_string[at] == ("CCCC" if c in cg.DECADE_STRING_OWNER else "GGGG") and by_number[at] == "GGGG", c
    assert by_string.count("A") == 4_100 - 36
    own = mq.owned_mask(lay.position, lay.index, lay.region, lay.chunk_id, lay.ref_start, labels.shape)
    for c in cg.DECADE_C:
        assert own[c, 4:].all() == (c in cg.DECADE_STRING_OWNER) and own[c + 1, :4].all() != (c in cg.DECADE_STRING_OWNER), c
