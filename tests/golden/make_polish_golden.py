"""Generates tests/golden/polish_golden.npz from the REFERENCE's own polisher code.

Run in the build container only (needs /root/reference and oracle/_ref/libref_polish.so, which `make -C oracle` builds):
`python tests/golden/make_polish_golden.py`. Expected values come from
  - SummaryGenerator::generate_summary (summary_generator.cpp) through oracle.reference_polish_flat,
  - ReadAligner::align_reads_to_reference (simple_aligner.cpp) through oracle.reference_polish_realign,
  - AlignmentSummarizer.chunk_images (AlignmentSummarizer.py), imported from the reference with a stand-in
    `pepper.build` module (the pybind11 extension, which chunk_images does not use) that is removed afterwards.
Inputs and outputs are stored as arrays only (data): quals are not stored (the polisher builder does not read them).

Keys:
  names                                builder cases
  <case>/in/<field>                    the packed batch (pv_batch_in fields)
  <case>/flat_images, flat_position, flat_index, region_row_off     SummaryGenerator.image / genomic_pos, per region
  <case>/sizes                         [(L, O)] at which chunks are stored
  <case>/L<L>_O<O>/images, position, index, region, chunk_id        chunk_images, region after region, padding included
  chain_names                          cases realigned first (create_summary with realignment_flag=True)
  chain/<name>/in/<field>, chain/<name>/win_off, win                the input batch and the realignment windows
  chain/<name>/realign_state, realign_pos, realign_cigar_off, realign_cigar   ReadAligner per input read
  chain/<name>/flat_*, L1000_O50/*     as above, on the realigned reads
  chunk_table/L<L>_O<O>/n, off, start, end   chunk_images' (start, end) spans for every n of the table
"""
import os
import sys
import types
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import realign_cases as rc  # noqa: E402
from oracle import oracle  # noqa: E402
from pepper_thesis_amd import realign, synth  # noqa: E402
from pepper_thesis_amd.batch import Read, Region, pack_regions  # noqa: E402
from test_oracle_polish import POLISH_EDGE_REGIONS, _reads_of  # noqa: E402

REFERENCE = "/root/reference"
IN_FIELDS = ("ref_start", "ref_end", "ref_off", "ref", "read_off", "read_pos", "read_flags", "read_mapq", "base_off",
             "bases", "cigar_off", "cigar")
SMALL_ROWS = 3000          # cases up to this many rows are also chunked at (64, 8) and (7, 0)
TABLE_SIZES = ((1000, 50), (100, 0), (64, 8), (16, 3), (7, 6))
TILE, BLOCK, WAVE = 512, 1024, 64   # k_polish_tiles columns per tile; k_polish_blk / k_polish_insoff block and wave


def reference_chunk_images():
    """AlignmentSummarizer.chunk_images from the reference, imported with a stand-in pepper.build"""
    saved = {k: sys.modules[k] for k in list(sys.modules) if k == "pepper" or k.startswith("pepper.")}
    for k in saved:
        del sys.modules[k]
    stub = types.ModuleType("pepper.build")
    stub.PEPPER = None
    sys.modules["pepper.build"] = stub
    sys.path.insert(0, REFERENCE)
    try:
        from pepper.modules.python.AlignmentSummarizer import AlignmentSummarizer
        return AlignmentSummarizer.chunk_images
    finally:
        sys.path.remove(REFERENCE)
        for k in [k for k in sys.modules if k == "pepper" or k.startswith("pepper.")]:
            del sys.modules[k]
        sys.modules.update(saved)


chunk_images = reference_chunk_images()


class _Summary:
    def __init__(self, image, genomic_pos):
        self.image, self.genomic_pos = image, genomic_pos


# ---- hand-made builder cases ----------------------------------------------------------------------------------------

def _rng_bases(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _ins_read(rng, anchor, k, before=6, after=6, rev=False, mapq=60):
    """a read whose k-base insert is anchored on reference column `anchor`"""
    cigar = "%dM%dI" % (before, k) + ("%dM" % after if after else "")
    return Read.make(anchor - before + 1, cigar, _rng_bases(rng, before + k + after), is_reverse=rev, mapq=mapq)


def hand_cases():
    rng = np.random.default_rng(7)
    out = {}
    # columns 10..12 covered only by deletions that start at 9: count / max(1, 0) * 254 wraps (2x: 508 -> 252,
    # 3x: 762 -> 250); the start column books the deletions' coverage once per deleted column
    out["del_only_2x"] = [Region(9, 13, b"NNNNN", [Read.make(9, "1M3D1M", "AC"), Read.make(9, "1M3D1M", "AC")])]
    out["del_only_3x"] = [Region(9, 14, b"NNNNNN", [Read.make(9, "1M3D1M", "AC", is_reverse=k == 1) for k in range(3)] +
                                 [Read.make(10, "2D3M", "GGT")])]
    # a column deeper than 255 reads, a deletion-only column below 300 deletions (76200 -> low byte) and mixed columns
    deep = [Read.make(100, "5M", _rng_bases(rng, 5), is_reverse=bool(k & 1)) for k in range(300)]
    deep += [Read.make(104, "1M4D2M", "ACG") for _ in range(300)]
    deep += [Read.make(100, "3M2I3M", _rng_bases(rng, 8)) for _ in range(40)]
    out["coverage_300"] = [Region(100, 112, b"A" * 13, deep)]
    # inserts of 1..400 bases on distinct anchors (insert rows with index > 255), some anchors shared by two lengths
    reads, anchor = [], 20
    for k in list(range(1, 12)) + [63, 64, 65, 127, 128, 200, 254, 255, 256, 257, 300, 399, 400]:
        reads.append(_ins_read(rng, anchor, k, rev=bool(k & 1)))
        if k in (64, 256, 400):
            reads.append(_ins_read(rng, anchor, k // 2 + 1, rev=True))
        anchor += 11
    out["long_inserts"] = [Region(10, anchor + 20, b"C" * (anchor + 11), reads)]
    # inserts anchored on ref_end (dropped by the `ref_position > region_end` break) and on ref_end - 1 (kept)
    out["insert_at_ref_end"] = [Region(100, 150, b"G" * 51, [
        Read.make(141, "10M5I", _rng_bases(rng, 15)), Read.make(141, "10M3I2M", _rng_bases(rng, 15)),
        Read.make(140, "10M4I", _rng_bases(rng, 14), is_reverse=True), Read.make(140, "10M2I5M", _rng_bases(rng, 17)),
        Read.make(100, "51M", _rng_bases(rng, 51))])]
    # reads starting before the region: clipped M runs, soft clip, an insert anchored before the start and on it
    out["before_start"] = [Region(100, 140, b"T" * 41, [
        Read.make(90, "5S30M", _rng_bases(rng, 35)), Read.make(80, "15M3I10M2D20M", _rng_bases(rng, 48)),
        Read.make(95, "5M2I30M", _rng_bases(rng, 37), is_reverse=True), Read.make(70, "20M", _rng_bases(rng, 20)),
        Read.make(90, "4H3S12M4I6M", _rng_bases(rng, 25)), Read.make(99, "1M1I40M", _rng_bases(rng, 42))])]
    # a deletion spanning the whole region (starts before it: no coverage booked inside), another ending on it
    out["del_whole_region"] = [Region(200, 220, b"A" * 21, [
        Read.make(195, "3M30D3M", "ACGTAC"), Read.make(195, "3M30D3M", "ACGTAC", is_reverse=True),
        Read.make(200, "5M", "ACGTA"), Read.make(210, "2M20D1M", "ACG"), Read.make(215, "3M3N3M", "CCCGGG")])]
    # lower-case, IUPAC and N bases, in M runs and inserts, both strands
    odd = b"acgtnNRYKMSWBDHVuU*=.-"
    out["odd_bases"] = [Region(300, 340, b"acgtNRYK" * 5 + b"a", [
        Read.make(300, "41M", _rng_bases(rng, 41, odd)), Read.make(300, "41M", _rng_bases(rng, 41, odd), is_reverse=True),
        Read.make(305, "5M6I10M", _rng_bases(rng, 21, odd)), Read.make(310, "5M6I10M", _rng_bases(rng, 21, odd), is_reverse=True),
        Read.make(320, "10M", "acgtACGTnN")])]
    # mapq 0 is skipped, mapq 1 counts
    out["mapq_0_1"] = [Region(50, 70, b"C" * 21, [
        Read.make(50, "21M", _rng_bases(rng, 21), mapq=0), Read.make(50, "21M", _rng_bases(rng, 21), mapq=1),
        Read.make(55, "3M4I3M", _rng_bases(rng, 10), mapq=0), Read.make(55, "3M2I3M", _rng_bases(rng, 8), mapq=1),
        Read.make(60, "2M5D2M", "ACGT", mapq=0), Read.make(60, "2M3D2M", "ACGT", mapq=1, is_reverse=True)])]
    # a region starting at 0: an insert as the first op (anchor -1) and a deletion on column 0
    out["start_at_0"] = [Region(0, 30, b"A" * 31, [
        Read.make(0, "3I20M", _rng_bases(rng, 23)), Read.make(0, "2D10M", _rng_bases(rng, 10)),
        Read.make(0, "1M2I10M", _rng_bases(rng, 13), is_reverse=True), Read.make(0, "31M", _rng_bases(rng, 31))])]
    return out


def boundary_cases():
    """regions whose row count is exactly L-1, L, L+1, 2L-O-1, 2L-O, 2L-O+1 at (1000, 50), reached with inserts"""
    rng = np.random.default_rng(11)
    out = {}
    L, O = 1000, 50
    for j, n in enumerate((L - 1, L, L + 1, 2 * L - O - 1, 2 * L - O, 2 * L - O + 1)):
        n_ins = 3 + j
        total = 97 + 53 * j                   # insert rows
        R = n - total
        sizes = [total // n_ins] * n_ins
        sizes[-1] += total - sum(sizes)
        anchors = np.linspace(20, R - 20, n_ins).astype(int)
        reads = [Read.make(5000, "%dM" % R, _rng_bases(rng, R))]
        for a, k in zip(anchors.tolist(), sizes):
            reads.append(_ins_read(rng, 5000 + a, k, rev=bool(a & 1)))
            reads.append(_ins_read(rng, 5000 + a, max(1, k // 3)))
        out["rows_%d" % n] = [Region(5000, 5000 + R - 1, _rng_bases(rng, R), reads)]
    return out


def tile_cases():
    """k_polish_tiles' 512-column tiles and k_polish_blk / k_polish_insoff's 1024-column blocks (64-column waves)"""
    rng = np.random.default_rng(13)
    out = {}
    S = 10_000                                 # alone in a batch, column c of the region is global column c
    R = 1300
    reads = [Read.make(S, "%dM" % R, _rng_bases(rng, R)), Read.make(S, "%dM" % R, _rng_bases(rng, R), is_reverse=True)]
    for c in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE):
        reads.append(_ins_read(rng, S + c, 3 + c % 7, before=8, after=8))
        reads.append(_ins_read(rng, S + c, 1, before=c % 5 + 1, after=3, rev=True))
    for c in (TILE - 3, TILE - 1, TILE, 2 * TILE - 2):       # deletions crossing a tile boundary, starting on either side
        reads.append(Read.make(S + c - 4, "4M6D4M", _rng_bases(rng, 8), is_reverse=bool(c & 1)))
    reads.append(Read.make(S + TILE - 30, "60M", _rng_bases(rng, 60)))        # M runs crossing
    reads.append(Read.make(S + 2 * TILE - 1, "2M", _rng_bases(rng, 2)))
    reads.append(Read.make(S + TILE - 1, "1M600D1M", "AC"))                   # a deletion over a whole tile
    out["tile_edges"] = [Region(S, S + R - 1, _rng_bases(rng, R), reads)]
    # > 2 scan blocks: inserts on block boundaries (1023 | 1024, 2047 | 2048) and wave boundaries inside a block
    S, R = 20_000, 2600
    reads = [Read.make(S, "%dM" % R, _rng_bases(rng, R))]
    for c in (WAVE - 1, WAVE, BLOCK - WAVE - 1, BLOCK - WAVE, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + WAVE - 1, BLOCK + WAVE,
              2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 7 * WAVE, R - 2, R - 1):
        reads.append(_ins_read(rng, S + c, 1 + c % 13, before=10, after=min(10, R - 1 - c), rev=bool(c & 2)))
    out["scan_blocks"] = [Region(S, S + R - 1, _rng_bases(rng, R), reads)]
    return out


def random_cases():
    out = {}
    rng = np.random.default_rng(17)
    for k, (R, depth, rl) in enumerate(((5000, 40, 1500), (2000, 100, 300), (4000, 20, 3000), (1200, 80, 200),
                                        (2500, 8, 800))):
        reg = synth.synth_region(600 + k, region_len=R, depth=depth, read_len=rl, site_every=int(rng.integers(20, 120)),
                                 ref_start=int(rng.integers(0, 5)) * 1000 + 100, mismatch=0.01 + 0.01 * k,
                                 ins_rate=0.01 + 0.005 * k, del_rate=0.01 + 0.005 * k, n_rate=0.002 * (k % 2))
        mq = rng.choice([0, 1, 60, 60, 60, 60], len(reg.reads))
        reg.reads = [replace(rd, mapq=int(m)) for rd, m in zip(reg.reads, mq)]
        out["random%d" % k] = [reg]
    return out


def p1_edge_regions():
    b = cases.all_edges_batch()
    return [Region(int(b.ref_start[g]), int(b.ref_end[g]), b"N" * int(b.ref_end[g] - b.ref_start[g] + 1), _reads_of(b, g))
            for g in range(b.n_regions)]


# ---- expected values --------------------------------------------------------------------------------------------------

def _store_batch(blob, key, batch):
    for f in IN_FIELDS:
        blob["%s/in/%s" % (key, f)] = np.ascontiguousarray(getattr(batch, f))


def _store_outputs(blob, key, batch, sizes):
    img, pos, idx, off = oracle.reference_polish_flat(batch)
    blob[key + "/flat_images"], blob[key + "/flat_position"] = img, pos
    blob[key + "/flat_index"], blob[key + "/region_row_off"] = idx, off
    blob[key + "/sizes"] = np.asarray(sizes, np.int32)
    for L, O in sizes:
        ims, pss, ids, regs, cids = [], [], [], [], []
        for g in range(batch.n_regions):
            r0, r1 = int(off[g]), int(off[g + 1])
            summ = _Summary([list(map(int, r)) for r in img[r0:r1]], list(zip(pos[r0:r1].tolist(), idx[r0:r1].tolist())))
            images, labels, positions, chunk_ids = chunk_images(summ, L, O)
            for im, ps, cid in zip(images, positions, chunk_ids):
                ims.append(np.asarray(im, np.float64).astype(np.uint8))
                pa = np.asarray(ps, np.int64).reshape(L, 2)
                pss.append(pa[:, 0])
                ids.append(pa[:, 1].astype(np.int32))
                regs.append(g)
                cids.append(cid)
        k = "%s/L%d_O%d/" % (key, L, O)
        blob[k + "images"] = np.stack(ims)
        blob[k + "position"] = np.stack(pss)
        blob[k + "index"] = np.stack(ids)
        blob[k + "region"] = np.asarray(regs, np.int32)
        blob[k + "chunk_id"] = np.asarray(cids, np.int32)
    return len(img)


def builder_cases():
    out = {"polish_edges": POLISH_EDGE_REGIONS, "p1_edges": p1_edge_regions()}
    out.update(hand_cases())
    out.update(boundary_cases())
    out.update(tile_cases())
    out.update(random_cases())
    return out


def chain_cases():
    """the realignment fixture's regions with strands and mapq varied, and two seeded regions"""
    rng = np.random.default_rng(19)
    out = {}
    src = [(name, s, e, w, reads) for name, s, e, w, reads in rc.edge_regions()]
    for seed in range(3):
        s, e, w, reads = rc.random_region(300 + seed, start=2000 * seed, n_reads=40, long_ins=0.003 * seed)
        src.append(("random%d" % seed, s, e, w, reads))
    for name, s, e, w, reads in src:
        reads = [replace(rd, is_reverse=bool(rng.random() < 0.5), mapq=int(rng.choice([0, 1, 60, 60]))) for rd in reads]
        out[name] = (rc.as_region(s, e, w, reads), w)
    return out


def chunk_table(blob):
    for L, O in TABLE_SIZES:
        ns = list(range(1, 3 * L + 1)) + [10 * L + 3]
        offs, starts, ends = [0], [], []
        for n in ns:
            images, _, positions, _ = chunk_images(_Summary([[0] * 10] * n, [(i, 0) for i in range(n)]), L, O)
            for ps in positions:
                real = [p for p, _ in ps if p >= 0]
                starts.append(real[0])
                ends.append(real[-1] + 1)
            offs.append(len(starts))
        k = "chunk_table/L%d_O%d/" % (L, O)
        blob[k + "n"] = np.asarray(ns, np.int64)
        blob[k + "off"] = np.asarray(offs, np.int64)
        blob[k + "start"] = np.asarray(starts, np.int32)
        blob[k + "end"] = np.asarray(ends, np.int32)


def main():
    assert oracle.have_reference_polish(), "build oracle/_ref first: make -C oracle"
    blob = {}
    names = []
    for name, regs in builder_cases().items():
        b = pack_regions(regs)
        n = int((b.ref_end - b.ref_start + 1).sum())
        _store_batch(blob, name, b)
        img = oracle.reference_polish_flat(b)[0]
        sizes = [(1000, 50)] + ([(64, 8), (7, 0)] if len(img) <= SMALL_ROWS else [])
        rows = _store_outputs(blob, name, b, sizes)
        names.append(name)
        print("%-18s regions=%d columns=%6d rows=%6d reads=%5d sizes=%s" % (name, b.n_regions, n, rows, b.n_reads, sizes))
    blob["names"] = np.asarray(names, dtype="S")
    chain = []
    for name, (reg, w) in chain_cases().items():
        b = pack_regions([reg])
        woff, win = realign.pack_windows([w])
        st, pos, _, coff, cig = oracle.reference_polish_realign(b, woff, win)
        assert (st != 3).all(), name
        keep = st == 1
        reads = [Read(int(p), cig[coff[k]:coff[k + 1]].copy(), rd.bases, rd.quals, rd.is_reverse, rd.mapq)
                 for k, (p, rd) in enumerate(zip(pos.tolist(), reg.reads)) if keep[k]]
        rb = pack_regions([Region(reg.ref_start, reg.ref_end, reg.ref, reads)])
        key = "chain/" + name
        _store_batch(blob, key, b)
        blob[key + "/win_off"], blob[key + "/win"] = woff, win
        blob[key + "/realign_state"], blob[key + "/realign_pos"] = st, pos
        blob[key + "/realign_cigar_off"], blob[key + "/realign_cigar"] = coff, cig
        rows = _store_outputs(blob, key, rb, [(1000, 50)])
        chain.append(name)
        print("chain %-12s reads=%3d kept=%3d rows=%5d" % (name, b.n_reads, int(keep.sum()), rows))
    blob["chain_names"] = np.asarray(chain, dtype="S")
    chunk_table(blob)
    path = os.path.join(ROOT, "tests", "golden", "polish_golden.npz")
    np.savez_compressed(path, **blob)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
