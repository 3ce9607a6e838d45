"""Host checker of the haplotype selection (the rule of pv_batch_select_hp in include/pepper_hip.h) in plain numpy on a
RegionBatch: a boolean mask over the reads, then np.repeat / fancy indexing over the offsets. No scan, no gather by pieces."""
import numpy as np

from pepper_thesis_amd.batch import RegionBatch


def keep_mask(read_hp, n_reads: int, haplotype: int) -> np.ndarray:
    """kept iff untagged (no tags at all, or tag 0) or tagged with the haplotype"""
    assert haplotype >= 1
    if read_hp is None:
        return np.ones(n_reads, bool)
    hp = np.asarray(read_hp)
    assert hp.shape == (n_reads,)
    return (hp == 0) | (hp == haplotype)


def _payload(off, data, keep):
    """the elements of the kept reads, in order, and their new offsets"""
    lens = np.diff(off)
    new_off = np.concatenate([[0], np.cumsum(lens[keep])]).astype(np.int64)
    elem_keep = np.repeat(keep, lens)
    return new_off, data[off[0]:off[-1]][elem_keep]


def select(batch: RegionBatch, haplotype: int):
    """-> (RegionBatch of the kept reads: the region arrays are the input's own objects, src_read int64 [kept])"""
    n = batch.n_reads
    keep = keep_mask(batch.read_hp, n, haplotype)
    src = np.flatnonzero(keep).astype(np.int64)
    region_of = np.repeat(np.arange(batch.n_regions), np.diff(batch.read_off))
    per_region = np.bincount(region_of[keep], minlength=batch.n_regions)
    read_off = np.concatenate([[0], np.cumsum(per_region)]).astype(np.int64)
    base_off, bases = _payload(batch.base_off, batch.bases, keep)
    _, quals = _payload(batch.base_off, batch.quals, keep)
    cigar_off, cigar = _payload(batch.cigar_off, batch.cigar, keep)
    out = RegionBatch(batch.n_regions, batch.ref_start, batch.ref_end, batch.cand_start, batch.cand_end, batch.ref_off, batch.ref,
                      read_off, batch.read_pos[src], batch.read_flags[src], batch.read_mapq[src], base_off, bases, quals,
                      cigar_off, cigar, list(batch.contigs), None if batch.read_hp is None else np.asarray(batch.read_hp)[src])
    return out, src


READ_FIELDS = ("read_off", "read_pos", "read_flags", "read_mapq", "base_off", "bases", "quals", "cigar_off", "cigar")


def make_batch(read_lens, cigar_lens, reads_per_region, read_hp=None, seed=0) -> RegionBatch:
    """a batch with the given read and cigar lengths and random contents (the selection looks at offsets and tags only);
    every region is 10 columns of draft"""
    rng = np.random.default_rng(seed)
    read_lens, cigar_lens = np.asarray(read_lens, np.int64), np.asarray(cigar_lens, np.int64)
    per = np.asarray(reads_per_region, np.int64)
    n, G = len(read_lens), len(per)
    assert int(per.sum()) == n == len(cigar_lens)
    off = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)
    base_off, cigar_off = off(read_lens), off(cigar_lens)
    start = np.arange(G, dtype=np.int64) * 10
    return RegionBatch(G, start, start + 9, start.copy(), start + 9, off(np.full(G, 10)), rng.integers(65, 70, 10 * G).astype(np.uint8),
                       off(per), rng.integers(0, 1 << 40, n).astype(np.int64), rng.integers(0, 2, n).astype(np.uint8),
                       rng.integers(0, 61, n).astype(np.uint8), base_off, rng.integers(0, 256, int(base_off[-1])).astype(np.uint8),
                       rng.integers(0, 256, int(base_off[-1])).astype(np.uint8), cigar_off,
                       rng.integers(0, 1 << 32, int(cigar_off[-1]), dtype=np.uint64).astype(np.uint32), ["c"] * G,
                       None if read_hp is None else np.asarray(read_hp, np.int32))
