"""Host checker of the polisher's stitch: a plain-Python restatement of the reference's small_chunk_stitch +
create_consensus_sequence (pepper/modules/python/Stitch.py:37-128) and perform_stitch (perform_stitch.py:43-84).

It works the reference's way on purpose - one dict keyed by (position, index) per worker, a region's chunk ids walked in
STRING order (sorted HDF5 key names: "10" < "2"), a global sort, worker results ordered by their first position - so that
the tests see, rather than assume, that the device's per-region, chunk-major emission gives the same string.
"""
import re
from typing import Dict, List, Sequence, Tuple

import numpy as np

LABEL_DECODER = {0: "", 1: "A", 2: "C", 3: "G", 4: "T"}
BUFFER_POSITIONS = 2 * 100   # 2 * ImageSizeOptions.MIN_IMAGE_OVERLAP


class RegionChunks:
    """what the prediction file holds for one region: contig_start, contig_end and {chunk id: (position, index, bases)}"""

    def __init__(self, start: int, end: int):
        self.start, self.end = int(start), int(end)
        self.chunks: Dict[int, Tuple[np.ndarray, np.ndarray, np.ndarray]] = {}


def small_chunk_stitch(regions: Sequence[RegionChunks]):
    """Stitch.py:37-86 -> (first_pos, last_pos, sequence), (-1, -1, '') when nothing is kept"""
    pred = {}
    for reg in regions:
        for name in sorted(str(c) for c in reg.chunks):
            positions, indices, bases = reg.chunks[int(name)]
            for pos, indx, base in zip(positions.tolist(), indices.tolist(), bases.tolist()):
                if reg.start > 0 and pos <= reg.start + BUFFER_POSITIONS:
                    continue
                if indx < 0 or pos < 0:
                    continue
                pred[(pos, indx)] = base
    if not pred:
        return -1, -1, ""
    keys = sorted(pred)
    seq = "".join(LABEL_DECODER[pred[k]] for k in keys)   # KeyError on a label outside 0..4, as in the reference
    return keys[0][0], keys[-1][0], seq


def create_consensus_sequence(regions: Sequence[RegionChunks], threads: int = 1) -> str:
    """Stitch.py:89-128: regions sorted by (start, end), dealt to workers in runs of max(2, n // threads + 1)"""
    regs = sorted(regions, key=lambda r: (r.start, r.end))
    step = max(2, int(len(regs) / threads) + 1)
    parts = [small_chunk_stitch(regs[i:i + step]) for i in range(0, len(regs), step)]
    parts = sorted((p for p in parts if p[0] != -1 and p[1] != -1), key=lambda p: (p[0], p[1]))
    return "".join(p[2] for p in parts)


def natural_key(s: str):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]


def fasta_text(contig_seqs: Dict[str, str]) -> str:
    """perform_stitch.py:61-84: natural contig order, non-empty sequences only, one line each"""
    return "".join(">%s\n%s\n" % (c, contig_seqs[c]) for c in sorted(contig_seqs, key=natural_key) if contig_seqs[c])


def regions_from_chunks(position, index, region, chunk_id, labels, spans: Sequence[Tuple[int, int]]) -> List[RegionChunks]:
    """the builder's chunk arrays + P2 labels -> one RegionChunks per batch region (spans[g] = (start, end) of region g)"""
    regs = [RegionChunks(s, e) for s, e in spans]
    for k in range(len(chunk_id)):
        regs[int(region[k])].chunks[int(chunk_id[k])] = (np.asarray(position[k]), np.asarray(index[k]), np.asarray(labels[k]))
    return regs


def stitch_contigs(position, index, region, chunk_id, labels, names: Sequence[Tuple[str, int, int]], threads: int = 1) -> Dict[str, str]:
    """names[g] = (contig, start, end) of batch region g -> {contig: polished sequence}"""
    regs = regions_from_chunks(position, index, region, chunk_id, labels, [(s, e) for _, s, e in names])
    by_contig: Dict[str, List[RegionChunks]] = {}
    for (c, _, _), r in zip(names, regs):
        by_contig.setdefault(c, []).append(r)
    return {c: create_consensus_sequence(rs, threads) for c, rs in by_contig.items()}


def kept_nonzero_count(position, index, labels, region, chunk_id, region_start) -> int:
    """an independent count of the polished bases, in numpy: kept (region, position, index) triples, each taking the label of
    its chunk that is last in string order of the chunk id, counted where that label is non-zero"""
    pos, idx, lab = np.asarray(position), np.asarray(index), np.asarray(labels)
    g = np.broadcast_to(np.asarray(region)[:, None], pos.shape)
    ids = np.asarray(chunk_id)
    names = np.array([str(c) for c in ids])
    rank = np.broadcast_to(np.argsort(np.argsort(names, kind="stable"), kind="stable")[:, None], pos.shape)
    rs = np.asarray(region_start)[g]
    keep = (pos >= 0) & (idx >= 0) & ~((rs > 0) & (pos <= rs + BUFFER_POSITIONS))
    g, p, x, r, lb = g[keep], pos[keep], idx[keep], rank[keep], lab[keep]
    if not len(g):
        return 0
    o = np.lexsort((r, x, p, g))
    g, p, x, lb = g[o], p[o], x[o], lb[o]
    last = np.ones(len(g), bool)
    last[:-1] = (g[1:] != g[:-1]) | (p[1:] != p[:-1]) | (x[1:] != x[:-1])
    return int((lb[last] != 0).sum())
