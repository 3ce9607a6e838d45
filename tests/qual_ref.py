"""Host checker of the polisher's per-base quality (include/pepper_hip.h, pv_polish_row_qual / pv_polish_stitch_qual).

The row rule in numpy float32, with the thresholds computed the way the rule defines them (not read from the library):
  cnt = 1 on the seq_overlap rows at either end of a chunk, else 2 (the reference's `counts`, predict_distributed_gpu.py:96-104);
  err = float32(1) - acc[r][label[r]] / cnt;   q = #{k in 1..93 : err <= T[k]},  T[k] = float32(10^(-k/10)).
The stitch of the quality plane works the reference's way, on tests/stitch_ref.py: one dict keyed by (position, index), a
region's chunk ids walked in STRING order, a global sort, and `base != 0` deciding which columns give a byte (Stitch.py:37-91,
where the quality string is commented out).
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np

import stitch_ref as sr

QUAL_MAX = 93
T = np.float32(10.0 ** (-np.arange(1, 94) / 10.0))   # T[k - 1] is the rule's T[k]


def row_counts(L: int = 1000, O: int = 50) -> np.ndarray:
    cnt = np.full(L, 2.0, np.float32)
    cnt[:O] = 1.0
    cnt[L - O:] = 1.0
    return cnt


def qual_of_err(err) -> np.ndarray:
    """float32 err (any shape) -> uint8 q; a NaN passes no threshold"""
    err = np.asarray(err, np.float32)
    return (err[..., None] <= T).sum(-1).astype(np.uint8)


def row_qual(labels, acc, O: int = 50) -> np.ndarray:
    """labels uint8 [B, L], acc float32 [B, L, 5] -> uint8 [B, L]; a label above 4 gives 0"""
    labels = np.asarray(labels, np.uint8)
    acc = np.asarray(acc, np.float32)
    assert labels.ndim == 2 and acc.shape == labels.shape + (5,)
    ok = labels <= 4
    v = np.take_along_axis(acc, np.where(ok, labels, 0).astype(np.intp)[..., None], axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        err = np.float32(1.0) - v / row_counts(labels.shape[1], O)[None, :]
        assert err.dtype == np.float32
        q = qual_of_err(err)
    q[~ok] = 0
    return q


def regions_with_qual(position, index, region, chunk_id, labels, row_q, spans: Sequence[Tuple[int, int]]) -> List[sr.RegionChunks]:
    """sr.regions_from_chunks with a fourth array per chunk: its row qualities"""
    regs = [sr.RegionChunks(s, e) for s, e in spans]
    for k in range(len(chunk_id)):
        regs[int(region[k])].chunks[int(chunk_id[k])] = (np.asarray(position[k]), np.asarray(index[k]), np.asarray(labels[k]),
                                                         np.asarray(row_q[k]))
    return regs


def small_chunk_stitch_qual(regions: Sequence[sr.RegionChunks]):
    """sr.small_chunk_stitch carrying (base, quality) -> (first_pos, last_pos, sequence, raw quality bytes)"""
    pred = {}
    for reg in regions:
        for name in sorted(str(c) for c in reg.chunks):
            positions, indices, bases, quals = reg.chunks[int(name)]
            for pos, indx, base, q in zip(positions.tolist(), indices.tolist(), bases.tolist(), quals.tolist()):
                if reg.start > 0 and pos <= reg.start + sr.BUFFER_POSITIONS:
                    continue
                if indx < 0 or pos < 0:
                    continue
                pred[(pos, indx)] = (base, q)
    if not pred:
        return -1, -1, "", b""
    keys = sorted(pred)
    seq = "".join(sr.LABEL_DECODER[pred[k][0]] for k in keys)
    qual = bytes(pred[k][1] for k in keys if pred[k][0] != 0)
    assert len(qual) == len(seq)
    return keys[0][0], keys[-1][0], seq, qual


def create_consensus_qual(regions: Sequence[sr.RegionChunks], threads: int = 1) -> Tuple[str, bytes]:
    """sr.create_consensus_sequence for (sequence, qualities)"""
    regs = sorted(regions, key=lambda r: (r.start, r.end))
    step = max(2, int(len(regs) / threads) + 1)
    parts = [small_chunk_stitch_qual(regs[i:i + step]) for i in range(0, len(regs), step)]
    parts = sorted((p for p in parts if p[0] != -1 and p[1] != -1), key=lambda p: (p[0], p[1]))
    return "".join(p[2] for p in parts), b"".join(p[3] for p in parts)


def stitch_contigs_qual(position, index, region, chunk_id, labels, row_q, names: Sequence[Tuple[str, int, int]],
                        threads: int = 1) -> Dict[str, Tuple[str, bytes]]:
    """names[g] = (contig, start, end) of batch region g -> {contig: (polished sequence, raw qualities)}"""
    regs = regions_with_qual(position, index, region, chunk_id, labels, row_q, [(s, e) for _, s, e in names])
    by: Dict[str, List[sr.RegionChunks]] = {}
    for (c, _, _), r in zip(names, regs):
        by.setdefault(c, []).append(r)
    return {c: create_consensus_qual(rs, threads) for c, rs in by.items()}


def fastq_text(contigs: Dict[str, Tuple[str, bytes]]) -> bytes:
    """one four-line record per contig with a non-empty sequence, natural contig order, qualities + 33"""
    out = b""
    for c in sorted(contigs, key=sr.natural_key):
        seq, q = contigs[c]
        if seq:
            out += b"@" + c.encode() + b"\n" + seq.encode() + b"\n+\n" + bytes(v + 33 for v in q) + b"\n"
    return out


def threshold_rows(rng=None):
    """hand-placed rows around the thresholds: -> (label, acc value, cnt, expected q) tuples. For cnt in (1, 2) and
    k in (1, 10, 20, 93): acc values whose err is T[k] exactly where float32 allows, and the neighbouring float32 values of
    acc (one ulp to either side); then err = 0, err < 0 and NaN. The expected q is worked from the definition with Python
    floats (float64 holds every float32 sum, quotient by 2 and difference from 1 here exactly, rounded once to float32)."""
    rows = []

    def q_of(v: np.float32, cnt: float) -> int:
        if np.isnan(v):
            return 0
        quo = np.float32(float(v) / cnt)                 # exact for cnt 1, 2 (barring underflow, not reached here)
        err = np.float32(1.0 - float(quo))               # one rounding, as the float32 subtract
        return int(sum(1 for k in range(1, 94) if float(err) <= float(T[k - 1])))

    for cnt in (1.0, 2.0):
        for k in (1, 10, 20, 93):
            v0 = np.float32((1.0 - float(T[k - 1])) * cnt)
            for v in (np.nextafter(v0, np.float32(-np.inf)), v0, np.nextafter(v0, np.float32(np.inf))):
                rows.append((k % 5, np.float32(v), cnt, q_of(np.float32(v), cnt)))
        rows.append((1, np.float32(cnt), cnt, 93))                                        # err = 0
        rows.append((2, np.nextafter(np.float32(cnt), np.float32(np.inf)), cnt, 93))      # err < 0: acc a hair over cnt
        rows.append((3, np.float32(np.nan), cnt, 0))
        rows.append((4, np.float32(0.0), cnt, 0))                                         # err = 1 > T[1]
    return rows
