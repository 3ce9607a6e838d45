"""Secondary figure: pv_assess_place_dev on a synthetic truth of 16 contigs (32 Mbp in all) and a 32 Mbp assembly cut from it
in 1 Mbp pieces, every other one reverse-complemented, with about 1 % planted errors, at step 1024, inputs resident in HBM.
The whole call is timed by events around blocks of calls, the sort and the pass over the truth by the context's own HIP events
(pv_profile_begin) in a profiled run of its own. The yardstick is the scoring behind it: pv_assess_dev on the pairs that the
placement composes (each piece, oriented, against its interval of the truth), timed the same way in the same process.
Writes profiles/assess_place_bench.json.
Runnable alone: python tools/bench_assess_place.py [--mbp 32] [--contigs 16] [--piece 1000000] [--step 1024] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_assess import synthetic_pair  # noqa: E402

COMPLEMENT = np.arange(256, dtype=np.uint8)
COMPLEMENT[np.frombuffer(b"ACGT", np.uint8)] = np.frombuffer(b"TGCA", np.uint8)


def synthetic(mbp, contigs, piece, error):
    """-> (assembly pieces, truth contigs, where = [(truth contig, strand, lo, hi)]), uint8 arrays"""
    per = int(mbp * 1e6) // contigs
    truth, asm, where = [], [], []
    for t in range(contigs):
        a, b, _ = synthetic_pair(per, error, seed=100 + t)
        truth.append(b)
        # cut the erroneous copy where the truth is cut: the copy's position of truth position x is found by its length ratio,
        # which is all the placement needs
        cuts = list(range(0, per, piece)) + [per]
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            p = a[lo * len(a) // per:hi * len(a) // per]
            strand = (len(asm) & 1)
            asm.append(COMPLEMENT[p][::-1].copy() if strand else p)
            where.append((t, strand, lo, hi))
    return asm, truth, where


def timed(torch, stream, call, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(n):
        call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def run(ctx, dev, mbp=32.0, contigs=16, piece=1000000, step=1024, min_hits=3, error=0.01, reps=20, blocks=5, segment=1024,
        max_shift=8192):
    import torch
    from pepper_thesis_amd import _ffi
    asm, truth, where = synthetic(mbp, contigs, piece, error)
    n, m = len(asm), len(truth)
    a_off = np.zeros(n + 1, np.int64)
    b_off = np.zeros(m + 1, np.int64)
    a_off[1:] = np.cumsum([len(a) for a in asm])
    b_off[1:] = np.cumsum([len(b) for b in truth])
    need = ctx.assess_place_scratch_bytes(a_off, step)
    up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    A, B, ao, bo = up(np.concatenate(asm)), up(np.concatenate(truth)), up(a_off), up(b_off)
    recs = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream

    def place():
        ctx.assess_place_dev(A.data_ptr(), ao.data_ptr(), n, B.data_ptr(), bo.data_ptr(), m, step, min_hits, recs.data_ptr(),
                             scratch.data_ptr(), need, cnt.data_ptr(), stream=st)
    for _ in range(3):
        place()
    torch.cuda.synchronize()
    assert cnt.tolist()[:3] == [n, 0, -1], cnt.tolist()
    r = recs.cpu().numpy().reshape(-1).view(np.dtype(_ffi.pv_assess_placement))
    assert (r["status"] == _ffi.PV_ASSESS_PLACED).all() and [(int(x["truth"]), int(x["strand"])) for x in r] == [w[:2] for w in where]
    off_by = max(max(abs(int(x["b_lo"]) - w[2]), abs(int(x["b_hi"]) - w[3])) for x, w in zip(r, where))

    # the scoring behind it: the composed pairs through pv_assess_dev
    pa = [COMPLEMENT[a][::-1].copy() if int(x["strand"]) else a for a, x in zip(asm, r)]
    pb = [truth[int(x["truth"])][int(x["b_lo"]):int(x["b_hi"])] for x in r]
    pa_off, pb_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    pa_off[1:] = np.cumsum([len(a) for a in pa])
    pb_off[1:] = np.cumsum([len(b) for b in pb])
    cap = int(sum(len(a) // segment + 1 for a in pa))
    s_need = ctx.assess_scratch_bytes(pa_off, segment)
    PA, PB, pao, pbo = up(np.concatenate(pa)), up(np.concatenate(pb)), up(pa_off), up(pb_off)
    segs = torch.zeros((cap, 8), dtype=torch.int64, device=dev)
    so = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    tot = torch.zeros((n, 16), dtype=torch.int64, device=dev)
    s_scratch = torch.zeros(s_need, dtype=torch.uint8, device=dev)
    s_cnt = torch.zeros(4, dtype=torch.int64, device=dev)

    def score():
        ctx.assess_dev(PA.data_ptr(), pao.data_ptr(), PB.data_ptr(), pbo.data_ptr(), n, segment, max_shift, cap, segs.data_ptr(),
                       so.data_ptr(), tot.data_ptr(), s_scratch.data_ptr(), s_need, s_cnt.data_ptr(), stream=st)
    for _ in range(2):
        score()
    torch.cuda.synchronize()
    assert int(s_cnt[1]) == 0, s_cnt.tolist()
    per = max(1, reps // blocks)
    t_place, t_score = [], []
    for _ in range(blocks):
        t_place.append(timed(torch, stream, place, per))
        t_score.append(timed(torch, stream, score, per))
    ctx.profile_begin("k_pl_")
    for _ in range(per):
        place()
    torch.cuda.synchronize()
    prof = {k: v[0] / v[1] for k, v in ctx.profile_end().items()}
    t = tot.cpu().numpy().sum(axis=0)
    truth_bases, ms = int(b_off[-1]), float(np.median(t_place))
    return {"workload": "truth %d contigs, %d bases; assembly %d pieces, %d bases, every other one reverse-complemented, %.1f %% "
                        "planted errors" % (m, truth_bases, n, int(a_off[-1]), 100 * error),
            "step": step, "min_hits": min_hits, "samples": int(sum((len(a) - 32) // step + 1 for a in asm)),
            "scratch_mib": round(need / 2**20, 2), "blocks": blocks, "reps_per_block": per,
            "placed": int((r["status"] == 0).sum()), "interval_ends_off_by_at_most": off_by,
            "assess_place_dev_ms": stats(t_place), "kernel_ms": {k: round(v, 3) for k, v in sorted(prof.items())},
            "scan_truth_mbp_per_s": round(truth_bases / prof["k_pl_scan"] / 1e3, 1),
            "sort_share_of_call": round(prof["k_pl_sort"] / ms, 3),
            "assess_dev_ms_on_the_placed_pairs": stats(t_score), "assess_dev_scratch_mib": round(s_need / 2**20, 1),
            "assess_dev_unaligned_segments": int(t[2]),
            "placement_over_scoring": round(ms / float(np.median(t_score)), 3),
            "note": "both calls timed by events around blocks of unprofiled calls, alternating; kernel_ms: HIP events around "
                    "the sort's launches and the pass over the truth in a profiled run of pv_assess_place_dev of its own"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=32.0)
    ap.add_argument("--contigs", type=int, default=16)
    ap.add_argument("--piece", type=int, default=1000000)
    ap.add_argument("--step", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "assess_place_bench.json"))
    args = ap.parse_args()
    from pepper_thesis_amd import runtime
    ctx = runtime.Context(0)
    res = run(ctx, "cuda:0", args.mbp, args.contigs, args.piece, args.step, reps=args.reps)
    ctx.close()
    with open(args.output, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
