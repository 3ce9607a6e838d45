"""Secondary figure: pv_assess_dev on one synthetic contig pair, 5 Mbp of random truth and an assembly with about 1 % planted
substitutions, deletions and insertions, inputs resident in HBM. Anchor search, band sweep and traceback are timed by the
context's own HIP events (pv_profile_begin), the whole call by events around it. Writes profiles/assess_bench.json.
--errors adds a leg under the key "errors": pv_assess_errors_dev with a quality array against pv_assess_dev on the same
workload in the same process, each in five blocks of repetitions so that the run-to-run spread shows.
Runnable alone: python tools/bench_assess.py [--mbp 5] [--error 0.01] [--segment 1024] [--reps 50] [--errors]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_pair(n, error, seed=20):
    """-> (assembly, truth) uint8 arrays: every truth base is, with probability `error`, substituted, dropped or followed by
    an extra base (a third each)"""
    rng = np.random.default_rng(seed)
    truth = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    kind = rng.choice(4, n, p=[1 - error, error / 3, error / 3, error / 3])
    asm = truth.copy()
    sub = kind == 1
    asm[sub] = np.frombuffer(b"ACGT", np.uint8)[(rng.integers(1, 4, int(sub.sum())) + np.searchsorted(
        np.frombuffer(b"ACGT", np.uint8), truth[sub])) % 4]
    reps = np.ones(n, np.int64)
    reps[kind == 2] = 0
    reps[kind == 3] = 2
    return np.repeat(asm, reps), truth, {"sub": int(sub.sum()), "del": int((kind == 2).sum()), "ins": int((kind == 3).sum())}


def run(ctx, dev, mbp=5.0, error=0.01, segment=1024, max_shift=8192, reps=50):
    import torch
    asm, truth, planted = synthetic_pair(int(mbp * 1e6), error)
    a_off = np.array([0, len(asm)], np.int64)
    b_off = np.array([0, len(truth)], np.int64)
    cap = len(asm) // segment + 1
    need = ctx.assess_scratch_bytes(a_off, segment)
    A, B = torch.from_numpy(asm).to(dev), torch.from_numpy(truth).to(dev)
    ao, bo = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
    segs = torch.zeros((cap, 8), dtype=torch.int64, device=dev)
    so = torch.zeros(2, dtype=torch.int64, device=dev)
    tot = torch.zeros((1, 16), dtype=torch.int64, device=dev)
    scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream

    def call():
        ctx.assess_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), 1, segment, max_shift, cap, segs.data_ptr(),
                       so.data_ptr(), tot.data_ptr(), scratch.data_ptr(), need, cnt.data_ptr(), stream=st)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert int(cnt[1]) == 0, cnt.tolist()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        call()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    ctx.profile_begin("k_as_")
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    prof = ctx.profile_end()
    t = tot.cpu().numpy()[0]
    M, S, I, D = (int(t[k]) for k in (4, 5, 6, 7))
    return {"workload": "1 pair, truth %d bases, assembly %d bases, planted %s" % (len(truth), len(asm), planted),
            "segment": segment, "max_shift": max_shift, "reps": reps, "scratch_mib": round(need / 2**20, 1),
            "ms_per_call": round(ms, 3), "mbp_per_s": round(len(asm) / ms / 1e3, 1),
            "kernel_ms": {k: round(v[0] / v[1], 3) for k, v in sorted(prof.items())},
            "segments": int(t[0]), "unaligned": int(t[2]), "edge": int(t[3]), "matches": M, "sub": S, "ins": I, "del": D,
            "qv": round(-10 * np.log10(max(S + I + D, 1) / (M + S + I + D)), 2),
            "note": "kernel_ms: HIP events around each launch (a profiled run of its own); ms_per_call: events around the "
                    "unprofiled call, all seven launches"}


def run_errors(ctx, dev, mbp=5.0, error=0.01, segment=1024, max_shift=8192, reps=50, blocks=5):
    """pv_assess_errors_dev (qualities given: every launch runs) and pv_assess_dev, interleaved block by block"""
    import torch
    asm, truth, planted = synthetic_pair(int(mbp * 1e6), error)
    qual = np.random.default_rng(21).integers(2, 61, len(asm)).astype(np.uint8)
    a_off = np.array([0, len(asm)], np.int64)
    b_off = np.array([0, len(truth)], np.int64)
    cap = len(asm) // segment + 1
    ecap = (len(asm) + len(truth)) // 16 + 1024
    need = ctx.assess_errors_scratch_bytes(a_off, segment)
    A, B, Q = (torch.from_numpy(x).to(dev) for x in (asm, truth, qual))
    ao, bo = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
    segs = torch.zeros((cap, 8), dtype=torch.int64, device=dev)
    so, eo = (torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(2))
    tot = torch.zeros((1, 16), dtype=torch.int64, device=dev)
    errs = torch.zeros((ecap, 4), dtype=torch.int64, device=dev)
    qh = torch.zeros((1, 94, 4), dtype=torch.int64, device=dev)
    scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    st = stream.cuda_stream

    def plain():
        ctx.assess_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), 1, segment, max_shift, cap, segs.data_ptr(),
                       so.data_ptr(), tot.data_ptr(), scratch.data_ptr(), need, cnt.data_ptr(), stream=st)

    def with_errors():
        ctx.assess_errors_dev(A.data_ptr(), ao.data_ptr(), B.data_ptr(), bo.data_ptr(), 1, segment, max_shift, cap,
                              segs.data_ptr(), so.data_ptr(), tot.data_ptr(), Q.data_ptr(), ecap, errs.data_ptr(), eo.data_ptr(),
                              qh.data_ptr(), scratch.data_ptr(), need, cnt.data_ptr(), stream=st)

    def timed(call, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            call()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    for _ in range(3):
        plain()
        with_errors()
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert int(c[1]) == 0, c.tolist()
    per = max(1, reps // blocks)
    t_plain, t_err = [], []
    for _ in range(blocks):
        t_plain.append(timed(plain, per))
        t_err.append(timed(with_errors, per))
    ctx.profile_begin("k_as_")
    for _ in range(per):
        with_errors()
    torch.cuda.synchronize()
    prof = ctx.profile_end()
    t, h = tot.cpu().numpy()[0], qh.cpu().numpy()[0]
    assert int(h[:, 0].sum()) == int(t[4] + t[5] + t[6]) and h[:, 1:].sum(axis=0).tolist() == t[5:8].tolist()

    def stats(v):
        return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    return {"workload": "as above, qualities uniform in 2..60", "blocks": blocks, "reps_per_block": per,
            "scratch_mib": round(need / 2**20, 1), "error_records": int(c[4]), "err_capacity": ecap,
            "assess_dev_ms": stats(t_plain), "assess_errors_dev_ms": stats(t_err),
            "kernel_ms": {k: round(v[0] / v[1], 3) for k, v in sorted(prof.items())},
            "note": "both calls timed by events around blocks of unprofiled calls, alternating; kernel_ms: a profiled run of "
                    "pv_assess_errors_dev of its own"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=5.0)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--segment", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--errors", action="store_true", help="add the pv_assess_errors_dev leg (key \"errors\")")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "assess_bench.json"))
    args = ap.parse_args()
    from pepper_thesis_amd import runtime
    ctx = runtime.Context(0)
    res = run(ctx, "cuda:0", args.mbp, args.error, args.segment, reps=args.reps)
    if args.errors:
        res["errors"] = run_errors(ctx, "cuda:0", args.mbp, args.error, args.segment, reps=args.reps)
    ctx.close()
    with open(args.output, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
