#!/usr/bin/env python3
"""`pepper kmer_qv` on the synthetic contig of tools/bench_polish_e2e.py (tools/bench_filepath.make_files: 60x, 10 kb reads),
scoring the draft itself.

  build    pv_kmer_table_build_dev, wall time to the stream's end, the median of --reps
  count    k_km_count under HIP events: every batch of the run is uploaded once and counted `n` times, n chosen so that the
           timed kernels take at least a second together; read Mbases/s, and the read bytes per second against the HBM peak
           (one byte per base: the table look-ups, which stay in L2, are not counted)
  summary  pv_kmer_support_dev under HIP events, the median of --reps
  e2e      kmer_qv.stream_reads (reader threads, upload, count) plus the summary: wall time and the reader's share
  host     the same rule on the host: NumPy keys, one sort of the assembly's, searchsorted per batch, --threads threads; its
           per-position counts are compared with the device's

  complete with --completeness, after the legs above (which run as they did): k_km_count_all with one part under HIP events, the
           first pass over the reads (every key the assembly lacks claims its slot) and `n` further ones (every key finds it),
           beside k_km_count of the same session; the flush and the spectrum; the distinct reads-only keys and the load factor;
           the end-to-end wall with the flag

  python tools/bench_kmer_qv.py [--mbp 3.0] [--threads 16] [--reps 5] [-k 21] [--out profiles/kmer_qv_bench.json]
  python tools/bench_kmer_qv.py --completeness [--read_table_mb 4096] --out profiles/kmer_qv_complete_bench.json
"""
import argparse
import concurrent.futures
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GB_S = 8000.0   # MI355X


def host_keys(codes: np.ndarray, k: int):
    """codes uint8 (0..3, 4 = no base) -> (canonical keys uint64 of every window start, valid mask) for len - k + 1 starts"""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    c = (codes & 3).astype(np.uint64)
    fwd, rev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        w = c[j:j + n]
        fwd |= w << np.uint64(2 * (k - 1 - j))
        rev |= (np.uint64(3) - w) << np.uint64(2 * j)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    return np.minimum(fwd, rev), (bad[k:k + n] - bad[:n]) == 0


_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i


def host_count(asm: bytes, batches, k: int, threads: int):
    """-> (per-position counts uint32 with NO_KEY, seconds): the rule with one sorted array of the assembly's distinct keys"""
    t0 = time.perf_counter()
    keys, ok = host_keys(_LUT[np.frombuffer(asm, np.uint8)], k)
    uniq, inverse = np.unique(keys[ok], return_inverse=True)

    def one(b):
        bases, off = b
        rk, rok = host_keys(_LUT[bases], k)
        n = len(rk)
        # a window must end inside the read it starts in
        owner = np.searchsorted(off, np.arange(n), side="right") - 1
        rok &= np.arange(n) + k <= off[owner + 1]
        rk = rk[rok]
        at = np.searchsorted(uniq, rk)
        at[at == len(uniq)] = 0
        hit = uniq[at] == rk
        return np.bincount(at[hit], minlength=len(uniq))
    total = np.zeros(len(uniq), np.int64)
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as ex:
        for part in ex.map(one, batches):
            total += part
    plane = np.full(len(asm), 0xFFFFFFFF, np.uint32)
    plane[np.flatnonzero(ok)] = np.minimum(total[inverse], 1 << 30).astype(np.uint32)
    return plane, time.perf_counter() - t0


def complete_legs(ctx, kq, args, asm, k, bam, fa, ivs, reps, res):
    """the legs of --completeness on the workload of the legs above; `reps`: the passes the count leg timed"""
    from pepper_thesis_amd import bamio
    slots = kq.read_slots(args.read_table_mb)
    out = {"read_table_mb": args.read_table_mb, "slots": slots}
    sc = kq.Scorer(ctx, "assembly", asm, k, 1024, slots)
    ctx.synchronize()
    hb, hf = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    filled = [bamio.fill_batch(hb, hf, [iv], 0, False, 1.0, 0, max_reads=kq.READ_LIMIT) for iv in ivs]
    n_bases = sum(int(len(f.batch.bases)) for f in filled)
    # the first pass claims the slots, the further ones find them: both under HIP events, each batch uploaded once per pass kind
    first = again = launches = 0.0
    for f in filled:
        dev, totals, keep = ctx.upload_batch(f.batch)
        ctx.profile_begin("k_km_count_all")
        sc.count_all(dev.bases, dev.base_off, totals[0], totals[1], 0, 1)
        ctx.synchronize()
        first += ctx.profile_end()["k_km_count_all"][0]
        ctx.profile_begin("k_km_count_all")
        for _ in range(reps):
            sc.count_all(dev.bases, dev.base_off, totals[0], totals[1], 0, 1)
        ctx.synchronize()
        ms, n = ctx.profile_end()["k_km_count_all"]
        again, launches = again + ms, launches + n
    for f in filled:
        f.close()
    count_ms = res["count"]["kernel_ms"] / res["count"]["passes"]
    out["count_all"] = {"first_pass_ms": round(first, 3), "further_passes": reps, "further_kernel_ms": round(again, 3),
                        "further_pass_ms": round(again / reps, 3), "launches": int(launches) + len(filled),
                        "read_mbases_per_s_first": round(n_bases / (first * 1e-3) / 1e6, 1),
                        "k_km_count_pass_ms": round(count_ms, 3), "first_over_k_km_count": round(first / count_ms, 2),
                        "further_over_k_km_count": round(again / reps / count_ms, 2)}
    ctx.profile_begin("kmer_reads_flush")
    sc.flush()
    out["flush_ms"] = round(ctx.profile_end()["kmer_reads_flush"][0], 3)
    out["reads_only_keys"], out["load_factor"] = sc.ro_keys, round(sc.ro_keys / slots, 4)
    ctx.profile_begin("kmer_spectrum")
    for _ in range(args.reps):
        sc.spectrum()
    ms, n = ctx.profile_end()["kmer_spectrum"]
    out["spectrum_ms"] = round(ms / n, 3)
    ctx.profile_begin("k_kr_init")
    ctx.kmer_reads_table_init_dev(sc.rtable.data_ptr(), sc.rtable_bytes, slots, kq.CAP)
    ctx.synchronize()
    out["init_ms"] = round(ctx.profile_end()["k_kr_init"][0], 3)
    # end to end with the flag: a fresh scorer, one pass, the flush, the summary, the spectrum and the two texts
    T = {}
    t0 = time.perf_counter()
    sc = kq.Scorer(ctx, "assembly", asm, k, 1024, slots)
    kq.stream_reads(ctx, bam, fa, ivs, [sc], args.threads, T, part=(0, 1))
    sc.flush()
    sc.texts(1)
    _, share = sc.completeness_texts(2)
    wall = time.perf_counter() - t0
    out["e2e"] = {"wall_s": round(wall, 3), "reader_wait_s": round(T["read_s"], 3), "device_s": round(T["device_s"], 3),
                  "wall_without_flag_s": res["e2e"]["wall_s"], "ratio": round(wall / res["e2e"]["wall_s"], 2),
                  "completeness_at_2": share, "reads_only_keys": sc.ro_keys}
    return out


def say(msg):
    print("[bench_kmer_qv] " + msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=3.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("-k", "--kmer", type=int, default=21)
    ap.add_argument("--interval", type=int, default=500000)
    ap.add_argument("--completeness", action="store_true", default=False, help="add the legs of kmer_qv --completeness")
    ap.add_argument("--read_table_mb", type=float, default=4096.0,
                    help="with --completeness: the reads-only table, as the command's (its default of 1024 is too small for the "
                         "default workload's read k-mers in one pass)")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    args = ap.parse_args()
    import torch
    from bench_filepath import make_files
    from pepper_thesis_amd import bamio, runtime
    from pepper_thesis_amd import kmer_qv as kq
    k = args.kmer
    d = tempfile.mkdtemp(prefix="pv_kmer_qv_")
    try:
        bam, fa, info = make_files(d, int(args.mbp * 1_000_000))
        say("files written in %.1f s" % info["synth_and_write_s"])
        asm = kq.read_fasta(fa)
        ivs = kq.read_intervals([(n, len(s)) for n, s in asm], args.interval)
        ctx = runtime.Context(0)
        try:
            res = {"mbp": args.mbp, "k": k, "threads": args.threads, "interval": args.interval, "reads": info["reads"],
                   "read_bases": info["bases"]}
            sc = kq.Scorer(ctx, "assembly", asm, k, 1024)
            ctx.synchronize()
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ctx.kmer_table_build_dev(sc.A.data_ptr(), sc.ao.data_ptr(), sc.n, k, kq.CAP, sc.table.data_ptr(), sc.table_bytes,
                                         sc.bcnt.data_ptr())
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            res["build_ms"] = round(float(np.median(times)), 3)
            res["table_bytes"], res["keyed_entries"] = sc.table_bytes, int(sc.bcnt.cpu().numpy()[0])
            # the batches, read once and kept on the host
            hb, hf = bamio.BamHandler(bam), bamio.FastaHandler(fa)
            t0 = time.perf_counter()
            filled = [bamio.fill_batch(hb, hf, [iv], 0, False, 1.0, 0, max_reads=kq.READ_LIMIT) for iv in ivs]
            res["one_thread_read_s"] = round(time.perf_counter() - t0, 3)
            batches = [(np.array(f.batch.bases), np.array(f.batch.base_off)) for f in filled]
            n_bases = sum(len(b) for b, _ in batches)
            say("build %.3f ms; %d batches read" % (res["build_ms"], len(filled)))
            # the count kernel alone
            reps, per_pass = 1, None
            for attempt in (0, 1):
                ctx.profile_begin("k_km_count")
                for f in filled:
                    dev, totals, keep = ctx.upload_batch(f.batch)
                    for _ in range(reps):
                        sc.count(dev.bases, dev.base_off, totals[0], totals[1])
                    ctx.synchronize()
                ms, launches = ctx.profile_end()["k_km_count"]
                if attempt == 0:
                    per_pass = ms
                    reps = int(1000.0 / max(ms, 1e-3)) + 2
            res["count"] = {"passes": reps, "launches": launches, "kernel_ms": round(ms, 3), "first_pass_ms": round(per_pass, 3),
                            "read_mbases_per_s": round(n_bases * reps / (ms * 1e-3) / 1e6, 1),
                            "read_gb_per_s": round(n_bases * reps / (ms * 1e-3) / 1e9, 2), "hbm_peak_gb_per_s": HBM_PEAK_GB_S}
            res["count"]["share_of_hbm_peak"] = round(res["count"]["read_gb_per_s"] / HBM_PEAK_GB_S, 4)
            for f in filled:
                f.close()
            say("count: %s" % json.dumps(res["count"]))
            # the summary
            ctx.profile_begin("kmer_support")
            for _ in range(args.reps):
                sc.summary(1)
            ms, launches = ctx.profile_end()["kmer_support"]
            res["summary_ms"] = round(ms / launches, 3)
            # end to end: a fresh table, the reader threads, the upload, the count, the summary
            T = {}
            t0 = time.perf_counter()
            sc = kq.Scorer(ctx, "assembly", asm, k, 1024)
            kq.stream_reads(ctx, bam, fa, ivs, [sc], args.threads, T)
            _, (unsup, kmers, qv) = sc.texts(1)
            wall = time.perf_counter() - t0
            res["e2e"] = {"wall_s": round(wall, 3), "reader_wait_s": round(T["read_s"], 3), "device_s": round(T["device_s"], 3),
                          "reader_share": round(T["read_s"] / wall, 3), "read_mbases_per_s": round(T["read_bases"] / wall / 1e6, 1),
                          "unsupported": unsup, "kmers": kmers, "qv": qv}
            say("e2e: %s" % json.dumps(res["e2e"]))
            # the per-position counts of that run, for the comparison with the host's
            plane = torch.zeros(sc.N + 1, dtype=torch.int32, device="cuda")
            outs = [torch.zeros(n, dtype=torch.int64, device="cuda") for n in (3 * sc.n, sc.n + 1, sc.N // 1024 + sc.n + 1, 3, 256, 8)]
            torch.cuda.synchronize()
            ctx.kmer_support_dev(sc.table.data_ptr(), sc.table_bytes, sc.ao.data_ptr(), sc.n, 1, 1024, outs[0].data_ptr(),
                                 outs[1].data_ptr(), len(outs[2]), outs[2].data_ptr(), 0, 0, outs[4].data_ptr(), plane.data_ptr(),
                                 outs[5].data_ptr())
            ctx.synchronize()
            dev_plane = plane.cpu().numpy().view(np.uint32)[:sc.N]
            if args.completeness:
                res["complete"] = complete_legs(ctx, kq, args, asm, k, bam, fa, ivs, reps, res)
                say("complete: %s" % json.dumps(res["complete"]))
        finally:
            ctx.close()
        host_plane, host_s = host_count(b"".join(kq.upper(s) for _, s in asm), batches, k, args.threads)
        res["host"] = {"count_s": round(host_s, 3), "read_mbases_per_s": round(n_bases / host_s / 1e6, 1),
                       "equals_device": bool(np.array_equal(host_plane, dev_plane))}
        dev_s = res["build_ms"] * 1e-3 + res["count"]["kernel_ms"] * 1e-3 / reps
        res["host_over_device_kernels"] = round(host_s / dev_s, 1)
        res["host_over_e2e"] = round(host_s / res["e2e"]["wall_s"], 2)
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
