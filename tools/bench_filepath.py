"""bench.py secondary leg: the REAL-FILE path with stage timers. Primary figure: the FUSED form call_variant runs by default
(pipeline.call_variant_fused: BAM + BAI / FASTA + FAI on disk -> native readers on a thread pool -> HIP image builder -> the
windows stay in HBM -> HIP RNN -> prediction HDF5 on a writer thread). Beside it the reference's two steps through image HDF5
files: make_images (image HDF5) -> run_inference (image HDF5 -> HIP RNN -> prediction HDF5).
The BAM is synthetic (SURVEY 8(d) shape: one contig of >= 1 Mbp at 60x, 10 kb reads, planted sites) and is written here
with the library's own BAM writer (pvio_write_bam); nothing under oracle/ is used. Not part of `value`.

  python tools/bench_filepath.py [--mbp 3.2]   (32 intervals of 100 kb: two per reader thread of a 16-core share)
  python tools/bench_filepath.py --gpu_decode [--out result.json]
        host inflate, `gpu_inflate=True` and `gpu_decode=True` alternating, three runs each
  python tools/bench_filepath.py --gpu_inflate [--out result.json]
        the fused path with the host inflate (default) and with `gpu_inflate=True`, alternating, three runs each: wall and
        Mbp/s of both modes, the inflate kernel's time and output GB/s, H2D / D2H time. (bench.py calls run() only.)
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_files(dirname, contig_len, depth=60, read_len=10_000, site_every=198, seed=77, hp_seed=None):
    """synthetic contig + reads -> ref.fa(.fai), reads.bam(.bai). hp_seed: the reads carry HP tags dealt by that seed, about a
    third each untagged, HP:1 and HP:2 (info["hp_counts"])"""
    from pepper_thesis_amd import bamio, synth
    from pepper_thesis_amd.batch import pack_regions
    t0 = time.perf_counter()
    reg = synth.synth_region(seed, region_len=contig_len, depth=depth, read_len=read_len, site_every=site_every, ref_start=0,
                             contig="chr20")
    b = pack_regions([reg])
    fa = os.path.join(dirname, "ref.fa")
    width = 60
    with open(fa, "wb") as f:
        f.write(b">chr20 synthetic\n")
        off = f.tell()
        ref = np.frombuffer(reg.ref, dtype=np.uint8)
        pad = (-len(ref)) % width
        lines = np.concatenate([ref, np.zeros(pad, np.uint8)]).reshape(-1, width)
        body = np.concatenate([lines, np.full((lines.shape[0], 1), 10, np.uint8)], axis=1).reshape(-1)
        body = body[body != 0]
        f.write(body.tobytes())
        if body[-1] != 10:
            f.write(b"\n")
    with open(fa + ".fai", "w") as f:
        f.write("chr20\t%d\t%d\t%d\t%d\n" % (len(ref), off, width, width + 1))
    bam = os.path.join(dirname, "reads.bam")
    hp = None if hp_seed is None else np.random.default_rng(hp_seed).integers(0, 3, b.n_reads).astype(np.int32)
    bamio.write_bam(bam, [("chr20", contig_len)], np.zeros(b.n_reads, np.int32), b, level=1, read_hp=hp)
    more = {} if hp is None else dict(hp_counts=np.bincount(hp, minlength=3).tolist())
    return bam, fa, dict(more, reads=b.n_reads, bases=b.n_bases, synth_and_write_s=time.perf_counter() - t0,
                         bam_bytes=os.path.getsize(bam), inflate_backend=bamio.inflate_backend())


def run(ctx, weights, dev=None, mbp=3.2, keep_dir=None):
    from pepper_thesis_amd import make_images, pipeline, run_inference
    from pepper_thesis_amd.batch import PRESETS
    d = keep_dir or tempfile.mkdtemp(prefix="pv_filepath_")
    try:
        contig_len = int(mbp * 1_000_000)
        bam, fa, info = make_files(d, contig_len)
        P = PRESETS["ont_r9_guppy5_sup"]
        swept = contig_len / 1e6
        # warm the page cache and the workspaces with a small region (untimed)
        pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "warm", "p.hdf"), P, region="chr20:0-50000", min_mapq=5)
        runs = []
        for k in range(3):   # the median of three runs (a 3.2 Mbp job lasts ~0.1 s: thread wake-ups alone move it by several per cent)
            t_k = {}
            n = pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "pred_fused", "pepper_prediction.hdf"), P, min_mapq=5, timers=t_k)
            runs.append(t_k)
        walls = [r["wall_s"] for r in runs]
        t_f = sorted(runs, key=lambda r: r["wall_s"])[1]
        gpu_f = t_f["upload_s"] + t_f["device_call_s"] + t_f["readback_s"]
        out = {
            "workload": "synthetic chr20 of %.2f Mbp at 60x (10 kb reads): %d reads, %.1f M bases, BAM %.1f MB; %d intervals of 100 kb"
                        % (swept, info["reads"], info["bases"] / 1e6, info["bam_bytes"] / 1e6, t_f["intervals"]),
            "form": "fused (call_variant default): windows stay in HBM between the builder and the network, no image files",
            "windows": n, "mbp_per_s": swept / t_f["wall_s"], "windows_per_s": n / t_f["wall_s"], "wall_s": t_f["wall_s"],
            "wall_s_of_3_runs": walls,
            "reader_threads": t_f["reader_threads"], "inflate_helpers_per_reader": t_f["inflate_helpers"], "inflate_backend": info.get("inflate_backend"),
            "reader_in_bgzf_s": t_f["read_inflate_cpu_s"], "helper_inflate_cpu_s": t_f["read_helper_cpu_s"], "record_decode_clip_cpu_s": t_f["read_decode_cpu_s"],
            "MB_inflated": t_f["bytes_inflated"] / 1e6,
            "main_thread_waiting_for_readers_s": t_f["reader_stall_s"], "merge_s": t_f["merge_s"], "upload_s": t_f["upload_s"],
            "device_call_s(builder+rnn kernels)": t_f["device_call_s"], "readback_s": t_f["readback_s"],
            "hdf5_write_s(writer thread)": t_f["hdf5_write_s"], "load_weights_s": t_f["load_weights_s"],
            "host_share": 1.0 - gpu_f / t_f["wall_s"],
            "note": "host share = 1 - (uploads + kernels + read-backs) / wall; %d reader threads with %d BGZF inflate helpers each run ahead of the GPU, "
                    "the prediction file is written by its own thread" % (t_f["reader_threads"], t_f["inflate_helpers"]),
        }
        # the whole of call_variant: BAM -> prediction file -> the five VCFs (candidates selected on the pipeline's writer thread
        # while it runs; de-duplication, records and bgzip + tabix afterwards), median of three
        from pepper_thesis_amd import find_candidates as fcm
        e2e = []
        for k in range(3):
            t0 = time.perf_counter()
            coll = fcm.CandidateCollector(fa, fcm.CandidateOptions())
            t_k = {}
            pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "pred_e2e", "pepper_prediction.hdf"), P, min_mapq=5, timers=t_k, on_rows=coll)
            t1 = time.perf_counter()
            counts = fcm.process_candidates(os.path.join(d, "pred_e2e"), fa, "SAMPLE", os.path.join(d, "vcf_e2e"), fcm.CandidateOptions(), selected=coll.selected)
            t2 = time.perf_counter()
            e2e.append((t2 - t0, t1 - t0, t2 - t1, t_k.get("on_rows_s", 0.0), counts["total"]))
        e2e.sort()
        out["bam_to_vcf"] = {"wall_s": e2e[1][0], "mbp_per_s": swept / e2e[1][0], "pipeline_s": e2e[1][1], "records_and_vcf_writing_s": e2e[1][2],
                             "candidate_selection_on_writer_thread_s": e2e[1][3], "vcf_records": e2e[1][4],
                             "note": "call_variant end to end on one rank (synthetic weights: nearly every window becomes a record)"}
        # the reference's two steps through image files, for comparison
        t_img = {}
        n1 = make_images.generate_images(ctx, bam, fa, os.path.join(d, "images"), P, min_mapq=5, timers=t_img)
        t_inf = {}
        files = [os.path.join(d, "images", f) for f in sorted(os.listdir(os.path.join(d, "images"))) if f.endswith(".hdf5")]
        os.makedirs(os.path.join(d, "pred"), exist_ok=True)
        n2 = run_inference.predict_files(ctx, weights, files, os.path.join(d, "pred", "pepper_prediction.hdf"), 512, 16, timers=t_inf)
        assert n2 == n1 == n, (n, n1, n2)
        wall = t_img["wall_s"] + t_inf["wall_s"]
        out["two_step"] = {
            "mbp_per_s": swept / wall, "windows_per_s": n / wall,
            "make_images": {"wall_s": t_img["wall_s"], "mbp_per_s": swept / t_img["wall_s"],
                            "main_thread_waiting_for_readers_s": t_img["reader_stall_s"],
                            "builder_call_s(h2d+kernels+d2h)": t_img["builder_call_s"], "hdf5_write_s": t_img["hdf5_write_s"]},
            "run_inference": {"wall_s": t_inf["wall_s"], "hdf5_read_s": t_inf["hdf5_read_s"],
                              "predict_call_s(h2d+kernels+d2h)": t_inf["predict_call_s"], "hdf5_write_s": t_inf["hdf5_write_s"]},
            "host_share": 1.0 - (t_img["builder_call_s"] + t_inf["predict_call_s"]) / wall,
        }
        return out
    finally:
        if keep_dir is None:
            shutil.rmtree(d, ignore_errors=True)


def run_gpu_inflate(ctx, weights, mbp=3.2, runs=3):
    """host vs GPU BGZF inflate on the fused call_variant path: alternating runs, `runs` of each"""
    from pepper_thesis_amd import pipeline
    from pepper_thesis_amd.batch import PRESETS
    d = tempfile.mkdtemp(prefix="pv_filepath_gi_")
    try:
        contig_len = int(mbp * 1_000_000)
        bam, fa, info = make_files(d, contig_len)
        P = PRESETS["ont_r9_guppy5_sup"]
        swept = contig_len / 1e6
        for gi in (False, True):   # warm the page cache, the workspaces and the pinned host pool (untimed)
            pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "warm", "p.hdf"), P, min_mapq=5, gpu_inflate=gi)
        res = {False: [], True: []}
        for k in range(runs):
            for gi in (False, True):
                t_k = {}
                n = pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "pred_%d" % gi, "pepper_prediction.hdf"), P,
                                                min_mapq=5, timers=t_k, gpu_inflate=gi)
                t_k["windows"] = n
                res[gi].append(t_k)

        def leg(rs, gi):
            walls = [r["wall_s"] for r in rs]
            med = sorted(rs, key=lambda r: r["wall_s"])[len(rs) // 2]
            o = {"wall_s_median": med["wall_s"], "wall_s_runs": walls, "mbp_per_s_median": swept / med["wall_s"],
                 "mbp_per_s_runs": [swept / w for w in walls], "windows": med["windows"],
                 "reader_threads": med["reader_threads"], "reader_in_bgzf_cpu_s": med["read_inflate_cpu_s"],
                 "record_decode_clip_cpu_s": med["read_decode_cpu_s"], "main_thread_waiting_for_readers_s": med["reader_stall_s"],
                 "device_call_s(builder+rnn)": med["device_call_s"], "upload_s": med["upload_s"], "readback_s": med["readback_s"]}
            if gi:
                kms = [r["gpu_inflate_kernel_ms"] for r in rs]
                o.update({
                    "inflate_kernel_ms_runs": kms, "inflate_kernel_ms_median": med["gpu_inflate_kernel_ms"],
                    "inflate_output_GB": med["gpu_inflate_bytes"] / 1e9,
                    "inflate_output_GB_per_s": med["gpu_inflate_bytes"] / 1e6 / max(med["gpu_inflate_kernel_ms"], 1e-9),
                    "inflate_launches": med["gpu_inflate_launches"], "blocks_gpu": med["gpu_inflate_blocks"],
                    "blocks_inflated_on_host": med["gpu_inflate_blocks_host"],
                    "h2d_ms": med["gpu_inflate_h2d_ms"], "d2h_ms": med["gpu_inflate_d2h_ms"],
                    "plan_cpu_s": med["gpu_inflate_plan_cpu_s"],
                    "note": "kernel / H2D / D2H ms are summed over the launches (HIP events on the inflate stream); the copies "
                            "and kernels of concurrent launches are not serialized against the builder's stream"})
            return o
        return {"workload": "synthetic chr20 of %.2f Mbp at 60x (10 kb reads): %d reads, BAM %.1f MB"
                            % (swept, info["reads"], info["bam_bytes"] / 1e6),
                "form": "fused call_variant path, host inflate (default) vs gpu_inflate=True, alternating runs",
                "host_inflate": leg(res[False], False), "gpu_inflate": leg(res[True], True),
                "host_over_gpu_wall_median": sorted(r["wall_s"] for r in res[False])[runs // 2] /
                sorted(r["wall_s"] for r in res[True])[runs // 2]}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run_gpu_decode(ctx, weights, mbp=3.2, runs=3):
    """host inflate (default) vs gpu_inflate vs gpu_decode on the fused call_variant path: alternating runs, `runs` of each"""
    from pepper_thesis_amd import pipeline
    from pepper_thesis_amd.batch import PRESETS
    d = tempfile.mkdtemp(prefix="pv_filepath_gd_")
    modes = {"host_inflate": {}, "gpu_inflate": {"gpu_inflate": True}, "gpu_decode": {"gpu_decode": True}}
    try:
        contig_len = int(mbp * 1_000_000)
        bam, fa, info = make_files(d, contig_len)
        P = PRESETS["ont_r9_guppy5_sup"]
        swept = contig_len / 1e6
        for kw in modes.values():   # warm the page cache, the workspaces and the pinned host pool (untimed)
            pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "warm", "p.hdf"), P, min_mapq=5, **kw)
        res = {m: [] for m in modes}
        for k in range(runs):
            for m, kw in modes.items():
                t_k = {}
                t_k["windows"] = pipeline.call_variant_fused(ctx, weights, bam, fa, os.path.join(d, "pred_" + m, "pepper_prediction.hdf"),
                                                             P, min_mapq=5, timers=t_k, **kw)
                res[m].append(t_k)

        def leg(rs):
            walls = [r["wall_s"] for r in rs]
            med = sorted(rs, key=lambda r: r["wall_s"])[len(rs) // 2]
            o = {"wall_s_median": med["wall_s"], "wall_s_runs": walls, "wall_s_spread": max(walls) - min(walls),
                 "mbp_per_s_median": swept / med["wall_s"], "windows": med["windows"]}
            for k in ("reader_threads", "read_inflate_cpu_s", "read_decode_cpu_s", "reader_stall_s", "device_call_s", "upload_s",
                      "readback_s", "gpu_inflate_kernel_ms", "gpu_inflate_bytes", "gpu_inflate_launches", "gpu_inflate_h2d_ms",
                      "gpu_inflate_d2h_ms", "gpu_inflate_plan_cpu_s", "gpu_inflate_blocks_host", "gpu_decode_plan_cpu_s", "gpu_decode_plan_wall_s",
                      "gpu_decode_scan_ms", "gpu_decode_fill_ms", "gpu_decode_host_s", "gpu_decode_h2d_bytes", "gpu_decode_d2h_bytes",
                      "gpu_decode_groups", "gpu_decode_groups_host", "gpu_decode_records", "reads", "bases"):
                if k in med:
                    o[k] = med[k]
            if "gpu_decode_scan_ms" in med:
                gb = med["gpu_inflate_bytes"] / 1e9
                o["scan_GB_per_s_over_inflated_bytes"] = gb / max(med["gpu_decode_scan_ms"] / 1e3, 1e-12)
                o["fill_GB_per_s_over_inflated_bytes"] = gb / max(med["gpu_decode_fill_ms"] / 1e3, 1e-12)
            return o
        return {"workload": "synthetic chr20 of %.2f Mbp at 60x (10 kb reads): %d reads, BAM %.1f MB"
                            % (swept, info["reads"], info["bam_bytes"] / 1e6),
                "form": "fused call_variant path; host inflate (default), gpu_inflate=True, gpu_decode=True; alternating runs; the "
                        "ms figures are HIP-event sums over the launches of the service stream",
                **{m: leg(res[m]) for m in modes}}
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=float, default=3.2)
    ap.add_argument("--gpu_inflate", action="store_true", help="the host-vs-GPU BGZF inflate comparison instead of the default leg")
    ap.add_argument("--gpu_decode", action="store_true", help="host inflate vs --gpu_inflate vs --gpu_decode, three runs each")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON result here")
    a = ap.parse_args()
    from pepper_thesis_amd import runtime, synth
    c = runtime.Context(0)
    if a.gpu_decode:
        r = run_gpu_decode(c, synth.make_weights_p1(1234), mbp=a.mbp)
    elif a.gpu_inflate:
        r = run_gpu_inflate(c, synth.make_weights_p1(1234), mbp=a.mbp)
    else:
        r = run(c, synth.make_weights_p1(1234), mbp=a.mbp)
    txt = json.dumps(r, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")
