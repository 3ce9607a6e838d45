#!/usr/bin/env python3
"""The polisher end to end, and its stitch step on its own.

  stitch leg: the 2121-chunk batch of tools/bench_polish.py (8 synthetic regions of 100 k columns) through the builder and the
              bi-GRU once; then pv_polish_stitch_dev alone, timed with HIP events (per kernel and the whole call), against the
              reference-style host stitch (tests/stitch_ref.py: dict + string-sorted chunk ids + global sort) on the same labels,
              and the bytes each way has to move off the device.
  e2e leg:    a synthetic contig (tools/bench_filepath.make_files: 60x, 10 kb reads) written as BAM + FASTA, then
              polish.polish_fused (readers -> builder -> bi-GRU -> stitch -> FASTA): wall time and draft Mbp/s.

  --realign: the e2e leg runs twice in one process on the same files, without and with `polish --realign`, then the
              realigner alone on every region of the workload (launches of the chain's size), its kernels timed with HIP
              events: forward + reverse DP cells, banded cells (score-only passes + the direction pass) and GCUPS.

  --d_ids a,b,...: the e2e leg runs the `polish` command instead, in fresh processes: once with `-d_ids a,b,...` (one rank per
              id) and once on device a alone with PV_SHARED_DEVICE=1 (the kernel forms the ranks use when they share a device);
              wall times of both and whether the two FASTA files are byte-identical. Ranks that share one card split its CPUs
              and its device: such a wall time is a correctness rehearsal, not a scaling figure.

  steps leg:  the same synthetic contig through `python -m pepper_thesis_amd.pepper make_images -> call_consensus -> stitch`
              and through `pepper polish`, each command a fresh process with PV_SHARED_DEVICE=1 (start-up, context creation
              and model load included): wall time of every command, the sizes of the image and prediction files, and whether
              the two FASTA files are byte-identical. Written to profiles/polish_steps_bench.json with --out.

  --gpu_decode: the e2e leg reads the BAM through `polish --gpu_decode` (inflate, record decode and clipping on the device).

  --qualities: the e2e leg runs in one process on the same files, without and with `polish --qualities` (the FASTQ beside
              the FASTA) in turn, twice each, then once more each way with the stitch and the row-quality calls bracketed by HIP events: what
              the flag adds on the device (pv_polish_row_qual_dev, the quality plane of the stitch) and on the wall.

  --edits:    the same comparison for `polish --edits` (the edits VCF beside the FASTA): wall times of both forms, twice each,
              then the stitch and the edit calls bracketed by HIP events, the records and the bytes that come back from the
              device, and the VCF's size. The weights are random, so most rows are edits: the record count says nothing
              about a trained model.

  --edits --evidence: `polish --edits` without and with --evidence: wall times of both forms, twice each, then HIP events around
              the builder call without a plane, with the depth plane and with both, and around the edits / evidence call.
  --min_depth N: the same comparison for `polish --min_depth N`: wall times of both forms, twice each, then one more run each way
              with the builder, the mask and the stitch calls bracketed by HIP events, and the rows the mask rewrote. The parent
              commit's plain figure (profiles/polish_e2e_bench.json) is recorded beside them as the yardstick.

  --min_qual Q: the same comparison for `polish --min_qual Q`: wall times of both forms, twice each, then one more run each way
              (with --edits, so that the edit call stands beside it) with the row-quality, filter, stitch and edit calls bracketed
              by HIP events, and the rows the filter took back. The weights are random: nearly every column is an edit and
              whole regions are single runs, so the reverted fraction and the host time say nothing about a trained model.

  -hp:        the same comparison for `polish -hp` on a BAM whose reads carry HP tags (about a third each untagged, 1 and 2, a
              fixed seed): wall times of the plain form and the -hp form on that file, twice each, then one more -hp run with
              --realign with the selection, the realigner and the builder calls bracketed by HIP events, and the selection's
              achieved bytes per second (payload read + payload written over its time).

  --vote:     `polish` with the seeded model against `polish --vote` without one: wall times of both forms, twice each, then one
              more --vote run with --qualities whose vote kernels are bracketed by HIP events, the chunks they saw, and the
              bytes per second the two kernels move by the per-row byte count kept in vote_leg.

  --runs N:   `polish --vote` against `polish --vote --runs --min_run N`: wall times of both forms, twice each, then two more
              --runs runs under HIP events: the whole calls (image builder, column vote, run vote), and the run vote's kernels.

  python tools/bench_polish_e2e.py [--leg stitch|e2e|steps|all] [--mbp 2.0] [--reps 20] [--realign] [--d_ids 0,0] [--gpu_decode]
                                   [--qualities] [--edits [--evidence]] [--min_depth N] [--min_qual Q] [--min_support K] [-hp] [--vote] [--runs N] [--out f]
For the rocprofv3 row run the stitch leg alone under `rocprofv3 --kernel-trace --stats -d <dir> -- python ... --leg stitch`.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stitch_leg(reps=20):
    import numpy as np
    import torch
    import stitch_ref as sr
    from pepper_thesis_amd import runtime, synth
    from pepper_thesis_amd.batch import pack_regions
    from pepper_thesis_amd.device import DeviceBatch, DevicePolishOut
    dev = "cuda:0"
    regs = [synth.synth_region(1234 + 97 * i, site_every=260, ref_start=1_000_000 + i * 100_000) for i in range(8)]
    b = pack_regions(regs)
    ctx = runtime.Context(0)
    ctx.load_p2(synth.make_weights_p2(4321, 3.0))
    db = DeviceBatch(b, dev)
    do = DevicePolishOut(2400, device=dev)
    labels = torch.zeros((2400, 1000), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.polish_summarize_dev(db, do)
    ctx.synchronize()
    n = do.n_chunks()
    assert do.status() == 0 and n <= do.capacity, (do.status(), n)
    ctx.forward_p2_dev(do.images.data_ptr(), n, labels.data_ptr())
    seq = torch.zeros(n * 1000, dtype=torch.uint8, device=dev)
    roff = torch.zeros(b.n_regions + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.synchronize()

    def stitch():
        ctx.polish_stitch_dev(do, n, labels.data_ptr(), db.t["ref_start"].data_ptr(), b.n_regions, roff.data_ptr(),
                              seq.data_ptr(), seq.numel(), counts.data_ptr())

    for _ in range(3):
        stitch()
    ctx.synchronize()
    ctx.profile_begin()
    for _ in range(reps):
        stitch()
    pr = ctx.profile_end()
    ms = {k: v[0] / reps for k, v in pr.items() if "stitch" in k}
    total, status = (int(v) for v in counts[:2].tolist())
    assert status == 0, status
    # device form + the only read-back it needs (offsets + bases), timed on the host clock
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        stitch()
        ctx.synchronize()
        got = seq[:int(counts[0].item())].cpu().numpy().tobytes()
        roff.cpu()
    dev_call_ms = (time.perf_counter() - t0) / reps * 1e3
    # the reference's way: labels, positions and indices back to the host, then the per-base Python stitch
    t0 = time.perf_counter()
    h = dict(position=do.position[:n].cpu().numpy(), index=do.index[:n].cpu().numpy(), region=do.region[:n].cpu().numpy(),
             chunk_id=do.chunk_id[:n].cpu().numpy(), labels=labels[:n].cpu().numpy())
    t_copy = time.perf_counter() - t0
    spans = list(zip(b.ref_start.tolist(), b.ref_end.tolist()))
    t0 = time.perf_counter()
    rc = sr.regions_from_chunks(h["position"], h["index"], h["region"], h["chunk_id"], h["labels"], spans)
    host = b"".join(sr.create_consensus_sequence([r]).encode() for r in rc)
    t_host = time.perf_counter() - t0
    assert host == got, "device stitch differs from the host checker"
    ctx.close()
    cols = n * 1000
    return {"chunks": n, "columns": cols, "bases_out": total, "reps": reps,
            "event_ms": {k: round(v, 4) for k, v in ms.items()},
            "device_call_plus_readback_ms": round(dev_call_ms, 3),
            "device_bytes_read_per_column": 2 * (8 + 4 + 1), "readback_bytes": total + 8 * (b.n_regions + 1),
            "host_reference_style": {"readback_ms": round(t_copy * 1e3, 2), "readback_bytes": cols * 13 + n * 8,
                                     "stitch_ms": round(t_host * 1e3, 1)}}


def _e2e_run(polish, ctx, bam, fa, model, out, threads, realign, info, gpu_decode=False, **options):
    """options: the polish.ChainOptions of the run"""
    o = polish.ChainOptions(**options)
    kw = dict(o.keywords(), gpu_decode=True) if gpu_decode else o.keywords()
    # warm-up on a small region (code objects, allocator), then the timed run
    polish.polish_fused(bam, fa, model, out + "_warm", region="chr20:0-50000", threads=threads, ctx=ctx, realign=realign, **kw)
    T = {}
    t0 = time.perf_counter()
    path = polish.polish_fused(bam, fa, model, out, threads=threads, ctx=ctx, timers=T, realign=realign, **kw)
    wall = time.perf_counter() - t0
    size = os.path.getsize(path)
    res = {"draft_bp": T["bases_in"], "reads": info["reads"], "regions": T["regions"], "batches": T["batches"],
           "polished_bp": T["bases_out"], "fasta_bytes": size, "wall_s": round(wall, 3),
           "read_s": round(T["read_s"], 3), "device_s": round(T["device_s"], 3),
           "draft_mbp_per_s": round(T["bases_in"] / wall / 1e6, 4), "reader_threads": threads}
    if o.use_hp:
        res.update(use_hp=True, fasta_bytes_hp2=os.path.getsize(polish.hp_path(path[:-len("_hp1.fa")] + ".fa", 2)),
                   tags={k: T[k] for k in polish.HP_TIMERS})
    for p in polish.PASSES:   # the option's value (the run vote's as min_run) and the pass's counts
        if getattr(o, p.option):
            res[{"vote_runs": "min_run"}.get(p.option, p.option)] = getattr(o, p.option)
            res.update({k: T[k] for k in p.timers + (("draft_regions",) if p.option == "min_depth" else ())})
    if o.qualities:
        fq = polish.output_fastq_path(path)
        res["qualities"], res["fastq_bytes"] = True, os.path.getsize(fq)
    if o.edits:
        from pepper_thesis_amd import polish_edits
        vcf = polish_edits.output_vcf_path(path)
        res.update(edits=True, edit_records=T["edit_records"], vcf_records=T["vcf_records"], vcf_bytes=os.path.getsize(vcf),
                   tbi_bytes=os.path.getsize(vcf + ".tbi"),
                   # 16 bytes a record and the region offsets of every launch
                   edits_readback_bytes=16 * T["edit_records"] + 8 * (T["regions"] + T["batches"]))
    if o.evidence:
        res.update(evidence=True, evidence_readback_bytes=8 * T["edit_records"], one_strand_records=T.get("one_strand_records", 0))
    if gpu_decode:
        import hashlib
        import torch
        res["gpu_decode"] = True
        res["torch_max_memory_allocated_bytes"] = int(torch.cuda.max_memory_allocated())   # decode and chain tensors, warm-up included
        res["fasta_sha256"] = hashlib.sha256(open(path, "rb").read()).hexdigest()
        res["timers"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in sorted(T.items())
                         if k in ("plan_s", "decode_s", "chain_runs") or k.startswith("gpu_")}
    return res


def realign_stats(ctx, bam, fa, per_launch=1024):
    """the realigner alone on every region of the workload: kernel time (HIP events) and cells"""
    import numpy as np
    from pepper_thesis_amd import bamio, polish, realign
    from pepper_thesis_amd.batch import pack_regions
    from pepper_thesis_amd.polish_summary import region_from_files
    b, f = bamio.BamHandler(bam), bamio.FastaHandler(fa)
    regs = []
    for c in f.get_chromosome_names():
        for s, e in polish.polish_intervals(f.get_chromosome_sequence_length(c)):
            r = region_from_files(b, f, c, s, e, realign=True)
            if r is not None:
                regs.append(r)
    ms, launches = {}, 0
    fwd = rev = band = 0
    n_reads = n_re = 0
    for i in range(0, len(regs), per_launch):
        part = regs[i:i + per_launch]
        batch = pack_regions(part)
        woff, win = realign.pack_windows([r.window for r in part])
        ctx.profile_begin("k_rl")
        res = ctx.polish_realign(batch, woff, win)
        for k, (t, n) in ctx.profile_end().items():
            ms[k] = ms.get(k, 0.0) + t
        launches += 1
        g = np.searchsorted(batch.read_off, np.arange(batch.n_reads), "right") - 1
        off = batch.read_pos - batch.ref_start[g]
        qlen = np.diff(batch.base_off)
        wlen = woff[g + 1] - woff[g]
        ok = (off >= 0) & (off < wlen) & (qlen > 0)
        fwd += int((qlen[ok] * (wlen[ok] - off[ok])).sum())
        m = res.state == 1
        rb, re_, qb, qe = (res.ends[m, k].astype(np.int64) for k in range(4))
        rev += int(((qe + 1) * (re_ + 1)).sum())   # the reverse sweep stops early: an upper bound
        rs, qs, w = re_ - rb + 1, qe - qb + 1, res.band[m].astype(np.int64)
        w0 = np.abs(rs - qs) + 1
        while True:   # score-only passes w0, 2 w0, ..., w, then the direction pass at w
            live = w0 <= w
            if not live.any():
                break
            band += int((qs[live] * np.minimum(2 * w0[live] + 1, rs[live])).sum())
            w0 = w0 * 2
        band += int((qs * np.minimum(2 * w + 1, rs)).sum())
        n_reads += batch.n_reads
        n_re += res.n_realigned
    score_ms = ms.get("k_rl_score_fwd", 0.0) + ms.get("k_rl_score_rev", 0.0)
    band_ms = sum(v for k, v in ms.items() if k.startswith("k_rl_band"))
    return {"regions": len(regs), "reads": n_reads, "realigned": n_re, "launches": launches,
            "kernel_ms": {k: round(v, 3) for k, v in sorted(ms.items())},
            "score_cells": {"forward": fwd, "reverse_upper_bound": rev},
            "band_cells_upper_bound": band,
            "score_gcups": round((fwd + rev) / (score_ms * 1e-3) / 1e9, 1) if score_ms else None,
            "band_gcups": round(band / (band_ms * 1e-3) / 1e9, 1) if band_ms else None}


def _quality_events(polish, ctx, bam, fa, model, out, threads, qualities, edits=False, min_depth=0, min_qual=0, evidence=False,
                    min_support=0):
    """one more run with the calls whose profile names start with polish_ bracketed by HIP events -> {name: [ms, launches]}"""
    ctx.profile_begin("polish_")
    try:
        kw = {"min_qual": min_qual} if min_qual else {}
        if evidence:
            kw["evidence"] = True
        if min_support:
            kw["min_support"] = min_support
        polish.polish_fused(bam, fa, model, out, threads=threads, ctx=ctx, qualities=qualities, edits=edits, min_depth=min_depth, **kw)
    finally:
        pr = ctx.profile_end()
    return {k: [round(v[0], 4), v[1]] for k, v in sorted(pr.items())
            if k in ("polish_stitch", "polish_row_qual", "polish_edits", "polish_edits_evidence", "polish_mask", "polish_filter",
                     "polish_filter_support", "polish_pipeline")}


def min_depth_leg(mbp=3.0, threads=16, min_depth=3):
    """polish without and with --min_depth on one synthetic contig, in one process on the same files"""
    import hashlib
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_min_depth_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for m in (0, min_depth):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "masked" if m else "plain"), threads, False, info,
                                 min_depth=m)
                    runs.append(dict(r, min_depth=m, order=len(runs)))
            res = {"runs": runs, "without_min_depth": runs[2], "with_min_depth": runs[3]}
            sha = [hashlib.sha256(open(os.path.join(d, n, "_pepper_polished.fa"), "rb").read()).hexdigest() for n in ("plain", "masked")]
            res["fasta_identical"] = sha[0] == sha[1]
            res["event_ms_launches"] = {
                "without_min_depth": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "plain_ev"), threads, False),
                "with_min_depth": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "masked_ev"), threads, False,
                                                  min_depth=min_depth),
                # the mask's worst case: a threshold no depth reaches, so every row loads its position, index and draft byte
                "with_min_depth_65535": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "all_ev"), threads, False,
                                                        min_depth=65535)}
            try:
                with open(os.path.join(ROOT, "profiles", "polish_e2e_bench.json")) as fh:
                    res["parent_plain_wall_s"] = json.load(fh)["e2e"]["wall_s"]
            except (OSError, KeyError, ValueError):
                res["parent_plain_wall_s"] = None
            res["note"] = ("polish_pipeline: the image builder call (every kernel of it; with the flag it also writes the depth plane); "
                           "polish_mask: count + finish + write kernels of one mask call; polish_stitch: count + scan + write; HIP "
                           "events around every call of a run, summed over the run's launches. The weights are random, so the FASTA "
                           "of the plain run is not the draft and the two FASTA files differ wherever a row was masked")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def min_support_leg(mbp=3.0, threads=16, min_support=1):
    """polish without and with --min_support on one synthetic contig, in one process on the same files; the quality filter
    (--min_qual 20) is timed in the same process for comparison"""
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_min_support_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for m in (0, min_support):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "supported" if m else "plain"), threads, False, info,
                                 min_support=m)
                    runs.append(dict(r, min_support=m, order=len(runs)))
            res = {"runs": runs, "without_min_support": runs[2], "with_min_support": runs[3]}
            ev = lambda name, **kw: _quality_events(polish, ctx, bam, fa, model, os.path.join(d, name), threads, False, True, **kw)
            res["event_ms_launches"] = {
                "without": ev("plain_ev"),
                "with_min_support": ev("sup_ev", min_support=min_support),
                # every run that is not pinned goes: no count reaches 65535
                "with_min_support_65535": ev("all_ev", min_support=65535),
                "with_min_qual_20": ev("qual_ev", min_qual=20)}
            try:
                with open(os.path.join(ROOT, "profiles", "polish_e2e_bench.json")) as fh:
                    res["parent_plain_wall_s"] = json.load(fh)["e2e"]["wall_s"]
            except (OSError, KeyError, ValueError):
                res["parent_plain_wall_s"] = None
            res["note"] = ("polish_pipeline: the image builder call (with the flag it also writes the depth and the counts plane); "
                           "polish_filter_support / polish_filter: runs + carry + write kernels of one filter call; HIP events around "
                           "every call of a run with --edits, summed over the run's launches. The weights are random, so nearly "
                           "every column is an edit and whole regions are single runs")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def select_kernels(ctx, reads=67_000, regions=1000, reps=20):
    """pv_batch_select_hp_dev alone on a synthetic batch of the shape of one launch of the 3 Mbp run (clipped reads of 600 to
    1700 bases, tags a third each): microseconds per call of every kernel and of the whole call (HIP events, two profiled
    rounds: the kernels, then the call), and bytes per second of the bases / qualities gather and of the call"""
    import numpy as np
    import torch
    import select_ref as sel
    from pepper_thesis_amd.device import DeviceBatch, DeviceSelectOut
    rng = np.random.default_rng(1)
    b = sel.make_batch(rng.integers(600, 1700, reads), rng.integers(20, 60, reads), np.full(regions, reads // regions),
                       rng.integers(0, 3, reads), 2)
    db = DeviceBatch(b)
    so = DeviceSelectOut(regions, b.n_reads, b.n_bases, b.n_cigar, want_src=False)
    torch.cuda.synchronize()
    for _ in range(3):
        ctx.batch_select_hp_dev(db, 1, so)
    ctx.synchronize()
    out = {"reads": reads, "bases": b.n_bases, "cigar_words": b.n_cigar, "reps": reps, "us_per_call": {}}
    for only in ("k_sel", "polish_select"):
        ctx.profile_begin(only)
        for _ in range(reps):
            ctx.batch_select_hp_dev(db, 1, so)
        out["us_per_call"].update({k: round(v[0] / reps * 1e3, 2) for k, v in ctx.profile_end().items()})
    kept, kb, kc, status = so.counts.cpu().numpy().tolist()
    assert status == 0, status
    out["kept_reads_bases_words"] = [kept, kb, kc]
    out["payload_bytes_read_plus_written"] = 2 * (2 * kb + 4 * kc)
    out["gather_bases_gb_per_s"] = round(4 * kb / (out["us_per_call"]["k_sel_gather_bases"] * 1e-6) / 1e9, 1)
    out["call_gb_per_s"] = round(out["payload_bytes_read_plus_written"] / (out["us_per_call"]["polish_select"] * 1e-6) / 1e9, 1)
    return out


def hp_leg(mbp=3.0, threads=16):
    """polish without and with -hp on one synthetic contig whose reads carry HP tags, in one process on the same files"""
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_hp_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000), hp_seed=2024)
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for hp in (False, True):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "hp" if hp else "plain"), threads, False, info, use_hp=hp)
                    runs.append(dict(r, use_hp=hp, order=len(runs)))
            res = {"runs": runs, "without_hp": runs[2], "with_hp": runs[3], "hp_counts_of_the_file": info["hp_counts"]}
            res["hp_over_plain_wall"] = round(runs[3]["wall_s"] / runs[2]["wall_s"], 3)
            # one more -hp run, with --realign, the selection, realigner and builder calls between HIP events
            ctx.profile_begin("polish_")
            try:
                T = {}
                polish.polish_fused(bam, fa, model, os.path.join(d, "hp_ev"), threads=threads, ctx=ctx, realign=True, use_hp=True, timers=T)
            finally:
                pr = ctx.profile_end()
            keep = ("polish_select", "polish_realign", "polish_pipeline", "polish_stitch")
            res["event_ms_launches"] = {k: [round(v[0], 4), v[1]] for k, v in sorted(pr.items()) if k in keep}
            # the selection's payload as the chain counted it: bases, qualities and cigar words of the kept reads, read once and
            # written once, both passes of every launch
            sel_ms, payload = pr.get("polish_select", [0.0, 0])[0], int(T.get("hp_payload_bytes", 0))
            res["selection"] = {"reads_seen": T.get("hp_reads", 0), "calls": pr.get("polish_select", [0.0, 0])[1], "ms": round(sel_ms, 3),
                                "payload_bytes_read_plus_written": payload,
                                "achieved_gb_per_s": round(payload / (sel_ms * 1e-3) / 1e9, 1) if sel_ms else None,
                                "hbm_copy_rate_gb_per_s_for_comparison": 6290}
            res["selection_kernels"] = select_kernels(ctx)
            try:
                with open(os.path.join(ROOT, "profiles", "polish_e2e_bench.json")) as fh:
                    res["parent_plain_wall_s"] = json.load(fh)["e2e"]["wall_s"]
            except (OSError, KeyError, ValueError):
                res["parent_plain_wall_s"] = None
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def min_qual_leg(mbp=3.0, threads=16, min_qual=20):
    """polish without and with --min_qual on one synthetic contig, in one process on the same files"""
    import hashlib
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_min_qual_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for q in (0, min_qual):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "filtered" if q else "plain"), threads, False, info,
                                 min_qual=q)
                    runs.append(dict(r, min_qual=q, order=len(runs)))
            res = {"runs": runs, "without_min_qual": runs[2], "with_min_qual": runs[3]}
            sha = [hashlib.sha256(open(os.path.join(d, n, "_pepper_polished.fa"), "rb").read()).hexdigest() for n in ("plain", "filtered")]
            res["fasta_identical"], res["plain_fasta_sha256"] = sha[0] == sha[1], sha[0]
            res["event_ms_launches"] = {
                "without_min_qual": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "plain_ev"), threads, False, True),
                "with_min_qual": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "filtered_ev"), threads, False, True,
                                                 min_qual=min_qual),
                # every run that is not pinned goes: the write pass stores every edit row
                "with_min_qual_94": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "all_ev"), threads, False, True,
                                                    min_qual=94)}
            try:
                with open(os.path.join(ROOT, "profiles", "polish_e2e_bench.json")) as fh:
                    res["parent_plain_wall_s"] = json.load(fh)["e2e"]["wall_s"]
            except (OSError, KeyError, ValueError):
                res["parent_plain_wall_s"] = None
            res["note"] = ("polish_filter: runs + carry + write kernels of one filter call; polish_row_qual: the row kernel and its "
                           "status kernel (with the flag they run also without --qualities); polish_stitch / polish_edits: count + "
                           "scan + write; HIP events around every call of a run with --edits, summed over the run's launches. The "
                           "weights are random: nearly every column is an edit, whole regions are single runs and no quality "
                           "reaches the threshold, so the reverted rows and the host time are not those of a trained model, and "
                           "the two FASTA files differ wherever a run was taken back")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def edits_leg(mbp=3.0, threads=16):
    """polish without and with --edits on one synthetic contig, in one process on the same files"""
    import hashlib
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_edits_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for e in (False, True):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "edits" if e else "plain"), threads, False, info, edits=e)
                    runs.append(dict(r, edits=e, order=len(runs)))
            res = {"runs": runs, "without_edits": runs[2], "with_edits": runs[3]}
            sha = [hashlib.sha256(open(os.path.join(d, n, "_pepper_polished.fa"), "rb").read()).hexdigest() for n in ("plain", "edits")]
            res["fasta_identical"] = sha[0] == sha[1]
            res["event_ms_launches"] = {
                "without_edits": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "plain_ev"), threads, False),
                "with_edits": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "edits_ev"), threads, False, True)}
            res["note"] = ("polish_stitch / polish_edits: count + scan + write kernels of one call; HIP events around every call of a "
                           "run, summed over the run's launches. The weights are random: most rows are edits, so the record count "
                           "and the bytes read back are far above what a trained model gives")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def evidence_leg(mbp=3.0, threads=16):
    """polish --edits without and with --evidence on one synthetic contig, in one process on the same files"""
    import hashlib
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import bamio, polish, polish_edits, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_evidence_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            runs = []
            for k in range(2):
                for e in (False, True):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "evidence" if e else "edits"), threads, False, info,
                                 edits=True, evidence=e)
                    runs.append(dict(r, evidence=e, order=len(runs)))
            res = {"runs": runs, "without_evidence": runs[2], "with_evidence": runs[3]}
            sha = [hashlib.sha256(open(os.path.join(d, n, "_pepper_polished.fa"), "rb").read()).hexdigest() for n in ("edits", "evidence")]
            res["fasta_identical"], res["fasta_sha256"] = sha[0] == sha[1], sha[0]
            vcf = [bamio.bgzf_read_all(polish_edits.output_vcf_path(os.path.join(d, n, "_pepper_polished.fa"))).decode().split("\n")
                   for n in ("edits", "evidence")]
            blank = [l if l.startswith("#") or not l else "\t".join(l.split("\t")[:7] + ["."]) for l in vcf[1] if not l.startswith("##INFO=")]
            res["vcf_identical_but_info"] = blank == vcf[0]
            ev = lambda name, **kw: _quality_events(polish, ctx, bam, fa, model, os.path.join(d, name), threads, False, **kw)
            res["event_ms_launches"] = {
                "plain": ev("plain_ev"),                                             # the builder without a plane
                "edits": ev("edits_ev", edits=True),                                 # ... and the edits call
                "edits_min_depth_1": ev("depth_ev", edits=True, min_depth=1),        # the builder with the depth plane
                "edits_evidence": ev("evidence_ev", edits=True, evidence=True)}      # both planes, the evidence call
            res["note"] = ("polish_pipeline: the builder call; polish_edits / polish_edits_evidence: count + scan + write kernels of "
                           "one call; HIP events around every call of a run, summed over the run's launches. The weights are random: "
                           "nearly every column is an edit, the worst case for the evidence call, and neither the record count nor "
                           "the host time represents a trained model")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def qualities_leg(mbp=3.0, threads=16):
    """polish without and with --qualities on one synthetic contig, in one process on the same files"""
    import hashlib
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_qual_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            # the two forms alternate, twice each: the first timed run of a process also grows the workspace to the launch size
            runs = []
            for k in range(2):
                for q in (False, True):
                    r = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "qual" if q else "plain"), threads, False, info,
                                 qualities=q)
                    runs.append(dict(r, qualities=q, order=len(runs)))
            res = {"runs": runs, "without_qualities": runs[2], "with_qualities": runs[3]}
            sha = [hashlib.sha256(open(os.path.join(d, n, "_pepper_polished.fa"), "rb").read()).hexdigest() for n in ("plain", "qual")]
            res["fasta_identical"] = sha[0] == sha[1]
            res["event_ms_launches"] = {
                "without_qualities": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "plain_ev"), threads, False),
                "with_qualities": _quality_events(polish, ctx, bam, fa, model, os.path.join(d, "qual_ev"), threads, True)}
            res["note"] = ("polish_stitch: count + scan + write kernels of one stitch call; polish_row_qual: the row kernel and its "
                           "status kernel; HIP events around every call of a run, summed over the run's launches")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def vote_leg(mbp=2.0, threads=16):
    """polish with the seeded model and polish --vote (no model) on one synthetic contig, in one process on the same files,
    each twice in alternation; then one more --vote run, with qualities, whose vote kernels are bracketed by HIP events
    (k_vote_count, k_vote_write; the one-block finish between them is not bracketed) and whose chunks are counted, so that
    the bytes the two kernels move per second can be set against the HBM peak"""
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_vote_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            runs = []
            for rep in range(2):
                for v in (False, True):
                    r = _e2e_run(polish, ctx, bam, fa, None if v else model, os.path.join(d, "vote" if v else "model"), threads, False,
                                 info, vote=v)
                    runs.append(dict(r, vote=v, order=len(runs)))
            res = {"runs": runs, "without_vote": runs[2], "with_vote": runs[3]}
            seen = {"chunks": 0, "calls": 0}
            real = ctx.polish_vote_dev

            def counting(dout, n_chunks, *a, **k):
                seen["chunks"] += int(n_chunks)
                seen["calls"] += 1
                return real(dout, n_chunks, *a, **k)
            ctx.polish_vote_dev = counting
            ctx.profile_begin("k_vote")
            try:
                polish.polish_fused(bam, fa, None, os.path.join(d, "vote_ev"), threads=threads, ctx=ctx, qualities=True, vote=True)
            finally:
                pr = ctx.profile_end()
                del ctx.polish_vote_dev
            rows = seen["chunks"] * 1000
            ms = {k: [round(v[0], 4), v[1]] for k, v in sorted(pr.items())}
            # per row: position 8, index 4, counts 20, depth 2 and the draft byte read by both kernels; label 1 and acc 20 written
            count_b, write_b = rows * (8 + 4 + 20 + 2 + 1), rows * (8 + 4 + 20 + 2 + 1 + 1 + 20)
            res["vote_kernels"] = {"chunks": seen["chunks"], "calls": seen["calls"], "kernel_ms": ms, "with_acc": True,
                                   "bytes": {"k_vote_count": count_b, "k_vote_write": write_b}}
            for k, b in (("k_vote_count", count_b), ("k_vote_write", write_b)):
                if k in pr and pr[k][0] > 0:
                    res["vote_kernels"][k + "_gb_per_s"] = round(b / (pr[k][0] * 1e-3) / 1e9, 1)
            res["note"] = ("without_vote runs the seeded random model: its sequence is noise and only its time is of interest; "
                           "the vote kernels' bytes count every plane a row reads once per kernel (the insert rows' depth and the "
                           "base rows' draft byte both counted for every row)")
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def runs_leg(mbp=2.0, threads=16, min_run=3):
    """polish --vote without and with --runs on one synthetic contig, in one process on the same files, each twice in
    alternation; then two more --vote --runs runs with qualities under HIP events: one brackets the whole calls (the image
    builder, the column vote, the run vote), the other the run vote's kernels (the one-block finish is not bracketed)"""
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime
    d = tempfile.mkdtemp(prefix="pv_polish_runs_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        ctx = runtime.Context(0)
        try:
            runs = []
            for rep in range(2):
                for v in (0, min_run):
                    r = _e2e_run(polish, ctx, bam, fa, None, os.path.join(d, "runs" if v else "vote"), threads, False, info,
                                 vote=True, vote_runs=v)
                    runs.append(dict(r, runs=bool(v), order=len(runs)))
            res = {"runs": runs, "without_runs": runs[2], "with_runs": runs[3]}
            for key, only in (("calls_ms", "polish_"), ("run_vote_kernels_ms", "k_runs")):
                ctx.profile_begin(only)
                try:
                    polish.polish_fused(bam, fa, None, os.path.join(d, "ev_" + key), threads=threads, ctx=ctx, qualities=True,
                                        vote=True, vote_runs=min_run)
                finally:
                    pr = ctx.profile_end()
                res[key] = {k: [round(v[0], 4), v[1]] for k, v in sorted(pr.items())}
            b, r = res["calls_ms"].get("polish_pipeline"), res["calls_ms"].get("polish_vote_runs")
            if b and r and b[0] > 0:
                res["run_vote_over_builder"] = round(r[0] / b[0], 3)
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def e2e_leg(mbp=2.0, threads=16, realign=False, gpu_decode=False):
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_e2e_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        try:
            out = _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "out"), threads, False, info, gpu_decode)
            if not realign:
                return out
            res = {"without_realign": out,
                   "with_realign": _e2e_run(polish, ctx, bam, fa, model, os.path.join(d, "out_rl"), threads, True, info, gpu_decode)}
            res["realign"] = st = realign_stats(ctx, bam, fa)
            rl_s = sum(st["kernel_ms"].values()) / 1e3
            res["realign"]["kernel_s"] = round(rl_s, 3)
            res["realign"]["share_of_e2e_wall"] = round(rl_s / res["with_realign"]["wall_s"], 3)
            return res
        finally:
            ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _polish_command(bam, fa, model, out, threads, d_ids, realign, shared_env):
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""))
    env.pop("PV_SHARED_DEVICE", None)
    if shared_env:
        env["PV_SHARED_DEVICE"] = "1"
    cmd = [sys.executable, "-m", "pepper_thesis_amd", "polish", "-b", bam, "-f", fa, "-m", model, "-o", out, "-t", str(threads),
           "-d_ids", d_ids] + (["--realign"] if realign else [])
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1800)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("polish -d_ids %s: exit status %d\n%s" % (d_ids, r.returncode, r.stderr[-3000:]))
    with open(os.path.join(out, "_pepper_polished.fa"), "rb") as fh:
        return fh.read(), round(wall, 3)


def ranks_leg(mbp=2.0, threads=16, d_ids="0,0", realign=False):
    """`polish -d_ids <d_ids>` against `polish -d_ids <first id>` with PV_SHARED_DEVICE=1, each a fresh process (start-up, context
    creation and model load included in the wall time)"""
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import synth
    d = tempfile.mkdtemp(prefix="pv_polish_ranks_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        first = d_ids.split(",")[0]
        one, wall_one = _polish_command(bam, fa, model, os.path.join(d, "one"), threads, first, realign, True)
        many, wall_many = _polish_command(bam, fa, model, os.path.join(d, "many"), threads, d_ids, realign, False)
        return {"draft_bp": int(mbp * 1_000_000), "reads": info["reads"], "realign": realign, "reader_threads_total": threads,
                "single": {"d_ids": first, "env": "PV_SHARED_DEVICE=1", "wall_s": wall_one, "fasta_bytes": len(one)},
                "ranks": {"d_ids": d_ids, "wall_s": wall_many, "fasta_bytes": len(many)},
                "identical": one == many,
                "note": "ranks sharing a device split its CPUs and the card: a correctness rehearsal, not a scaling figure"}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _pepper_command(argv, what):
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else ""),
               PV_SHARED_DEVICE="1")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m", "pepper_thesis_amd.pepper"] + argv, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=1800)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: exit status %d\n%s" % (what, r.returncode, r.stderr[-3000:]))
    return round(wall, 3)


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d))


def steps_leg(mbp=3.0, threads=16):
    """make_images -> call_consensus -> stitch against the fused polish on one synthetic contig, each a fresh process"""
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import synth
    d = tempfile.mkdtemp(prefix="pv_polish_steps_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        img, pred = os.path.join(d, "img"), os.path.join(d, "pred")
        res = {"draft_bp": int(mbp * 1_000_000), "reads": info["reads"], "threads": threads, "env": "PV_SHARED_DEVICE=1"}
        res["polish_s"] = _pepper_command(["polish", "-b", bam, "-f", fa, "-m", model, "-o", os.path.join(d, "fused"), "-t",
                                           str(threads)], "polish")
        res["make_images_s"] = _pepper_command(["make_images", "-b", bam, "-f", fa, "-o", img, "-t", str(threads)], "make_images")
        res["call_consensus_s"] = _pepper_command(["call_consensus", "-i", img, "-m", model, "-o", pred], "call_consensus")
        res["stitch_s"] = _pepper_command(["stitch", "-i", pred, "-o", os.path.join(d, "steps", "p")], "stitch")
        res["steps_total_s"] = round(res["make_images_s"] + res["call_consensus_s"] + res["stitch_s"], 3)
        res["image_files"], res["image_bytes"] = len(os.listdir(img)), _dir_bytes(img)
        res["prediction_files"], res["prediction_bytes"] = len(os.listdir(pred)), _dir_bytes(pred)
        with open(os.path.join(d, "fused", "_pepper_polished.fa"), "rb") as a, open(os.path.join(d, "steps", "p_pepper_polished.fa"),
                                                                                     "rb") as b:
            fused, steps = a.read(), b.read()
        res["fasta_bytes"], res["identical"] = len(fused), fused == steps
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("stitch", "e2e", "steps", "all"), default="all")
    ap.add_argument("--mbp", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--realign", action="store_true", help="e2e leg without and with polish --realign, plus realigner stats")
    ap.add_argument("--d_ids", type=str, default=None,
                    help="e2e leg: the polish command with these -d_ids against the first id alone with PV_SHARED_DEVICE=1")
    ap.add_argument("--gpu_decode", action="store_true",
                    help="e2e leg: the device read path (polish --gpu_decode); adds the decode timers and the FASTA's sha256")
    ap.add_argument("--qualities", action="store_true",
                    help="e2e leg without and with polish --qualities, plus HIP-event times of the stitch and row-quality calls")
    ap.add_argument("--edits", action="store_true",
                    help="e2e leg without and with polish --edits, plus HIP-event times of the stitch and the edit calls")
    ap.add_argument("--evidence", action="store_true",
                    help="with --edits: e2e leg of polish --edits without and with --evidence, plus HIP-event times of the builder "
                         "without a plane, with the depth plane and with both, and of the edits call against the evidence call")
    ap.add_argument("--min_depth", type=int, default=0,
                    help="e2e leg without and with polish --min_depth N, plus HIP-event times of the builder, mask and stitch calls")
    ap.add_argument("--min_qual", type=int, default=0,
                    help="e2e leg without and with polish --min_qual Q, plus HIP-event times of the row-quality, filter, stitch and edit calls")
    ap.add_argument("--min_support", type=int, default=0,
                    help="e2e leg without and with polish --min_support K, plus HIP-event times of the builder, the support filter, "
                         "the quality filter (at 20, in a run of its own), stitch and edit calls")
    ap.add_argument("-hp", "--use_hp_info", action="store_true",
                    help="e2e leg without and with polish -hp on a BAM with HP tags, plus HIP-event times of the selection, realigner and builder calls")
    ap.add_argument("--vote", action="store_true",
                    help="e2e leg with the seeded model and with polish --vote (no model), plus HIP-event times of the vote kernels "
                         "and the bytes they move per second")
    ap.add_argument("--runs", type=int, default=0, metavar="MIN_RUN",
                    help="e2e leg of polish --vote without and with --runs --min_run MIN_RUN, plus HIP-event times of the image "
                         "builder, the column vote and the run vote, and of the run vote's kernels")
    ap.add_argument("--out", type=str, default=None, help="also write the JSON to this file")
    a = ap.parse_args()
    out = {}
    if a.leg in ("stitch", "all"):
        out["stitch"] = stitch_leg(a.reps)
    if a.leg in ("e2e", "all"):
        if a.use_hp_info:
            out["e2e"] = hp_leg(a.mbp, a.threads)
        elif a.runs:
            out["e2e"] = runs_leg(a.mbp, a.threads, a.runs)
        elif a.vote:
            out["e2e"] = vote_leg(a.mbp, a.threads)
        elif a.min_support:
            out["e2e"] = min_support_leg(a.mbp, a.threads, a.min_support)
        elif a.min_qual:
            out["e2e"] = min_qual_leg(a.mbp, a.threads, a.min_qual)
        elif a.min_depth:
            out["e2e"] = min_depth_leg(a.mbp, a.threads, a.min_depth)
        elif a.edits:
            out["e2e"] = evidence_leg(a.mbp, a.threads) if a.evidence else edits_leg(a.mbp, a.threads)
        elif a.qualities:
            out["e2e"] = qualities_leg(a.mbp, a.threads)
        else:
            out["e2e"] = ranks_leg(a.mbp, a.threads, a.d_ids, a.realign) if a.d_ids else e2e_leg(a.mbp, a.threads, a.realign, a.gpu_decode)
    if a.leg == "steps":
        out["steps"] = steps_leg(a.mbp, a.threads)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
