#!/usr/bin/env python3
"""The polisher end to end, and its stitch step on its own.

  stitch leg: the 2121-chunk batch of tools/bench_polish.py (8 synthetic regions of 100 k columns) through the builder and the
              bi-GRU once; then pv_polish_stitch_dev alone, timed with HIP events (per kernel and the whole call), against the
              reference-style host stitch (tests/stitch_ref.py: dict + string-sorted chunk ids + global sort) on the same labels,
              and the bytes each way has to move off the device.
  e2e leg:    a synthetic contig (tools/bench_filepath.make_files: 60x, 10 kb reads) written as BAM + FASTA, then
              polish.polish_fused (readers -> builder -> bi-GRU -> stitch -> FASTA): wall time and draft Mbp/s.

  python tools/bench_polish_e2e.py [--leg stitch|e2e|all] [--mbp 2.0] [--reps 20]
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


def e2e_leg(mbp=2.0, threads=16):
    import numpy as np
    from bench_filepath import make_files
    from pepper_thesis_amd import polish, runtime, synth
    d = tempfile.mkdtemp(prefix="pv_polish_e2e_")
    try:
        bam, fa, info = make_files(d, int(mbp * 1_000_000))
        model = os.path.join(d, "model.npz")
        np.savez(model, **synth.make_weights_p2(4321, 3.0))
        ctx = runtime.Context(0)
        # warm-up on a small region (code objects, allocator), then the timed run
        polish.polish_fused(bam, fa, model, os.path.join(d, "warm"), region="chr20:0-50000", threads=threads, ctx=ctx)
        T = {}
        t0 = time.perf_counter()
        path = polish.polish_fused(bam, fa, model, os.path.join(d, "out"), threads=threads, ctx=ctx, timers=T)
        wall = time.perf_counter() - t0
        ctx.close()
        size = os.path.getsize(path)
        return {"draft_bp": T["bases_in"], "reads": info["reads"], "regions": T["regions"], "batches": T["batches"],
                "polished_bp": T["bases_out"], "fasta_bytes": size, "wall_s": round(wall, 3),
                "read_s": round(T["read_s"], 3), "device_s": round(T["device_s"], 3),
                "draft_mbp_per_s": round(T["bases_in"] / wall / 1e6, 4), "reader_threads": threads}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("stitch", "e2e", "all"), default="all")
    ap.add_argument("--mbp", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    out = {}
    if a.leg in ("stitch", "all"):
        out["stitch"] = stitch_leg(a.reps)
    if a.leg in ("e2e", "all"):
        out["e2e"] = e2e_leg(a.mbp, a.threads)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
