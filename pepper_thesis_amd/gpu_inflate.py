"""The opt-in GPU inflate stage of the BAM readers (`--gpu_inflate`).

A reader thread plans its intervals' BGZF blocks (bamio.plan_blocks: header walk, raw payloads), hands the plan to the ONE
service thread of this module and waits; the service takes every plan that is waiting (up to a call's worth of reader
groups), lays the payloads and block tables end to end in a pinned host buffer, copies it up, runs pv_bgzf_inflate_dev on a
stream of its own, copies the inflated bytes and the per-block statuses back into pinned host memory and hands every reader
its slice; the reader then parses records from it (bamio.fill_batch_blocks). Only the service thread makes HIP calls here,
and pv_bgzf_inflate_dev uses no context workspace, so the inflate runs beside the builder and RNN calls on the context's
own stream. A block that fails (corrupt payload, CRC32 or length mismatch) fails its reader with an IOError naming the
block's compressed offset, as the host reader does.
"""
import queue
import threading
import time
from concurrent.futures import Future

import numpy as np

from . import _ffi

MARGIN_BLOCKS = 1   # blocks planned past every BAI chunk's last block (a block still missing is inflated on the host)


def _align8(n: int) -> int:
    return (n + 7) & ~7


class GpuInflater:
    def __init__(self, ctx, max_plans: int, T: dict):
        import torch
        self.ctx, self.max_plans, self.T = ctx, max(1, int(max_plans)), T
        self.dev = "cuda:%d" % ctx.device_id
        self.stream = torch.cuda.Stream(device=self.dev)
        for k in ("gpu_inflate_kernel_ms", "gpu_inflate_h2d_ms", "gpu_inflate_d2h_ms", "gpu_inflate_plan_cpu_s"):
            T.setdefault(k, 0.0)
        for k in ("gpu_inflate_launches", "gpu_inflate_blocks", "gpu_inflate_bytes", "gpu_inflate_blocks_host"):
            T.setdefault(k, 0)
        self.lock = threading.Lock()   # guards T from the reader threads
        self.q: "queue.Queue" = queue.Queue()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def submit(self, plan) -> Future:
        """-> a Future of (pinned uint8 tensor holding the plan's blocks at plan.out_off, bytes)"""
        f: Future = Future()
        self.q.put((plan, f))
        return f

    def add(self, key: str, v):
        with self.lock:
            self.T[key] += v

    def close(self):
        self.q.put(None)
        self.thread.join()

    def _run(self):
        stop = False
        while not stop:
            item = self.q.get()
            if item is None:
                break
            items = [item]
            while len(items) < self.max_plans:
                try:
                    nxt = self.q.get_nowait()
                except queue.Empty:
                    break
                if nxt is None:
                    stop = True
                    break
                items.append(nxt)
            try:
                self._launch(items)
            except BaseException as e:   # every waiting reader gets the error; none is left waiting
                for _, f in items:
                    if not f.done():
                        f.set_exception(e)

    def _launch(self, items):
        import torch
        plans = [p for p, _ in items]
        n = sum(p.n_blocks for p in plans)
        pay_bytes = sum(int(p.payload.size) for p in plans)
        out_bytes = sum(p.out_bytes for p in plans)
        # one pinned staging buffer: payloads, then the table arrays (8-byte aligned)
        sizes = [("payload", pay_bytes), ("in_off", 8 * n), ("out_off", 8 * n), ("clen", 4 * n), ("isize", 4 * n), ("crc", 4 * n)]
        offs, o = {}, 0
        for k, s in sizes:
            offs[k] = o
            o = _align8(o + s)
        up = torch.empty(max(o, 8), dtype=torch.uint8, pin_memory=True)
        h = up.numpy()
        views = {k: h[offs[k]:offs[k] + s] for k, s in sizes}
        in_off = views["in_off"].view(np.int64)
        out_off = views["out_off"].view(np.int64)
        clen, isize, crc = views["clen"].view(np.int32), views["isize"].view(np.int32), views["crc"].view(np.uint32)
        pb = ob = bi = 0
        first = []
        for p in plans:
            k = p.n_blocks
            views["payload"][pb:pb + p.payload.size] = p.payload
            in_off[bi:bi + k] = p.in_off + pb
            out_off[bi:bi + k] = p.out_off + ob
            clen[bi:bi + k], isize[bi:bi + k], crc[bi:bi + k] = p.clen, p.isize, p.crc
            first.append((bi, ob))
            pb += int(p.payload.size)
            ob += p.out_bytes
            bi += k
        down = torch.empty(max(out_bytes, 1), dtype=torch.uint8, pin_memory=True)
        status_h = torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        with torch.cuda.stream(self.stream):
            d_up = torch.empty_like(up, device=self.dev)
            d_out = torch.empty(max(out_bytes, 1), dtype=torch.uint8, device=self.dev)
            d_status = torch.empty(max(n, 1), dtype=torch.int32, device=self.dev)
            d_counts = torch.empty(4, dtype=torch.int64, device=self.dev)
            ev[0].record(self.stream)
            d_up.copy_(up, non_blocking=True)
            ev[1].record(self.stream)
            base = d_up.data_ptr()
            self.ctx.bgzf_inflate_dev(base + offs["payload"], pay_bytes, n, base + offs["in_off"], base + offs["clen"],
                                      base + offs["isize"], base + offs["crc"], base + offs["out_off"], d_out.data_ptr(),
                                      out_bytes, d_status.data_ptr(), d_counts.data_ptr(), self.stream.cuda_stream)
            ev[2].record(self.stream)
            down.copy_(d_out, non_blocking=True)
            status_h.copy_(d_status, non_blocking=True)
            ev[3].record(self.stream)
        self.stream.synchronize()
        with self.lock:
            T = self.T
            T["gpu_inflate_h2d_ms"] += ev[0].elapsed_time(ev[1])
            T["gpu_inflate_kernel_ms"] += ev[1].elapsed_time(ev[2])
            T["gpu_inflate_d2h_ms"] += ev[2].elapsed_time(ev[3])
            T["gpu_inflate_launches"] += 1
            T["gpu_inflate_blocks"] += n
            T["gpu_inflate_bytes"] += out_bytes
        status = status_h.numpy()[:n]
        dv = down.numpy()
        for (p, f), (b0, o0) in zip(items, first):
            st = status[b0:b0 + p.n_blocks]
            bad = np.flatnonzero(st != _ffi.PV_BGZF_OK)
            if bad.size:
                i = int(bad[0])
                f.set_exception(IOError("BGZF block at offset %d: %s (corrupt file; GPU inflate)" %
                                        (int(p.coffset[i]), _ffi.BGZF_STATUS_NAMES.get(int(st[i]), "status %d" % int(st[i])))))
            else:
                f.set_result((down, dv[o0:o0 + p.out_bytes]))


def read_group_gpu(inflater: GpuInflater, bam, fasta, ivs, min_mapq, include_supplementary, downsample_rate, safe_bases):
    """plan -> GPU inflate -> records: what bamio.fill_batch returns, for one reader group (runs on a reader thread)"""
    from .bamio import fill_batch_blocks, plan_blocks
    t0 = time.perf_counter()
    plan = plan_blocks(bam, ivs, safe_bases, MARGIN_BLOCKS)
    inflater.add("gpu_inflate_plan_cpu_s", time.perf_counter() - t0)
    keep, data = inflater.submit(plan).result()
    fb = fill_batch_blocks(bam, fasta, ivs, plan.coffset, plan.next_coffset, plan.isize, plan.out_off, data, min_mapq,
                           include_supplementary, downsample_rate, safe_bases)
    del keep
    inflater.add("gpu_inflate_blocks_host", fb.blocks_host)
    return fb
