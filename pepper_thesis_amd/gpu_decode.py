"""The opt-in GPU record decode of the BAM readers (`--gpu_decode`; it implies `--gpu_inflate`).

Reader threads only plan: the BGZF blocks of their intervals (bamio.plan_blocks), the interval table the reader works out
before it reads a byte (bamio.plan_intervals) and the reference bytes (one pvio_fasta_fetch per interval). The consumer hands
a call's worth of planned groups to the ONE service thread of this module, which lays payloads, tables and reference bytes
end to end in a pinned buffer and runs, on a stream of its own:

    H2D -> pv_bgzf_inflate_dev -> pv_bam_scan_dev -> D2H of the per-interval counts (64 bytes per interval)
        -> host: reservoir indices where an interval holds more reads than min(MAX_READS_IN_REGION, rate * n), region table
        -> pv_bam_fill_dev

The result is a DecodedBatch: a device-resident pv_batch_in plus read_hp, in the layout and order of bamio.fill_batch, which
the *_dev builders take as it is (it offers what device.DeviceBatch offers). No inflated byte and no read array crosses PCIe.
A group whose walk needs bytes outside the plan (reads longer than the plan's 32 kb look-ahead) is read through the
gpu_inflate route instead - its inflated bytes are copied down and bamio.fill_batch_blocks parses them - and counted in the
timer `gpu_decode_groups_host`. A corrupt record or block fails with the host reader's own message.

The polisher (`polish --gpu_decode`) uses the same kernels with its own settings (no safe bases, MAPQ 0, 1500 reads, draft
bytes padded with N past the contig end, realign windows) and its own shape of work: about a thousand 1 kb regions per chain
launch. region_groups cuts the work list into reader groups (short runs of regions that share BGZF blocks), plan_launches
packs groups into scans whose workspace stays under a budget, compose_launches cuts the scanned regions into the launches the
host path would make, and GpuDecoder.scan_groups / realize run them (decoded_launches, polish.polish_pieces).
"""
import queue
import threading
import time
from collections import deque
from concurrent.futures import Future, ThreadPoolExecutor

import numpy as np

from . import _ffi, bamio
from .gpu_inflate import MARGIN_BLOCKS, _align8

REC_MIN_BYTES = 36   # block_size field + the 32 fixed bytes: no record is shorter, so bytes / 36 + 1 slots always suffice
SLOT_BYTES = 60      # decode workspace per record slot (include/pepper_hip.h)
DEFAULT_WS_BUDGET = 4 << 30   # bytes of decode workspace one scan may allocate (DESIGN.md 4.6 has the measured sizes)
GROUP_REGIONS = 16   # regions of one polisher reader group at most: the 1 kb regions of one 16 kb BAI window
GROUP_SHIFT = 14     # ... regions whose starts share start >> 14 fall into the same smallest BAI bin: the same chunks and blocks


def safe_slots(out_bytes: int) -> int:
    """record slots that always suffice for one interval of a group with out_bytes inflated bytes"""
    return int(out_bytes) // REC_MIN_BYTES + 1


def interval_slots(out_bytes: int, min_record_bytes: int = REC_MIN_BYTES) -> int:
    """slots for one interval when no record is taken to be shorter than min_record_bytes (never more than safe_slots)"""
    return min(safe_slots(out_bytes), int(out_bytes) // max(int(min_record_bytes), REC_MIN_BYTES) + 1)


def decode_ws_bytes(n_intervals: int, slots: int) -> int:
    """bytes GpuDecoder allocates as the workspace of one scan: pv_bam_decode_ws_bytes (12 per-slot arrays, 60 bytes per slot,
    each rounded up to 8 bytes, and 44 bytes per interval) rounded up to whole int64 words plus one"""
    up8 = lambda x: (int(x) + 7) & ~7
    N, S = int(n_intervals), int(slots)
    lib = 3 * up8(8 * S) + 9 * up8(4 * S) + 24 * N + 8 * (N + 1) + 3 * up8(4 * N) + 8
    return 8 * max(lib // 8 + 1, 1)


def region_groups(work, max_regions: int = GROUP_REGIONS):
    """the polisher's reader groups: `work` (objects with contig, start, end, in run order) -> lists of consecutive entries
    of one contig, starts ascending inside one 16 kb BAI window, max_regions at most. Such regions ask the index for the
    same bins, so a group's blocks are read and inflated once. Every entry lands in exactly one group, in order."""
    groups, cur = [], []
    for w in work:
        if cur and (len(cur) >= max_regions or w.contig != cur[0].contig or w.start < cur[-1].start
                    or (w.start >> GROUP_SHIFT) != (cur[0].start >> GROUP_SHIFT)):
            groups.append(cur)
            cur = []
        cur.append(w)
    if cur:
        groups.append(cur)
    return groups


def plan_launches(sizes, budget=None, min_record_bytes=REC_MIN_BYTES):
    """Which groups share a scan. sizes: [(intervals, inflated bytes)] of the planned groups in order; budget: bytes of decode
    workspace one scan may allocate (None: no limit). -> [("dev", [group indices], [slots per interval of each])
    | ("host", [group index], None)] covering every group once, in order. A scan is cut before the group that would take
    its workspace past the budget; a group whose safe-rule workspace alone is over the budget goes the host route (so a
    retry with the safe rule always fits). min_record_bytes: the slot rule, one value or one per group."""
    out, cur, per, n, slots = [], [], [], 0, 0

    def cut():
        nonlocal cur, per, n, slots
        if cur:
            out.append(("dev", cur, per))
        cur, per, n, slots = [], [], 0, 0

    for gi, (n_iv, out_bytes) in enumerate(sizes):
        n_iv = int(n_iv)
        if budget is not None and decode_ws_bytes(n_iv, n_iv * safe_slots(out_bytes)) > budget:
            cut()
            out.append(("host", [gi], None))
            continue
        p = interval_slots(out_bytes, min_record_bytes[gi] if isinstance(min_record_bytes, (list, tuple)) else min_record_bytes)
        if budget is not None and cur and decode_ws_bytes(n + n_iv, slots + n_iv * p) > budget:
            cut()
        cur.append(gi)
        per.append(p)
        n += n_iv
        slots += n_iv * p
    cut()
    return out


def compose_launches(scans, per_launch: int, on_part=None):
    """The chain launches of the polisher from scanned groups. scans: iterable, in work order, of objects with kind ("dev" |
    "host" | an exception, raised here), reads (reads kept per interval; 0 drops the region), key (groups with the same key
    were scanned together: their regions can share one fill) and n (intervals). -> lists of parts [kind, key, [(scan, k)]]:
    per_launch regions with reads each (the last may be short), in order - what the host path's flush makes of the same
    regions. Consecutive regions of one kind and key share a part.
    A None among the scans says that nothing with the keys seen so far follows: the open part is complete. on_part(part) is
    called once for every part as soon as it is complete - at such a None, when another part begins, or when its launch is
    cut - and what it returns takes the part's place in the launch (the decoder fills a scan's regions there and lets the
    scan's buffers go before the next scan runs)."""
    cur, n, is_open = [], 0, False

    def close():
        nonlocal is_open
        if is_open:
            is_open = False
            if on_part is not None:
                cur[-1] = on_part(cur[-1])

    for gs in scans:
        if gs is None:
            close()
            continue
        if isinstance(gs.kind, BaseException):
            raise gs.kind
        for k in range(gs.n):
            if int(gs.reads[k]) <= 0:
                continue
            if is_open and cur[-1][0] == gs.kind and cur[-1][1] is gs.key:
                cur[-1][2].append((gs, k))
            else:
                close()
                cur.append([gs.kind, gs.key, [(gs, k)]])
                is_open = True
            n += 1
            if n == per_launch:
                close()
                yield cur
                cur, n = [], 0
    close()
    if cur:
        yield cur


class PlannedGroup:
    """what a reader thread prepares for one group of intervals (host work only)"""

    def __init__(self, bam, fasta, ivs, safe_bases, pad_ref=False, windows=False, works=None):
        """pad_ref: the polisher's reference bytes - draft [start, end] padded with N to end - start + 1 past the contig end
        (polish_summary.region_from_files); windows: also its realign window per interval, draft [start, min(end +
        realign.SAFE_BASES, contig length)); works: the caller's own object per interval (polish.Work)."""
        from .realign import SAFE_BASES
        t0, c0 = time.perf_counter(), time.thread_time()
        self.ivs = list(ivs)
        self.works = works
        self.plan = bamio.plan_blocks(bam, ivs, safe_bases, MARGIN_BLOCKS)
        self.ivp = bamio.plan_intervals(bam, ivs, safe_bases)
        self.refs, self.ref_err = [], []
        self.windows = [] if windows else None
        for k, iv in enumerate(self.ivs):
            if pad_ref and int(iv[1]) < 0:
                raise ValueError("gpu_decode: region %s:%d-%d starts before the contig" % tuple(iv))
            try:   # (the reader fetches only for intervals with reads: an error here is raised only if this one has some)
                r = bamio.fetch_reference(fasta, iv[0], int(self.ivp.rs[k]), int(self.ivp.re[k]) + 1)
                if pad_ref:
                    want = int(iv[2]) - int(iv[1]) + 1
                    if r.size < want:   # past the contig end: columns without reads; the polisher never reads the bytes
                        r = np.concatenate([r, np.full(want - r.size, ord("N"), np.uint8)])
                if windows:
                    stop = min(int(iv[2]) + SAFE_BASES, fasta.get_chromosome_sequence_length(iv[0]))
                    self.windows.append(bamio.fetch_reference(fasta, iv[0], int(iv[1]), stop).tobytes())
                self.refs.append(r)
                self.ref_err.append(None)
            except IOError as e:
                self.refs.append(np.zeros(0, np.uint8))
                self.ref_err.append(e)
                if windows and len(self.windows) <= k:
                    self.windows.append(b"")
        self.t_plan, self.cpu_plan = time.perf_counter() - t0, time.thread_time() - c0   # wall and CPU seconds of this thread


class DecodedBatch:
    """A device-resident batch as bamio.fill_batch lays it out. `c` is the pv_batch_in of device pointers; read_hp the int32
    tags; the totals the *_dev builders take as attributes, as on device.DeviceBatch. interval_index / reads_seen as on
    bamio.FilledBatch (interval_index counts through `intervals`, the intervals of the groups decoded together)."""

    def __init__(self, t, n_regions, intervals, interval_index, reads_seen, n_reads, n_ref_bytes, max_region_len, event):
        self.t, self.n_regions, self.intervals = t, int(n_regions), list(intervals)
        self.interval_index, self.reads_seen = interval_index, reads_seen
        self.n_reads, self.n_bases, self.n_cigar = int(n_reads), 0, 0   # (bases / words: set when the totals are back)
        self.qmax = 0   # the longest read (set with the totals when the decoder was asked for it: the realigner's bound)
        self.n_ref_bytes, self.max_region_len = int(n_ref_bytes), int(max_region_len)
        self.read_hp = t["read_hp"]
        self.event = event
        c = _ffi.pv_batch_in()
        c.n_regions = self.n_regions
        for f in _BATCH_FIELDS:
            setattr(c, f, t[f].data_ptr())
        self.c = c

    def wait_on(self, ctx):
        """order the decode (service stream) before whatever ctx's stream runs next"""
        import torch
        torch.cuda.ExternalStream(ctx.stream, device="cuda:%d" % ctx.device_id).wait_event(self.event)

    def uploaded(self):
        """the triple Context.summarize_uploaded takes (as Context.upload_batches returns it)"""
        return self.c, [self.n_reads, self.n_bases, self.n_cigar, self.n_ref_bytes], self

    def to_host(self):
        """-> (batch.RegionBatch, read_hp int32 array): a host copy, for tests and tools"""
        from .batch import RegionBatch
        sizes = dict(read_pos=self.n_reads, read_flags=self.n_reads, read_mapq=self.n_reads, base_off=self.n_reads + 1,
                     bases=self.n_bases, quals=self.n_bases, cigar_off=self.n_reads + 1, cigar=self.n_cigar, ref=self.n_ref_bytes)
        a = {}
        for f in _BATCH_FIELDS:
            v = self.t[f].cpu().numpy()
            v = v[:sizes[f]] if f in sizes else v
            a[f] = v.view(np.uint32) if f == "cigar" else v
        names = [self.intervals[int(i)][0] for i in self.interval_index]
        b = RegionBatch(self.n_regions, *[a[f] for f in _BATCH_FIELDS], names)
        return b, self.read_hp.cpu().numpy()[:self.n_reads]


_BATCH_FIELDS = ("ref_start", "ref_end", "cand_start", "cand_end", "ref_off", "ref", "read_off", "read_pos", "read_flags",
                 "read_mapq", "base_off", "bases", "quals", "cigar_off", "cigar")


def _stage(sizes):
    """offsets of 8-byte aligned pieces laid end to end -> (offsets, total bytes)"""
    offs, o = {}, 0
    for k, s in sizes:
        offs[k] = o
        o = _align8(o + int(s))
    return offs, max(o, 8)


class _Scan:
    """what one pv_bam_scan_dev call left: the groups it covered, where each begins (first block, first data byte, first
    interval), the per-interval counts and block status on the host, and the device buffers the fills read"""

    def __init__(self, groups, per):
        self.groups, self.per = list(groups), list(per)


class GroupScan:
    """one planned group after its scan, as compose_launches takes it: kind "dev" | "host" | an exception; reads kept per
    interval; key: the _Scan a "dev" group's fills read (regions of one key can share a fill), for a "host" group the group
    itself; regions: a "host" group's polish_summary regions (None where there are no reads)"""

    def __init__(self, group, kind, reads, key, gi=0, regions=None):
        self.group, self.kind, self.reads, self.key, self.gi, self.regions = group, kind, reads, key, gi, regions
        self.n = len(group.ivs)


class GpuDecoder:
    def __init__(self, ctx, bam_path, fasta_path, min_mapq, include_supplementary, downsample_rate, safe_bases, T: dict,
                 max_reads=None, ws_budget=None, min_record_bytes=REC_MIN_BYTES, adaptive_slots=False, realign=False):
        """max_reads: the reservoir's read limit per interval (None: bamio.MAX_READS_IN_REGION, read when it is used).
        The rest is used by scan_groups (the polisher's form) only - ws_budget: bytes of decode workspace one scan may
        allocate (None: DEFAULT_WS_BUDGET); min_record_bytes: slots per interval = bytes of the group's blocks /
        min_record_bytes + 1 (36: the safe rule; more gives fewer slots, and a group that runs out is scanned again, once,
        with the safe rule); adaptive_slots: after the first scan, size the slots from the records per inflated byte the
        scans have seen so far (four times the densest interval); realign: host-route regions fetch their realign window."""
        import torch
        self.ctx, self.T = ctx, T
        self.bam_path, self.fasta_path = bam_path, fasta_path
        self.min_mapq, self.include_supplementary = int(min_mapq), bool(include_supplementary)
        self.downsample_rate, self.safe_bases = float(downsample_rate), int(safe_bases)
        self.max_reads = max_reads
        self.ws_budget = DEFAULT_WS_BUDGET if ws_budget is None else int(ws_budget)
        self.min_record_bytes, self.adaptive_slots, self.realign = int(min_record_bytes), bool(adaptive_slots), bool(realign)
        self.live = [0, 0]    # bytes of the live scans: workspaces, all device buffers (_account)
        self.density = 0.0    # records walked per inflated byte of the group: the largest any interval has shown
        self.want_qmax = self.realign   # the fills also reduce the longest read of the batch (the realigner's bound)
        self.dev = "cuda:%d" % ctx.device_id
        self.stream = torch.cuda.Stream(device=self.dev)
        for k in ("gpu_inflate_kernel_ms", "gpu_inflate_h2d_ms", "gpu_decode_scan_ms",
                  "gpu_decode_fill_ms", "gpu_decode_host_s"):
            T.setdefault(k, 0.0)
        for k in ("gpu_inflate_launches", "gpu_inflate_blocks", "gpu_inflate_bytes", "gpu_inflate_blocks_host", "gpu_decode_groups",
                  "gpu_decode_groups_host", "gpu_decode_h2d_bytes", "gpu_decode_d2h_bytes", "gpu_decode_records"):
            T.setdefault(k, 0)
        self.handles = None   # the service thread's own reader pair, opened when a group first needs the host route
        self.closing = False
        self.q: "queue.Queue" = queue.Queue()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _read_limit(self):
        return int(bamio.MAX_READS_IN_REGION if self.max_reads is None else self.max_reads)

    def submit(self, groups) -> Future:
        """-> a Future of the list of items of these groups, in order: ("dev", DecodedBatch), ("host", bamio.FilledBatch)
        or ("error", exception)"""
        f: Future = Future()
        self.q.put((lambda: self._launch(groups), f))
        return f

    def iterate(self, gen, depth=2):
        """run a generator on the service thread, `depth` items ahead of the consumer at most -> an iterator of its items
        (an exception of the generator is raised where the consumer takes the next item)"""
        out: "queue.Queue" = queue.Queue(maxsize=depth)

        def put(x):
            while not self.closing:
                try:
                    out.put(x, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def job():
            try:
                for x in gen:
                    if not put(("item", x)):
                        return
                put(("end", None))
            except BaseException as e:
                put(("error", e))

        self.q.put((job, Future()))
        while True:
            kind, x = out.get()
            if kind == "end":
                return
            if kind == "error":
                raise x
            yield x

    def close(self):
        self.closing = True
        self.q.put(None)
        self.thread.join()

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                break
            fn, f = item
            try:
                f.set_result(fn())
            except BaseException as e:
                f.set_exception(e)

    # ---- the host route of one group (reads longer than the plan's look-ahead) ------------------------------------------
    def _open_handles(self):
        if self.handles is None:
            self.handles = (bamio.BamHandler(self.bam_path), bamio.FastaHandler(self.fasta_path))
        return self.handles

    def _host_group(self, g, data):
        bam, fasta = self._open_handles()
        p = g.plan
        fb = bamio.fill_batch_blocks(bam, fasta, g.ivs, p.coffset, p.next_coffset, p.isize, p.out_off, data,
                                     self.min_mapq, self.include_supplementary, self.downsample_rate, self.safe_bases,
                                     max_reads=self._read_limit())
        self.T["gpu_inflate_blocks_host"] += fb.blocks_host
        return fb

    def _error(self, g, k, row, blk_status, coffset):
        st, voff, d1, d2 = int(row[3]), int(row[4]), int(row[5]), int(row[6])
        if st == _ffi.PV_BAMDEC_BAD_BLOCK:
            msg = "BGZF block at offset %d: %s (corrupt file; GPU inflate)" % (
                int(coffset[d1]), _ffi.BGZF_STATUS_NAMES.get(int(blk_status[d1]), "status %d" % int(blk_status[d1])))
        elif st == _ffi.PV_BAMDEC_BAD_RECORD:
            msg = "corrupt BAM record (negative l_seq)" if d2 < 0 else "corrupt BAM record (fields need %d bytes, block_size %d)" % (d2, d1)
        elif st == _ffi.PV_BAMDEC_CIGAR_LONGER:
            msg = "CIGAR longer than SEQ in a BAM record"
        elif st == _ffi.PV_BAMDEC_BLOCK_SIZE:
            msg = "corrupt BAM record (block_size %d)" % d1
        elif st == _ffi.PV_BAMDEC_SEEK:
            msg = "seek failed in BAM"
        else:
            msg = "block or interval table rejected by the device (status %d)" % st
        return IOError("fill_batch: %s [interval %s:%d-%d, virtual offset %d; GPU decode]" % ((msg,) + tuple(g.ivs[k]) + (voff,)))

    def _scan(self, groups, per=None, ws_limit=None) -> _Scan:
        """H2D, inflate and pv_bam_scan_dev of these groups in one launch; per: record slots for every interval of each
        group (None: the safe rule); ws_limit: the scan is refused if its workspace would be larger -> the _Scan, counts
        on the host"""
        import torch
        T, ctx = self.T, self.ctx
        if per is None:
            per = [safe_slots(g.plan.out_bytes) for g in groups]
        sc = _Scan(groups, per)
        plans = [g.plan for g in groups]
        nb = sum(p.n_blocks for p in plans)
        N = sum(len(g.ivs) for g in groups)
        pay_bytes = sum(int(p.payload.size) for p in plans)
        out_bytes = sum(p.out_bytes for p in plans)
        n_chunks = sum(g.ivp.n_chunks for g in groups)
        ref_bytes = sum(int(r.size) for g in groups for r in g.refs)
        sizes = [("payload", pay_bytes), ("in_off", 8 * nb), ("out_off", 8 * nb), ("coffset", 8 * nb), ("next", 8 * nb),
                 ("clen", 4 * nb), ("isize", 4 * nb), ("crc", 4 * nb),
                 ("iv_rs", 8 * N), ("iv_re", 8 * N), ("iv_blk0", 8 * N), ("iv_blk1", 8 * N), ("iv_chunk_off", 8 * (N + 1)),
                 ("iv_rec_off", 8 * (N + 1)), ("chunk_beg", 8 * n_chunks), ("chunk_end", 8 * n_chunks), ("iv_tid", 4 * N),
                 ("iv_dropped", N), ("ref", ref_bytes)]
        offs, total = _stage(sizes)
        up = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        h = up.numpy()
        sz = dict(sizes)

        def view(k, dtype):
            return h[offs[k]:offs[k] + sz[k]].view(dtype)

        v64 = {k: view(k, np.int64) for k in ("in_off", "out_off", "coffset", "next", "iv_rs", "iv_re", "iv_blk0", "iv_blk1",
                                               "iv_chunk_off", "iv_rec_off", "chunk_beg", "chunk_end")}
        clen, isize, iv_tid = view("clen", np.int32), view("isize", np.int32), view("iv_tid", np.int32)
        crc, payload, dropped, ref = view("crc", np.uint32), view("payload", np.uint8), view("iv_dropped", np.uint8), view("ref", np.uint8)
        pb = ob = bi = ii = ci = slots = rb = 0
        first, ref_at = [], []          # per group (first block, first data byte, first interval); per interval its ref bytes' place
        v64["iv_chunk_off"][0] = 0
        v64["iv_rec_off"][0] = 0
        for g, per_iv in zip(groups, per):
            p, ivp, k, n = g.plan, g.ivp, g.plan.n_blocks, len(g.ivs)
            payload[pb:pb + p.payload.size] = p.payload
            v64["in_off"][bi:bi + k] = p.in_off + pb
            v64["out_off"][bi:bi + k] = p.out_off + ob
            v64["coffset"][bi:bi + k], v64["next"][bi:bi + k] = p.coffset, p.next_coffset
            clen[bi:bi + k], isize[bi:bi + k], crc[bi:bi + k] = p.clen, p.isize, p.crc
            v64["iv_rs"][ii:ii + n], v64["iv_re"][ii:ii + n], iv_tid[ii:ii + n] = ivp.rs, ivp.re, ivp.tid
            v64["iv_blk0"][ii:ii + n], v64["iv_blk1"][ii:ii + n] = bi, bi + k
            v64["iv_chunk_off"][ii + 1:ii + n + 1] = ivp.chunk_off[1:] + ci
            v64["chunk_beg"][ci:ci + ivp.n_chunks], v64["chunk_end"][ci:ci + ivp.n_chunks] = ivp.chunk_beg, ivp.chunk_end
            dropped[ii:ii + n] = ivp.dropped
            v64["iv_rec_off"][ii + 1:ii + n + 1] = slots + int(per_iv) * np.arange(1, n + 1, dtype=np.int64)
            slots += int(per_iv) * n
            for r in g.refs:
                ref[rb:rb + r.size] = r
                ref_at.append(rb)
                rb += int(r.size)
            first.append((bi, ob, ii))
            pb += int(p.payload.size); ob += p.out_bytes; bi += k; ii += n; ci += ivp.n_chunks
        ws_bytes = int(ctx.lib.pv_bam_decode_ws_bytes(N, slots))
        if ws_bytes < 0 or slots >= (1 << 31):
            raise _ffi.PepperHipError(_ffi.PV_ERR_LIMIT, "gpu_decode: too many record slots for one launch")
        ws_words = max(ws_bytes // 8 + 1, 1)
        if ws_limit is not None and 8 * ws_words > ws_limit:   # (decode_ws_bytes and the library disagree: never expected)
            raise _ffi.PepperHipError(_ffi.PV_ERR_LIMIT, "gpu_decode: a scan of %d intervals and %d slots needs %d bytes of "
                                      "workspace, over the budget of %d" % (N, slots, 8 * ws_words, ws_limit))
        if ws_limit is not None:   # (the polisher's form: scan_groups made these timers)
            self._account(sc, 8 * ws_words, 8 * ws_words + total + max(out_bytes, 8))
        counts_h = torch.empty((max(N, 1), 8), dtype=torch.int64, pin_memory=True)
        status_h = torch.empty(max(nb, 1), dtype=torch.int32, pin_memory=True)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        cin = _ffi.pv_bam_decode_in()
        with torch.cuda.stream(self.stream):
            d_up = torch.empty(total, dtype=torch.uint8, device=self.dev)
            d_out = torch.empty(max(out_bytes, 8), dtype=torch.uint8, device=self.dev)
            d_status = torch.empty(max(nb, 1), dtype=torch.int32, device=self.dev)
            d_c4 = torch.empty(4, dtype=torch.int64, device=self.dev)
            d_ws = torch.empty(ws_words, dtype=torch.int64, device=self.dev)
            d_counts = torch.zeros((max(N, 1), 8), dtype=torch.int64, device=self.dev)
            ev[0].record(self.stream)
            d_up.copy_(up, non_blocking=True)
            ev[1].record(self.stream)
            base = d_up.data_ptr()
            ctx.bgzf_inflate_dev(base + offs["payload"], pay_bytes, nb, base + offs["in_off"], base + offs["clen"],
                                 base + offs["isize"], base + offs["crc"], base + offs["out_off"], d_out.data_ptr(), out_bytes,
                                 d_status.data_ptr(), d_c4.data_ptr(), self.stream.cuda_stream)
            ev[2].record(self.stream)
            cin.data, cin.data_bytes, cin.n_blocks = d_out.data_ptr(), out_bytes, nb
            cin.coffset, cin.next_coffset, cin.out_off = base + offs["coffset"], base + offs["next"], base + offs["out_off"]
            cin.isize, cin.blk_status = base + offs["isize"], d_status.data_ptr()
            cin.n_intervals, cin.include_supplementary, cin.min_mapq = N, int(self.include_supplementary), self.min_mapq
            for k in ("iv_tid", "iv_rs", "iv_re", "iv_blk0", "iv_blk1", "iv_chunk_off", "chunk_beg", "chunk_end", "iv_dropped", "iv_rec_off"):
                setattr(cin, k, base + offs[k])
            cin.rec_slots, cin.n_chunks = slots, n_chunks
            ctx.bam_scan_dev(cin, d_ws.data_ptr(), d_ws.numel() * 8, d_counts.data_ptr(), self.stream.cuda_stream)
            ev[3].record(self.stream)
            counts_h.copy_(d_counts, non_blocking=True)
            status_h.copy_(d_status, non_blocking=True)
        self.stream.synchronize()
        T["gpu_inflate_h2d_ms"] += ev[0].elapsed_time(ev[1])
        T["gpu_inflate_kernel_ms"] += ev[1].elapsed_time(ev[2])
        T["gpu_decode_scan_ms"] += ev[2].elapsed_time(ev[3])
        T["gpu_inflate_launches"] += 1
        T["gpu_inflate_blocks"] += nb
        T["gpu_inflate_bytes"] += out_bytes
        T["gpu_decode_groups"] += len(groups)
        T["gpu_decode_h2d_bytes"] += total
        T["gpu_decode_d2h_bytes"] += counts_h.numel() * 8 + status_h.numel() * 4
        sc.cnt, sc.blk_status = counts_h.numpy(), status_h.numpy()
        T["gpu_decode_records"] += int(sc.cnt[:N, 7].sum())
        sc.first, sc.ref_at, sc.ref_base, sc.coffset = first, ref_at, offs["ref"], v64["coffset"].copy()
        sc.cin, sc.d_ws, sc.d_up, sc.d_out, sc.keep = cin, d_ws, d_up, d_out, (d_status, d_c4, d_counts)
        return sc

    def _account(self, sc, ws_bytes, all_bytes):
        """the scan's workspace, and all of its device buffers (workspace, uploaded tables and payloads, inflated bytes), count
        as live until the _Scan object goes away; the timers keep the largest single workspace and the largest live sums"""
        import weakref
        T, live = self.T, self.live
        live[0] += ws_bytes
        live[1] += all_bytes
        T["gpu_decode_ws_peak_bytes"] = max(T["gpu_decode_ws_peak_bytes"], ws_bytes)
        T["gpu_decode_ws_live_peak_bytes"] = max(T["gpu_decode_ws_live_peak_bytes"], live[0])
        T["gpu_decode_buffers_live_peak_bytes"] = max(T["gpu_decode_buffers_live_peak_bytes"], live[1])

        def gone():
            live[0] -= ws_bytes
            live[1] -= all_bytes
        weakref.finalize(sc, gone)

    def _kind(self, sc, gi):
        """group gi of the scan: "dev" (decoded on the device), "host" (the host route) or the exception to raise"""
        g, (b0, o0, i0) = sc.groups[gi], sc.first[gi]
        cnt, blk_status = sc.cnt, sc.blk_status
        for k in range(len(g.ivs)):
            st = int(cnt[i0 + k, 3])
            if st == _ffi.PV_BAMDEC_PAST_PLAN:
                # the host route parses this group's inflated bytes: as in gpu_inflate mode, any failed block of its plan
                # fails the group (the device only reports the blocks under records it walked before it stopped)
                bad = np.flatnonzero(blk_status[b0:b0 + g.plan.n_blocks] != _ffi.PV_BGZF_OK)
                if bad.size:
                    i = int(bad[0])
                    return IOError("BGZF block at offset %d: %s (corrupt file; GPU inflate)" % (
                        int(g.plan.coffset[i]), _ffi.BGZF_STATUS_NAMES.get(int(blk_status[b0 + i]), "status %d" % int(blk_status[b0 + i]))))
                return "host"
            if st != _ffi.PV_BAMDEC_OK:
                return self._error(g, k, cnt[i0 + k], blk_status, sc.coffset)
            if cnt[i0 + k, 0] > 0 and g.ref_err[k] is not None:
                return g.ref_err[k]
        return "dev"

    def _launch(self, groups):
        import torch
        T = self.T
        sc = self._scan(groups)
        t_host = time.perf_counter()
        d_out = sc.d_out
        # every group: decoded on the device, or the host route, or an error - in the reader's order
        kinds = [self._kind(sc, gi) for gi in range(len(groups))]
        items, fills, run = [], [], []

        def close_run():
            if run:
                fl = self._fill(sc, run)
                if fl is not None:
                    fills.append(fl)
                    items.append(("dev", fl[0]))
                del run[:]

        for gi, (g, kind) in enumerate(zip(groups, kinds)):
            if kind == "dev":
                run.append(gi)
                continue
            close_run()
            if kind == "host":
                T["gpu_decode_groups_host"] += 1
                b0, o0, i0 = sc.first[gi]
                down = torch.empty(max(g.plan.out_bytes, 1), dtype=torch.uint8, pin_memory=True)
                with torch.cuda.stream(self.stream):
                    down.copy_(d_out[o0:o0 + max(g.plan.out_bytes, 1)] if g.plan.out_bytes else d_out[:1], non_blocking=True)
                self.stream.synchronize()
                T["gpu_decode_d2h_bytes"] += g.plan.out_bytes
                try:
                    items.append(("host", self._host_group(g, down.numpy()[:g.plan.out_bytes])))
                except IOError as e:
                    items.append(("error", e))
            else:
                items.append(("error", kind))
        close_run()
        self._finish_fills(fills)
        T["gpu_decode_host_s"] += time.perf_counter() - t_host
        return items

    def _finish_fills(self, fills):
        """wait for the fills and take their totals (bases, CIGAR words, status; the longest read where it was asked for)"""
        if not fills:
            return
        T = self.T
        self.stream.synchronize()
        for db, totals_h, e0, e1 in fills:
            T["gpu_decode_fill_ms"] += e0.elapsed_time(e1)
            n_reads, n_bases, n_cigar, st = (int(x) for x in totals_h[:4].tolist())
            if st != _ffi.PV_OK or n_reads != db.n_reads:
                raise _ffi.PepperHipError(st or _ffi.PV_ERR_STATE, "gpu_decode: the fill reported status %d" % st)
            db.n_bases, db.n_cigar = n_bases, n_cigar
            if totals_h.numel() > 4:
                db.qmax = int(totals_h[4])
            T["gpu_decode_d2h_bytes"] += 8 * totals_h.numel()

    def _fill(self, sc, run, pick=None, detach=False):
        """the fill of consecutive device-decoded groups of one scan (run: their indices; pick: the (group index, interval)
        pairs to take, in order, instead of every interval of `run`) -> (DecodedBatch, pinned totals, two timing events)
        or None when no region is left. detach: the batch takes a copy of its reference bytes and keeps no buffer of the scan
        alive (the polisher's form: the scan goes away once its regions are filled)"""
        import torch
        groups, first, cnt, cin, d_ws, d_up, ref_base, ref_at = (sc.groups, sc.first, sc.cnt, sc.cin, sc.d_ws, sc.d_up,
                                                                  sc.ref_base, sc.ref_at)
        ivs_all, reg = [], []   # reg: (launch interval, index in ivs_all, reads, kept indices or None)
        if pick is None:
            pick = [(gi, k) for gi in run for k in range(len(groups[gi].ivs))]
        max_reads = self._read_limit()
        for gi, k in pick:
            g, i0 = groups[gi], first[gi][2]
            iv = g.ivs[k]
            n = int(cnt[i0 + k, 0])
            got = int(g.refs[k].size)
            keep = None
            if n > 0:
                limit = max(int(min(float(max_reads), self.downsample_rate * n)), 0)
                if n > limit:
                    keep = bamio.reservoir_indices(n, self.downsample_rate, max_reads, bamio.RANDOM_SEED)
            n_out = n if keep is None else len(keep)
            if n_out > 0 and got > 0:
                reg.append((i0 + k, len(ivs_all), n, keep, n_out, iv, got, int(g.ivp.rs[k])))
            ivs_all.append(iv)
        if not reg:
            return None
        G = len(reg)
        n_out = np.array([r[4] for r in reg], np.int64)
        got = np.array([r[6] for r in reg], np.int64)
        rs = np.array([r[7] for r in reg], np.int64)
        re_c = rs + got - 1
        read_off = np.concatenate([[0], np.cumsum(n_out)]).astype(np.int64)
        ref_off = np.concatenate([[0], np.cumsum(got)]).astype(np.int64)
        sel = [r[3] for r in reg if r[3] is not None]
        sel_off, o = np.full(G, -1, np.int64), 0
        for j, r in enumerate(reg):
            if r[3] is not None:
                sel_off[j] = o
                o += len(r[3])
        small = dict(ref_start=rs, ref_end=re_c, cand_start=np.array([r[5][1] for r in reg], np.int64),
                     cand_end=np.minimum(np.array([r[5][2] for r in reg], np.int64), re_c), ref_off=ref_off, read_off=read_off,
                     sel_off=sel_off, sel=np.concatenate(sel).astype(np.int64) if sel else np.zeros(1, np.int64),
                     reg_iv=np.array([r[0] for r in reg], np.int32))
        offs, total = _stage([(k, v.nbytes) for k, v in small.items()])
        up = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        for k, v in small.items():
            up.numpy()[offs[k]:offs[k] + v.nbytes] = v.view(np.uint8)
        n_reads = int(read_off[-1])
        base_cap = int(sum(int(cnt[r[0], 1]) for r in reg))
        cigar_cap = int(sum(int(cnt[r[0], 2]) for r in reg))
        n_tot = 5 if self.want_qmax else 4   # {reads, bases, CIGAR words, status} and, for the realigner, the longest read
        totals_h = torch.zeros(n_tot, dtype=torch.int64, pin_memory=True)
        with torch.cuda.stream(self.stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            d_small = torch.empty(total, dtype=torch.uint8, device=self.dev)
            d_small.copy_(up, non_blocking=True)
            t = {k: d_small[offs[k]:offs[k] + small[k].nbytes].view(torch.int64)
                 for k in ("ref_start", "ref_end", "cand_start", "cand_end", "ref_off", "read_off")}
            # the reference bytes went up with the plan; intervals that dropped out leave holes, closed here on the device
            pieces = [(ref_base + ref_at[r[0]], r[6]) for r in reg]
            if all(pieces[j][0] + pieces[j][1] == pieces[j + 1][0] for j in range(G - 1)):
                t["ref"] = d_up[pieces[0][0]:pieces[-1][0] + pieces[-1][1]]
                if detach:
                    t["ref"] = t["ref"].clone()
            else:
                t["ref"] = torch.cat([d_up[a:a + n] for a, n in pieces])
            t["read_pos"] = torch.empty(n_reads, dtype=torch.int64, device=self.dev)
            t["read_flags"] = torch.empty(n_reads, dtype=torch.uint8, device=self.dev)
            t["read_mapq"] = torch.empty(n_reads, dtype=torch.uint8, device=self.dev)
            t["read_hp"] = torch.empty(n_reads, dtype=torch.int32, device=self.dev)
            t["base_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=self.dev)
            t["cigar_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=self.dev)
            t["bases"] = torch.empty(max(base_cap, 1), dtype=torch.uint8, device=self.dev)
            t["quals"] = torch.empty(max(base_cap, 1), dtype=torch.uint8, device=self.dev)
            t["cigar"] = torch.empty(max(cigar_cap, 1), dtype=torch.int32, device=self.dev)
            d_totals = torch.zeros(n_tot, dtype=torch.int64, device=self.dev)
            event = torch.cuda.Event()
            db = DecodedBatch(t, G, ivs_all, np.array([r[1] for r in reg], np.int64), np.array([r[2] for r in reg], np.int64),
                              n_reads, int(ref_off[-1]), int(got.max()), event)
            sb = d_small.data_ptr()
            self.ctx.bam_fill_dev(cin, d_ws.data_ptr(), d_ws.numel() * 8, G, sb + offs["reg_iv"], sb + offs["read_off"],
                                  sb + offs["sel_off"], sb + offs["sel"], int(o), n_reads, base_cap, cigar_cap, db.c,
                                  t["read_hp"].data_ptr(), d_totals.data_ptr(), self.stream.cuda_stream)
            e1.record(self.stream)
            if self.want_qmax and n_reads:   # the longest read, for the realigner: a reduction behind the fill, no kernel of ours
                d_totals[4] = (t["base_off"][1:] - t["base_off"][:-1]).max()
            totals_h.copy_(d_totals, non_blocking=True)
            event.record(self.stream)
        t["_small"] = d_small
        if not detach:
            t["_up"] = d_up
        self.T["gpu_decode_h2d_bytes"] += total
        return db, totals_h, e0, e1

    # ---- the polisher's form: scans under a workspace budget, launches cut as the host path cuts them -------------------
    def _host_regions(self, g):
        """the polisher's host route of one group: polish_summary.region_from_files per region (None: no reads)"""
        from .polish_summary import region_from_files
        bam, fasta = self._open_handles()
        return [region_from_files(bam, fasta, c, s, e, realign=self.realign) for c, s, e in g.ivs]

    def _host_scan(self, g):
        self.T["gpu_decode_groups_host"] += 1
        regions = self._host_regions(g)
        return GroupScan(g, "host", [0 if r is None else len(r.reads) for r in regions], g, regions=regions)

    def _min_record_bytes(self):
        if self.adaptive_slots and self.density > 0.0:
            return max(REC_MIN_BYTES, int(1.0 / (4.0 * self.density)))
        return self.min_record_bytes

    def scan_groups(self, planned):
        """planned groups, in order -> a generator of a GroupScan for each, in order, with a None behind the groups of every
        scan (compose_launches: their regions can be filled now). One scan runs at a time and only when the consumer asks
        for its first group, so with a consumer that fills at every None one scan's buffers are live at a time.
        Scans are packed by plan_launches under the workspace budget. A scan in which a group ran out of slots (fewer than
        the safe rule were given) is dropped and its groups are scanned again, once, those groups with the safe rule; a
        group over the budget on its own and a group that reports PV_BAMDEC_PAST_PLAN are read on the host."""
        T = self.T
        for k in ("gpu_decode_slot_retries", "gpu_decode_groups_over_budget", "gpu_decode_ws_peak_bytes",
                  "gpu_decode_ws_live_peak_bytes", "gpu_decode_buffers_live_peak_bytes"):
            T.setdefault(k, 0)
        sizes = [(len(g.ivs), g.plan.out_bytes) for g in planned]

        def short_groups(sc):
            out = []
            for j, g in enumerate(sc.groups):
                i0 = sc.first[j][2]
                if sc.per[j] < safe_slots(g.plan.out_bytes) and bool((sc.cnt[i0:i0 + len(g.ivs), 3] == _ffi.PV_BAMDEC_BAD_TABLE).any()):
                    out.append(j)
            return out

        def run(entries, index, retry):
            for kind, gis, per in entries:
                if kind == "host":
                    T["gpu_decode_groups_over_budget"] += 1
                    yield self._host_scan(planned[index[gis[0]]])
                    continue
                sc = self._scan([planned[index[gi]] for gi in gis], per, self.ws_budget)
                short = [] if retry else short_groups(sc)
                if short:   # (PV_BAMDEC_BAD_TABLE under the safe rule is an error below: the second attempt failed)
                    del sc
                    T["gpu_decode_slot_retries"] += 1
                    mine = [index[gi] for gi in gis]
                    rule = [REC_MIN_BYTES if j in short else self._min_record_bytes() for j in range(len(mine))]
                    yield from run(plan_launches([sizes[i] for i in mine], self.ws_budget, rule), mine, True)
                    continue
                for j, g in enumerate(sc.groups):
                    i0 = sc.first[j][2]
                    rows = sc.cnt[i0:i0 + len(g.ivs)]
                    if g.plan.out_bytes:
                        self.density = max(self.density, float(rows[:, 7].max(initial=0)) / g.plan.out_bytes)
                    kind_g = self._kind(sc, j)
                    yield self._host_scan(g) if kind_g == "host" else GroupScan(g, kind_g, rows[:, 0].copy(), sc, j)
                del sc
                yield None

        return run(plan_launches(sizes, self.ws_budget, self._min_record_bytes()), list(range(len(planned))), False)

    def realize(self, launch):
        """parts of compose_launches -> the parts as the chain takes them: ("dev", DecodedBatch, windows, works) |
        ("host", batch.RegionBatch, windows, works); windows None unless the groups were planned with them. A decoded batch
        owns all it needs: the scan it was filled from can go away."""
        from .batch import pack_regions
        parts, fills = [], []
        for kind, key, regs in launch:
            works = [gs.group.works[k] if gs.group.works else gs.group.ivs[k] for gs, k in regs]
            if kind == "host":
                rs = [gs.regions[k] for gs, k in regs]
                parts.append(("host", pack_regions(rs), [r.window for r in rs] if self.realign else None, works))
                continue
            fl = self._fill(key, None, [(gs.gi, k) for gs, k in regs], detach=True)
            fills.append(fl)
            win = [gs.group.windows[k] for gs, k in regs] if regs[0][0].group.windows is not None else None
            parts.append(("dev", fl[0], win, works))
        self._finish_fills(fills)
        return parts


def decoded_launches(dec, planned, per_launch, scan_regions=None):
    """the polisher's launches from planned groups (an iterator, in work order): groups are handed to the decoder's
    scan_groups scan_regions regions at a time (default: one launch's worth), cut into launches by compose_launches, and
    every part is realized (filled) as soon as it is complete - before the next scan runs. dec: a GpuDecoder, or anything
    with its scan_groups and realize (CPU tests pass a stub). A generator: GpuDecoder.iterate runs it on the service thread.
    Adds the seconds spent in the decoder to the timer decode_s."""
    want = int(scan_regions or per_launch)
    T = getattr(dec, "T", {})

    def clock(t0):
        T["decode_s"] = T.get("decode_s", 0.0) + time.perf_counter() - t0

    def scanned(buf):
        it = iter(dec.scan_groups(buf))
        while True:
            t0 = time.perf_counter()
            try:
                gs = next(it)
            except StopIteration:
                clock(t0)
                break
            clock(t0)
            yield gs
        yield None

    def scans():
        buf, n = [], 0
        for g in planned:
            buf.append(g)
            n += len(g.ivs)
            if n >= want:
                yield from scanned(buf)
                buf, n = [], 0
        if buf:
            yield from scanned(buf)

    def on_part(part):
        t0 = time.perf_counter()
        r = dec.realize([part])[0]
        clock(t0)
        return r

    return compose_launches(scans(), per_launch, on_part)


def decode_groups(ctx, bam_path, fasta_path, groups_of_intervals, min_mapq=5, include_supplementary=False, downsample_rate=1.0,
                  safe_bases=100, T=None, max_reads=None):
    """One launch over several reader groups (lists of (contig, start, end)), for tests and tools -> the list of items
    GpuDecoder.submit gives: ("dev", DecodedBatch) | ("host", FilledBatch) | ("error", exception), and the timers in T."""
    T = T if T is not None else {}
    bam, fasta = bamio.BamHandler(bam_path), bamio.FastaHandler(fasta_path)
    dec = GpuDecoder(ctx, bam_path, fasta_path, min_mapq, include_supplementary, downsample_rate, safe_bases, T, max_reads=max_reads)
    try:
        planned = [PlannedGroup(bam, fasta, ivs, safe_bases) for ivs in groups_of_intervals]
        return dec.submit(planned).result()
    finally:
        dec.close()
        bam.close()
        fasta.close()


def decoded_batches(ctx, bam_path, fasta_path, groups, reads_per_call, n_thr, min_mapq, include_supplementary, downsample_rate,
                    safe_bases, T, merge, max_reads=None):
    """region_batches' generator in gpu_decode mode: (DecodedBatch, intervals of its regions) pairs in the default mode's
    order; a group that took the host route comes as the default mode's host batch (a list of parts when merge is False)."""
    T.setdefault("gpu_decode_plan_cpu_s", 0.0)    # reader threads: CPU seconds (time.thread_time) planning blocks + fetching FASTA
    T.setdefault("gpu_decode_plan_wall_s", 0.0)   # ... and their wall seconds
    dec = GpuDecoder(ctx, bam_path, fasta_path, min_mapq, include_supplementary, downsample_rate, safe_bases, T, max_reads=max_reads)
    tls = threading.local()

    def plan_group(ivs):
        if not hasattr(tls, "h"):
            tls.h = (bamio.BamHandler(bam_path), bamio.FastaHandler(fasta_path))
        return PlannedGroup(tls.h[0], tls.h[1], ivs, safe_bases)

    pool = ThreadPoolExecutor(n_thr)
    pending, jobs = deque(), deque()
    nxt = 0
    ahead = 2 * reads_per_call + n_thr + 2
    while nxt < len(groups) and len(pending) < ahead:
        pending.append(pool.submit(plan_group, groups[nxt]))
        nxt += 1

    def batches():
        nonlocal nxt
        try:
            while pending or jobs:
                t0 = time.perf_counter()
                while pending and len(jobs) < 2:   # one call's worth being decoded while the consumer works on the one before
                    planned = []
                    while pending and len(planned) < reads_per_call and (not planned or pending[0].done()):
                        planned.append(pending.popleft().result())
                        if nxt < len(groups):
                            pending.append(pool.submit(plan_group, groups[nxt]))
                            nxt += 1
                    for g in planned:
                        T["gpu_decode_plan_cpu_s"] += g.cpu_plan
                        T["gpu_decode_plan_wall_s"] += g.t_plan
                    jobs.append(dec.submit(planned))
                items = jobs.popleft().result()
                T["reader_stall_s"] += time.perf_counter() - t0
                for kind, x in items:
                    if kind == "error":
                        raise x
                    if kind == "dev":
                        T["bases"] += x.n_bases
                        T["reads"] += x.n_reads
                        yield x, [x.intervals[int(i)] for i in x.interval_index]
                    else:
                        names = [x.intervals[int(i)] for i in x.interval_index]
                        if x.batch.n_regions:
                            T["bases"] += x.batch.n_bases
                            T["reads"] += x.batch.n_reads
                            yield (x.batch if merge else [x.batch]), names
                        x.close()
                del items
        finally:
            for f in pending:
                f.cancel()
            pool.shutdown(wait=True)
            for j in jobs:
                try:
                    j.result()
                except BaseException:
                    pass
            dec.close()
    return batches()


def summarize_decoded(ctx, db: DecodedBatch, params, use_hp: bool = False):
    """the device-resident builder on a DecodedBatch, read back as batch.SummaryOut (what Context.summarize[_hp] returns for
    a host batch): make_images' path outside the fused pipeline"""
    import torch
    from .batch import SummaryOut
    from .device import DeviceOut
    dev = "cuda:%d" % ctx.device_id
    db.wait_on(ctx)
    cap = max(4096, 1024 * db.n_regions)
    scap = 16 * cap
    while True:
        images = torch.zeros((cap, _ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES), dtype=torch.int8, device=dev) if use_hp else None
        dout = DeviceOut(cap, scap, dev, images)
        torch.cuda.synchronize()
        if use_hp:
            ctx.summarize_hp_dev(db, params, dout)
        else:
            ctx.summarize_dev(db, params, dout)
        ctx.synchronize(check=False)
        n_out, str_bytes, status = (int(v) for v in dout.counts[:3].tolist())
        if status != _ffi.PV_OK:
            raise _ffi.PepperHipError(status, "image builder reported status %d" % status)
        if n_out <= cap and str_bytes <= scap:
            break
        cap, scap = max(cap, n_out), max(scap, str_bytes)
    off = dout.cand_off[:n_out + 1].cpu().numpy()
    raw = dout.cand_str[:int(off[-1]) if n_out else 0].cpu().numpy().tobytes()
    cands = [raw[int(off[i]):int(off[i + 1])].decode("latin-1") for i in range(n_out)]
    return SummaryOut(dout.region[:n_out].cpu().numpy(), dout.position[:n_out].cpu().numpy(), dout.depth[:n_out].cpu().numpy(),
                      dout.cand_freq[:n_out].cpu().numpy(), dout.images[:n_out].cpu().numpy(), cands, None)
