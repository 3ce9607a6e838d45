"""Thin Python handle on a pv_ctx (one HIP device + stream + workspace) of the C-ABI.

All compute happens in csrc/libpepper_hip.so; this module only marshals numpy arrays / device
pointers. There is no CPU fallback: constructing a Context without a HIP device raises.
"""
import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from .batch import OutBuffers, Params, RegionBatch, SummaryOut


def _dir_struct(w, prefix, suffix, keep):
    d = _ffi.pv_rnn_dir()
    for field, key in (("w_ih", "weight_ih_l0"), ("w_hh", "weight_hh_l0"), ("b_ih", "bias_ih_l0"), ("b_hh", "bias_hh_l0")):
        a = np.ascontiguousarray(w["%s.%s%s" % (prefix, key, suffix)], dtype=np.float32)
        keep.append(a)
        setattr(d, field, a.ctypes.data)
    return d


class _GraphCapture:
    def __init__(self, ctx, stream):
        self.ctx, self.stream, self.handle = ctx, int(stream or ctx.stream), None

    def __enter__(self):
        _ffi.check(self.ctx.lib.pv_graph_begin(self.ctx.handle, self.stream))
        return self

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        rc = self.ctx.lib.pv_graph_end(self.ctx.handle, C.byref(h))
        if et is None:
            _ffi.check(rc)
            self.handle = h
        elif rc == 0:
            self.ctx.lib.pv_graph_destroy(h)
        return False

    def launch(self, stream: int = 0):
        _ffi.check(self.ctx.lib.pv_graph_launch(self.handle, int(stream or self.stream)))

    def close(self):
        if self.handle:
            self.ctx.lib.pv_graph_destroy(self.handle)
            self.handle = None


class Context:
    """pv_create / pv_destroy with the reference operators as methods."""

    def __init__(self, device_id: int = 0):
        self.lib = _ffi.load()
        self.handle = self.lib.pv_create(int(device_id))
        if not self.handle:
            msg = self.lib.pv_last_error()
            raise _ffi.PepperHipError(_ffi.PV_ERR_NO_DEVICE, msg.decode() if msg else "pv_create failed")
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pv_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return int(self.lib.pv_stream(self.handle) or 0)

    def synchronize(self, check: bool = True):
        """wait for the context's stream. check=True also asks whether a poll of the split RNN forms gave up since the last
        synchronisation point (the outputs of such calls are poisoned on the device: NaN / label 255) and raises
        PepperHipError(PV_ERR_STATE) if so - callers of the asynchronous *_dev forms get the verdict where they wait."""
        _ffi.check(self.lib.pv_synchronize(self.handle))
        if check:
            n = self.exchange_timeouts()
            if n:
                raise _ffi.PepperHipError(_ffi.PV_ERR_STATE, "%d exchange polls of a split RNN form timed out: the outputs of the "
                                          "calls since the last synchronisation are poisoned (set_option('shared_device', 1) "
                                          "on a GPU shared with other work)" % n)

    def set_option(self, name: str, value: int):
        """kernel-form options of this context (include/pepper_hip.h, pv_set_option)"""
        _ffi.check(self.lib.pv_set_option(self.handle, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int()
        _ffi.check(self.lib.pv_get_option(self.handle, name.encode(), C.byref(v)))
        return int(v.value)

    def graph_capture(self, stream: int = 0):
        """context manager: the *_dev calls made inside (with this stream) are recorded into a hipGraph instead of run;
        `with ctx.graph_capture(s) as g: ...` then `g.launch()` per batch after refilling the same input buffers.
        Run the same calls once eagerly before (the workspace cannot grow inside a capture)."""
        return _GraphCapture(self, stream)

    def exchange_timeouts(self) -> int:
        """polls of the split kernel forms that gave up since the last call (synchronises; 0 = all results good)"""
        n = int(self.lib.pv_rnn_exchange_timeouts(self.handle))
        if n < 0:
            _ffi.check(n)
        return n

    def workspace_bytes(self) -> int:
        return int(self.lib.pv_workspace_bytes(self.handle))

    # ---- image builder ---------------------------------------------------------------------------
    def summarize(self, batch: RegionBatch, params: Params, want_i32: bool = False,
                  capacity: Optional[int] = None, str_capacity: Optional[int] = None) -> SummaryOut:
        """RegionalSummaryGenerator.generate_summary for every region of the batch (host buffers)."""
        cin, cp = batch.as_c(), params.as_c()
        cap = capacity or max(1024, batch.n_regions * 1024)
        scap = str_capacity or cap * 8
        for _ in range(3):
            ob = OutBuffers(cap, scap, want_i32)
            rc = self.lib.pv_summarize_regions(self.handle, C.byref(cin), C.byref(cp), C.byref(ob.c))
            if rc == _ffi.PV_ERR_CAPACITY:
                cap, scap = max(cap, int(ob.c.n_out)), max(scap, int(ob.c.str_bytes))
                continue
            _ffi.check(rc)
            return ob.result()
        _ffi.check(rc)

    def summarize_hp(self, batch: RegionBatch, params: Params, want_i32: bool = False,
                     capacity: Optional[int] = None, str_capacity: Optional[int] = None) -> SummaryOut:
        """RegionalSummaryGeneratorHP.generate_summary (haplotag-aware, 48 planes x 21 rows) for every region of the
        batch; batch.read_hp carries type_read::hp_tag (None = untagged reads); params must carry window 20 / 48 features
        (batch.hp_params)."""
        from .batch import hp_pointer
        cin, cp = batch.as_c(), params.as_c()
        cap = capacity or max(1024, batch.n_regions * 1024)
        scap = str_capacity or cap * 8
        for _ in range(3):
            ob = OutBuffers(cap, scap, want_i32, _ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES)
            rc = self.lib.pv_summarize_regions_hp(self.handle, C.byref(cin), hp_pointer(batch), C.byref(cp), C.byref(ob.c))
            if rc == _ffi.PV_ERR_CAPACITY:
                cap, scap = max(cap, int(ob.c.n_out)), max(scap, int(ob.c.str_bytes))
                continue
            _ffi.check(rc)
            return ob.result()
        _ffi.check(rc)

    # ---- RNN ------------------------------------------------------------------------------------------
    def load_p1(self, weights: dict, dtype: int = _ffi.PV_DTYPE_F32):
        """weights: state_dict of the pepper_variant TransducerGRU as numpy arrays (ModelHander.py:18-44)."""
        keep = []
        w = _ffi.pv_weights_p1()
        for d, suffix in enumerate(("", "_reverse")):
            w.encoder[d] = _dir_struct(weights, "encoder", suffix, keep)
            w.decoder[d] = _dir_struct(weights, "decoder", suffix, keep)
        for i in range(5):
            a = np.ascontiguousarray(weights["linear_%d.weight" % (i + 1)], dtype=np.float32)
            b = np.ascontiguousarray(weights["linear_%d.bias" % (i + 1)], dtype=np.float32)
            keep += [a, b]
            w.linear_w[i], w.linear_b[i] = a.ctypes.data, b.ctypes.data
        a = np.ascontiguousarray(weights["output_layer_type.weight"], dtype=np.float32)
        b = np.ascontiguousarray(weights["output_layer_type.bias"], dtype=np.float32)
        keep += [a, b]
        w.out_w, w.out_b = a.ctypes.data, b.ctypes.data
        _ffi.check(self.lib.pv_rnn_load_p1(self.handle, C.byref(w), int(dtype)))

    def forward_p1(self, images: np.ndarray, taps: bool = False):
        """images int8 [B,33,26] -> probs float32 [B,3] (+ encoder/decoder outputs when taps=True)."""
        x = np.ascontiguousarray(images, dtype=np.int8)
        assert x.ndim == 3 and x.shape[1:] == (33, 26), x.shape
        B = x.shape[0]
        probs = np.zeros((B, 3), np.float32)
        if not taps:
            _ffi.check(self.lib.pv_rnn_forward_p1(self.handle, x.ctypes.data, B, probs.ctypes.data))
            return probs
        enc = np.zeros((B, 33, 512), np.float32)
        dec = np.zeros((B, 33, 512), np.float32)
        _ffi.check(self.lib.pv_rnn_forward_p1_debug(self.handle, x.ctypes.data, B, probs.ctypes.data,
                                                    enc.ctypes.data, dec.ctypes.data))
        return probs, enc, dec

    def forward_p1_dev(self, d_images_ptr: int, B: int, d_probs_ptr: int, stream: int = 0):
        """device pointers in, asynchronous on `stream` (0 = the context's stream)."""
        _ffi.check(self.lib.pv_rnn_forward_p1_dev(self.handle, d_images_ptr, int(B), d_probs_ptr, stream or None))

    def load_p2(self, weights: dict, dtype: int = _ffi.PV_DTYPE_F32):
        keep = []
        w = _ffi.pv_weights_p2()
        for d, suffix in enumerate(("", "_reverse")):
            w.encoder[d] = _dir_struct(weights, "gru_encoder", suffix, keep)
            w.decoder[d] = _dir_struct(weights, "gru_decoder", suffix, keep)
        a = np.ascontiguousarray(weights["dense1.weight"], dtype=np.float32)
        b = np.ascontiguousarray(weights["dense1.bias"], dtype=np.float32)
        keep += [a, b]
        w.dense_w, w.dense_b = a.ctypes.data, b.ctypes.data
        _ffi.check(self.lib.pv_rnn_load_p2(self.handle, C.byref(w), int(dtype)))

    def forward_p2(self, images: np.ndarray, want_acc: bool = False):
        """images uint8 [B,1000,10] -> labels uint8 [B,1000] (+ accumulated softmax [B,1000,5])."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        assert x.ndim == 3 and x.shape[1:] == (1000, 10), x.shape
        B = x.shape[0]
        labels = np.zeros((B, 1000), np.uint8)
        acc = np.zeros((B, 1000, 5), np.float32) if want_acc else None
        _ffi.check(self.lib.pv_rnn_forward_p2(self.handle, x.ctypes.data, B, labels.ctypes.data,
                                              None if acc is None else acc.ctypes.data))
        return (labels, acc) if want_acc else labels

    def forward_p2_dev(self, d_images: int, B: int, d_labels: int, d_acc: int = 0, stream: int = 0):
        """asynchronous; device pointers: images uint8 [B,1000,10] -> labels uint8 [B,1000] (+ acc float [B,1000,5])."""
        _ffi.check(self.lib.pv_rnn_forward_p2_dev(self.handle, d_images, int(B), d_labels, d_acc or None, stream or None))

    def forward_p2_window(self, images: np.ndarray, hidden: Optional[np.ndarray] = None):
        """TransducerGRU.forward(x, hidden): images uint8 [B,100,10], hidden [B,2,128] or None -> (logits [B,100,5], hidden [B,2,128])"""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        assert x.ndim == 3 and x.shape[1:] == (100, 10), x.shape
        B = x.shape[0]
        h_in = None if hidden is None else np.ascontiguousarray(hidden, dtype=np.float32)
        assert h_in is None or h_in.shape == (B, 2, 128)
        logits = np.zeros((B, 100, 5), np.float32)
        h_out = np.zeros((B, 2, 128), np.float32)
        _ffi.check(self.lib.pv_rnn_forward_p2_window(self.handle, x.ctypes.data, None if h_in is None else h_in.ctypes.data, B,
                                                     logits.ctypes.data, h_out.ctypes.data))
        return logits, h_out

    # ---- device-resident forms (the fused pipeline / benchmark) -----------------------------------------
    def summarize_dev(self, dbatch: "DeviceBatch", params: Params, dout: "DeviceOut", stream: int = 0):
        """asynchronous; every array lives in HBM (see device.py). Counters land in dout.counts."""
        cp = params.as_c()
        _ffi.check(self.lib.pv_summarize_regions_dev(
            self.handle, C.byref(dbatch.c), C.byref(cp), dbatch.n_reads, dbatch.n_bases, dbatch.n_cigar,
            dbatch.n_ref_bytes, dbatch.max_region_len, C.byref(dout.c), dout.counts.data_ptr(), stream or None))

    def upload_batch(self, batch: RegionBatch, stream: int = 0):
        """host batch -> the context's workspace (pv_upload_batch); returns (pv_batch_in with device pointers, totals) for
        summarize_uploaded. Valid until the next upload on this context."""
        cin = batch.as_c()
        dev = _ffi.pv_batch_in()
        totals = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_upload_batch(self.handle, C.byref(cin), C.byref(dev), totals, stream or None))
        return dev, [int(v) for v in totals], cin   # cin keeps the host arrays referenced until the copies are done

    def upload_batches(self, batches, stream: int = 0):
        """several host batches (e.g. one per interval) laid end to end on the device without a host-side concatenation
        (pv_upload_batches); same return value as upload_batch"""
        cins = [b.as_c() for b in batches if b.n_regions]
        arr = (C.POINTER(_ffi.pv_batch_in) * max(len(cins), 1))(*[C.pointer(c) for c in cins])
        dev = _ffi.pv_batch_in()
        totals = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_upload_batches(self.handle, len(cins), arr, C.byref(dev), totals, stream or None))
        return dev, [int(v) for v in totals], (cins, arr)

    def summarize_uploaded(self, uploaded, params: Params, dout: "DeviceOut", max_region_len: int = 0, stream: int = 0):
        """the device-resident builder on a batch staged with upload_batch; counters land in dout.counts"""
        dev, (n_reads, n_bases, n_cigar, n_ref), _ = uploaded
        cp = params.as_c()
        _ffi.check(self.lib.pv_summarize_regions_dev(self.handle, C.byref(dev), C.byref(cp), n_reads, n_bases, n_cigar, n_ref,
                                                     int(max_region_len), C.byref(dout.c), dout.counts.data_ptr(), stream or None))

    def summarize_hp_dev(self, dbatch: "DeviceBatch", params: Params, dout: "DeviceOut", stream: int = 0):
        """asynchronous, device-resident haplotag-aware builder: dout.images must be an int8 [capacity,21,48] tensor"""
        cp = params.as_c()
        assert tuple(dout.images.shape[1:]) == (_ffi.PV_HP_WINDOW_ROWS, _ffi.PV_HP_FEATURES), dout.images.shape
        _ffi.check(self.lib.pv_summarize_regions_hp_dev(
            self.handle, C.byref(dbatch.c), None if dbatch.read_hp is None else dbatch.read_hp.data_ptr(), C.byref(cp),
            dbatch.n_reads, dbatch.n_bases, dbatch.n_cigar, dbatch.n_ref_bytes, C.byref(dout.c), dout.counts.data_ptr(),
            stream or None))

    def polish_summarize(self, batch: RegionBatch, seq_length: int = 1000, seq_overlap: int = 50, want_flat: bool = False,
                         want_depth: bool = False, want_counts: bool = False):
        """Polisher (P2) SummaryGenerator.generate_summary + chunk_images for a batch (host buffers), see polish_summary.py."""
        from .polish_summary import polish_summarize
        return polish_summarize(self, batch, seq_length, seq_overlap, want_flat, want_depth, want_counts)

    def polish_summarize_dev(self, dbatch: "DeviceBatch", dout: "DevicePolishOut", stream: int = 0):
        """asynchronous, device-resident: chunks land in dout.images ([capacity, seq_length, 10] uint8 in HBM), ready
        for forward_p2_dev; counters {n_chunks, n_rows, status, insert rows} in dout.counts."""
        _ffi.check(self.lib.pv_polish_summarize_regions_dev(
            self.handle, C.byref(dbatch.c), dbatch.n_reads, dbatch.n_bases, dbatch.n_cigar, dbatch.n_ref_bytes,
            dout.seq_length, dout.seq_overlap, C.byref(dout.c), dout.counts.data_ptr(), stream or None))

    def polish_realign(self, batch: RegionBatch, win_off: np.ndarray, win: np.ndarray, cigar_capacity: int = None):
        """the polisher's read realignment (pv_polish_realign, host buffers) -> realign.RealignResult; see realign.py"""
        from .realign import realign
        return realign(self, batch, win_off, win, cigar_capacity)

    def polish_realign_dev(self, dbatch: "DeviceBatch", d_win_off: int, d_win: int, max_query_len: int, dout, stream: int = 0):
        """asynchronous, device-resident realignment (pv_polish_realign_dev) into a realign.DeviceRealignOut; counters
        {n_cigar, status, realigned, dropped} in dout.counts"""
        _ffi.check(self.lib.pv_polish_realign_dev(
            self.handle, C.byref(dbatch.c), dbatch.n_reads, dbatch.n_bases, int(max_query_len), d_win_off, d_win,
            C.byref(dout.c), dout.counts.data_ptr(), stream or None))

    def batch_select_hp(self, batch: RegionBatch, haplotype: int, capacities=None):
        """the reads of one haplotype of a host batch (pv_batch_select_hp, host buffers) -> (RegionBatch of the kept reads,
        src_read int64 [kept]: their input indices); see batch_select.py"""
        from .batch_select import select_hp
        return select_hp(self, batch, haplotype, capacities)

    def batch_select_hp_dev(self, dbatch, haplotype: int, dout: "DeviceSelectOut", stream: int = 0):
        """asynchronous, device-resident selection of dbatch's reads by haplotype (pv_batch_select_hp_dev) into a
        device.DeviceSelectOut; counters {reads, bases, cigar words kept, status} in dout.counts. dbatch.read_hp None = no
        read is tagged (every read is kept)."""
        hp = getattr(dbatch, "read_hp", None)
        _ffi.check(self.lib.pv_batch_select_hp_dev(
            self.handle, C.byref(dbatch.c), None if hp is None else hp.data_ptr(), dbatch.n_reads, dbatch.n_bases, dbatch.n_cigar,
            int(haplotype), C.byref(dout.c), dout.counts.data_ptr(), stream or None))

    def bgzf_inflate(self, payload: np.ndarray, in_off, clen, isize, crc, out_off, out: np.ndarray = None):
        """host-buffer BGZF inflate (pv_bgzf_inflate) of a block table -> (out uint8, status int32 [n], counts (bytes,
        status, first bad block, its status)). A failed block does not raise: its status says why (the PV_BGZF_* codes).
        out None: a zeroed buffer of max(out_off + isize) bytes; bytes outside every block's range are left as given."""
        pay = np.ascontiguousarray(payload, np.uint8)
        ioff, ooff = np.ascontiguousarray(in_off, np.int64), np.ascontiguousarray(out_off, np.int64)
        cl, isz = np.ascontiguousarray(clen, np.int32), np.ascontiguousarray(isize, np.int32)
        cr = np.ascontiguousarray(crc, np.uint32)
        n = len(ioff)
        assert len(cl) == n and len(isz) == n and len(cr) == n and len(ooff) == n
        if out is None:
            out = np.zeros(int((ooff + isz).max()) if n else 0, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"]
        status = np.zeros(max(n, 1), np.int32)
        counts = (C.c_int64 * 4)()
        rc = self.lib.pv_bgzf_inflate(self.handle, _ffi.ptr(pay), pay.size, n, _ffi.ptr(ioff), _ffi.ptr(cl), _ffi.ptr(isz),
                                      _ffi.ptr(cr), _ffi.ptr(ooff), _ffi.ptr(out) if out.size else None, out.size,
                                      _ffi.ptr(status), counts)
        if rc != _ffi.PV_OK and not (rc == _ffi.PV_ERR_INVALID and counts[1] == _ffi.PV_ERR_INVALID):
            _ffi.check(rc)
        return out, status[:n], tuple(int(v) for v in counts)

    def bgzf_inflate_dev(self, d_payload: int, payload_bytes: int, n_blocks: int, d_in_off: int, d_clen: int, d_isize: int,
                         d_crc: int, d_out_off: int, d_out: int, out_bytes: int, d_status: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident BGZF inflate (pv_bgzf_inflate_dev): every argument a device address; statuses in
        d_status [n_blocks], {bytes, status, first bad block, its status} in d_counts (int64 [4]). Uses no workspace: it may
        run on its own stream beside the builder / RNN calls of this context."""
        _ffi.check(self.lib.pv_bgzf_inflate_dev(self.handle, d_payload, int(payload_bytes), int(n_blocks), d_in_off, d_clen,
                                                d_isize, d_crc, d_out_off, d_out, int(out_bytes), d_status, d_counts,
                                                stream or None))

    def bam_scan_dev(self, cin: "_ffi.pv_bam_decode_in", d_ws: int, ws_bytes: int, d_iv_counts: int, stream: int = 0):
        """asynchronous, device-resident scan phase of the BAM record decode (pv_bam_scan_dev): walks and measures the records
        of every interval of `cin`; int64 [n_intervals][8] counts land in d_iv_counts. Uses only the caller's workspace."""
        _ffi.check(self.lib.pv_bam_scan_dev(self.handle, C.byref(cin), d_ws, int(ws_bytes), d_iv_counts, stream or None))

    def bam_fill_dev(self, cin: "_ffi.pv_bam_decode_in", d_ws: int, ws_bytes: int, n_regions: int, d_reg_iv: int, d_read_off: int,
                     d_sel_off: int, d_sel: int, n_sel: int, n_reads: int, base_capacity: int, cigar_capacity: int,
                     out: "_ffi.pv_batch_in", d_read_hp: int, d_totals: int, stream: int = 0):
        """asynchronous fill phase (pv_bam_fill_dev) behind bam_scan_dev on the same stream: the read arrays of `out` and
        read_hp for the regions the host kept; {reads, bases, CIGAR words, status} in d_totals (int64 [4])."""
        _ffi.check(self.lib.pv_bam_fill_dev(self.handle, C.byref(cin), d_ws, int(ws_bytes), int(n_regions), d_reg_iv, d_read_off,
                                            d_sel_off, d_sel, int(n_sel), int(n_reads), int(base_capacity), int(cigar_capacity),
                                            C.byref(out), d_read_hp, d_totals, stream or None))

    def polish_stitch_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_region_start: int, n_regions: int,
                          d_region_off: int, d_seq: int, seq_capacity: int, d_counts: int, stream: int = 0, d_row_qual: int = 0,
                          d_qual: int = 0):
        """asynchronous, device-resident stitch (pv_polish_stitch_dev): the labels of dout's first n_chunks chunks -> polished
        bases in d_seq, region offsets in d_region_off [n_regions+1], {bases, status, first bad chunk, 0} in d_counts.
        With d_row_qual (uint8 [n_chunks, L]) and d_qual (uint8 [seq_capacity]) the quality plane too
        (pv_polish_stitch_qual_dev): one raw Phred byte in d_qual for every base of d_seq."""
        args = (self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_region_start, int(n_regions), dout.seq_length,
                dout.seq_overlap, d_region_off, d_seq, int(seq_capacity), d_counts, stream or None)
        if d_row_qual or d_qual:
            _ffi.check(self.lib.pv_polish_stitch_qual_dev(*args, d_row_qual or None, d_qual or None))
        else:
            _ffi.check(self.lib.pv_polish_stitch_dev(*args))

    @staticmethod
    def _host_polish_out(out, seq_length: int = None, depth: bool = False, counts: bool = False):
        """the host pv_polish_out view of a PolishOut's position, index, region and chunk_id -> (n_chunks, struct, the
        arrays it points into: keep them until the call returns). depth, counts: and of its depth / counts plane, uint16
        [n, seq_length] / [n, seq_length, 10]; one the PolishOut lacks stays null, for the call to refuse."""
        keep = [np.ascontiguousarray(a, t) for a, t in ((out.position, np.int64), (out.index, np.int32), (out.region, np.int32),
                                                        (out.chunk_id, np.int32))]
        c = _ffi.pv_polish_out()
        c.chunk_capacity = n = int(len(out.chunk_id))
        c.position, c.index, c.region, c.chunk_id = (_ffi.ptr(a) for a in keep)
        for want, field, more in ((depth, "depth", ()), (counts, "counts", (10,))):
            if want and getattr(out, field, None) is not None:
                plane = np.ascontiguousarray(getattr(out, field), np.uint16)
                assert plane.shape == (n, seq_length) + more, plane.shape
                setattr(c, field, _ffi.ptr(plane))
                keep.append(plane)
        return n, c, keep

    @staticmethod
    def _host_draft(batch):
        """the draft triple of the batch the chunks were built from (a RegionBatch's ref_start, ref_off, ref) as contiguous
        arrays -> (region starts int64, draft offsets int64 [n_regions+1], draft bytes or None)"""
        rs = np.ascontiguousarray(batch.ref_start, np.int64)
        ro = np.ascontiguousarray(batch.ref_off, np.int64)
        ref = None if batch.ref is None else np.ascontiguousarray(batch.ref, np.uint8)
        assert len(ro) == len(rs) + 1 and (ref is None or len(ref) >= int(ro[-1])), (len(ro), len(rs))
        return rs, ro, ref

    def _label_pass(self, call, out, labels, row_qual, batch, sizes, level, counts, in_place, depth=False, rowcounts=False):
        """one pass that rewrites labels and row qualities (pv_polish_mask_low_depth and the two filters; sizes: seq_length
        [, seq_overlap]) -> (labels, row_qual or None) after it. in_place: the arrays given (C-contiguous uint8) are rewritten
        and returned; else copies are."""
        n, c, keep = self._host_polish_out(out, sizes[0], depth, rowcounts)
        lab = labels if in_place else np.ascontiguousarray(labels, np.uint8)
        rq = row_qual if in_place or row_qual is None else np.ascontiguousarray(row_qual, np.uint8)
        assert lab.dtype == np.uint8 and (rq is None or rq.dtype == np.uint8)
        assert lab.shape == (n, sizes[0]) and (rq is None or rq.shape == lab.shape), lab.shape
        rs, ro, ref = self._host_draft(batch)
        lab_out = lab if in_place else np.zeros_like(lab)
        rq_out = rq if in_place or rq is None else np.zeros_like(rq)
        if counts is None:
            counts = (C.c_int64 * 4)()
        _ffi.check(call(self.handle, C.byref(c), n, _ffi.ptr(lab), _ffi.ptr(rq), _ffi.ptr(rs), _ffi.ptr(ro), _ffi.ptr(ref), len(rs),
                        *(int(v) for v in sizes), int(level), _ffi.ptr(lab_out), _ffi.ptr(rq_out), counts))
        return lab_out, rq_out

    def _polish_stitch(self, out, labels, row_qual, region_start, seq_capacity, seq_length, seq_overlap, counts):
        """polish_stitch (row_qual None) / polish_stitch_qual -> (region_off, seq bytes[, qual bytes])"""
        n, c, keep = self._host_polish_out(out)
        lab = np.ascontiguousarray(labels, np.uint8)
        rs = np.ascontiguousarray(region_start, np.int64)
        assert lab.shape == (n, seq_length), lab.shape
        cap = n * seq_length if seq_capacity is None else int(seq_capacity)
        region_off = np.zeros(len(rs) + 1, np.int64)
        seq = np.zeros(max(cap, 1), np.uint8)
        if counts is None:
            counts = (C.c_int64 * 4)()
        args = (self.handle, C.byref(c), n, _ffi.ptr(lab), _ffi.ptr(rs), len(rs), seq_length, seq_overlap, _ffi.ptr(region_off),
                _ffi.ptr(seq), cap, counts)
        if row_qual is None:
            _ffi.check(self.lib.pv_polish_stitch(*args))
            return region_off, seq[:int(counts[0])].tobytes()
        rq = np.ascontiguousarray(row_qual, np.uint8)
        assert rq.shape == lab.shape, (lab.shape, rq.shape)
        qual = np.zeros(max(cap, 1), np.uint8)
        _ffi.check(self.lib.pv_polish_stitch_qual(*args, _ffi.ptr(rq), _ffi.ptr(qual)))
        return region_off, seq[:int(counts[0])].tobytes(), qual[:int(counts[0])].tobytes()

    def polish_stitch(self, out, labels: np.ndarray, region_start: np.ndarray, seq_capacity: int = None,
                      seq_length: int = 1000, seq_overlap: int = 50, counts=None):
        """host-buffer stitch (pv_polish_stitch) of a PolishOut and its labels -> (region_off int64 [n_regions+1], seq bytes).
        seq_capacity None: every column's worth; a smaller one raises PepperHipError(PV_ERR_CAPACITY).
        counts: optional ctypes int64[4] that receives {bases, status, first bad chunk, 0}, also when the call raises."""
        return self._polish_stitch(out, labels, None, region_start, seq_capacity, seq_length, seq_overlap, counts)

    def polish_row_qual_dev(self, d_labels: int, d_acc: int, B: int, d_qual: int, d_counts: int, seq_length: int = 1000,
                            seq_overlap: int = 50, stream: int = 0):
        """asynchronous, device-resident row qualities (pv_polish_row_qual_dev): labels uint8 [B,L] and acc float [B,L,5] of
        forward_p2_dev -> qual uint8 [B,L]; {rows, status, first bad chunk, its first bad row} in d_counts."""
        _ffi.check(self.lib.pv_polish_row_qual_dev(self.handle, d_labels, d_acc, int(B), int(seq_length), int(seq_overlap), d_qual,
                                                   d_counts, stream or None))

    def polish_row_qual(self, labels: np.ndarray, acc: np.ndarray, seq_overlap: int = 50, counts=None) -> np.ndarray:
        """host-buffer row qualities (pv_polish_row_qual): labels uint8 [B,L], acc float32 [B,L,5] -> qual uint8 [B,L].
        A label above 4 raises PepperHipError(PV_ERR_STATE). counts: optional ctypes int64[4], filled also when the call raises."""
        lab = np.ascontiguousarray(labels, np.uint8)
        a = np.ascontiguousarray(acc, np.float32)
        assert lab.ndim == 2 and a.shape == lab.shape + (5,), (lab.shape, a.shape)
        qual = np.zeros(lab.shape, np.uint8)
        if counts is None:
            counts = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_polish_row_qual(self.handle, _ffi.ptr(lab), _ffi.ptr(a), lab.shape[0], lab.shape[1], int(seq_overlap),
                                               _ffi.ptr(qual), counts))
        return qual

    def polish_stitch_qual_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int, d_region_start: int,
                               n_regions: int, d_region_off: int, d_seq: int, d_qual: int, seq_capacity: int, d_counts: int,
                               stream: int = 0):
        """polish_stitch_dev with the quality plane, in the C entry point's argument order"""
        self.polish_stitch_dev(dout, n_chunks, d_labels, d_region_start, n_regions, d_region_off, d_seq, seq_capacity, d_counts,
                               stream, d_row_qual, d_qual)

    def polish_stitch_qual(self, out, labels: np.ndarray, row_qual: np.ndarray, region_start: np.ndarray, seq_capacity: int = None,
                           seq_length: int = 1000, seq_overlap: int = 50, counts=None):
        """polish_stitch with the quality plane (pv_polish_stitch_qual) -> (region_off, seq bytes, qual bytes: raw Phred)."""
        return self._polish_stitch(out, labels, row_qual, region_start, seq_capacity, seq_length, seq_overlap, counts)

    def polish_edits_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int, d_region_start: int,
                         d_ref_off: int, d_ref: int, n_regions: int, d_region_edit_off: int, d_edits: int, edit_capacity: int,
                         d_counts: int, stream: int = 0):
        """asynchronous, device-resident edit list (pv_polish_edits_dev): the labels of dout's first n_chunks chunks against the
        draft bytes d_ref / d_ref_off of the batch -> 16-byte records (polish_edits.EDIT_DTYPE) in d_edits, region offsets in
        d_region_edit_off [n_regions+1], {edits, status, first bad chunk, 0} in d_counts. d_row_qual 0: qual 255."""
        _ffi.check(self.lib.pv_polish_edits_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_row_qual or None, d_region_start, d_ref_off, d_ref or None,
            int(n_regions), dout.seq_length, dout.seq_overlap, d_region_edit_off, d_edits, int(edit_capacity), d_counts,
            stream or None))

    def polish_edits(self, out, labels: np.ndarray, batch, row_qual: np.ndarray = None, edit_capacity: int = None,
                     seq_length: int = 1000, seq_overlap: int = 50, counts=None, region_edit_off: np.ndarray = None):
        """host-buffer edit list (pv_polish_edits) of a PolishOut, its labels and the batch they were built from (ref_start,
        ref_off, ref: a RegionBatch) -> (region_edit_off int64 [n_regions+1], records as a polish_edits.EDIT_DTYPE array).
        edit_capacity None: one record per chunk row; a smaller one raises PepperHipError(PV_ERR_CAPACITY).
        counts: optional ctypes int64[4] that receives {edits, status, first bad chunk, 0}, and region_edit_off an optional
        int64 [n_regions+1] array that receives the offsets, also when the call raises."""
        return self._polish_edits(out, labels, batch, row_qual, edit_capacity, seq_length, seq_overlap, counts, region_edit_off)

    def _polish_edits(self, out, labels, batch, row_qual, edit_capacity, seq_length, seq_overlap, counts, region_edit_off,
                      with_ev=False, evidence=None):
        """polish_edits / (with_ev) polish_edits_evidence"""
        from .polish_edits import EDIT_DTYPE, EVIDENCE_DTYPE
        n, c, keep = self._host_polish_out(out, seq_length, depth=with_ev, counts=with_ev)
        lab = np.ascontiguousarray(labels, np.uint8)
        rq = None if row_qual is None else np.ascontiguousarray(row_qual, np.uint8)
        assert lab.shape == (n, seq_length) and (rq is None or rq.shape == lab.shape), lab.shape
        rs, ro, ref = self._host_draft(batch)
        cap = n * seq_length if edit_capacity is None else int(edit_capacity)
        if region_edit_off is None:
            region_edit_off = np.zeros(len(rs) + 1, np.int64)
        edits = np.zeros(max(cap, 1), EDIT_DTYPE)
        if counts is None:
            counts = (C.c_int64 * 4)()
        args = (self.handle, C.byref(c), n, _ffi.ptr(lab), _ffi.ptr(rq), _ffi.ptr(rs), _ffi.ptr(ro), _ffi.ptr(ref), len(rs),
                seq_length, seq_overlap, _ffi.ptr(region_edit_off), _ffi.ptr(edits))
        if not with_ev:
            _ffi.check(self.lib.pv_polish_edits(*args, cap, counts))
            return region_edit_off, edits[:int(counts[0])].copy()
        if evidence is None:
            evidence = np.zeros(max(cap, 1), EVIDENCE_DTYPE)
        assert evidence.dtype == EVIDENCE_DTYPE and len(evidence) >= cap and evidence.flags.c_contiguous
        _ffi.check(self.lib.pv_polish_edits_evidence(*args, _ffi.ptr(evidence), cap, counts))
        return region_edit_off, edits[:int(counts[0])].copy(), evidence[:int(counts[0])].copy()

    def polish_edits_evidence_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int, d_region_start: int,
                                  d_ref_off: int, d_ref: int, n_regions: int, d_region_edit_off: int, d_edits: int, d_evidence: int,
                                  edit_capacity: int, d_counts: int, stream: int = 0):
        """polish_edits_dev with one 8-byte evidence record (polish_edits.EVIDENCE_DTYPE) per edit record in d_evidence
        (pv_polish_edits_evidence_dev); dout must carry the depth and the counts plane"""
        _ffi.check(self.lib.pv_polish_edits_evidence_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_row_qual or None, d_region_start, d_ref_off, d_ref or None,
            int(n_regions), dout.seq_length, dout.seq_overlap, d_region_edit_off, d_edits, d_evidence or None, int(edit_capacity),
            d_counts, stream or None))

    def polish_edits_evidence(self, out, labels: np.ndarray, batch, row_qual: np.ndarray = None, edit_capacity: int = None,
                              seq_length: int = 1000, seq_overlap: int = 50, counts=None, region_edit_off: np.ndarray = None,
                              evidence: np.ndarray = None):
        """host-buffer form (pv_polish_edits_evidence) of a PolishOut with its depth and counts planes -> (region_edit_off,
        edit records, evidence records as a polish_edits.EVIDENCE_DTYPE array). The other arguments are polish_edits';
        evidence: an optional EVIDENCE_DTYPE array of at least the capacity that receives the records (tests look at what
        the call left alone)."""
        return self._polish_edits(out, labels, batch, row_qual, edit_capacity, seq_length, seq_overlap, counts, region_edit_off,
                                  True, evidence)

    def polish_mask_low_depth_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int, d_region_start: int,
                                  d_ref_off: int, d_ref: int, n_regions: int, min_depth: int, d_labels_out: int,
                                  d_row_qual_out: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident minimum-depth mask (pv_polish_mask_low_depth_dev): rows of dout's first n_chunks
        chunks whose depth (dout.depth) is below min_depth get the label that spells the draft byte under them (insert rows:
        0) and quality 0; {masked rows, status, first bad chunk, unmaskable rows} in d_counts. d_labels_out == d_labels and
        d_row_qual_out == d_row_qual run in place; d_row_qual 0 (with d_row_qual_out 0): no quality plane."""
        _ffi.check(self.lib.pv_polish_mask_low_depth_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_row_qual or None, d_region_start, d_ref_off, d_ref or None,
            int(n_regions), dout.seq_length, int(min_depth), d_labels_out, d_row_qual_out or None, d_counts, stream or None))

    def polish_mask_low_depth(self, out, labels: np.ndarray, batch, min_depth: int, row_qual: np.ndarray = None,
                              seq_length: int = 1000, counts=None, in_place: bool = False):
        """host-buffer minimum-depth mask (pv_polish_mask_low_depth) of a PolishOut with its depth plane, its labels and the
        batch they were built from (ref_start, ref_off, ref) -> (labels, row_qual or None) after the mask. in_place: the
        arrays given (C-contiguous uint8) are rewritten and returned; else copies are.
        counts: optional ctypes int64[4] that receives {masked rows, status, first bad chunk, unmaskable rows}, also when the
        call raises."""
        return self._label_pass(self.lib.pv_polish_mask_low_depth, out, labels, row_qual, batch, (seq_length,), min_depth, counts,
                                in_place, depth=True)

    def polish_filter_low_qual_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int, d_region_start: int,
                                   d_ref_off: int, d_ref: int, n_regions: int, min_qual: int, d_labels_out: int,
                                   d_row_qual_out: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident minimum-quality filter (pv_polish_filter_low_qual_dev): every run of adjacent owned
        edit columns of dout's first n_chunks chunks whose lowest row quality is below min_qual is taken back: its rows get the
        labels that spell the draft (insert rows: 0) and quality 0; {rows reverted, status, first bad chunk, rows of pinned
        runs below min_qual} in d_counts. d_labels_out == d_labels and d_row_qual_out == d_row_qual run in place; the row
        qualities are mandatory."""
        _ffi.check(self.lib.pv_polish_filter_low_qual_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_row_qual or None, d_region_start, d_ref_off, d_ref or None,
            int(n_regions), dout.seq_length, dout.seq_overlap, int(min_qual), d_labels_out, d_row_qual_out or None, d_counts,
            stream or None))

    def polish_filter_low_qual(self, out, labels: np.ndarray, batch, min_qual: int, row_qual: np.ndarray,
                               seq_length: int = 1000, seq_overlap: int = 50, counts=None, in_place: bool = False):
        """host-buffer minimum-quality filter (pv_polish_filter_low_qual) of a PolishOut, its labels, their row qualities and
        the batch they were built from (ref_start, ref_off, ref) -> (labels, row_qual) after the filter. in_place: the arrays
        given (C-contiguous uint8) are rewritten and returned; else copies are.
        counts: optional ctypes int64[4] that receives {rows reverted, status, first bad chunk, rows of pinned runs below
        min_qual}, also when the call raises."""
        return self._label_pass(self.lib.pv_polish_filter_low_qual, out, labels, row_qual, batch, (seq_length, seq_overlap), min_qual,
                                counts, in_place)

    def polish_filter_low_support_dev(self, dout: "DevicePolishOut", n_chunks: int, d_labels: int, d_row_qual: int,
                                      d_region_start: int, d_ref_off: int, d_ref: int, n_regions: int, min_support: int,
                                      d_labels_out: int, d_row_qual_out: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident minimum-support filter (pv_polish_filter_low_support_dev): every run of adjacent owned
        edit columns of dout's first n_chunks chunks whose weakest column is spelled by fewer than min_support reads (dout's
        counts plane; dout must carry depth and counts) is taken back: its rows get the labels that spell the draft (insert
        rows: 0) and quality 0; {rows reverted, status, first bad chunk, rows of pinned runs below min_support} in d_counts.
        d_labels_out == d_labels and d_row_qual_out == d_row_qual run in place; d_row_qual 0 (with d_row_qual_out 0): no
        quality plane."""
        _ffi.check(self.lib.pv_polish_filter_low_support_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_labels, d_row_qual or None, d_region_start, d_ref_off, d_ref or None,
            int(n_regions), dout.seq_length, dout.seq_overlap, int(min_support), d_labels_out, d_row_qual_out or None, d_counts,
            stream or None))

    def polish_filter_low_support(self, out, labels: np.ndarray, batch, min_support: int, row_qual: np.ndarray = None,
                                  seq_length: int = 1000, seq_overlap: int = 50, counts=None, in_place: bool = False):
        """host-buffer minimum-support filter (pv_polish_filter_low_support) of a PolishOut with its depth and counts planes,
        its labels, their row qualities (or None) and the batch they were built from (ref_start, ref_off, ref) -> (labels,
        row_qual or None) after the filter. in_place: the arrays given (C-contiguous uint8) are rewritten and returned; else
        copies are.
        counts: optional ctypes int64[4] that receives {rows reverted, status, first bad chunk, rows of pinned runs below
        min_support}, also when the call raises."""
        return self._label_pass(self.lib.pv_polish_filter_low_support, out, labels, row_qual, batch, (seq_length, seq_overlap),
                                min_support, counts, in_place, depth=True, rowcounts=True)

    def polish_vote_dev(self, dout: "DevicePolishOut", n_chunks: int, d_region_start: int, d_ref_off: int, d_ref: int,
                        n_regions: int, d_labels: int, d_acc: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident majority vote (pv_polish_vote_dev), in the place of forward_p2_dev: the counts and
        depth planes of dout's first n_chunks chunks (dout must carry both) and the draft bytes -> labels uint8 [n,L] in
        d_labels and, unless d_acc is 0, the five read fractions of every row times the windows that cover it in d_acc, float
        [n,L,5]; {rows whose winner is not the draft's, status, first bad chunk, base rows without reads} in d_counts."""
        _ffi.check(self.lib.pv_polish_vote_dev(
            self.handle, C.byref(dout.c), int(n_chunks), d_region_start, d_ref_off, d_ref or None, int(n_regions), dout.seq_length,
            dout.seq_overlap, d_labels, d_acc or None, d_counts, stream or None))

    def polish_vote(self, out, batch, seq_length: int = 1000, seq_overlap: int = 50, want_acc: bool = False, counts=None,
                    labels: np.ndarray = None, acc: np.ndarray = None):
        """host-buffer majority vote (pv_polish_vote) of a PolishOut with its depth and counts planes and the batch it was
        built from (ref_start, ref_off, ref) -> labels uint8 [n,L], or (labels, acc float32 [n,L,5]) with want_acc.
        counts: optional ctypes int64[4] that receives {rows whose winner is not the draft's, status, first bad chunk, base
        rows without reads}, also when the call raises. labels, acc: optional C-contiguous arrays that receive the planes
        (tests look at what the call left alone); acc implies want_acc."""
        n, c, keep = self._host_polish_out(out, seq_length, depth=True, counts=True)
        rs, ro, ref = self._host_draft(batch)
        if labels is None:
            labels = np.zeros((n, seq_length), np.uint8)
        if acc is None and want_acc:
            acc = np.zeros((n, seq_length, 5), np.float32)
        assert labels.dtype == np.uint8 and labels.shape == (n, seq_length), labels.shape
        assert acc is None or (acc.dtype == np.float32 and acc.shape == (n, seq_length, 5)), acc.shape
        if counts is None:
            counts = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_polish_vote(self.handle, C.byref(c), n, _ffi.ptr(rs), _ffi.ptr(ro), _ffi.ptr(ref), len(rs), seq_length,
                                           int(seq_overlap), _ffi.ptr(labels), _ffi.ptr(acc), counts))
        return labels if acc is None else (labels, acc)

    def polish_vote_runs_dev(self, dout: "DevicePolishOut", n_chunks: int, dbatch, d_region_start: int, d_ref_off: int,
                             d_ref: int, n_regions: int, min_run: int, d_labels: int, d_acc: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident run vote (pv_polish_vote_runs_dev) behind polish_vote_dev, in place on the same
        d_labels / d_acc (0: no acc): the reads of dbatch, the batch the builder was given, vote the length of every
        homopolymer run of the draft; {runs decided, status, first bad chunk, decided runs whose length changes, candidates,
        candidates skipped as adjacent} in the six int64 of d_counts."""
        _ffi.check(self.lib.pv_polish_vote_runs_dev(
            self.handle, C.byref(dout.c), int(n_chunks), C.byref(dbatch.c), dbatch.n_reads, dbatch.n_bases, dbatch.n_cigar,
            dbatch.n_ref_bytes, d_region_start, d_ref_off, d_ref or None, int(n_regions), dout.seq_length, dout.seq_overlap,
            int(min_run), d_labels, d_acc or None, d_counts, stream or None))

    def polish_vote_runs(self, out, batch, labels: np.ndarray, acc: np.ndarray = None, min_run: int = 3, seq_length: int = 1000,
                         seq_overlap: int = 50, counts=None):
        """host-buffer run vote (pv_polish_vote_runs) of a PolishOut and the host batch it was built from, in place on
        labels uint8 [n,L] and acc float32 [n,L,5] (or None), the planes polish_vote left -> labels, or (labels, acc).
        counts: optional ctypes int64[6] that receives the six counters, also when the call raises."""
        n, c, keep = self._host_polish_out(out)
        assert labels.dtype == np.uint8 and labels.shape == (n, seq_length) and labels.flags.c_contiguous, labels.shape
        assert acc is None or (acc.dtype == np.float32 and acc.shape == (n, seq_length, 5) and acc.flags.c_contiguous), acc.shape
        cin = batch.as_c()
        if counts is None:
            counts = (C.c_int64 * 6)()
        _ffi.check(self.lib.pv_polish_vote_runs(self.handle, C.byref(c), n, C.byref(cin), seq_length, int(seq_overlap), int(min_run),
                                                _ffi.ptr(labels), _ffi.ptr(acc), counts))
        return labels if acc is None else (labels, acc)

    # ---- assess ----------------------------------------------------------------------------------
    def assess_scratch_bytes(self, a_off: np.ndarray, segment: int) -> int:
        """bytes of scratch pv_assess_dev needs for assemblies with these (host) offsets"""
        ao = np.ascontiguousarray(a_off, np.int64)
        n = int(self.lib.pv_assess_scratch_bytes(len(ao) - 1, _ffi.ptr(ao), int(segment)))
        if n < 0:
            raise _ffi.PepperHipError(n, "assess: bad offsets or segment")
        return n

    def assess_dev(self, d_a: int, d_a_off: int, d_b: int, d_b_off: int, n_pairs: int, segment: int, max_shift: int,
                   seg_capacity: int, d_segs: int, d_pair_seg_off: int, d_totals: int, d_scratch: int, scratch_bytes: int,
                   d_counts: int, stream: int = 0):
        """asynchronous, device-resident pv_assess_dev: every array is a device pointer; {records, status, records needed,
        scratch needed} in d_counts. Under a status other than PV_OK the outputs hold -1 in every field."""
        _ffi.check(self.lib.pv_assess_dev(self.handle, d_a or None, d_a_off, d_b or None, d_b_off, int(n_pairs), int(segment),
                                          int(max_shift), int(seg_capacity), d_segs or None, d_pair_seg_off, d_totals or None,
                                          d_scratch or None, int(scratch_bytes), d_counts, stream or None))

    def assess(self, pairs, segment: int = 1024, max_shift: int = 8192, seg_capacity: int = None, counts=None, out=None):
        """host-buffer pv_assess of [(assembly bytes, truth bytes)], already upper-cased -> (segs, pair_seg_off, totals):
        segs a numpy record array of pv_assess_seg [n_segments], pair_seg_off int64 [n_pairs+1], totals int64 [n_pairs, 16].
        seg_capacity: records to provide (default: what the pairs need). counts: optional ctypes int64[4]; out: optional
        (segs [seg_capacity], pair_seg_off, totals) arrays that receive the outputs, also when the call raises."""
        n = len(pairs)
        a_off = np.zeros(n + 1, np.int64)
        b_off = np.zeros(n + 1, np.int64)
        a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
        b_off[1:] = np.cumsum([len(b) for _, b in pairs])
        A = np.frombuffer(b"".join(bytes(a) for a, _ in pairs) or b"\0", np.uint8)   # (never a null pointer: one unread byte)
        B = np.frombuffer(b"".join(bytes(b) for _, b in pairs) or b"\0", np.uint8)
        if seg_capacity is None:
            seg_capacity = int(sum(len(a) // int(segment) + 1 for a, _ in pairs))
        if out is None:
            out = (np.zeros(seg_capacity, np.dtype(_ffi.pv_assess_seg)), np.zeros(n + 1, np.int64),
                   np.zeros((n, _ffi.PV_ASSESS_TOTALS), np.int64))
        segs, seg_off, totals = out
        assert segs.dtype.itemsize == 64 and len(segs) >= seg_capacity and len(seg_off) == n + 1 and totals.shape == (n, 16)
        if counts is None:
            counts = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_assess(self.handle, _ffi.ptr(A), _ffi.ptr(a_off), _ffi.ptr(B), _ffi.ptr(b_off), n, int(segment), int(max_shift), int(seg_capacity),
                                      _ffi.ptr(segs) if len(segs) else None, _ffi.ptr(seg_off), _ffi.ptr(totals) if n else None,
                                      counts))
        return segs[:int(counts[0])], seg_off, totals

    def assess_errors_scratch_bytes(self, a_off: np.ndarray, segment: int) -> int:
        """bytes of scratch pv_assess_errors_dev needs for assemblies with these (host) offsets"""
        ao = np.ascontiguousarray(a_off, np.int64)
        n = int(self.lib.pv_assess_errors_scratch_bytes(len(ao) - 1, _ffi.ptr(ao), int(segment)))
        if n < 0:
            raise _ffi.PepperHipError(n, "assess: bad offsets or segment")
        return n

    def assess_errors_dev(self, d_a: int, d_a_off: int, d_b: int, d_b_off: int, n_pairs: int, segment: int, max_shift: int,
                          seg_capacity: int, d_segs: int, d_pair_seg_off: int, d_totals: int, d_q: int, err_capacity: int,
                          d_errs: int, d_pair_err_off: int, d_qhist: int, d_scratch: int, scratch_bytes: int, d_counts: int,
                          stream: int = 0):
        """asynchronous, device-resident pv_assess_errors_dev: every array is a device pointer (d_q and d_qhist both 0 without
        qualities); d_counts int64[8] = {segment records, status, slots needed, scratch needed, error records written, error
        records needed, 0, 0}. The status PV_ERR_CAPACITY (err_capacity too small) leaves every output but d_errs valid."""
        _ffi.check(self.lib.pv_assess_errors_dev(self.handle, d_a or None, d_a_off, d_b or None, d_b_off, int(n_pairs), int(segment),
                                                 int(max_shift), int(seg_capacity), d_segs or None, d_pair_seg_off,
                                                 d_totals or None, d_q or None, int(err_capacity), d_errs or None, d_pair_err_off,
                                                 d_qhist or None, d_scratch or None, int(scratch_bytes), d_counts, stream or None))

    def assess_errors(self, pairs, quals=None, segment: int = 1024, max_shift: int = 8192, err_capacity: int = None,
                      seg_capacity: int = None, counts=None, out=None):
        """host-buffer pv_assess_errors of [(assembly bytes, truth bytes)], already upper-cased, and optionally one array of raw
        Phred bytes (0..93) per assembly -> (segs, pair_seg_off, totals, errs, pair_err_off, qhist or None): errs a numpy record
        array of pv_assess_error, pair_err_off int64 [n_pairs+1], qhist int64 [n_pairs, 94, 4] = {bases, sub, ins, del}.
        err_capacity None: starts from (len A + len B) // 16 + 1024 records and, if the device reports PV_ERR_CAPACITY, calls
        once more with the need it reported. A given err_capacity is used as it is. counts: optional ctypes int64[8]; out:
        optional (segs, pair_seg_off, totals, errs [err_capacity], pair_err_off, qhist or None) arrays that receive the outputs,
        also when the call raises."""
        n = len(pairs)
        a_off = np.zeros(n + 1, np.int64)
        b_off = np.zeros(n + 1, np.int64)
        a_off[1:] = np.cumsum([len(a) for a, _ in pairs])
        b_off[1:] = np.cumsum([len(b) for _, b in pairs])
        A = np.frombuffer(b"".join(bytes(a) for a, _ in pairs) or b"\0", np.uint8)
        B = np.frombuffer(b"".join(bytes(b) for _, b in pairs) or b"\0", np.uint8)
        Q = None
        if quals is not None:
            assert len(quals) == n and all(len(q) == len(a) for q, (a, _) in zip(quals, pairs)), "one quality per assembly base"
            Q = np.ascontiguousarray(np.concatenate([np.frombuffer(bytes(q), np.uint8) for q in quals] + [np.zeros(1, np.uint8)]))
        if seg_capacity is None:
            seg_capacity = int(sum(len(a) // int(segment) + 1 for a, _ in pairs))
        sized = err_capacity is not None
        if not sized:
            err_capacity = (int(a_off[n]) + int(b_off[n])) // 16 + 1024
        if counts is None:
            counts = (C.c_int64 * 8)()
        for attempt in (0, 1):
            if out is None or attempt:
                out = (np.zeros(seg_capacity, np.dtype(_ffi.pv_assess_seg)), np.zeros(n + 1, np.int64),
                       np.zeros((n, _ffi.PV_ASSESS_TOTALS), np.int64), np.zeros(err_capacity, np.dtype(_ffi.pv_assess_error)),
                       np.zeros(n + 1, np.int64), None if Q is None else np.zeros((n, _ffi.PV_ASSESS_QBINS, 4), np.int64))
            segs, seg_off, totals, errs, err_off, qhist = out
            assert segs.dtype.itemsize == 64 and len(segs) >= seg_capacity and len(seg_off) == n + 1 and totals.shape == (n, 16)
            assert errs.dtype.itemsize == 32 and len(errs) >= err_capacity and len(err_off) == n + 1
            assert (qhist is None) == (Q is None) and (qhist is None or qhist.shape == (n, _ffi.PV_ASSESS_QBINS, 4))
            rc = self.lib.pv_assess_errors(self.handle, _ffi.ptr(A), _ffi.ptr(a_off), _ffi.ptr(B), _ffi.ptr(b_off), n, int(segment),
                                           int(max_shift), int(seg_capacity), _ffi.ptr(segs) if len(segs) else None,
                                           _ffi.ptr(seg_off), _ffi.ptr(totals) if n else None, _ffi.ptr(Q), int(err_capacity),
                                           _ffi.ptr(errs) if len(errs) else None, _ffi.ptr(err_off),
                                           _ffi.ptr(qhist) if Q is not None else None, counts)
            if rc == _ffi.PV_ERR_CAPACITY and not sized and attempt == 0:
                err_capacity = int(counts[5])   # the one sized second call
                continue
            _ffi.check(rc)
            break
        return segs[:int(counts[0])], seg_off, totals, errs[:int(counts[4])], err_off, qhist

    def assess_place_scratch_bytes(self, a_off: np.ndarray, step: int) -> int:
        """bytes of scratch pv_assess_place_dev needs for an assembly with these (host) offsets"""
        ao = np.ascontiguousarray(a_off, np.int64)
        n = int(self.lib.pv_assess_place_scratch_bytes(len(ao) - 1, _ffi.ptr(ao), int(step)))
        if n < 0:
            raise _ffi.PepperHipError(n, "assess place: bad offsets or step")
        return n

    def assess_place_dev(self, d_a: int, d_a_off: int, n_asm: int, d_b: int, d_b_off: int, n_truth: int, step: int, min_hits: int,
                         d_recs: int, d_scratch: int, scratch_bytes: int, d_counts: int, stream: int = 0):
        """asynchronous, device-resident pv_assess_place_dev: every array is a device pointer; {records, status, first bad contig
        or -1, scratch needed} in d_counts. Under a status other than PV_OK the records hold -1 in every field."""
        _ffi.check(self.lib.pv_assess_place_dev(self.handle, d_a or None, d_a_off or None, int(n_asm), d_b or None, d_b_off or None,
                                                int(n_truth), int(step), int(min_hits), d_recs or None, d_scratch or None,
                                                int(scratch_bytes), d_counts, stream or None))

    def assess_place(self, asm, truth, step: int = 1024, min_hits: int = 3, counts=None, out=None):
        """host-buffer pv_assess_place of [assembly contig bytes] on [truth contig bytes], both upper-cased -> a numpy record
        array of pv_assess_placement [len(asm)]. counts: optional ctypes int64[4]; out: an optional record array that receives
        the records, also when the call raises."""
        n, m = len(asm), len(truth)
        a_off = np.zeros(n + 1, np.int64)
        b_off = np.zeros(m + 1, np.int64)
        a_off[1:] = np.cumsum([len(a) for a in asm])
        b_off[1:] = np.cumsum([len(b) for b in truth])
        A = np.frombuffer(b"".join(bytes(a) for a in asm) or b"\0", np.uint8)   # (never a null pointer: one unread byte)
        B = np.frombuffer(b"".join(bytes(b) for b in truth) or b"\0", np.uint8)
        if out is None:
            out = np.zeros(n, np.dtype(_ffi.pv_assess_placement))
        assert out.dtype.itemsize == 40 and len(out) == n
        if counts is None:
            counts = (C.c_int64 * 4)()
        _ffi.check(self.lib.pv_assess_place(self.handle, _ffi.ptr(A), _ffi.ptr(a_off), n, _ffi.ptr(B), _ffi.ptr(b_off), m, int(step),
                                            int(min_hits), _ffi.ptr(out) if n else None, counts))
        return out

    def kmer_table_bytes(self, a_off: np.ndarray) -> int:
        """bytes of table pv_kmer_table_build_dev needs for an assembly with these (host) offsets"""
        ao = np.ascontiguousarray(a_off, np.int64)
        n = int(self.lib.pv_kmer_table_bytes(len(ao) - 1, _ffi.ptr(ao)))
        if n < 0:
            raise _ffi.PepperHipError(n, "kmer table: bad offsets")
        return n

    def kmer_table_build_dev(self, d_a: int, d_a_off: int, n_asm: int, k: int, cap: int, d_table: int, table_bytes: int,
                             d_counts: int, stream: int = 0):
        """asynchronous, device-resident pv_kmer_table_build_dev: {keyed entries, status, first bad contig or -1, table bytes
        needed} in d_counts"""
        _ffi.check(self.lib.pv_kmer_table_build_dev(self.handle, d_a or None, d_a_off or None, int(n_asm), int(k), int(cap),
                                                    d_table or None, int(table_bytes), d_counts, stream or None))

    def kmer_count_reads_dev(self, d_table: int, table_bytes: int, d_bases: int, d_base_off: int, n_reads: int, n_bases: int,
                             stream: int = 0):
        """asynchronous pv_kmer_count_reads_dev: the reads' k-mers added to the table's counters"""
        _ffi.check(self.lib.pv_kmer_count_reads_dev(self.handle, d_table or None, int(table_bytes), d_bases or None,
                                                    d_base_off or None, int(n_reads), int(n_bases), stream or None))

    def kmer_support_dev(self, d_table: int, table_bytes: int, d_a_off: int, n_asm: int, min_count: int, segment: int, d_contig: int,
                         d_seg_off: int, seg_capacity: int, d_segs: int, run_capacity: int, d_runs: int, d_hist: int,
                         d_pos_counts: int, d_counts: int, stream: int = 0):
        """asynchronous pv_kmer_support_dev: {runs written, status, runs needed, segment slots needed, summed length, 0, 0, 0} in
        d_counts (int64[8])"""
        _ffi.check(self.lib.pv_kmer_support_dev(self.handle, d_table or None, int(table_bytes), d_a_off or None, int(n_asm),
                                                int(min_count), int(segment), d_contig or None, d_seg_off or None, int(seg_capacity),
                                                d_segs or None, int(run_capacity), d_runs or None, d_hist or None,
                                                d_pos_counts or None, d_counts, stream or None))

    def kmer_support(self, asm, reads, k: int = 21, cap: int = _ffi.PV_KMER_MAX_CAP, min_count: int = 1, segment: int = 1024,
                     run_capacity=None, seg_capacity=None, want_positions: bool = True, counts=None, out=None):
        """host-buffer pv_kmer_support of [assembly contig bytes] (upper-cased) against [read bytes] -> (contig counts int64
        [n][3], seg_off int64 [n+1], segs int64, runs int64 [r][3], hist int64 [256], pos_counts uint32 or None). run_capacity
        None: a second call is made with the capacity the first reports. counts: optional ctypes int64[8]; out: optional
        (contig, seg_off, segs, runs, hist, pos_counts) arrays that receive the result, also when the call raises."""
        n = len(asm)
        a_off = np.zeros(n + 1, np.int64)
        b_off = np.zeros(len(reads) + 1, np.int64)
        a_off[1:] = np.cumsum([len(a) for a in asm])
        b_off[1:] = np.cumsum([len(r) for r in reads])
        A = np.frombuffer(b"".join(bytes(a) for a in asm) or b"\0", np.uint8)   # (never a null pointer: one unread byte)
        B = np.frombuffer(b"".join(bytes(r) for r in reads) or b"\0", np.uint8)
        if seg_capacity is None:
            seg_capacity = int(sum((len(a) + int(segment) - 1) // max(int(segment), 1) for a in asm))
        sized = run_capacity is not None
        if not sized:
            run_capacity = 1024
        if counts is None:
            counts = (C.c_int64 * 8)()
        for attempt in (0, 1):
            if out is None or attempt:
                out = (np.zeros((n, 3), np.int64), np.zeros(n + 1, np.int64), np.zeros(seg_capacity, np.int64),
                       np.zeros((run_capacity, 3), np.int64), np.zeros(_ffi.PV_KMER_HIST, np.int64),
                       np.zeros(int(a_off[n]), np.uint32) if want_positions else None)
            ctg, seg_off, segs, runs, hist, plane = out
            assert ctg.shape == (n, 3) and len(seg_off) == n + 1 and len(segs) >= seg_capacity and len(runs) >= run_capacity
            rc = self.lib.pv_kmer_support(self.handle, _ffi.ptr(A), _ffi.ptr(a_off), n, _ffi.ptr(B), _ffi.ptr(b_off), len(reads),
                                          int(k), int(cap), int(min_count), int(segment), _ffi.ptr(ctg) if n else None,
                                          _ffi.ptr(seg_off), int(seg_capacity), _ffi.ptr(segs) if len(segs) else None,
                                          int(run_capacity), _ffi.ptr(runs) if len(runs) else None, _ffi.ptr(hist),
                                          _ffi.ptr(plane) if plane is not None and len(plane) else None, counts)
            if rc == _ffi.PV_ERR_CAPACITY and not sized and attempt == 0:
                run_capacity = int(counts[2])   # the one sized second call
                continue
            _ffi.check(rc)
            break
        return ctg, seg_off, segs[:int(counts[3])], runs[:int(counts[0])], hist, plane

    def kmer_reads_table_bytes(self, slots: int) -> int:
        """bytes of a reads-only table of `slots` entries (a power of two from PV_KMER_READS_MIN_SLOTS up)"""
        n = int(self.lib.pv_kmer_reads_table_bytes(int(slots)))
        if n < 0:
            raise _ffi.PepperHipError(n, "kmer reads table: slots must be a power of two in [1024, 2^34] (got %d)" % slots)
        return n

    def kmer_reads_table_init_dev(self, d_rtable: int, rtable_bytes: int, slots: int, cap: int, stream: int = 0):
        """asynchronous pv_kmer_reads_table_init_dev: every slot empty, the head written"""
        _ffi.check(self.lib.pv_kmer_reads_table_init_dev(self.handle, d_rtable or None, int(rtable_bytes), int(slots), int(cap),
                                                         stream or None))

    def kmer_count_reads_all_dev(self, d_table: int, table_bytes: int, d_rtable: int, rtable_bytes: int, d_bases: int,
                                 d_base_off: int, n_reads: int, n_bases: int, part: int = 0, n_parts: int = 1, stream: int = 0):
        """asynchronous pv_kmer_count_reads_all_dev: the k-mers of this part added to the assembly table where it holds them, to
        the reads-only table where it does not"""
        _ffi.check(self.lib.pv_kmer_count_reads_all_dev(self.handle, d_table or None, int(table_bytes), d_rtable or None,
                                                        int(rtable_bytes), d_bases or None, d_base_off or None, int(n_reads),
                                                        int(n_bases), int(part), int(n_parts), stream or None))

    def kmer_reads_flush_dev(self, d_rtable: int, rtable_bytes: int, d_ro_hist: int, d_counts: int, stream: int = 0):
        """asynchronous pv_kmer_reads_flush_dev: the table's counts added to ro_hist (int64[256]), {distinct keys, status, dropped
        instances, slots} in d_counts (int64[4]), the table emptied"""
        _ffi.check(self.lib.pv_kmer_reads_flush_dev(self.handle, d_rtable or None, int(rtable_bytes), d_ro_hist or None,
                                                    d_counts or None, stream or None))

    def kmer_spectrum_dev(self, d_table: int, table_bytes: int, d_spectrum: int, d_counts: int, stream: int = 0):
        """asynchronous pv_kmer_spectrum_dev: the assembly's distinct keys by (multiplicity, count) added to spectrum
        (int64[4][256]), {distinct keys, status} in d_counts (int64[2])"""
        _ffi.check(self.lib.pv_kmer_spectrum_dev(self.handle, d_table or None, int(table_bytes), d_spectrum or None,
                                                 d_counts or None, stream or None))

    def kmer_spectrum(self, asm, reads, k: int = 21, cap: int = _ffi.PV_KMER_MAX_CAP, slots: int = _ffi.PV_KMER_READS_MIN_SLOTS,
                      n_parts: int = 1, counts=None):
        """host-buffer pv_kmer_spectrum of [assembly contig bytes] (upper-cased) against [read bytes] -> (ro_hist int64 [256],
        spectrum int64 [4][256]). counts: optional ctypes int64[8], filled also when the call raises."""
        n = len(asm)
        a_off = np.zeros(n + 1, np.int64)
        b_off = np.zeros(len(reads) + 1, np.int64)
        a_off[1:] = np.cumsum([len(a) for a in asm])
        b_off[1:] = np.cumsum([len(r) for r in reads])
        A = np.frombuffer(b"".join(bytes(a) for a in asm) or b"\0", np.uint8)   # (never a null pointer: one unread byte)
        B = np.frombuffer(b"".join(bytes(r) for r in reads) or b"\0", np.uint8)
        spectrum, ro_hist = np.zeros((4, _ffi.PV_KMER_HIST), np.int64), np.zeros(_ffi.PV_KMER_HIST, np.int64)
        if counts is None:
            counts = (C.c_int64 * 8)()
        _ffi.check(self.lib.pv_kmer_spectrum(self.handle, _ffi.ptr(A), _ffi.ptr(a_off), n, _ffi.ptr(B), _ffi.ptr(b_off), len(reads),
                                             int(k), int(cap), int(slots), int(n_parts), _ffi.ptr(spectrum), _ffi.ptr(ro_hist),
                                             counts))
        return ro_hist, spectrum

    def profile_begin(self, only: str = None):
        """bracket every kernel launch of this context with HIP events (only: just the kernels whose profile name starts
        with it - two events per launch put a few microseconds between kernels)"""
        if only:
            _ffi.check(self.lib.pv_profile_begin_only(self.handle, only.encode()))
        else:
            _ffi.check(self.lib.pv_profile_begin(self.handle))

    def profile_end(self) -> dict:
        """-> {kernel name: (total ms, launches)} measured with HIP events on the launch stream"""
        buf = C.create_string_buffer(4096)
        ms = (C.c_float * 64)()
        cnt = (C.c_int * 64)()
        n = self.lib.pv_profile_end(self.handle, buf, 4096, ms, cnt, 64)
        if n < 0:
            _ffi.check(n)
        names = buf.value.decode().split("\n") if n else []
        return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}
