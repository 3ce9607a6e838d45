"""Device-resident batches: torch is used only as the HBM allocator / stream provider here.

The C-ABI's *_dev entry points take raw device pointers; these helpers keep the owning torch tensors
alive next to the C structs that point into them.
"""
import numpy as np
import torch

from . import _ffi
from .batch import RegionBatch


def _as_tensor(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint32:  # torch has no uint32 arithmetic; reinterpret the bits
        return torch.from_numpy(a.view(np.int32).copy())
    return torch.from_numpy(np.ascontiguousarray(a))


class PinnedBatch:
    """Page-locked host copy of a RegionBatch's arrays: the source of asynchronous H2D copies
    (DeviceBatch.upload_async) when a reader thread hands batches to the GPU one ahead of the kernels."""

    def __init__(self, batch: RegionBatch):
        self.host = batch
        self.t = {f: _as_tensor(getattr(batch, f)).pin_memory() for f in RegionBatch.FIELDS}
        self.nbytes = sum(t.numel() * t.element_size() for t in self.t.values())


class DeviceBatch:
    """A RegionBatch uploaded to HBM once (the benchmark's 'inputs already resident' state)."""

    def __init__(self, batch: RegionBatch, device="cuda:0"):
        self.host = batch
        self.t = {}
        c = _ffi.pv_batch_in()
        c.n_regions = batch.n_regions
        for f in RegionBatch.FIELDS:
            t = _as_tensor(getattr(batch, f)).to(device)
            if t.numel() == 0:
                t = torch.zeros(1, dtype=t.dtype, device=device)
            self.t[f] = t
            setattr(c, f, t.data_ptr())
        self.c = c
        # type_read::hp_tag per read for the haplotag-aware builder (passed next to pv_batch_in); None = untagged
        self.read_hp = None if batch.read_hp is None else torch.from_numpy(batch.read_hp).to(device)
        self.n_reads, self.n_bases, self.n_cigar = batch.n_reads, batch.n_bases, batch.n_cigar
        self.n_ref_bytes = int(batch.ref.shape[0])
        self.max_region_len = batch.max_region_len

    def upload_async(self, pinned: PinnedBatch, stream: "torch.cuda.Stream"):
        """overwrite the device arrays with another batch of IDENTICAL array sizes, asynchronously on `stream`
        (PCIe copies from page-locked memory; the caller orders the kernels behind them with an event)"""
        with torch.cuda.stream(stream):
            for f, t in self.t.items():
                src = pinned.t[f]
                if src.numel() == 0:
                    continue
                assert src.shape == t.shape, (f, src.shape, t.shape)
                t.copy_(src, non_blocking=True)


class DeviceOut:
    """Caller-owned output arrays of pv_batch_out in HBM. `images` may alias a larger window buffer."""

    def __init__(self, capacity: int, str_capacity: int, device="cuda:0", images: torch.Tensor = None):
        self.capacity, self.str_capacity = int(capacity), int(str_capacity)
        self.region = torch.zeros(capacity, dtype=torch.int32, device=device)
        self.position = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.depth = torch.zeros(capacity, dtype=torch.uint8, device=device)
        self.cand_freq = torch.zeros(capacity, dtype=torch.uint8, device=device)
        # [capacity,33,26]; the haplotag-aware builder writes [capacity,21,48] (pass such a tensor as `images`)
        self.images = images if images is not None else torch.zeros((capacity, 33, 26), dtype=torch.int8, device=device)
        assert self.images.is_contiguous() and self.images.shape[0] >= capacity
        self.cand_str = torch.zeros(str_capacity, dtype=torch.uint8, device=device)
        self.cand_off = torch.zeros(capacity + 1, dtype=torch.int64, device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        c = _ffi.pv_batch_out()
        c.capacity, c.str_capacity = self.capacity, self.str_capacity
        c.region, c.position = self.region.data_ptr(), self.position.data_ptr()
        c.depth, c.cand_freq = self.depth.data_ptr(), self.cand_freq.data_ptr()
        c.images, c.images_i32 = self.images.data_ptr(), None
        c.cand_str, c.cand_off = self.cand_str.data_ptr(), self.cand_off.data_ptr()
        self.c = c

    def n_out(self) -> int:
        return int(self.counts[0].item())

    def status(self) -> int:
        return int(self.counts[2].item())


class DevicePolishOut:
    """Caller-owned chunk arrays of pv_polish_out in HBM (the polisher's image batches, input of forward_p2_dev)."""

    def __init__(self, chunk_capacity: int, seq_length: int = 1000, seq_overlap: int = 50, device="cuda:0", depth: bool = False,
                 counts: bool = False):
        """counts: also carry the raw counts plane uint16 [chunk_capacity, seq_length, 10] (pv_polish_out.counts), which the
        builder fills and pv_polish_edits_evidence_dev reads (as int16 bits, like depth).
        depth: also carry the read-depth plane uint16 [chunk_capacity, seq_length] (pv_polish_out.depth), which the
        builder fills and pv_polish_mask_low_depth_dev reads; without it the struct's pointer is null and nothing changes"""
        self.capacity, self.seq_length, self.seq_overlap = int(chunk_capacity), int(seq_length), int(seq_overlap)
        self.images = torch.zeros((chunk_capacity, seq_length, 10), dtype=torch.uint8, device=device)
        self.position = torch.zeros((chunk_capacity, seq_length), dtype=torch.int64, device=device)
        self.index = torch.zeros((chunk_capacity, seq_length), dtype=torch.int32, device=device)
        self.region = torch.zeros(chunk_capacity, dtype=torch.int32, device=device)
        self.chunk_id = torch.zeros(chunk_capacity, dtype=torch.int32, device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        c = _ffi.pv_polish_out()
        c.chunk_capacity, c.row_capacity = self.capacity, 0
        c.images, c.position, c.index = self.images.data_ptr(), self.position.data_ptr(), self.index.data_ptr()
        c.region, c.chunk_id = self.region.data_ptr(), self.chunk_id.data_ptr()
        c.flat_images = c.flat_position = c.flat_index = c.region_row_off = None
        # (an int16 tensor that holds the plane's uint16 bits: torch's unsigned 16-bit type has creation and copies only)
        self.depth = torch.zeros((chunk_capacity, seq_length), dtype=torch.int16, device=device) if depth else None
        c.depth = self.depth.data_ptr() if depth else None
        self.row_counts = torch.zeros((chunk_capacity, seq_length, 10), dtype=torch.int16, device=device) if counts else None
        c.counts = self.row_counts.data_ptr() if counts else None
        self.c = c

    def n_chunks(self) -> int:
        return int(self.counts[0].item())

    def status(self) -> int:
        return int(self.counts[2].item())

    def depth_numpy(self, n: int) -> np.ndarray:
        """the depth plane of the first n chunks on the host, uint16 [n, seq_length]"""
        return self.depth[:n].cpu().numpy().view(np.uint16)

    def row_counts_numpy(self, n: int) -> np.ndarray:
        """the counts plane of the first n chunks on the host, uint16 [n, seq_length, 10]"""
        return self.row_counts[:n].cpu().numpy().view(np.uint16)

    def set_row_counts(self, counts: np.ndarray):
        """a host counts plane uint16 [n, seq_length, 10] into the first n chunks"""
        self.row_counts[:len(counts)].copy_(torch.from_numpy(np.ascontiguousarray(counts, np.uint16).view(np.int16)))

    def set_depth(self, depth: np.ndarray):
        """a host depth plane uint16 [n, seq_length] into the first n chunks"""
        self.depth[:len(depth)].copy_(torch.from_numpy(np.ascontiguousarray(depth, np.uint16).view(np.int16)))


class DeviceSelectOut:
    """Caller-owned output arrays of pv_select_out in HBM (the reads of one haplotype, `polish -hp`). `fill` (a byte value)
    presets every array, for tests that look at what a call left alone."""

    def __init__(self, n_regions: int, read_capacity: int, base_capacity: int, cigar_capacity: int, device="cuda:0",
                 want_hp: bool = True, want_src: bool = True, fill: int = None):
        self.n_regions = int(n_regions)
        self.read_capacity, self.base_capacity, self.cigar_capacity = int(read_capacity), int(base_capacity), int(cigar_capacity)
        nr, nb, nc = self.read_capacity, self.base_capacity, self.cigar_capacity

        def buf(n, dtype):
            t = torch.empty(max(int(n), 1), dtype=dtype, device=device)
            if fill is not None:
                t.view(torch.uint8).fill_(int(fill))
            return t
        self.t = dict(read_off=buf(self.n_regions + 1, torch.int64), read_pos=buf(nr, torch.int64),
                      read_flags=buf(nr, torch.uint8), read_mapq=buf(nr, torch.uint8), base_off=buf(nr + 1, torch.int64),
                      bases=buf(nb, torch.uint8), quals=buf(nb, torch.uint8), cigar_off=buf(nr + 1, torch.int64),
                      cigar=buf(nc, torch.int32))
        self.read_hp = buf(nr, torch.int32) if want_hp else None
        self.src_read = buf(nr, torch.int64) if want_src else None
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)
        c = _ffi.pv_select_out()
        c.read_capacity, c.base_capacity, c.cigar_capacity = nr, nb, nc
        for f, t in self.t.items():
            setattr(c, f, t.data_ptr())
        c.read_hp = self.read_hp.data_ptr() if want_hp else None
        c.src_read = self.src_read.data_ptr() if want_src else None
        self.c = c

    def fits(self, n_regions: int, n_reads: int, n_bases: int, n_cigar: int) -> bool:
        return (self.n_regions >= n_regions and self.read_capacity >= n_reads and self.base_capacity >= n_bases
                and self.cigar_capacity >= n_cigar)


class SelectedDeviceBatch:
    """a device batch whose read arrays are a DeviceSelectOut's (the reads of one haplotype) and whose region arrays are the
    input's: what the realigner and the builders take in place of the DeviceBatch it was selected from"""

    def __init__(self, db, sel: DeviceSelectOut, n_reads: int, n_bases: int, n_cigar: int):
        c = _ffi.pv_batch_in()
        for f, _ in _ffi.pv_batch_in._fields_:
            setattr(c, f, getattr(db.c, f))
        for f, t in sel.t.items():
            setattr(c, f, t.data_ptr())
        self.c, self._keep = c, (db, sel)
        self.read_hp = sel.read_hp
        self.n_reads, self.n_bases, self.n_cigar = int(n_reads), int(n_bases), int(n_cigar)
        self.n_ref_bytes, self.max_region_len = db.n_ref_bytes, db.max_region_len
        self.t = db.t
