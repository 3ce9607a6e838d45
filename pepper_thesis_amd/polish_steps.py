"""The polisher step by step through files: `make_images`, `call_consensus` and `stitch` (pepper/pepper.py:287-306).

`polish` (polish.py) runs the three on the device without files. These are the reference's separate sub-commands, writing and
reading its two HDF5 formats (hdf5io.PolishImageStore / PolishPredictionStore), so that images or predictions can move between
machines, be kept, be re-stitched, or be handed to / taken from the reference's own sub-commands:

  make_images:    BAM + draft -> <output_dir>/pepper_hp_images_thread_<k>_<timestamp>.hdf, k < -t (ImageGenerationUI.py:198).
                  The regions of `polish` (polish.polish_work), read on reader threads, [realigned,] built on the device through
                  the chain of `polish` (polish.polish_pieces), the chunk arrays read back; region i goes to file i % -t.
  call_consensus: image files -> <output_dir>/pepper_prediction_<device id>.hdf. The *.hdf files of -i with a `summaries`
                  group, in sorted name order; file i goes to caller i % callers; a caller runs pv_rnn_forward_p2 on launches
                  of up to -bs chunks and writes the labels as `bases` and the reference's phred_score. Several -d_ids start
                  one rank per id (polish_rank's plan, launcher and supervisor); a repeated id gets `_<rank>` on later ranks.
                  --qualities: phred_score holds the row qualities instead (pv_polish_row_qual: every row, 0..93).
  stitch:         prediction files -> <output_file>_pepper_polished.fa (perform_stitch.py:39-84, Stitch.py:37-128). Every
                  contig's regions gathered from all files, laid out as pv_polish_stitch requires and stitched by that kernel.
                  --qualities: phred_score is stitched beside the bases (pv_polish_stitch_qual) into
                  <output_file>_pepper_polished.fq, the FASTQ of `polish --qualities`.

Every file is written under a temporary name and renamed when complete; a failing step leaves nothing under a final name.
"""
import argparse
import os
import re
import sys
import time
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _ffi
from .polish import log, natural_key

SEQ_LENGTH = 1000
SEQ_OVERLAP = 50            # ImageSizeOptions.SEQ_OVERLAP
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
STITCH_CHUNKS = 16384       # chunks per stitch launch (about 13 KB of host arrays each); launches split at region boundaries

# phred_score of predict_distributed_gpu.py:96-104, which applies -10 log10(1 - label / count) to the argmax LABEL with
# count 1 on the SEQ_OVERLAP columns at either end of a chunk and 2 on the others; inf -> 100, NaN and -0.0 -> 0 (astype(uint8)
# on x86), 3.0103 -> 3. Rows: count 1, count 2; columns: labels 0..4.
PHRED_TABLE = np.array([[0, 100, 0, 0, 0],
                        [0, 3, 100, 0, 0]], dtype=np.uint8)


def phred_scores(labels: np.ndarray) -> np.ndarray:
    """labels uint8 [B, L] in 0..4 -> the reference's phred_score uint8 [B, L]"""
    labels = np.asarray(labels)
    L = labels.shape[-1]
    count = np.full(L, 2, np.intp)
    count[:SEQ_OVERLAP] = 1
    count[L - SEQ_OVERLAP:] = 1
    return PHRED_TABLE[count - 1, labels]


def handle_output_directory(path: str) -> str:
    """UserInterfaceSupport.handle_output_directory (ImageGenerationUI.py:67-80)"""
    if not path.endswith("/"):
        path += "/"
    os.makedirs(path, exist_ok=True)
    return path


def hdf_files(directory: str) -> List[str]:
    """the files of a directory whose name ends in 'hdf' (get_file_paths_from_directory), in sorted name order"""
    return [os.path.join(directory, f) for f in sorted(os.listdir(directory))
            if f[-3:] == "hdf" and os.path.isfile(os.path.join(directory, f))]


def _remove(paths):
    for p in paths:
        try:
            os.remove(p)
        except FileNotFoundError:
            pass


# ---- make_images ------------------------------------------------------------------------------------------------------

class _ImageChain:
    """the chain contract of polish.polish_pieces (run(batch, windows) -> polish.ChainResult, close()) over the builder of
    polish's device chain: region_off are chunk offsets, and `bases` is the list of (image, position, index, chunk_id)"""

    def __init__(self, chain):
        self.chain = chain

    def run(self, batch, windows=None):
        _, n = self.chain.build(batch, windows)
        return self._chunks(n, batch.n_regions)

    def run_decoded(self, dec, windows=None):
        """run for a gpu_decode.DecodedBatch (make_images --gpu_decode)"""
        _, n = self.chain.build_decoded(dec, windows)
        return self._chunks(n, dec.n_regions)

    @property
    def ctx(self):
        return self.chain.ctx

    def _chunks(self, n, n_regions):
        from .polish import ChainResult
        d = self.chain.dout
        region = d.region[:n].cpu().numpy()
        images, position = d.images[:n].cpu().numpy(), d.position[:n].cpu().numpy()
        index, chunk_id = d.index[:n].cpu().numpy(), d.chunk_id[:n].cpu().numpy()
        region_off = np.searchsorted(region, np.arange(n_regions + 1), side="left")   # the builder emits regions ascending
        return ChainResult(region_off, [(images[k], position[k], index[k], int(chunk_id[k])) for k in range(n)])

    def close(self):
        self.chain.close()


def open_image_chain(device: int = 0) -> _ImageChain:
    from .polish import _DeviceChain
    from .runtime import Context
    return _ImageChain(_DeviceChain(Context(device), own_ctx=True))


def make_images(bam: str, fasta: str, region: Optional[str], output_dir: str, threads: int, realign: bool = False,
                chain=None, batch_size: int = 2048, gpu_decode: bool = False) -> List[str]:
    """-> the image files written. chain: an _ImageChain (CPU tests pass a stub), else one on device 0.
    gpu_decode: the device read path of polish.polish_pieces."""
    from . import polish
    from .bamio import BamHandler, FastaHandler
    from .hdf5io import PolishImageStore
    out_dir = handle_output_directory(output_dir)
    work, _ = polish.polish_work(FastaHandler(fasta), BamHandler(bam), region)
    stamp = time.strftime("%m%d%Y_%H%M%S")
    paths = [out_dir + "pepper_hp_images_thread_%d_%s.hdf" % (k, stamp) for k in range(threads)]
    log("TOTAL INTERVALS: %d, IMAGE FILES: %d IN %s" % (len(work), threads, out_dir))
    own = chain is None
    if own:
        chain = open_image_chain(0)
    stores, n_chunks = [], 0
    try:
        stores = [PolishImageStore(p + ".partial", "w") for p in paths]
        T = {}
        for p in polish.polish_pieces(bam, fasta, work, chain, batch_size, threads, realign, T, gpu_decode=gpu_decode):
            w = work[p.index]
            for image, position, index, chunk_id in p.bases:
                stores[p.index % threads].write_chunk(p.contig, w.start, w.end, chunk_id, image, position, index)
            n_chunks += len(p.bases)
        for s in stores:
            s.close()
        for p in paths:
            os.replace(p + ".partial", p)
    except BaseException:
        for s in stores:
            s.close()
        _remove(p + ".partial" for p in paths)
        raise
    finally:
        if own:
            chain.close()
    if polish.decode_report(T):
        log(polish.decode_report(T))
    log("FINISHED IMAGE GENERATION: %d CHUNKS" % n_chunks)
    return paths


def make_images_run(args, chain=None) -> int:
    for what, path in (("BAM", args.bam), ("FASTA", args.fasta)):
        if not os.path.isfile(path):
            sys.stderr.write("ERROR: CAN NOT LOCATE %s FILE.\n" % what)
            return 1
    if args.threads <= 0:
        sys.stderr.write("ERROR: THREADS NEEDS TO BE > 0.\n")
        return 1
    try:
        make_images(args.bam, args.fasta, args.region, args.output_dir, args.threads, bool(args.realign), chain,
                    gpu_decode=bool(getattr(args, "gpu_decode", False)))
    except Exception as e:
        sys.stderr.write("ERROR: make_images: %s: %s; no image file written.\n" % (type(e).__name__, e))
        return 1
    return 0


# ---- call_consensus ---------------------------------------------------------------------------------------------------

def image_files(image_dir: str) -> List[str]:
    """the image files of -i: *.hdf with a `summaries` group, sorted by name (the reference takes listdir order)"""
    from .hdf5io import H5File
    out = []
    for p in hdf_files(image_dir):
        with H5File(p) as f:
            if "summaries" in f:
                out.append(p)
            else:
                log("WARN: NO IMAGES FOUND IN FILE: " + p)
    return out


def prediction_path(out_dir: str, plan, rank: int) -> str:
    """pepper_prediction_<device id>.hdf (predict_distributed_gpu.py:26); a later rank on a repeated id adds _<rank>"""
    d = plan[rank].device
    repeat = any(p.device == d for p in plan[:rank])
    return os.path.join(out_dir, "pepper_prediction_%d%s.hdf" % (d, "_%d" % rank if repeat else ""))


def call_share(files: List[str], out_path: str, caller, batch_size: int, qualities: bool = False) -> int:
    """one caller: the chunks of `files` (file order, chunk groups in name order) through caller.p2_labels in launches of up to
    batch_size -> the prediction file at out_path; -> chunks written (no file when there are none).
    qualities: caller.p2_labels_and_qualities instead, and phred_score holds the row qualities, not the reference's table"""
    from .hdf5io import PolishImageStore, PolishPredictionStore
    tmp = out_path + ".partial"
    store = PolishPredictionStore(tmp, "w")
    n = 0
    try:
        pending = []

        def flush():
            images = np.stack([c["image"] for _, c in pending])
            if qualities:
                try:
                    labels, phred = (np.asarray(a) for a in caller.p2_labels_and_qualities(images))
                except _ffi.PepperHipError as e:
                    if e.code != _ffi.PV_ERR_STATE:
                        raise
                    raise _ffi.PepperHipError(_ffi.PV_ERR_STATE, "P2 labels outside 0..4 for chunks of %s" % pending[0][0]) from None
            else:
                labels = np.asarray(caller.p2_labels(images))
            if labels.shape != images.shape[:2] or labels.max(initial=0) > 4:   # a poisoned P2 call is never written
                raise _ffi.PepperHipError(_ffi.PV_ERR_STATE, "P2 labels outside 0..4 for chunks of %s" % pending[0][0])
            if not qualities:
                phred = phred_scores(labels)
            for k, (_, c) in enumerate(pending):
                store.write_prediction(c["contig"], c["region_start"], c["region_end"], c["chunk_id"], c["position"],
                                       c["index"], labels[k], phred[k])
            pending.clear()

        for path in files:
            with PolishImageStore(path) as s:
                for name in s.summaries():
                    c = s.read_chunk(name)
                    if c["image"].shape != (SEQ_LENGTH, 10) or c["position"].shape != (SEQ_LENGTH,) \
                            or c["index"].shape != (SEQ_LENGTH,):
                        raise ValueError("%s: chunk %s: image %s, position %s, index %s; expected (%d, 10), (%d,), (%d,)"
                                         % (path, name, c["image"].shape, c["position"].shape, c["index"].shape,
                                            SEQ_LENGTH, SEQ_LENGTH, SEQ_LENGTH))
                    pending.append((path, c))
                    n += 1
                    if len(pending) == batch_size:
                        flush()
        if pending:
            flush()
        store.close()
        if n:
            os.replace(tmp, out_path)
        else:
            _remove([tmp])
    except BaseException:
        store.close()
        _remove([tmp])
        raise
    return n


def call_consensus_rank(args, plan, rank: int, open_caller=None, state_dict=None) -> int:
    """rank `rank` of the plan: files i % world == rank -> its prediction file; -> 0 on success"""
    from . import polish
    if open_caller is None:
        open_caller = polish.open_device_chain
    me, world = plan[rank], len(plan)
    try:
        if state_dict is None:
            state_dict = polish.load_polish_model(args.model_path)
        out_dir = handle_output_directory(args.output_dir)
        files = image_files(args.image_dir)[rank::world]
        out_path = prediction_path(out_dir, plan, rank)
        log("[RANK %d/%d] CALLING %d IMAGE FILES ON DEVICE %d%s -> %s"
            % (rank, world, len(files), me.device, " (shared)" if me.shared_device else "", out_path))
        dtype = _ffi.PV_DTYPE_BF16_INPUT_GEMM if args.bf16 else _ffi.PV_DTYPE_F32
        t0 = time.perf_counter()
        caller = open_caller(me.device, me.shared_device, state_dict, dtype)
        try:
            n = call_share(files, out_path, caller, args.batch_size, bool(getattr(args, "qualities", False)))
        finally:
            caller.close()
    except Exception as e:
        sys.stderr.write("ERROR: [RANK %d/%d] call_consensus: %s: %s\n" % (rank, world, type(e).__name__, e))
        return 1
    log("[RANK %d/%d] PREDICTED %d CHUNKS IN %.2f SEC" % (rank, world, n, time.perf_counter() - t0))
    return 0


def consensus_argv(args) -> List[str]:
    argv = ["-i", args.image_dir, "-m", args.model_path, "-o", args.output_dir, "-bs", str(args.batch_size),
            "-t", str(args.threads)]
    if args.device_ids:
        argv += ["-d_ids", args.device_ids]
    if args.bf16:
        argv.append("--bf16")
    if getattr(args, "qualities", False):
        argv.append("--qualities")
    return argv


def call_consensus_run(args, open_caller=None, rank_cmd: Optional[List[str]] = None) -> int:
    """the `call_consensus` command. Several -d_ids: checks here (no GPU API is touched), then one rank per id in fresh child
    processes (`python -m pepper_thesis_amd.polish_steps <options>`, or rank_cmd + the options); any failing rank fails the
    command and the run's prediction files are removed."""
    from . import polish, polish_rank
    if not os.path.isfile(args.model_path):
        sys.stderr.write("ERROR: CAN NOT LOCATE MODEL FILE.\n")
        return 1
    if not os.path.isdir(args.image_dir):
        sys.stderr.write("ERROR: CAN NOT LOCATE IMAGE DIRECTORY.\n")
        return 1
    if args.batch_size <= 0 or args.threads <= 0:
        sys.stderr.write("ERROR: batch_size AND THREADS NEED TO BE > 0.\n")
        return 1
    try:
        plan = polish_rank.plan_ranks(args.device_ids, args.threads, "call_consensus")
        state_dict = polish.load_polish_model(args.model_path)
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        return 2
    out_dir = handle_output_directory(args.output_dir)
    if len(plan) == 1:
        return call_consensus_rank(args, plan, 0, open_caller, state_dict)
    cmd = (rank_cmd or [sys.executable, "-m", "pepper_thesis_amd.polish_steps"]) + consensus_argv(args)
    rc = polish_rank.launch(args, plan, cmd=cmd, what="call_consensus", lost="no prediction file of this run kept")
    if rc != 0:
        _remove(prediction_path(out_dir, plan, r) for r in range(len(plan)))
        return rc
    log("PREDICTION GENERATED SUCCESSFULLY.")
    return 0


# ---- stitch -----------------------------------------------------------------------------------------------------------

class RegionRef(NamedTuple):
    """one region group of a prediction file"""
    start: int
    end: int
    path: str
    contig: str
    name: str


def gather_regions(files: List[str]) -> Dict[str, List[RegionRef]]:
    """every contig's region groups from all files (perform_stitch.py:47-72), each contig's regions sorted by (start, end)
    (Stitch.py:96). A region present in two files is refused: the reference would emit its sequence twice."""
    from .hdf5io import PolishPredictionStore
    by: Dict[str, List[RegionRef]] = {}
    seen: Dict[Tuple[str, str], str] = {}
    for path in files:
        with PolishPredictionStore(path) as s:
            for contig in s.contigs():
                for name in s.regions(contig):
                    if (contig, name) in seen:
                        raise ValueError("region %s of contig %s is in two prediction files: %s and %s"
                                         % (name, contig, seen[(contig, name)], path))
                    seen[(contig, name)] = path
                    start, end = s.region_span(contig, name)
                    by.setdefault(contig, []).append(RegionRef(start, end, path, contig, name))
    for regs in by.values():
        regs.sort(key=lambda r: (r.start, r.end))
    return by


class StitchLayout(NamedTuple):
    """the arrays of one pv_polish_stitch call: regions ascending, a region's chunks contiguous with ids 0..k"""
    position: np.ndarray      # int64 [n, L]
    index: np.ndarray         # int32 [n, L]
    region: np.ndarray        # int32 [n]
    chunk_id: np.ndarray      # int32 [n]
    labels: np.ndarray        # uint8 [n, L]
    region_start: np.ndarray  # int64 [n_regions]
    regions: List[RegionRef]
    chunk_names: List[str]    # [n] the group name of every chunk, for messages
    row_qual: Optional[np.ndarray] = None   # uint8 [n, L] the chunks' phred_score (stitch --qualities)


def _region_chunks(s, ref: RegionRef, qualities: bool = False):
    """a region's chunks in id order 0..k -> [(name, chunk)]; a gap in the ids or a name that is no id is refused.
    qualities: every chunk also holds its phred_score; one that is missing or not uint8 [SEQ_LENGTH] is refused"""
    names = s.chunk_names(ref.contig, ref.name)
    ids = []
    for nm in names:
        if not re.fullmatch(r"[0-9]+", nm):
            raise ValueError("%s: region %s: chunk group %r is not a chunk id" % (ref.path, ref.name, nm))
        ids.append(int(nm))
    order = sorted(range(len(ids)), key=lambda k: ids[k])
    for want, k in enumerate(order):
        if ids[k] != want:
            raise ValueError("%s: region %s: chunk ids %s have a gap at %d" % (ref.path, ref.name, sorted(ids), want))
    out = [(names[k], s.read_chunk(ref.contig, ref.name, names[k])) for k in order]
    if qualities:
        for name, c in out:
            q = s.read_phred(ref.contig, ref.name, name)
            if q is None or q.dtype != np.uint8 or q.shape != (SEQ_LENGTH,):
                raise ValueError("%s: chunk %s/%s/%s: %s; stitch --qualities needs the uint8 [%d] phred_score of "
                                 "call_consensus --qualities"
                                 % (ref.path, ref.contig, ref.name, name,
                                    "no phred_score" if q is None else "phred_score is %s %s" % (q.dtype, list(q.shape)), SEQ_LENGTH))
            c["phred_score"] = q
    return out


def stitch_layouts(regions: List[RegionRef], max_chunks: int = STITCH_CHUNKS, qualities: bool = False):
    """the regions of one contig (sorted) -> StitchLayout per launch of up to max_chunks chunks (more only for a region that is
    larger on its own), split at region boundaries. qualities: the layouts carry row_qual"""
    from .hdf5io import PolishPredictionStore
    stores: Dict[str, PolishPredictionStore] = {}
    try:
        group: List[Tuple[RegionRef, list]] = []
        size = 0
        for ref in regions:
            if ref.path not in stores:
                stores[ref.path] = PolishPredictionStore(ref.path)
            chunks = _region_chunks(stores[ref.path], ref, qualities)
            if group and size + len(chunks) > max_chunks:
                yield _layout(group, qualities)
                group, size = [], 0
            group.append((ref, chunks))
            size += len(chunks)
        if group:
            yield _layout(group, qualities)
    finally:
        for s in stores.values():
            s.close()


def _layout(group, qualities: bool = False) -> StitchLayout:
    n = sum(len(c) for _, c in group)
    rq = np.empty((n, SEQ_LENGTH), np.uint8) if qualities else None
    pos = np.empty((n, SEQ_LENGTH), np.int64)
    idx = np.empty((n, SEQ_LENGTH), np.int32)
    lab = np.empty((n, SEQ_LENGTH), np.uint8)
    region, chunk_id, names = np.empty(n, np.int32), np.empty(n, np.int32), []
    k = 0
    for g, (ref, chunks) in enumerate(group):
        for cid, (name, c) in enumerate(chunks):
            for what, a in (("position", c["position"]), ("index", c["index"]), ("bases", c["bases"])):
                if a.shape != (SEQ_LENGTH,):
                    raise ValueError("%s: region %s, chunk %s: %s has shape %s, expected (%d,)"
                                     % (ref.path, ref.name, name, what, a.shape, SEQ_LENGTH))
            if c["index"].size and (c["index"].min() < INT32_MIN or c["index"].max() > INT32_MAX):
                raise ValueError("%s: region %s, chunk %s: index beyond int32" % (ref.path, ref.name, name))
            pos[k], idx[k], lab[k] = c["position"], c["index"], c["bases"]
            if qualities:
                rq[k] = c["phred_score"]
            region[k], chunk_id[k] = g, cid
            names.append("%s/%s/%s" % (ref.contig, ref.name, name))
            k += 1
    return StitchLayout(pos, idx, region, chunk_id, lab, np.array([r.start for r, _ in group], np.int64), [r for r, _ in group],
                        names, rq)


def stitch_layout_bases(ctx, lay: StitchLayout, qualities: bool = False):
    """pv_polish_stitch on one layout -> (polished bases, None) of every region. A kept label above 4 is refused by the
    kernel (PV_ERR_STATE) and reported with the chunk it is in.
    qualities: pv_polish_stitch_qual with the layout's row_qual -> (bases, raw Phred bytes) of every region."""
    import ctypes as C
    from .polish_summary import PolishOut
    counts = (C.c_int64 * 4)()
    out = PolishOut(None, lay.position, lay.index, lay.region, lay.chunk_id)
    try:
        if qualities:
            roff, seq, qual = ctx.polish_stitch_qual(out, lay.labels, lay.row_qual, lay.region_start, counts=counts)
        else:
            (roff, seq), qual = ctx.polish_stitch(out, lay.labels, lay.region_start, counts=counts), None
    except _ffi.PepperHipError as e:
        bad = int(counts[2])
        if e.code == _ffi.PV_ERR_STATE and 0 <= bad < len(lay.chunk_names):
            ref = lay.regions[int(lay.region[bad])]
            raise ValueError("%s: chunk %s holds a label above 4" % (ref.path, lay.chunk_names[bad])) from None
        raise
    return [(seq[a:b], None if qual is None else qual[a:b]) for a, b in zip(roff[:-1], roff[1:])]


def stitch(input_dir: str, output_file: str, ctx=None, qualities: bool = False) -> str:
    """-> path of the polished FASTA. ctx: a context (made on device 0 at the first launch when None). The FASTA is written
    only after every contig stitched. qualities: and the FASTQ beside it (polish.output_fastq_path), before the FASTA."""
    from .polish import output_fastq_path, write_fasta, write_fastq
    quals: Dict[str, bytes] = {}
    files = hdf_files(input_dir)
    by = gather_regions(files)
    own = None
    seqs: Dict[str, bytes] = {}
    try:
        for contig in sorted(by, key=natural_key):
            log("PROCESSING CONTIG: " + contig)
            parts: List[Tuple[bytes, Optional[bytes]]] = []
            for lay in stitch_layouts(by[contig], qualities=qualities):
                if ctx is None:
                    from .runtime import Context
                    ctx = own = Context(0)
                parts += stitch_layout_bases(ctx, lay, qualities)
            if qualities:
                quals[contig] = b"".join(q for _, q in parts)
            seqs[contig] = b"".join(s for s, _ in parts)
            log("FINISHED PROCESSING %s, POLISHED SEQUENCE LENGTH: %d." % (contig, len(seqs[contig])))
    finally:
        if own is not None:
            own.close()
    path = output_file + "_pepper_polished.fa"
    Path(path).resolve().parent.mkdir(parents=True, exist_ok=True)
    if qualities:
        write_fastq(output_fastq_path(path), seqs, quals)
    write_fasta(path + ".partial", seqs)
    os.replace(path + ".partial", path)
    return path


def stitch_run(args, ctx=None) -> int:
    if not os.path.isdir(args.input_dir):
        sys.stderr.write("ERROR: CAN NOT LOCATE INPUT DIRECTORY.\n")
        return 1
    try:
        path = stitch(args.input_dir, args.output_file, ctx, bool(getattr(args, "qualities", False)))
    except (ValueError, _ffi.PepperHipError) as e:
        sys.stderr.write("ERROR: stitch: %s; no FASTA written.\n" % e)
        return 1
    log("POLISHED FASTA: " + path)
    return 0


def main(argv=None) -> int:
    """one rank of `call_consensus -d_ids a,b,...` (started by call_consensus_run; RANK / WORLD_SIZE from the environment)"""
    from . import pepper, polish_rank
    args = pepper.call_consensus_parser(argparse.ArgumentParser(prog="call_consensus rank")).parse_args(argv)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    plan = polish_rank.plan_ranks(args.device_ids, args.threads, "call_consensus")
    if len(plan) != world or not 0 <= rank < world:
        sys.stderr.write("ERROR: call_consensus rank: RANK=%d, WORLD_SIZE=%d with -d_ids %r: one rank per listed id\n"
                         % (rank, world, args.device_ids))
        return 2
    return call_consensus_rank(args, plan, rank)


if __name__ == "__main__":
    sys.exit(main())
