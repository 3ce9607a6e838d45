"""`polish` on several devices: the launcher (`polish -d_ids a,b,...` with two ids or more) and the rank it starts.

The reference's call_consensus deals its image files over the device ids and starts one caller per id (mp.spawn + a gloo
group). Here regions are independent from the read through to the stitch, so the work shards with no exchange until the end:

  parent (polish.run): checks the inputs, touches no GPU API, starts one fresh child per listed id,
      python -m pepper_thesis_amd.polish_rank <the polish options>
    with RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT in its environment, and waits for all of them. A child
    that exits non-zero or dies on a signal makes the parent stop the others and return non-zero; no rank is restarted.
  rank r: device ids[r]; regions i % world == r of the single-rank region list (polish.polish_work), through the single-rank
    chain (polish.polish_pieces); reader threads max(1, -t // world); context option shared_device = 1 when another rank uses
    the same device. Then ONE exchange over gloo, with a finite timeout:
      1. all-gather of every rank's status: if any rank failed, every rank returns non-zero and no FASTA is written;
      2. all-gather of the counts (pieces, bytes);
      3. padded gathers to rank 0 of the piece table (int64: contig index, region start, length, region index) and the bytes;
      4. rank 0 runs the single-rank merge (polish.write_polished_fasta); the other ranks write nothing.
    About one byte per polished base plus 32 bytes per region move, once. RCCL is not used: it refuses two ranks on one GPU,
    and the payload is small.

Byte identity with the single-rank run holds where the P2 labels of a chunk do not depend on the other chunks of its launch:
with shared_device = 1 (the one-workgroup GRU forms, which a single-rank run gets with PV_SHARED_DEVICE=1) and launches
within one tile-size family (tests/test_polish_ranks_gpu.py).
"""
import os
import socket
import subprocess
import sys
import time
import traceback
from datetime import timedelta
from typing import List, NamedTuple, Optional

MAX_RANKS = 16
EXCHANGE_TIMEOUT_S = 3600.0   # the longest a rank waits in a collective: for the slowest rank to finish its share


class RankPlan(NamedTuple):
    rank: int
    device: int
    shared_device: bool   # another rank of the run uses this device
    threads: int          # reader threads of this rank


def parse_device_ids(device_ids: Optional[str]) -> List[int]:
    if not device_ids:
        return []
    try:
        return [int(d) for d in str(device_ids).split(",") if d.strip() != ""]
    except ValueError:
        raise ValueError("-d_ids %r: expected a comma list of device ids" % device_ids) from None


def plan_ranks(device_ids: Optional[str], threads: int, what: str = "polish") -> List[RankPlan]:
    """-d_ids -> one RankPlan per listed id (rank r on ids[r]); no -d_ids is one rank on device 0. A pure function: no GPU
    API is touched. More than MAX_RANKS ids are refused (ValueError). what: the command, for the message."""
    ids = parse_device_ids(device_ids) or [0]
    if len(ids) > MAX_RANKS:
        raise ValueError("-d_ids lists %d ids: %s starts at most %d ranks" % (len(ids), what, MAX_RANKS))
    world = len(ids)
    return [RankPlan(r, d, ids.count(d) > 1, max(1, int(threads) // world)) for r, d in enumerate(ids)]


def rank_argv(args, plan: List[RankPlan]) -> List[str]:
    """the polish options a rank is started with (-g and -w change nothing and are left out)"""
    argv = ["-b", args.bam, "-f", args.fasta, "-m", args.model_path, "-o", args.output_file, "-t", str(args.threads),
            "-bs", str(args.batch_size), "-d_ids", ",".join(str(p.device) for p in plan)]
    if args.region:
        argv += ["-r", args.region]
    if args.bf16:
        argv.append("--bf16")
    if getattr(args, "realign", False):
        argv.append("--realign")
    if getattr(args, "gpu_decode", False):
        argv.append("--gpu_decode")
    return argv


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _describe(rc: int) -> str:
    return "signal %d" % -rc if rc < 0 else "exit status %d" % rc


def supervise(cmds: List[List[str]], envs: List[dict], poll_s: float = 0.2, what: str = "polish",
              lost: str = "no FASTA written") -> int:
    """start one child per command and wait for all of them -> 0 when every child exits 0. The first child that exits
    non-zero or dies on a signal stops the others (SIGTERM, then SIGKILL after 10 s); its status is returned (1 for a
    signal). Nothing is restarted. what / lost: the command and what its failure leaves out, for the message."""
    from .polish import log
    procs = []
    failed = None
    try:
        for cmd, env in zip(cmds, envs):
            procs.append(subprocess.Popen(cmd, env=env))
        while failed is None:
            live = False
            for r, p in enumerate(procs):
                rc = p.poll()
                if rc is None:
                    live = True
                elif rc != 0:
                    failed = (r, rc)
                    break
            if not live:
                break
            if failed is None:
                time.sleep(poll_s)
    finally:
        stopped = [p for p in procs if p.poll() is None]
        for p in stopped:
            p.terminate()
        for p in stopped:
            try:
                p.wait(timeout=10)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    if failed is not None:
        r, rc = failed
        sys.stderr.write("ERROR: %s: rank %d ended with %s%s; %s.\n"
                         % (what, r, _describe(rc), "; %d other rank(s) stopped" % len(stopped) if stopped else "", lost))
        return rc if rc > 0 else 1
    log("ALL %d RANKS FINISHED" % len(procs))
    return 0


def launch(args, plan: List[RankPlan], cmd: Optional[List[str]] = None, what: str = "polish",
           lost: str = "no FASTA written") -> int:
    """the parent of a multi-device run: one child per plan entry, by default `python -m pepper_thesis_amd.polish_rank`
    with the polish options (cmd: another rank command, the same for every rank; the rank reads RANK / WORLD_SIZE). Touches
    no GPU API (a process that has initialised the GPU must not be forked into ranks)."""
    from .polish import log
    world = len(plan)
    pkg_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if cmd is None:
        cmd = [sys.executable, "-m", "pepper_thesis_amd.polish_rank"] + rank_argv(args, plan)
    port = str(_free_port())
    envs = []
    for p in plan:
        env = dict(os.environ, RANK=str(p.rank), WORLD_SIZE=str(world), LOCAL_RANK=str(p.rank), LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        env["PYTHONPATH"] = pkg_root + (os.pathsep + os.environ["PYTHONPATH"] if os.environ.get("PYTHONPATH") else "")
        envs.append(env)
    log("STARTING %d RANKS ON DEVICES %s" % (world, ",".join(str(p.device) for p in plan)))
    return supervise([cmd] * world, envs, what=what, lost=lost)


def _polish_share(args, me: RankPlan, world: int, open_chain, T: dict):
    """this rank's regions through the chain -> (pieces, the whole region list, FASTA path on rank 0 else None)"""
    from . import _ffi, polish
    from .bamio import BamHandler, FastaHandler
    state_dict = polish.load_polish_model(args.model_path)
    work, T["bases_in"] = polish.polish_work(FastaHandler(args.fasta), BamHandler(args.bam), args.region)
    mine = work[me.rank::world]
    out_path = polish.output_fasta_path(args.output_file) if me.rank == 0 else None
    polish.log("[RANK %d/%d] POLISHING %d OF %d REGIONS ON DEVICE %d%s, %d READER THREADS"
               % (me.rank, world, len(mine), len(work), me.device, " (shared)" if me.shared_device else "", me.threads))
    dtype = _ffi.PV_DTYPE_BF16_INPUT_GEMM if args.bf16 else _ffi.PV_DTYPE_F32
    chain = open_chain(me.device, me.shared_device, state_dict, dtype)
    try:
        pieces = list(polish.polish_pieces(args.bam, args.fasta, mine, chain, args.batch_size, me.threads,
                                           bool(getattr(args, "realign", False)), T,
                                           gpu_decode=bool(getattr(args, "gpu_decode", False))))
    finally:
        chain.close()
    return pieces, work, out_path


def _exchange(dist, rank: int, world: int, pieces, work, out_path) -> Optional[dict]:
    """steps 2-4 of the exchange; -> the sequences on rank 0, None elsewhere"""
    import numpy as np
    import torch
    from . import polish
    from .dist import _gather_padded
    table = torch.tensor([[work[p.index].contig_index, p.start, len(p.bases), p.index] for p in pieces],
                         dtype=torch.int64).reshape(len(pieces), 4)
    blob = np.frombuffer(b"".join(p.bases for p in pieces), dtype=np.uint8)
    data = torch.from_numpy(blob.copy())
    counts = [torch.zeros(2, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(counts, torch.tensor([len(pieces), blob.size], dtype=torch.int64))
    counts = [(int(c[0]), int(c[1])) for c in counts]
    tables = _gather_padded(table, max(max(n for n, _ in counts), 1), 0, world, rank)
    datas = _gather_padded(data, max(max(b for _, b in counts), 1), 0, world, rank)
    if rank != 0:
        return None
    merged = []
    for r in range(world):
        n, nb = counts[r]
        rows, buf = tables[r][:n].tolist(), datas[r][:nb].numpy()
        off = 0
        for ci, start, length, i in rows:
            w = work[i]
            if w.contig_index != ci or w.start != start or i % world != r:
                raise RuntimeError("polish exchange: rank %d sent region %d as (%d, %d); rank 0 has (%d, %d)"
                                   % (r, i, ci, start, w.contig_index, w.start))
            merged.append(polish.Piece(w.contig, start, i, buf[off:off + length].tobytes()))
            off += length
        if off != nb:
            raise RuntimeError("polish exchange: rank %d sent %d bytes for pieces of %d" % (r, nb, off))
        tables[r] = datas[r] = None
    return polish.write_polished_fasta(out_path, merged)


def run(args, open_chain=None, timeout_s: float = EXCHANGE_TIMEOUT_S) -> int:
    """one rank of a multi-device `polish` (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment); -> 0 on
    success. open_chain: polish.open_device_chain by default (CPU tests pass a stub)."""
    import torch.distributed as dist
    from . import polish
    if open_chain is None:
        open_chain = polish.open_device_chain
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    try:
        plan = plan_ranks(args.device_ids, args.threads)
    except ValueError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        return 2
    if len(plan) != world or not 0 <= rank < world:
        sys.stderr.write("ERROR: polish_rank: RANK=%d, WORLD_SIZE=%d with -d_ids %r: one rank per listed id\n"
                         % (rank, world, args.device_ids))
        return 2
    me = plan[rank]
    t0 = time.perf_counter()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=timeout_s))
    try:
        T = {}
        status = ""
        try:
            pieces, work, out_path = _polish_share(args, me, world, open_chain, T)
        except Exception as e:   # reported through the exchange: every rank then fails, none waits for a missing peer
            status = "%s: %s" % (type(e).__name__, e)
            traceback.print_exc()
            sys.stderr.write("ERROR: [RANK %d/%d] %s\n" % (rank, world, status))
        statuses = [None] * world
        dist.all_gather_object(statuses, status)
        bad = [(r, s) for r, s in enumerate(statuses) if s]
        if bad:
            if rank == 0:
                sys.stderr.write("ERROR: polish: %s; no FASTA written.\n"
                                 % "; ".join("rank %d failed (%s)" % (r, s) for r, s in bad))
            return 1
        if polish.decode_report(T):
            polish.log("[RANK %d/%d] %s" % (rank, world, polish.decode_report(T)))
        polish.log("[RANK %d/%d] POLISHED %d REGIONS, %d BASES (%.2f SEC)"
                   % (rank, world, T["regions"], sum(len(p.bases) for p in pieces), time.perf_counter() - t0))
        try:
            seqs = _exchange(dist, rank, world, pieces, work, out_path)
        except Exception as e:
            sys.stderr.write("ERROR: [RANK %d/%d] polish exchange: %s: %s\n" % (rank, world, type(e).__name__, e))
            return 1
        if rank == 0:
            polish.log("POLISHED FASTA: %s (%d RANKS, %d BASES IN %.2f SEC)"
                       % (out_path, world, sum(len(s) for s in seqs.values()), time.perf_counter() - t0))
        return 0
    finally:
        dist.destroy_process_group()


def main(argv=None) -> int:
    import argparse
    from . import cli
    ap = argparse.ArgumentParser(prog="polish_rank", description="one rank of `polish -d_ids a,b,...` (started by polish)")
    return run(cli.polish_parser(ap).parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
