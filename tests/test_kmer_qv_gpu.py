"""pv_kmer_support and its device forms against the rule's restatement (tests/kmer_qv_ref.py): every output is compared for
equality (they are integers), at the smallest shapes where the kernels can go wrong: contig and read borders, the count
tile and its halo, the sort span, the directory, the cap, the run capacity, every status, and a replay as one graph."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmer_qv_ref as R  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, SPAN = _ffi.PV_KMER_TILE, _ffi.PV_KMER_SORT_SPAN
NAMES = ("contig counts", "seg_off", "segs", "runs", "hist", "position counts")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off


def same(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)), name


def check(ctx, contigs, reads, k, cap=1 << 30, min_count=1, segment=32):
    want = R.support(contigs, reads, k, cap, min_count, segment)
    got = ctx.kmer_support(contigs, reads, k, cap, min_count, segment)
    same(got, want)
    return want


def test_constants_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pepper_hip.h")).read()
    for name in ("PV_KMER_TILE", "PV_KMER_SORT_SPAN", "PV_KMER_HIST", "PV_KMER_MIN_K", "PV_KMER_MAX_K"):
        assert "#define %s %d\n" % (name, getattr(_ffi, name)) in hdr, name
    assert TILE % 256 == 0


@pytest.mark.parametrize("k", [11, 21, 31])
def test_contig_lengths_other_bytes_and_contig_borders(hip_ctx, k):
    rng = np.random.default_rng(100 + k)
    body = seq(rng, 5 * k)
    every_k = b"".join(body[i:i + k - 1] + b"N" for i in range(0, 4 * k, k))   # an N every k bases: no key anywhere
    u, v, w = seq(rng, 3 * k), seq(rng, 2 * k + 3), seq(rng, k + 5)
    contigs = [b"", seq(rng, k - 1), seq(rng, k), seq(rng, k + 1), b"N" * 40, every_k, body[:3 * k].lower(), u, v, b"", w,
               body[:2 * k] + b"R" + body[2 * k:]]
    # the reads hold the contigs joined end to end: every k-mer across a contig border is a read k-mer, and would be
    # supported if the table wrongly held it
    reads = [b"".join(c.upper() for c in contigs), u + v + w, rc(v + w), body]
    want = check(hip_ctx, contigs, reads, k, min_count=2)
    assert want[0][:, 0].tolist()[:7] == [0, 0, 1, 2, 0, 0, 0]
    assert want[0][4:7, 2].tolist() == [41 - k, len(every_k) - k + 1, 2 * k + 1]


def test_reads_at_the_count_tile_and_its_halo(hip_ctx):
    k = 21
    rng = np.random.default_rng(7)
    s = seq(rng, 3 * TILE + 100)
    reads = [b"", s[:k - 1], s[5:5 + k], s[:TILE - 1], s[7:7 + TILE], s[:TILE + 1], s[3:3 + TILE + k - 1], b"", s]
    want = check(hip_ctx, [s, rc(s[100:100 + 3 * k])], reads, k, segment=1024)
    assert int(want[5][0]) == 3 and int(want[5][5]) == 5


def test_many_reads_of_k_minus_1_bytes_give_no_kmer(hip_ctx):
    k = 21
    rng = np.random.default_rng(8)
    s = seq(rng, TILE + 600)
    reads = [s[i:i + k - 1] for i in range(0, len(s), k - 1)]   # laid end to end they spell s again
    want = check(hip_ctx, [s], reads, k)
    assert int(want[0][0, 1]) == len(s) - k + 1 and int(want[4][0]) == len(s) - k + 1


def test_a_read_border_on_every_offset_of_the_halo(hip_ctx):
    k = 11
    rng = np.random.default_rng(9)
    s = seq(rng, 2 * TILE)
    reads, cur = [], 0
    for d in range(k + 1):   # the second read of pair d begins d bytes before a tile's end
        target = (cur // TILE + 1) * TILE - d
        reads += [s[d:d + target - cur], s[TILE - d:TILE - d + 2 * k]]
        cur = target + 2 * k
        assert (cur - 2 * k + d) % TILE == 0
    check(hip_ctx, [s], reads, k, segment=4096)


def test_other_bytes_at_a_tiles_first_and_last_byte(hip_ctx):
    k = 21
    rng = np.random.default_rng(10)
    s = bytearray(seq(rng, 2 * TILE + 50))
    for i, c in ((0, b"N"), (TILE - 1, b"N"), (TILE, b"R"), (2 * TILE - 1, b"n")):
        s[i:i + 1] = c
    clean = bytes(s).replace(b"N", b"A").replace(b"R", b"C").replace(b"n", b"G")
    want = check(hip_ctx, [clean], [bytes(s)], k, segment=512)
    assert len(want[3]) == 3   # around 0, around the tiles' border, around the second tile's end


@pytest.mark.parametrize("k", [11, 31])
def test_strands_and_duplicates_report_the_full_count(hip_ctx, k):
    rng = np.random.default_rng(11 + k)
    u = seq(rng, k + 4)
    x, y, z, w = (seq(rng, n) for n in (40, 55, 33, 70))
    contigs = [x + u + y + u + z + rc(u), w + u]
    reads = [rc(u)] * 3 + [rc(y)]   # u only as its reverse complement
    want = check(hip_ctx, contigs, reads, k)
    plane = want[5]
    for at in (len(x), len(x + u + y), len(x + u + y + u + z), len(contigs[0]) + len(w)):
        assert plane[at:at + 5].tolist() == [3] * 5, at
    assert plane[len(x + u):len(x + u) + len(y) - k + 1].tolist() == [1] * (len(y) - k + 1)


@pytest.mark.parametrize("k", [11, 21, 31])
@pytest.mark.parametrize("size", [SPAN - 1, SPAN, SPAN + 1, 5 * SPAN // 2 + 3])
def test_k_and_table_sizes_around_the_sort_span(hip_ctx, k, size):
    rng = np.random.default_rng(size * 31 + k)
    a, b = seq(rng, size - size // 3), seq(rng, size // 3)
    reads = [a[10:300], rc(a[200:900]), b, b[:50], seq(rng, 400), a[len(a) - 40:]]
    want = check(hip_ctx, [a, b], reads, k, min_count=2, segment=256)
    assert int(want[0][:, 0].sum()) == size - 2 * (k - 1)


@pytest.mark.parametrize("k", [11, 21])
def test_keys_that_share_their_top_directory_bits(hip_ctx, k):
    rng = np.random.default_rng(50 + k)
    contigs = [b"AAAAAAA" + seq(rng, k - 7) for _ in range(300)]   # canonical keys whose top 12 bits are 0
    contigs += [b"TTTTTTT" + seq(rng, k - 7) for _ in range(40)] + [b"A" * (k + 3), b"T" * k]
    reads = contigs[::3] + [rc(c) for c in contigs[1::3]] + [b"A" * 40]
    want = check(hip_ctx, contigs, reads, k)
    assert all(R.canon(c) >> (2 * k - 12) == 0 for c in contigs[:300])
    assert int(want[0][:, 0].sum()) == 340 + 4 + 1


def test_the_cap_and_min_count_equal_to_it(hip_ctx):
    k = 11
    rng = np.random.default_rng(12)
    u = [seq(rng, k) for _ in range(5)]
    contigs = [u[0] + b"N" + u[1] + b"N" + u[2], u[3] + b"N" + u[4]]
    reads = [u[0]] * 2 + [u[1]] * 3 + [rc(u[2])] * 4 + [u[3]] * 1000
    want = check(hip_ctx, contigs, reads, k, cap=3, min_count=3)
    plane = want[5]
    assert [int(plane[i]) for i in (0, k + 1, 2 * k + 2, 3 * k + 2, 4 * k + 3)] == [2, 3, 3, 3, 0]
    assert want[3].tolist() == [[0, 0, 0], [1, k + 1, k + 1]]
    check(hip_ctx, contigs, reads, k, cap=1, min_count=1)


def test_run_capacity_zero_and_exact(hip_ctx):
    k = 21
    rng = np.random.default_rng(13)
    s = seq(rng, 900)
    a = bytearray(s)
    for p in (100, 400, 401, 700):
        a[p] = ord("A") if a[p] != ord("A") else ord("C")
    contigs, reads = [bytes(a), s[:300]], [s, s[:500]]
    want = R.support(contigs, reads, k, 1 << 30, 1, 64)
    need = len(want[3])
    assert need == 3
    for cap_runs in (0, need - 1):
        counts = (C.c_int64 * 8)()
        out = (np.zeros((2, 3), np.int64), np.zeros(3, np.int64), np.zeros(len(want[2]), np.int64), np.full((cap_runs, 3), 7, np.int64),
               np.zeros(256, np.int64), np.zeros(1200, np.uint32))
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.kmer_support(contigs, reads, k, segment=64, run_capacity=cap_runs, counts=counts, out=out)
        assert e.value.code == _ffi.PV_ERR_CAPACITY and list(counts)[:4] == [0, _ffi.PV_ERR_CAPACITY, need, len(want[2])]
        assert (out[3] == 7).all()   # no run record is written
        same(out[:3] + (want[3],) + out[4:], want)
    same(hip_ctx.kmer_support(contigs, reads, k, segment=64, run_capacity=need), want)
    same(hip_ctx.kmer_support(contigs, reads, k, segment=64), want)


class Dev:
    """the device buffers of the three device calls, outputs filled with 7 where a call is to write"""

    def __init__(self, ctx, contigs, a_off=None, segment=32, run_capacity=64, spare=256):
        import torch
        self.torch, self.ctx, self.n, self.segment = torch, ctx, len(contigs), segment
        true_off = offsets(contigs)
        self.N = int(true_off[-1])
        self.need = ctx.kmer_table_bytes(true_off)
        self.A = torch.from_numpy(np.frombuffer(b"".join(contigs) + b"\0", np.uint8).copy()).cuda()
        self.ao = torch.from_numpy(np.asarray(true_off if a_off is None else a_off, np.int64)).cuda()
        self.table = torch.zeros(self.need + spare, dtype=torch.uint8, device="cuda")
        assert self.table.data_ptr() % 256 == 0
        self.seg_capacity = int(sum((len(c) + segment - 1) // segment for c in contigs))
        self.run_capacity = run_capacity
        full = lambda shape, dt=torch.int64: torch.full(shape, 7, dtype=dt, device="cuda")  # noqa: E731
        self.ctg, self.seg_off, self.segs = full((self.n + 1, 3)), full((self.n + 2,)), full((self.seg_capacity + 1,))
        self.runs, self.hist, self.plane = full((run_capacity + 1, 3)), full((257,)), full((self.N + 1,), torch.int32)
        self.bcnt, self.scnt = full((4,)), full((8,))
        self.keep = []
        torch.cuda.synchronize()

    def build(self, k, cap=1 << 30, table_bytes=None, stream=0):
        self.ctx.kmer_table_build_dev(self.A.data_ptr(), self.ao.data_ptr(), self.n, k, cap, self.table.data_ptr(),
                                      self.need if table_bytes is None else table_bytes, self.bcnt.data_ptr(), stream=stream)

    def stage(self, reads):
        b = self.torch.from_numpy(np.frombuffer(b"".join(reads) + b"\0", np.uint8).copy()).cuda()
        o = self.torch.from_numpy(offsets(reads)).cuda()
        self.torch.cuda.synchronize()
        self.keep.append((b, o))
        return b, o, len(reads), int(sum(len(r) for r in reads))

    def count(self, staged, stream=0):
        b, o, n, nb = staged
        self.ctx.kmer_count_reads_dev(self.table.data_ptr(), self.need, b.data_ptr(), o.data_ptr(), n, nb, stream=stream)

    def support(self, min_count=1, seg_capacity=None, stream=0):
        self.ctx.kmer_support_dev(self.table.data_ptr(), self.need, self.ao.data_ptr(), self.n, min_count, self.segment,
                                  self.ctg.data_ptr(), self.seg_off.data_ptr(), self.seg_capacity if seg_capacity is None else seg_capacity,
                                  self.segs.data_ptr(), self.run_capacity, self.runs.data_ptr(), self.hist.data_ptr(),
                                  self.plane.data_ptr(), self.scnt.data_ptr(), stream=stream)

    def outputs(self):
        """-> (what `same` takes, with the runs cut to the count; the spare entries behind every output; the counts)"""
        self.ctx.synchronize()
        c = self.scnt.cpu().numpy()
        ctg, so, sg, ru, hi = (t.cpu().numpy() for t in (self.ctg, self.seg_off, self.segs, self.runs, self.hist))
        pl = self.plane.cpu().numpy().view(np.uint32)
        r = max(int(c[0]), 0)
        spare = np.concatenate([ctg[self.n:].ravel(), so[self.n + 1:], sg[self.seg_capacity:], ru[self.run_capacity:].ravel(), hi[256:],
                                pl[self.N:].astype(np.int64)])
        return (ctg[:self.n], so[:self.n + 1], sg[:self.seg_capacity], ru[:r], hi[:256], pl[:self.N]), spare, c

    def raw(self):
        self.ctx.synchronize()
        return [t.cpu().numpy() for t in (self.ctg[:self.n], self.seg_off[:self.n + 1], self.segs[:self.seg_capacity],
                                          self.runs[:self.run_capacity], self.hist[:256], self.plane[:self.N])]


def test_three_counting_calls_equal_one_in_either_order(hip_ctx):
    k = 21
    rng = np.random.default_rng(14)
    s = seq(rng, 3000)
    contigs = [s[:1800], s[1700:] + seq(rng, 200)]
    batches = [[s[:700], rc(s[300:1400])], [s[1000:2900], b"", s[:k]], [seq(rng, 300), s[1500:1700]] * 2]
    want = R.support(contigs, [r for b in batches for r in b], k, 1 << 30, 2, 32)
    for order in ((0, 1, 2), (2, 0, 1)):
        d = Dev(hip_ctx, contigs)
        d.build(k)
        for i in order:
            d.count(d.stage(batches[i]))
        d.support(min_count=2)
        got, spare, c = d.outputs()
        same(got, want)
        assert (spare == 7).all() and c.tolist() == [len(want[3]), 0, len(want[3]), len(want[2]), len(s) + 300, 0, 0, 0]
        assert d.bcnt.cpu().numpy().tolist() == [int(want[0][:, 0].sum()), 0, -1, d.need]
    d = Dev(hip_ctx, contigs)
    d.build(k)
    d.count(d.stage([r for b in batches for r in b]))
    d.support(min_count=2)
    same(d.outputs()[0], want)
    # the summary may be asked again after more reads
    d.count(d.stage(batches[0]))
    d.support(min_count=2)
    same(d.outputs()[0], R.support(contigs, [r for b in batches for r in b] + batches[0], k, 1 << 30, 2, 32))


def poisoned(d, plane=True):
    raw = d.raw()
    assert all((x == -1).all() for x in raw[:5])
    assert (raw[5] == -1).all() if plane else (raw[5] == 7).all()


def test_every_status_and_its_poison(hip_ctx):
    k = 21
    rng = np.random.default_rng(15)
    contigs = [seq(rng, 300), seq(rng, 200), seq(rng, 100)]
    reads = [contigs[0], contigs[2]]
    E, L = _ffi.PV_ERR_INVALID, _ffi.PV_ERR_LIMIT
    # offsets that decrease: the first bad contig is named; the summary of such a table is refused and poisoned
    d = Dev(hip_ctx, contigs, a_off=[0, 300, 250, 600])
    d.build(k)
    d.count(d.stage(reads))
    d.support()
    hip_ctx.synchronize()
    assert d.bcnt.cpu().numpy().tolist()[:3] == [0, E, 1]
    assert d.scnt.cpu().numpy().tolist() == [0, E, 0, 0, 0, 0, 0, 0]
    poisoned(d, plane=False)
    # a summed length of 2^31: nothing of A is read
    d = Dev(hip_ctx, contigs, a_off=[0, 300, 500, 1 << 31])
    d.build(k)
    d.support()
    hip_ctx.synchronize()
    b = d.bcnt.cpu().numpy().tolist()
    assert b[:3] == [0, L, -1] and b[3] > 20 * (1 << 31)
    assert d.scnt.cpu().numpy().tolist()[:2] == [0, E]
    # a table below the need, by one byte and by almost all of it
    for short in (1, None):
        d = Dev(hip_ctx, contigs)
        d.build(k, table_bytes=d.need - 1 if short else hip_ctx.kmer_table_bytes(np.zeros(1, np.int64)))
        d.count(d.stage(reads))
        d.support()
        hip_ctx.synchronize()
        assert d.bcnt.cpu().numpy().tolist() == [0, L, -1, d.need]
        assert d.scnt.cpu().numpy().tolist()[:2] == [0, E]
        poisoned(d)
    d = Dev(hip_ctx, contigs)
    with pytest.raises(_ffi.PepperHipError) as e:   # not even a head
        d.build(k, table_bytes=512)
    assert e.value.code == L
    hip_ctx.synchronize()
    assert d.bcnt.cpu().numpy().tolist()[:3] == [0, L, -1]
    # a good table: min_count above its cap, too few segment slots, offsets of another assembly
    d = Dev(hip_ctx, contigs)
    d.build(k, cap=5)
    d.count(d.stage(reads))
    d.support(min_count=6)
    hip_ctx.synchronize()
    assert d.scnt.cpu().numpy().tolist()[:5] == [0, E, 0, d.seg_capacity, 600]
    poisoned(d)
    d.support(min_count=5, seg_capacity=d.seg_capacity - 1)
    hip_ctx.synchronize()
    assert d.scnt.cpu().numpy().tolist()[:5] == [0, L, 0, d.seg_capacity, 600]
    other = Dev(hip_ctx, [contigs[0], contigs[1], contigs[2] + b"A"])
    other.table = d.table
    other.need = d.need
    other.support(min_count=5)
    hip_ctx.synchronize()
    assert other.scnt.cpu().numpy().tolist()[:2] == [0, E]
    poisoned(other)
    d.support(min_count=5)   # and the table is still good
    same(d.outputs()[0], R.support(contigs, reads, k, 5, 5, 32))
    # refused by the calls themselves
    for kw in (dict(k=20), dict(k=9), dict(k=33), dict(cap=0), dict(cap=(1 << 30) + 1), dict(min_count=0), dict(segment=48),
               dict(segment=0)):
        with pytest.raises(_ffi.PepperHipError) as e:
            hip_ctx.kmer_support(contigs, reads, **kw)
        assert e.value.code == E, kw
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.kmer_table_build_dev(0, d.ao.data_ptr(), 3, k, 5, d.table.data_ptr(), d.need, d.bcnt.data_ptr())
    assert e.value.code == E
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.kmer_count_reads_dev(0, d.need, d.A.data_ptr(), d.ao.data_ptr(), 3, 600)
    assert e.value.code == E
    # the host form checks the offsets itself, with the same status and poison
    counts = (C.c_int64 * 8)()
    out = [np.full(s, 7, np.int64) for s in ((2, 3), (3,), (4,), (5, 3), (256,))]
    a_off = np.array([0, 50, 40], np.int64)
    A = np.frombuffer(contigs[0], np.uint8)
    boff = np.zeros(1, np.int64)
    rc_ = hip_ctx.lib.pv_kmer_support(hip_ctx.handle, _ffi.ptr(A), _ffi.ptr(a_off), 2, _ffi.ptr(A), _ffi.ptr(boff), 0, k, 5, 1, 32,
                                      _ffi.ptr(out[0]), _ffi.ptr(out[1]), 4, _ffi.ptr(out[2]), 5, _ffi.ptr(out[3]), _ffi.ptr(out[4]),
                                      None, counts)
    assert rc_ == E and counts[1] == E and counts[5] == 1 and all((x == -1).all() for x in out)


def test_no_contigs_and_no_reads(hip_ctx):
    k = 21
    got = hip_ctx.kmer_support([], [b"ACGT" * 20], k)
    assert got[0].shape == (0, 3) and got[1].tolist() == [0] and len(got[2]) == 0 and len(got[3]) == 0 and not got[4].any()
    rng = np.random.default_rng(16)
    contigs = [seq(rng, 100), b""]
    want = check(hip_ctx, contigs, [], k)
    assert want[3].tolist() == [[0, 0, 100 - k]] and int(want[4][0]) == 100 - k + 1
    check(hip_ctx, contigs, [b"", b""], k)
    check(hip_ctx, [b"", b""], [contigs[0]], k)
    d = Dev(hip_ctx, [])
    d.build(k)
    d.count(d.stage([contigs[0]]))
    d.support()
    got, spare, c = d.outputs()
    assert (spare == 7).all() and c.tolist() == [0] * 8 and got[1].tolist() == [0] and not got[4].any()
    assert d.bcnt.cpu().numpy().tolist()[:3] == [0, 0, -1]


def test_build_count_and_summary_replay_as_one_graph(hip_ctx):
    """one linear chain on the context's stream; between replays the reads change under the same buffers"""
    import torch
    k = 21
    rng = np.random.default_rng(17)
    s = seq(rng, 2 * SPAN + 700)
    contigs = [s[:SPAN], s[SPAN:]]
    variants = [s[:3000] + rc(s[2500:]), rc(s) + b"N" + s[:499], s[1000:] + b"NNNN" + s[:1496]]
    assert len({len(v) for v in variants}) == 1
    read_off = [0, 2000, 2000, 3000, len(variants[0])]
    cut = lambda v: [v[a:b] for a, b in zip(read_off, read_off[1:])]  # noqa: E731
    d = Dev(hip_ctx, contigs, run_capacity=256)
    staged = d.stage(cut(variants[0]))
    st = hip_ctx.stream

    def passes():
        d.build(k, cap=3, stream=st)
        d.count(staged, stream=st)
        d.support(min_count=2, stream=st)

    def refill(i):
        staged[0][:len(variants[i])].copy_(torch.from_numpy(np.frombuffer(variants[i], np.uint8).copy()))
        for t in (d.ctg, d.seg_off, d.segs, d.runs, d.hist, d.plane, d.scnt, d.bcnt):
            t.fill_(7)
        torch.cuda.synchronize()

    for i in range(3):
        refill(i)
        passes()
        same(d.outputs()[0], R.support(contigs, cut(variants[i]), k, 3, 2, 32))
    with hip_ctx.graph_capture(st) as g:
        passes()
    try:
        for i in (1, 2, 0, 0):
            refill(i)
            g.launch()
            got, spare, _ = d.outputs()
            same(got, R.support(contigs, cut(variants[i]), k, 3, 2, 32))
            assert (spare == 7).all()
    finally:
        g.close()
