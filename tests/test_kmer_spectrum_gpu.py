"""pv_kmer_spectrum and its device forms against the rule's restatement (tests/kmer_spectrum_ref.py): ro_hist, the spectrum and
the assembly's counters are compared for equality (they are integers), at the smallest shapes where the kernels can go wrong:
the count tile and its halo, read borders, the parts, the cap, a probe chain that wraps past the table's end, a nearly full and
an overfull table, the flush's reset, every status, and a replay as one graph."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmer_qv_ref as R  # noqa: E402
import kmer_spectrum_ref as S  # noqa: E402

from pepper_thesis_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, MIN_SLOTS = _ffi.PV_KMER_TILE, _ffi.PV_KMER_READS_MIN_SLOTS
E, L, CAPACITY = _ffi.PV_ERR_INVALID, _ffi.PV_ERR_LIMIT, _ffi.PV_ERR_CAPACITY
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes())


def rc(s):
    return bytes(s).translate(_COMP)[::-1]


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return off


def kmer_of(x, k):
    return bytes(b"ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


class Dev:
    """the device buffers of the device calls; ro_hist and the spectrum accumulate, so they start at 0"""

    def __init__(self, ctx, contigs, k, cap=1 << 30, slots=MIN_SLOTS, build=True, init=True):
        import torch
        self.torch, self.ctx, self.contigs, self.k, self.cap, self.slots, self.n = torch, ctx, contigs, k, cap, slots, len(contigs)
        off = offsets(contigs)
        self.N = int(off[-1])
        self.need = ctx.kmer_table_bytes(off)
        self.A = torch.from_numpy(np.frombuffer(b"".join(contigs) + b"\0", np.uint8).copy()).cuda()
        self.ao = torch.from_numpy(off).cuda()
        self.table = torch.zeros(self.need + 256, dtype=torch.uint8, device="cuda")
        self.rbytes = ctx.kmer_reads_table_bytes(slots)
        self.rtable = torch.zeros(self.rbytes + 256, dtype=torch.uint8, device="cuda")
        assert self.table.data_ptr() % 256 == 0 and self.rtable.data_ptr() % 256 == 0
        self.ro_hist = torch.zeros(257, dtype=torch.int64, device="cuda")
        self.spec = torch.zeros(4 * 256 + 1, dtype=torch.int64, device="cuda")
        self.bcnt, self.fcnt, self.scnt = (torch.full((n,), 7, dtype=torch.int64, device="cuda") for n in (4, 5, 3))
        self.keep = []
        torch.cuda.synchronize()
        if build:
            self.build()
        if init:
            self.init()

    def build(self, table_bytes=None, stream=0):
        self.ctx.kmer_table_build_dev(self.A.data_ptr(), self.ao.data_ptr(), self.n, self.k, self.cap, self.table.data_ptr(),
                                      self.need if table_bytes is None else table_bytes, self.bcnt.data_ptr(), stream=stream)

    def init(self, slots=None, cap=None, stream=0):
        self.ctx.kmer_reads_table_init_dev(self.rtable.data_ptr(), self.rbytes, self.slots if slots is None else slots,
                                           self.cap if cap is None else cap, stream=stream)

    def stage(self, reads):
        b = self.torch.from_numpy(np.frombuffer(b"".join(reads) + b"\0", np.uint8).copy()).cuda()
        o = self.torch.from_numpy(offsets(reads)).cuda()
        self.torch.cuda.synchronize()
        self.keep.append((b, o))
        return b, o, len(reads), int(sum(len(r) for r in reads))

    def count_all(self, staged, part=0, n_parts=1, rbytes=None, stream=0):
        b, o, n, nb = staged
        self.ctx.kmer_count_reads_all_dev(self.table.data_ptr(), self.need, self.rtable.data_ptr(), self.rbytes if rbytes is None else rbytes,
                                          b.data_ptr(), o.data_ptr(), n, nb, part, n_parts, stream=stream)

    def count(self, staged):
        b, o, n, nb = staged
        self.ctx.kmer_count_reads_dev(self.table.data_ptr(), self.need, b.data_ptr(), o.data_ptr(), n, nb)

    def flush(self, rbytes=None, stream=0):
        """-> {distinct keys, status, dropped, slots} (not read back when a stream is given)"""
        self.ctx.kmer_reads_flush_dev(self.rtable.data_ptr(), self.rbytes if rbytes is None else rbytes, self.ro_hist.data_ptr(),
                                      self.fcnt.data_ptr(), stream=stream)
        if stream:
            return None
        self.ctx.synchronize()
        f = self.fcnt.cpu().numpy().tolist()
        assert f[4] == 7
        return f[:4]

    def spectrum(self, stream=0):
        self.ctx.kmer_spectrum_dev(self.table.data_ptr(), self.need, self.spec.data_ptr(), self.scnt.data_ptr(), stream=stream)

    def every_part(self, staged, n_parts):
        """one counting call and one flush per part -> the flushes' counts"""
        out = []
        for p in range(n_parts):
            self.count_all(staged, p, n_parts)
            out.append(self.flush())
        return out

    def results(self):
        """-> (ro_hist [256], spectrum [4][256], {distinct assembly keys, status}); the spare word behind each is untouched"""
        self.ctx.synchronize()
        ro, sp, sc = (t.cpu().numpy() for t in (self.ro_hist, self.spec, self.scnt))
        assert ro[256] == 0 and sp[1024] == 0 and sc[2] == 7
        return ro[:256], sp[:1024].reshape(4, 256), sc[:2].tolist()

    def slots_now(self):
        """the reads-only table as it lies: (keys uint64 [slots], counts uint32 [slots]) - the layout the header gives"""
        self.ctx.synchronize()
        raw = self.rtable.cpu().numpy()
        return raw[256:256 + 8 * self.slots].view(np.uint64), raw[256 + 8 * self.slots:256 + 12 * self.slots].view(np.uint32)

    def plane(self):
        """the assembly's counters by flat position, through the summary"""
        torch = self.torch
        S_ = sum((len(c) + 31) // 32 for c in self.contigs)
        z = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")  # noqa: E731
        ctg, so, sg, hist, cnt = z(3 * self.n), z(self.n + 1), z(S_), z(256), z(8)
        plane = torch.zeros(self.N + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.ctx.kmer_support_dev(self.table.data_ptr(), self.need, self.ao.data_ptr(), self.n, 1, 32, ctg.data_ptr(), so.data_ptr(), S_,
                                  sg.data_ptr(), 0, 0, hist.data_ptr(), plane.data_ptr(), cnt.data_ptr())
        self.ctx.synchronize()
        assert int(cnt.cpu().numpy()[1]) in (_ffi.PV_OK, CAPACITY)   # (no run record was asked for)
        return plane.cpu().numpy().view(np.uint32)[:self.N].tobytes()


def same(got, want):
    assert np.array_equal(got[0], want[0]), "ro_hist"
    assert np.array_equal(got[1], want[1]), "spectrum"


def check(ctx, contigs, reads, k, cap=1 << 30, slots=MIN_SLOTS, n_parts=1):
    """the host form and the device forms against the restatement -> (ro_hist, spectrum) of the restatement"""
    want = S.spectrum(contigs, reads, k, cap)
    same(ctx.kmer_spectrum(contigs, reads, k, cap, slots, n_parts), want)
    d = Dev(ctx, contigs, k, cap, slots)
    flushes = d.every_part(d.stage(reads), n_parts)
    d.spectrum()
    ro, sp, sc = d.results()
    same((ro, sp), want)
    assert all(f[1:] == [0, 0, slots] for f in flushes) and sum(f[0] for f in flushes) == int(want[0].sum())
    assert sc == [int(want[1].sum()), 0]
    assert d.plane() == b"".join(p.tobytes() for p in R.position_counts(contigs, R.read_counts(reads, k), k, cap))
    return want


@pytest.mark.parametrize("k", [11, 21, 31])
def test_hits_and_misses_at_every_k(hip_ctx, k):
    rng = np.random.default_rng(200 + k)
    a, b, u = seq(rng, 700), seq(rng, 300), seq(rng, k + 6)
    contigs = [a + u + b[:100], b"", b + u + b"N" + rc(u), a[:k - 1], a[50:50 + k].lower()]
    foreign = seq(rng, 400)
    reads = [a[100:600], rc(a[300:700] + u), foreign, rc(foreign[100:300]), foreign[:k], b[:150] + b"N" + foreign[350:], b"", u, u,
             foreign[:k - 1]]
    want = check(hip_ctx, contigs, reads, k)
    assert int(want[0][1]) > 50 and int(want[0][2]) > 100 and int(want[1][:, 0].sum()) > 0
    assert int(want[1][2:].sum()) == 7   # u's k-mers lie in the assembly three times
    check(hip_ctx, contigs, reads, k, n_parts=3)


def test_reads_at_the_count_tile_and_its_halo(hip_ctx):
    k = 21
    rng = np.random.default_rng(21)
    s = seq(rng, 3 * TILE + 100)
    reads = [b"", s[:k - 1], s[5:5 + k], s[:TILE - 1], s[7:7 + TILE], s[:TILE + 1], s[3:3 + TILE + k - 1], b"", s]
    # the assembly holds the middle of s: the k-mers before and behind it are misses, on both sides of every tile border
    check(hip_ctx, [s[TILE - 300:2 * TILE + 40], rc(s[100:100 + 3 * k])], reads, k, slots=16384)


def test_a_read_border_on_every_offset_of_the_halo(hip_ctx):
    k = 11
    rng = np.random.default_rng(22)
    s = seq(rng, 2 * TILE)
    reads, cur = [], 0
    for d in range(k + 1):   # the second read of pair d begins d bytes before a tile's end
        target = (cur // TILE + 1) * TILE - d
        reads += [s[d:d + target - cur], s[TILE - d:TILE - d + 2 * k]]
        cur = target + 2 * k
        assert (cur - 2 * k + d) % TILE == 0
    check(hip_ctx, [s[:TILE // 2], s[TILE + 7:TILE + 600]], reads, k, slots=16384)
    check(hip_ctx, [], reads, k, slots=16384, n_parts=7)


def test_many_reads_of_k_minus_1_bytes_give_no_kmer(hip_ctx):
    k = 21
    rng = np.random.default_rng(23)
    s = seq(rng, TILE + 600)
    reads = [s[i:i + k - 1] for i in range(0, len(s), k - 1)]   # laid end to end they spell s again
    want = check(hip_ctx, [s[:500]], reads, k)
    assert not want[0].any() and int(want[1][0, 0]) == 500 - k + 1 == int(want[1].sum())


def test_other_bytes_at_a_tiles_first_and_last_byte(hip_ctx):
    k = 21
    rng = np.random.default_rng(24)
    s = bytearray(seq(rng, 2 * TILE + 50))
    for i, c in ((0, b"N"), (TILE - 1, b"N"), (TILE, b"R"), (2 * TILE - 1, b"n")):
        s[i:i + 1] = c
    clean = bytes(s).replace(b"N", b"A").replace(b"R", b"C").replace(b"n", b"G")
    want = check(hip_ctx, [clean[TILE - 200:TILE + 200]], [bytes(s)], k, slots=16384)
    # 1 + (k + 1) + k k-mers of the read lie over one of the four bytes and have no key; the assembly's k + 1 over the tiles'
    # border are in no read, its others are hits
    assert int(want[1][0, 0]) == k + 1 and int(want[1][0, 1]) == 400 - k + 1 - (k + 1)
    assert int(want[0][1]) == len(s) - k + 1 - (2 * k + 2) - (400 - k + 1 - (k + 1)) == int(want[0].sum())


def test_both_strands_of_a_kmer_land_in_one_entry(hip_ctx):
    k = 31
    rng = np.random.default_rng(25)
    x, a = seq(rng, k), seq(rng, 200)
    want = check(hip_ctx, [a], [x, rc(x), a[:40], rc(x), x + b"N" + rc(x)], k)
    assert want[0].nonzero()[0].tolist() == [5] and int(want[0][5]) == 1


def test_the_parts_change_nothing_and_the_counters_are_those_of_the_plain_count(hip_ctx):
    k = 21
    rng = np.random.default_rng(26)
    s = seq(rng, 6000)
    contigs = [s[:2500], s[2400:4000] + s[100:300]]
    reads = [s[i:i + 900] for i in range(0, 5200, 370)] + [rc(s[4000:5500]), seq(rng, 800), b"N" * 30]
    plain = Dev(hip_ctx, contigs, k, init=False)
    plain.count(plain.stage(reads))
    planes, outs = [plain.plane()], []
    for n_parts in (1, 3, 7):
        d = Dev(hip_ctx, contigs, k, slots=8192)
        flushes = d.every_part(d.stage(reads), n_parts)
        d.spectrum()
        outs.append(d.results())
        planes.append(d.plane())
        assert all(f[1] == 0 for f in flushes) and (n_parts == 1 or all(f[0] > 0 for f in flushes))
    assert len(set(planes)) == 1
    want = S.spectrum(contigs, reads, k)
    for o in outs:
        same(o, want)
    assert int(want[0].sum()) > 2000 and int(want[1][1].sum()) == (100 - k + 1) + (200 - k + 1)


@pytest.mark.parametrize("cap", [1 << 30, 7])
def test_5000_copies_of_one_kmer_the_assembly_lacks(hip_ctx, cap):
    k = 21
    rng = np.random.default_rng(27)
    x, a = seq(rng, k), seq(rng, 100)
    d = Dev(hip_ctx, [a], k, cap)
    d.count_all(d.stage([x] * 5000))
    keys, counts = d.slots_now()
    at = np.flatnonzero(keys != np.uint64(0xFFFFFFFFFFFFFFFF)).tolist()
    assert at == [S.home_of(R.canon(x), MIN_SLOTS)] and int(keys[at[0]]) == R.canon(x)
    # (a counter is left alone once it has reached the cap: what overshoots is bounded by the lanes in flight, and the flush caps)
    assert int(counts[at[0]]) == 5000 if cap > 5000 else cap <= int(counts[at[0]]) < 5000
    assert int(counts.sum()) == int(counts[at[0]])
    assert d.flush() == [1, 0, 0, MIN_SLOTS]
    ro = d.results()[0]
    assert ro.nonzero()[0].tolist() == [min(cap, 255)] and int(ro.sum()) == 1
    assert np.array_equal(ro, S.spectrum([a], [x] * 5000, k, cap)[0])


def test_a_chain_that_wraps_past_the_end_and_a_load_near_09(hip_ctx):
    k = 11
    rng = np.random.default_rng(28)
    a = seq(rng, 300)
    in_asm = set(S.asm_keys([a], k))
    tail, other, seen = [], [], set(in_asm)
    while len(tail) < 64 or len(other) < 860:   # brute force: one key in 256 has its home in the last four slots
        x = int(rng.integers(0, 1 << (2 * k)))
        x = min(x, R.rc_key(x, k))
        if x in seen:
            continue
        if S.home_of(x, MIN_SLOTS) >= MIN_SLOTS - 4:
            if len(tail) < 64:
                tail.append(x)
                seen.add(x)
        elif len(other) < 860:
            other.append(x)
            seen.add(x)
    d = Dev(hip_ctx, [a], k)
    reads = [kmer_of(x, k) for x in tail] + [rc(kmer_of(x, k)) for x in tail[::2]]
    d.count_all(d.stage(reads))
    keys, counts = d.slots_now()
    taken = np.flatnonzero(keys != np.uint64(0xFFFFFFFFFFFFFFFF)).tolist()
    assert taken == list(range(60)) + list(range(MIN_SLOTS - 4, MIN_SLOTS))   # 64 keys from the last four slots on, around the end
    assert sorted(int(x) for x in keys[taken]) == sorted(tail) and sorted(counts[taken].tolist()) == [1] * 32 + [2] * 32
    more = [kmer_of(x, k) for x in other] + [a[20:200]]
    d.count_all(d.stage(more))
    assert d.flush() == [64 + 860, 0, 0, MIN_SLOTS]   # a load factor of 0.90
    d.spectrum()
    same(d.results()[:2], S.spectrum([a], reads + more, k))


def test_an_overfull_table_is_reported_and_the_memory_serves_again(hip_ctx):
    k = 11
    rng = np.random.default_rng(29)
    a, many = seq(rng, 300), seq(rng, 5000 + k - 1)
    assert len(set(S.asm_keys([many], k)) - set(S.asm_keys([a], k))) > 4000
    d = Dev(hip_ctx, [a], k)
    d.count_all(d.stage([many]))
    f = d.flush()
    assert f[1] == CAPACITY and f[2] > 0 and f[3] == MIN_SLOTS
    assert not d.results()[0].any()   # ro_hist is left alone under that status
    with pytest.raises(_ffi.PepperHipError) as e:
        hip_ctx.kmer_spectrum([a], [many], k)
    assert e.value.code == CAPACITY and "dropped" in str(e.value)
    few = [many[:400], rc(many[200:700]), a[:100]]
    d.build()
    d.init()
    d.count_all(d.stage(few))
    assert d.flush() == [int(S.spectrum([a], few, k)[0].sum()), 0, 0, MIN_SLOTS]
    d.spectrum()
    same(d.results()[:2], S.spectrum([a], few, k))


def test_a_flush_empties_the_table_and_ro_hist_accumulates(hip_ctx):
    k = 21
    rng = np.random.default_rng(30)
    a, u, v = seq(rng, 400), seq(rng, 300), seq(rng, 200)
    d = Dev(hip_ctx, [a], k)
    first, second = [u, u[:100], a[:50]], [v, rc(u[:150]), v]
    d.count_all(d.stage(first))
    one = S.spectrum([a], first, k)[0]
    assert d.flush() == [int(one.sum()), 0, 0, MIN_SLOTS]
    assert np.array_equal(d.results()[0], one)
    assert d.flush() == [0, 0, 0, MIN_SLOTS]   # nothing is left: a second flush adds nothing
    assert np.array_equal(d.results()[0], one)
    keys, counts = d.slots_now()
    assert (keys == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and not counts.any()
    d.count_all(d.stage(second))               # u's k-mers again: counted from 0, in a table of their own pass
    two = S.spectrum([a], second, k)[0]
    assert d.flush() == [int(two.sum()), 0, 0, MIN_SLOTS]
    assert np.array_equal(d.results()[0], one + two)


def test_conservation_of_the_keyed_read_instances(hip_ctx):
    k = 21
    rng = np.random.default_rng(31)
    s = seq(rng, 3000)
    contigs = [s[:1500], s[1000:2000], rc(s[1200:1400])]   # keys held once, twice and three times
    reads = [s[i:i + 700] for i in range(0, 2400, 150)] + [seq(rng, 500), b"ACGTN" * 30]
    ro, sp = check(hip_ctx, contigs, reads, k, slots=4096)
    instances = sum(R.read_counts(reads, k).values())
    c = np.arange(256)
    assert int(ro[255]) == 0 and not sp[:, 255].any() and int((c * ro).sum() + (c * sp).sum()) == instances
    assert sp[1].any() and sp[2].any()


def test_every_status(hip_ctx):
    k = 21
    rng = np.random.default_rng(32)
    a, r = seq(rng, 300), [seq(rng, 200)]
    # a reads-only table that was never initialised counts nothing, in either table
    d = Dev(hip_ctx, [a], k, init=False)
    staged = d.stage(r + [a])
    d.count_all(staged)
    assert d.flush() == [0, E, 0, 0]
    d.spectrum()
    ro, sp, sc = d.results()
    assert not ro.any() and sc == [300 - k + 1, 0] and int(sp[0, 0]) == 300 - k + 1
    # rtable_bytes that contradict the head: 2048 slots in what is said to hold 1024
    d = Dev(hip_ctx, [a], k, slots=2048)
    small = hip_ctx.kmer_reads_table_bytes(1024)
    d.count_all(staged, rbytes=small)
    assert d.flush(rbytes=small) == [0, E, 0, 0]
    assert d.flush() == [0, 0, 0, 2048] and not d.results()[0].any()
    d.count_all(staged)   # and the table is still good
    assert d.flush() == [200 - k + 1, 0, 0, 2048]
    # an assembly table not built PV_OK counts nothing and has no spectrum
    d = Dev(hip_ctx, [a], k, build=False)
    d.build(table_bytes=d.need - 1)
    d.count_all(staged)
    assert d.flush() == [0, 0, 0, MIN_SLOTS]
    d.spectrum()
    ro, sp, sc = d.results()
    assert d.bcnt.cpu().numpy().tolist()[1] == L and sc == [0, E] and not sp.any() and not ro.any()
    # refused by the calls themselves
    d = Dev(hip_ctx, [a], k)
    b, o, n, nb = staged
    bad = [lambda: d.init(slots=1000), lambda: d.init(slots=512), lambda: d.init(slots=2048), lambda: d.init(cap=0),
           lambda: d.init(cap=(1 << 30) + 1), lambda: d.count_all(staged, 1, 1), lambda: d.count_all(staged, 0, 0),
           lambda: d.count_all(staged, -1, 3), lambda: d.count_all(staged, 0, 4097), lambda: d.count_all(staged, rbytes=255),
           lambda: hip_ctx.kmer_reads_table_init_dev(0, d.rbytes, MIN_SLOTS, 5),
           lambda: hip_ctx.kmer_reads_table_init_dev(d.rtable.data_ptr() + 8, d.rbytes, MIN_SLOTS, 5),
           lambda: hip_ctx.kmer_count_reads_all_dev(0, d.need, d.rtable.data_ptr(), d.rbytes, b.data_ptr(), o.data_ptr(), n, nb),
           lambda: hip_ctx.kmer_count_reads_all_dev(d.table.data_ptr(), d.need, 0, d.rbytes, b.data_ptr(), o.data_ptr(), n, nb),
           lambda: hip_ctx.kmer_count_reads_all_dev(d.table.data_ptr(), d.need, d.rtable.data_ptr(), d.rbytes, b.data_ptr(), 0, n, nb),
           lambda: hip_ctx.kmer_reads_flush_dev(d.rtable.data_ptr(), d.rbytes, 0, d.fcnt.data_ptr()),
           lambda: hip_ctx.kmer_reads_flush_dev(d.rtable.data_ptr(), d.rbytes, d.ro_hist.data_ptr(), 0),
           lambda: hip_ctx.kmer_spectrum_dev(d.table.data_ptr(), d.need, 0, d.scnt.data_ptr()),
           lambda: hip_ctx.kmer_spectrum_dev(0, d.need, d.spec.data_ptr(), d.scnt.data_ptr()),
           lambda: hip_ctx.kmer_spectrum([a], r, k=20), lambda: hip_ctx.kmer_spectrum([a], r, cap=0),
           lambda: hip_ctx.kmer_spectrum([a], r, slots=1025), lambda: hip_ctx.kmer_spectrum([a], r, n_parts=0),
           lambda: hip_ctx.kmer_spectrum([a], r, n_parts=4097)]
    for i, call in enumerate(bad):
        with pytest.raises(_ffi.PepperHipError) as e:
            call()
        assert e.value.code == E, i
    for slots in (0, 1023, 1025, 1 << 35):
        with pytest.raises(_ffi.PepperHipError):
            hip_ctx.kmer_reads_table_bytes(slots)
    assert hip_ctx.kmer_reads_table_bytes(1024) == 256 + 12 * 1024 and hip_ctx.kmer_reads_table_bytes(1 << 34) == 256 + 12 * (1 << 34)
    d.count_all(staged)   # none of the refused calls touched the tables
    assert d.flush() == [200 - k + 1, 0, 0, MIN_SLOTS]


def test_empty_input(hip_ctx):
    import ctypes as C
    k = 21
    counts = (C.c_int64 * 8)()
    ro, sp = hip_ctx.kmer_spectrum([], [], k, counts=counts)
    assert not ro.any() and not sp.any() and list(counts) == [0, 0, 0, MIN_SLOTS, 0, 0, 0, 0]
    rng = np.random.default_rng(33)
    a = seq(rng, 100)
    check(hip_ctx, [a, b""], [], k)
    check(hip_ctx, [a], [b"", b""], k)
    want = check(hip_ctx, [b"", b""], [a], k)
    assert int(want[0][1]) == 100 - k + 1
    check(hip_ctx, [], [a, rc(a)], k, n_parts=3)


def test_init_count_flush_and_spectrum_replay_as_one_graph(hip_ctx):
    """one linear chain on the context's stream; between replays the reads change under the same buffers"""
    import torch
    k = 21
    rng = np.random.default_rng(34)
    s = seq(rng, 3000)
    contigs = [s[:1200], s[1100:1800]]
    variants = [s[:2000] + rc(s[1500:2500]), rc(s), s[1000:] + b"NNNN" + s[:996]]
    assert len({len(v) for v in variants}) == 1
    read_off = [0, 1200, 1200, 2100, len(variants[0])]
    cut = lambda v: [v[a:b] for a, b in zip(read_off, read_off[1:])]  # noqa: E731
    d = Dev(hip_ctx, contigs, k, cap=3, slots=4096, build=False, init=False)
    staged = d.stage(cut(variants[0]))
    st = hip_ctx.stream

    def passes():
        d.build(stream=st)
        d.init(stream=st)
        for p in range(2):
            d.count_all(staged, p, 2, stream=st)
            d.flush(stream=st)
        d.spectrum(stream=st)

    def refill(i):
        staged[0][:len(variants[i])].copy_(torch.from_numpy(np.frombuffer(variants[i], np.uint8).copy()))
        for t in (d.ro_hist, d.spec):
            t.zero_()
        for t in (d.fcnt, d.scnt, d.bcnt):
            t.fill_(7)
        torch.cuda.synchronize()

    for i in range(3):
        refill(i)
        passes()
        same(d.results()[:2], S.spectrum(contigs, cut(variants[i]), k, 3))
    with hip_ctx.graph_capture(st) as g:
        passes()
    try:
        for i in (1, 2, 0, 0):
            refill(i)
            g.launch()
            same(d.results()[:2], S.spectrum(contigs, cut(variants[i]), k, 3))
            assert d.fcnt.cpu().numpy().tolist()[1:] == [0, 0, 4096, 7]
    finally:
        g.close()
