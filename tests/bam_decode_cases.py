"""Cases for the BAM record decode kernels (csrc/bam_decode.hip) and the host side of their direct harness: record streams cut
into made-up blocks, the block / chunk / interval tables of one launch, and what the restatement (bam_decode_ref) expects of
every interval and of a fill. Nothing here needs BGZF, a BAI or a FASTA, and nothing is imported from the package.

Every interval of a case carries a `check` of what it was built to hold, evaluated on the restatement's result: a case whose
check fails is a broken case."""
import struct

import numpy as np

import bam_decode_ref as ref
import bam_writer as bw

CO0, CO_STEP = 1000, 77          # made-up compressed offsets: block i of a group "starts" at CO0 + CO_STEP * i
BIG = (1 << 29) - 1              # a contig length that holds every position used here


def rec(pos, cigar, seq=None, **kw):
    qn = sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    seq = seq if seq is not None else ("ACGTTGCA" * (qn // 8 + 1))[:qn]
    r = dict(tid=0, pos=pos, mapq=60, flag=0, cigar=cigar, seq=seq, qual=[(7 * i + 3) % 60 for i in range(len(seq))], name="r", aux=b"")
    r.update(kw)
    return r


class Stream:
    """records (dicts; `raw` bytes in a dict stand for the record as written) and unrelated bytes (bytes items), end to end,
    cut into blocks at `cuts` (a repeated cut: a block of isize 0; "auto": every 60000 bytes)"""

    def __init__(self, items, cuts=()):
        self.records, self.starts, self.at = [], [], {}
        parts, p = [], 0
        for it in items:
            if isinstance(it, (bytes, bytearray)):
                parts.append(bytes(it))
                p += len(it)
                continue
            b = it["raw"] if it.get("raw") is not None else bw.record_bytes(it)
            self.records.append(it)
            self.starts.append(p)
            self.at[id(it)] = (p, len(b))
            parts.append(b)
            p += len(b)
        self.data, self.size = b"".join(parts), p
        if isinstance(cuts, str):
            cuts = list(range(60000, p, 60000))
        edges = [0] + sorted(cuts) + [p]
        assert edges[1] >= 0 and edges[-2] <= p
        self.start = edges[:-1]
        self.isize = [edges[i + 1] - edges[i] for i in range(len(edges) - 1)]
        assert all(0 <= n <= 65536 for n in self.isize), self.isize
        nb = len(self.isize)
        self.coffset = [CO0 + CO_STEP * i for i in range(nb)]
        self.next_coffset = self.coffset[1:] + [CO0 + CO_STEP * nb]

    def end(self, k):
        return self.starts[k] + self.at[id(self.records[k])][1]

    def voff(self, p):
        """Bgzf::tell at byte p of the stream: a consumed non-empty block reports offset 0 of the next one"""
        if p == 0:
            return self.coffset[0] << 16
        for b, (s, n) in enumerate(zip(self.start, self.isize)):
            if n > 0 and s < p <= s + n:
                return (self.coffset[b] << 16) | (p - s) if p < s + n else self.next_coffset[b] << 16
        raise AssertionError("offset %d outside the stream" % p)

    def records_in(self, beg, end):
        return [r for r, s in zip(self.records, self.starts) if beg <= s < end]


def stream(records, cuts=()):
    return Stream(records, cuts)


class Launch:
    """the tables of one pv_bam_scan_dev call: groups (streams) packed end to end in `data`, intervals in any order"""

    def __init__(self, include_supp=False, min_mapq=0):
        self.supp, self.mq = include_supp, min_mapq
        self.groups, self.ivs = [], []
        self.n_blocks = self.data_bytes = 0

    def group(self, st):
        self.groups.append((st, self.n_blocks, self.data_bytes))
        self.n_blocks += len(st.isize)
        self.data_bytes += st.size
        return len(self.groups) - 1

    def interval(self, gi, tid, rs, re, chunks=None, dropped=0, slots=None, vchunks=None, check=None, name=""):
        """chunks: [beg, end) byte offsets of the stream (record starts); vchunks: the virtual offsets, where the tell rule is
        not what the case wants; slots: record slots (default: exactly the records listed)"""
        st = self.groups[gi][0]
        chunks = [(0, st.size)] if chunks is None else chunks
        exp = ref.decode_interval([st.records_in(b, e) for b, e in chunks], tid, rs, re, self.supp, self.mq)
        if exp["status"] == ref.OK and dropped and not exp["done"]:
            exp["status"] = ref.PAST_PLAN
        vch = vchunks if vchunks is not None else [(st.voff(b), st.voff(e)) for b, e in chunks]
        self.ivs.append(dict(gi=gi, tid=tid, rs=rs, re=re, vchunks=vch, dropped=dropped, slots=exp["n_rec"] if slots is None else slots,
                             exp=exp, check=check, name=name))
        return len(self.ivs) - 1

    def one(self, items, tid, rs, re, cuts=(), **kw):
        """a group of its own with one interval over all of it"""
        return self.interval(self.group(Stream(items, cuts)), tid, rs, re, **kw)

    def tables(self):
        g = self.groups
        t = dict(data=np.frombuffer(b"".join(st.data for st, _, _ in g), np.uint8).copy(), data_bytes=self.data_bytes, n_blocks=self.n_blocks,
                 coffset=np.array([c for st, _, _ in g for c in st.coffset], np.int64),
                 next_coffset=np.array([c for st, _, _ in g for c in st.next_coffset], np.int64),
                 out_off=np.array([off + s for st, _, off in g for s in st.start], np.int64),
                 isize=np.array([n for st, _, _ in g for n in st.isize], np.int32),
                 blk_status=np.zeros(self.n_blocks, np.int32), n_intervals=len(self.ivs), include_supplementary=int(self.supp), min_mapq=self.mq,
                 iv_tid=np.array([iv["tid"] for iv in self.ivs], np.int32), iv_rs=np.array([iv["rs"] for iv in self.ivs], np.int64),
                 iv_re=np.array([iv["re"] for iv in self.ivs], np.int64),
                 iv_blk0=np.array([g[iv["gi"]][1] for iv in self.ivs], np.int64),
                 iv_blk1=np.array([g[iv["gi"]][1] + len(g[iv["gi"]][0].isize) for iv in self.ivs], np.int64),
                 iv_chunk_off=np.concatenate([[0], np.cumsum([len(iv["vchunks"]) for iv in self.ivs])]).astype(np.int64),
                 chunk_beg=np.array([c[0] for iv in self.ivs for c in iv["vchunks"]], np.int64),
                 chunk_end=np.array([c[1] for iv in self.ivs for c in iv["vchunks"]], np.int64),
                 iv_dropped=np.array([iv["dropped"] for iv in self.ivs], np.uint8),
                 iv_rec_off=np.concatenate([[0], np.cumsum([iv["slots"] for iv in self.ivs])]).astype(np.int64))
        t["rec_slots"], t["n_chunks"] = int(t["iv_rec_off"][-1]), int(t["iv_chunk_off"][-1])
        return t

    def reported_voff(self, t, at):
        """the virtual offset the device reports for byte `at` of `data`: in the last block that starts at or before it"""
        b = int(np.searchsorted(t["out_off"], at, side="right")) - 1
        return (int(t["coffset"][b]) << 16) | (at - int(t["out_off"][b]))

    def expected_counts(self, t, i):
        """counts[i] of the scan: {reads kept, bases, CIGAR words, status, offender's virtual offset, detail, detail, records}"""
        iv = self.ivs[i]
        e = iv["exp"]
        at, d1 = -1, 0
        if e["offender"] is not None:
            st, _, off = self.groups[iv["gi"]]
            p, n = st.at[id(e["listed"][e["offender"]])]
            at, d1 = self.reported_voff(t, off + p), n - 4
        return [len(e["reads"]), e["n_bases"], e["n_cigar"], e["status"], at, d1, 0, e["n_rec"]]

    def checks(self):
        """every interval's own check, on the restatement's result"""
        for i, iv in enumerate(self.ivs):
            if iv["check"] is not None:
                assert iv["check"](iv["exp"]), "broken case: interval %d %s" % (i, iv["name"])


def expected_fill(launch, regions):
    """regions: [(interval or None, kept indices or None)]; None as interval or an index outside the kept reads stands for a
    read the fill must refuse -> the output arrays, and `written`: which output reads are written"""
    reads = []
    for i, sel in regions:
        kept = launch.ivs[i]["exp"]["reads"] if i is not None else []
        if i is None:
            reads += [None] * len(sel)
        else:
            reads += kept if sel is None else [kept[k] if k is not None and 0 <= k < len(kept) else None for k in sel]
    n = len(reads)
    nb = [len(r["seq"]) if r else 0 for r in reads]
    nc = [len(r["cigar"]) if r else 0 for r in reads]
    out = dict(read_pos=np.array([r["pos"] if r else 0 for r in reads], np.int64), read_flags=np.array([r["rev"] if r else 0 for r in reads], np.uint8),
               read_mapq=np.array([r["mapq"] if r else 0 for r in reads], np.uint8), read_hp=np.array([r["hp"] if r else 0 for r in reads], np.int32),
               base_off=np.concatenate([[0], np.cumsum(nb)]).astype(np.int64), cigar_off=np.concatenate([[0], np.cumsum(nc)]).astype(np.int64),
               bases=np.frombuffer(b"".join(r["seq"] for r in reads if r), np.uint8), quals=np.frombuffer(b"".join(r["qual"] for r in reads if r), np.uint8),
               cigar=np.array([w for r in reads if r for w in r["cigar"]], np.uint32),
               written=np.array([r is not None for r in reads], bool), read_off=np.concatenate([[0], np.cumsum(
                   [len(launch.ivs[i]["exp"]["reads"]) if sel is None else len(sel) for i, sel in regions])]).astype(np.int64))
    assert n == int(out["read_off"][-1])
    return out


# ---- a. the CIGAR clip at the turn seams -----------------------------------------------------------------------------------

_KINDS = (0, 1, 0, 2, 7, 4, 8, 3)


def _ops(n):
    """n operations of one to ten bases, M-like ones between I / D / S / N; the first and the last are matches"""
    ops = [(_KINDS[k % 8], 1 + (7 * k + 3) % 10) for k in range(n)]
    ops[0], ops[-1] = (0, ops[0][1]), (0, ops[-1][1])
    return ops


def _one_read(n_ops, first_op=None, first_len=None):
    def check(e):
        ok = len(e["reads"]) == 1 and e["status"] == ref.OK
        if ok and n_ops is not None:
            ok = len(e["reads"][0]["cigar"]) == n_ops
        if ok and first_op is not None:
            ok = e["reads"][0]["cigar"][0] == (first_len << 4) | first_op
        return ok
    return check


def _nothing(n_rec=1, status=ref.OK):
    return lambda e: e["n_rec"] == n_rec and not e["reads"] and e["status"] == status


def clip_launch():
    L = Launch()
    P = 1000
    for n in (63, 64, 65, 127, 128, 129, 193):
        ops = _ops(n)
        r = rec(P, ops)
        g = L.group(Stream([r]))
        rl = bw.ref_len(ops)
        L.interval(g, 0, P + rl // 3, P + 2 * rl // 3, check=_one_read(None), name="%d ops, window inside" % n)
        L.interval(g, 0, P, P + rl // 2, check=lambda e: len(e["reads"]) == 1 and e["reads"][0]["pos"] == P, name="%d ops, from the first base" % n)
        L.interval(g, 0, P + rl // 2, P + rl - 1, check=lambda e, ops=ops: len(e["reads"]) == 1 and e["reads"][0]["cigar"][-1] & 0xF == 0
                   and e["reads"][0]["cigar"][-1] >> 4 <= ops[-1][1], name="%d ops, to the last base" % n)
        L.interval(g, 0, P - 5, P + rl + 5, check=_one_read(n), name="%d ops, whole" % n)
    # leading operations wholly left of the window: the first kept match is operation `lead`
    for lead in (62, 63, 64, 65, 127, 128):
        front = [((0, 2, 1)[k % 3], 1) for k in range(lead)]
        for nxt in (1, 4, 2, 3):
            ops = front + [(0, 5), (nxt, 3), (0, 4)]
            g = L.group(Stream([rec(P, ops)]))
            s0 = P + bw.ref_len(front)
            for i0 in (0, 2):
                L.interval(g, 0, s0 + i0, s0 + 40, name="first kept match is operation %d, then %d, i0 %d" % (lead, nxt, i0),
                           check=lambda e, s0=s0, i0=i0, nxt=nxt: len(e["reads"]) == 1 and e["reads"][0]["pos"] == s0 + i0
                           and e["reads"][0]["cigar"] == [((5 - i0) << 4), (3 << 4) | nxt, 4 << 4])
    # `stop` around the last base of lane 63's operation (operation 63, and 127 one turn on)
    for last in (63, 127):
        for nxt in ((1, 3), (2, 3), (0, 3)):
            ops = [(0, 1)] * last + [(0, 4), nxt, (0, 2)]
            g = L.group(Stream([rec(P, ops)]))
            stop = P + last + 3
            L.interval(g, 0, P, stop - 1, check=_one_read(last + 1), name="stop one base before the end of operation %d" % last)
            L.interval(g, 0, P, stop, name="stop on the last base of operation %d, then %r" % (last, nxt),
                       check=lambda e, last=last: _one_read(last + 1)(e) and e["reads"][0]["cigar"][-1] == 4 << 4)
            L.interval(g, 0, P, stop + 1, name="stop one base after operation %d, then %r" % (last, nxt),
                       check=lambda e, last=last, nxt=nxt: len(e["reads"]) == 1 and len(e["reads"][0]["cigar"]) == last + (3 if nxt[0] == 1 else 2))
    for op in (2, 3):   # a D and an N cut at `stop`
        L.one([rec(P, [(0, 5), (op, 10), (0, 5)])], 0, P, P + 8, name="%d cut at stop" % op,
              check=lambda e, op=op: len(e["reads"]) == 1 and e["reads"][0]["cigar"] == [5 << 4, (4 << 4) | op])
    for op in (1, 2):   # an I and a D at the window's first position, ahead of the first kept match: neither is kept
        L.one([rec(P, [(0, 5), (op, 3), (0, 5)])], 0, P + 5, P + 100, name="%d at the window's first position" % op,
              check=lambda e, op=op: len(e["reads"]) == 1 and e["reads"][0]["cigar"] == [5 << 4] and e["reads"][0]["pos"] == P + (5 if op == 1 else 8))
    odd = [(0, 3), (0, 0), (1, 0), (2, 0), (5, 2), (6, 2)] + [(c, 2) for c in range(9, 16)] + [(0, 3)]
    L.one([rec(P, odd)], 0, P - 10, P + 100, name="zero lengths and codes 5, 6, 9..15",
          check=lambda e: len(e["reads"]) == 1 and e["reads"][0]["cigar"] == [3 << 4, 3 << 4] and len(e["reads"][0]["seq"]) == 6)
    skip = (1 << 28) - 1
    g = L.group(Stream([rec(10, [(0, 3), (3, skip), (0, 3)])]))
    L.interval(g, 0, 0, 100, name="N of 2^28 - 1 cut at stop", check=lambda e: len(e["reads"]) == 1 and e["reads"][0]["cigar"] == [3 << 4, (88 << 4) | 3])
    L.interval(g, 0, 13 + skip, 13 + skip + 50, name="behind an N of 2^28 - 1", check=lambda e: e["reads"] and e["reads"][0]["pos"] == 13 + skip)
    L.one([rec(P, [(4, 3), (1, 4)])], 0, P - 10, P + 10, name="only I / S", check=_nothing())
    L.one([rec(P, [(2, 5)], seq="")], 0, P - 10, P + 10, name="only D, l_seq 0", check=_nothing())
    g = L.group(Stream([rec(P, [(0, 5)])]))
    L.interval(g, 0, P - 50, P + 1, name="pos == re - 1", check=lambda e: len(e["reads"]) == 1 and len(e["reads"][0]["seq"]) == 2)   # (the window's last base is re itself)
    L.interval(g, 0, P - 50, P, name="pos == re", check=lambda e: e["n_rec"] == 0 and e["done"])
    # CIGAR longer than SEQ
    longer = lambda e: e["status"] == ref.CIGAR_LONGER and e["offender"] == 0 and not e["reads"]   # noqa: E731
    L.one([rec(P, [(0, 10)], seq="ACGTACGT")], 0, P - 10, P + 100, name="excess in the window, turn 0", check=longer)
    L.one([rec(P, [(0, 1)] * 70, seq="ACGTTGCA" * 8 + "AC")], 0, P - 10, P + 100, name="excess in the window, turn 1", check=longer)
    L.one([rec(P, [(0, 5), (1, 4)], seq="ACGTACG")], 0, P - 10, P + 100, name="excess in a kept I behind a good match", check=longer)
    L.one([rec(P, [(0, 20)], seq="ACGTACGTAC")], 0, P + 30, P + 100, name="excess left of the window", check=_nothing())
    L.one([rec(P, [(0, 20)], seq="ACGTACGTAC")], 0, P - 10, P + 5, name="excess right of the window",
          check=lambda e: e["status"] == ref.OK and len(e["reads"]) == 1 and len(e["reads"][0]["seq"]) == 6)
    many = [rec(P + k, [(0, 4)], seq="AC" if k in (10, 270) else None) for k in range(300)]
    L.one(many, 0, P - 10, P + 1000, name="two offenders, one in each pass of the counts: the first is reported",
          check=lambda e: e["status"] == ref.CIGAR_LONGER and e["offender"] == 10 and e["n_rec"] == 300 and len(e["reads"]) == 298)
    return L


# ---- b. aux fields ---------------------------------------------------------------------------------------------------------

def _tag(tag, ty, fmt=None, v=None, raw=b""):
    return tag + ty + (struct.pack(fmt, v) if fmt else b"") + raw


def _cg(words, sub=b"I"):
    return b"CGB" + sub + struct.pack("<I", len(words)) + b"".join(struct.pack("<I", (l << 4) | op) for op, l in words)


def aux_records():
    """-> [(record, what it holds, check on its read or None)]"""
    hp1, hp2 = _tag(b"HP", b"C", "<B", 1), _tag(b"HP", b"s", "<h", -2)
    out = []

    def add(aux, name, hp=None, kept=True, **kw):
        cig = kw.pop("cigar", [(0, 40)])
        out.append((rec(2000 + len(out), cig, aux=aux, **kw), name, hp, kept))

    for ty in (b"Z", b"H"):
        for k in (62, 63, 64, 65, 127, 128):
            f = b"XX" + ty + b"a" * k + b"\x00"
            add(hp1 + f, "%s NUL at %d, HP in front" % (ty, k), 1)
            add(f + hp2, "%s NUL at %d, HP behind" % (ty, k), -2)
    add(hp1 + b"XXZ" + b"a" * 70, "Z without NUL, HP in front", 1)
    add(b"XXZ" + b"a" * 70 + hp2, "Z without NUL, HP behind", 0)
    for st, n in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4)):
        add(b"XXB" + st + struct.pack("<I", 3) + bytes(range(1, 3 * n + 1)) + hp2, "B array of %s" % st, -2)
    add(hp1 + b"XXBd" + struct.pack("<I", 1) + bytes(8) + hp2, "B array of an unknown sub-type", 1)
    add(hp1 + b"XXBC" + struct.pack("<I", 1000) + bytes(4) + hp2, "B array past the record", 1)
    add(b"XXBC" + struct.pack("<I", 0) + hp2, "B array of 0 elements", -2)
    add(hp1 + b"X", "one stray byte", 1)
    add(hp1 + b"XX", "two stray bytes", 1)
    add(hp1 + _tag(b"HP", b"A", raw=b"x"), "HP:A after HP:C", 1)
    add(hp1 + _tag(b"HP", b"f", "<f", 2.0), "HP:f after HP:C", 1)
    add(hp1 + _tag(b"HP", b"Z", raw=b"2\x00"), "HP:Z after HP:C", 1)
    for ty, fmt, v in ((b"c", "<b", -3), (b"C", "<B", 200), (b"s", "<h", -300), (b"S", "<H", 40000), (b"i", "<i", -70000), (b"I", "<I", 70000)):
        add(_tag(b"HP", ty, fmt, v), "HP:%s" % ty, v)
    ph = [(4, 40), (3, 40)]
    two = [(0, 20), (2, 5), (0, 20)]
    add(_cg([(0, 40)]) + _cg(two), "two CG:B,I fields", 0, cigar=ph)
    add(_cg([(0, 40)], b"i"), "CG:B,i", 0, kept=False, cigar=ph)
    add(_cg([(0, 40)]), "CG behind a placeholder whose S is not l_seq", 0, cigar=[(4, 39), (3, 40), (0, 1)])
    add(_cg([]), "CG of 0 words", 0, kept=False, cigar=ph)
    for n in (64, 65):
        words = [(0, 1), (1, 1)] * ((n - 1) // 2) + [(0, 1)] * (1 + (n - 1) % 2)
        qn = sum(l for op, l in words if op != 2)
        add(_cg(words), "CG of %d words" % n, 0, cigar=[(4, qn), (3, bw.ref_len(words))], seq=("ACGTTGCA" * 20)[:qn])
    return out


def aux_launch():
    L = Launch()
    items = aux_records()
    recs = [r for r, _, _, _ in items]
    want = [(name, hp) for _, name, hp, kept in items if kept]

    def check(e):
        got = [r["hp"] for r in e["reads"]]
        cg = {name: r for (name, _), r in zip(want, e["reads"])}
        return (e["n_rec"] == len(items) and got == [hp for _, hp in want] and len(cg["two CG:B,I fields"]["cigar"]) == 1
                and cg["CG behind a placeholder whose S is not l_seq"]["cigar"] == [1 << 4]
                and len(cg["CG of 64 words"]["cigar"]) == 64 and len(cg["CG of 65 words"]["cigar"]) == 65)
    L.one(recs, 0, 1000, 5000, cuts=(), check=check, name="aux fields")
    return L


# ---- c. block geometry -----------------------------------------------------------------------------------------------------

def six_records():
    return [rec(100 + 7 * k, [(0, 6 + k), (1, 2), (0, 3)], flag=16 * (k % 2), mapq=20 + k, aux=_tag(b"HP", b"C", "<B", 1 + k % 2) + b"NMi" + bytes(4), name="q%d" % k)
            for k in range(6)]


def full_block_records():
    """six records; the fourth, its aux padded, ends exactly at byte 65536 of the stream"""
    head = [rec(100 + k, [(0, 4)], name="f%d" % k) for k in range(3)]
    pad = 65536 - Stream(head).size - len(bw.record_bytes(rec(110, [(0, 4)], aux=b"XXZ\x00")))
    return head + [rec(110, [(0, 4)], aux=b"XXZ" + b"p" * pad + b"\x00")] + [rec(120 + k, [(0, 4)]) for k in range(2)]


def geometry_launch():
    L = Launch()
    recs = six_records()
    whole = Stream(recs)
    n = whole.size
    all_six = lambda e: len(e["reads"]) == 6 and e["n_rec"] == 6   # noqa: E731
    for cut in range(1, n):
        L.one(recs, 0, 0, 1000, cuts=(cut,), check=all_six, name="cut at %d" % cut)
    s2, s3 = whole.starts[2], whole.starts[3]
    for cuts, name in (((0,), "an empty block first: the chunk begins in it"), ((s2, s2), "an empty block between records"),
                       ((s2, s2, s2), "two empty blocks in a row"), ((n,), "an empty block last"), ((s2 + 5, s2 + 5, s3, s3), "empty blocks inside a record")):
        L.one(recs, 0, 0, 1000, cuts=cuts, check=all_six, name=name)
    g = L.group(Stream(recs, (s2, s2)))
    L.interval(g, 0, 0, 1000, chunks=[(s2, n)], name="the chunk begins in an empty block between records",
               check=lambda e, st=L.groups[g][0]: e["n_rec"] == 4 and st.voff(s2) == (CO0 + CO_STEP) << 16)
    # a block of exactly 65536 bytes whose last record ends at its end
    full = full_block_records()
    st = Stream(full, (65536,))
    assert st.end(3) == 65536 and st.isize[0] == 65536
    g = L.group(st)
    L.interval(g, 0, 0, 1000, chunks=[(0, 65536)], name="chunk_end at offset 0 of the block behind a full block",
               check=lambda e, st=st: e["n_rec"] == 4 and st.voff(65536) == (CO0 + CO_STEP) << 16)
    L.interval(g, 0, 0, 1000, chunks=[(0, st.starts[5])], name="chunk_end one record further", check=lambda e: e["n_rec"] == 5)
    # two chunks with unrelated bytes between them, an empty chunk, a walk that ends in its first chunk
    junk = bytes([0xFF, 0x00, 0x13]) * 23
    st = Stream(recs[:3] + [junk] + recs[3:], (50,))
    g = L.group(st)
    two = [(0, st.end(2)), (st.starts[3], st.size)]
    L.interval(g, 0, 0, 1000, chunks=two, check=all_six, name="two chunks and a gap")
    L.interval(g, 0, 0, 1000, chunks=[(0, st.end(2)), (st.starts[3], st.starts[3]), (st.starts[3], st.size)], check=all_six, name="an empty chunk")
    L.interval(g, 0, 0, recs[2]["pos"], chunks=two, name="pos >= re in the first chunk", check=lambda e: e["n_rec"] == 2 and e["done"])
    L.interval(g, 0, 0, recs[5]["pos"], chunks=two, dropped=1, name="dropped chunks, the end met", check=lambda e: e["status"] == ref.OK and e["done"] and e["n_rec"] == 5)
    L.interval(g, 0, 0, 1000, chunks=two, dropped=1, name="dropped chunks, the end not met", check=lambda e: e["status"] == ref.PAST_PLAN and e["n_rec"] == 6)
    # the previous tid, the next tid and unplaced records at the end
    mixed = ([rec(100 + k, [(0, 5)], tid=0) for k in range(2)] + [rec(50 + k, [(0, 5)], tid=1) for k in range(3)] + [rec(10 + k, [(0, 5)], tid=2) for k in range(2)]
             + [rec(-1, [], tid=-1, seq="ACGT", flag=4) for k in range(2)])
    g = L.group(Stream(mixed, (100, 300)))
    L.interval(g, 1, 0, 1000, name="between the previous and the next tid", check=lambda e: e["n_rec"] == 3 and e["done"] and len(e["reads"]) == 3)
    L.interval(g, 2, 0, 1000, name="unplaced records behind the last tid", check=lambda e: e["n_rec"] == 2 and not e["done"])
    L.interval(g, 2, 0, 1000, dropped=1, name="unplaced records do not end the walk", check=lambda e: e["status"] == ref.PAST_PLAN)
    return L


# ---- d. statuses: one bad interval between two good ones -------------------------------------------------------------------

def good_records(base):
    return [rec(base + 3 * k, [(0, 8), (2, 1), (0, 4)], aux=_tag(b"HP", b"C", "<B", 2), flag=16 * (k % 2)) for k in range(3)]


def straddling_records():
    """three records in two blocks; the second record lies across the cut"""
    recs = good_records(400)
    return recs, (Stream(recs).starts[1] + 20,)


def status_launch(bad_items, bad_cuts=(), order=("A", "bad", "B"), **bad_kw):
    """intervals A, bad, B in this order; the groups' bytes in `order` -> (launch, index of the bad interval's group)"""
    L = Launch()
    streams = dict(A=Stream(good_records(100), (30,)), B=Stream(good_records(200)), bad=Stream(bad_items, bad_cuts))
    gi = {k: L.group(streams[k]) for k in order}
    three = lambda e: len(e["reads"]) == 3 and e["status"] == ref.OK   # noqa: E731
    L.interval(gi["A"], 0, 0, 1000, check=three, name="good A")
    L.interval(gi["bad"], 0, 0, 1000, name="bad", **bad_kw)
    L.interval(gi["B"], 0, 0, 1000, check=three, name="good B")
    return L, gi["bad"]


def _patched(r, at, fmt, v):
    b = bytearray(bw.record_bytes(r))
    struct.pack_into(fmt, b, at, v)
    return dict(r, raw=bytes(b))


def status_cases():
    """-> [dict(name, launch, bad (the interval that must report `status`), tamper (on the tables, or None), status,
    detail {column of counts: value})]; every other interval must decode exactly"""
    out = []

    def add(name, status, made, tamper=None, detail=None, bad=1):
        out.append(dict(name=name, launch=made[0], g=made[1], bad=bad, tamper=tamper, status=status, detail=detail or {}))

    def put(key, i, v=None, d=None):
        def tamper(t, blk0):
            k = blk0 + i if key in ("isize", "out_off", "next_coffset", "blk_status", "coffset") else i
            if key in ("rec_slots", "data_bytes"):
                t[key] += d
            else:
                t[key][k] = v if v is not None else t[key][k] + d
        return tamper

    T, P = ref.BAD_TABLE, ref.PAST_PLAN
    add("iv_blk0 < 0", T, status_launch(good_records(400)), put("iv_blk0", 1, -1), {7: 0})
    add("iv_blk1 > n_blocks", T, status_launch(good_records(400), order=("A", "B", "bad")), put("iv_blk1", 1, d=1), {7: 0})
    add("a slot range past rec_slots (the table is cumulative: only the last interval can have one)", T, status_launch(good_records(400)),
        put("rec_slots", 0, d=-1), {7: 0}, bad=2)
    L = Launch()
    ga, gb = L.group(Stream(good_records(100), (30,))), L.group(Stream(good_records(400)))
    for g in (ga, gb, ga):
        L.interval(g, 0, 0, 1000, check=lambda e: len(e["reads"]) == 3)

    def back(t, blk0):   # interval 1 = chunks [1, 0); interval 2 = chunks [0, 1), which are interval 0's
        t["iv_chunk_off"][:] = [0, 1, 0, 1]
    add("iv_chunk_off decreasing", T, (L, gb), back, {7: 0})
    add("out_off + isize > data_bytes", T, status_launch(good_records(400), order=("A", "B", "bad")), put("data_bytes", 0, d=-1))
    add("isize 65537", T, status_launch(good_records(400)), put("isize", 0, 65537))
    recs, cut = straddling_records()
    add("out_off[b+1] != out_off[b] + isize[b]", T, status_launch(recs, cut), put("out_off", 1, d=1), {7: 1})
    add("one slot too few", T, status_launch(good_records(400), slots=2), None, {7: 2})
    add("coffset[b+1] != next_coffset[b] under a record", P, status_launch(recs, cut), put("next_coffset", 0, d=1), {7: 1})
    add("the last block ends inside a record", P, status_launch(recs, cut), put("iv_blk1", 1, d=-1), {7: 1})
    add("a chunk whose block is not in the range", P, status_launch(good_records(400), vchunks=[((CO0 + 1) << 16, (CO0 + 5 * CO_STEP) << 16)]), None, {7: 0})
    n = Stream(good_records(400)).size
    add("a chunk that begins past the end of its block", ref.SEEK, status_launch(good_records(400), vchunks=[((CO0 << 16) | (n + 1), (CO0 + CO_STEP) << 16)]),
        None, {7: 0})
    made = status_launch(good_records(400))
    add("blk_status != 0 under the chunk's first block", ref.BAD_BLOCK, made, put("blk_status", 0, 3), {5: made[0].groups[made[1]][1], 7: 0})
    made = status_launch(recs, cut)
    add("blk_status != 0 under a record's second block", ref.BAD_BLOCK, made, put("blk_status", 1, 9), {5: made[0].groups[made[1]][1] + 1, 7: 1})
    for bs in (31, (1 << 30) + 1):
        r = good_records(400)
        made = status_launch([r[0], _patched(r[1], 0, "<I", bs), r[2]])
        add("block_size %d" % bs, ref.BLOCK_SIZE, made, None, {5: bs, 7: 1, 4: "record 1"})
    r = good_records(400)
    bs = len(bw.record_bytes(r[1])) - 4
    add("negative l_seq", ref.BAD_RECORD, status_launch([r[0], _patched(r[1], 4 + 16, "<i", -5), r[2]]), None, {5: bs, 6: -1, 7: 1, 4: "record 1"})
    r = [dict(x, aux=b"") for x in good_records(400)]
    bs = len(bw.record_bytes(r[1])) - 4
    add("fields one byte more than block_size", ref.BAD_RECORD, status_launch([r[0], _patched(r[1], 0, "<I", bs - 1), r[2]]), None,
        {5: bs - 1, 6: bs, 7: 1, 4: "record 1"})
    return out


# ---- e. pass sizes of the scans ----------------------------------------------------------------------------------------------

def tiny(pos, **kw):
    return rec(pos, [(0, 1)], seq="ACGT"[pos % 4], **kw)


def intervals_launch(n):
    """n intervals over one stream, 0..3 records each; the first, the middle and the last are empty"""
    L = Launch()
    per = [0 if i in (0, n // 2, n - 1) else i % 4 for i in range(n)]
    recs = [tiny(10 * i + j) for i in range(n) for j in range(per[i])]
    st = Stream(recs)
    g = L.group(st)
    k = 0
    for i in range(n):
        beg = st.starts[k] if k < len(recs) else 0   # (an empty chunk at the very end of the stream would name a block past the table)
        end = st.starts[k + per[i]] if k + per[i] < len(recs) else st.size
        chunks = [(beg, end)] if per[i] else [[(0, 0)], [], [(beg, beg)]][i % 3]
        L.interval(g, 0, 10 * i, 10 * i + 9, chunks=chunks, check=lambda e, i=i: e["n_rec"] == per[i] == len(e["reads"]), name="interval %d" % i)
        k += per[i]
    return L


def _thirds(n, base=0):
    """n tiny records; every third is dropped: by flag, by MAPQ (the launch asks for 5) or because it keeps nothing"""
    recs = []
    for k in range(n):
        if k % 3 != 1:
            recs.append(tiny(base + k))
        elif k % 9 == 1:
            recs.append(tiny(base + k, flag=0x400))
        elif k % 9 == 4:
            recs.append(tiny(base + k, mapq=4))
        else:
            recs.append(rec(base + k, [(1, 1)]))
    return recs


def records_launch(sizes=(255, 256, 257, 600)):
    L = Launch(min_mapq=5)
    for n in sizes:
        L.one(_thirds(n), 0, 0, 100000, cuts="auto", check=lambda e, n=n: e["n_rec"] == n and len(e["reads"]) == n - (n + 1) // 3, name="%d records" % n)
    return L


def fill_launch(total):
    """four intervals that keep `total` reads between them; the second keeps none"""
    L = Launch(min_mapq=5)
    kept = [total // 2, 0, total - total // 2 - 7, 7]
    for j, k in enumerate(kept):
        recs = [rec(50 * j + i, [(0, 1 + i % 3), (1, i % 2), (0, 1)], flag=16 * (i % 2), mapq=5 + i % 50, aux=_tag(b"HP", b"C", "<B", i % 3)) for i in range(k)]
        recs += [tiny(50 * j + k, mapq=0)] * 1   # one record that the filter drops: the interval lists it and keeps nothing of it
        L.one(recs, 0, 0, 100000, cuts="auto", check=lambda e, k=k: len(e["reads"]) == k and e["n_rec"] == k + 1, name="%d kept" % k)
    assert sum(kept) == total
    return L


def capped_launch(n=16390):
    L = Launch()
    L.one([tiny(k) for k in range(n)], 0, 0, 100000, cuts="auto", check=lambda e: len(e["reads"]) == n == e["n_rec"], name="%d records" % n)
    return L


# ---- f. the fill's limits ------------------------------------------------------------------------------------------------------

def fill_limits_launch():
    L = Launch()
    P = 1000
    for n in (1, 63, 64, 65, 129):
        for q0 in (0, 1, 2):   # the first kept SEQ index, odd and even (behind a soft clip of q0 bases)
            seq = ("=ACMGRSVTWYHKDBN" * 9)[:n + q0]
            qual = [(0, 255, 93, 1)[i % 4] for i in range(n + q0)]
            L.one([rec(P, ([(4, q0)] if q0 else []) + [(0, n)], seq=seq, qual=qual)], 0, P, P + n, name="%d bases from SEQ index %d" % (n, q0),
                  check=lambda e, n=n, seq=seq, q0=q0: len(e["reads"]) == 1 and e["reads"][0]["seq"] == seq[q0:].encode() and len(e["reads"][0]["seq"]) == n)
    L.one([rec(P, [(0, 32)], seq="=ACMGRSVTWYHKDBN" * 2, qual=[0, 255] * 16)], 0, P + 1, P + 100, name="all sixteen codes from an odd index",
          check=lambda e: e["reads"][0]["seq"] == ("=ACMGRSVTWYHKDBN" * 2)[1:].encode() and set(e["reads"][0]["qual"]) == {0, 255})
    return L


ALL_LAUNCHES = dict(clip=clip_launch, aux=aux_launch, geometry=geometry_launch, intervals_257=lambda: intervals_launch(257),
                    records=records_launch, fill_1025=lambda: fill_launch(1025), capped=capped_launch, fill_limits=fill_limits_launch)
