"""A token-level DEFLATE (RFC 1951) writer and a stream inspector in plain Python: what a compressor never emits, a test can
still spell out. No tests here.

Tokens are ("lit", byte) and ("match", length, distance[, length symbol]); expand() copies them out byte by byte. Malformed
streams also use ("sym", s) (one literal/length code alone), ("dsym", s) (one distance code alone) and ("bits", value, n).
huffman_block() writes a dynamic block from code lengths the caller gives, fixed_block() a fixed one and Bits.stored() a
stored one. complete_lengths() draws a random complete prefix code. stream_stats() parses a valid stream with a decoder of
its own and reports what the stream holds, so that a case can assert that it carries the feature it is named for.

`rng` is a random.Random everywhere in this module.
"""
import bisect

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORD = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CLEXT = {16: 2, 17: 3, 18: 7}
CLBASE = {16: 3, 17: 3, 18: 11}
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


REV15 = [0] * 32768
for _i in range(1, 32768):
    REV15[_i] = (REV15[_i >> 1] >> 1) | ((_i & 1) << 14)


def rev(code, nbits):
    """the low nbits (<= 15) of code in reverse order"""
    return REV15[code & 0x7FFF] >> (15 - nbits)


class Bits:
    """LSB-first bit writer (RFC 1951 3.1.1); Huffman codes go MSB-first"""

    def __init__(self):
        self.buf, self.acc, self.k = bytearray(), 0, 0

    @property
    def n(self):
        return 8 * len(self.buf) + self.k

    def _spill(self, nbytes):
        self.buf += (self.acc & ((1 << (8 * nbytes)) - 1)).to_bytes(nbytes, "little")
        self.acc >>= 8 * nbytes
        self.k -= 8 * nbytes

    def put(self, val, nbits):
        self.acc |= (val & ((1 << nbits) - 1)) << self.k
        self.k += nbits
        if self.k >= 64:
            self._spill(self.k >> 3)
        return self

    def code(self, c, nbits):
        return self.put(rev(c, nbits), nbits)

    def lit_fixed(self, sym):
        if sym < 144:
            return self.code(0x30 + sym, 8)
        if sym < 256:
            return self.code(0x190 + sym - 144, 9)
        if sym < 280:
            return self.code(sym - 256, 7)
        return self.code(0xC0 + sym - 280, 8)

    def align(self):
        self.k = (self.k + 7) // 8 * 8
        return self

    def tobytes(self):
        """the stream, ending in the byte of its last bit"""
        return bytes(self.buf) + self.acc.to_bytes((self.k + 7) // 8, "little")

    def bytes(self):
        """the stream and one zero byte of slack behind it"""
        return self.tobytes() + b"\x00"

    def stored(self, data: bytes, final=0):
        """a stored block (RFC 1951 3.2.4): header, pad to a byte, LEN, NLEN, the bytes"""
        self.put(final, 1).put(0, 2).align()
        self.put(len(data), 16).put(~len(data), 16)
        self._spill(self.k >> 3)
        self.buf += data
        return self

    def match_fixed(self, length, dist):
        """a length/distance pair with the fixed codes, extra bits included"""
        li = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
        self.lit_fixed(257 + li).put(length - LBASE[li], LEXT[li])
        di = max(i for i in range(30) if DBASE[i] <= dist)
        return self.code(di, 5).put(dist - DBASE[di], DEXT[di])


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> per symbol (code with its first stream bit lowest, length), None for a symbol without a code"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for L in range(1, 16):
        code = (code + cnt[L - 1]) << 1
        nxt[L] = code
    out = [None] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = (rev(nxt[l], l), l)
            nxt[l] += 1
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


_LENGTH_SYMBOLS = {n: [257 + i for i in range(29) if LBASE[i] <= n < LBASE[i] + (1 << LEXT[i])] for n in range(3, 259)}


def length_symbols(length):
    """every literal/length symbol that can spell `length`, smallest first (258 is 284 + extra 31 as well as 285)"""
    return _LENGTH_SYMBOLS[length]


def dist_symbol(dist):
    return bisect.bisect_right(DBASE, dist) - 1


def expand(tokens, history=b""):
    """the bytes the tokens stand for, behind `history`; a match is copied byte by byte, so it may overlap itself"""
    out = bytearray(history)
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        elif t[0] == "match":
            length, dist = t[1], t[2]
            assert 3 <= length <= 258 and 1 <= dist <= min(len(out), 32768), t
            p = len(out) - dist
            if dist >= length:           # source and destination apart: the byte-by-byte copy is this slice
                out += out[p:p + length]
            else:
                for j in range(length):
                    out.append(out[p + j])
        else:
            raise ValueError("expand: %r stands for no bytes" % (t,))
    return bytes(out[len(history):])


def write_tokens(bits, tokens, lit_lens, dist_lens, eob=True):
    lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)

    def put(codes, s, what):
        if s >= len(codes) or codes[s] is None:
            raise ValueError("%s symbol %d has no code" % (what, s))
        bits.put(*codes[s])

    for t in tokens:
        if t[0] == "lit":
            put(lc, t[1], "literal")
        elif t[0] == "match":
            length, dist = t[1], t[2]
            if len(t) > 3:
                ls = t[3]
                assert ls in length_symbols(length), t
            else:
                have = [s for s in length_symbols(length) if s < len(lit_lens) and lit_lens[s]]
                if not have:
                    raise ValueError("no length symbol with a code spells %d" % length)
                ls = have[0]
            put(lc, ls, "length")
            bits.put(length - LBASE[ls - 257], LEXT[ls - 257])
            ds = dist_symbol(dist)
            put(dc, ds, "distance")
            bits.put(dist - DBASE[ds], DEXT[ds])
        elif t[0] == "sym":
            put(lc, t[1], "literal/length")
        elif t[0] == "dsym":
            put(dc, t[1], "distance")
        elif t[0] == "bits":
            bits.put(t[1], t[2])
        else:
            raise ValueError(t)
    if eob:
        put(lc, 256, "end-of-block")
    return bits


def fixed_block(bits, tokens, final, eob=True):
    bits.put(final, 1).put(1, 2)
    return write_tokens(bits, tokens, FIXED_LIT, FIXED_DIST, eob)


def balanced_lengths(n):
    """a complete code of n >= 2 symbols with lengths floor(log2 n) and one more"""
    k = n.bit_length() - 1
    short = (2 << k) - n
    return [k] * short + [k + 1] * (n - short)


def rle_lengths(lens, style):
    """the code-length symbols (symbol, extra value) that send `lens`: "plain" every length on its own, "runs" greedily with
    16/17/18 over the whole array, which is the literal/length and the distance lengths in one"""
    if style == "plain":
        return [(l, 0) for l in lens]
    assert style == "runs", style
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        if v == 0:
            if run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
            elif run >= 3:
                k = run
                out.append((17, k - 3))
            else:
                k = 1
                out.append((0, 0))
            i += k
            continue
        out.append((v, 0))
        i += 1
        rest = run - 1
        while rest >= 3:
            k = min(rest, 6)
            out.append((16, k - 3))
            rest -= k
            i += k
    return out


def expand_header(cl_syms):
    """the code lengths that a list of code-length symbols sends"""
    lens = []
    for s, e in cl_syms:
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + e)
        else:
            lens += [0] * (CLBASE[s] + e)
    return lens


def default_cl_lens(cl_syms):
    used = sorted({s for s, _ in cl_syms})
    if len(used) == 1:                   # the code-length code must be complete: a second symbol, never sent
        used.append(0 if used[0] else 1)
    cl = [0] * 19
    for s, l in zip(used, balanced_lengths(len(used))):
        cl[s] = l
    return cl


def write_header(bits, final, hlit, hdist, cl_syms, cl_lens=None, hclen=None):
    """the header of a dynamic block from an explicit list of code-length symbols, well-formed or not"""
    if cl_lens is None:
        cl_lens = default_cl_lens(cl_syms)
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CLORD[k]]])
    assert all(cl_lens[CLORD[k]] == 0 for k in range(hclen, 19)), "hclen cuts off a code length"
    bits.put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(hclen - 4, 4)
    for k in range(hclen):
        bits.put(cl_lens[CLORD[k]], 3)
    codes = canonical_codes(cl_lens)
    for s, e in cl_syms:
        bits.put(*codes[s])
        if s >= 16:
            bits.put(e, CLEXT[s])
    return bits


def huffman_block(bits, tokens, lit_lens, dist_lens, final, cl_lens=None, header="plain", hclen=None, eob=True):
    """a dynamic block: `header` is "plain", "runs" or the list of code-length symbols itself (which must send lit_lens +
    dist_lens); cl_lens are the 19 lengths of the code-length code, by default a balanced code of the symbols sent"""
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
    cl_syms = rle_lengths(lit_lens + dist_lens, header) if isinstance(header, str) else list(header)
    assert expand_header(cl_syms) == lit_lens + dist_lens
    write_header(bits, final, len(lit_lens), len(dist_lens), cl_syms, cl_lens, hclen)
    return write_tokens(bits, tokens, lit_lens, dist_lens, eob)


def complete_lengths(rng, symbols, max_len, force_max=False):
    """a random complete prefix code of `symbols` symbols, none longer than max_len: split random leaves of a tree that
    starts as one leaf; with force_max the tree starts as a path down to max_len. The leaves go to the symbols in shuffled
    order. One symbol alone gets the single one-bit code, which is incomplete and legal for a distance code."""
    n = symbols
    if n == 1:
        return [1]
    assert 2 <= n <= 1 << max_len
    if force_max and n > max_len:
        leaves = list(range(1, max_len + 1)) + [max_len]
    else:
        leaves = [1, 1]
    done = [d for d in leaves if d >= max_len]
    todo = [d for d in leaves if d < max_len]
    while len(done) + len(todo) < n:
        i = int(rng.random() * len(todo))
        d = todo[i] + 1
        if d < max_len:
            todo[i] = d
            todo.append(d)
        else:
            todo[i] = todo[-1]
            todo.pop()
            done += [d, d]
    leaves = done + todo
    rng.shuffle(leaves)
    assert kraft(leaves) == 32768
    return leaves


# ---- the inspector ------------------------------------------------------------------------------------------------------

class _Reader:
    def __init__(self, data):
        self.d, self.p, self.acc, self.cnt, self.pos = data, 0, 0, 0, 0

    def peek(self, n):
        while self.cnt < n:              # bits past the end read as zero; take() refuses to consume them
            chunk = self.d[self.p:self.p + 8]
            self.acc |= int.from_bytes(chunk, "little") << self.cnt
            self.p += 8
            self.cnt += 64
        return self.acc & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.acc >>= n
        self.cnt -= n
        self.pos += n
        if self.pos > 8 * len(self.d):
            raise ValueError("stream ends inside a symbol")
        return v

    def seek_byte(self, q):
        self.p, self.acc, self.cnt, self.pos = q, 0, 0, 8 * q


class _Code:
    def __init__(self, lens, what):
        self.what = what
        self.by_len, self.seen = {}, {}
        for s, c in enumerate(canonical_codes(lens)):
            if c:
                self.by_len.setdefault(c[1], {})[c[0]] = s
        self.order = sorted(self.by_len)
        self.declared = max(self.order) if self.order else 0
        self.n = sum(1 for l in lens if l)
        k = kraft(lens)
        if k > 32768 or (k < 32768 and self.n and not (what != "code-length" and self.n == 1 and self.declared == 1)):
            raise ValueError("%s code is over-subscribed or incomplete" % what)

    def lookup(self, w):
        """(symbol, length) of the code that starts the 15 bits w"""
        hit = self.seen.get(w & 511)
        if hit:
            return hit
        for L in self.order:
            s = self.by_len[L].get(w & ((1 << L) - 1))
            if s is not None:
                if L <= 9:               # the next 9 bits decide this symbol: remember them
                    self.seen[w & 511] = (s, L)
                return s, L
        raise ValueError("no %s code matches" % self.what)

    def read(self, r):
        s, L = self.lookup(r.peek(15))
        r.take(L)
        return s, L


def stream_stats(payload):
    """parse a valid raw DEFLATE stream. Returns a dict:
      blocks: per block dict(type, start_bit, and for a dynamic block hlit, hdist, hclen, runs = [(symbol, index, count)],
              cross = the runs that start below hlit and end above it, dist_codes = distance symbols with a code)
      cl/lit/dist_declared, cl/lit/dist_used: the longest code length declared and used, over the dynamic blocks
      cross_runs, cross16/17/18: runs across the literal/distance boundary
      max_pair_bits, pairs: [(start bit, bits, length, distance)] of the pairs of >= 45 bits
      dist_single, dist_absent: dynamic blocks whose distance code is one one-bit code / holds no code at all
      lit_syms_used, dist_syms_used: the symbols used in the dynamic blocks; max_dist; match_at: [(output offset, length,
      distance)] of every match; n_literals, n_matches, end_bit; out: the decoded bytes
    Raises ValueError on a malformed stream."""
    r = _Reader(payload)
    out = bytearray()
    st = dict(blocks=[], cl_declared=0, cl_used=0, lit_declared=0, lit_used=0, dist_declared=0, dist_used=0, cross_runs=0,
              cross16=0, cross17=0, cross18=0, max_pair_bits=0, pairs=[], dist_single=0, dist_absent=0, n_literals=0,
              n_matches=0, max_dist=0, lit_syms_used=set(), dist_syms_used=set(), match_at=[])
    final = 0
    while not final:
        start = r.pos
        final, btype = r.take(1), r.take(2)
        if btype == 3:
            raise ValueError("block type 3")
        if btype == 0:
            blk = dict(type="stored", start_bit=start)
            r.take((-r.pos) % 8)
            ln, nln = r.take(16), r.take(16)
            if ln != (~nln & 0xFFFF):
                raise ValueError("stored LEN/NLEN")
            q = r.pos >> 3
            if q + ln > len(payload):
                raise ValueError("stored block runs past the end")
            out += payload[q:q + ln]
            r.seek_byte(q + ln)
            blk["len"] = ln
            st["blocks"].append(blk)
            continue
        if btype == 1:
            blk = dict(type="fixed", start_bit=start)
            lit, dist = _Code(FIXED_LIT, "literal/length"), _Code(FIXED_DIST + [5, 5], "distance")
        else:
            hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
            if hlit > 286 or hdist > 30:
                raise ValueError("too many length or distance symbols")
            cll = [0] * 19
            for k in range(hclen):
                cll[CLORD[k]] = r.take(3)
            cl = _Code(cll, "code-length")
            lens, runs = [], []
            while len(lens) < hlit + hdist:
                s, L = cl.read(r)
                st["cl_used"] = max(st["cl_used"], L)
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16 and not lens:
                    raise ValueError("repeat without a length before it")
                k = CLBASE[s] + r.take(CLEXT[s])
                if len(lens) + k > hlit + hdist:
                    raise ValueError("repeat past the end of the lengths")
                runs.append((s, len(lens), k))
                lens += [lens[-1] if s == 16 else 0] * k
            if lens[256] == 0:
                raise ValueError("no end-of-block code")
            lit, dist = _Code(lens[:hlit], "literal/length"), _Code(lens[hlit:], "distance")
            cross = [x for x in runs if x[1] < hlit < x[1] + x[2]]
            blk = dict(type="dynamic", start_bit=start, hlit=hlit, hdist=hdist, hclen=hclen, runs=runs, cross=cross,
                       dist_codes=[s for s, l in enumerate(lens[hlit:]) if l], lit_lens=lens[:hlit], dist_lens=lens[hlit:])
            st["cl_declared"] = max(st["cl_declared"], cl.declared)
            st["lit_declared"] = max(st["lit_declared"], lit.declared)
            st["dist_declared"] = max(st["dist_declared"], dist.declared)
            st["cross_runs"] += len(cross)
            for x in cross:
                st["cross%d" % x[0]] += 1
            st["dist_single"] += dist.n == 1 and dist.declared == 1
            st["dist_absent"] += dist.n == 0
        st["blocks"].append(blk)
        dynamic = btype == 2
        # the symbols of the block, with the reader's state in locals: 48 buffered bits hold the longest pair
        d, total, acc, cnt, p, pos = payload, 8 * len(payload), r.acc, r.cnt, r.p, r.pos
        lseen, dseen, lit_syms, dist_syms = lit.seen, dist.seen, set(), set()
        lit_used = dist_used = 0
        while True:
            if cnt < 48:
                acc |= int.from_bytes(d[p:p + 8], "little") << cnt
                p += 8
                cnt += 64
            if pos > total:
                raise ValueError("stream ends inside a symbol")
            p0 = pos
            hit = lseen.get(acc & 511) or lit.lookup(acc & 0x7FFF)
            s, L = hit
            acc >>= L
            cnt -= L
            pos += L
            if L > lit_used:
                lit_used = L
            if s < 256:
                out.append(s)
                lit_syms.add(s)
                continue
            lit_syms.add(s)
            if s == 256:
                break
            if s > 285:
                raise ValueError("literal/length symbol %d" % s)
            e = LEXT[s - 257]
            length = LBASE[s - 257] + (acc & ((1 << e) - 1))
            acc >>= e
            ds, L = dseen.get(acc & 511) or dist.lookup(acc & 0x7FFF)
            if L > dist_used:
                dist_used = L
            if ds > 29:
                raise ValueError("distance symbol %d" % ds)
            acc >>= L
            k = DEXT[ds]
            dd = DBASE[ds] + (acc & ((1 << k) - 1))
            acc >>= k
            cnt -= e + L + k
            pos += e + L + k
            if pos > total:
                raise ValueError("stream ends inside a symbol")
            if dd > len(out):
                raise ValueError("distance too far back")
            q = len(out) - dd
            st["match_at"].append((len(out), length, dd))
            if dd >= length:
                out += out[q:q + length]
            else:
                for j in range(length):
                    out.append(out[q + j])
            dist_syms.add(ds)
            if dd > st["max_dist"]:
                st["max_dist"] = dd
            nb = pos - p0
            if nb > st["max_pair_bits"]:
                st["max_pair_bits"] = nb
            if nb >= 45:
                st["pairs"].append((p0, nb, length, dd))
        if pos > total:
            raise ValueError("stream ends inside a symbol")
        r.acc, r.cnt, r.p, r.pos = acc, cnt, p, pos
        st["n_matches"] = len(st["match_at"])
        st["n_literals"] = len(out) - sum(m[1] for m in st["match_at"]) - sum(b.get("len", 0) for b in st["blocks"])
        if dynamic:
            st["lit_used"], st["dist_used"] = max(st["lit_used"], lit_used), max(st["dist_used"], dist_used)
            st["lit_syms_used"] |= lit_syms
            st["dist_syms_used"] |= dist_syms
    st["end_bit"] = r.pos
    st["out"] = bytes(out)
    return st


AGGREGATE_MAX = ("cl_declared", "cl_used", "lit_declared", "lit_used", "dist_declared", "dist_used", "max_pair_bits")
AGGREGATE_SUM = ("cross_runs", "cross16", "cross17", "cross18", "dist_single", "dist_absent", "n_literals", "n_matches")


def aggregate_stats(stats):
    """one summary of many stream_stats results"""
    agg = dict(streams=0, blocks=0, stored=0, fixed=0, dynamic=0, max_hlit=0, max_hdist=0, max_hclen=0, pairs_ge_45=0, bytes=0)
    for k in AGGREGATE_MAX + AGGREGATE_SUM:
        agg[k] = 0
    for st in stats:
        agg["streams"] += 1
        agg["bytes"] += len(st["out"])
        agg["pairs_ge_45"] += len(st["pairs"])
        for b in st["blocks"]:
            agg["blocks"] += 1
            agg[b["type"]] += 1
            if b["type"] == "dynamic":
                agg["max_hlit"] = max(agg["max_hlit"], b["hlit"])
                agg["max_hdist"] = max(agg["max_hdist"], b["hdist"])
                agg["max_hclen"] = max(agg["max_hclen"], b["hclen"])
        for k in AGGREGATE_MAX:
            agg[k] = max(agg[k], st[k])
        for k in AGGREGATE_SUM:
            agg[k] += int(st[k])
    return agg
