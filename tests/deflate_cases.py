"""Raw DEFLATE streams at the format's own limits, for the BGZF inflate kernel: named cases and seeded generators, built with
deflate_writer and shared by the CPU test (zlib agrees with every expected output and every refusal; every case carries the
feature it is named for) and the GPU test (the kernel agrees too).

accepted() -> [Case(name, raw, payload, tokens, check)]: raw is what the stream decodes to (stored bytes as given, tokens
through deflate_writer.expand), check(stream_stats(payload)) is the feature the case is named for; named() is the same as
(name, raw, payload). refused() -> [(name, payload, isize, crc, status name)]. seeded_streams() and mutation_inputs() are
the generators of the differential and the mutation run; judge() is zlib's verdict on an untrusted stream.

Everything is built once per process and must be left unchanged.
"""
import collections
import functools
import random
import zlib

import deflate_writer as dw
from deflate_writer import DBASE, DEXT, LBASE, LEXT, Bits

Case = collections.namedtuple("Case", "name raw payload tokens check")

COPY_DISTS = list(range(1, 67)) + [127, 128, 129]
COPY_LENS = [3, 63, 64, 65, 66, 128, 129, 258]
ISIZES = sorted({4095, 4096, 4097, 8192, 32767, 32768, 32769, 65535} |
                {4096 * k + r for k in (0, 1, 15) for r in (1, 63, 64, 65, 4032, 4033)})


def crc32(b):
    return zlib.crc32(b) & 0xFFFFFFFF


class Stream:
    """blocks written one after the other, with the bytes they stand for and the tokens that say so"""

    def __init__(self):
        self.bits, self.raw, self.tokens = Bits(), bytearray(), []

    def _add(self, tokens):
        self.raw += dw.expand(tokens, self.raw)
        self.tokens += tokens

    def stored(self, data, final=0):
        self.bits.stored(bytes(data), final)
        self.raw += data
        self.tokens += [("lit", b) for b in data]
        return self

    def fixed(self, tokens, final=0):
        dw.fixed_block(self.bits, tokens, final)
        self._add(tokens)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=0, **kw):
        dw.huffman_block(self.bits, tokens, lit_lens, dist_lens, final, **kw)
        self._add(tokens)
        return self

    def case(self, name, check):
        return Case(name, bytes(self.raw), self.bits.tobytes(), self.tokens, check)


def lens_of(n, assigned):
    lens = [0] * n
    for s, l in assigned.items():
        lens[s] = l
    return lens


def lits(rng, n, alphabet=None):
    return [("lit", rng.choice(alphabet) if alphabet else rng.randrange(256)) for _ in range(n)]


def history(s, rng, n, period=29):
    """a fixed block of `period` random literals and (258, period) matches: at least n bytes of history in about n / 160
    bytes of stream, and no two bytes `period` apart by chance alone"""
    toks = lits(rng, period)
    toks += [("match", 258, period)] * (-(-(n - period) // 258))
    s.fixed(toks)
    return s


def fill_to(tokens, pos, target, period):
    """matches at distance `period` (>= 258) and a few literals up to output offset `target`"""
    while pos + 258 <= target:
        tokens.append(("match", 258, period))
        pos += 258
    if target - pos >= 3:
        tokens.append(("match", target - pos, period))
    else:
        tokens += [("lit", 0x30 + k) for k in range(target - pos)]


# ---- random streams -------------------------------------------------------------------------------------------------------

def random_tokens(rng, size, pos, p_lit, alphabet):
    """`size` bytes worth of literals and matches; a match has a random length, a random spelling of it and a random
    distance up to what has been written (`pos` bytes before these tokens)"""
    toks, left = [], size
    while left:
        if pos == 0 or left < 3 or rng.random() < p_lit:
            toks.append(("lit", alphabet[int(rng.random() * len(alphabet))]))
            pos += 1
            left -= 1
            continue
        mx = min(258, left)
        length = rng.randint(3, min(mx, 12)) if rng.random() < 0.5 else rng.randint(3, mx)
        far = min(pos, 32768)
        dist = rng.randint(1, min(far, 70)) if rng.random() < 0.4 else rng.randint(1, far)
        toks.append(("match", length, dist, rng.choice(dw.length_symbols(length))))
        pos += length
        left -= length
    return toks


def used_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if t[0] == "lit":
            lit.add(t[1])
        else:
            lit.add(t[3])
            dist.add(dw.dist_symbol(t[2]))
    return lit, dist


def random_code(rng, used, alphabet, floor, max_len, force_max):
    """code lengths over `alphabet` symbols: a random complete code of the used symbols and a few more, sometimes with
    unused zero lengths sent behind the last one"""
    syms = set(used)
    for _ in range(rng.randint(0, 6)):
        syms.add(rng.randrange(alphabet))
    while len(syms) > 1 << max_len:
        max_len += 1
    syms = sorted(syms)
    n = max(floor, syms[-1] + 1 if syms else 0)
    if rng.random() < 0.3:
        n = rng.randint(n, alphabet)
    lens = [0] * n
    if syms:
        for s, l in zip(syms, dw.complete_lengths(rng, len(syms), max_len, force_max)):
            lens[s] = l
    return lens


def give_longest(lens, sym):
    """swap code lengths so that `sym` holds the longest one; the code stays complete"""
    top = max(range(len(lens)), key=lambda s: lens[s])
    lens[sym], lens[top] = lens[top], lens[sym]


def random_block(s, rng, tokens, final, kinds=("stored", "fixed", "dynamic", "dynamic")):
    kind = rng.choice(kinds)
    if kind == "stored":
        data = dw.expand(tokens, s.raw)
        s.bits.stored(data, final)
        s.raw += data
        s.tokens += tokens
    elif kind == "fixed":
        s.fixed(tokens, final)
    else:
        lit_used, dist_used = used_symbols(tokens)
        max_len = rng.randint(7, 15)
        far = [t for t in tokens if t[0] == "match" and 277 <= t[3] <= 284]
        stress = bool(far) and rng.random() < 0.2
        if stress:                       # the longest codes on the pair with the most extra bits
            max_len = 15
        lit = random_code(rng, lit_used, 286, 257, max_len, stress or rng.random() < 0.5)
        dist = random_code(rng, dist_used, 30, 1, max_len, stress or rng.random() < 0.5)
        if stress:
            t = max(far, key=lambda t: t[2])
            give_longest(lit, t[3])
            give_longest(dist, dw.dist_symbol(t[2]))
        cl_syms = dw.rle_lengths(lit + dist, rng.choice(("plain", "runs", "runs")))
        sent = sorted({x for x, _ in cl_syms})
        cl = None
        if len(sent) >= 2 and rng.random() < 0.5:      # a random code-length code, up to its 7 bits
            cl = lens_of(19, dict(zip(sent, dw.complete_lengths(rng, len(sent), 7, rng.random() < 0.5))))
        s.dynamic(tokens, lit, dist, final, header=cl_syms, cl_lens=cl)


def random_stream(rng, max_size=8192, max_blocks=6):
    size = rng.randint(1, max_size)
    cuts = sorted(rng.randint(0, size) for _ in range(rng.randint(1, max_blocks) - 1)) + [size]
    p_lit = rng.choice((0.2, 0.5, 0.8, 0.95))
    alphabet = rng.sample(range(256), rng.choice((2, 4, 16, 64, 256)))
    s, pos = Stream(), 0
    for k, c in enumerate(cuts):
        random_block(s, rng, random_tokens(rng, c - pos, pos, p_lit, alphabet), int(k == len(cuts) - 1))
        pos = c
    return s


@functools.lru_cache(None)
def seeded_streams(n=2000, seed=20240):
    """[(raw, payload, tokens)] of the differential run"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = random_stream(rng)
        out.append((bytes(s.raw), s.bits.tobytes(), s.tokens))
    return out


def judge(payload):
    """zlib's verdict on an untrusted stream: ("accept", bytes) where it reaches the end of the stream with at most 65536
    bytes (it may stop before the payload's end), ("drop", None) where it gives more, ("refuse", None) everywhere else"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, 65537)
    except zlib.error:
        return "refuse", None
    if len(out) > 65536:
        return "drop", None
    return ("accept", out) if d.eof else ("refuse", None)


@functools.lru_cache(None)
def mutation_inputs(n=3000, seed=777):
    """[(raw of the unharmed stream, the stream with 1-3 bits flipped)]: half from zlib at levels 1-9, half from the writer"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        if i % 2:
            s = random_stream(rng)
            raw, pay = bytes(s.raw), s.bits.tobytes()
        else:
            size = rng.randint(1, 8192)
            alphabet = rng.sample(range(256), rng.choice((4, 16, 64, 256)))
            raw = dw.expand(random_tokens(rng, size, 0, rng.choice((0.2, 0.5, 0.8)), alphabet))
            co = zlib.compressobj(rng.randint(1, 9), zlib.DEFLATED, -15)
            pay = co.compress(raw) + co.flush()
        pay = bytearray(pay)
        for _ in range(rng.randint(1, 3)):
            b = rng.randrange(8 * len(pay))
            pay[b >> 3] ^= 1 << (b & 7)
        out.append((raw, bytes(pay)))
    return out


# ---- the named cases ------------------------------------------------------------------------------------------------------

def _code_lengths(rng):
    out = []
    ladder = list(range(1, 15)) + [15, 15]

    # lengths 1, 2, ..., 14, 15, 15 on the literal/length code, every symbol used
    syms = rng.sample(range(256), 15) + [256]
    rng.shuffle(syms)
    toks = [("lit", x) for x in syms if x != 256] * 3
    rng.shuffle(toks)
    s = Stream().dynamic(toks, lens_of(257, dict(zip(syms, ladder))), [0], 1, header="runs")
    out.append(s.case("lit_lengths_1_to_15", lambda st: st["lit_declared"] == st["lit_used"] == 15 and
                      sorted(l for l in st["blocks"][0]["lit_lens"] if l) == ladder and len(st["lit_syms_used"]) == 16))

    # the same on the distance code: symbols 0..15 reach back at most 256 bytes
    dsyms = list(range(16))
    rng.shuffle(dsyms)
    lit = dw.complete_lengths(rng, 286, 12)
    toks = lits(rng, 260)
    for d in range(16):
        toks.append(("match", rng.randint(3, 20), DBASE[d] + rng.randrange(1 << DEXT[d])))
    s = Stream().dynamic(toks, lit, lens_of(16, dict(zip(dsyms, ladder))), 1, header="runs")
    out.append(s.case("dist_lengths_1_to_15", lambda st: st["dist_declared"] == st["dist_used"] == 15 and
                      sorted(st["blocks"][0]["dist_lens"]) == ladder and len(st["dist_syms_used"]) == 16))

    # 10 and 11 bits side by side, the last code of the primary table and the first behind it, in both codes
    edge = list(range(1, 8)) + [10] * 4 + [11] * 8
    lsyms = rng.sample(range(256), 12) + [256] + list(range(257, 263))
    dsyms = list(range(19))
    rng.shuffle(lsyms)
    rng.shuffle(dsyms)
    toks = lits(rng, 1100, [x for x in lsyms if x < 256])
    for k in range(19 * 2):
        d = k % 19
        toks += [("match", 3 + k % 6, DBASE[d] + rng.randrange(1 << DEXT[d])), ("lit", [x for x in lsyms if x < 256][k % 12])]
    s = Stream().dynamic(toks, lens_of(263, dict(zip(lsyms, edge))), lens_of(19, dict(zip(dsyms, edge))), 1, header="runs")
    out.append(s.case("lengths_10_and_11", lambda st: sorted(l for l in st["blocks"][0]["lit_lens"] if l) == edge and
                      sorted(st["blocks"][0]["dist_lens"]) == edge and len(st["lit_syms_used"]) == 19 and
                      len(st["dist_syms_used"]) == 19 and st["lit_used"] == st["dist_used"] == 11))

    # a random complete code of all 286 symbols, each used, one of them 15 bits long
    lit, dist = dw.complete_lengths(rng, 286, 15, True), dw.complete_lengths(rng, 30, 15, True)
    toks = [("lit", x) for x in range(256)]
    rng.shuffle(toks)
    for ls in range(257, 286):
        i = ls - 257
        d = rng.randrange(16)
        toks += [("match", LBASE[i] + rng.randrange(1 << LEXT[i]), DBASE[d] + rng.randrange(1 << DEXT[d]), ls),
                 ("lit", rng.randrange(256))]
    s = Stream().dynamic(toks, lit, dist, 1, header="plain")
    out.append(s.case("random_286_symbols_15_bits", lambda st: st["blocks"][0]["hlit"] == 286 and st["lit_used"] == 15 and
                      len(st["lit_syms_used"]) == 286))

    # a code-length code 1, 2, ..., 6, 7, 7 bits long with both 7-bit codes used, all 19 of its lengths sent
    ladder7 = [1, 2, 3, 4, 5, 6, 7, 7]
    syms = rng.sample(range(256), 7) + [256]
    cl = lens_of(19, dict(zip(range(8), ladder7)))            # length value v is sent with a code of ladder7[v] bits
    toks = lits(rng, 40, syms[:7])
    s = Stream().dynamic(toks + [("lit", x) for x in syms[:7]], lens_of(257, dict(zip(syms, ladder7))), [0], 1, cl_lens=cl,
                         header="plain", hclen=19)
    out.append(s.case("code_length_code_7_bits", lambda st: st["cl_declared"] == st["cl_used"] == 7 and
                      st["blocks"][0]["hclen"] == 19))

    # the smallest header of a block that decodes: HLIT = 257, HDIST = 1 and HCLEN = 5. With HCLEN = 4 only 16, 17, 18 and 0
    # have codes, so no length but zero can be sent and the block has no end-of-block code: that one is among the refusals.
    toks = lits(rng, 64, list(range(255)))
    s = Stream().dynamic(toks, [8] * 255 + [0, 8], [0], 1, header="plain")
    out.append(s.case("minimum_header", lambda st: (st["blocks"][0]["hlit"], st["blocks"][0]["hdist"],
                                                    st["blocks"][0]["hclen"]) == (257, 1, 5)))
    return out


def _pair_case(seed, k, lsym, dsym):
    rng = random.Random(seed)
    s = history(Stream(), rng, DBASE[dsym] + 300)
    have = len(s.raw)
    # literal/length: 'a' one bit, fourteen more symbols 2..15 bits, the length symbol the other 15-bit code
    others = rng.sample([x for x in range(256) if x != 97], 13) + [256]
    rng.shuffle(others)
    lit = lens_of(lsym + 1, dict(zip(others, range(2, 16))))
    lit[97], lit[lsym] = 1, 15
    # distance: fifteen near symbols 1..15 bits, the far symbol the other 15-bit code
    near = list(range(15))
    rng.shuffle(near)
    dist = lens_of(dsym + 1, dict(zip(near, range(1, 16))))
    dist[dsym] = 15
    i = lsym - 257
    length = LBASE[i] + rng.randrange(32)
    d = DBASE[dsym] + rng.randrange(min(8192, have - DBASE[dsym]))
    toks = [("lit", 97)] * k + [("match", length, d, lsym)] + [("lit", x) for x in others if x != 256]
    s.dynamic(toks, lit, dist, 1, header="runs")
    return s


def _pairs(rng):
    out = []
    combos = [(l, d) for l in (281, 282, 283, 284) for d in (28, 29)]

    def start(s):
        (p0, nb, _, _), = dw.stream_stats(s.bits.tobytes())["pairs"]
        assert nb == 48
        return p0

    for off in range(32):
        lsym, dsym = combos[off % 8]
        k = (off - start(_pair_case(100 + off, 0, lsym, dsym))) % 32
        s = _pair_case(100 + off, k, lsym, dsym)
        out.append(s.case("pair_48_bits_at_bit_%d" % off,
                          lambda st, off=off: st["max_pair_bits"] == 48 and st["pairs"][0][0] % 32 == off and
                          st["lit_used"] == st["dist_used"] == 15))
    # the pair across payload byte 256 * k, where the kernel's window of 64 dwords ends
    for edge, back in ((2048, 47), (2048, 24), (2048, 1), (4096, 47), (4096, 24), (4096, 1)):
        lsym, dsym = combos[(edge + back) % 4 * 2]      # distance symbol 28: the history block stays short
        k = edge - back - start(_pair_case(200 + back, 0, lsym, dsym))
        assert k >= 0, k
        s = _pair_case(200 + back, k, lsym, dsym)
        out.append(s.case("pair_48_bits_across_byte_%d_from_bit_%d" % (edge // 8, edge - back),
                          lambda st, edge=edge, back=back: st["pairs"][0][:2] == (edge - back, 48)))
    return out


def _table_extent(rng):
    s = history(Stream(), rng, 32768)
    lit, dist = dw.complete_lengths(rng, 286, 15, True), dw.complete_lengths(rng, 30, 15, True)
    toks = lits(rng, 5) + [("match", 258, 24577, 284), ("lit", 7), ("match", 258, 32768, 285), ("lit", 9),
                           ("match", 227, 32768, 284), ("match", 258, 32768, 284), ("match", 3, 24577)]
    s.dynamic(toks, lit, dist, 1, header="plain")
    return [s.case("hlit_286_hdist_30", lambda st: (st["blocks"][1]["hlit"], st["blocks"][1]["hdist"]) == (286, 30) and
                   {284, 285} <= st["lit_syms_used"] and 29 in st["dist_syms_used"] and st["max_dist"] == 32768 and
                   {(258, 24577), (258, 32768)} <= {m[1:] for m in st["match_at"]})]


RUN_ENDS_AT_TOTAL = (lens_of(258, {97: 1, 256: 2, 257: 2}), [1, 1] + [0] * 28)


def _header_runs(rng):
    out = []

    def one(name, lit, dist, toks, check, **kw):
        kw.setdefault("header", "runs")
        out.append(Stream().dynamic(toks, lit, dist, 1, **kw).case(name, lambda st: check(st["blocks"][0], st)))

    a = [("lit", 97)]
    # 16: lens[256] = 2 is sent, then 16 repeats it over lens[257] and the four distance lengths, to the very end
    one("run_16_across_boundary", lens_of(258, {97: 2, 98: 3, 99: 3, 256: 2, 257: 2}), [2, 2, 2, 2],
        [("lit", 97), ("lit", 98), ("lit", 99), ("lit", 98)] + [("match", 3, d) for d in (1, 2, 3, 4)],
        lambda b, st: b["cross"] == [(16, 257, 5)] and st["cross16"] == 1 and st["n_matches"] == 4)
    # 17: three zeros, two literal/length lengths and the first distance length
    one("run_17_across_boundary", lens_of(260, {97: 1, 256: 2, 257: 2}), [0, 1, 1], a * 5 + [("match", 3, 2), ("match", 3, 3)],
        lambda b, st: b["cross"] == [(17, 258, 3)] and st["n_matches"] == 2)
    # 18: 28 zeros up to HLIT = 286 and five more
    one("run_18_across_boundary", lens_of(286, {97: 1, 256: 2, 257: 2}), [0] * 5 + [1, 1],
        a * 13 + [("match", 3, 7), ("match", 3, 12)], lambda b, st: b["cross"] == [(18, 258, 33)] and st["n_matches"] == 2)
    one("run_18_of_138", lens_of(258, {138: 2, 139: 2, 256: 2, 257: 2}), [1, 1],
        [("lit", 138), ("lit", 139), ("match", 3, 1), ("match", 3, 2)], lambda b, st: (18, 0, 138) in b["runs"])
    one("run_16_of_6", lens_of(257, dict.fromkeys(list(range(97, 104)) + [256], 3)), [0], lits(rng, 30, list(range(97, 104))),
        lambda b, st: (16, 98, 6) in b["runs"])
    # a 16 behind an 18 repeats the zero: no compressor sends that
    syms = [(18, 97 - 11), (16, 0), (2, 0), (3, 0), (18, 138 - 11), (18, 16 - 11), (1, 0), (3, 0), (1, 0), (1, 0)]
    one("run_16_right_after_18", lens_of(258, {100: 2, 101: 3, 256: 1, 257: 3}), [1, 1],
        [("lit", 100), ("lit", 101), ("match", 3, 2), ("match", 3, 1)], lambda b, st: b["runs"][:2] == [(18, 0, 97), (16, 97, 3)],
        header=syms)
    lit, dist = RUN_ENDS_AT_TOTAL
    one("run_ends_at_hlit_plus_hdist", lit, dist, a * 4 + [("match", 3, 1), ("match", 3, 2)],
        lambda b, st: b["runs"][-1] == (18, 260, 28) and b["hlit"] + b["hdist"] == 288)
    return out


def _degenerate(rng):
    out = []
    a = [("lit", 97)]
    s = Stream().dynamic(a * 3 + [("match", 3, 1), ("match", 4, 1)] + a, lens_of(259, {97: 1, 256: 2, 257: 3, 258: 3}), [1], 1)
    out.append(s.case("single_distance_code_used", lambda st: st["dist_single"] == 1 and st["n_matches"] == 2))
    s = Stream().dynamic(lits(rng, 20, [97, 98]), lens_of(257, {97: 1, 98: 2, 256: 2}), [0], 1)
    out.append(s.case("no_distance_code_literals_only", lambda st: st["dist_absent"] == 1 and st["blocks"][0]["hdist"] == 1))
    s = Stream().dynamic([], lens_of(257, {256: 1}), [0], 1)
    out.append(s.case("only_end_of_block", lambda st: st["out"] == b"" and st["blocks"][0]["type"] == "dynamic" and
                      [l for l in st["blocks"][0]["lit_lens"] if l] == [1]))
    return out


def _big_small(s, rng, big, final):
    """one dynamic block: HLIT = 286 and HDIST = 30 with long codes, or HLIT = 257 and HDIST = 1 with short ones"""
    pos = len(s.raw)
    if big:
        toks = random_tokens(rng, 700, pos, 0.7, list(range(256)))
        s.dynamic(toks, dw.complete_lengths(rng, 286, 15, True), dw.complete_lengths(rng, 30, 15, True), final,
                  header=rng.choice(("plain", "runs")))
    else:
        syms = rng.sample(range(256), 5)
        s.dynamic(lits(rng, 200, syms), lens_of(257, dict(zip(syms + [256], [1, 2, 3, 4, 5, 5]))), [1], final, header="runs")


def _chains(rng):
    out = []
    # about 300 small blocks of every type in one member
    s = Stream()
    alphabet = list(range(256))
    for k in range(300):
        random_block(s, rng, random_tokens(rng, rng.randint(0, 40), len(s.raw), 0.6, alphabet), int(k == 299),
                     ("stored", "fixed", "dynamic"))
    out.append(s.case("chain_of_300_blocks", lambda st: len(st["blocks"]) == 300 and
                      all(sum(b["type"] == t for b in st["blocks"]) >= 50 for t in ("stored", "fixed", "dynamic"))))

    # empty stored blocks whose header starts at every bit of a byte: a fixed block of one 9-bit literal is 19 bits long
    s = Stream()
    for phase in (0, 5, 2, 7, 4, 1, 6, 3):
        while s.bits.n % 8 != phase:
            s.fixed([("lit", rng.randrange(144, 256))])
        s.stored(b"")
    s.fixed(lits(rng, 9), 1)
    out.append(s.case("empty_stored_blocks_at_every_bit", lambda st: {b["start_bit"] % 8 for b in st["blocks"]
                                                                      if b["type"] == "stored" and b["len"] == 0} == set(range(8))))

    s = Stream().stored(bytes(rng.randrange(256) for _ in range(65535))).fixed([("lit", 0x5A)], 1)
    out.append(s.case("stored_65535_and_one_literal", lambda st: len(st["out"]) == 65536 and st["blocks"][0]["len"] == 65535))

    # matches that reach back over block boundaries: into a stored block, into the dynamic block before
    s = Stream().stored(bytes(rng.randrange(256) for _ in range(300)))
    lit, dist = dw.complete_lengths(rng, 286, 13, True), dw.complete_lengths(rng, 30, 13, True)
    s.dynamic([("match", 40, 300), ("lit", 1), ("match", 258, 341), ("match", 5, 1)] + lits(rng, 50), lit, dist, header="runs")
    n1 = len(s.raw)
    lit, dist = dw.complete_lengths(rng, 286, 15, True), dw.complete_lengths(rng, 30, 15, True)
    s.dynamic([("match", 100, 50), ("match", 258, n1), ("lit", 2), ("match", 30, n1 - 290)], lit, dist, header="runs")
    s.fixed([("match", 258, len(s.raw)), ("match", 3, 3), ("match", 70, 400)], 1)
    out.append(s.case("matches_across_block_boundaries", lambda st: [b["type"] for b in st["blocks"]] ==
                      ["stored", "dynamic", "dynamic", "fixed"] and st["match_at"][0] == (300, 40, 300) and
                      (n1, 100, 50) in st["match_at"]))

    # a large table, then a small one that leaves most of the large one's entries behind, and the reverse
    for name, order in (("tables_big_then_small", (1, 0)), ("tables_small_then_big", (0, 1)),
                        ("tables_big_small_big_small", (1, 0, 1, 0))):
        s = Stream()
        for k, big in enumerate(order):
            _big_small(s, rng, big, int(k == len(order) - 1))
        out.append(s.case(name, lambda st, order=order: [(b["hlit"], b["hdist"]) for b in st["blocks"]] ==
                          [((286, 30) if big else (257, 1)) for big in order] and st["dist_single"] == order.count(0)))
    return out


def _copies(rng):
    out = []
    # every distance around the 64-lane chunk with every length around it, one after the other
    lit, dist = dw.complete_lengths(rng, 286, 12), dw.complete_lengths(rng, 30, 9)
    toks = lits(rng, 130)
    for d in COPY_DISTS:
        for ln in COPY_LENS:
            toks += [("match", ln, d), ("lit", rng.randrange(256))]
    s = Stream().dynamic(toks, lit, dist, 1, header="runs")
    out.append(s.case("copies_dist_x_len", lambda st: {m[1:] for m in st["match_at"]} ==
                      {(ln, d) for d in COPY_DISTS for ln in COPY_LENS}))
    # each of them again across output offset 4096 (a flush of the ring) and across 32768 (the ring's wrap)
    for d in COPY_DISTS:
        for ln in COPY_LENS:
            toks = lits(rng, 300)
            p = 300
            for edge in (4096, 32768):
                at = edge - rng.randint(1, ln - 1)
                fill_to(toks, p, at, 300)
                toks += [("match", ln, d)] + lits(rng, 2)
                p = at + ln + 2
            s = Stream().fixed(toks, 1)
            out.append(s.case("copy_dist_%d_len_%d_across_4096_and_32768" % (d, ln),
                              lambda st, d=d, ln=ln: all(any(m[1:] == (ln, d) and m[0] < e < m[0] + ln for m in st["match_at"])
                                                         for e in (4096, 32768))))
    return out


def _sizes(rng):
    out = []
    for size in ISIZES:
        s, pos = Stream(), 0
        cuts = sorted(rng.randint(0, size) for _ in range(2)) + [size]
        for k, c in enumerate(cuts):
            random_block(s, rng, random_tokens(rng, c - pos, pos, 0.3, list(range(256))), int(k == 2), ("fixed", "dynamic"))
            pos = c
        out.append(s.case("isize_%d" % size, lambda st, size=size: len(st["out"]) == size))
    return out


@functools.lru_cache(None)
def accepted():
    rng = random.Random(1951)
    cases = []
    for group in (_code_lengths, _pairs, _table_extent, _header_runs, _degenerate, _chains, _copies, _sizes):
        cases += group(rng)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:                       # no case may quietly miss its target
        assert c.check(dw.stream_stats(c.payload)), c.name
    return cases


def named():
    return [(c.name, c.raw, c.payload) for c in accepted()]


@functools.lru_cache(None)
def refused():
    """(name, payload, isize, crc, name of the expected PV_BGZF_* status): zlib refuses each of them too"""
    out = []
    tail = [("bits", 0, 32)]
    lit, dist = RUN_ENDS_AT_TOTAL
    syms = dw.rle_lengths(lit + dist, "runs")
    assert syms[-1] == (18, 28 - 11)
    b = dw.write_header(Bits(), 1, 258, 30, syms[:-1] + [(18, 28 - 11 + 1)]).put(0, 32)
    out.append(("run_one_past_the_end", b.tobytes(), 10, 0, "PV_BGZF_BAD_CODE_LENGTHS"))
    b = dw.write_header(Bits(), 1, 257, 1, [(16, 0), (0, 0), (8, 0)]).put(0, 32)
    out.append(("first_symbol_is_16", b.tobytes(), 10, 0, "PV_BGZF_BAD_CODE_LENGTHS"))
    b = dw.write_header(Bits(), 1, 257, 1, dw.rle_lengths(lens_of(257, {97: 1, 98: 1}) + [0], "runs")).put(0, 32)
    out.append(("no_end_of_block_code", b.tobytes(), 10, 0, "PV_BGZF_BAD_CODE_LENGTHS"))
    # HCLEN = 4: only 16, 17, 18 and 0 can have codes, so every length is zero
    b = dw.write_header(Bits(), 1, 257, 1, [(18, 127), (18, 109)], cl_lens=lens_of(19, {18: 1, 0: 1}), hclen=4).put(0, 32)
    out.append(("hclen_4_sends_no_length", b.tobytes(), 10, 0, "PV_BGZF_BAD_CODE_LENGTHS"))
    a = [("lit", 97)]
    b = dw.huffman_block(Bits(), a * 3 + [("sym", 257), ("bits", 1, 1)] + tail, lens_of(259, {97: 1, 256: 2, 257: 3, 258: 3}),
                         [1], 1)
    out.append(("single_distance_code_other_bit", b.tobytes(), 10, 0, "PV_BGZF_BAD_SYMBOL"))
    b = dw.huffman_block(Bits(), a * 3 + [("sym", 257)] + tail, lens_of(258, {97: 1, 256: 2, 257: 2}), [0], 1)
    out.append(("no_distance_code_but_a_match", b.tobytes(), 10, 0, "PV_BGZF_BAD_SYMBOL"))
    return out


# ---- whole blocks from the writer, and from libdeflate's compressor --------------------------------------------------------

def greedy_tokens(data):
    """a small greedy tokeniser: the last place where the next three bytes were seen, taken as far as it matches"""
    toks, seen, i, n = [], {}, 0, len(data)
    while i < n:
        j = None
        if i + 3 <= n:
            key = data[i:i + 3]
            j = seen.get(key)
            seen[key] = i
        if j is not None and i - j <= 32768:
            ln = 3
            while ln < 258 and i + ln < n and data[j + ln] == data[i + ln]:
                ln += 1
            toks.append(("match", ln, i - j))
            i += ln
        else:
            toks.append(("lit", data[i]))
            i += 1
    return toks


def writer_deflate(rng):
    """bytes -> one dynamic block with random complete codes of up to 15 bits and a run-length-encoded header"""
    def deflate(data):
        toks = greedy_tokens(data)
        assert dw.expand(toks) == data
        lit, dist = dw.complete_lengths(rng, 286, 15, True), dw.complete_lengths(rng, 30, 15, True)
        return dw.huffman_block(Bits(), toks, lit, dist, 1, header="runs").tobytes()
    return deflate


def libdeflate_compress():
    """(data, level) -> raw DEFLATE stream from libdeflate's compressor, or None where the library does not load"""
    import ctypes as C
    lib = None
    for name in ("libdeflate.so.0", "libdeflate.so", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0", "/opt/conda/lib/libdeflate.so.0"):
        try:
            lib = C.CDLL(name)
            break
        except OSError:
            continue
    if lib is None:
        return None
    lib.libdeflate_alloc_compressor.restype = C.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [C.c_int]
    lib.libdeflate_deflate_compress.restype = C.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    lib.libdeflate_deflate_compress_bound.restype = C.c_size_t
    lib.libdeflate_deflate_compress_bound.argtypes = [C.c_void_p, C.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [C.c_void_p]

    def compress(data, level):
        c = lib.libdeflate_alloc_compressor(level)
        assert c
        try:
            buf = C.create_string_buffer(lib.libdeflate_deflate_compress_bound(c, len(data)))
            n = lib.libdeflate_deflate_compress(c, data, len(data), buf, len(buf))
            assert n > 0
            return buf.raw[:n]
        finally:
            lib.libdeflate_free_compressor(c)
    return compress
