// bgzf_inflate.hip — batched BGZF block inflate (RFC 1951 raw DEFLATE + the gzip trailer's CRC32 and ISIZE) on gfx950.
//
// One wavefront per BGZF block, one single-wave workgroup per block (about 39 KB of LDS each, so four per CU). The wave
// decodes its stream wave-uniformly: every control value is read with readfirstlane, so the bit buffer, the table entries
// and the branches live in scalar registers. Per wave in LDS:
//   * a 32 KiB history ring: every output byte is written there first. A DEFLATE distance is at most 32768 and a copy only
//     reads bytes written before it starts (a short period is replicated with j % dist), so the ring always holds the source;
//   * the literal/length and distance codes: a 10-bit primary table ((symbol << 4) | length) plus the canonical count /
//     sorted-symbol arrays that decode the rare codes longer than 10 bits bit by bit;
//   * a 256-entry CRC32 table.
// Tables are built lane-parallel: counts by ballot/popcount, symbols sorted by ballot ranks, and every lane fills 16 primary
// entries by a prefix search of the canonical code. Literals are stored by one lane; matches and stored blocks by all 64.
// The ring is flushed to the block's output range 4 KiB at a time; at each flush every lane runs the CRC32 over a 64-byte
// slice and the slices are combined with x^(8n) mod P factors (zlib's crc32_combine algebra).
//
// Safety: a block's loads stay in [payload + in_off, + clen) and its stores in [out + out_off, + isize); the block table
// itself is checked against the buffer sizes first. Bits past clen read as zero and the reader counts what it consumed: a
// symbol whose bits end past clen stops the block (BGZF_INPUT_OVERRUN) before it is acted on. Every loop consumes at least
// one bit or output byte per iteration and both are bounded, and a guard counter bounds the symbol loops besides.
#include "pv_common.hpp"

namespace {

constexpr int BW = 64;              // lanes: one wavefront per block
constexpr int RING = 32768;
constexpr int RMASK = RING - 1;
constexpr int PBITS = 10;
constexpr int PSIZE = 1 << PBITS;
constexpr int FLUSH = 4096;         // ring -> global + CRC granule (64 lanes x 64-byte slices)
constexpr uint32_t CRC_POLY = 0xEDB88320u;

struct Huff {
    uint16_t tab[PSIZE];            // (symbol << 4) | length for codes of <= PBITS bits; 0: a longer code or no code
    uint16_t sym[288];              // symbols sorted by (length, value)
    uint16_t cnt[16];               // codes per length
    uint16_t first[16];             // canonical first code of each length (MSB-first)
    uint16_t offs[16];              // index in sym of the first symbol of each length
};
struct Smem {
    uint8_t ring[RING];
    Huff lit, dist;                 // dist also holds the code-length code while the dynamic header is read
    uint32_t crc[256];
    uint8_t lens[320];
    uint8_t cll[20];
};

__constant__ uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                   131, 163, 195, 227, 258};
__constant__ uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                   2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t CLORD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int U(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t Uu(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// a*b mod P in the reflected representation (zlib's multmodp)
__device__ uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P, n < 2^16 bytes; x2n[k] = x^(2^k) mod P
__device__ uint32_t x8n(const uint32_t* x2n, uint32_t n) {
    uint32_t p = 0x80000000u;
    for (int k = 3; n; n >>= 1, k++)
        if (n & 1) p = multmodp(x2n[k], p);
    return p;
}

// the canonical code of lens[0..n) -> h. 0 ok, else the code is over-subscribed or incomplete where zlib rejects it:
// incomplete is allowed only for a literal/length or distance code that is a single one-bit code (`single_ok`), and a code
// without any symbol is accepted (it decodes nothing).
__device__ __noinline__ int build_huff(Huff& h, const uint8_t* lens, int n, bool single_ok, int lane) {
    int cnt[16];
#pragma unroll
    for (int L = 0; L < 16; L++) cnt[L] = 0;
    for (int b = 0; b < n; b += BW) {
        const int s = b + lane;
        const int l = s < n ? lens[s] : 0;
#pragma unroll
        for (int L = 1; L < 16; L++) cnt[L] += __popcll(__ballot(l == L));
    }
    int left = 1, maxl = 0, code = 0, off = 0;
    int first[16], offs[16];
    first[0] = offs[0] = 0;
#pragma unroll
    for (int L = 1; L < 16; L++) {
        left = (left << 1) - cnt[L];
        if (left < 0) return 1;
        if (cnt[L]) maxl = L;
        code = (code + cnt[L - 1]) << 1;
        first[L] = code;
        offs[L] = off;
        off += cnt[L];
    }
    if (maxl > 0 && left > 0 && !(single_ok && maxl == 1)) return 1;
    if (lane < 16) {
        int c = 0, f = 0, o = 0;
#pragma unroll
        for (int L = 0; L < 16; L++)
            if (L == lane) { c = cnt[L]; f = first[L]; o = offs[L]; }
        h.cnt[lane] = (uint16_t)c; h.first[lane] = (uint16_t)f; h.offs[lane] = (uint16_t)o;
    }
    // symbols in canonical order: rank among the same-length symbols before it = ballot prefix
    int base[16];
#pragma unroll
    for (int L = 0; L < 16; L++) base[L] = offs[L];
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int b = 0; b < n; b += BW) {
        const int s = b + lane;
        const int l = s < n ? lens[s] : 0;
#pragma unroll
        for (int L = 1; L < 16; L++) {
            const uint64_t m = __ballot(l == L);
            if (l == L) h.sym[base[L] + __popcll(m & lt)] = (uint16_t)s;
            base[L] += __popcll(m);
        }
    }
    __syncthreads();
    // primary table: entry idx holds the code whose bits (first stream bit = MSB of the code) prefix idx's low bits
    for (int idx = lane; idx < PSIZE; idx += BW) {
        const uint32_t r = __brev((uint32_t)idx) >> (32 - PBITS);
        uint16_t e = 0;
#pragma unroll
        for (int L = 1; L <= PBITS; L++) {
            const uint32_t c = (r >> (PBITS - L)) - (uint32_t)first[L];
            if (e == 0 && c < (uint32_t)cnt[L]) e = (uint16_t)((h.sym[offs[L] + c] << 4) | L);
        }
        h.tab[idx] = e;
    }
    __syncthreads();
    return 0;
}

struct BlockArgs {
    const uint8_t* payload;
    int64_t payload_bytes;
    int64_t n;
    const int64_t* in_off;
    const int32_t* clen;
    const int32_t* isize;
    const uint32_t* crc;
    const int64_t* out_off;
    uint8_t* out;
    int64_t out_bytes;
    int32_t* status;
};

__global__ __launch_bounds__(BW) void k_bgzf_inflate(BlockArgs a) {
    __shared__ Smem sm;
    __shared__ uint32_t x2n[32];
    const int lane = threadIdx.x;
    const int64_t blk = blockIdx.x;
    int st = PV_BGZF_OK;
    const int64_t ioff = a.in_off[blk], ooff = a.out_off[blk];
    const int clen = a.clen[blk], isize = a.isize[blk];
    if (ioff < 0 || clen < 0 || ioff > a.payload_bytes - clen || ooff < 0 || isize < 0 || isize > 65536 ||
        ooff > a.out_bytes - isize) {
        if (lane == 0) a.status[blk] = PV_BGZF_BAD_ARGS;
        return;
    }
    const uint8_t* __restrict__ in = a.payload + ioff;
    uint8_t* __restrict__ out = a.out + ooff;
    for (int i = lane; i < 256; i += BW) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
        sm.crc[i] = c;
    }
    if (lane == 0) {
        uint32_t p = 0x40000000u;   // x^1
        for (int k = 0; k < 32; k++) { x2n[k] = p; p = multmodp(p, p); }
    }
    __syncthreads();

    // ---- bit reader: a window of 64 dwords of the payload, one per lane; bb/nb/nextw are wave-uniform ----
    int wbase = -BW;
    uint32_t win = 0;
    auto getw = [&](int w) -> uint32_t {
        if (w < wbase || w >= wbase + BW) {
            wbase = w;
            const int b = 4 * (w + lane);
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (b + k < clen) v |= (uint32_t)in[b + k] << (8 * k);
            win = v;
        }
        return Uu(__builtin_amdgcn_readlane(win, w - wbase));
    };
    uint64_t bb = 0;
    int nb = 0, nextw = 0;
    auto need32 = [&]() {
        if (nb < 32) { bb |= (uint64_t)getw(nextw) << nb; nextw++; nb += 32; }
    };
    auto drop = [&](int k) { bb >>= k; nb -= k; };
    auto over = [&]() { return nextw * 32 - nb > 8 * clen; };
    // restart the reader at byte q of the payload (after a stored block)
    auto seek_byte = [&](int q) {
        nextw = q >> 2;
        bb = 0; nb = 0;
        need32();
        drop(8 * (q & 3));
    };
    // one symbol of h from the (>= 15) buffered bits; -1 = no code matches
    auto decode = [&](const Huff& h) -> int {
        const int e = U(h.tab[bb & (PSIZE - 1)]);
        if (e) { drop(e & 15); return e >> 4; }
        int code = 0, first = 0, index = 0;
        for (int L = 1; L < 16; L++) {
            code |= (int)((bb >> (L - 1)) & 1);
            const int c = U(h.cnt[L]);
            if (code - c < first) { drop(L); return U(h.sym[index + (code - first)]); }
            index += c; first += c;
            first <<= 1; code <<= 1;
        }
        return -1;
    };

    // ---- output: ring + flush to global with the CRC ----
    int pos = 0, flushed = 0;
    uint32_t crcst = 0xFFFFFFFFu;
    auto flush = [&](bool all) {
        while (pos - flushed >= FLUSH || (all && pos > flushed)) {
            const int n = min(FLUSH, pos - flushed);
            __syncthreads();
            for (int i = lane; i < n; i += BW) out[flushed + i] = sm.ring[(flushed + i) & RMASK];
            const int s0 = 64 * lane, s1 = min(s0 + 64, n);
            uint32_t c = 0;
            for (int i = s0; i < s1; i++) c = sm.crc[(c ^ sm.ring[(flushed + i) & RMASK]) & 0xFF] ^ (c >> 8);
            if (s1 > s0 && s1 < n) c = multmodp(x8n(x2n, (uint32_t)(n - s1)), c);
            for (int d = 1; d < BW; d <<= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
            crcst = multmodp(x8n(x2n, (uint32_t)n), crcst) ^ Uu(c);
            flushed += n;
        }
    };

    int guard = 8 * clen + 64;      // symbols + block headers: each consumes at least one bit
    bool last = false;
    while (!last) {
        need32();
        last = bb & 1;
        const int type = (int)((bb >> 1) & 3);
        drop(3);
        if (over() || --guard < 0) { st = PV_BGZF_INPUT_OVERRUN; break; }
        if (type == 3) { st = PV_BGZF_BAD_BTYPE; break; }
        if (type == 0) {
            drop(nb & 7);
            need32();
            const int len = (int)(bb & 0xFFFF), nlen = (int)((bb >> 16) & 0xFFFF);
            drop(32);
            if (over()) { st = PV_BGZF_INPUT_OVERRUN; break; }
            if (len != (~nlen & 0xFFFF)) { st = PV_BGZF_STORED_LEN; break; }
            const int q = (nextw * 32 - nb) >> 3;
            if (len > clen - q) { st = PV_BGZF_INPUT_OVERRUN; break; }
            if (len > isize - pos) { st = PV_BGZF_OUTPUT_OVERFLOW; break; }
            for (int j0 = 0; j0 < len; j0 += BW) {
                const int k = min(BW, len - j0);
                if (lane < k) sm.ring[(pos + lane) & RMASK] = in[q + j0 + lane];
                pos += k;
                flush(false);
            }
            seek_byte(q + len);
            continue;
        }
        if (type == 1) {
            for (int s = lane; s < 320; s += BW) sm.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
            __syncthreads();
            build_huff(sm.lit, sm.lens, 288, true, lane);
            build_huff(sm.dist, sm.lens + 288, 32, true, lane);
        } else {
            need32();
            const int hlit = (int)(bb & 31) + 257, hdist = (int)((bb >> 5) & 31) + 1, hclen = (int)((bb >> 10) & 15) + 4;
            drop(14);
            if (hlit > 286 || hdist > 30) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
            if (lane < 19) sm.cll[lane] = 0;
            __syncthreads();
            for (int k = 0; k < hclen; k++) {
                need32();
                if (lane == 0) sm.cll[CLORD[k]] = (uint8_t)(bb & 7);
                drop(3);
            }
            __syncthreads();
            if (over()) { st = PV_BGZF_INPUT_OVERRUN; break; }
            if (build_huff(sm.dist, sm.cll, 19, false, lane)) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
            const int ntot = hlit + hdist;
            int i = 0;
            while (i < ntot) {
                need32();
                const int sym = decode(sm.dist);
                if (sym < 0) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
                if (sym < 16) {
                    if (lane == 0) sm.lens[i] = (uint8_t)sym;
                    i++;
                } else {
                    int v = 0, rep;
                    if (sym == 16) {
                        if (i == 0) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
                        __syncthreads();
                        v = U(sm.lens[i - 1]);
                        rep = 3 + (int)(bb & 3); drop(2);
                    } else if (sym == 17) {
                        rep = 3 + (int)(bb & 7); drop(3);
                    } else {
                        rep = 11 + (int)(bb & 127); drop(7);
                    }
                    if (rep > ntot - i) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
                    for (int r = lane; r < rep; r += BW) sm.lens[i + r] = (uint8_t)v;
                    i += rep;
                }
                if (over()) { st = PV_BGZF_INPUT_OVERRUN; break; }
            }
            if (st) break;
            __syncthreads();
            if (U(sm.lens[256]) == 0) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
            if (build_huff(sm.lit, sm.lens, hlit, true, lane)) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
            if (build_huff(sm.dist, sm.lens + hlit, hdist, true, lane)) { st = PV_BGZF_BAD_CODE_LENGTHS; break; }
        }
        // ---- the compressed data of a Huffman block ----
        for (;;) {
            if (--guard < 0) { st = PV_BGZF_INPUT_OVERRUN; break; }
            need32();
            const int sym = decode(sm.lit);
            if (sym < 0 || sym > 285) { st = PV_BGZF_BAD_SYMBOL; break; }
            if (sym < 256) {
                if (over()) { st = PV_BGZF_INPUT_OVERRUN; break; }
                if (pos >= isize) { st = PV_BGZF_OUTPUT_OVERFLOW; break; }
                if (lane == 0) sm.ring[pos & RMASK] = (uint8_t)sym;
                pos++;
                flush(false);
                continue;
            }
            if (sym == 256) {
                if (over()) st = PV_BGZF_INPUT_OVERRUN;
                break;
            }
            const int li = sym - 257;
            const int le = LEXT[li];
            const int len = LBASE[li] + (int)(bb & ((1u << le) - 1));
            drop(le);
            need32();
            const int ds = decode(sm.dist);
            if (ds < 0 || ds > 29) { st = PV_BGZF_BAD_SYMBOL; break; }
            const int de = DEXT[ds];
            const int dist = DBASE[ds] + (int)(bb & ((1u << de) - 1));
            drop(de);
            if (over()) { st = PV_BGZF_INPUT_OVERRUN; break; }
            if (dist > pos) { st = PV_BGZF_DIST_TOO_FAR; break; }
            if (len > isize - pos) { st = PV_BGZF_OUTPUT_OVERFLOW; break; }
            for (int j0 = 0; j0 < len; j0 += BW) {
                const int j = j0 + lane;
                uint8_t v = 0;
                if (j < len) v = sm.ring[(pos - dist + (dist >= len ? j : j % dist)) & RMASK];
                __syncthreads();
                if (j < len) sm.ring[(pos + j) & RMASK] = v;
            }
            pos += len;
            flush(false);
        }
        if (st) break;
    }
    if (st == PV_BGZF_OK && pos != isize) st = PV_BGZF_OUTPUT_SHORT;
    if (st == PV_BGZF_OK) {
        flush(true);
        if ((crcst ^ 0xFFFFFFFFu) != a.crc[blk]) st = PV_BGZF_CRC_MISMATCH;
    }
    if (lane == 0) a.status[blk] = st;
}

// d_counts = {bytes of the good blocks, PV_OK / PV_ERR_INVALID, first bad block or -1, its status}
__global__ __launch_bounds__(256) void k_bgzf_counts(const int32_t* __restrict__ status, const int32_t* __restrict__ isize,
                                                      int64_t n, int64_t* __restrict__ counts) {
    __shared__ int64_t s_bytes[256], s_bad[256];
    int64_t bytes = 0, bad = INT64_MAX;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        if (status[i] == PV_BGZF_OK) bytes += isize[i];
        else if (i < bad) bad = i;
    }
    s_bytes[threadIdx.x] = bytes; s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_bytes[threadIdx.x] += s_bytes[threadIdx.x + s];
            s_bad[threadIdx.x] = min(s_bad[threadIdx.x], s_bad[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t b = s_bad[0];
        counts[0] = s_bytes[0];
        counts[1] = b == INT64_MAX ? PV_OK : PV_ERR_INVALID;
        counts[2] = b == INT64_MAX ? -1 : b;
        counts[3] = b == INT64_MAX ? 0 : status[b];
    }
}

}  // namespace

extern "C" int pv_bgzf_inflate_dev(pv_ctx* ctx, const uint8_t* payload, int64_t payload_bytes, int64_t n_blocks,
                                   const int64_t* in_off, const int32_t* clen, const int32_t* isize, const uint32_t* crc,
                                   const int64_t* out_off, uint8_t* out, int64_t out_bytes, int32_t* status, int64_t* d_counts,
                                   void* stream) {
    PV_CHECK(ctx && d_counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_blocks >= 0 && payload_bytes >= 0 && out_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(n_blocks == 0 || (payload && in_off && clen && isize && crc && out_off && out && status), PV_ERR_INVALID,
             "bgzf_inflate: block table, payload or output missing");
    PV_CHECK(n_blocks < (1ll << 31), PV_ERR_LIMIT, "too many blocks for one launch");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = pv_pick_stream(ctx, stream);
    BlockArgs a;
    a.payload = payload; a.payload_bytes = payload_bytes; a.n = n_blocks;
    a.in_off = in_off; a.clen = clen; a.isize = isize; a.crc = crc; a.out_off = out_off;
    a.out = out; a.out_bytes = out_bytes; a.status = status;
    if (n_blocks > 0) {
        // the context's event profile (pv_profile_begin) is not thread-safe: only a call on the context's own stream, which
        // cannot overlap other calls of the context, records into it. A call on a stream of its own may run on another thread
        // beside the context's calls, so it is left out of that profile (rocprofv3 still sees the kernel by its name).
        if (st == ctx->stream) {
            pv_prof_scope ps(ctx, "k_bgzf_inflate", st);
            k_bgzf_inflate<<<(unsigned)n_blocks, BW, 0, st>>>(a);
        } else {
            k_bgzf_inflate<<<(unsigned)n_blocks, BW, 0, st>>>(a);
        }
    }
    k_bgzf_counts<<<1, 256, 0, st>>>(status, isize, n_blocks, d_counts);
    PV_HIP(hipGetLastError());
    return PV_OK;
}

template <typename T>
static int bg_stage(pv_ctx* ctx, const char* name, const T* src, size_t n, T** dst, hipStream_t st) {
    int rc = pv_get(ctx, name, n > 0 ? n : 1, dst);
    if (rc) return rc;
    if (n > 0) PV_HIP(hipMemcpyAsync(*dst, src, n * sizeof(T), hipMemcpyHostToDevice, st));
    return PV_OK;
}

extern "C" int pv_bgzf_inflate(pv_ctx* ctx, const uint8_t* payload, int64_t payload_bytes, int64_t n_blocks,
                               const int64_t* in_off, const int32_t* clen, const int32_t* isize, const uint32_t* crc,
                               const int64_t* out_off, uint8_t* out, int64_t out_bytes, int32_t* status, int64_t* counts) {
    PV_CHECK(ctx && counts, PV_ERR_INVALID, "null argument");
    PV_CHECK(n_blocks >= 0 && payload_bytes >= 0 && out_bytes >= 0, PV_ERR_INVALID, "negative sizes");
    PV_CHECK(n_blocks == 0 || (payload && in_off && clen && isize && crc && out_off && out && status), PV_ERR_INVALID,
             "bgzf_inflate: block table, payload or output missing");
    PV_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)n_blocks;
    const uint8_t* d_pay = nullptr;
    const int64_t *d_ioff = nullptr, *d_ooff = nullptr;
    const int32_t *d_clen = nullptr, *d_isize = nullptr;
    const uint32_t* d_crc = nullptr;
    uint8_t* d_out = nullptr;
    int32_t* d_status = nullptr;
    int64_t* d_counts = nullptr;
    int rc;
    if ((rc = bg_stage(ctx, "bg.payload", payload, (size_t)payload_bytes, (uint8_t**)&d_pay, st))) return rc;
    if ((rc = bg_stage(ctx, "bg.in_off", in_off, n, (int64_t**)&d_ioff, st))) return rc;
    if ((rc = bg_stage(ctx, "bg.clen", clen, n, (int32_t**)&d_clen, st))) return rc;
    if ((rc = bg_stage(ctx, "bg.isize", isize, n, (int32_t**)&d_isize, st))) return rc;
    if ((rc = bg_stage(ctx, "bg.crc", crc, n, (uint32_t**)&d_crc, st))) return rc;
    if ((rc = bg_stage(ctx, "bg.out_off", out_off, n, (int64_t**)&d_ooff, st))) return rc;
    // the output is staged from the caller's buffer so that bytes outside every block's range come back unchanged
    if ((rc = bg_stage(ctx, "bg.out", (const uint8_t*)out, (size_t)out_bytes, &d_out, st))) return rc;
    if ((rc = pv_get(ctx, "bg.status", n > 0 ? n : 1, &d_status))) return rc;
    if ((rc = pv_get(ctx, "bg.counts", (size_t)4, &d_counts))) return rc;
    rc = pv_bgzf_inflate_dev(ctx, d_pay, payload_bytes, n_blocks, d_ioff, d_clen, d_isize, d_crc, d_ooff, d_out, out_bytes,
                             d_status, d_counts, st);
    if (rc) return rc;
    PV_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (n > 0) PV_HIP(hipMemcpyAsync(status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (out_bytes > 0) PV_HIP(hipMemcpyAsync(out, d_out, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    PV_HIP(hipStreamSynchronize(st));
    PV_CHECK(counts[1] == PV_OK, PV_ERR_INVALID, "bgzf_inflate: block %lld failed with status %lld", (long long)counts[2],
             (long long)counts[3]);
    return PV_OK;
}
