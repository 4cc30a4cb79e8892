// PNG frame encode (include/sagen.h: sagen_png_filter, sagen_deflate): the five row filters with the minimum-sum-of-absolute-values choice,
// and a zlib stream whose deflate blocks hold a per-block Huffman code and runs at distance 1 - no hash table, no parse: every position
// knows its token from its run alone.  It replaces the host's Image.save behind the overlay writers (the reference muxes lossless
// frames, myutils.py:246-279).
//
// The same code runs on the device (png.hip) and on the host (csrc_cpu/sagen_cpu.cpp, tools/png_encode_check.cpp: plain loops,
// png_filter_host and deflate_host below): the token rule, the length symbols, the Huffman code (sort key, Moffat-Katajainen lengths,
// the 15-bit limit, the canonical codes), the block costs and the choice, the block header, the positions, Adler-32 and the bit sink are
// written once.  What differs is who walks: 256 threads a block there, one loop here.
//
// One block = PNG_BLOCK input bytes (16 384: the probe of the issue was made at this size; a code's header is 153 bytes, 0.9 % of it).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define PNG_FN __host__ __device__ __forceinline__
#else
#define PNG_FN inline
#endif
// a word of the zeroed stream that two writers may share: OR commutes, the result does not depend on the order
#if defined(__HIP_DEVICE_COMPILE__)
#define PNG_OR(p, v) atomicOr((p), (v))
#else
#define PNG_OR(p, v) (void)(*(p) |= (v))
#endif

namespace sagen {

constexpr int PNG_BLOCK = 16384;                   // input bytes per deflate block
constexpr int PNG_CHUNK = 64;                      // bytes one thread of the device walks: PNG_BLOCK / 256
constexpr int PNG_CHUNKS = PNG_BLOCK / PNG_CHUNK;
constexpr int PNG_SYMS = 286;                      // literals, end of block, the 29 length symbols
constexpr int PNG_MAX_BITS = 15;
constexpr int PNG_DYN_HEADER = 3 + 14 + 19 * 3 + (PNG_SYMS + 1) * 4;     // 1222 bits: every length sent plainly, as a 4-bit code
constexpr int PNG_STORED = 0, PNG_FIXED = 1, PNG_DYNAMIC = 2;
constexpr long long PNG_MAX_LENGTH = 1LL << 28, PNG_MAX_STRIDE = 1LL << 28;
constexpr int PNG_MAX_DIM = 16384, PNG_MAX_FRAMES = 65535;
constexpr uint32_t PNG_ADLER = 65521;

// ---- the row filters ---------------------------------------------------------------------------------------------------------------
PNG_FN int png_abs(int v) { return v < 0 ? -v : v; }

PNG_FN int png_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = png_abs(p - a), pb = png_abs(p - b), pc = png_abs(p - c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// filter `type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) of v with a = left, b = above, c = above left (0 outside the image)
PNG_FN int png_filtered(int type, int v, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
    return (v - pred) & 255;
}

PNG_FN int png_filter_cost(int v) { return v < 128 ? v : 256 - v; }     // min(v, 256 - v)

// byte x of a row of wc = w components bytes with its three neighbours; up: the row above or null
PNG_FN void png_neighbours(const uint8_t* cur, const uint8_t* up, int x, int bpp, int& v, int& a, int& b, int& c) {
    v = cur[x];
    a = x >= bpp ? cur[x - bpp] : 0;
    b = up ? up[x] : 0;
    c = up && x >= bpp ? up[x - bpp] : 0;
}

// the filter of the smallest sum, the lowest number among equals
PNG_FN int png_filter_choice(long long s0, long long s1, long long s2, long long s3, long long s4) {
    int best = 0;
    long long least = s0;
    if (s1 < least) least = s1, best = 1;
    if (s2 < least) least = s2, best = 2;
    if (s3 < least) least = s3, best = 3;
    if (s4 < least) least = s4, best = 4;
    return best;
}

inline void png_filter_host(const uint8_t* frames, int n, int w, int h, int comps, uint8_t* rows) {
    const size_t wc = (size_t)w * comps;
    for (size_t r = 0; r < (size_t)n * h; ++r) {
        const uint8_t* cur = frames + r * wc;
        const uint8_t* up = r % h ? cur - wc : nullptr;
        long long sum[5] = {0, 0, 0, 0, 0};
        int v, a, b, c;
        for (int x = 0; x < (int)wc; ++x) {
            png_neighbours(cur, up, x, comps, v, a, b, c);
            for (int t = 0; t < 5; ++t) sum[t] += png_filter_cost(png_filtered(t, v, a, b, c));
        }
        const int best = png_filter_choice(sum[0], sum[1], sum[2], sum[3], sum[4]);
        uint8_t* o = rows + r * (wc + 1);
        o[0] = (uint8_t)best;
        for (int x = 0; x < (int)wc; ++x) {
            png_neighbours(cur, up, x, comps, v, a, b, c);
            o[1 + x] = (uint8_t)png_filtered(best, v, a, b, c);
        }
    }
}

inline int png_filter_args_check(const void* frames, int n, int w, int h, int comps, const void* rows, const char** why) {
    if (n < 0 || w < 1 || h < 1) return *why = "n < 0, w < 1 or h < 1", SAGEN_ERR_SHAPE;
    if (comps != 1 && comps != 3) return *why = "components other than 1 (grey) or 3 (RGB)", SAGEN_ERR_UNSUPPORTED;
    if (w > PNG_MAX_DIM || h > PNG_MAX_DIM || n > PNG_MAX_FRAMES) return *why = "w or h above 16384, or n above 65535", SAGEN_ERR_UNSUPPORTED;
    if (!frames || !rows) return *why = "null argument", SAGEN_ERR_NULL;
    return SAGEN_OK;
}

// ---- the geometry of a deflate call ------------------------------------------------------------------------------------------------
struct DeflateGeom {
    int n, nblocks;                                // frames; blocks per frame: ceil(length / PNG_BLOCK), one (empty) block for length 0
    long long length, stride;
    long long cap;                                 // bytes per frame of the stream in scratch: its bound, up to a multiple of 16
};

struct DeflateScratch {
    size_t kind, bits, s1, tt, at, table, stream, total;      // byte offsets of the regions
};

inline int deflate_blocks(long long length) { return length <= 0 ? 1 : (int)((length + PNG_BLOCK - 1) / PNG_BLOCK); }

// Every block costs at most what it costs stored behind the worst bit position (3 + 7 bits, LEN, NLEN, the bytes): 42 bits + its bytes.
// With the 2 bytes in front and Adler-32 behind: length + 6 + ceil(5.25 blocks) <= length + 6 blocks + 7.
inline long long deflate_max_bytes(long long length) { return length + 6 + (21LL * deflate_blocks(length) + 3) / 4; }

inline int deflate_geom_fill(DeflateGeom& g, int n, long long length, long long stride, const char** why) {
    if (n < 0 || length < 0) return *why = "n < 0 or length < 0", SAGEN_ERR_SHAPE;
    if (stride < 4 || stride % 4) return *why = "stride < 4 or not a multiple of 4", SAGEN_ERR_SHAPE;
    if (n > PNG_MAX_FRAMES) return *why = "n above 65535", SAGEN_ERR_UNSUPPORTED;
    if (length > PNG_MAX_LENGTH || stride > PNG_MAX_STRIDE) return *why = "length or stride above 2^28", SAGEN_ERR_UNSUPPORTED;
    g.n = n, g.length = length, g.stride = stride;
    g.nblocks = deflate_blocks(length);
    g.cap = (deflate_max_bytes(length) + 15) / 16 * 16;
    return SAGEN_OK;
}

// The stream is kept at its BOUND in scratch, as sagen_jpeg_encode keeps its own: sizes[f] is exact whatever the stride, and only
// min(sizes[f], stride) bytes ever reach out.
inline DeflateScratch deflate_scratch_layout(const DeflateGeom& g) {
    DeflateScratch s;
    auto up = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t blocks = (size_t)g.n * g.nblocks;
    s.kind = 0;                                                          // int32 [n][nblocks]: PNG_STORED / FIXED / DYNAMIC
    s.bits = up(s.kind + blocks * sizeof(int32_t));                      // int32 [n][nblocks]: the block's bits (stored: behind its padding)
    s.s1 = up(s.bits + blocks * sizeof(int32_t));                        // uint32 [n][nblocks]: sum of the block's bytes
    s.tt = up(s.s1 + blocks * sizeof(uint32_t));                         // uint64 [n][nblocks]: sum of (block length - position) byte
    s.at = up(s.tt + blocks * sizeof(uint64_t));                         // int64 [n][nblocks]: the block's first bit in the frame's stream
    s.table = up(s.at + blocks * sizeof(int64_t));                       // uint32 [n][nblocks][PNG_SYMS]: (reversed code << 4) | length
    s.stream = up(s.table + blocks * PNG_SYMS * sizeof(uint32_t));       // uint8 [n][cap], zeroed
    s.total = s.stream + (size_t)g.n * (size_t)g.cap;
    return s;
}

inline int deflate_args_check(DeflateGeom& g, const void* data, int n, long long length, const void* out, long long stride, const void* sizes,
                              const void* status, const void* scratch, size_t scratch_bytes, const char** why) {
    const int rc = deflate_geom_fill(g, n, length, stride, why);
    if (rc != SAGEN_OK) return rc;
    if ((!data && length > 0) || !out || !sizes || !status || !scratch) return *why = "null argument", SAGEN_ERR_NULL;
    if ((uintptr_t)out % 4 || (uintptr_t)sizes % 4 || (uintptr_t)status % 4 || (uintptr_t)scratch % 16)
        return *why = "out / sizes / status / scratch must be aligned to 4 / 4 / 4 / 16 bytes", SAGEN_ERR_SHAPE;
    if (scratch_bytes < deflate_scratch_layout(g).total) return *why = "scratch too small", SAGEN_ERR_WORKSPACE;
    return SAGEN_OK;
}

PNG_FN int deflate_block_length(long long length, int b) {
    const long long left = length - (long long)b * PNG_BLOCK;
    return left < PNG_BLOCK ? (int)left : PNG_BLOCK;
}

// ---- tokens ------------------------------------------------------------------------------------------------------------------------
// The token at a position that lies k bytes behind the first byte of its run (a maximal run of equal bytes inside the block) and `rem`
// bytes in front of the run's end (rem >= 1): the run's first byte is a literal, the others are covered in chunks of 258 by matches
// of distance 1, a last chunk shorter than 3 by literals.  Returns 0: nothing starts here, 1: a literal, 2: a match of `len`.
PNG_FN int png_token(int k, int rem, int& len) {
    len = 0;
    if (k == 0) return 1;
    const int r = (k - 1) % 258;                                         // the position inside its chunk
    const int chunk = rem + r < 258 ? rem + r : 258;
    if (chunk < 3) return 1;
    if (r) return 0;
    len = chunk;
    return 2;
}

// match length 3..258 -> its symbol, the number of extra bits and their value (RFC 1951, 3.2.5)
PNG_FN void png_length_symbol(int len, int& sym, int& ebits, int& extra) {
    const int l = len - 3;
    ebits = 0, extra = 0;
    if (len == 258) {
        sym = 285;
    } else if (l < 8) {
        sym = 257 + l;
    } else {
        int hb = 3;
        while (l >> (hb + 1)) ++hb;
        ebits = hb - 2;
        sym = 257 + 4 * ebits + 4 + ((l >> ebits) & 3);
        extra = l & ((1 << ebits) - 1);
    }
}

PNG_FN int png_length_extra_bits(int sym) {
    const int c = sym - 257;
    return c < 8 || c == 28 ? 0 : (c - 4) >> 2;
}

PNG_FN void png_fixed_code(int sym, uint32_t& code, int& len) {
    if (sym < 144)
        code = 0x30 + sym, len = 8;
    else if (sym < 256)
        code = 0x190 + sym - 144, len = 9;
    else if (sym < 280)
        code = sym - 256, len = 7;
    else
        code = 0xC0 + sym - 280, len = 8;
}

PNG_FN uint32_t png_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r = (r << 1) | (code & 1), code >>= 1;
    return r;
}

PNG_FN uint32_t png_pack(uint32_t code, int len) { return (png_reverse(code, len) << 4) | (uint32_t)len; }

// ---- one chunk of 64 bytes (16 words, the bytes behind the block's end zero) ---------------------------------------------------------
PNG_FN int png_chunk_byte(const uint32_t* chunk, int i) { return (int)((chunk[i >> 2] >> (8 * (i & 3))) & 255u); }

// bit i: a run starts at position base + i (the block's first byte, a byte unlike the one in front of it, or the block's end l);
// prev: the byte in front of the chunk (anything for base == 0).  s1 / tt: the chunk's share of the two Adler sums.
PNG_FN uint64_t png_chunk_mask(const uint32_t* chunk, int prev, int base, int l, uint32_t& s1, uint32_t& tt) {
    uint64_t neq = 0;
    s1 = 0, tt = 0;
    for (int i = 0; i < PNG_CHUNK; ++i) {
        const int p = base + i, v = png_chunk_byte(chunk, i);
        if (p <= l && (p == 0 || p == l || v != prev)) neq |= 1ull << i;
        if (p < l) s1 += (uint32_t)v, tt += (uint32_t)(l - p) * (uint32_t)v;         // <= 64 x 16384 x 255 < 2^32
        prev = v;
    }
    return neq;
}

// Every token of the chunk in order.  left: the last run start in front of `base` (not read when bit 0 of neq is set); right: the first
// run start at or behind base + 64.  emit(byte, kind, len) with kind 1 or 2.
template <class F>
PNG_FN void png_chunk_walk(const uint32_t* chunk, uint64_t neq, int base, int l, int left, int right, F&& emit) {
    int k = base - 1 - left;
    for (int i = 0; i < PNG_CHUNK; ++i) {
        const int p = base + i;
        if (p >= l) break;
        k = (neq >> i) & 1 ? 0 : k + 1;
        const uint64_t above = i < 63 ? neq >> (i + 1) : 0;
        const int rem = above ? 1 + __builtin_ctzll(above) : right - p;
        int len;
        const int kind = png_token(k, rem, len);
        if (kind) emit(png_chunk_byte(chunk, i), kind, len);
    }
}

// ---- the Huffman code of a block -----------------------------------------------------------------------------------------------------
// The place of symbol s among the used symbols in the order (count, symbol).
PNG_FN int png_huff_rank(const int* hist, int s) {
    const int c = hist[s];
    int r = 0;
    for (int t = 0; t < PNG_SYMS; ++t) {
        const int h = hist[t];
        r += h > 0 && (h < c || (h == c && t < s));
    }
    return r;
}

// a[0..n): the counts in rising order -> the code lengths (falling), n >= 2: the in-place minimum-redundancy construction of Moffat and
// Katajainen (1995); then lengths above 15 are cut to 15 and the Kraft sum is brought back to 1 by moving one code a level down for
// each unit of excess (the heuristic limit, not the optimal one: it matters for counts that fall like Fibonacci numbers only).
// cnt[0..15] is left holding the number of codes of each length.  One caller; the arrays may lie in LDS.
PNG_FN void png_huff_lengths(int* a, int n, int* cnt) {
    for (int l = 0; l <= PNG_MAX_BITS; ++l) cnt[l] = 0;
    if (n < 2) {
        if (n == 1) a[0] = 1, cnt[1] = 1;
        return;
    }
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || a[root] < a[leaf]) {
            a[next] = a[root];
            a[root++] = next;
        } else {
            a[next] = a[leaf++];
        }
        if (leaf >= n || (root < next && a[root] < a[leaf])) {
            a[next] += a[root];
            a[root++] = next;
        } else {
            a[next] += a[leaf++];
        }
    }
    a[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && a[root] == dpth) ++used, --root;
        while (avbl > used) a[next--] = dpth, --avbl;
        avbl = 2 * used, ++dpth, used = 0;
    }
    long long total = 0;
    for (int r = 0; r < n; ++r) {
        const int l = a[r] < PNG_MAX_BITS ? a[r] : PNG_MAX_BITS;
        ++cnt[l];
        total += 1LL << (PNG_MAX_BITS - l);
    }
    while (total > (1LL << PNG_MAX_BITS)) {
        --cnt[PNG_MAX_BITS];
        for (int l = PNG_MAX_BITS - 1; l > 0; --l) {
            if (cnt[l]) {
                --cnt[l], cnt[l + 1] += 2;
                break;
            }
        }
        --total;
    }
    int r = 0;
    for (int l = PNG_MAX_BITS; l > 0; --l)
        for (int c = 0; c < cnt[l]; ++c) a[r++] = l;
}

// the first canonical code of each length (RFC 1951, 3.2.2)
PNG_FN void png_huff_first_codes(const int* cnt, int* first) {
    int code = 0;
    first[0] = 0;
    for (int l = 1; l <= PNG_MAX_BITS; ++l) {
        code = (code + (l > 1 ? cnt[l - 1] : 0)) << 1;
        first[l] = code;
    }
}

PNG_FN uint32_t png_huff_entry(const int* lens, const int* first, int s) {
    const int len = lens[s];
    if (!len) return 0;
    int code = first[len];
    for (int t = 0; t < s; ++t) code += lens[t] == len;
    return png_pack((uint32_t)code, len);
}

// the block's bits as a dynamic and as a fixed block, header, end of block and the distance codes (1 bit / 5 bits a match) included
PNG_FN void png_block_costs(const int* hist, const int* lens, int n_used, int& dyn, int& fix) {
    dyn = PNG_DYN_HEADER, fix = 3;
    for (int s = 0; s < PNG_SYMS; ++s) {
        const int h = hist[s];
        if (!h) continue;
        uint32_t code;
        int fl;
        png_fixed_code(s, code, fl);
        const int extra = s > 256 ? png_length_extra_bits(s) : 0;
        dyn += h * (lens[s] + extra + (s > 256 ? 1 : 0));
        fix += h * (fl + extra + (s > 256 ? 5 : 0));
    }
    if (n_used < 2) dyn = 0x7fffffff;                                    // (the empty block: a code of one symbol is not complete)
}

// The cheapest of stored / fixed / dynamic; a stored block counts at its worst padding, so the choice does not depend on the bits in
// front of it.  bits: what the block adds to the stream (stored: behind the byte boundary that follows its 3 header bits).
PNG_FN int png_block_choice(int l, int dyn, int fix, int& bits) {
    const int stored = 42 + 8 * l;
    if (stored <= fix && stored <= dyn) return bits = 32 + 8 * l, PNG_STORED;
    if (fix <= dyn) return bits = fix, PNG_FIXED;
    return bits = dyn, PNG_DYNAMIC;
}

// where a block ends that starts at bit `pos`
PNG_FN long long png_block_end(long long pos, int kind, int bits) { return (kind == PNG_STORED ? (pos + 3 + 7) & ~7LL : pos) + bits; }

// ---- bits ----------------------------------------------------------------------------------------------------------------------------
// The stream is LSB first: bit i of it is bit i % 32 of little-endian word i / 32.  Huffman codes arrive reversed (png_pack).
PNG_FN void png_or_bits(uint32_t* words, long long pos, uint32_t bits, int len) {     // len <= 32, bits < 2^len
    if (!len) return;
    const uint64_t v = (uint64_t)bits << (pos & 31);
    if ((uint32_t)v) PNG_OR(words + (pos >> 5), (uint32_t)v);
    if (v >> 32) PNG_OR(words + (pos >> 5) + 1, (uint32_t)(v >> 32));
}

// One writer of a contiguous range of bits: a word the range covers wholly is stored, the first and the last are ORed when shared.
struct PngSink {
    uint32_t* words;
    long long w;
    uint64_t acc;
    int n;
    bool shared;
};

PNG_FN void png_sink_open(PngSink& s, uint32_t* words, long long pos) {
    s.words = words, s.w = pos >> 5, s.n = (int)(pos & 31), s.acc = 0, s.shared = s.n != 0;
}

PNG_FN void png_sink_put(PngSink& s, uint32_t bits, int len) {                         // len <= 32, bits < 2^len
    s.acc |= (uint64_t)bits << s.n;
    s.n += len;
    if (s.n >= 32) {
        const uint32_t v = (uint32_t)s.acc;
        if (!s.shared)
            s.words[s.w] = v;
        else if (v)
            PNG_OR(s.words + s.w, v);
        s.acc >>= 32, s.n -= 32, ++s.w, s.shared = false;
    }
}

PNG_FN void png_sink_close(PngSink& s) {
    if (s.n && (uint32_t)s.acc) PNG_OR(s.words + s.w, (uint32_t)s.acc);
}

// a token's bits through table[sym] = (reversed code << 4) | length; dist_bits zeros follow a match (the single distance code 0)
PNG_FN int png_token_bits(const uint32_t* table, int byte, int kind, int len, int dist_bits, uint32_t& bits) {
    if (kind == 1) {
        const uint32_t e = table[byte];
        bits = e >> 4;
        return (int)(e & 15);
    }
    int sym, ebits, extra;
    png_length_symbol(len, sym, ebits, extra);
    const uint32_t e = table[sym];
    const int cl = (int)(e & 15);
    bits = (e >> 4) | ((uint32_t)extra << cl);
    return cl + ebits + dist_bits;                                      // <= 15 + 5 + 5
}

// the first 17 bits of a dynamic block: BFINAL, BTYPE = 2, HLIT = 286, HDIST = 1, HCLEN = 19
PNG_FN uint32_t png_dyn_header17(bool final) { return (final ? 1u : 0u) | (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13); }

// Code-length code: the sixteen lengths 0..15 get 4 bits each (complete), 16 - 18 none.  Item j of the 19 three-bit fields, in the order
// 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15:
PNG_FN uint32_t png_clen_field(int j) { return j < 3 ? 0u : 4u; }

// item s of the 287 code lengths that follow (the 286 of the block's code, then the distance code's 1), 4 bits
PNG_FN uint32_t png_len_field(const uint32_t* table, int s) { return png_reverse(s < PNG_SYMS ? table[s] & 15u : 1u, 4); }

// everything of a dynamic / fixed block but its tokens and the end of block, by ONE writer (the device spreads the fields over threads)
PNG_FN void png_block_header(uint32_t* words, long long at, int kind, bool final, const uint32_t* table) {
    if (kind == PNG_FIXED) {
        png_or_bits(words, at, (final ? 1u : 0u) | (1u << 1), 3);
        return;
    }
    png_or_bits(words, at, png_dyn_header17(final), 17);
    for (int j = 0; j < 19; ++j) png_or_bits(words, at + 17 + 3 * j, png_clen_field(j), 3);
    for (int s = 0; s <= PNG_SYMS; ++s) png_or_bits(words, at + 17 + 57 + 4 * s, png_len_field(table, s), 4);
}

// a stored block's header bits, LEN and NLEN; returns the bit at which its bytes start
PNG_FN long long png_stored_header(uint32_t* words, long long at, bool final, int l) {
    png_or_bits(words, at, final ? 1u : 0u, 3);
    const long long p = (at + 3 + 7) & ~7LL;
    png_or_bits(words, p, (uint32_t)l | ((~(uint32_t)l & 0xffffu) << 16), 32);
    return p + 32;
}

// the bytes of one chunk of a stored block
PNG_FN void png_stored_chunk(uint32_t* words, long long bit, const uint32_t* chunk, int base, int l) {
    if (base >= l) return;
    PngSink s;
    png_sink_open(s, words, bit);
    for (int j = 0; j < PNG_CHUNK / 4; ++j) {
        const int left = l - base - 4 * j;
        if (left <= 0) break;
        const int nb = left < 4 ? left : 4;
        png_sink_put(s, nb < 4 ? chunk[j] & ((1u << (8 * nb)) - 1u) : chunk[j], 8 * nb);
    }
    png_sink_close(s);
}

PNG_FN uint32_t png_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// a block's share of Adler-32's second sum: sum of (length - position) byte over its bytes, mod 65521; o: the block's first position
PNG_FN uint32_t png_adler_share(long long length, long long o, int l, uint32_t s1, uint64_t tt) {
    return (uint32_t)(((uint64_t)((length - o - l) % PNG_ADLER) * (s1 % PNG_ADLER) + tt % PNG_ADLER) % PNG_ADLER);
}

// the frame's two ends: 78 01 in front, Adler-32 (big-endian) behind the last block's byte; returns the stream's bytes
PNG_FN long long png_frame_ends(uint32_t* words, long long end_bit, long long length, uint32_t sum1, uint32_t sum2) {
    const long long bytes = (end_bit + 7) >> 3;
    const uint32_t a = (1 + sum1) % PNG_ADLER, b = (uint32_t)((length % PNG_ADLER + sum2) % PNG_ADLER);
    png_or_bits(words, 0, 0x0178u, 16);
    png_or_bits(words, 8 * bytes, png_bswap((b << 16) | a), 32);
    return bytes + 4;
}

// ---- the host loop -------------------------------------------------------------------------------------------------------------------
struct PngBlockPlan {
    uint64_t masks[PNG_CHUNKS];
    uint32_t chunks[PNG_CHUNKS][PNG_CHUNK / 4];
    int left[PNG_CHUNKS], right[PNG_CHUNKS];
};

// the chunks of block `src[0..l)`, their run masks and each chunk's nearest run starts on either side
inline void png_block_stage_host(const uint8_t* src, int l, PngBlockPlan& p, uint32_t& s1, uint64_t& tt) {
    s1 = 0, tt = 0;
    std::memset(p.chunks, 0, sizeof(p.chunks));
    if (l > 0) std::memcpy(p.chunks, src, (size_t)l);
    for (int t = 0; t < PNG_CHUNKS; ++t) {
        uint32_t a, b;
        p.masks[t] = png_chunk_mask(p.chunks[t], t ? png_chunk_byte(p.chunks[t - 1], PNG_CHUNK - 1) : 0, t * PNG_CHUNK, l, a, b);
        s1 += a, tt += b;
    }
    int last = 0;
    for (int t = 0; t < PNG_CHUNKS; ++t) {
        p.left[t] = last;
        if (p.masks[t]) last = t * PNG_CHUNK + 63 - __builtin_clzll(p.masks[t]);
    }
    int next = l;
    for (int t = PNG_CHUNKS - 1; t >= 0; --t) {
        p.right[t] = next;
        if (p.masks[t]) next = t * PNG_CHUNK + __builtin_ctzll(p.masks[t]);
    }
}

// sagen_deflate on host pointers, after deflate_args_check: the device's passes (png.hip) as loops over frames, blocks and chunks
inline void deflate_host(const uint8_t* data, const DeflateGeom& g, uint8_t* out, int32_t* sizes, int32_t* status, void* scratch) {
    const DeflateScratch lay = deflate_scratch_layout(g);
    char* base = (char*)scratch;
    int32_t* kind = (int32_t*)(base + lay.kind);
    int32_t* bits = (int32_t*)(base + lay.bits);
    uint32_t* s1 = (uint32_t*)(base + lay.s1);
    uint64_t* tt = (uint64_t*)(base + lay.tt);
    int64_t* at = (int64_t*)(base + lay.at);
    uint32_t* tables = (uint32_t*)(base + lay.table);
    std::memset(base + lay.stream, 0, (size_t)g.n * (size_t)g.cap);
    PngBlockPlan* plan = new PngBlockPlan;
    for (int f = 0; f < g.n; ++f) {
        uint32_t* words = (uint32_t*)(base + lay.stream + (size_t)f * (size_t)g.cap);
        // the plan of every block
        for (int b = 0; b < g.nblocks; ++b) {
            const size_t id = (size_t)f * g.nblocks + b;
            const int l = deflate_block_length(g.length, b);
            png_block_stage_host(l > 0 ? data + (size_t)f * (size_t)g.length + (size_t)b * PNG_BLOCK : nullptr, l, *plan, s1[id], tt[id]);
            int hist[PNG_SYMS] = {}, a[PNG_SYMS], order[PNG_SYMS], lens[PNG_SYMS] = {}, cnt[PNG_MAX_BITS + 1], first[PNG_MAX_BITS + 1];
            for (int t = 0; t < PNG_CHUNKS; ++t)
                png_chunk_walk(plan->chunks[t], plan->masks[t], t * PNG_CHUNK, l, plan->left[t], plan->right[t], [&](int byte, int k, int len) {
                    int sym = byte, ebits, extra;
                    if (k == 2) png_length_symbol(len, sym, ebits, extra);
                    ++hist[sym];
                });
            hist[256] = 1;
            int n_used = 0;
            for (int s = 0; s < PNG_SYMS; ++s) {
                if (!hist[s]) continue;
                const int r = png_huff_rank(hist, s);
                order[r] = s, a[r] = hist[s], ++n_used;
            }
            png_huff_lengths(a, n_used, cnt);
            png_huff_first_codes(cnt, first);
            for (int r = 0; r < n_used; ++r) lens[order[r]] = a[r];
            int dyn, fix, nbits;
            png_block_costs(hist, lens, n_used, dyn, fix);
            kind[id] = png_block_choice(l, dyn, fix, nbits);
            bits[id] = nbits;
            for (int s = 0; s < PNG_SYMS; ++s) tables[id * PNG_SYMS + s] = png_huff_entry(lens, first, s);
        }
        // positions, Adler-32, the size
        long long pos = 16;
        uint32_t sum1 = 0, sum2 = 0;
        for (int b = 0; b < g.nblocks; ++b) {
            const size_t id = (size_t)f * g.nblocks + b;
            const int l = deflate_block_length(g.length, b);
            at[id] = pos;
            pos = png_block_end(pos, kind[id], bits[id]);
            sum1 = (sum1 + s1[id] % PNG_ADLER) % PNG_ADLER;
            sum2 = (sum2 + png_adler_share(g.length, (long long)b * PNG_BLOCK, l, s1[id], tt[id])) % PNG_ADLER;
        }
        const long long need = png_frame_ends(words, pos, g.length, sum1, sum2);
        sizes[f] = (int32_t)need;
        status[f] = need > g.stride ? SAGEN_DEFLATE_ST_CAPACITY : 0;
        // the bits
        for (int b = 0; b < g.nblocks; ++b) {
            const size_t id = (size_t)f * g.nblocks + b;
            const int l = deflate_block_length(g.length, b);
            const bool final = b == g.nblocks - 1;
            uint32_t unused1;
            uint64_t unused2;
            png_block_stage_host(l > 0 ? data + (size_t)f * (size_t)g.length + (size_t)b * PNG_BLOCK : nullptr, l, *plan, unused1, unused2);
            if (kind[id] == PNG_STORED) {
                const long long body = png_stored_header(words, at[id], final, l);
                for (int t = 0; t < PNG_CHUNKS; ++t) png_stored_chunk(words, body + 8LL * t * PNG_CHUNK, plan->chunks[t], t * PNG_CHUNK, l);
                continue;
            }
            uint32_t table[PNG_SYMS];
            for (int s = 0; s < PNG_SYMS; ++s) {
                uint32_t code;
                int len;
                png_fixed_code(s, code, len);
                table[s] = kind[id] == PNG_FIXED ? png_pack(code, len) : tables[id * PNG_SYMS + s];
            }
            const int dist_bits = kind[id] == PNG_FIXED ? 5 : 1;
            png_block_header(words, at[id], kind[id], final, table);
            long long p = at[id] + (kind[id] == PNG_FIXED ? 3 : PNG_DYN_HEADER);
            for (int t = 0; t < PNG_CHUNKS; ++t) {
                PngSink s;
                png_sink_open(s, words, p);
                png_chunk_walk(plan->chunks[t], plan->masks[t], t * PNG_CHUNK, l, plan->left[t], plan->right[t], [&](int byte, int k, int len) {
                    uint32_t v;
                    const int nb = png_token_bits(table, byte, k, len, dist_bits, v);
                    png_sink_put(s, v, nb);
                    p += nb;
                });
                png_sink_close(s);
            }
            png_or_bits(words, p, table[256] >> 4, (int)(table[256] & 15));
        }
        const long long copy = sizes[f] < g.stride ? sizes[f] : g.stride;
        std::memcpy(out + (size_t)f * (size_t)g.stride, words, (size_t)copy);
    }
    delete plan;
}

}  // namespace sagen
