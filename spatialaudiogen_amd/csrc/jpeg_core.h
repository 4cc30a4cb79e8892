// Baseline JPEG decode (include/sagen.h: sagen_jpeg_decode): the per-lane entropy decode, the per-block inverse DCT and the
// per-pixel upsampling and colour conversion, in the integer arithmetic of libjpeg's default path ("islow" inverse DCT, "fancy"
// triangle upsampling, 16-bit fixed-point YCbCr -> RGB), so that the result is that library's byte for byte.  It replaces the
// host decode behind every frame reader of the reference (feeder.py:18-23, PIL / skimage).
//
// The same code runs on the device (jpeg.hip) and on the host (csrc_cpu/sagen_cpu.cpp, tools/jpeg_mutate.cpp: plain loops).
//
// Hostile input: the bytes come from files.  Every loop below is bounded by the checked geometry (MCUs x blocks x at most 64
// coefficient steps x at most 16 code bits), every index into a table is either proven in range by jpeg_check_frame /
// jpeg_huff_build or masked, the bit window never loads a word outside [start, end) of its segment, and the transform's arithmetic
// is unsigned (wraps modulo 2^32 where a hostile stream overflows it; for coefficients an encoder can make from 8-bit samples no
// intermediate leaves 31 bits and the result is the signed one).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define JPEG_FN __host__ __device__ __forceinline__
#else
#define JPEG_FN inline
#endif
#if defined(__clang__)
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_UNROLL
#endif

namespace sagen {

constexpr int JPEG_MAX_DIM = 16384;
constexpr int JPEG_MAX_FRAMES = 65535;
constexpr int JPEG_HUFF_SPEC = 272;            // 16 counts + 256 symbols
constexpr int JPEG_MAX_RESTART = 65535;

// What a checked call works with, by value in the kernel arguments.
struct JpegGeom {
    int n, w, h, ncomp, hs, vs;
    int mcus_x, mcus_y, mcus, bpm;             // MCUs per row / column / frame, blocks per MCU
    int yw, yh, cw, ch;                        // padded planes (multiples of 8); cw = ch = 0 for grey
    int dw, dh;                                // the chroma planes' true size: ceil(w / hs) x ceil(h / vs)
    int blocks;                                // per frame
    int plane_bytes;                           // per frame: yw yh + 2 cw ch
};

// a Huffman table as the decoder wants it (jpeg_huff_build)
struct JpegHuff {
    uint16_t lut[256];                         // next 8 bits -> (length << 8) | symbol, 0: no code of <= 8 bits
    int32_t maxcode[18];                       // [l]: the largest code of length l, -1: none
    int32_t valoff[17];                        // [l]: index of the first symbol of length l minus its code
    uint8_t sym[256];
    int32_t ok;
};
static_assert(sizeof(JpegHuff) == 912, "JpegHuff is carved out of the scratch in 16-byte units");
static_assert(sizeof(sagen_jpeg_frame) == 64, "include/sagen.h documents 64 bytes");

struct JpegScratch {
    size_t huff, coef, planes, total;          // byte offsets of the three regions
};

inline int jpeg_geom_fill(JpegGeom& g, int n, int w, int h, int ncomp, int hs, int vs, const char** why) {
    *why = "";
    if (n < 0 || w < 1 || h < 1) return *why = "n < 0 or a dimension < 1", SAGEN_ERR_SHAPE;
    const bool grey = ncomp == 1 && hs == 1 && vs == 1;
    const bool colour = ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
    if (!grey && !colour) return *why = "components / sampling outside 1 x (1,1), 3 x {(1,1), (2,1), (2,2)}", SAGEN_ERR_UNSUPPORTED;
    if (w > JPEG_MAX_DIM || h > JPEG_MAX_DIM || n > JPEG_MAX_FRAMES) return *why = "a dimension above 16384 or n > 65535", SAGEN_ERR_UNSUPPORTED;
    g.n = n, g.w = w, g.h = h, g.ncomp = ncomp, g.hs = hs, g.vs = vs;
    g.mcus_x = (w + 8 * hs - 1) / (8 * hs), g.mcus_y = (h + 8 * vs - 1) / (8 * vs), g.mcus = g.mcus_x * g.mcus_y;
    g.bpm = ncomp == 1 ? 1 : hs * vs + 2;
    g.yw = g.mcus_x * 8 * hs, g.yh = g.mcus_y * 8 * vs;
    g.cw = ncomp == 1 ? 0 : g.mcus_x * 8, g.ch = ncomp == 1 ? 0 : g.mcus_y * 8;
    g.dw = (w + hs - 1) / hs, g.dh = (h + vs - 1) / vs;
    g.blocks = g.mcus * g.bpm;
    g.plane_bytes = g.yw * g.yh + 2 * g.cw * g.ch;
    if ((long long)n * g.blocks > 0x7fffffffLL || (long long)n * w * h * 3 > 0x7fffffffLL)
        return *why = "more than 2^31 - 1 blocks or output bytes in one call", SAGEN_ERR_UNSUPPORTED;
    return SAGEN_OK;
}

inline JpegScratch jpeg_scratch_layout(const JpegGeom& g, int n_hufftabs) {
    JpegScratch s;
    s.huff = 0;
    s.coef = (size_t)n_hufftabs * sizeof(JpegHuff);                               // 912 = 57 x 16
    s.planes = s.coef + (size_t)g.n * g.blocks * 64 * sizeof(int16_t);            // 128 bytes per block
    s.total = s.planes + ((size_t)g.n * g.plane_bytes + 15) / 16 * 16;
    return s;
}

// the checks of sagen_jpeg_decode that need no look at device memory; g is filled when SAGEN_OK comes back
inline int jpeg_args_check(JpegGeom& g, const void* bytes, long long total_bytes, const void* frames, int n, const void* segments, int n_segments,
                           const void* qtabs, int n_qtabs, const void* hufftabs, int n_hufftabs, int w, int h, int ncomp, int hs, int vs,
                           const void* out, const void* status, const void* scratch, size_t scratch_bytes, const char** why) {
    const int rc = jpeg_geom_fill(g, n, w, h, ncomp, hs, vs, why);
    if (rc != SAGEN_OK) return rc;
    if (!bytes || !frames || !segments || !qtabs || !hufftabs || !out || !status || !scratch) return *why = "null argument", SAGEN_ERR_NULL;
    if (total_bytes < 0 || total_bytes % 4) return *why = "total_bytes negative or not a multiple of 4", SAGEN_ERR_SHAPE;
    if (total_bytes > 0x7fffffffLL) return *why = "more than 2^31 - 1 bytes in one call", SAGEN_ERR_UNSUPPORTED;
    if (n_segments < n || n_qtabs < 1 || n_hufftabs < 1) return *why = "n_segments < n or a table count < 1", SAGEN_ERR_SHAPE;
    if (n_hufftabs > 65536 || n_qtabs > 65536) return *why = "more than 65536 tables", SAGEN_ERR_UNSUPPORTED;
    if ((uintptr_t)bytes % 4 || (uintptr_t)frames % 8 || (uintptr_t)segments % 4 || (uintptr_t)qtabs % 2 || (uintptr_t)status % 4 ||
        (uintptr_t)scratch % 16)
        return *why = "bytes / frames / segments / qtabs / status / scratch must be aligned to 4 / 8 / 4 / 2 / 4 / 16 bytes", SAGEN_ERR_SHAPE;
    if (scratch_bytes < jpeg_scratch_layout(g, n_hufftabs).total) return *why = "scratch too small", SAGEN_ERR_WORKSPACE;
    return SAGEN_OK;
}

// ---- Huffman tables --------------------------------------------------------------------------------------------------------------
JPEG_FN void jpeg_huff_build(const uint8_t* spec, JpegHuff& t) {
    int total = 0;
    for (int l = 0; l < 16; ++l) total += spec[l];
    for (int i = 0; i < 256; ++i) t.lut[i] = 0, t.sym[i] = spec[16 + i];
    for (int l = 0; l < 18; ++l) t.maxcode[l] = -1;
    for (int l = 0; l < 17; ++l) t.valoff[l] = 0;
    t.ok = 0;
    if (total > 256) return;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = spec[l - 1];
        if (code + cnt > (1 << l)) return;                       // not a prefix code: the codes of this length do not fit
        t.valoff[l] = k - code;
        if (cnt) t.maxcode[l] = code + cnt - 1;
        if (l <= 8)
            for (int c = 0; c < cnt; ++c)
                for (int j = 0; j < (1 << (8 - l)); ++j) t.lut[((code + c) << (8 - l)) + j] = (uint16_t)((l << 8) | spec[16 + k + c]);
        k += cnt;
        code = (code + cnt) << 1;
    }
    t.ok = 1;
}

// ---- the bit window ----------------------------------------------------------------------------------------------------------------
// 32 bits, the next bit at the top.  Bytes come out of one cached aligned word; FF 00 gives FF; a byte wanted at or behind `end`
// is a zero that counts as `fake`: a lane has overrun its segment when it has consumed one (nbits < fake).
struct JpegBits {
    const uint32_t* words;
    uint32_t pos, end, cur, buf;
    int nbits, fake;
    uint32_t st;
};

JPEG_FN void jpeg_bits_open(JpegBits& b, const uint8_t* bytes, uint32_t start, uint32_t end) {
    b.words = (const uint32_t*)bytes;
    b.pos = start, b.end = end, b.buf = 0, b.nbits = 0, b.fake = 0, b.st = 0;
    b.cur = start < end ? b.words[start >> 2] : 0;
}

JPEG_FN uint32_t jpeg_next_byte(JpegBits& b) {                    // pos < end
    const uint32_t v = (b.cur >> (8 * (b.pos & 3))) & 255u;
    ++b.pos;
    if ((b.pos & 3) == 0 && b.pos < b.end) b.cur = b.words[b.pos >> 2];
    return v;
}

JPEG_FN void jpeg_fill(JpegBits& b) {
    while (b.nbits <= 24) {
        uint32_t v = 0;
        if (b.pos < b.end) {
            v = jpeg_next_byte(b);
            if (v == 0xFF) {
                if (b.pos < b.end) {
                    if (jpeg_next_byte(b) != 0) b.st |= SAGEN_JPEG_ST_MARKER, b.pos = b.end, b.fake += 8, v = 0;   // a marker inside the segment
                } else {
                    b.st |= SAGEN_JPEG_ST_OVERRUN, b.fake += 8, v = 0;                                           // cut between FF and 00
                }
            }
        } else {
            b.fake += 8;
        }
        b.buf |= v << (24 - b.nbits);
        b.nbits += 8;
    }
}

JPEG_FN void jpeg_skip(JpegBits& b, int n) { b.buf <<= n, b.nbits -= n; }

JPEG_FN int jpeg_get_bits(JpegBits& b, int n) {                   // 1 <= n <= 16
    jpeg_fill(b);
    const int v = (int)(b.buf >> (32 - n));
    jpeg_skip(b, n);
    return v;
}

JPEG_FN int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// the next symbol, or -1 (SAGEN_JPEG_ST_CODE)
JPEG_FN int jpeg_decode_symbol(JpegBits& b, const JpegHuff& t) {
    jpeg_fill(b);
    const uint32_t e = t.lut[b.buf >> 24];
    if (e) {
        jpeg_skip(b, (int)(e >> 8));
        return (int)(e & 255u);
    }
    const int top = (int)(b.buf >> 16);
    for (int l = 9; l <= 16; ++l) {
        const int code = top >> (16 - l);
        if (code <= t.maxcode[l]) {
            jpeg_skip(b, l);
            return t.sym[(code + t.valoff[l]) & 255];
        }
    }
    b.st |= SAGEN_JPEG_ST_CODE;
    return -1;
}

// natural (row-major) position of the k-th coefficient of the zigzag order
JPEG_FN int jpeg_natural(int k) {
    static constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[k & 63];
}

JPEG_FN int jpeg_block_component(const JpegGeom& g, int j) { return g.ncomp == 1 || j < g.hs * g.vs ? 0 : j - g.hs * g.vs + 1; }

// ---- descriptors -------------------------------------------------------------------------------------------------------------------
// 0, or the status bits of a frame whose descriptor, segment rows or tables cannot be used; nothing of such a frame is decoded
JPEG_FN uint32_t jpeg_check_frame(const sagen_jpeg_frame& f, int fi, const int32_t* segments, int n_segments, long long total_bytes, int n_qtabs,
                                  int n_hufftabs, const JpegGeom& g, const JpegHuff* huff) {
    if (f.scan_offset < 0 || f.scan_bytes < 0 || f.scan_offset + (long long)f.scan_bytes > total_bytes) return SAGEN_JPEG_ST_DESC;
    if (f.restart_interval < 0 || f.restart_interval > JPEG_MAX_RESTART) return SAGEN_JPEG_ST_DESC;
    const int want = f.restart_interval ? (g.mcus + f.restart_interval - 1) / f.restart_interval : 1;
    if (f.n_segments != want || f.first_segment < 0 || (long long)f.first_segment + f.n_segments > n_segments) return SAGEN_JPEG_ST_DESC;
    uint32_t st = 0;
    for (int c = 0; c < g.ncomp; ++c) {
        if (f.qtab[c] < 0 || f.qtab[c] >= n_qtabs || f.dctab[c] < 0 || f.dctab[c] >= n_hufftabs || f.actab[c] < 0 || f.actab[c] >= n_hufftabs)
            return SAGEN_JPEG_ST_DESC;
        if (!huff[f.dctab[c]].ok || !huff[f.actab[c]].ok) st |= SAGEN_JPEG_ST_TABLE;
    }
    const int32_t* rows = segments + 2 * (size_t)f.first_segment;
    for (int k = 0; k < f.n_segments; ++k) {
        const int32_t off = rows[2 * k + 1];
        if (rows[2 * k] != fi || off > f.scan_bytes || (k == 0 ? off != 0 : off < rows[2 * k - 1] + 2)) return SAGEN_JPEG_ST_DESC;
    }
    return st;
}

// ---- entropy decode of one segment ---------------------------------------------------------------------------------------------------
// Segment k of a frame that passed jpeg_check_frame: its MCUs' non-zero coefficients, undequantised, in natural order, into the
// frame's (zeroed) coefficient blocks coef[(mcu bpm + j) 64 ..].  Returns the status bits it found.
JPEG_FN uint32_t jpeg_decode_segment(const uint8_t* bytes, const sagen_jpeg_frame& f, const int32_t* segments, int k, const JpegGeom& g,
                                     const JpegHuff* huff, int16_t* coef) {
    const int32_t* rows = segments + 2 * (size_t)f.first_segment;
    const uint32_t start = (uint32_t)(f.scan_offset + rows[2 * k + 1]);
    const uint32_t end = (uint32_t)(f.scan_offset + (k + 1 < f.n_segments ? rows[2 * k + 3] - 2 : f.scan_bytes));
    if (k > 0 && (bytes[start - 2] != 0xFF || bytes[start - 1] != 0xD0 + ((k - 1) & 7))) return SAGEN_JPEG_ST_MARKER;
    const int ri = f.restart_interval;
    const int m0 = ri ? k * ri : 0, m1 = ri && m0 + ri < g.mcus ? m0 + ri : g.mcus;
    JpegBits b;
    jpeg_bits_open(b, bytes, start, end);
    int pred[3] = {0, 0, 0};
    for (int m = m0; m < m1; ++m) {
        for (int j = 0; j < g.bpm; ++j) {
            const int c = jpeg_block_component(g, j);
            const JpegHuff& dc = huff[f.dctab[c]];
            const JpegHuff& ac = huff[f.actab[c]];
            int16_t* blk = coef + ((size_t)m * g.bpm + j) * 64;
            const int t = jpeg_decode_symbol(b, dc);
            if (t < 0) return b.st;
            if (t > 11) return b.st | SAGEN_JPEG_ST_RANGE;
            // (three named predictors, not pred[c]: a register array indexed at run time would live in scratch memory)
            int p = c == 0 ? pred[0] : (c == 1 ? pred[1] : pred[2]);
            if (t) p += jpeg_extend(jpeg_get_bits(b, t), t);
            if (p < -32768 || p > 32767) return b.st | SAGEN_JPEG_ST_RANGE;
            if (c == 0) pred[0] = p; else if (c == 1) pred[1] = p; else pred[2] = p;
            if (p) blk[0] = (int16_t)p;
            for (int i = 1; i < 64;) {
                const int rs = jpeg_decode_symbol(b, ac);
                if (rs < 0) return b.st;
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (r != 15) break;                                  // EOB
                    i += 16;                                             // ZRL
                    if (i > 64) return b.st | SAGEN_JPEG_ST_INDEX;
                    continue;
                }
                i += r;
                if (i > 63) return b.st | SAGEN_JPEG_ST_INDEX;
                if (s > 10) return b.st | SAGEN_JPEG_ST_RANGE;
                blk[jpeg_natural(i)] = (int16_t)jpeg_extend(jpeg_get_bits(b, s), s);   // (never 0: EXTEND of s >= 1 bits)
                ++i;
            }
            if (b.nbits < b.fake) return b.st | SAGEN_JPEG_ST_OVERRUN;
            if (b.st) return b.st;
        }
    }
    // what is left may be the padding of the last byte, nothing more
    if (b.pos < b.end || b.nbits - b.fake >= 8) b.st |= SAGEN_JPEG_ST_TRAILING;
    return b.st;
}

// ---- inverse DCT ---------------------------------------------------------------------------------------------------------------------
JPEG_FN int jpeg_sar(uint32_t x, int n) { return (int)x >> n; }   // arithmetic shift of the signed reading

// one 1-D pass of jidctint.c's jpeg_idct_islow on in[0 .. 7 stride], before the descale
JPEG_FN void jpeg_idct_1d(const uint32_t i0, const uint32_t i1, const uint32_t i2, const uint32_t i3, const uint32_t i4, const uint32_t i5,
                          const uint32_t i6, const uint32_t i7, uint32_t o[8]) {
    uint32_t z1 = (i2 + i6) * 4433u;
    uint32_t tmp2 = z1 - i6 * 15137u, tmp3 = z1 + i2 * 6270u;
    uint32_t tmp0 = (i0 + i4) * 8192u, tmp1 = (i0 - i4) * 8192u;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i7, tmp1 = i5, tmp2 = i3, tmp3 = i1;
    z1 = tmp0 + tmp3;
    uint32_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995, z3 *= (uint32_t)-16069, z4 *= (uint32_t)-3196;
    z3 += z5, z4 += z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3, o[7] = tmp10 - tmp3, o[1] = tmp11 + tmp2, o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1, o[5] = tmp12 - tmp1, o[3] = tmp13 + tmp0, o[4] = tmp13 - tmp0;
}

JPEG_FN uint8_t jpeg_clamp(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// coef: one block's 64 undequantised coefficients in natural order; q: its table in zigzag order -> px[64] row-major samples.
// Every index below is a constant once the loops are unrolled: ws lives in registers on the device.
JPEG_FN void jpeg_idct_block(const int16_t* coef, const uint16_t* q, uint8_t px[64]) {
    uint32_t ws[64];
    JPEG_UNROLL
    for (int k = 0; k < 64; ++k) {
        constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
        ws[nat[k]] = (uint32_t)(int32_t)coef[nat[k]] * (uint32_t)q[k];
    }
    JPEG_UNROLL
    for (int c = 0; c < 8; ++c) {                                                   // columns: (x + 1024) >> 11
        uint32_t o[8];
        jpeg_idct_1d(ws[c], ws[8 + c], ws[16 + c], ws[24 + c], ws[32 + c], ws[40 + c], ws[48 + c], ws[56 + c], o);
        JPEG_UNROLL
        for (int r = 0; r < 8; ++r) ws[8 * r + c] = (uint32_t)jpeg_sar(o[r] + 1024u, 11);
    }
    JPEG_UNROLL
    for (int r = 0; r < 8; ++r) {                                                   // rows: (x + 2^17) >> 18, + 128, clamped
        uint32_t o[8];
        jpeg_idct_1d(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6], ws[8 * r + 7], o);
        JPEG_UNROLL
        for (int c = 0; c < 8; ++c) px[8 * r + c] = jpeg_clamp(jpeg_sar(o[c] + (1u << 17), 18) + 128);
    }
}

// where block j of MCU m lands: the component's plane (offset inside the frame's planes), its row length, the block's corner
JPEG_FN void jpeg_block_place(const JpegGeom& g, int m, int j, int& comp, size_t& plane, int& stride, int& x0, int& y0) {
    const int mx = m % g.mcus_x, my = m / g.mcus_x;
    comp = jpeg_block_component(g, j);
    if (comp == 0) {
        plane = 0, stride = g.yw;
        x0 = (mx * g.hs + j % g.hs) * 8, y0 = (my * g.vs + j / g.hs) * 8;
    } else {
        plane = (size_t)g.yw * g.yh + (size_t)(comp - 1) * g.cw * g.ch, stride = g.cw;
        x0 = mx * 8, y0 = my * 8;
    }
}

// ---- upsampling and colour -----------------------------------------------------------------------------------------------------------
// the chroma sample of output pixel (x, y): jdsample.c's fullsize copy, h2v1_fancy_upsample or h2v2_fancy_upsample on the
// dw x dh plane p (rows of `stride` bytes), neighbours replicated at the plane's own edges
JPEG_FN int jpeg_chroma(const uint8_t* p, int stride, int dw, int dh, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * stride + x];
    const int c = x >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (size_t)y * stride;
        if (x & 1) return c == dw - 1 ? row[c] : (3 * row[c] + row[c + 1] + 2) >> 2;
        return c == 0 ? row[0] : (3 * row[c] + row[c - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    int rn = (y & 1) ? r + 1 : r - 1;
    rn = rn < 0 ? 0 : (rn > dh - 1 ? dh - 1 : rn);
    const uint8_t* near = p + (size_t)r * stride;
    const uint8_t* far = p + (size_t)rn * stride;
    const int here = 3 * near[c] + far[c];
    if (x & 1) return c == dw - 1 ? (4 * here + 7) >> 4 : (3 * here + 3 * near[c + 1] + far[c + 1] + 7) >> 4;
    return c == 0 ? (4 * here + 8) >> 4 : (3 * here + 3 * near[c - 1] + far[c - 1] + 8) >> 4;
}

// pixel (x, y) of a frame from its planes (jdcolor.c's ycc_rgb_convert: F(v) = int(v 65536 + 0.5))
JPEG_FN void jpeg_pixel(const JpegGeom& g, const uint8_t* planes, int x, int y, uint8_t rgb[3]) {
    const int lum = planes[(size_t)y * g.yw + x];
    if (g.ncomp == 1) {
        rgb[0] = rgb[1] = rgb[2] = (uint8_t)lum;
        return;
    }
    const uint8_t* cbp = planes + (size_t)g.yw * g.yh;
    const uint8_t* crp = cbp + (size_t)g.cw * g.ch;
    const int cb = jpeg_chroma(cbp, g.cw, g.dw, g.dh, g.hs, g.vs, x, y) - 128, cr = jpeg_chroma(crp, g.cw, g.dw, g.dh, g.hs, g.vs, x, y) - 128;
    rgb[0] = jpeg_clamp(lum + ((91881 * cr + 32768) >> 16));
    rgb[1] = jpeg_clamp(lum + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    rgb[2] = jpeg_clamp(lum + ((116130 * cb + 32768) >> 16));
}

// ---- the whole decode as plain loops on host pointers (the CPU twin and tools/jpeg_mutate.cpp; jpeg.hip runs the same five
// stages as kernels) ----------------------------------------------------------------------------------------------------------------
// the first stages: zeroed coefficients, the derived tables, every frame's initial status
inline void jpeg_front_host(long long total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, int n_qtabs,
                            const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, JpegHuff* huff, int16_t* coef, int32_t* status) {
    for (size_t i = 0; i < (size_t)g.n * g.blocks * 64; ++i) coef[i] = 0;
    for (int t = 0; t < n_hufftabs; ++t) jpeg_huff_build(hufftabs + (size_t)t * JPEG_HUFF_SPEC, huff[t]);
    for (int f = 0; f < g.n; ++f) status[f] = (int32_t)jpeg_check_frame(frames[f], f, segments, n_segments, total_bytes, n_qtabs, n_hufftabs, g, huff);
}

// one lane per segment; gate (may be null): only the frames whose gate[f] is not 0
inline void jpeg_entropy_host(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, const JpegGeom& g,
                              const JpegHuff* huff, int16_t* coef, int32_t* status, const int32_t* gate) {
    for (int s = 0; s < n_segments; ++s) {
        const int f = segments[2 * (size_t)s];
        if (f < 0 || f >= g.n || (status[f] & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE))) continue;
        if (gate && !gate[f]) continue;
        const long long k = (long long)s - frames[f].first_segment;
        if (k < 0 || k >= frames[f].n_segments) continue;
        status[f] |= (int32_t)jpeg_decode_segment(bytes, frames[f], segments, (int)k, g, huff, coef + (size_t)f * g.blocks * 64);
    }
}

// inverse DCT into the planes, upsampling and colour into out
inline void jpeg_back_host(const sagen_jpeg_frame* frames, const uint16_t* qtabs, const JpegGeom& g, const int16_t* coef, const int32_t* status,
                           uint8_t* planes, uint8_t* out) {
    for (int f = 0; f < g.n; ++f) {
        if (status[f] & SAGEN_JPEG_ST_DESC) continue;
        uint8_t* fp = planes + (size_t)f * g.plane_bytes;
        for (int b = 0; b < g.blocks; ++b) {
            int comp, stride, x0, y0;
            size_t plane;
            jpeg_block_place(g, b / g.bpm, b % g.bpm, comp, plane, stride, x0, y0);
            uint8_t px[64];
            jpeg_idct_block(coef + ((size_t)f * g.blocks + b) * 64, qtabs + (size_t)frames[f].qtab[comp] * 64, px);
            for (int r = 0; r < 8; ++r)
                for (int c = 0; c < 8; ++c) fp[plane + (size_t)(y0 + r) * stride + x0 + c] = px[8 * r + c];
        }
        for (int y = 0; y < g.h; ++y)
            for (int x = 0; x < g.w; ++x) jpeg_pixel(g, fp, x, y, out + (((size_t)f * g.h + y) * g.w + x) * 3);
    }
}

inline void jpeg_decode_host(const uint8_t* bytes, long long total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                             const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out,
                             int32_t* status, void* scratch) {
    const JpegScratch lay = jpeg_scratch_layout(g, n_hufftabs);
    JpegHuff* huff = (JpegHuff*)((char*)scratch + lay.huff);
    int16_t* coef = (int16_t*)((char*)scratch + lay.coef);
    uint8_t* planes = (uint8_t*)scratch + lay.planes;
    jpeg_front_host(total_bytes, frames, segments, n_segments, n_qtabs, hufftabs, n_hufftabs, g, huff, coef, status);
    jpeg_entropy_host(bytes, frames, segments, n_segments, g, huff, coef, status, nullptr);
    jpeg_back_host(frames, qtabs, g, coef, status, planes, out);
}

}  // namespace sagen
