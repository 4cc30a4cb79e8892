// Baseline JPEG encode (include/sagen.h: sagen_jpeg_encode): colour conversion, edge replication, chroma downsampling, the "islow"
// forward DCT, quantisation and the Huffman code of one coefficient, in the integer arithmetic of libjpeg's default path, so that
// the stream is that library's bit for bit.  It replaces the host encode behind the frame writers (PIL's save at quality 95; the
// reference leaves it to ffmpeg's "%06d.jpg" extraction, scraping/preprocess.py:183-196).
//
// The same code runs on the device (jpeg_enc.hip) and on the host (csrc_cpu/sagen_cpu.cpp, tools/jpeg_encode_check.cpp: plain
// loops, jpeg_encode_host below).  Every >> is an arithmetic shift of a signed 32-bit integer; for 8-bit samples nothing leaves
// 32 bits (the largest product is 12 bits + PASS1_BITS + 3 bits of growth + a 15-bit constant).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sagen.h"
#include "jpeg_core.h"

namespace sagen {

constexpr int JPEG_ENC_BLOCK_BITS = 1658;          // 9 + 11 bits of DC, 63 x (16 + 10) bits of AC: sagen_jpeg_encode_max_bytes
constexpr int JPEG_ENC_CODE_BITS = 1660;           // what the tables allow at most: the chroma DC code of category 11 has 11 bits, not 9.
                                                   // The scratch is sized by this one, so that no index rests on what samples can reach
constexpr long long JPEG_ENC_MAX_STRIDE = 1LL << 28;

// What a checked call works with, by value in the kernel arguments.
struct JpegEncGeom {
    int n, w, h, ncomp, hs, vs;
    int mcus_x, mcus_y, bpm;                       // MCUs per row / column, blocks per MCU
    int wb, hb;                                    // luma blocks that hold image samples: ceil(w / 8) x ceil(h / 8); the rest are dummies
    int blocks;                                    // per frame, dummies included
    long long stride;                              // bytes per row of out
    long long cap;                                 // bytes per frame of the unstuffed stream in scratch: its bound, a multiple of 16
    int seg_blocks, nseg;                          // blocks per restart segment and segments per frame; without markers: blocks, 1
    int all_real;                                  // sagen_jpeg_transcode: the coefficients are a file's, every block is coded as it stands
};

// the four standard tables (Annex K.3 - K.6) as an encoder wants them: symbol -> (code << 8) | length, 0: no such symbol
struct JpegEncHuff {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

struct JpegEncSpec {
    uint8_t counts[16];
    uint8_t symbols[162];
    int n;
};

constexpr JpegEncSpec JPEG_ENC_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegEncSpec JPEG_ENC_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegEncSpec JPEG_ENC_AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr JpegEncSpec JPEG_ENC_AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

constexpr void jpeg_enc_huff_fill(const JpegEncSpec& s, uint32_t* table) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int c = 0; c < s.counts[l - 1]; ++c) table[s.symbols[k++]] = (code++ << 8) | (uint32_t)l;
        code <<= 1;
    }
}

constexpr JpegEncHuff jpeg_enc_huff_make() {
    JpegEncHuff t = {};
    jpeg_enc_huff_fill(JPEG_ENC_DC_LUMA, t.dc[0]);
    jpeg_enc_huff_fill(JPEG_ENC_DC_CHROMA, t.dc[1]);
    jpeg_enc_huff_fill(JPEG_ENC_AC_LUMA, t.ac[0]);
    jpeg_enc_huff_fill(JPEG_ENC_AC_CHROMA, t.ac[1]);
    return t;
}

struct JpegEncScratch {
    size_t coef, counts, tiles, tile_at, frame_bits, qok, ff_tiles, ff_at, stream, total;   // byte offsets of the regions
    size_t seg_pad, seg_at;                        // behind the stream, only where nseg > 1
    int scan_tiles;                                // tiles of JPEG_ENC_SCAN_TILE blocks per frame
    long long ff_tiles_n;                          // tiles of JPEG_ENC_FF_TILE unstuffed bytes per frame
};
constexpr int JPEG_ENC_SCAN_TILE = 256;            // blocks per workgroup of the bit-position scan
constexpr int JPEG_ENC_FF_TILE = 4096;             // unstuffed bytes per workgroup of the stuffing scan (256 threads x 16 bytes)

inline long long jpeg_enc_max_bytes(long long blocks) { return 2 * ((blocks * JPEG_ENC_BLOCK_BITS + 7) / 8) + 2; }

// With nseg restart segments: each segment is filled to a byte of its own, and ceil(a / 8) + ceil(b / 8) <= ceil((a + b) / 8) + 1, so
// the unstuffed bytes grow by at most nseg - 1; stuffing can double them (a fill byte that comes out as FF included); the nseg - 1
// markers of two bytes are not stuffed.
inline long long jpeg_enc_rst_max_bytes(long long blocks, long long nseg) { return jpeg_enc_max_bytes(blocks) + 4 * (nseg - 1); }

inline int jpeg_enc_geom_fill(JpegEncGeom& g, int n, int w, int h, int ncomp, int hs, int vs, long long stride, const char** why) {
    JpegGeom d;
    const int rc = jpeg_geom_fill(d, n, w, h, ncomp, hs, vs, why);                 // the decoder's scope is the encoder's
    if (rc != SAGEN_OK) return rc;
    if (stride < 1 || stride % 4) return *why = "stride < 1 or not a multiple of 4", SAGEN_ERR_SHAPE;
    if (stride > JPEG_ENC_MAX_STRIDE) return *why = "stride above 2^28", SAGEN_ERR_UNSUPPORTED;
    g.n = n, g.w = w, g.h = h, g.ncomp = ncomp, g.hs = hs, g.vs = vs;
    g.mcus_x = d.mcus_x, g.mcus_y = d.mcus_y, g.bpm = d.bpm, g.blocks = d.blocks;
    g.wb = (w + 7) / 8, g.hb = (h + 7) / 8;
    g.stride = stride;
    g.cap = (((long long)g.blocks * JPEG_ENC_CODE_BITS + 7) / 8 + 15) / 16 * 16;
    g.seg_blocks = g.blocks, g.nseg = 1, g.all_real = 0;
    return SAGEN_OK;
}

// the restart interval of sagen_jpeg_encode_rst on a filled g: an interval that reaches over the whole frame writes no marker
inline int jpeg_enc_geom_rst(JpegEncGeom& g, int restart_interval, const char** why) {
    if (restart_interval < 0 || restart_interval > 65535) return *why = "restart_interval outside 0..65535", SAGEN_ERR_UNSUPPORTED;
    const long long mcus = (long long)g.mcus_x * g.mcus_y;
    if (restart_interval == 0 || restart_interval >= mcus) return SAGEN_OK;
    g.seg_blocks = restart_interval * g.bpm;
    g.nseg = (int)((mcus + restart_interval - 1) / restart_interval);
    g.cap = (((long long)g.blocks * JPEG_ENC_CODE_BITS + 7) / 8 + (g.nseg - 1) + 15) / 16 * 16;     // a fill of up to 7 bits per segment
    return SAGEN_OK;
}

// The unstuffed stream is kept at its BOUND, not at stride: sizes[f] is then exact whatever the stride, and a frame that does not
// fit costs no second pass to find out what it needs.
inline JpegEncScratch jpeg_enc_scratch_layout(const JpegEncGeom& g) {
    JpegEncScratch s;
    auto up = [](size_t x) { return (x + 15) / 16 * 16; };
    s.scan_tiles = (g.blocks + JPEG_ENC_SCAN_TILE - 1) / JPEG_ENC_SCAN_TILE;
    s.ff_tiles_n = (g.cap + JPEG_ENC_FF_TILE - 1) / JPEG_ENC_FF_TILE;
    s.coef = 0;                                                                    // int16 [n][blocks][64], zigzag order
    s.counts = s.coef + (size_t)g.n * g.blocks * 64 * sizeof(int16_t);             // int32 [n][blocks]: bits, then the position in the tile
    s.tiles = up(s.counts + (size_t)g.n * g.blocks * sizeof(int32_t));             // int32 [n][scan_tiles]: bits per tile
    s.tile_at = up(s.tiles + (size_t)g.n * s.scan_tiles * sizeof(int32_t));        // int64 [n][scan_tiles]: the tile's first bit
    s.frame_bits = up(s.tile_at + (size_t)g.n * s.scan_tiles * sizeof(int64_t));   // int64 [n]
    s.qok = up(s.frame_bits + (size_t)g.n * sizeof(int64_t));                      // int32: whether the quantisation tables may be used
    s.ff_tiles = s.qok + 16;                                                       // int32 [n][ff_tiles_n]: FF bytes per tile
    s.ff_at = up(s.ff_tiles + (size_t)g.n * s.ff_tiles_n * sizeof(int32_t));       // int64 [n][ff_tiles_n]: FF bytes before the tile
    s.stream = up(s.ff_at + (size_t)g.n * s.ff_tiles_n * sizeof(int64_t));         // uint8 [n][cap]
    s.total = s.stream + (size_t)g.n * g.cap;
    s.seg_pad = s.seg_at = s.total;
    if (g.nseg > 1) {
        s.seg_at = s.seg_pad + (size_t)g.n * g.nseg * sizeof(int64_t);             // int64 [n][nseg]: fill bits in front of the segment
        s.total = s.seg_at + (size_t)g.n * g.nseg * sizeof(int64_t);               // int64 [n][nseg]: its first unstuffed byte
    }
    return s;
}

// the checks of sagen_jpeg_encode that need no look at device memory; g is filled when SAGEN_OK comes back
inline int jpeg_enc_args_check(JpegEncGeom& g, const void* frames, int n, int w, int h, int ncomp, int hs, int vs, const void* qtabs, const void* out,
                               long long stride, const void* sizes, const void* status, const void* scratch, size_t scratch_bytes, const char** why,
                               int restart_interval = 0) {
    int rc = jpeg_enc_geom_fill(g, n, w, h, ncomp, hs, vs, stride, why);
    if (rc != SAGEN_OK) return rc;
    rc = jpeg_enc_geom_rst(g, restart_interval, why);
    if (rc != SAGEN_OK) return rc;
    if (!frames || !qtabs || !out || !sizes || !status || !scratch) return *why = "null argument", SAGEN_ERR_NULL;
    if ((uintptr_t)out % 4 || (uintptr_t)sizes % 4 || (uintptr_t)status % 4 || (uintptr_t)qtabs % 2 || (uintptr_t)scratch % 16)
        return *why = "out / sizes / status / qtabs / scratch must be aligned to 4 / 4 / 4 / 2 / 16 bytes", SAGEN_ERR_SHAPE;
    if (scratch_bytes < jpeg_enc_scratch_layout(g).total) return *why = "scratch too small", SAGEN_ERR_WORKSPACE;
    return SAGEN_OK;
}

// ---- where a block lies ------------------------------------------------------------------------------------------------------------
// block b of a frame's scan order: its component (0, 1, 2), its block coordinates in that component's plane, whether it is a dummy
JPEG_FN void jpeg_enc_block_place(const JpegEncGeom& g, int b, int& comp, int& by, int& bx, bool& dummy) {
    const int mcu = b / g.bpm, j = b % g.bpm, my = mcu / g.mcus_x, mx = mcu % g.mcus_x, luma = g.hs * g.vs;     // (grey: hs = vs = 1)
    if (j < luma) {
        comp = 0, by = my * g.vs + j / g.hs, bx = mx * g.hs + j % g.hs;
        dummy = !g.all_real && (by >= g.hb || bx >= g.wb);
    } else {
        comp = j - luma + 1, by = my, bx = mx, dummy = false;
    }
}

// the block whose DC predicts block b's: the nearest earlier block of its component that is no dummy (a dummy repeats the DC in
// front of it, so it changes no prediction), or -1 at the start of the frame.  At most hs vs steps: block 0 of an MCU is never a dummy.
JPEG_FN int jpeg_enc_pred_block_frame(const JpegEncGeom& g, int b) {
    const int luma = g.hs * g.vs, j = b % g.bpm;
    if (j >= luma) return b >= g.bpm ? b - g.bpm : -1;
    int p = b;
    for (int step = 0; step < 5; ++step) {
        p = p % g.bpm == 0 ? p - g.bpm + luma - 1 : p - 1;
        if (p < 0) return -1;
        int comp, by, bx;
        bool dummy;
        jpeg_enc_block_place(g, p, comp, by, bx, dummy);
        if (!dummy) return p;
    }
    return -1;                                                       // (not reached)
}

// the same inside restart segments: a prediction does not reach into the segment in front (a segment starts with an MCU, whose
// block 0 is no dummy, so the dummies of a segment still find the DC they repeat)
JPEG_FN int jpeg_enc_pred_block(const JpegEncGeom& g, int b) {
    const int p = jpeg_enc_pred_block_frame(g, b);
    return g.nseg > 1 && p >= 0 && p / g.seg_blocks != b / g.seg_blocks ? -1 : p;
}

// ---- samples ---------------------------------------------------------------------------------------------------------------------
JPEG_FN int jpeg_enc_component(const uint8_t* px, int comp) {
    const int r = px[0], g = px[1], b = px[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// sample (y, x) of component comp's padded plane, from one frame [h][w][3] (or [h][w] grey).  Columns: the IMAGE's are replicated;
// rows: the image's up to a multiple of vs, then the COMPONENT's last row.
JPEG_FN int jpeg_enc_sample(const JpegEncGeom& g, const uint8_t* frame, int comp, int y, int x) {
    if (g.ncomp == 1) {
        const int yy = y < g.h ? y : g.h - 1, xx = x < g.w ? x : g.w - 1;
        return frame[(size_t)yy * g.w + xx];
    }
    const int fh = comp ? g.hs : 1, fv = comp ? g.vs : 1;
    const int hc = (g.h + fv - 1) / fv;
    if (y >= hc) y = hc - 1;
    int sum = 0;
    for (int j = 0; j < fv; ++j) {
        int yy = y * fv + j;
        yy = yy < g.h ? yy : g.h - 1;
        for (int i = 0; i < fh; ++i) {
            int xx = x * fh + i;
            xx = xx < g.w ? xx : g.w - 1;
            sum += jpeg_enc_component(frame + ((size_t)yy * g.w + xx) * 3, comp);
        }
    }
    if (fh == 1) return sum;
    return fv == 2 ? (sum + 1 + (x & 1)) >> 2 : (sum + (x & 1)) >> 1;
}

// ---- forward DCT and quantisation ------------------------------------------------------------------------------------------------
// one pass over eight values at d[0], d[S], ... d[7 S]; FIRST: the row pass
template <int S, bool FIRST>
JPEG_FN void jpeg_enc_fdct_pass(int* d) {
    constexpr int sh = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7 * S], t1 = d[S] + d[6 * S], t2 = d[2 * S] + d[5 * S], t3 = d[3 * S] + d[4 * S];
    int t7 = d[0] - d[7 * S], t6 = d[S] - d[6 * S], t5 = d[2 * S] - d[5 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4, d[4 * S] = (t10 - t11) * 4;
    } else {
        d[0] = (t10 + t11 + 2) >> 2, d[4 * S] = (t10 - t11 + 2) >> 2;
    }
    const int z = (t12 + t13) * 4433;
    d[2 * S] = (z + t13 * 6270 + (1 << (sh - 1))) >> sh;
    d[6 * S] = (z - t12 * 15137 + (1 << (sh - 1))) >> sh;
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = -16069 * z3 + z5, z4 = -3196 * z4 + z5;
    d[7 * S] = (t4 + z1 + z3 + (1 << (sh - 1))) >> sh;
    d[5 * S] = (t5 + z2 + z4 + (1 << (sh - 1))) >> sh;
    d[3 * S] = (t6 + z2 + z3 + (1 << (sh - 1))) >> sh;
    d[S] = (t7 + z1 + z4 + (1 << (sh - 1))) >> sh;
}

// d: 64 samples minus 128, row-major, transformed in place; q: the table in zigzag order (entries 1..255: the caller checks) ->
// zz[64] quantised coefficients in zigzag order.  Every index is a constant once the loops are unrolled.
JPEG_FN void jpeg_enc_fdct_quant(int* d, const uint16_t* q, int16_t* zz) {
    JPEG_UNROLL
    for (int r = 0; r < 8; ++r) jpeg_enc_fdct_pass<1, true>(d + 8 * r);
    JPEG_UNROLL
    for (int c = 0; c < 8; ++c) jpeg_enc_fdct_pass<8, false>(d + c);
    JPEG_UNROLL
    for (int k = 0; k < 64; ++k) {
        const int c = d[jpeg_natural(k)], Q = 8 * (int)q[k];
        const int a = ((c < 0 ? -c : c) + (Q >> 1)) / Q;
        zz[k] = (int16_t)(c < 0 ? -a : a);
    }
}

// whether a quantisation table entry may be used (a zero would divide; above 255 is no baseline table)
JPEG_FN bool jpeg_enc_qtabs_ok(const uint16_t* qtabs, int ncomp) {
    bool ok = true;
    for (int k = 0; k < (ncomp == 1 ? 64 : 128); ++k) ok = ok && qtabs[k] >= 1 && qtabs[k] <= 255;
    return ok;
}

// block b of `frame` -> zz[64]
JPEG_FN void jpeg_enc_block(const JpegEncGeom& g, const uint8_t* frame, const uint16_t* qtabs, int comp, int by, int bx, int16_t* zz) {
    int d[64];
    JPEG_UNROLL
    for (int r = 0; r < 8; ++r) {
        JPEG_UNROLL
        for (int c = 0; c < 8; ++c) d[8 * r + c] = jpeg_enc_sample(g, frame, comp, 8 * by + r, 8 * bx + c) - 128;
    }
    jpeg_enc_fdct_quant(d, qtabs + (comp ? 64 : 0), zz);
}

// ---- the code of one coefficient ----------------------------------------------------------------------------------------------------
// the magnitude category: the bit length of |v|
JPEG_FN int jpeg_enc_category(int v) {
    uint32_t a = (uint32_t)(v < 0 ? -(long long)v : v);
    int n = 0;
    while (a) ++n, a >>= 1;
    return n;
}

// What one coefficient adds to the stream, right-aligned in `bits` (at most 3 x 11 + 16 + 10 = 59 of them): for the DC (dc = true)
// v is the difference to the prediction; for an AC coefficient v != 0 follows `run` zeros (<= 62): run >> 4 codes of F0, then the
// code of (run & 15) << 4 | category, then the value bits.  Returns the bit count; sets range for a category baseline has no code for
// (the bits are then those of category 0 / 1: the frame is lost, the stream stays bounded).
JPEG_FN int jpeg_enc_code(const JpegEncHuff& t, int tab, bool dc, int run, int v, uint64_t& bits, bool& range) {
    int cat = jpeg_enc_category(v);
    if (cat > (dc ? 11 : 10)) range = true, cat = dc ? 0 : 1, v = dc ? 0 : 1;
    const uint32_t value = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    int len = 0;
    bits = 0;
    if (!dc) {
        const uint32_t zrl = t.ac[tab][0xF0];
        for (int i = 0; i < (run >> 4); ++i) bits = (bits << (zrl & 255)) | (zrl >> 8), len += (int)(zrl & 255);
    }
    const uint32_t e = dc ? t.dc[tab][cat] : t.ac[tab][((run & 15) << 4) | cat];
    bits = (((bits << (e & 255)) | (e >> 8)) << cat) | value;
    return len + (int)(e & 255) + cat;
}

// ---- the host loop -----------------------------------------------------------------------------------------------------------------
struct JpegEncWriter {
    uint8_t* out;
    long long stride, pos;                                           // pos: bytes the stream has needed so far
    uint32_t acc;
    int nacc;                                                        // bits waiting in acc (< 8)
};

inline void jpeg_enc_put(JpegEncWriter& wr, uint64_t bits, int len) {
    for (int i = len - 1; i >= 0; --i) {
        wr.acc = (wr.acc << 1) | (uint32_t)((bits >> i) & 1);
        if (++wr.nacc == 8) {
            if (wr.pos < wr.stride) wr.out[wr.pos] = (uint8_t)wr.acc;
            ++wr.pos;
            if ((wr.acc & 255) == 255) {
                if (wr.pos < wr.stride) wr.out[wr.pos] = 0;
                ++wr.pos;
            }
            wr.acc = 0, wr.nacc = 0;
        }
    }
}

// sagen_jpeg_encode on host pointers, after jpeg_enc_args_check: frame by frame, block by block, bit by bit; the scratch is not used
// With `coef` ([n][blocks][64] int16, zigzag order: sagen_jpeg_transcode) the blocks are taken from there, frames and qtabs are not read.
inline void jpeg_encode_host(const uint8_t* frames, const JpegEncGeom& g, const uint16_t* qtabs, uint8_t* out, int32_t* sizes, int32_t* status,
                             const int16_t* coef = nullptr) {
    static const JpegEncHuff huff = jpeg_enc_huff_make();
    const bool qok = coef || jpeg_enc_qtabs_ok(qtabs, g.ncomp);
    for (int f = 0; f < g.n; ++f) {
        status[f] = qok ? 0 : SAGEN_JPEG_ENC_ST_RANGE;
        sizes[f] = 0;
        if (!qok) continue;
        const uint8_t* frame = coef ? nullptr : frames + (size_t)f * g.h * g.w * g.ncomp;
        JpegEncWriter wr = {out + (size_t)f * g.stride, g.stride, 0, 0, 0};
        int pred[3] = {0, 0, 0};
        bool range = false;
        for (int b = 0; b < g.blocks; ++b) {
            if (g.nseg > 1 && b > 0 && b % g.seg_blocks == 0) {       // a restart: ones to the byte, the marker unstuffed, predictions to 0
                if (wr.nacc) jpeg_enc_put(wr, 0x7F, 8 - wr.nacc);
                const uint8_t marker[2] = {0xFF, (uint8_t)(0xD0 + ((b / g.seg_blocks - 1) & 7))};
                for (int i = 0; i < 2; ++i, ++wr.pos)
                    if (wr.pos < wr.stride) wr.out[wr.pos] = marker[i];
                pred[0] = pred[1] = pred[2] = 0;
            }
            int comp, by, bx;
            bool dummy;
            jpeg_enc_block_place(g, b, comp, by, bx, dummy);
            const int tab = comp ? 1 : 0;
            uint64_t bits;
            if (dummy) {
                const int len = jpeg_enc_code(huff, tab, true, 0, 0, bits, range);
                jpeg_enc_put(wr, bits, len);
                jpeg_enc_put(wr, huff.ac[tab][0] >> 8, (int)(huff.ac[tab][0] & 255));
                continue;
            }
            int16_t zz[64];
            if (coef)
                for (int k = 0; k < 64; ++k) zz[k] = coef[((size_t)f * g.blocks + b) * 64 + k];
            else
                jpeg_enc_block(g, frame, qtabs, comp, by, bx, zz);
            int len = jpeg_enc_code(huff, tab, true, 0, zz[0] - pred[comp], bits, range);
            jpeg_enc_put(wr, bits, len);
            pred[comp] = zz[0];
            int run = 0;
            for (int k = 1; k < 64; ++k) {
                if (zz[k] == 0) {
                    ++run;
                    continue;
                }
                len = jpeg_enc_code(huff, tab, false, run, zz[k], bits, range);
                jpeg_enc_put(wr, bits, len);
                run = 0;
            }
            if (run) jpeg_enc_put(wr, huff.ac[tab][0] >> 8, (int)(huff.ac[tab][0] & 255));
        }
        if (wr.nacc) jpeg_enc_put(wr, 0x7F, 8 - wr.nacc);
        sizes[f] = (int32_t)(wr.pos > 0x7fffffffLL ? 0x7fffffffLL : wr.pos);
        if (wr.pos > g.stride) status[f] |= SAGEN_JPEG_ENC_ST_CAPACITY;
        if (range) status[f] |= SAGEN_JPEG_ENC_ST_RANGE;
    }
}

// ---- sagen_jpeg_transcode: the decoder's entropy stage into coefficients, the encoder's entropy half out of them ------------------------
// a block of a file can hold what the tables allow, not only what 8-bit samples reach: the bound is taken at JPEG_ENC_CODE_BITS
inline long long jpeg_transcode_max_bytes(long long blocks, long long nseg) { return 2 * ((blocks * JPEG_ENC_CODE_BITS + 7) / 8) + 2 + 4 * (nseg - 1); }

struct JpegTranscodeScratch {
    size_t dec, enc, enc_status, total;            // the decoder's tables + natural-order coefficients, the encoder's regions, int32 [n]
};

inline JpegTranscodeScratch jpeg_transcode_scratch_layout(const JpegGeom& d, const JpegEncGeom& g, int n_hufftabs) {
    JpegTranscodeScratch s;
    s.dec = 0;
    s.enc = (jpeg_scratch_layout(d, n_hufftabs).planes + 15) / 16 * 16;            // (the planes are not made)
    s.enc_status = (s.enc + jpeg_enc_scratch_layout(g).total + 15) / 16 * 16;
    s.total = (s.enc_status + (size_t)g.n * sizeof(int32_t) + 15) / 16 * 16;
    return s;
}

// the geometry of both halves; every block of the source scan is coded (all_real)
inline int jpeg_transcode_geom_fill(JpegGeom& d, JpegEncGeom& g, int n, int w, int h, int ncomp, int hs, int vs, int restart_interval, long long stride,
                                    int n_hufftabs, const char** why) {
    int rc = jpeg_geom_fill(d, n, w, h, ncomp, hs, vs, why);
    if (rc != SAGEN_OK) return rc;
    rc = jpeg_enc_geom_fill(g, n, w, h, ncomp, hs, vs, stride, why);
    if (rc != SAGEN_OK) return rc;
    rc = jpeg_enc_geom_rst(g, restart_interval, why);
    if (rc != SAGEN_OK) return rc;
    if (n_hufftabs < 1) return *why = "a table count < 1", SAGEN_ERR_SHAPE;
    if (n_hufftabs > 65536) return *why = "more than 65536 tables", SAGEN_ERR_UNSUPPORTED;
    g.all_real = 1;
    return SAGEN_OK;
}

inline int jpeg_transcode_args_check(JpegGeom& d, JpegEncGeom& g, const void* bytes, long long total_bytes, const void* frames, int n, const void* segments,
                                     int n_segments, const void* hufftabs, int n_hufftabs, int w, int h, int ncomp, int hs, int vs, int restart_interval,
                                     const void* out, long long stride, const void* sizes, const void* status, const void* scratch, size_t scratch_bytes,
                                     const char** why) {
    const int rc = jpeg_transcode_geom_fill(d, g, n, w, h, ncomp, hs, vs, restart_interval, stride, n_hufftabs, why);
    if (rc != SAGEN_OK) return rc;
    if (!bytes || !frames || !segments || !hufftabs || !out || !sizes || !status || !scratch) return *why = "null argument", SAGEN_ERR_NULL;
    if (total_bytes < 0 || total_bytes % 4) return *why = "total_bytes negative or not a multiple of 4", SAGEN_ERR_SHAPE;
    if (total_bytes > 0x7fffffffLL) return *why = "more than 2^31 - 1 bytes in one call", SAGEN_ERR_UNSUPPORTED;
    if (n_segments < n) return *why = "n_segments < n", SAGEN_ERR_SHAPE;
    if ((uintptr_t)bytes % 4 || (uintptr_t)frames % 8 || (uintptr_t)segments % 4 || (uintptr_t)out % 4 || (uintptr_t)sizes % 4 || (uintptr_t)status % 4 ||
        (uintptr_t)scratch % 16)
        return *why = "bytes / frames / segments / out / sizes / status / scratch must be aligned to 4 / 8 / 4 / 4 / 4 / 4 / 16 bytes", SAGEN_ERR_SHAPE;
    if (scratch_bytes < jpeg_transcode_scratch_layout(d, g, n_hufftabs).total) return *why = "transcode scratch too small", SAGEN_ERR_WORKSPACE;
    return SAGEN_OK;
}

constexpr int JPEG_TRANSCODE_QTABS = 0x7fffffff;   // no quantisation table is read: any non-negative index of a descriptor passes the check

// sagen_jpeg_transcode on host pointers, after jpeg_transcode_args_check
inline void jpeg_transcode_host(const uint8_t* bytes, long long total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                                const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& d, const JpegEncGeom& g, uint8_t* out, int32_t* sizes,
                                int32_t* status, void* scratch) {
    const JpegTranscodeScratch lay = jpeg_transcode_scratch_layout(d, g, n_hufftabs);
    const JpegScratch dl = jpeg_scratch_layout(d, n_hufftabs);
    JpegHuff* huff = (JpegHuff*)((char*)scratch + dl.huff);
    int16_t* nat = (int16_t*)((char*)scratch + dl.coef);
    int16_t* zz = (int16_t*)((char*)scratch + lay.enc + jpeg_enc_scratch_layout(g).coef);
    int32_t* enc_status = (int32_t*)((char*)scratch + lay.enc_status);
    const size_t total = (size_t)d.n * d.blocks * 64;
    for (size_t i = 0; i < total; ++i) nat[i] = 0;
    for (int t = 0; t < n_hufftabs; ++t) jpeg_huff_build(hufftabs + (size_t)t * JPEG_HUFF_SPEC, huff[t]);
    for (int f = 0; f < d.n; ++f)
        status[f] = (int32_t)jpeg_check_frame(frames[f], f, segments, n_segments, total_bytes, JPEG_TRANSCODE_QTABS, n_hufftabs, d, huff);
    for (int s = 0; s < n_segments; ++s) {
        const int f = segments[2 * (size_t)s];
        if (f < 0 || f >= d.n || (status[f] & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE))) continue;
        const long long k = (long long)s - frames[f].first_segment;
        if (k < 0 || k >= frames[f].n_segments) continue;
        status[f] |= (int32_t)jpeg_decode_segment(bytes, frames[f], segments, (int)k, d, huff, nat + (size_t)f * d.blocks * 64);
    }
    for (size_t i = 0; i < total; ++i) zz[i] = nat[(i & ~(size_t)63) + jpeg_natural((int)(i & 63))];
    jpeg_encode_host(nullptr, g, nullptr, out, sizes, enc_status, zz);
    for (int f = 0; f < d.n; ++f) status[f] |= enc_status[f] << 8;
}

}  // namespace sagen
