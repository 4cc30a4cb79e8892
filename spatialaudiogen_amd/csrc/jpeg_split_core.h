// Entropy decode of a scan WITHOUT restart markers on many lanes (include/sagen.h: sagen_jpeg_decode_split): every restart segment - the
// whole scan where there is no interval - is cut into chunks of chunk_bytes bytes, one lane per chunk, and the lanes find their own entry
// states by self-synchronisation of the Huffman stream (Klein & Wiseman 2003; Weissenberger & Schmidt 2018).  The same code runs on the
// device (jpeg_split.hip) and on the host (jpeg_split_decode_host below: the CPU twin and tools/jpeg_split_mutate.cpp).
//
// A decoder's STATE at a symbol boundary (a symbol is a code and its extra bits) is (position of the next bit, block j inside the MCU,
// zigzag index i; i = 0: a DC code comes next); equal states have equal futures.  The POSITION is canonical in the STUFFED stream:
// 8 x (index in `bytes` of the data byte that holds the next bit) + (bit inside it, 0 the top one), where an FF data byte is named by
// the index of its stuffed 00 (a 00 behind an FF is always stuffing and never a data byte, so the index is unique; and a scan that ends
// in FF 00 cut between the two still has a symbol boundary at or behind the cut).  jpeg_split_position finds it by stepping back from
// the window's read position over the data bytes the window still holds, and jpeg_split_open opens a window on it.
//
// Stages (a launch each on the device; the order comes from the launch boundaries alone, no lane waits on another):
//   plan      chunks per segment = max(1, ceil(bytes / chunk_bytes)) from the CHECKED descriptors, their exclusive prefix sum, chunk ->
//             segment by search in it; a segment whose chunks end behind max_chunks marks its frame CAPACITY
//   rounds    round 0: chunk 0 of a segment starts from the true state, every other chunk from the guess (its own first bit, j = 0,
//             i = 0); each lane decodes LENIENTLY (a non-code skips a bit, a run past coefficient 63 ends the block, a category is
//             taken as it is) to the first symbol boundary at or behind its chunk's end and records that exit and the blocks it
//             finished.  Round r >= 1: a chunk whose predecessor's exit of round r - 1 differs from the entry it last used decodes
//             again from that exit (exits are double-buffered: a round reads what the round before wrote, nothing of its own).
//             A marker, or the segment's end, inside a pass is an INVALID exit, not an error.  After round r the chunks 0 .. r of
//             every segment are exact, whatever the stream
//   place     a chunk is settled when the entry it last used is its predecessor's final exit; a frame with an unsettled chunk is
//             UNSETTLED, one with an invalid entry ANOMALY.  The exclusive prefix sum of the finished blocks gives each chunk's first
//             block, which must agree with its entry's j
//   write     one lane per chunk of a frame still unmarked decodes STRICTLY - the checks of jpeg_decode_segment - from its entry, stores
//             the non-zero AC coefficients and the DC DIFFERENCE, and stops at its recorded exit (the last chunk: at the segment's
//             block count, followed by jpeg_decode_segment's trailing check; chunk 0: behind the restart-marker check).  Any status
//             bit, an exit or a block count other than the recorded one marks the frame ANOMALY
//   dc        inclusive prefix sum of the differences per segment and component in scan order; a sum outside 16 bits: ANOMALY
//   redo      every marked frame is zeroed again and decoded by jpeg_decode_segment, one lane per segment: its coefficients and its
//             status come from there.  So out and status are the one-lane path's BY CONSTRUCTION: an unmarked frame's chunks decoded
//             without a status bit, each from where the one before stopped, to the segment's block count and a clean end - which is
//             the one-lane decode with status 0 - and every other frame IS the one-lane decode.
//
// Hostile input: a pass consumes at least one bit per step and ends within 8 chunk_bytes + 32 bits behind its entry (a symbol is at
// most 16 code bits and 16 extra bits; an entry lies less than a symbol behind the chunk's start); the strict pass is bounded by the
// segment's block count x 64 steps as well; the bit window never loads a word outside its segment, the step back reads bytes the
// window has read; every table index is a checked one; block indices are compared with the segment's count before they are used.
#pragma once
#include "jpeg_core.h"

namespace sagen {

constexpr int JPEG_SPLIT_TILE = 256;                          // chunks, segments and DC terms are scanned in tiles of 256
constexpr uint64_t JPEG_SPLIT_INVALID = 1ull << 62;           // an exit nobody can continue from / an entry nobody can start from
constexpr uint64_t JPEG_SPLIT_FIXED = 1ull << 63;             // (entries only) chunk 0 of a segment, or an unused slot: never re-entered

struct JpegSplitScratch {
    JpegScratch base;
    size_t fpath, seg_first, seg_tiles, chunk_seg, entry, exit0, exit1, nblk, blk_local, blk_tiles, dc_local, dc_tiles, total;
    long long n_seg_tiles, n_blk_tiles;
    int dc_tiles_per_comp;
};

inline size_t jpeg_split_align(size_t x) { return (x + 15) / 16 * 16; }

inline JpegSplitScratch jpeg_split_scratch_layout(const JpegGeom& g, int n_hufftabs, int n_segments, long long max_chunks) {
    JpegSplitScratch s;
    s.base = jpeg_scratch_layout(g, n_hufftabs);
    s.n_seg_tiles = ((long long)n_segments + JPEG_SPLIT_TILE - 1) / JPEG_SPLIT_TILE;
    s.n_blk_tiles = (max_chunks + JPEG_SPLIT_TILE - 1) / JPEG_SPLIT_TILE;
    s.dc_tiles_per_comp = (g.mcus * (g.ncomp == 1 ? 1 : g.hs * g.vs) + JPEG_SPLIT_TILE - 1) / JPEG_SPLIT_TILE;
    size_t at = jpeg_split_align(s.base.total);
    s.fpath = at, at = jpeg_split_align(at + (size_t)g.n * 2 * 4);           // [2][n]: the marks of plan and place; of write and dc
    s.seg_first = at, at = jpeg_split_align(at + ((size_t)n_segments + 1) * 8);
    s.seg_tiles = at, at = jpeg_split_align(at + ((size_t)s.n_seg_tiles + 1) * 8);
    s.chunk_seg = at, at = jpeg_split_align(at + (size_t)max_chunks * 4);
    s.entry = at, at = jpeg_split_align(at + (size_t)max_chunks * 8);
    s.exit0 = at, at = jpeg_split_align(at + (size_t)max_chunks * 8);
    s.exit1 = at, at = jpeg_split_align(at + (size_t)max_chunks * 8);
    s.nblk = at, at = jpeg_split_align(at + (size_t)max_chunks * 4);
    s.blk_local = at, at = jpeg_split_align(at + (size_t)max_chunks * 4);
    s.blk_tiles = at, at = jpeg_split_align(at + ((size_t)s.n_blk_tiles + 1) * 8);
    s.dc_local = at, at = jpeg_split_align(at + (size_t)g.n * g.blocks * 4);
    s.dc_tiles = at, at = jpeg_split_align(at + (size_t)g.n * 3 * s.dc_tiles_per_comp * 4);
    s.total = at;
    return s;
}

// the checks of sagen_jpeg_decode_split beyond jpeg_args_check's (which has filled g)
inline int jpeg_split_args_check(const JpegGeom& g, int n_hufftabs, int n_segments, int chunk_bytes, int rounds, long long max_chunks, const void* path,
                                 size_t scratch_bytes, const char** why) {
    if (chunk_bytes < 16 || chunk_bytes > 65536 || chunk_bytes % 4) return *why = "chunk_bytes is no multiple of 4 in [16, 65536]", SAGEN_ERR_SHAPE;
    if (rounds < 1 || rounds > 64) return *why = "rounds outside [1, 64]", SAGEN_ERR_SHAPE;
    if (max_chunks < n_segments || max_chunks > 0x7fffffffLL) return *why = "max_chunks outside [n_segments, 2^31 - 1]", SAGEN_ERR_SHAPE;
    if ((uintptr_t)path % 4) return *why = "path must be aligned to 4 bytes", SAGEN_ERR_SHAPE;
    if (scratch_bytes < jpeg_split_scratch_layout(g, n_hufftabs, n_segments, max_chunks).total) return *why = "scratch too small for the split decode", SAGEN_ERR_WORKSPACE;
    return SAGEN_OK;
}

JPEG_FN uint64_t jpeg_split_state(uint64_t bitpos, int j, int i) { return bitpos << 9 | (uint64_t)j << 6 | (uint64_t)i; }

// Row s of `segments` as the one-lane path sees it (jpeg_entropy_kernel's checks): false for a row nobody decodes
JPEG_FN bool jpeg_split_segment(const sagen_jpeg_frame* frames, const int32_t* segments, long long s, const JpegGeom& g, const int32_t* status,
                                int& f, int& k, uint32_t& start, uint32_t& end) {
    f = segments[2 * s];
    if (f < 0 || f >= g.n || (status[f] & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE))) return false;
    const sagen_jpeg_frame& fr = frames[f];
    const long long kk = s - fr.first_segment;
    if (kk < 0 || kk >= fr.n_segments) return false;
    k = (int)kk;
    const int32_t* rows = segments + 2 * (size_t)fr.first_segment;
    start = (uint32_t)(fr.scan_offset + rows[2 * k + 1]);                                 // as jpeg_decode_segment
    end = (uint32_t)(fr.scan_offset + (k + 1 < fr.n_segments ? rows[2 * k + 3] - 2 : fr.scan_bytes));
    return true;
}

JPEG_FN long long jpeg_split_chunks_of(uint32_t start, uint32_t end, int chunk_bytes) {
    const long long len = (long long)end - (long long)start;                               // >= 0 behind jpeg_check_frame
    return len <= 0 ? 1 : (len + chunk_bytes - 1) / chunk_bytes;
}

// the last s in [0, n) with first[s] <= c (first: non-decreasing, first[0] = 0 <= c < first[n])
JPEG_FN long long jpeg_split_search(const int64_t* first, long long n, long long c) {
    long long lo = 0, hi = n;                                                             // first[lo] <= c < first[hi]
    while (hi - lo > 1) {
        const long long mid = lo + (hi - lo) / 2;
        if (first[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// the MCUs and blocks of segment k of a frame
JPEG_FN void jpeg_split_segment_blocks(const sagen_jpeg_frame& fr, int k, const JpegGeom& g, int& m0, int& seg_blocks) {
    const int ri = fr.restart_interval;
    m0 = ri ? k * ri : 0;
    const int m1 = ri && m0 + ri < g.mcus ? m0 + ri : g.mcus;
    seg_blocks = (m1 - m0) * g.bpm;
}

// Position of the next bit of a window with status 0 that has consumed no fake bit; start / end: the segment's.  The data byte that
// holds the bit is found by stepping back over the data bytes the window holds; an FF data byte is named by its stuffed 00.
JPEG_FN uint64_t jpeg_split_position(const JpegBits& b, const uint8_t* bytes, uint32_t start, uint32_t end) {
    const int real = b.nbits - b.fake;
    uint32_t p = b.pos;
    for (int k = (real + 7) >> 3; k > 0; --k) {
        --p;
        if (bytes[p] == 0 && p > start && bytes[p - 1] == 0xFF) --p;                      // a stuffed 00: the data byte is the FF in front of it
    }
    if (p + 1 < end && bytes[p] == 0xFF && bytes[p + 1] == 0) ++p;
    return (uint64_t)p * 8 + (uint64_t)((8 - (real & 7)) & 7);
}

JPEG_FN void jpeg_split_open(JpegBits& b, const uint8_t* bytes, uint64_t bitpos, uint32_t start, uint32_t end) {
    uint32_t p = (uint32_t)(bitpos >> 3);
    if (p > start && p < end && bytes[p] == 0 && bytes[p - 1] == 0xFF) --p;              // the stuffed 00 names its FF
    jpeg_bits_open(b, bytes, p, end);
    const int skip = (int)(bitpos & 7);
    if (skip) {
        jpeg_fill(b);
        jpeg_skip(b, skip);
    }
}

// the guess of chunk ci > 0: the first bit of the data byte its first byte names
JPEG_FN uint64_t jpeg_split_guess(uint32_t at) { return jpeg_split_state((uint64_t)at * 8, 0, 0); }

// One lenient pass from `entry` to the first symbol boundary at or behind chunk_end: the exit state, or JPEG_SPLIT_INVALID where a
// marker or the segment's end came first; nblk: the blocks finished on the way.
JPEG_FN uint64_t jpeg_split_sync(const uint8_t* bytes, const sagen_jpeg_frame& fr, const JpegGeom& g, const JpegHuff* huff, uint32_t start,
                                 uint32_t end, uint32_t chunk_end, uint64_t entry, int& nblk) {
    JpegBits b;
    jpeg_split_open(b, bytes, entry >> 9, start, end);
    int j = (int)(entry >> 6) & 7, i = (int)entry & 63;
    nblk = 0;
    for (;;) {
        if (b.st || b.nbits < b.fake) return JPEG_SPLIT_INVALID;
        if (b.pos + 1 >= chunk_end) {                            // (the position's byte is at most the one the window reads next, + 1)
            const uint64_t at = jpeg_split_position(b, bytes, start, end);
            if (at >= (uint64_t)chunk_end * 8) return jpeg_split_state(at, j, i);
        }
        const int c = jpeg_block_component(g, j);
        const int v = jpeg_decode_symbol(b, huff[i == 0 ? fr.dctab[c] : fr.actab[c]]);
        if (v < 0) {                                             // no code: skip a bit (>= 25 are in the window behind the failed look)
            b.st &= ~(uint32_t)SAGEN_JPEG_ST_CODE;
            jpeg_skip(b, 1);
            continue;
        }
        if (i == 0) {
            const int s = v > 16 ? 16 : v;
            if (s) jpeg_get_bits(b, s);
            i = 1;
            continue;
        }
        const int r = v >> 4, s = v & 15;
        if (s == 0) {
            i = r == 15 ? i + 16 : 64;
        } else {
            i += r + 1;
            jpeg_get_bits(b, s);
        }
        if (i >= 64) {
            i = 0, j = j + 1 == g.bpm ? 0 : j + 1;
            ++nblk;
        }
    }
}

// The strict pass of one chunk of a settled frame, from its true entry; coef: the segment's first block.  first_block: the chunk's first
// block inside the segment (< = seg_blocks, first_block % bpm == the entry's j).  Returns 0 or SAGEN_JPEG_PATH_ANOMALY.
JPEG_FN int32_t jpeg_split_write(const uint8_t* bytes, const sagen_jpeg_frame& fr, const JpegGeom& g, const JpegHuff* huff, uint32_t start, uint32_t end,
                                 uint32_t chunk_end, bool last, uint64_t entry, uint64_t want_exit, int want_nblk, int first_block, int seg_blocks,
                                 int16_t* coef) {
    JpegBits b;
    jpeg_split_open(b, bytes, entry >> 9, start, end);
    int j = (int)(entry >> 6) & 7, i = (int)entry & 63;
    int at_block = first_block, nblk = 0;
    for (;;) {
        if (!last) {
            if (b.st || b.nbits < b.fake) return SAGEN_JPEG_PATH_ANOMALY;
            if (b.pos + 1 >= chunk_end && jpeg_split_position(b, bytes, start, end) >= (uint64_t)chunk_end * 8) break;
        }
        if (at_block >= seg_blocks) break;
        const int c = jpeg_block_component(g, j);
        int16_t* blk = coef + (size_t)at_block * 64;
        if (i == 0) {
            const int t = jpeg_decode_symbol(b, huff[fr.dctab[c]]);
            if (t < 0 || t > 11) return SAGEN_JPEG_PATH_ANOMALY;
            if (t) blk[0] = (int16_t)jpeg_extend(jpeg_get_bits(b, t), t);                  // the DIFFERENCE; the dc stage sums
            i = 1;
            continue;
        }
        const int rs = jpeg_decode_symbol(b, huff[fr.actab[c]]);
        if (rs < 0) return SAGEN_JPEG_PATH_ANOMALY;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r != 15) {
                i = 64;                                          // EOB
            } else {
                i += 16;                                         // ZRL
                if (i > 64) return SAGEN_JPEG_PATH_ANOMALY;
            }
        } else {
            i += r;
            if (i > 63 || s > 10) return SAGEN_JPEG_PATH_ANOMALY;
            blk[jpeg_natural(i)] = (int16_t)jpeg_extend(jpeg_get_bits(b, s), s);
            ++i;
        }
        if (i == 64) {
            if (b.nbits < b.fake || b.st) return SAGEN_JPEG_PATH_ANOMALY;
            i = 0, j = j + 1 == g.bpm ? 0 : j + 1;
            ++at_block, ++nblk;
        }
    }
    if (b.st || b.nbits < b.fake) return SAGEN_JPEG_PATH_ANOMALY;
    if (!last) return jpeg_split_state(jpeg_split_position(b, bytes, start, end), j, i) == want_exit && nblk == want_nblk ? 0 : SAGEN_JPEG_PATH_ANOMALY;
    if (at_block != seg_blocks || i != 0) return SAGEN_JPEG_PATH_ANOMALY;
    return b.pos < b.end || b.nbits - b.fake >= 8 ? SAGEN_JPEG_PATH_ANOMALY : 0;          // jpeg_decode_segment's TRAILING
}

// what a lane knows of its chunk
struct JpegSplitChunk {
    int f, k, m0, seg_blocks;
    uint32_t start, end, chunk_start, chunk_end;
    long long c0, ci, nci;                                       // the segment's first chunk, this one's number in it, the segment's count
};

JPEG_FN bool jpeg_split_chunk(const sagen_jpeg_frame* frames, const int32_t* segments, const JpegGeom& g, const int32_t* status, const int64_t* seg_first,
                              long long s, long long c, int chunk_bytes, JpegSplitChunk& k) {
    if (!jpeg_split_segment(frames, segments, s, g, status, k.f, k.k, k.start, k.end)) return false;
    k.c0 = seg_first[s], k.nci = seg_first[s + 1] - k.c0, k.ci = c - k.c0;
    k.chunk_start = k.start + (uint32_t)(k.ci * chunk_bytes);
    k.chunk_end = k.ci + 1 < k.nci ? k.chunk_start + (uint32_t)chunk_bytes : k.end;
    jpeg_split_segment_blocks(frames[k.f], k.k, g, k.m0, k.seg_blocks);
    return true;
}

// round 0 of chunk c (s: its segment row, or -1 for a slot nobody uses)
JPEG_FN void jpeg_split_round0(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, const JpegGeom& g, const JpegHuff* huff,
                               const int32_t* status, const int64_t* seg_first, long long s, long long c, int chunk_bytes, uint64_t* entry,
                               uint64_t* exit, int32_t* nblk) {
    JpegSplitChunk k;
    if (s < 0 || !jpeg_split_chunk(frames, segments, g, status, seg_first, s, c, chunk_bytes, k)) {
        entry[c] = JPEG_SPLIT_FIXED | JPEG_SPLIT_INVALID, exit[c] = JPEG_SPLIT_INVALID, nblk[c] = 0;
        return;
    }
    const uint64_t e = k.ci == 0 ? jpeg_split_state((uint64_t)k.start * 8, 0, 0) : jpeg_split_guess(k.chunk_start);
    int nb;
    exit[c] = jpeg_split_sync(bytes, frames[k.f], g, huff, k.start, k.end, k.chunk_end, e, nb);
    entry[c] = k.ci == 0 ? e | JPEG_SPLIT_FIXED : e;
    nblk[c] = nb;
}

// round r >= 1 of chunk c: exit_in is what round r - 1 wrote, exit_out what this round writes
JPEG_FN void jpeg_split_round(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, const JpegGeom& g, const JpegHuff* huff,
                              const int32_t* status, const int64_t* seg_first, const int32_t* chunk_seg, long long c, int chunk_bytes, uint64_t* entry,
                              const uint64_t* exit_in, uint64_t* exit_out, int32_t* nblk) {
    const uint64_t e = entry[c];
    const uint64_t p = e & JPEG_SPLIT_FIXED ? e : exit_in[c - 1];                          // (chunk 0 of the call is FIXED)
    if (p == e) {
        exit_out[c] = exit_in[c];
        return;
    }
    entry[c] = p;
    JpegSplitChunk k;
    if (p == JPEG_SPLIT_INVALID || !jpeg_split_chunk(frames, segments, g, status, seg_first, chunk_seg[c], c, chunk_bytes, k)) {
        exit_out[c] = JPEG_SPLIT_INVALID, nblk[c] = 0;
        return;
    }
    int nb;
    exit_out[c] = jpeg_split_sync(bytes, frames[k.f], g, huff, k.start, k.end, k.chunk_end, p, nb);
    nblk[c] = nb;
}

// 0, UNSETTLED or ANOMALY for chunk c after the last round (exit: the final exits)
JPEG_FN int32_t jpeg_split_settled(const uint64_t* entry, const uint64_t* exit, long long c) {
    const uint64_t e = entry[c];
    if (e & JPEG_SPLIT_FIXED) return 0;
    if (e != exit[c - 1]) return SAGEN_JPEG_PATH_UNSETTLED;
    return e == JPEG_SPLIT_INVALID ? SAGEN_JPEG_PATH_ANOMALY : 0;
}

// the strict pass of chunk c of segment row s; blk_first: the exclusive prefix sum of nblk over all chunks at c and at the segment's first
JPEG_FN int32_t jpeg_split_write_chunk(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, const JpegGeom& g,
                                       const JpegHuff* huff, const int32_t* status, const int64_t* seg_first, long long s, long long c, int chunk_bytes,
                                       const uint64_t* entry, const uint64_t* exit, const int32_t* nblk, long long blk_at_c, long long blk_at_c0,
                                       int16_t* coef, int& f) {
    JpegSplitChunk k;
    f = -1;
    if (!jpeg_split_chunk(frames, segments, g, status, seg_first, s, c, chunk_bytes, k)) return 0;
    f = k.f;
    const uint64_t e = entry[c] & ~JPEG_SPLIT_FIXED;
    const long long first = blk_at_c - blk_at_c0;
    if (e & JPEG_SPLIT_INVALID || first < 0 || first > k.seg_blocks || (int)(first % g.bpm) != ((int)(e >> 6) & 7)) return SAGEN_JPEG_PATH_ANOMALY;
    if (k.ci == 0 && k.k > 0 && (bytes[k.start - 2] != 0xFF || bytes[k.start - 1] != 0xD0 + ((k.k - 1) & 7))) return SAGEN_JPEG_PATH_ANOMALY;
    return jpeg_split_write(bytes, frames[k.f], g, huff, k.start, k.end, k.chunk_end, k.ci + 1 == k.nci, e, exit[c], nblk[c], (int)first, k.seg_blocks,
                            coef + ((size_t)k.f * g.blocks + (size_t)k.m0 * g.bpm) * 64);
}

// ---- the DC terms of a component in scan order ------------------------------------------------------------------------------------------
JPEG_FN int jpeg_split_dc_per_mcu(const JpegGeom& g, int comp) { return comp == 0 && g.ncomp == 3 ? g.hs * g.vs : 1; }
// term t of component comp -> its block inside the frame
JPEG_FN int jpeg_split_dc_block(const JpegGeom& g, int comp, int t) {
    const int per = jpeg_split_dc_per_mcu(g, comp);
    return (t / per) * g.bpm + (comp == 0 ? t % per : g.hs * g.vs + comp - 1);
}
// ... -> the first term of its restart segment
JPEG_FN int jpeg_split_dc_base(const JpegGeom& g, int comp, int t, int restart_interval) {
    const int per = jpeg_split_dc_per_mcu(g, comp);
    return restart_interval ? (t / per) / restart_interval * restart_interval * per : 0;
}
// the terms of a component in front of component comp inside dc_local's frame row
JPEG_FN int jpeg_split_dc_offset(const JpegGeom& g, int comp) { return comp == 0 ? 0 : g.mcus * g.hs * g.vs + (comp - 1) * g.mcus; }

JPEG_FN int32_t jpeg_split_path_value(int32_t bits) {             // the first cause, in the order of the stages
    return bits & SAGEN_JPEG_PATH_CAPACITY ? SAGEN_JPEG_PATH_CAPACITY : (bits & SAGEN_JPEG_PATH_UNSETTLED ? SAGEN_JPEG_PATH_UNSETTLED : (bits ? SAGEN_JPEG_PATH_ANOMALY : 0));
}

// ---- the whole call as plain loops on host pointers: the stages of jpeg_split.hip in their order -------------------------------------
inline void jpeg_split_decode_host(const uint8_t* bytes, long long total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                                   const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out,
                                   int32_t* status, void* scratch, int chunk_bytes, int rounds, long long max_chunks, int32_t* path) {
    const JpegSplitScratch lay = jpeg_split_scratch_layout(g, n_hufftabs, n_segments, max_chunks);
    char* sc = (char*)scratch;
    JpegHuff* huff = (JpegHuff*)(sc + lay.base.huff);
    int16_t* coef = (int16_t*)(sc + lay.base.coef);
    uint8_t* planes = (uint8_t*)sc + lay.base.planes;
    int32_t* fpath = (int32_t*)(sc + lay.fpath);
    int64_t* seg_first = (int64_t*)(sc + lay.seg_first);
    int32_t* chunk_seg = (int32_t*)(sc + lay.chunk_seg);
    uint64_t* entry = (uint64_t*)(sc + lay.entry);
    uint64_t* exits[2] = {(uint64_t*)(sc + lay.exit0), (uint64_t*)(sc + lay.exit1)};
    int32_t* nblk = (int32_t*)(sc + lay.nblk);
    jpeg_front_host(total_bytes, frames, segments, n_segments, n_qtabs, hufftabs, n_hufftabs, g, huff, coef, status);
    for (int f = 0; f < g.n; ++f) fpath[f] = 0;
    // plan
    long long total = 0;
    for (long long s = 0; s < n_segments; ++s) {
        int f, k;
        uint32_t start, end;
        seg_first[s] = total;
        if (!jpeg_split_segment(frames, segments, s, g, status, f, k, start, end)) continue;
        total += jpeg_split_chunks_of(start, end, chunk_bytes);
        if (total > max_chunks) fpath[f] |= SAGEN_JPEG_PATH_CAPACITY;
    }
    seg_first[n_segments] = total;
    for (long long c = 0; c < max_chunks; ++c) {
        long long s = -1;
        if (c < total) {
            s = jpeg_split_search(seg_first, n_segments, c);
            const int f = segments[2 * s];
            if (fpath[f]) s = -1;
        }
        chunk_seg[c] = (int32_t)s;
        jpeg_split_round0(bytes, frames, segments, g, huff, status, seg_first, s, c, chunk_bytes, entry, exits[0], nblk);
    }
    for (int r = 1; r < rounds; ++r)
        for (long long c = 0; c < max_chunks; ++c)
            jpeg_split_round(bytes, frames, segments, g, huff, status, seg_first, chunk_seg, c, chunk_bytes, entry, exits[(r - 1) & 1], exits[r & 1], nblk);
    const uint64_t* fin = exits[(rounds - 1) & 1];
    // place
    int32_t* blk_local = (int32_t*)(sc + lay.blk_local);
    int64_t* blk_tiles = (int64_t*)(sc + lay.blk_tiles);
    long long run = 0;
    for (long long c = 0; c < max_chunks; ++c) {
        if (c % JPEG_SPLIT_TILE == 0) blk_tiles[c / JPEG_SPLIT_TILE] = run;
        blk_local[c] = (int32_t)(run - blk_tiles[c / JPEG_SPLIT_TILE]);
        if (chunk_seg[c] < 0) continue;
        const int32_t mark = jpeg_split_settled(entry, fin, c);
        if (mark) fpath[segments[2 * (size_t)chunk_seg[c]]] |= mark;
        run += nblk[c];
    }
    // write: the frames no stage above has marked (the marks of this stage are not read by it)
    int32_t* late = fpath + g.n;
    for (int f = 0; f < g.n; ++f) late[f] = 0;
    for (long long c = 0; c < max_chunks; ++c) {
        const long long s = chunk_seg[c];
        if (s < 0 || fpath[segments[2 * s]]) continue;
        const long long c0 = seg_first[s];
        int f;
        const int32_t mark = jpeg_split_write_chunk(bytes, frames, segments, g, huff, status, seg_first, s, c, chunk_bytes, entry, fin, nblk,
                                                    blk_tiles[c / JPEG_SPLIT_TILE] + blk_local[c], blk_tiles[c0 / JPEG_SPLIT_TILE] + blk_local[c0], coef, f);
        if (mark && f >= 0) late[f] |= mark;
    }
    // dc: every frame (a marked one is zeroed and decoded again below)
    for (int f = 0; f < g.n; ++f) {
        if (status[f] & SAGEN_JPEG_ST_DESC) continue;             // (nothing of it was decoded: all zero)
        for (int comp = 0; comp < g.ncomp; ++comp) {
            const int terms = g.mcus * jpeg_split_dc_per_mcu(g, comp);
            uint32_t sum = 0;
            for (int t = 0; t < terms; ++t) {
                if (t == jpeg_split_dc_base(g, comp, t, frames[f].restart_interval)) sum = 0;
                int16_t* blk = coef + ((size_t)f * g.blocks + jpeg_split_dc_block(g, comp, t)) * 64;
                sum += (uint32_t)(int32_t)blk[0];
                const int32_t p = (int32_t)sum;
                if (p < -32768 || p > 32767) late[f] |= SAGEN_JPEG_PATH_ANOMALY;
                blk[0] = (int16_t)p;
            }
        }
    }
    // redo
    for (int f = 0; f < g.n; ++f) {
        fpath[f] = jpeg_split_path_value(fpath[f] | late[f]);
        if (path) path[f] = fpath[f];
        if (!fpath[f]) continue;
        int16_t* fc = coef + (size_t)f * g.blocks * 64;
        for (size_t i = 0; i < (size_t)g.blocks * 64; ++i) fc[i] = 0;
    }
    jpeg_entropy_host(bytes, frames, segments, n_segments, g, huff, coef, status, fpath);
    jpeg_back_host(frames, qtabs, g, coef, status, planes, out);
}

}  // namespace sagen
