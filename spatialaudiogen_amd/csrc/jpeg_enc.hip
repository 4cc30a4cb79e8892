// Baseline JPEG encode on the device (gfx950): [n][h][w][3] uint8 RGB in, the entropy-coded data of each frame out -
// include/sagen.h: sagen_jpeg_encode; the arithmetic is csrc/jpeg_enc_core.h, shared with the CPU twin.  It replaces the host encode
// (PIL / libjpeg, one thread) behind project and flow.  Unlike the decoder no stage walks a frame: an encoder knows every block's
// bit count before it writes a bit, so two prefix sums place the bits and the stuffed bytes.
//
//   jpeg_enc_init_kernel        the quantisation tables checked once (an entry outside 1..255: every frame RANGE, no block is made)
//   jpeg_enc_dct_kernel         one thread per block that holds image samples: colour conversion, edge replication and chroma
//                               downsampling straight from the frame, the islow forward DCT and the quantisation with the block in
//                               statically indexed registers, 64 int16 in zigzag order as eight 16-byte stores
//   jpeg_enc_bits_kernel<0>     one WAVE per block, lane k holds coefficient k: a ballot of the non-zero lanes gives each its run, each
//                               lane forms its own codes (at most 59 bits), a wave prefix sum gives the block's bit count
//   jpeg_enc_scan_tiles_kernel  exclusive prefix sum over each tile of 256 blocks, and the tile's sum
//   jpeg_enc_scan_sums_kernel   one workgroup per frame over the tile sums (1/256 of the blocks): each tile's first bit, the frame's bits
//   jpeg_enc_seg_kernel         (restart intervals only) one workgroup per frame over its segments: each segment starts on a byte, so
//                               the fill bits of the segments in front move its blocks; the segment's first unstuffed byte
//   jpeg_enc_bits_kernel<1>     the same wave again, now with its position: the lanes OR their bits into the block's words in LDS,
//                               then whole words go out as plain stores and the (at most two) words shared with the neighbouring
//                               blocks by integer atomicOr on the zeroed stream - OR commutes, the result does not depend on the order;
//                               the wave of the last block, and of each restart segment's last block, adds the fill bits
//   jpeg_enc_ff_kernel<0>       per tile of 4096 unstuffed bytes: the FF bytes in it
//   jpeg_enc_ff_sums_kernel     one workgroup per frame over the tile counts: FFs in front of each tile, sizes[f], CAPACITY
//   jpeg_enc_ff_kernel<1>       one thread per 16 unstuffed bytes: each byte, and its 00, to out where that lies below stride; the thread
//                               that holds a restart segment's first byte puts the (unstuffed) marker in front of it
// No workgroup waits on another: the order comes from the launch boundaries alone.
//
// sagen_jpeg_transcode (run_jpeg_transcode below) re-segments existing files without computing a pixel: the decoder's tables, check and
// entropy stages (jpeg.hip: jpeg_coefficients_launch) fill natural-order coefficients, jpeg_enc_reorder_kernel puts them into zigzag
// order where the stages above from jpeg_enc_bits_kernel<0> on expect them, and jpeg_enc_status_merge_kernel joins the two status words.
//
// tools/jpeg_encode_rate.py measures the stages; DESIGN.md says what they cost.
#include "kernels.h"
#include "jpeg_enc_core.h"
#include "group_scan.h"

namespace sagen {

namespace {

constexpr int ENC_THREADS = 256;
constexpr int ENC_WAVES = SCAN_WAVES;               // (group_scan.h: the scans are over workgroups of ENC_THREADS)
constexpr int ENC_WORDS = 56;                      // (31 + 1660 + 7 fill bits) / 32: 54 words; the last lane starts in word 52 at most and reaches two further

__constant__ JpegEncHuff c_enc_huff = jpeg_enc_huff_make();

__global__ __launch_bounds__(64) void jpeg_enc_init_kernel(const uint16_t* __restrict__ qtabs, const JpegEncGeom g, int32_t* __restrict__ qok,
                                                           int32_t* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    const bool ok = jpeg_enc_qtabs_ok(qtabs, g.ncomp);
    if (f == 0) *qok = ok ? 1 : 0;
    if (f < g.n) status[f] = ok ? 0 : SAGEN_JPEG_ENC_ST_RANGE;
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_dct_kernel(const uint8_t* __restrict__ frames, const uint16_t* __restrict__ qtabs,
                                                                   const JpegEncGeom g, const int32_t* __restrict__ qok,
                                                                   int16_t* __restrict__ coef) {
    const long long id = (long long)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (id >= (long long)g.n * g.blocks || !*qok) return;
    const int f = (int)(id / g.blocks), b = (int)(id % g.blocks);
    int comp, by, bx;
    bool dummy;
    jpeg_enc_block_place(g, b, comp, by, bx, dummy);
    if (dummy) return;                                                // (never read: jpeg_enc_bits_kernel knows it from the geometry)
    int16_t zz[64];
    jpeg_enc_block(g, frames + (size_t)f * g.h * g.w * g.ncomp, qtabs, comp, by, bx, zz);
    uint4* dst = (uint4*)(coef + id * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (uint32_t)(uint16_t)zz[8 * i + 2 * j] | ((uint32_t)(uint16_t)zz[8 * i + 2 * j + 1] << 16);
        dst[i] = make_uint4(p[0], p[1], p[2], p[3]);
    }
}

// WRITE = false: counts[block] = its bits.  WRITE = true: counts[block] is its first bit inside its tile (jpeg_enc_scan_tiles_kernel),
// tile_at the tile's first bit in the frame; the bits go into the frame's (zeroed) unstuffed stream.
template <bool WRITE>
__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_bits_kernel(const int16_t* __restrict__ coef, const JpegEncGeom g,
                                                                    const int32_t* __restrict__ qok, int32_t* __restrict__ counts,
                                                                    const int64_t* __restrict__ tile_at, int scan_tiles,
                                                                    const int64_t* __restrict__ seg_pad, uint32_t* __restrict__ stream,
                                                                    int32_t* status) {
    __shared__ uint32_t words[ENC_WAVES][ENC_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long id = (long long)blockIdx.x * ENC_WAVES + wave;
    const bool inside = id < (long long)g.n * g.blocks;              // (uniform over the wave, like everything derived from id)
    const bool live = inside && *qok != 0;
    int len = 0, f = 0, b = 0;
    uint64_t bits = 0;
    bool range = false;
    if (live) {
        f = (int)(id / g.blocks), b = (int)(id % g.blocks);
        int comp, by, bx;
        bool dummy;
        jpeg_enc_block_place(g, b, comp, by, bx, dummy);
        const int tab = comp ? 1 : 0;
        const uint32_t eob = c_enc_huff.ac[tab][0];
        if (dummy) {
            if (lane == 0) len = jpeg_enc_code(c_enc_huff, tab, true, 0, 0, bits, range);
            if (lane == 63) bits = eob >> 8, len = (int)(eob & 255);
        } else {
            const int v = coef[id * 64 + lane];
            const unsigned long long nz = __ballot(lane > 0 && v != 0);
            if (lane == 0) {
                const int p = jpeg_enc_pred_block(g, b);
                const int pred = p < 0 ? 0 : coef[((long long)f * g.blocks + p) * 64];
                len = jpeg_enc_code(c_enc_huff, tab, true, 0, v - pred, bits, range);
            } else if (v != 0) {
                const unsigned long long below = nz & ((1ull << lane) - 1ull);
                const int prev = below ? 63 - __clzll((long long)below) : 0;
                len = jpeg_enc_code(c_enc_huff, tab, false, lane - prev - 1, v, bits, range);
            } else if (lane == 63) {
                bits = eob >> 8, len = (int)(eob & 255);              // the block ends in zeros: end of block
            }
        }
    }
    int pre = 0, tot = len;
    wave_scan(lane, pre, tot);
    if constexpr (!WRITE) {
        if (inside && lane == 0) counts[id] = tot;
        if (range) atomicOr(&status[f], (int32_t)SAGEN_JPEG_ENC_ST_RANGE);
    } else {
        long long pos = 0;
        int off = 0, fill = 0;
        if (live) {
            pos = tile_at[(size_t)f * scan_tiles + b / JPEG_ENC_SCAN_TILE] + counts[id];
            bool last = b == g.blocks - 1;
            if (g.nseg > 1) {                                         // the fill bits of the segments in front; a segment's last block adds its own
                pos += seg_pad[(size_t)f * g.nseg + b / g.seg_blocks];
                last = last || (b + 1) % g.seg_blocks == 0;
            }
            off = (int)(pos & 31);
            if (last && ((off + tot) & 7)) fill = 8 - ((off + tot) & 7);
        }
        if (lane < ENC_WORDS) words[wave][lane] = 0;
        __syncthreads();
        if (live && len > 0) {                                        // bit i of the block at word i / 32, bit 31 - i % 32
            const int o = off + pre, wi = o >> 5, r = o & 31;
            const uint64_t top = bits << (64 - len);
            const uint32_t hi = (uint32_t)(top >> 32), lo = (uint32_t)top;
            const uint32_t w0 = hi >> r, w1 = r ? (hi << (32 - r)) | (lo >> r) : lo, w2 = r ? lo << (32 - r) : 0u;
            if (w0) atomicOr(&words[wave][wi], w0);
            if (w1) atomicOr(&words[wave][wi + 1], w1);
            if (w2) atomicOr(&words[wave][wi + 2], w2);
        }
        if (fill && lane == 0) {                                      // the ones behind the frame's last bit, inside its byte
            const int end = off + tot;
            atomicOr(&words[wave][end >> 5], ((1u << fill) - 1u) << (32 - (end & 31) - fill));
        }
        __syncthreads();
        const int end = off + tot + fill, nwords = (end + 31) >> 5;   // <= 54
        if (live && lane < nwords) {
            const long long gw = (pos >> 5) + lane;
            if ((gw + 1) * 4 <= g.cap) {                              // (always: cap is the bound)
                uint32_t* dst = stream + (size_t)f * (size_t)(g.cap / 4) + gw;
                const uint32_t be = __builtin_bswap32(words[wave][lane]);   // memory is MSB first
                const bool shared = (lane == 0 && off) || (lane == nwords - 1 && (end & 31));
                if (!shared)
                    *dst = be;
                else if (be)
                    atomicOr(dst, be);
            }
        }
    }
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_scan_tiles_kernel(int32_t* __restrict__ counts, const JpegEncGeom g, int scan_tiles,
                                                                          int32_t* __restrict__ tiles) {
    __shared__ int lds[ENC_WAVES];
    const int f = blockIdx.y, b = blockIdx.x * JPEG_ENC_SCAN_TILE + threadIdx.x;
    const size_t at = (size_t)f * g.blocks + b;
    const int v = b < g.blocks ? counts[at] : 0;
    int total;
    const int pre = group_scan(v, lds, total);                       // <= 256 x 1660
    if (b < g.blocks) counts[at] = pre;
    if (threadIdx.x == 0) tiles[(size_t)f * scan_tiles + blockIdx.x] = total;
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_scan_sums_kernel(const int32_t* __restrict__ tiles, int scan_tiles,
                                                                         int64_t* __restrict__ tile_at, int64_t* __restrict__ frame_bits) {
    __shared__ int lds[ENC_WAVES];
    const int f = blockIdx.x;
    long long carry = 0;
    for (int t0 = 0; t0 < scan_tiles; t0 += ENC_THREADS) {
        const int t = t0 + threadIdx.x;
        const int v = t < scan_tiles ? tiles[(size_t)f * scan_tiles + t] : 0;
        int total;
        const int pre = group_scan(v, lds, total);                   // <= 256 x 256 x 1660 < 2^31
        if (t < scan_tiles) tile_at[(size_t)f * scan_tiles + t] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) frame_bits[f] = carry;
}

// Restart segments (nseg > 1 only): one workgroup per frame over its segments.  A segment's bits are the difference of two positions
// of the frame-wide scan above, its fill the 0..7 bits to its byte; the exclusive prefix sum of the fills is what every block of the
// segment adds to its position (seg_pad), and that plus the segment's own first bit its first unstuffed byte (seg_at).  frame_bits
// becomes the whole frame's, fills included: a multiple of 8.
__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_seg_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ tile_at,
                                                                   int scan_tiles, const JpegEncGeom g, int64_t* __restrict__ seg_pad,
                                                                   int64_t* __restrict__ seg_at, int64_t* __restrict__ frame_bits) {
    __shared__ int lds[ENC_WAVES];
    const int f = blockIdx.x;
    const long long all = frame_bits[f];
    long long carry = 0;
    for (int s0 = 0; s0 < g.nseg; s0 += ENC_THREADS) {
        const int s = s0 + threadIdx.x;
        long long first = 0;
        int pad = 0;
        if (s < g.nseg) {
            const long long b0 = (long long)s * g.seg_blocks, b1 = b0 + g.seg_blocks;                 // b0 < blocks
            first = tile_at[(size_t)f * scan_tiles + b0 / JPEG_ENC_SCAN_TILE] + counts[(size_t)f * g.blocks + b0];
            const long long end = b1 >= g.blocks ? all : tile_at[(size_t)f * scan_tiles + b1 / JPEG_ENC_SCAN_TILE] + counts[(size_t)f * g.blocks + b1];
            pad = (int)(-(end - first) & 7);
        }
        int total;
        const int pre = group_scan(pad, lds, total);                 // <= 256 x 7
        if (s < g.nseg) {
            seg_pad[(size_t)f * g.nseg + s] = carry + pre;
            seg_at[(size_t)f * g.nseg + s] = (first + carry + pre) >> 3;
        }
        carry += total;
    }
    __syncthreads();                                                  // (every thread has read frame_bits[f])
    if (threadIdx.x == 0) frame_bits[f] = all + carry;
}

// WRITE = false: ff_tiles[tile] = the FF bytes among the tile's unstuffed bytes.  WRITE = true: the bytes go to out, each FF with its 00.
template <bool WRITE>
__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_ff_kernel(const uint8_t* __restrict__ stream, const JpegEncGeom g, long long ff_tiles_n,
                                                                  const int64_t* __restrict__ frame_bits, int32_t* __restrict__ ff_tiles,
                                                                  const int64_t* __restrict__ ff_at, const int64_t* __restrict__ seg_at,
                                                                  uint8_t* __restrict__ out) {
    __shared__ int lds[ENC_WAVES];
    const int f = blockIdx.y;
    const long long bytes = (frame_bits[f] + 7) >> 3, first = (long long)blockIdx.x * JPEG_ENC_FF_TILE;
    const size_t tile = (size_t)f * (size_t)ff_tiles_n + blockIdx.x;
    if (first >= bytes) return;                                       // (the whole workgroup; jpeg_enc_ff_sums_kernel stops before this tile)
    const long long at = first + threadIdx.x * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < bytes) v = *(const uint4*)(stream + (size_t)f * (size_t)g.cap + at);     // at + 16 <= cap: both are multiples of 16
    const int valid = at >= bytes ? 0 : (bytes - at < 16 ? (int)(bytes - at) : 16);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) cnt += i < valid && ((w[i >> 2] >> (8 * (i & 3))) & 255u) == 255u;
    int total;
    const int pre = group_scan(cnt, lds, total);
    if constexpr (!WRITE) {
        if (threadIdx.x == 0) ff_tiles[tile] = total;
    } else {
        long long o = at + ff_at[tile] + pre;
        uint8_t* row = out + (size_t)f * (size_t)g.stride;
        // Restart markers: segment k >= 1 starts at unstuffed byte seg_at[k] (strictly rising: a segment holds at least one byte), and
        // FF D0+((k-1)&7) stands in front of that byte, never stuffed.  k: the first segment that starts at or behind this thread's bytes.
        int k = g.nseg;
        long long next = -1;
        if (g.nseg > 1 && valid) {
            const int64_t* sa = seg_at + (size_t)f * g.nseg;
            int lo = 1, hi = g.nseg;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sa[mid] < at) lo = mid + 1;
                else hi = mid;
            }
            k = lo;
            o += 2 * (k - 1);
            if (k < g.nseg) next = sa[k];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < valid) {
                if (at + i == next) {
                    if (o < g.stride) row[o] = 0xFF;
                    if (o + 1 < g.stride) row[o + 1] = (uint8_t)(0xD0 + ((k - 1) & 7));
                    o += 2, ++k;
                    next = k < g.nseg ? seg_at[(size_t)f * g.nseg + k] : -1;
                }
                const uint32_t byte = (w[i >> 2] >> (8 * (i & 3))) & 255u;
                if (o < g.stride) row[o] = (uint8_t)byte;
                ++o;
                if (byte == 255u) {
                    if (o < g.stride) row[o] = 0;
                    ++o;
                }
            }
        }
    }
}

__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_ff_sums_kernel(const int32_t* __restrict__ ff_tiles, long long ff_tiles_n,
                                                                       const int64_t* __restrict__ frame_bits, long long stride, int nseg,
                                                                       int64_t* __restrict__ ff_at, int32_t* __restrict__ sizes,
                                                                       int32_t* __restrict__ status) {
    __shared__ int lds[ENC_WAVES];
    const int f = blockIdx.x;
    const long long bytes = (frame_bits[f] + 7) >> 3, used = (bytes + JPEG_ENC_FF_TILE - 1) / JPEG_ENC_FF_TILE;     // <= ff_tiles_n
    long long carry = 0;
    for (long long t0 = 0; t0 < used; t0 += ENC_THREADS) {
        const long long t = t0 + threadIdx.x;
        const int v = t < used ? ff_tiles[(size_t)f * (size_t)ff_tiles_n + t] : 0;
        int total;
        const int pre = group_scan(v, lds, total);
        if (t < used) ff_at[(size_t)f * (size_t)ff_tiles_n + t] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) {
        const long long need = bytes + carry + (bytes ? 2 * (nseg - 1) : 0);     // the markers; a frame that was not coded has none
        sizes[f] = (int32_t)(need > 0x7fffffffLL ? 0x7fffffffLL : need);
        if (need > stride) status[f] |= SAGEN_JPEG_ENC_ST_CAPACITY;  // (the kernels that OR bits into status have finished)
    }
}

// sagen_jpeg_transcode: a file's coefficients from the decoder's natural order into the encoder's zigzag order, one thread each;
// the encoder's entropy half finds its go-ahead (qok) and a zeroed status of its own
__global__ __launch_bounds__(ENC_THREADS) void jpeg_enc_reorder_kernel(const int16_t* __restrict__ nat, long long total, int n,
                                                                       int16_t* __restrict__ zz, int32_t* __restrict__ qok,
                                                                       int32_t* __restrict__ enc_status) {
    const long long i = (long long)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (i == 0) *qok = 1;
    if (i < n) enc_status[i] = 0;
    if (i < total) zz[i] = nat[(i & ~63LL) + jpeg_natural((int)(i & 63))];
}

__global__ __launch_bounds__(64) void jpeg_enc_status_merge_kernel(const int32_t* __restrict__ enc_status, int n, int32_t* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < n) status[f] |= enc_status[f] << 8;                      // (the decoder's kernels that OR bits into status have finished)
}

// the entropy half: from the zigzag coefficients in scratch to out, sizes and the ENC_ST bits ORed into status
void jpeg_enc_entropy_launch(const JpegEncGeom& g, const JpegEncScratch& lay, char* base, uint8_t* out, int32_t* sizes, int32_t* status,
                             hipStream_t s) {
    int16_t* coef = (int16_t*)(base + lay.coef);
    int32_t* counts = (int32_t*)(base + lay.counts);
    int32_t* tiles = (int32_t*)(base + lay.tiles);
    int64_t* tile_at = (int64_t*)(base + lay.tile_at);
    int64_t* frame_bits = (int64_t*)(base + lay.frame_bits);
    int32_t* qok = (int32_t*)(base + lay.qok);
    int32_t* ff_tiles = (int32_t*)(base + lay.ff_tiles);
    int64_t* ff_at = (int64_t*)(base + lay.ff_at);
    uint8_t* stream = (uint8_t*)(base + lay.stream);
    int64_t* seg_pad = (int64_t*)(base + lay.seg_pad);               // (both read only where g.nseg > 1)
    int64_t* seg_at = (int64_t*)(base + lay.seg_at);
    const long long total = (long long)g.n * g.blocks;
    hipLaunchKernelGGL(jpeg_enc_bits_kernel<false>, dim3(cdiv(total, (long long)ENC_WAVES)), dim3(ENC_THREADS), 0, s, coef, g, qok, counts, tile_at,
                       lay.scan_tiles, seg_pad, (uint32_t*)stream, status);
    hipLaunchKernelGGL(jpeg_enc_scan_tiles_kernel, dim3(lay.scan_tiles, g.n), dim3(ENC_THREADS), 0, s, counts, g, lay.scan_tiles, tiles);
    hipLaunchKernelGGL(jpeg_enc_scan_sums_kernel, dim3(g.n), dim3(ENC_THREADS), 0, s, tiles, lay.scan_tiles, tile_at, frame_bits);
    if (g.nseg > 1)
        hipLaunchKernelGGL(jpeg_enc_seg_kernel, dim3(g.n), dim3(ENC_THREADS), 0, s, counts, tile_at, lay.scan_tiles, g, seg_pad, seg_at, frame_bits);
    hipLaunchKernelGGL(jpeg_enc_bits_kernel<true>, dim3(cdiv(total, (long long)ENC_WAVES)), dim3(ENC_THREADS), 0, s, coef, g, qok, counts, tile_at,
                       lay.scan_tiles, seg_pad, (uint32_t*)stream, status);
    hipLaunchKernelGGL(jpeg_enc_ff_kernel<false>, dim3((unsigned)lay.ff_tiles_n, g.n), dim3(ENC_THREADS), 0, s, stream, g, lay.ff_tiles_n, frame_bits,
                       ff_tiles, ff_at, seg_at, out);
    hipLaunchKernelGGL(jpeg_enc_ff_sums_kernel, dim3(g.n), dim3(ENC_THREADS), 0, s, ff_tiles, lay.ff_tiles_n, frame_bits, g.stride, g.nseg, ff_at, sizes,
                       status);
    hipLaunchKernelGGL(jpeg_enc_ff_kernel<true>, dim3((unsigned)lay.ff_tiles_n, g.n), dim3(ENC_THREADS), 0, s, stream, g, lay.ff_tiles_n, frame_bits,
                       ff_tiles, ff_at, seg_at, out);
}

}  // namespace

int jpeg_coefficients_launch(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                             int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, JpegHuff* huff, int16_t* coef, int32_t* status,
                             void* stream);                          // jpeg.hip

int run_jpeg_transcode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                       const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& d, const JpegEncGeom& g, uint8_t* out, int32_t* sizes, int32_t* status,
                       void* scratch, void* hip_stream) {
    const hipStream_t s = (hipStream_t)hip_stream;
    const JpegTranscodeScratch lay = jpeg_transcode_scratch_layout(d, g, n_hufftabs);
    const JpegScratch dl = jpeg_scratch_layout(d, n_hufftabs);
    const JpegEncScratch el = jpeg_enc_scratch_layout(g);
    char* base = (char*)scratch;
    JpegHuff* huff = (JpegHuff*)(base + dl.huff);
    int16_t* nat = (int16_t*)(base + dl.coef);
    char* enc = base + lay.enc;
    int32_t* enc_status = (int32_t*)(base + lay.enc_status);
    const int rc = jpeg_coefficients_launch(bytes, total_bytes, frames, segments, n_segments, JPEG_TRANSCODE_QTABS, hufftabs, n_hufftabs, d, huff, nat,
                                            status, hip_stream);
    if (rc != SAGEN_OK) return rc;
    const long long total = (long long)g.n * g.blocks * 64;          // >= n
    SAGEN_HIP_CHECK(hipMemsetAsync(enc + el.stream, 0, (size_t)g.n * (size_t)g.cap, s));
    hipLaunchKernelGGL(jpeg_enc_reorder_kernel, dim3(cdiv(total, (long long)ENC_THREADS)), dim3(ENC_THREADS), 0, s, nat, total, g.n,
                       (int16_t*)(enc + el.coef), (int32_t*)(enc + el.qok), enc_status);
    jpeg_enc_entropy_launch(g, el, enc, out, sizes, enc_status, s);
    hipLaunchKernelGGL(jpeg_enc_status_merge_kernel, dim3(cdiv(g.n, 64)), dim3(64), 0, s, enc_status, g.n, status);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_jpeg_encode(const uint8_t* frames, const JpegEncGeom& g, const uint16_t* qtabs, uint8_t* out, int32_t* sizes, int32_t* status,
                    void* scratch, void* hip_stream) {
    const hipStream_t s = (hipStream_t)hip_stream;
    const JpegEncScratch lay = jpeg_enc_scratch_layout(g);
    char* base = (char*)scratch;
    int32_t* qok = (int32_t*)(base + lay.qok);
    const long long total = (long long)g.n * g.blocks;
    SAGEN_HIP_CHECK(hipMemsetAsync(base + lay.stream, 0, (size_t)g.n * (size_t)g.cap, s));        // the unstuffed bit streams
    hipLaunchKernelGGL(jpeg_enc_init_kernel, dim3(cdiv(g.n, 64)), dim3(64), 0, s, qtabs, g, qok, status);
    hipLaunchKernelGGL(jpeg_enc_dct_kernel, dim3(cdiv(total, (long long)ENC_THREADS)), dim3(ENC_THREADS), 0, s, frames, qtabs, g, qok,
                       (int16_t*)(base + lay.coef));
    jpeg_enc_entropy_launch(g, lay, base, out, sizes, status, s);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
