// sagen_jpeg_decode_split on the device (gfx950): the entropy stage of csrc/jpeg.hip with many lanes per restart segment - per frame
// where there is no restart interval - by self-synchronisation of the Huffman stream.  The algorithm, its stages and the argument
// for "out and status are the one-lane path's" are csrc/jpeg_split_core.h, shared with the CPU twin; this file is the launches.
//
//   jpeg_split_seg_tiles_kernel    per tile of 256 segment rows: chunks of each row from the checked descriptors, their exclusive prefix
//                                  sum inside the tile, the tile's sum
//   jpeg_split_seg_sums_kernel     one workgroup over the tile sums: chunks in front of each tile; zeroes the frames' marks
//   jpeg_split_seg_finish_kernel   per row: its first chunk in the call; CAPACITY for the frame of a row that ends behind max_chunks
//   jpeg_split_round0_kernel       one lane per chunk slot: chunk -> row by search, the lenient pass from the true state / the guess
//   jpeg_split_round_kernel        rounds - 1 launches: a chunk whose predecessor's exit is not the entry it used decodes again from
//                                  it; every other lane copies its exit into this round's buffer and leaves
//   jpeg_split_place_tiles_kernel  settled? (UNSETTLED / ANOMALY marks); exclusive prefix sum of the finished blocks per tile of chunks
//   jpeg_split_place_sums_kernel   one workgroup over those tile sums
//   jpeg_split_write_kernel        one lane per chunk of an unmarked frame: the strict pass, coefficients and DC differences stored
//   jpeg_split_dc_tiles_kernel / _dc_sums_kernel / _dc_apply_kernel   the DC prefix sum per frame and component as a tile scan; the
//                                  apply takes the segment's base off, checks 16 bits and stores
//   jpeg_split_finish_kernel       per frame: the path value
//   jpeg_split_zero_kernel         zeroes the coefficient blocks of the frames with a path other than 0; jpeg.hip's one-lane entropy
//                                  kernel, gated the same way, decodes them again.  On a healthy call both return at once
// and jpeg.hip's tables, check, inverse DCT and pixel kernels around them, unchanged.  No workgroup waits on another and no flag is
// polled: the order comes from the launch boundaries alone, and the number of launches depends on the arguments only.
//
// The lanes of a wave walk different streams and diverge by construction; a launch with few chunks spreads them thin by the rule of
// jpeg_entropy_kernel (JPEG_SPLIT_WAVES waves get one lane each before any gets a second).  The lookahead tables stay in global memory.
// tools/jpeg_split_rate.py measures; DESIGN.md says what came out.
#include "kernels.h"
#include "jpeg_split_core.h"
#include "group_scan.h"

namespace sagen {

// jpeg.hip
int jpeg_front_launch(int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, int n_qtabs, const uint8_t* hufftabs,
                      int n_hufftabs, const JpegGeom& g, JpegHuff* huff, int16_t* coef, int32_t* status, void* stream);
int jpeg_entropy_redo_launch(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, const JpegGeom& g,
                             const JpegHuff* huff, int16_t* coef, int32_t* status, const int32_t* gate, void* stream);
int jpeg_back_launch(const sagen_jpeg_frame* frames, const uint16_t* qtabs, const JpegGeom& g, const int16_t* coef, const int32_t* status, uint8_t* planes,
                     uint8_t* out, void* stream);

namespace {

constexpr int JPEG_SPLIT_WAVES = 2048;             // 256 CUs x 4 SIMDs x 2, as JPEG_ENTROPY_WAVES

struct SplitArgs {
    const uint8_t* bytes;
    const sagen_jpeg_frame* frames;
    const int32_t* segments;
    const JpegHuff* huff;
    const int32_t* status;
    int64_t* seg_first;
    int32_t* chunk_seg;
    uint64_t* entry;
    int32_t* nblk;
    int32_t* fpath;                                  // [2][n]
    long long max_chunks;
    int n_segments, chunk_bytes, lanes;
};

__device__ __forceinline__ long long split_lane(const SplitArgs& a) {
    if ((int)threadIdx.x >= a.lanes) return -1;
    const long long c = (long long)blockIdx.x * a.lanes + threadIdx.x;
    return c < a.max_chunks ? c : -1;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_seg_tiles_kernel(const SplitArgs a, const JpegGeom g, int64_t* __restrict__ seg_tiles) {
    __shared__ int lds[SCAN_WAVES];
    const long long s = (long long)blockIdx.x * JPEG_SPLIT_TILE + threadIdx.x;
    long long v = 0;
    if (s < a.n_segments) {
        int f, k;
        uint32_t start, end;
        if (jpeg_split_segment(a.frames, a.segments, s, g, a.status, f, k, start, end)) v = jpeg_split_chunks_of(start, end, a.chunk_bytes);
    }
    long long total;
    const long long pre = group_scan64(v, lds, total);               // v <= 2^27 + 1
    if (s < a.n_segments) a.seg_first[s] = pre;
    if (threadIdx.x == 0) seg_tiles[blockIdx.x] = total;
}

// exclusive prefix sum of tiles[0 .. count) in place, the sum into tiles[count]; each value below 2^43
__device__ __forceinline__ void split_scan_tiles(int64_t* tiles, long long count, int* lds) {
    long long carry = 0;
    for (long long t0 = 0; t0 < count; t0 += SCAN_THREADS) {
        const long long t = t0 + threadIdx.x;
        const long long v = t < count ? tiles[t] : 0;
        long long total;
        const long long pre = group_scan64(v, lds, total);
        if (t < count) tiles[t] = carry + pre;
        carry += total;
    }
    if (threadIdx.x == 0) tiles[count] = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_seg_sums_kernel(int64_t* __restrict__ seg_tiles, long long n_seg_tiles, int32_t* __restrict__ fpath,
                                                                           int n) {
    __shared__ int lds[SCAN_WAVES];
    split_scan_tiles(seg_tiles, n_seg_tiles, lds);
    for (int i = threadIdx.x; i < 2 * n; i += SCAN_THREADS) fpath[i] = 0;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_seg_finish_kernel(const SplitArgs a, const JpegGeom g, const int64_t* __restrict__ seg_tiles,
                                                                             long long n_seg_tiles) {
    const long long s = (long long)blockIdx.x * JPEG_SPLIT_TILE + threadIdx.x;
    if (s == 0) a.seg_first[a.n_segments] = seg_tiles[n_seg_tiles];
    if (s >= a.n_segments) return;
    const long long first = seg_tiles[blockIdx.x] + a.seg_first[s];
    a.seg_first[s] = first;
    int f, k;
    uint32_t start, end;
    if (!jpeg_split_segment(a.frames, a.segments, s, g, a.status, f, k, start, end)) return;
    if (first + jpeg_split_chunks_of(start, end, a.chunk_bytes) > a.max_chunks) atomicOr(&a.fpath[f], (int32_t)SAGEN_JPEG_PATH_CAPACITY);
}

__global__ __launch_bounds__(64) void jpeg_split_round0_kernel(const SplitArgs a, const JpegGeom g, uint64_t* __restrict__ exit_out) {
    const long long c = split_lane(a);
    if (c < 0) return;
    long long s = -1;
    if (c < a.seg_first[a.n_segments]) {
        s = jpeg_split_search(a.seg_first, a.n_segments, c);
        if (a.fpath[a.segments[2 * s]]) s = -1;                       // (CAPACITY, a launch ago; the row is a valid one: it has chunks)
    }
    a.chunk_seg[c] = (int32_t)s;
    jpeg_split_round0(a.bytes, a.frames, a.segments, g, a.huff, a.status, a.seg_first, s, c, a.chunk_bytes, a.entry, exit_out, a.nblk);
}

__global__ __launch_bounds__(64) void jpeg_split_round_kernel(const SplitArgs a, const JpegGeom g, const uint64_t* __restrict__ exit_in,
                                                              uint64_t* __restrict__ exit_out) {
    const long long c = split_lane(a);
    if (c < 0) return;
    jpeg_split_round(a.bytes, a.frames, a.segments, g, a.huff, a.status, a.seg_first, a.chunk_seg, c, a.chunk_bytes, a.entry, exit_in, exit_out, a.nblk);
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_place_tiles_kernel(const SplitArgs a, const uint64_t* __restrict__ exit_final,
                                                                              int32_t* __restrict__ blk_local, int64_t* __restrict__ blk_tiles) {
    __shared__ int lds[SCAN_WAVES];
    const long long c = (long long)blockIdx.x * JPEG_SPLIT_TILE + threadIdx.x;
    int v = 0;
    if (c < a.max_chunks) {
        const int32_t s = a.chunk_seg[c];
        if (s >= 0) {
            v = a.nblk[c];                                           // <= (8 x 65536 + 32) / 2 bits: 256 of them stay below 2^26
            const int32_t mark = jpeg_split_settled(a.entry, exit_final, c);
            if (mark) atomicOr(&a.fpath[a.segments[2 * (size_t)s]], mark);
        }
    }
    int total;
    const int pre = group_scan(v, lds, total);
    if (c < a.max_chunks) blk_local[c] = pre;
    if (threadIdx.x == 0) blk_tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_place_sums_kernel(int64_t* __restrict__ blk_tiles, long long n_blk_tiles) {
    __shared__ int lds[SCAN_WAVES];
    split_scan_tiles(blk_tiles, n_blk_tiles, lds);
}

__global__ __launch_bounds__(64) void jpeg_split_write_kernel(const SplitArgs a, const JpegGeom g, const uint64_t* __restrict__ exit_final,
                                                              const int32_t* __restrict__ blk_local, const int64_t* __restrict__ blk_tiles,
                                                              int16_t* __restrict__ coef) {
    const long long c = split_lane(a);
    if (c < 0) return;
    const long long s = a.chunk_seg[c];
    if (s < 0 || a.fpath[a.segments[2 * s]]) return;                 // (marks of earlier launches; this one writes the second row only)
    const long long c0 = a.seg_first[s];
    int f;
    const int32_t mark = jpeg_split_write_chunk(a.bytes, a.frames, a.segments, g, a.huff, a.status, a.seg_first, s, c, a.chunk_bytes, a.entry, exit_final,
                                                a.nblk, blk_tiles[c / JPEG_SPLIT_TILE] + blk_local[c], blk_tiles[c0 / JPEG_SPLIT_TILE] + blk_local[c0],
                                                coef, f);
    if (mark && f >= 0) atomicOr(&a.fpath[g.n + f], mark);
}

// ---- the DC prefix sums: grid (tiles, components, frames) -------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_dc_tiles_kernel(const int16_t* __restrict__ coef, const JpegGeom g,
                                                                           const int32_t* __restrict__ status, int tiles_per_comp,
                                                                           int32_t* __restrict__ dc_local, uint32_t* __restrict__ dc_tiles) {
    __shared__ int lds[SCAN_WAVES];
    const int comp = blockIdx.y, f = blockIdx.z, t = blockIdx.x * JPEG_SPLIT_TILE + threadIdx.x;
    const int terms = g.mcus * jpeg_split_dc_per_mcu(g, comp);
    const bool live = t < terms && !(status[f] & SAGEN_JPEG_ST_DESC);
    const int v = live ? coef[((size_t)f * g.blocks + jpeg_split_dc_block(g, comp, t)) * 64] : 0;
    int total;
    const int pre = group_scan(v, lds, total);                       // |v| < 2^15
    if (live) dc_local[(size_t)f * g.blocks + jpeg_split_dc_offset(g, comp) + t] = pre + v;
    if (threadIdx.x == 0) dc_tiles[((size_t)f * 3 + comp) * tiles_per_comp + blockIdx.x] = (uint32_t)total;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_dc_sums_kernel(uint32_t* __restrict__ dc_tiles, const JpegGeom g, int tiles_per_comp) {
    __shared__ int lds[SCAN_WAVES];
    const int comp = blockIdx.x, f = blockIdx.y;
    const int count = (g.mcus * jpeg_split_dc_per_mcu(g, comp) + JPEG_SPLIT_TILE - 1) / JPEG_SPLIT_TILE;
    uint32_t* tiles = dc_tiles + ((size_t)f * 3 + comp) * tiles_per_comp;
    uint32_t carry = 0;                                               // modulo 2^32: differences of two sums are what is used
    for (int t0 = 0; t0 < count; t0 += SCAN_THREADS) {
        const int t = t0 + threadIdx.x;
        const int v = t < count ? (int)tiles[t] : 0;                 // |v| < 2^23
        int total;
        const int pre = group_scan(v, lds, total);
        if (t < count) tiles[t] = carry + (uint32_t)pre;
        carry += (uint32_t)total;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_dc_apply_kernel(int16_t* __restrict__ coef, const sagen_jpeg_frame* __restrict__ frames,
                                                                           const JpegGeom g, const int32_t* __restrict__ status, int tiles_per_comp,
                                                                           const int32_t* __restrict__ dc_local, const uint32_t* __restrict__ dc_tiles,
                                                                           int32_t* __restrict__ late) {
    const int comp = blockIdx.y, f = blockIdx.z, t = blockIdx.x * JPEG_SPLIT_TILE + threadIdx.x;
    if (t >= g.mcus * jpeg_split_dc_per_mcu(g, comp) || (status[f] & SAGEN_JPEG_ST_DESC)) return;
    const int32_t* local = dc_local + (size_t)f * g.blocks + jpeg_split_dc_offset(g, comp);
    const uint32_t* tiles = dc_tiles + ((size_t)f * 3 + comp) * tiles_per_comp;
    const int base = jpeg_split_dc_base(g, comp, t, frames[f].restart_interval);          // 0 <= base <= t: the interval passed the check
    const uint32_t here = tiles[t / JPEG_SPLIT_TILE] + (uint32_t)local[t];
    const uint32_t before = base > 0 ? tiles[(base - 1) / JPEG_SPLIT_TILE] + (uint32_t)local[base - 1] : 0u;
    const int32_t p = (int32_t)(here - before);
    if (p < -32768 || p > 32767) atomicOr(&late[f], (int32_t)SAGEN_JPEG_PATH_ANOMALY);
    coef[((size_t)f * g.blocks + jpeg_split_dc_block(g, comp, t)) * 64] = (int16_t)p;
}

__global__ __launch_bounds__(64) void jpeg_split_finish_kernel(int32_t* __restrict__ fpath, int n, int32_t* __restrict__ path) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    const int32_t v = jpeg_split_path_value(fpath[f] | fpath[n + f]);
    fpath[f] = v;
    if (path) path[f] = v;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_split_zero_kernel(int16_t* __restrict__ coef, const JpegGeom g, const int32_t* __restrict__ fpath) {
    const long long id = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x;              // one 16-byte piece each: 8 per block
    if (id >= (long long)g.n * g.blocks * 8) return;
    if (!fpath[id / ((long long)g.blocks * 8)]) return;
    ((uint4*)coef)[id] = make_uint4(0u, 0u, 0u, 0u);
}

inline unsigned split_grid(long long items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

int run_jpeg_decode_split(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                          const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out, int32_t* status,
                          void* scratch, void* stream, int chunk_bytes, int rounds, int64_t max_chunks, int32_t* path) {
    const hipStream_t st = (hipStream_t)stream;
    const JpegSplitScratch lay = jpeg_split_scratch_layout(g, n_hufftabs, n_segments, max_chunks);
    char* sc = (char*)scratch;
    JpegHuff* huff = (JpegHuff*)(sc + lay.base.huff);
    int16_t* coef = (int16_t*)(sc + lay.base.coef);
    uint8_t* planes = (uint8_t*)sc + lay.base.planes;
    int64_t* seg_tiles = (int64_t*)(sc + lay.seg_tiles);
    uint64_t* exit0 = (uint64_t*)(sc + lay.exit0);
    uint64_t* exit1 = (uint64_t*)(sc + lay.exit1);
    int32_t* blk_local = (int32_t*)(sc + lay.blk_local);
    int64_t* blk_tiles = (int64_t*)(sc + lay.blk_tiles);
    int32_t* dc_local = (int32_t*)(sc + lay.dc_local);
    uint32_t* dc_tiles = (uint32_t*)(sc + lay.dc_tiles);
    SplitArgs a;
    a.bytes = bytes, a.frames = frames, a.segments = segments, a.huff = huff, a.status = status;
    a.seg_first = (int64_t*)(sc + lay.seg_first), a.chunk_seg = (int32_t*)(sc + lay.chunk_seg), a.entry = (uint64_t*)(sc + lay.entry);
    a.nblk = (int32_t*)(sc + lay.nblk), a.fpath = (int32_t*)(sc + lay.fpath);
    a.max_chunks = max_chunks, a.n_segments = n_segments, a.chunk_bytes = chunk_bytes;
    const long long per_wave = (max_chunks + JPEG_SPLIT_WAVES - 1) / JPEG_SPLIT_WAVES;
    a.lanes = per_wave > 64 ? 64 : (int)per_wave;
    const unsigned lane_grid = split_grid(max_chunks, a.lanes);

    const int rc = jpeg_front_launch(total_bytes, frames, segments, n_segments, n_qtabs, hufftabs, n_hufftabs, g, huff, coef, status, stream);
    if (rc != SAGEN_OK) return rc;
    hipLaunchKernelGGL(jpeg_split_seg_tiles_kernel, dim3((unsigned)lay.n_seg_tiles), dim3(SCAN_THREADS), 0, st, a, g, seg_tiles);
    hipLaunchKernelGGL(jpeg_split_seg_sums_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, seg_tiles, lay.n_seg_tiles, a.fpath, g.n);
    hipLaunchKernelGGL(jpeg_split_seg_finish_kernel, dim3((unsigned)lay.n_seg_tiles), dim3(SCAN_THREADS), 0, st, a, g, seg_tiles, lay.n_seg_tiles);
    hipLaunchKernelGGL(jpeg_split_round0_kernel, dim3(lane_grid), dim3(64), 0, st, a, g, exit0);
    for (int r = 1; r < rounds; ++r)
        hipLaunchKernelGGL(jpeg_split_round_kernel, dim3(lane_grid), dim3(64), 0, st, a, g, r & 1 ? exit0 : exit1, r & 1 ? exit1 : exit0);
    const uint64_t* exit_final = (rounds - 1) & 1 ? exit1 : exit0;
    hipLaunchKernelGGL(jpeg_split_place_tiles_kernel, dim3((unsigned)lay.n_blk_tiles), dim3(SCAN_THREADS), 0, st, a, exit_final, blk_local, blk_tiles);
    hipLaunchKernelGGL(jpeg_split_place_sums_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, blk_tiles, lay.n_blk_tiles);
    hipLaunchKernelGGL(jpeg_split_write_kernel, dim3(lane_grid), dim3(64), 0, st, a, g, exit_final, blk_local, blk_tiles, coef);
    const dim3 dc_grid(lay.dc_tiles_per_comp, g.ncomp, g.n);
    hipLaunchKernelGGL(jpeg_split_dc_tiles_kernel, dc_grid, dim3(SCAN_THREADS), 0, st, coef, g, status, lay.dc_tiles_per_comp, dc_local, dc_tiles);
    hipLaunchKernelGGL(jpeg_split_dc_sums_kernel, dim3(g.ncomp, g.n), dim3(SCAN_THREADS), 0, st, dc_tiles, g, lay.dc_tiles_per_comp);
    hipLaunchKernelGGL(jpeg_split_dc_apply_kernel, dc_grid, dim3(SCAN_THREADS), 0, st, coef, frames, g, status, lay.dc_tiles_per_comp, dc_local, dc_tiles,
                       a.fpath + g.n);
    hipLaunchKernelGGL(jpeg_split_finish_kernel, dim3(split_grid(g.n, 64)), dim3(64), 0, st, a.fpath, g.n, path);
    hipLaunchKernelGGL(jpeg_split_zero_kernel, dim3(split_grid((long long)g.n * g.blocks * 8, SCAN_THREADS)), dim3(SCAN_THREADS), 0, st, coef, g, a.fpath);
    const int rc2 = jpeg_entropy_redo_launch(bytes, frames, segments, n_segments, g, huff, coef, status, a.fpath, stream);
    if (rc2 != SAGEN_OK) return rc2;
    return jpeg_back_launch(frames, qtabs, g, coef, status, planes, out, stream);
}

}  // namespace sagen
