// PNG frame encode on the device (gfx950): the row filters and a zlib stream per frame - include/sagen.h: sagen_png_filter, sagen_deflate;
// the arithmetic is csrc/png_core.h, shared with the CPU twin.  It replaces the host's Image.save (PIL / zlib, one thread) behind the
// overlay writers.  As in jpeg_enc.hip no stage walks a frame: a position knows its token from its run alone, a block knows its bits
// before it writes one.
//
//   png_filter_kernel      one workgroup per row: the five filters' sums of min(v, 256 - v), the smallest wins, the row is written
//   deflate_plan_kernel    one workgroup per block of 16 384 bytes, a thread per chunk of 64: the chunk's run starts as a 64-bit mask, the
//                          nearest run start on either side through the wave's ballot (the two segmented scans), every token into the
//                          histogram of the 286 symbols, the two Adler sums; then the Huffman code in LDS (rank sort by all threads,
//                          lengths and the 15-bit limit by one, canonical codes by all), the three costs, the choice
//   deflate_place_kernel   one workgroup per frame over its blocks (1 / 16 384 of the bytes): each block's first bit - a stored block
//                          rounds up to a byte, so the positions are a walk, 256 blocks at a time through LDS - Adler-32, sizes[f],
//                          CAPACITY, and the stream's two ends
//   deflate_bits_kernel    the block again with its code and its position: each thread's bit count, a prefix sum over the 256, then the
//                          thread writes its own contiguous range - whole words as plain stores, the two it may share with its neighbours
//                          by atomicOr on the zeroed stream (OR commutes: the result does not depend on the order)
//   deflate_copy_kernel    min(sizes[f], stride) bytes of the frame's stream to out; nothing else of out is touched
// No workgroup waits on another: the order comes from the launch boundaries alone.
//
// tools/png_encode_rate.py measures the stages; DESIGN.md says what they cost.
#include "kernels.h"
#include "png_core.h"
#include "wave_reduce.h"

namespace sagen {

namespace {

constexpr int PNG_THREADS = 256;
constexpr int PNG_WAVES = PNG_THREADS / 64;
constexpr int PNG_PITCH = PNG_CHUNK / 4 + 1;       // words between two chunks in LDS: odd, so the 64 lanes of a wave read 64 banks
static_assert(PNG_CHUNKS == PNG_THREADS, "one thread per chunk");

template <int M = 1>
__device__ __forceinline__ int wave_sum_i(int v) {
    if constexpr (M < 64) {
        int a, b;
        lane_pair<M>(v, a, b);
        return wave_sum_i<M * 2>(a + b);
    } else {
        return v;
    }
}

// exclusive prefix sum over the 64 lanes (pre) and the wave's sum (tot), by the butterfly of wave_reduce.h (as in jpeg_enc.hip)
template <int M = 1>
__device__ __forceinline__ void wave_scan_i(int lane, int& pre, int& tot) {
    if constexpr (M < 64) {
        int a, b;
        lane_pair<M>(tot, a, b);
        const int other = a + b - tot;
        if (lane & M) pre += other;
        tot = a + b;
        wave_scan_i<M * 2>(lane, pre, tot);
    }
}

__device__ __forceinline__ int group_scan_i(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pre = 0, tot = v;
    wave_scan_i(lane, pre, tot);
    if (lane == 0) lds[wave] = tot;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < PNG_WAVES; ++i) {
        const int t = lds[i];
        base += i < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return base + pre;
}

__global__ __launch_bounds__(PNG_THREADS) void png_filter_kernel(const uint8_t* __restrict__ frames, int w, int h, int comps,
                                                                 uint8_t* __restrict__ rows) {
    __shared__ int part[PNG_WAVES][5];
    const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wc = w * comps;
    const size_t r = (size_t)blockIdx.y * h + y;
    const uint8_t* cur = frames + r * wc;
    const uint8_t* up = y ? cur - wc : nullptr;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, v, a, b, c;
    for (int x = threadIdx.x; x < wc; x += PNG_THREADS) {
        png_neighbours(cur, up, x, comps, v, a, b, c);
        s0 += png_filter_cost(png_filtered(0, v, a, b, c));
        s1 += png_filter_cost(png_filtered(1, v, a, b, c));
        s2 += png_filter_cost(png_filtered(2, v, a, b, c));
        s3 += png_filter_cost(png_filtered(3, v, a, b, c));
        s4 += png_filter_cost(png_filtered(4, v, a, b, c));
    }
    s0 = wave_sum_i(s0), s1 = wave_sum_i(s1), s2 = wave_sum_i(s2), s3 = wave_sum_i(s3), s4 = wave_sum_i(s4);     // <= 128 x 49 152 a row
    if (lane == 0) part[wave][0] = s0, part[wave][1] = s1, part[wave][2] = s2, part[wave][3] = s3, part[wave][4] = s4;
    __syncthreads();
    s0 = s1 = s2 = s3 = s4 = 0;
    for (int i = 0; i < PNG_WAVES; ++i) s0 += part[i][0], s1 += part[i][1], s2 += part[i][2], s3 += part[i][3], s4 += part[i][4];
    const int best = png_filter_choice(s0, s1, s2, s3, s4);
    uint8_t* o = rows + r * ((size_t)wc + 1);
    if (threadIdx.x == 0) o[0] = (uint8_t)best;
    for (int x = threadIdx.x; x < wc; x += PNG_THREADS) {
        png_neighbours(cur, up, x, comps, v, a, b, c);
        o[1 + x] = (uint8_t)png_filtered(best, v, a, b, c);
    }
}

// the block's bytes into LDS, chunk t at words[t PNG_PITCH], zeros behind its end l; src may be unaligned
__device__ __forceinline__ void block_stage(const uint8_t* __restrict__ src, int l, uint32_t* words) {
    for (int j = threadIdx.x; j < PNG_BLOCK / 4; j += PNG_THREADS) {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k)
            if (4 * j + k < l) v |= (uint32_t)src[4 * j + k] << (8 * k);
        words[(j >> 4) * PNG_PITCH + (j & 15)] = v;
    }
    __syncthreads();
}

// The chunk's run mask and the two Adler shares, then the nearest run start on either side of the chunk: the lanes of a wave find the
// nearest chunk that holds one in the wave's ballot, the other waves' ballots lie in LDS.
__device__ __forceinline__ uint64_t block_runs(const uint32_t* words, int l, uint64_t* masks, uint64_t* any, int& left, int& right, uint32_t& s1,
                                               uint32_t& tt) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int prev = t ? (int)(words[(t - 1) * PNG_PITCH + 15] >> 24) : 0;
    const uint64_t neq = png_chunk_mask(words + t * PNG_PITCH, prev, t * PNG_CHUNK, l, s1, tt);
    masks[t] = neq;
    const uint64_t mine = __ballot(neq != 0);
    if (lane == 0) any[wave] = mine;
    __syncthreads();
    int from = -1;
    uint64_t m = mine & ((1ull << lane) - 1ull);
    if (m) from = wave * 64 + 63 - __builtin_clzll(m);
    for (int i = wave - 1; i >= 0 && from < 0; --i) {
        const uint64_t a = any[i];
        if (a) from = i * 64 + 63 - __builtin_clzll(a);
    }
    left = from < 0 ? 0 : from * PNG_CHUNK + 63 - __builtin_clzll(masks[from]);
    from = -1;
    m = lane < 63 ? mine >> (lane + 1) : 0;
    if (m) from = t + 1 + __builtin_ctzll(m);
    for (int i = wave + 1; i < PNG_WAVES && from < 0; ++i) {
        const uint64_t a = any[i];
        if (a) from = i * 64 + __builtin_ctzll(a);
    }
    right = from < 0 ? l : from * PNG_CHUNK + __builtin_ctzll(masks[from]);
    return neq;
}

__global__ __launch_bounds__(PNG_THREADS) void deflate_plan_kernel(const uint8_t* __restrict__ data, const DeflateGeom g, int32_t* __restrict__ kind,
                                                                   int32_t* __restrict__ bits, uint32_t* __restrict__ s1_out,
                                                                   uint64_t* __restrict__ tt_out, uint32_t* __restrict__ tables) {
    __shared__ uint32_t words[PNG_CHUNKS * PNG_PITCH];
    __shared__ uint64_t masks[PNG_CHUNKS], any[PNG_WAVES];
    __shared__ int hist[PNG_SYMS], sorted[PNG_SYMS], order[PNG_SYMS], lens[PNG_SYMS], cnt[PNG_MAX_BITS + 1], first[PNG_MAX_BITS + 1];
    __shared__ int n_used;
    __shared__ uint32_t s1_sum;
    __shared__ unsigned long long tt_sum;
    const int t = threadIdx.x, f = blockIdx.y, b = blockIdx.x;
    const size_t id = (size_t)f * g.nblocks + b;
    const int l = deflate_block_length(g.length, b);
    for (int s = t; s < PNG_SYMS; s += PNG_THREADS) hist[s] = s == 256 ? 1 : 0, lens[s] = 0;
    if (t == 0) n_used = 0, s1_sum = 0, tt_sum = 0;
    block_stage(data + (size_t)f * (size_t)g.length + (size_t)b * PNG_BLOCK, l, words);
    int left, right;
    uint32_t s1, tt;
    const uint64_t neq = block_runs(words, l, masks, any, left, right, s1, tt);
    png_chunk_walk(words + t * PNG_PITCH, neq, t * PNG_CHUNK, l, left, right, [&](int byte, int k, int len) {
        int sym = byte, ebits, extra;
        if (k == 2) png_length_symbol(len, sym, ebits, extra);
        atomicAdd(&hist[sym], 1);
    });
    if (s1) atomicAdd(&s1_sum, s1);
    if (tt) atomicAdd(&tt_sum, (unsigned long long)tt);
    __syncthreads();
    for (int s = t; s < PNG_SYMS; s += PNG_THREADS) {
        if (hist[s]) {
            const int r = png_huff_rank(hist, s);
            order[r] = s, sorted[r] = hist[s];
            atomicAdd(&n_used, 1);
        }
    }
    __syncthreads();
    if (t == 0) {
        png_huff_lengths(sorted, n_used, cnt);
        png_huff_first_codes(cnt, first);
    }
    __syncthreads();
    for (int r = t; r < n_used; r += PNG_THREADS) lens[order[r]] = sorted[r];
    __syncthreads();
    if (t == 0) {
        int dyn, fix, nbits;
        png_block_costs(hist, lens, n_used, dyn, fix);
        kind[id] = png_block_choice(l, dyn, fix, nbits);
        bits[id] = nbits;
        s1_out[id] = s1_sum;
        tt_out[id] = tt_sum;
    }
    for (int s = t; s < PNG_SYMS; s += PNG_THREADS) tables[id * PNG_SYMS + s] = png_huff_entry(lens, first, s);
}

__global__ __launch_bounds__(PNG_THREADS) void deflate_place_kernel(const int32_t* __restrict__ kind, const int32_t* __restrict__ bits,
                                                                    const uint32_t* __restrict__ s1, const uint64_t* __restrict__ tt,
                                                                    const DeflateGeom g, int64_t* __restrict__ at, uint8_t* __restrict__ stream,
                                                                    int32_t* __restrict__ sizes, int32_t* __restrict__ status) {
    __shared__ int s_kind[PNG_THREADS], s_bits[PNG_THREADS];
    __shared__ long long s_at[PNG_THREADS];
    __shared__ long long carry;
    __shared__ uint32_t sum1, sum2;
    const int t = threadIdx.x, f = blockIdx.x;
    if (t == 0) carry = 16, sum1 = 0, sum2 = 0;
    uint32_t a1 = 0, a2 = 0;
    for (int b0 = 0; b0 < g.nblocks; b0 += PNG_THREADS) {
        const int b = b0 + t;
        const size_t id = (size_t)f * g.nblocks + b;
        if (b < g.nblocks) {
            s_kind[t] = kind[id], s_bits[t] = bits[id];
            a1 = (a1 + s1[id] % PNG_ADLER) % PNG_ADLER;
            a2 = (a2 + png_adler_share(g.length, (long long)b * PNG_BLOCK, deflate_block_length(g.length, b), s1[id], tt[id])) % PNG_ADLER;
        }
        __syncthreads();
        if (t == 0) {
            long long p = carry;
            const int m = g.nblocks - b0 < PNG_THREADS ? g.nblocks - b0 : PNG_THREADS;
            for (int i = 0; i < m; ++i) {
                s_at[i] = p;
                p = png_block_end(p, s_kind[i], s_bits[i]);
            }
            carry = p;
        }
        __syncthreads();
        if (b < g.nblocks) at[id] = s_at[t];
        __syncthreads();
    }
    atomicAdd(&sum1, a1);                                                // <= 256 x 65 520
    atomicAdd(&sum2, a2);
    __syncthreads();
    if (t == 0) {
        const long long need = png_frame_ends((uint32_t*)(stream + (size_t)f * (size_t)g.cap), carry, g.length, sum1 % PNG_ADLER, sum2 % PNG_ADLER);
        sizes[f] = (int32_t)need;
        status[f] = need > g.stride ? SAGEN_DEFLATE_ST_CAPACITY : 0;
    }
}

__global__ __launch_bounds__(PNG_THREADS) void deflate_bits_kernel(const uint8_t* __restrict__ data, const DeflateGeom g,
                                                                   const int32_t* __restrict__ kind, const int64_t* __restrict__ at,
                                                                   const uint32_t* __restrict__ tables, uint8_t* __restrict__ stream) {
    __shared__ uint32_t words[PNG_CHUNKS * PNG_PITCH];
    __shared__ uint64_t masks[PNG_CHUNKS], any[PNG_WAVES];
    __shared__ uint32_t table[PNG_SYMS];
    __shared__ int lds[PNG_WAVES];
    const int t = threadIdx.x, f = blockIdx.y, b = blockIdx.x;
    const size_t id = (size_t)f * g.nblocks + b;
    const int l = deflate_block_length(g.length, b), k = kind[id];     // (uniform over the workgroup, like every branch on k below)
    const long long pos = at[id];
    const bool final = b == g.nblocks - 1;
    uint32_t* out = (uint32_t*)(stream + (size_t)f * (size_t)g.cap);
    block_stage(data + (size_t)f * (size_t)g.length + (size_t)b * PNG_BLOCK, l, words);
    if (k == PNG_STORED) {
        const long long body = ((pos + 3 + 7) & ~7LL) + 32;
        if (t == 0) png_stored_header(out, pos, final, l);
        png_stored_chunk(out, body + 8LL * t * PNG_CHUNK, words + t * PNG_PITCH, t * PNG_CHUNK, l);
        return;
    }
    for (int s = t; s < PNG_SYMS; s += PNG_THREADS) {
        uint32_t code;
        int len;
        png_fixed_code(s, code, len);
        table[s] = k == PNG_FIXED ? png_pack(code, len) : tables[id * PNG_SYMS + s];
    }
    int left, right;
    uint32_t s1, tt;
    const uint64_t neq = block_runs(words, l, masks, any, left, right, s1, tt);     // (its barrier also covers `table`)
    const int dist_bits = k == PNG_FIXED ? 5 : 1, head = k == PNG_FIXED ? 3 : PNG_DYN_HEADER;
    int mine = 0;
    png_chunk_walk(words + t * PNG_PITCH, neq, t * PNG_CHUNK, l, left, right, [&](int byte, int kk, int len) {
        uint32_t v;
        mine += png_token_bits(table, byte, kk, len, dist_bits, v);
    });
    int total;
    const int pre = group_scan_i(mine, lds, total);                      // <= 16 384 x 15 bits
    PngSink sink;
    png_sink_open(sink, out, pos + head + pre);
    png_chunk_walk(words + t * PNG_PITCH, neq, t * PNG_CHUNK, l, left, right, [&](int byte, int kk, int len) {
        uint32_t v;
        const int nb = png_token_bits(table, byte, kk, len, dist_bits, v);
        png_sink_put(sink, v, nb);
    });
    png_sink_close(sink);
    if (t == 0) png_or_bits(out, pos + head + total, table[256] >> 4, (int)(table[256] & 15));
    // the header's fields, one per thread (png_block_header is the same thing by one writer)
    if (k == PNG_FIXED) {
        if (t == 0) png_or_bits(out, pos, (final ? 1u : 0u) | (1u << 1), 3);
    } else {
        if (t == 0) png_or_bits(out, pos, png_dyn_header17(final), 17);
        if (t < 19) png_or_bits(out, pos + 17 + 3 * t, png_clen_field(t), 3);
        for (int s = t; s <= PNG_SYMS; s += PNG_THREADS) png_or_bits(out, pos + 17 + 57 + 4 * s, png_len_field(table, s), 4);
    }
}

__global__ __launch_bounds__(PNG_THREADS) void deflate_copy_kernel(const uint8_t* __restrict__ stream, const DeflateGeom g,
                                                                   const int32_t* __restrict__ sizes, uint8_t* __restrict__ out) {
    const int f = blockIdx.y;
    const long long need = sizes[f], n = need < g.stride ? need : g.stride;
    const long long o = ((long long)blockIdx.x * PNG_THREADS + threadIdx.x) * 16;
    if (o >= n) return;
    const uint8_t* src = stream + (size_t)f * (size_t)g.cap + o;         // 16-byte aligned; o + 16 <= cap: both are multiples of 16
    uint8_t* dst = out + (size_t)f * (size_t)g.stride + o;               // 4-byte aligned
    if (o + 16 <= n) {
        const uint4 v = *(const uint4*)src;
        uint32_t* d = (uint32_t*)dst;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
        for (int i = 0; i < (int)(n - o); ++i) dst[i] = src[i];
    }
}

}  // namespace

int run_png_filter(const uint8_t* frames, int n, int w, int h, int components, uint8_t* rows, void* hip_stream) {
    hipLaunchKernelGGL(png_filter_kernel, dim3(h, n), dim3(PNG_THREADS), 0, (hipStream_t)hip_stream, frames, w, h, components, rows);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_deflate(const uint8_t* data, const DeflateGeom& g, uint8_t* out, int32_t* sizes, int32_t* status, void* scratch, void* hip_stream) {
    const hipStream_t s = (hipStream_t)hip_stream;
    const DeflateScratch lay = deflate_scratch_layout(g);
    char* base = (char*)scratch;
    int32_t* kind = (int32_t*)(base + lay.kind);
    int32_t* bits = (int32_t*)(base + lay.bits);
    uint32_t* s1 = (uint32_t*)(base + lay.s1);
    uint64_t* tt = (uint64_t*)(base + lay.tt);
    int64_t* at = (int64_t*)(base + lay.at);
    uint32_t* tables = (uint32_t*)(base + lay.table);
    uint8_t* stream = (uint8_t*)(base + lay.stream);
    const long long reach = g.cap < g.stride ? g.cap : g.stride;
    SAGEN_HIP_CHECK(hipMemsetAsync(stream, 0, (size_t)g.n * (size_t)g.cap, s));
    hipLaunchKernelGGL(deflate_plan_kernel, dim3(g.nblocks, g.n), dim3(PNG_THREADS), 0, s, data, g, kind, bits, s1, tt, tables);
    hipLaunchKernelGGL(deflate_place_kernel, dim3(g.n), dim3(PNG_THREADS), 0, s, kind, bits, s1, tt, g, at, stream, sizes, status);
    hipLaunchKernelGGL(deflate_bits_kernel, dim3(g.nblocks, g.n), dim3(PNG_THREADS), 0, s, data, g, kind, at, tables, stream);
    hipLaunchKernelGGL(deflate_copy_kernel, dim3(cdiv(reach, 16LL * PNG_THREADS), g.n), dim3(PNG_THREADS), 0, s, stream, g, sizes, out);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
