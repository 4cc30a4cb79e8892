// Frame batches from a resident clip (gfx950) - include/sagen.h: sagen_assemble_frames; the arithmetic is csrc/feed_core.h, shared
// with the CPU twin.  It stands where the reader threads of the reference stack, roll and un-code decoded frames on the host
// (feeder.py:106-161) and the batch then crosses the bus: here the decoded clip stays on the device (jpeg.hip) and a batch is one
// launch over it.
//
//   assemble_kernel<MODE>   one thread per output pixel, consecutive threads along a row; a workgroup row of the grid per output
//                           item, striding over the items (n_out may exceed what gridDim.y takes).  The item's frame index and roll
//                           are uniform over the workgroup (scalar loads); an index outside [0, n_frames) writes zeros and reads no
//                           frame, the roll is reduced into [0, w) before it meets a column: no content of index / shift can move
//                           an address outside the two arrays.  Three byte loads, then three byte stores (MODE 0) or three float
//                           stores; the 256 / 512 table entries are staged in LDS once per workgroup.  Rows are 3 w bytes and a
//                           roll starts anywhere, so nothing here assumes an alignment of the frames.  Offsets are 64-bit.
//
// tools/feed_rate.py measures it; DESIGN.md 3.17 says what bounds it.
#include "kernels.h"
#include "feed_core.h"

#pragma clang fp contract(off)

namespace sagen {

namespace {

constexpr int FEED_THREADS = 256;
constexpr int FEED_GRID_ITEMS = 1024;

template <int MODE>
__global__ __launch_bounds__(FEED_THREADS) void assemble_kernel(const uint8_t* __restrict__ frames, int n_frames, int h, int w,
                                                                const int32_t* __restrict__ index, const int32_t* __restrict__ shift,
                                                                int n_out, const float* __restrict__ table,
                                                                const double* __restrict__ scale_lo, void* __restrict__ out_) {
    constexpr int NT = feed_table_floats(MODE);
    __shared__ float tab[NT > 0 ? NT : 1];
    if (MODE != FEED_BYTES) {
        for (int k = threadIdx.x; k < NT; k += FEED_THREADS) tab[k] = table[k];
        __syncthreads();
    }
    const int hw = h * w;                                          // <= 2^28 (FEED_MAX_DIM^2)
    const int pix = (int)blockIdx.x * FEED_THREADS + (int)threadIdx.x;
    if (pix >= hw) return;
    const int y = pix / w, x = pix - y * w;
    for (int i = blockIdx.y; i < n_out; i += gridDim.y) {
        const long long o = ((long long)i * hw + pix) * 3;
        const int f = index[i];
        if (f < 0 || f >= n_frames) {                              // padding
            if (MODE == FEED_BYTES) {
                uint8_t* q = (uint8_t*)out_ + o;
                q[0] = 0; q[1] = 0; q[2] = 0;
            } else {
                float* q = (float*)out_ + o;
                q[0] = 0.f; q[1] = 0.f; q[2] = 0.f;
            }
            continue;
        }
        const int sx = feed_src_x(x, feed_roll(shift[i], w), w);
        const uint8_t* p = frames + ((long long)f * hw + (long long)y * w + sx) * 3;
        const uint8_t b0 = p[0], b1 = p[1], b2 = p[2];
        if (MODE == FEED_BYTES) {
            uint8_t* q = (uint8_t*)out_ + o;
            q[0] = b0; q[1] = b1; q[2] = b2;
        } else if (MODE == FEED_TABLE) {
            float* q = (float*)out_ + o;
            q[0] = tab[b0]; q[1] = tab[b1]; q[2] = tab[b2];
        } else {
            float v[3];
            feed_flow_pixel(b0, b2, tab, tab + 256, scale_lo[2 * (long long)f], scale_lo[2 * (long long)f + 1], v);
            float* q = (float*)out_ + o;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
        }
    }
}

}  // namespace

int run_assemble_frames(const uint8_t* frames, int n_frames, int h, int w, const int32_t* index, const int32_t* shift, int n_out, int mode,
                        const float* table, const double* scale_lo, void* out, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv((long)h * w, FEED_THREADS), n_out < FEED_GRID_ITEMS ? n_out : FEED_GRID_ITEMS), block(FEED_THREADS);
    switch (mode) {
        case FEED_BYTES: hipLaunchKernelGGL((assemble_kernel<FEED_BYTES>), grid, block, 0, s, frames, n_frames, h, w, index, shift, n_out, table, scale_lo, out); break;
        case FEED_TABLE: hipLaunchKernelGGL((assemble_kernel<FEED_TABLE>), grid, block, 0, s, frames, n_frames, h, w, index, shift, n_out, table, scale_lo, out); break;
        default: hipLaunchKernelGGL((assemble_kernel<FEED_FLOW>), grid, block, 0, s, frames, n_frames, h, w, index, shift, n_out, table, scale_lo, out); break;
    }
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
