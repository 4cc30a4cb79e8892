// Frame batches from a resident clip (include/sagen.h: sagen_assemble_frames): the per-pixel arithmetic of the step between the JPEG
// decoder and the network - which source pixel an output pixel of a rolled frame reads, and the un-coding of the flow folder's polar
// bytes (feeder.py:147-160 of the reference; FlowFrames.frames here).
//
// The same code runs on the device (feed.hip) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).  Every intermediate of the flow
// un-coding is rounded through a float32 cast, and the two products have no sum behind them: there is nothing to contract.
#pragma once
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define FEED_FN __host__ __device__ __forceinline__
#else
#define FEED_FN inline
#endif

namespace sagen {

constexpr int FEED_MAX_DIM = 16384;
enum { FEED_BYTES = 0, FEED_TABLE = 1, FEED_FLOW = 2 };                // `mode`
constexpr int feed_table_floats(int mode) { return mode == FEED_FLOW ? 512 : (mode == FEED_TABLE ? 256 : 0); }   // cos[256] then sin[256]

// the roll of one item, reduced once: s in [0, w) with s = shift (mod w) in the mathematical sense, any int32 shift
FEED_FN int feed_roll(int32_t shift, int w) {
    const int m = (int)(shift % (int32_t)w);           // w >= 1: the one overflowing case of %, a divisor of -1, cannot occur
    return m < 0 ? m + w : m;
}

// output column x of an item rolled by s reads source column (x - s) mod w; x, s in [0, w)
FEED_FN int feed_src_x(int x, int s, int w) {
    const int d = x - s;
    return d < 0 ? d + w : d;
}

// (b0, b2) -> (m cos a, m sin a, m): m = b2 * scale + lo in two steps, each a double operation rounded once to float32 - which is
// the float32 operation itself when scale and lo are float32 values widened (53 >= 2 * 24 + 2), and what numpy's in-place update of
// a float32 array by a float64 operand computes otherwise
FEED_FN void feed_flow_pixel(uint8_t b0, uint8_t b2, const float* cos_t, const float* sin_t, double scale, double lo, float out[3]) {
    float m = (float)((double)b2 * scale);
    m = (float)((double)m + lo);
    out[0] = m * cos_t[b0];
    out[1] = m * sin_t[b0];
    out[2] = m;
}

}  // namespace sagen
