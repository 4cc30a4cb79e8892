// Audio windows from a resident clip (include/sagen.h: sagen_assemble_audio): the per-row arithmetic of the step between the wav
// pieces and the network - which source row a window row reads (the lead / read_from / read_count columns of feeder.window_table),
// what a stored sample is worth as a double (feeder.load_wav), and the yaw rotation of a first-order row (feeder.py:92-101 of the
// reference; feeder.rotation_matrix_z here).
//
// The same code runs on the device (audio_feed.hip) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).  The rotation is two
// products and a sum per output: contraction is off in both translation units, so each product is rounded before it is added.
#pragma once
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define AUDIO_FEED_FN __host__ __device__ __forceinline__
#else
#define AUDIO_FEED_FN inline
#endif
#if defined(__clang__)
#define AUDIO_FEED_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define AUDIO_FEED_NO_CONTRACT                 // g++ has no such pragma: the twin's build line passes -ffp-contract=off
#endif

namespace sagen {

constexpr int AUDIO_FEED_MAX_CHANNELS = 16;
constexpr int AUDIO_FEED_MAX_SIZE = 1 << 24;
enum { AUDIO_I16 = 0, AUDIO_F32 = 1, AUDIO_F64 = 2 };                  // `sample_type`
constexpr int audio_feed_elem_bytes(int sample_type) { return sample_type == AUDIO_I16 ? 2 : (sample_type == AUDIO_F32 ? 4 : 8); }

// Row j (0 <= j < size <= 2^24) of a window: true and *src in [0, n_samples) when it is a source row, false when it is padding.
// k = j - lead fits int64 for any int32 lead; with 0 <= k < count <= 2^31 - 1 neither -k nor n_samples - k (n_samples >= 0) can
// overflow, and read_from + k then lies in [0, n_samples): any int32 / int64 content is legal.
AUDIO_FEED_FN bool audio_feed_src_row(int j, int32_t lead, int64_t read_from, int32_t count, int64_t n_samples, int64_t* src) {
    const int64_t k = (int64_t)j - (int64_t)lead;
    if (k < 0 || k >= (int64_t)count) return false;
    if (read_from < -k || read_from >= n_samples - k) return false;
    *src = read_from + k;
    return true;
}

// what feeder.load_wav makes of a stored sample
AUDIO_FEED_FN double audio_feed_value(int16_t s) { return (double)s / 32768.0; }
AUDIO_FEED_FN double audio_feed_value(float s) { return (double)s; }
AUDIO_FEED_FN double audio_feed_value(double s) { return s; }

// (W, Y, Z, X) about the vertical axis by (c, s) = (cos, sin): Y' = c Y + s X, X' = c X - s Y, in this order
AUDIO_FEED_FN void audio_feed_rotate(double v[4], double c, double s) {
    AUDIO_FEED_NO_CONTRACT
    const double y = v[1], x = v[3];
    const double cy = c * y, sx = s * x, cx = c * x, sy = s * y;
    v[1] = cy + sx;
    v[3] = cx - sy;
}

}  // namespace sagen
