// Rational polyphase FIR resampling and windowed RMS (include/sagen.h: sagen_resample_fir, sagen_window_rms): the index arithmetic,
// the checks and the per-output sums.  In place of resampy's 'kaiser_fast' in load_wav (pyutils/iolib/audio.py:23), ffmpeg's
// `-ar 48000` + `pan` remap (scraping/preprocess.py:14-34) and AmbisonicArray.convert (pyutils/ambisonics/common.py:34-59); a
// resampler of our own, bit-compatible with none of them.
//
// The same code runs on the device (resample.hip) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).  Every sum is fp64 in ONE
// order, each product rounded before it is added (compiled WITHOUT contraction), so that both builds and a numpy restatement of the
// definition give the same fp64 value before the one rounding to fp32.
//
//   y[n][o] = sum_m h[n M - m L] z[m][o],   z[m][o] = sum_c mix[o][c] x[m][c]   (mix absent: z = x),   |n M - m L| <= H
//
// With p = (n M) mod L the taps output n uses are h[p + j L]: row p of the phase table, stored so that t ascending is m ascending:
//   taps[p][t] = h[kmax(p) - t L],  kmax(p) = p + L floor((H - p) / L)  (the largest k <= H congruent to p), zero where below -H
//   m = m0(n) + t,  m0(n) = ceil((n M - H) / L)  (the first row output n reaches)
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define RESAMPLE_FN __host__ __device__ __forceinline__
#else
#define RESAMPLE_FN inline
#endif
#if defined(__clang__)
#define RESAMPLE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RESAMPLE_NO_CONTRACT                   // g++ has no such pragma: the twin's build line passes -ffp-contract=off
#endif

namespace sagen {

constexpr int RESAMPLE_MAX_CHANNELS = 64;
constexpr int RESAMPLE_MAX_T = 4096;                           // taps per phase
constexpr int RESAMPLE_MAX_RATIO = 1 << 20;                    // L and M: n M stays below 2^61
constexpr long long RESAMPLE_MAX_POS = 1ll << 40;              // stream positions, input and output
constexpr long long RESAMPLE_MAX_TABLE_BYTES = 64ll << 20;
constexpr int RMS_LANES = 64;                                  // partial sums per window: one per lane of a wave

// What a checked call works with, by value in the kernel arguments.
struct ResampleArgs {
    long long x0, n_in, n0, n;
    int c_in, c_out, L, M, H, T;
};

RESAMPLE_FN long long rs_floor_div(long long a, long long b) {          // b > 0
    const long long q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

RESAMPLE_FN long long rs_ceil_div(long long a, long long b) { return -rs_floor_div(-a, b); }

// first input row output n reaches, and its phase
RESAMPLE_FN long long rs_first_row(long long n, int L, int M, int H) { return rs_ceil_div(n * M - H, L); }
RESAMPLE_FN int rs_phase(long long n, int L, int M) { return (int)((n * M) % L); }

// z[m][o] of a row of the x buffer (r: row of the buffer, already known to lie inside it)
RESAMPLE_FN double rs_mix_row(const float* x, long long r, int c_in, const double* mix, int o) {
    RESAMPLE_NO_CONTRACT
    const float* row = x + r * c_in;
    if (!mix) return (double)row[o];
    const double* mr = mix + (long long)o * c_in;
    double acc = 0.;
    for (int c = 0; c < c_in; ++c) acc = acc + mr[c] * (double)row[c];
    return acc;
}

// sum_t taps[t] z[t * stride], t ascending: `taps` is the row of the phase, z the mixed rows from m0(n) on
template <class Z>
RESAMPLE_FN double rs_dot(const double* taps, const Z* z, int stride, int T) {
    RESAMPLE_NO_CONTRACT
    double acc = 0.;
    for (int t = 0; t < T; ++t) acc = acc + taps[t] * z[(long long)t * stride];
    return acc;
}

// the checks of sagen_resample_fir behind the null and n == 0 ones; *why names the parameter
inline int resample_args_fill(ResampleArgs& a, long long x0, long long n_in, int c_in, int L, int M, int H, int T, bool has_mix, int c_out,
                              long long n0, long long n, const char** why) {
    *why = "";
    if (L <= 0 || M <= 0 || T <= 0) { *why = "L, M and T must be positive"; return SAGEN_ERR_SHAPE; }
    if (H < 0) { *why = "H is negative"; return SAGEN_ERR_SHAPE; }
    if (x0 < 0 || n_in < 0 || n0 < 0 || n < 0) { *why = "negative x0, n_in, n0 or n"; return SAGEN_ERR_SHAPE; }
    if (c_in < 1 || c_out < 1) { *why = "c_in and c_out must be positive"; return SAGEN_ERR_SHAPE; }
    if (!has_mix && c_in != c_out) { *why = "c_out differs from c_in without a mix"; return SAGEN_ERR_SHAPE; }
    if ((long long)T != (2ll * H + 1 + L - 1) / L) { *why = "T is not ceil((2 H + 1) / L)"; return SAGEN_ERR_SHAPE; }
    if (c_in > RESAMPLE_MAX_CHANNELS || c_out > RESAMPLE_MAX_CHANNELS) { *why = "more than 64 channels"; return SAGEN_ERR_UNSUPPORTED; }
    if (T > RESAMPLE_MAX_T) { *why = "T above 4096"; return SAGEN_ERR_UNSUPPORTED; }
    if (L > RESAMPLE_MAX_RATIO || M > RESAMPLE_MAX_RATIO) { *why = "L or M above 2^20"; return SAGEN_ERR_UNSUPPORTED; }
    if ((long long)L * T * (long long)sizeof(double) > RESAMPLE_MAX_TABLE_BYTES) { *why = "tap table above 64 MiB"; return SAGEN_ERR_UNSUPPORTED; }
    if (x0 > RESAMPLE_MAX_POS || n_in > RESAMPLE_MAX_POS || n0 > RESAMPLE_MAX_POS || n > RESAMPLE_MAX_POS) {
        *why = "a position or count above 2^40";
        return SAGEN_ERR_UNSUPPORTED;
    }
    a.x0 = x0; a.n_in = n_in; a.n0 = n0; a.n = n;
    a.c_in = c_in; a.c_out = c_out; a.L = L; a.M = M; a.H = H; a.T = T;
    return SAGEN_OK;
}

// the checks of sagen_window_rms behind the null and count == 0 ones
inline int window_rms_check(long long n, int channels, int channel, long long first, long long hop, long long length, long long count,
                            const char** why) {
    *why = "";
    if (n < 0 || count < 0) { *why = "negative n or count"; return SAGEN_ERR_SHAPE; }
    if (channels < 1 || channel < 0 || channel >= channels) { *why = "channel outside the row"; return SAGEN_ERR_SHAPE; }
    if (length < 1 || hop < 0 || first < 0) { *why = "length must be positive, hop and first non-negative"; return SAGEN_ERR_SHAPE; }
    if (n > RESAMPLE_MAX_POS || channels > (1 << 20)) { *why = "n above 2^40 or more than 2^20 channels"; return SAGEN_ERR_UNSUPPORTED; }
    // the last window ends at first + (count - 1) hop + length <= n, without forming a product that could overflow
    if (length > n || first > n - length) { *why = "a window reaches past the rows"; return SAGEN_ERR_SHAPE; }
    if (hop > 0 && count - 1 > (n - length - first) / hop) { *why = "a window reaches past the rows"; return SAGEN_ERR_SHAPE; }
    if (count > (1ll << 31) - 1) { *why = "more than 2^31 - 1 windows"; return SAGEN_ERR_UNSUPPORTED; }
    return SAGEN_OK;
}

// lane l of a window's 64 partial sums: the squares of the samples j = l, l + 64, ... in ascending order (a square of an fp32 value
// is exact in fp64)
RESAMPLE_FN double rms_partial(const float* x, long long start, int channels, int channel, long long length, int lane) {
    RESAMPLE_NO_CONTRACT
    double acc = 0.;
    for (long long j = lane; j < length; j += RMS_LANES) {
        const double v = (double)x[(start + j) * channels + channel];
        acc = acc + v * v;
    }
    return acc;
}

// the butterfly the device's wave_sum_f64 performs on the partials (lane l adds lane l ^ 1, then ^ 2, ... ^ 32; a + b == b + a, so
// every lane holds the same bits), then the root of the mean
inline double rms_finish_host(double (&p)[RMS_LANES], long long length) {
    RESAMPLE_NO_CONTRACT
    for (int m = 1; m < RMS_LANES; m <<= 1) {
        double q[RMS_LANES];
        for (int l = 0; l < RMS_LANES; ++l) q[l] = p[l] + p[l ^ m];
        for (int l = 0; l < RMS_LANES; ++l) p[l] = q[l];
    }
    return std::sqrt(p[0] / (double)length);
}

}  // namespace sagen
