// Audio windows from a resident clip (gfx950) - include/sagen.h: sagen_assemble_audio; the arithmetic is csrc/audio_feed_core.h,
// shared with the CPU twin.  It stands where the reader threads of the reference cut every window out of the 1-second wav pieces,
// pad and rotate it on the host (feeder.py:50-103) and the batch then crosses the bus, and where train.py:107-111 slices the
// network's input and target out of it afterwards: here the clip's samples stay on the device as stored and a batch is one launch.
//
//   assemble_audio_kernel<T, PATH>   one thread per window row, consecutive threads along the window; a workgroup row of the grid
//                           per item, striding over the items (n_out may exceed what gridDim.y takes).  The item's lead, read_from,
//                           count and (cos, sin) are uniform over the workgroup (scalar loads).  Whether a row reads a sample is
//                           decided by audio_feed_src_row, which no int32 / int64 content can push out of [0, n_samples).  A row is
//                           widened to fp64 in registers, rotated there, narrowed once and written to every requested output in
//                           the same pass.
//                             PATH_VEC4   4 channels, `samples` aligned to a row (int16: 8 bytes, fp32 / fp64: 16) and `full`
//                                         to 16: a row is one 8-byte, one 16-byte or two 16-byte loads and one 16-byte store
//                             PATH_ROW4   4 channels, element loads and stores (a base aligned only to its element); the same values
//                             PATH_ANY    1..16 channels, channel by channel; no rotation (it needs 4 channels)
//                           mono rows are 4 bytes and target rows 4 (channels - 1) bytes per lane, consecutive over the lanes.
//                           Offsets are 64-bit.
//
// tools/audio_feed_rate.py measures it; DESIGN.md 3.18 says what bounds it.
#include "kernels.h"
#include "audio_feed_core.h"

#pragma clang fp contract(off)

namespace sagen {

namespace {

constexpr int AUDIO_FEED_THREADS = 256;
constexpr int AUDIO_FEED_GRID_ITEMS = 1024;
enum { PATH_ANY = 0, PATH_ROW4 = 1, PATH_VEC4 = 2 };

struct alignas(8) I16x4 { int16_t v[4]; };
struct alignas(16) F32x4 { float v[4]; };
struct alignas(16) F64x2 { double v[2]; };

__device__ __forceinline__ void load_row4(const int16_t* p, double v[4]) {
    const I16x4 r = *reinterpret_cast<const I16x4*>(p);
    for (int c = 0; c < 4; ++c) v[c] = audio_feed_value(r.v[c]);
}
__device__ __forceinline__ void load_row4(const float* p, double v[4]) {
    const F32x4 r = *reinterpret_cast<const F32x4*>(p);
    for (int c = 0; c < 4; ++c) v[c] = audio_feed_value(r.v[c]);
}
__device__ __forceinline__ void load_row4(const double* p, double v[4]) {
    const F64x2 a = *reinterpret_cast<const F64x2*>(p), b = *reinterpret_cast<const F64x2*>(p + 2);
    v[0] = a.v[0]; v[1] = a.v[1]; v[2] = b.v[0]; v[3] = b.v[1];
}

template <typename T, int PATH>
__global__ __launch_bounds__(AUDIO_FEED_THREADS) void assemble_audio_kernel(const T* __restrict__ samples, long long n_samples, int channels,
                                                                            const int32_t* __restrict__ lead,
                                                                            const int64_t* __restrict__ read_from,
                                                                            const int32_t* __restrict__ count,
                                                                            const double* __restrict__ rot, int n_out, int size, int t_off,
                                                                            int t_len, float* __restrict__ full, float* __restrict__ mono,
                                                                            float* __restrict__ target) {
    const int j = (int)blockIdx.x * AUDIO_FEED_THREADS + (int)threadIdx.x;         // size <= 2^24
    if (j >= size) return;
    const bool in_target = target && j >= t_off && j - t_off < t_len;
    for (int i = blockIdx.y; i < n_out; i += gridDim.y) {
        const int32_t ld = lead[i], cnt = count[i];
        const int64_t rf = read_from[i];
        const long long row = (long long)i * size + j;
        int64_t src = 0;
        const bool live = audio_feed_src_row(j, ld, rf, cnt, (int64_t)n_samples, &src);
        if (PATH == PATH_ANY) {
            const long long trow = ((long long)i * t_len + (j - t_off)) * (channels - 1);
            for (int c = 0; c < channels; ++c) {
                const float v = live ? (float)audio_feed_value(samples[src * channels + c]) : 0.f;
                if (full) full[row * channels + c] = v;
                if (c == 0) {
                    if (mono) mono[row] = v;
                } else if (in_target) {
                    target[trow + (c - 1)] = v;
                }
            }
        } else {
            F32x4 o = {{0.f, 0.f, 0.f, 0.f}};
            if (live) {
                double v[4];
                if (PATH == PATH_VEC4) {
                    load_row4(samples + src * 4, v);
                } else {
                    for (int c = 0; c < 4; ++c) v[c] = audio_feed_value(samples[src * 4 + c]);
                }
                if (rot) audio_feed_rotate(v, rot[2 * (long long)i], rot[2 * (long long)i + 1]);
                for (int c = 0; c < 4; ++c) o.v[c] = (float)v[c];
            }
            if (full) {
                if (PATH == PATH_VEC4) {
                    *reinterpret_cast<F32x4*>(full + row * 4) = o;
                } else {
                    for (int c = 0; c < 4; ++c) full[row * 4 + c] = o.v[c];
                }
            }
            if (mono) mono[row] = o.v[0];
            if (in_target) {
                float* q = target + ((long long)i * t_len + (j - t_off)) * 3;
                q[0] = o.v[1]; q[1] = o.v[2]; q[2] = o.v[3];
            }
        }
    }
}

template <typename T>
void launch(int path, dim3 grid, hipStream_t s, const void* samples, int64_t n_samples, int channels, const int32_t* lead,
            const int64_t* read_from, const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full,
            float* mono, float* target) {
    const dim3 block(AUDIO_FEED_THREADS);
    const T* p = (const T*)samples;
    const long long n = (long long)n_samples;
    switch (path) {
        case PATH_VEC4: hipLaunchKernelGGL((assemble_audio_kernel<T, PATH_VEC4>), grid, block, 0, s, p, n, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
        case PATH_ROW4: hipLaunchKernelGGL((assemble_audio_kernel<T, PATH_ROW4>), grid, block, 0, s, p, n, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
        default: hipLaunchKernelGGL((assemble_audio_kernel<T, PATH_ANY>), grid, block, 0, s, p, n, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
    }
}

}  // namespace

int run_assemble_audio(const void* samples, int sample_type, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from,
                       const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono,
                       float* target, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(size, AUDIO_FEED_THREADS), n_out < AUDIO_FEED_GRID_ITEMS ? n_out : AUDIO_FEED_GRID_ITEMS);
    const uintptr_t row_align = sample_type == AUDIO_I16 ? 8 : 16;
    int path = PATH_ANY;                                               // (rot implies channels == 4: the entry point has seen to it)
    if (channels == 4) path = (((uintptr_t)samples) % row_align == 0 && ((uintptr_t)full) % 16 == 0) ? PATH_VEC4 : PATH_ROW4;
    switch (sample_type) {
        case AUDIO_I16: launch<int16_t>(path, grid, s, samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
        case AUDIO_F32: launch<float>(path, grid, s, samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
        default: launch<double>(path, grid, s, samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target); break;
    }
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
