// Rational polyphase FIR resampling and windowed RMS (gfx950): sagen_resample_fir / sagen_window_rms of include/sagen.h - in place
// of resampy's 'kaiser_fast' in load_wav (pyutils/iolib/audio.py:23), ffmpeg's `-ar 48000` + `pan` remap (scraping/preprocess.py:
// 14-34), AmbisonicArray.convert (pyutils/ambisonics/common.py:34-59) and compute_audio_pow (scraping/preprocess.py:146-153).  The
// arithmetic is resample_core.h's, shared with the CPU twin.
//
//   y[n][o] = sum_m h[n M - m L] z[m][o],   z[m][o] = sum_c mix[o][c] x[m][c]
//
// A workgroup owns `nt` consecutive outputs of `cg` output channels (blockIdx.y walks the channel groups).  The input rows that run
// reaches - from m0(first output) to m0(last output) + T - 1 - are staged ONCE in LDS as fp64, already mixed: z, not x, so that the
// contraction reads one double per tap whatever C_in is, and the rows outside the buffer are staged as zeros, so that the contraction
// has no bounds of its own.  One work item = (output, channel of the group): T multiply-adds in one fp64 accumulator, t ascending,
// the taps of phase (n M) mod L read as one contiguous row of the table (consecutive outputs stride through the table by M rows;
// a row is what one item walks, so every cache line it fetches is used to the end).  The launcher sizes the tile so that the staged
// rows fit RS_LDS_DOUBLES.
//
// BOUNDS.  x is read only at rows 0 <= r < n_in, y written only at rows < n, the table read at p < L, t < T.  The LDS slot of
// (item, t) is (m0(n) - m0(first) + t) * cg + channel < rows * cg: m0 is monotone in n, and an item whose rows would not lie inside
// the staged run is skipped (the launcher's tile makes that impossible; the test is the kernel's own guarantee).
#include "kernels.h"
#include "resample_core.h"

namespace sagen {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_DOUBLES = 6144;          // 48 KiB of staged rows
constexpr int RS_MAX_TILE = 512;              // outputs per workgroup
constexpr int RS_MAX_GROUP = 8;               // output channels per workgroup

__global__ __launch_bounds__(RS_THREADS) void resample_fir_kernel(const float* __restrict__ x,        // [n_in][c_in]
                                                                  const double* __restrict__ taps,    // [L][T]
                                                                  const double* __restrict__ mix,     // [c_out][c_in] or null
                                                                  float* __restrict__ y,              // [n][c_out]
                                                                  const ResampleArgs a, const int tile, const int group, const int cap) {
    extern __shared__ double rs_lds[];
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * tile;                  // of the tile, among the n outputs
    if (t0 >= a.n) return;
    const int nt = (int)(a.n - t0 < tile ? a.n - t0 : tile);
    const int o0 = blockIdx.y * group;
    if (o0 >= a.c_out) return;
    const int cg = a.c_out - o0 < group ? a.c_out - o0 : group;
    const long long rbase = rs_first_row(a.n0 + t0, a.L, a.M, a.H);
    long long want = rs_first_row(a.n0 + t0 + nt - 1, a.L, a.M, a.H) - rbase + a.T;
    const int rows = (int)(want < cap / cg ? want : cap / cg);          // (want <= cap / group by the launcher's choice of tile)

    // ---- stage: slot row * cg + c holds z[rbase + row][o0 + c]; zero where the buffer has no such row
    for (int i = tid; i < rows * cg; i += RS_THREADS) {
        const int row = i / cg, c = i - row * cg;
        const long long r = rbase + row - a.x0;
        double v = 0.;
        if (r >= 0 && r < a.n_in) v = rs_mix_row(x, r, a.c_in, mix, o0 + c);
        rs_lds[i] = v;
    }
    __syncthreads();

    // ---- contract
    for (int item = tid; item < nt * cg; item += RS_THREADS) {
        const int j = item / cg, c = item - j * cg;
        const long long n = a.n0 + t0 + j;
        const long long off = rs_first_row(n, a.L, a.M, a.H) - rbase;
        if (off < 0 || off + a.T > rows) continue;
        const double acc = rs_dot(taps + (long long)rs_phase(n, a.L, a.M) * a.T, rs_lds + off * cg + c, cg, a.T);
        y[(t0 + j) * a.c_out + o0 + c] = (float)acc;
    }
}

// one wave per window: 64 partial sums in the fixed order of rms_partial, the butterfly of wave_sum_f64, the root of the mean
__global__ __launch_bounds__(RS_THREADS) void window_rms_kernel(const float* __restrict__ x, int channels, int channel, long long first,
                                                                long long hop, long long length, long long count, double* __restrict__ rms) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (RS_THREADS / 64) + wave;
    if (w >= count) return;                                              // (wave-uniform)
    const double s = wave_sum_f64(rms_partial(x, first + w * hop, channels, channel, length, lane));
    if (lane == 0) rms[w] = sqrt(s / (double)length);
}

}  // namespace

int run_resample_fir(const float* x, const double* taps, const double* mix, float* y, const ResampleArgs& a, const char** why, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    // the widest channel group whose staged run leaves room for at least 16 outputs' worth of rows, then the longest tile that fits
    int group = a.c_out < RS_MAX_GROUP ? a.c_out : RS_MAX_GROUP;
    while (group > 1 && (long long)(a.T + 16) * group > RS_LDS_DOUBLES) group = (group + 1) / 2;
    const long long cap_rows = RS_LDS_DOUBLES / group;                   // >= T: T <= 4096 < 6144
    long long tile = (cap_rows - a.T) * a.L / a.M + 1;                   // ceil((tile - 1) M / L) + T <= cap_rows
    if (tile > RS_MAX_TILE) tile = RS_MAX_TILE;
    const long long blocks = (a.n + tile - 1) / tile;
    if (blocks > 0x7fffffffll) {
        *why = "n needs more than 2^31 - 1 workgroups";
        return SAGEN_ERR_UNSUPPORTED;
    }
    const long long rows = (tile - 1) * a.M / a.L + 1 + a.T;             // an upper bound of what a tile stages
    const size_t lds = (size_t)(rows < cap_rows ? rows : cap_rows) * group * sizeof(double);
    const dim3 grid((unsigned)blocks, (unsigned)cdiv(a.c_out, group));
    hipLaunchKernelGGL(resample_fir_kernel, grid, dim3(RS_THREADS), lds, s, x, taps, mix, y, a, (int)tile, group, (int)(lds / sizeof(double)));
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_window_rms(const float* x, int channels, int channel, int64_t first, int64_t hop, int64_t length, int64_t count, double* rms,
                   void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(count, RS_THREADS / 64));
    hipLaunchKernelGGL(window_rms_kernel, grid, dim3(RS_THREADS), 0, s, x, channels, channel, first, hop, length, count, rms);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
