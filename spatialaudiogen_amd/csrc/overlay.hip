// The sound-direction heat map painted over the 360-degree frames (gfx950): the visual half of the reference's output stage,
// myutils.gen_360video(overlay_map=True) (myutils.py:246-279) over SphericalAmbisonicsVisualizer (pyutils/ambisonics/
// distance.py:16-59) - see include/sagen.h for the contract.
//
//   sagen_power_map_windows   rms[m][p] = sqrt(mean_k (ambi[(m window + k) stride] . sh[p])^2), 4 or 9 channels.  As in
//                             elementwise.hip the audio is read ONCE whatever the mesh size: one workgroup per window takes the
//                             C (C + 1) / 2 second moments (fp64 partials per thread, combined over the wave and the four waves in
//                             a fixed order: no atomics), then every (window, node) evaluates y^T S y in fp64.  The partials are
//                             fp64 because y^T S y CANCELS where a node's projection nearly vanishes (the null of a plane wave; any
//                             node of a one-sample window): products rounded to fp32 leave sqrt(2^-24) of the map's maximum there
//                             (measured 1.6e-5 at window = 1, over the 1e-5 bar), while the product of two fp32 values is exact in
//                             fp64.  The pass stays bound by its reads: 45 fp64 FMAs per 36-byte row.
//   sagen_overlay_blend       per frame a GRID pass (one workgroup: min / max of the two maps, normalise, interpolate, colour
//                             index, table look-up, the four clip bounds -> scratch [node][r, g, b, v] fp64) and a PIXEL pass (a
//                             workgroup per 512 pixels of one output row: the two grid rows the row touches are staged in LDS with
//                             a zero column either side, a thread finishes 4 pixels = 12 bytes: bilinear taps, clip, blend, store).
//
// All of the blend is fp64 in exactly the operation order of the header: the uint8 truncation and the int(v * 255) colour index
// turn a last-bit difference into a wrong pixel.  Hence no contraction anywhere in this file (a * b + c stays two roundings);
// the moment partials ask for their fused multiply-add by name.
#include "kernels.h"
#include "wave_reduce.h"

#pragma clang fp contract(off)

namespace sagen {

namespace {

// ---- power maps of a strided stream ------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void overlay_moments_kernel(const float* __restrict__ ambi, int stride, long long window,
                                                              double* __restrict__ S) {
    constexpr int M = C * (C + 1) / 2;
    const long long first = (long long)blockIdx.x * window;        // decimated index of the window's first sample
    double acc[M];
#pragma unroll
    for (int q = 0; q < M; ++q) acc[q] = 0.0;
    for (long long k = threadIdx.x; k < window; k += 256) {
        const long long row = (first + k) * stride;                // < n_rows: n_maps windows fit into ceil(n_rows / stride) samples
        double a[C];
        if (C == 4) {
            const float4 t = *(const float4*)(ambi + row * 4);
            a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
        } else {                                                   // 36-byte rows: no 16-byte alignment to rely on
#pragma unroll
            for (int c = 0; c < C; ++c) a[c] = (double)ambi[row * C + c];
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
            for (int j = i; j < C; ++j, ++q) acc[q] = fma(a[i], a[j], acc[q]);
    }
    __shared__ double red[4][M];
#pragma unroll
    for (int q = 0; q < M; ++q) {
        const double v = wave_sum_f64(acc[q]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < M) S[(long long)blockIdx.x * M + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

template <int C>
__global__ __launch_bounds__(256) void overlay_map_kernel(const double* __restrict__ Sall, double window, const float* __restrict__ sh, int P,
                                                          int p_blocks, float* __restrict__ rms) {
    constexpr int M = C * (C + 1) / 2;
    const int m = blockIdx.x / p_blocks;
    const int p = (blockIdx.x % p_blocks) * 256 + threadIdx.x;
    if (p >= P) return;
    const double* S = Sall + (long long)m * M;
    double y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = (double)sh[(long long)p * C + c];
    double e = 0.0;
    int q = 0;
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int j = i; j < C; ++j, ++q) {
            const double t = y[i] * S[q] * y[j];
            e += i == j ? t : 2.0 * t;
        }
    rms[(long long)m * P + p] = (float)sqrt(fmax(e, 0.0) / window);
}

// ---- blend ----------------------------------------------------------------------------------------------------------------------
struct BlendArgs {
    long long map0, frame0;
    int mh, mw, h, w, fpm, vec;
    double sy, sx;                 // mh / h, mw / w
};

// every thread of the 256 returns the maximum of `v` over the workgroup (an exact operation: the order does not matter)
__device__ __forceinline__ double block_max_f64(double v, double* red4) {
    v = wave_max_f64(v);
    __syncthreads();               // (red4 may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red4[0], red4[1]), fmax(red4[2], red4[3]));
}

// grid [n_frames][mh mw][4] = (r, g, b, v) of every node, bounds [n_frames][4] = (lo, hi) of the colours and of v
__global__ __launch_bounds__(256) void overlay_grid_kernel(const float* __restrict__ maps, const double* __restrict__ lut,
                                                           double* __restrict__ grid, double* __restrict__ bounds, const BlendArgs a) {
    __shared__ double red4[4];
    const int f = blockIdx.x, N = a.mh * a.mw;
    const long long F = a.frame0 + f, prev = F / a.fpm;
    const double beta = (double)(F % a.fpm) / (double)a.fpm;
    const float* mp = maps + (prev - a.map0) * N;
    const float* mc = mp + N;
    float pl = INFINITY, ph = -INFINITY, cl = INFINITY, ch = -INFINITY;
    for (int n = threadIdx.x; n < N; n += 256) {
        const float u = mp[n], v = mc[n];
        pl = fminf(pl, u); ph = fmaxf(ph, u);
        cl = fminf(cl, v); ch = fmaxf(ch, v);
    }
    const double pmin = -block_max_f64(-(double)pl, red4), pmax = block_max_f64((double)ph, red4);
    const double cmin = -block_max_f64(-(double)cl, red4), cmax = block_max_f64((double)ch, red4);
    const double pden = (pmax - pmin) + 0.005, cden = (cmax - cmin) + 0.005;
    double klo = INFINITY, khi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
    double* g = grid + (long long)f * N * 4;
    for (int n = threadIdx.x; n < N; n += 256) {
        const double u = ((double)mp[n] - pmin) / pden, c = ((double)mc[n] - cmin) / cden;
        double v = (1.0 - beta) * u + beta * c;
        v = v * 2.0 - 0.7;
        if (v < 0.0) v = 0.0;
        int idx = (int)(v * 255.0);
        if (idx > 255) idx = 255;
        const double r = lut[idx * 3], gg = lut[idx * 3 + 1], b = lut[idx * 3 + 2];
        *(double2*)(g + (long long)n * 4) = make_double2(r, gg);
        *(double2*)(g + (long long)n * 4 + 2) = make_double2(b, v);
        klo = fmin(klo, fmin(r, fmin(gg, b))); khi = fmax(khi, fmax(r, fmax(gg, b)));
        vlo = fmin(vlo, v); vhi = fmax(vhi, v);
    }
    klo = -block_max_f64(-klo, red4); khi = block_max_f64(khi, red4);
    vlo = -block_max_f64(-vlo, red4); vhi = block_max_f64(vhi, red4);
    if (threadIdx.x == 0) {
        double* bo = bounds + (long long)f * 4;
        bo[0] = klo; bo[1] = khi; bo[2] = vlo; bo[3] = vhi;
    }
}

// resize()'s clip: into [lo, hi] of the resized array; an array that does not contain 0 keeps the exact zeros of the constant border
__device__ __forceinline__ double clip_resized(double v, double lo, double hi, bool spans_zero) {
    if (!spans_zero && v == 0.0) return 0.0;
    return fmin(fmax(v, lo), hi);
}

constexpr int PIX_THREADS = 128;
constexpr int PIX_PER_THREAD = 4;
constexpr int PIX_PER_BLOCK = PIX_THREADS * PIX_PER_THREAD;
// output rows per workgroup.  Four rows (100 VGPRs, 19 KB of LDS at 72 columns) were built and were not faster than one: the pass is
// bound by its fp64 instructions, and what four rows save in staging and column coordinates they lose in resident waves
constexpr int PIX_ROWS = 1;
static_assert(PIX_ROWS * 2 * 1002 * 4 * sizeof(double) <= 65536, "the staged rows of the widest map (1000 columns) must fit 64 KB of LDS");

// A workgroup finishes R consecutive output rows x 512 pixels of one frame.  The frame bytes of its rows are requested first,
// so that their latency runs under the staging; the column coordinates of a thread's 4 pixels serve all R rows.
template <int R>
__global__ __launch_bounds__(PIX_THREADS) void overlay_pixel_kernel(const double* __restrict__ grid, const double* __restrict__ bounds,
                                                                     const uint8_t* __restrict__ frames, uint8_t* __restrict__ out,
                                                                     const BlendArgs a) {
    extern __shared__ double2 overlay_lds2[];    // [R][2 rows][mw + 2 columns][2 double2]: column j of the map at slot j + 1
    const int yb = blockIdx.y * R, f = blockIdx.z, cols = a.mw + 2;
    const int x0 = (blockIdx.x * PIX_THREADS + threadIdx.x) * PIX_PER_THREAD;
    const bool live = x0 < a.w;
    const int npx = a.w - x0 < PIX_PER_THREAD ? a.w - x0 : PIX_PER_THREAD;
    uint8_t px[R][PIX_PER_THREAD * 3];
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        if (!live || yb + rr >= a.h) continue;
        const long long off = (((long long)f * a.h + yb + rr) * a.w + x0) * 3;
        if (a.vec) {                                             // w % 4 == 0 and 4-byte aligned bases: the 12 bytes are three aligned words
            const uint32_t* p = (const uint32_t*)(frames + off);
            const uint32_t u0 = p[0], u1 = p[1], u2 = p[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                px[rr][i] = (uint8_t)(u0 >> (8 * i)); px[rr][4 + i] = (uint8_t)(u1 >> (8 * i)); px[rr][8 + i] = (uint8_t)(u2 >> (8 * i));
            }
        } else {
#pragma unroll
            for (int i = 0; i < PIX_PER_THREAD * 3; ++i) px[rr][i] = i < npx * 3 ? frames[off + i] : (uint8_t)0;
        }
    }
    const double2* g2 = (const double2*)(grid + (long long)f * a.mh * a.mw * 4);
    for (int i = threadIdx.x; i < 2 * R * cols; i += PIX_THREADS) {
        const int rr = i / (2 * cols), k = i - rr * 2 * cols;
        const double r = ((double)(yb + rr) + 0.5) * a.sy - 0.5;   // (a row past the frame's end stages rows nobody reads)
        const int row = (int)(k < cols ? floor(r) : ceil(r)), j = (k < cols ? k : k - cols) - 1;
        double2 lo = make_double2(0.0, 0.0), hi = lo;            // outside the map: 0 (mode = 'constant', cval = 0)
        if (row >= 0 && row < a.mh && j >= 0 && j < a.mw) {
            lo = g2[((long long)row * a.mw + j) * 2];
            hi = g2[((long long)row * a.mw + j) * 2 + 1];
        }
        overlay_lds2[i * 2] = lo;
        overlay_lds2[i * 2 + 1] = hi;
    }
    const double* bo = bounds + (long long)f * 4;
    const double klo = bo[0], khi = bo[1], vlo = bo[2], vhi = bo[3];
    const bool kz = klo <= 0.0 && 0.0 <= khi, vz = vlo <= 0.0 && 0.0 <= vhi;
    double dc[PIX_PER_THREAD];
    int j0[PIX_PER_THREAD], j1[PIX_PER_THREAD];
#pragma unroll
    for (int i = 0; i < PIX_PER_THREAD; ++i) {
        const int x = x0 + i;                                    // (past the row's end the last column stands in: the slots stay inside the staged columns)
        const double c = ((double)(x < a.w ? x : a.w - 1) + 0.5) * a.sx - 0.5;
        const double c0 = floor(c), c1 = ceil(c);
        dc[i] = c - c0;
        j0[i] = ((int)c0 + 1) * 4;
        j1[i] = ((int)c1 + 1) * 4;
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int y = yb + rr;
        if (y >= a.h) break;
        const double r = ((double)y + 0.5) * a.sy - 0.5;
        const double dr = r - floor(r);
        const double* row0 = (const double*)overlay_lds2 + (long long)rr * 2 * cols * 4;
        const double* row1 = row0 + (long long)cols * 4;
#pragma unroll
        for (int i = 0; i < PIX_PER_THREAD; ++i) {
            double val[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double top = (1.0 - dc[i]) * row0[j0[i] + k] + dc[i] * row0[j1[i] + k];
                const double bot = (1.0 - dc[i]) * row1[j0[i] + k] + dc[i] * row1[j1[i] + k];
                val[k] = (1.0 - dr) * top + dr * bot;
            }
            const double alpha = clip_resized(val[3], vlo, vhi, vz) * 0.6;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double dir = clip_resized(val[k], klo, khi, kz) * 255.0;
                const double o = alpha * dir + (1.0 - alpha) * (double)px[rr][i * 3 + k];
                px[rr][i * 3 + k] = (uint8_t)(int)o;
            }
        }
        const long long off = (((long long)f * a.h + y) * a.w + x0) * 3;
        if (a.vec) {
            uint32_t u[3];
#pragma unroll
            for (int wd = 0; wd < 3; ++wd)
                u[wd] = (uint32_t)px[rr][4 * wd] | (uint32_t)px[rr][4 * wd + 1] << 8 | (uint32_t)px[rr][4 * wd + 2] << 16 | (uint32_t)px[rr][4 * wd + 3] << 24;
            uint32_t* p = (uint32_t*)(out + off);
            p[0] = u[0]; p[1] = u[1]; p[2] = u[2];
        } else {
#pragma unroll
            for (int i = 0; i < PIX_PER_THREAD * 3; ++i)
                if (i < npx * 3) out[off + i] = px[rr][i];
        }
    }
}

}  // namespace

int run_power_map_windows(const float* ambi, int channels, int stride, int64_t window, int n_maps, const float* sh, int P, float* rms,
                          double* moments, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const int p_blocks = cdiv(P, 256);
    if (channels == 4) {
        hipLaunchKernelGGL(overlay_moments_kernel<4>, dim3(n_maps), dim3(256), 0, s, ambi, stride, window, moments);
        SAGEN_LAUNCH_CHECK();
        hipLaunchKernelGGL(overlay_map_kernel<4>, dim3(n_maps * p_blocks), dim3(256), 0, s, moments, (double)window, sh, P, p_blocks, rms);
    } else {
        hipLaunchKernelGGL(overlay_moments_kernel<9>, dim3(n_maps), dim3(256), 0, s, ambi, stride, window, moments);
        SAGEN_LAUNCH_CHECK();
        hipLaunchKernelGGL(overlay_map_kernel<9>, dim3(n_maps * p_blocks), dim3(256), 0, s, moments, (double)window, sh, P, p_blocks, rms);
    }
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_overlay_blend(const float* maps, int64_t map0, int mh, int mw, const double* lut, const uint8_t* frames, int n_frames,
                      int64_t frame0, int h, int w, int frames_per_map, uint8_t* out, void* scratch, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    BlendArgs a;
    a.map0 = map0; a.frame0 = frame0; a.mh = mh; a.mw = mw; a.h = h; a.w = w; a.fpm = frames_per_map;
    a.vec = w % 4 == 0 && ((uintptr_t)frames) % 4 == 0 && ((uintptr_t)out) % 4 == 0;
    a.sy = (double)mh / (double)h;
    a.sx = (double)mw / (double)w;
    double* grid = (double*)scratch;
    double* bounds = (double*)((char*)scratch + overlay_blend_grid_bytes(mh, mw, n_frames));
    hipLaunchKernelGGL(overlay_grid_kernel, dim3(n_frames), dim3(256), 0, s, maps, lut, grid, bounds, a);
    SAGEN_LAUNCH_CHECK();
    const size_t row_pair = (size_t)2 * (mw + 2) * 4 * sizeof(double);  // <= 2 * 1002 * 32 = 64 128 bytes
    hipLaunchKernelGGL(overlay_pixel_kernel<PIX_ROWS>, dim3(cdiv(w, PIX_PER_BLOCK), cdiv(h, PIX_ROWS), n_frames), dim3(PIX_THREADS),
                       PIX_ROWS * row_pair, s, grid, bounds, frames, out, a);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
