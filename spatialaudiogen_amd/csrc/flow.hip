// Dense optical flow on the device (gfx950): a pyramidal Horn-Schunck estimator with warping, aware of the equirectangular seam,
// and the reference's polar byte coding of a flow field - include/sagen.h: sagen_optical_flow, sagen_flow_encode; the per-pixel
// arithmetic is csrc/flow_core.h, shared with the CPU twin.  It stands in for the reference's offline FlowNet2 pass
// (scraping/preprocess.py:156-204, scraping/flow.py); it is another estimator, not that network.
//
//   flow_luma_kernel      uint8 RGB -> fp64 luma, level 0 of every frame's pyramid
//   flow_down_kernel      level l -> level l + 1 (2 x 2 means)
//   flow_smooth_kernel    the separable binomial of one level, both passes in one thread (25 loads; once per level and frame)
//   flow_upsample_kernel  the start of a level: zero on the coarsest, else twice the bilinear fetch of the coarser flow
//   flow_deriv_kernel     per warp: the second image warped at the pixel and its four neighbours, Ix, Iy, It, and a copy of the
//                         flow the warp linearises around
//   flow_jacobi_kernel<F> F Jacobi sweeps per launch (temporal blocking).  A workgroup owns a tile of 64 x 16 pixels and computes a
//                         region of (64 + 2 F) x (16 + 2 F): after sweep s the pixels at least s inside the region are exact, so
//                         after F sweeps the tile is.  Every thread keeps the coefficients (Ix, Iy, It, u0, v0) of its <= K region
//                         pixels in registers for all F sweeps; (u, v) of the region lives in LDS, which the threads read their
//                         eight neighbours from and write their new values to between two barriers.  A region pixel IS an image
//                         pixel - column (x0 + rx) mod w under wrap, so a region wider than the image just holds pixels twice - and
//                         the clamp at the image border is a neighbour OFFSET of zero, decided per pixel by its image index: no
//                         ghost cell exists that could go stale between sweeps.  A wave of 64 works on consecutive x.
//   flow_store_kernel     fp64 (u, v) -> fp32, the one rounding of the result
//   flow_minmax_kernel    per frame FLOW_ENC_PARTS partial (min, max) of the fp32 magnitude: lane butterflies of wave_reduce.h, then
//                         four waves through LDS; no atomics
//   flow_encode_kernel    every wave folds the partials (one per lane) into the frame's limits, then codes its pixels
//
// All frame pairs of a call go in one launch per step (gridDim.z = pairs or frames).
#include "kernels.h"
#include "flow_core.h"
#include <utility>

#pragma clang fp contract(off)

namespace sagen {

namespace {

constexpr int FLOW_THREADS = 256;
constexpr int JT_X = 64, JT_Y = 16;             // the tile of the Jacobi sweep
constexpr int FLOW_AUTO_FUSE = 4;               // what fuse = 0 takes: the fastest depth of profiles/flow_rate.jsonl

__global__ __launch_bounds__(FLOW_THREADS) void flow_luma_kernel(const uint8_t* __restrict__ frames, double* __restrict__ pyr, int hw,
                                                                 size_t pyr_stride) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= hw) return;
    const size_t f = blockIdx.z;
    pyr[f * pyr_stride + i] = flow_luma(frames + (f * hw + i) * 3);
}

// fine: level l (2 ch x 2 cw) at pyr + fine_off, coarse: level l + 1 (ch x cw) at pyr + coarse_off, per frame
__global__ __launch_bounds__(FLOW_THREADS) void flow_down_kernel(double* __restrict__ pyr, size_t fine_off, size_t coarse_off, int ch, int cw,
                                                                 size_t pyr_stride) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= ch * cw) return;
    const int y = i / cw, x = i - y * cw;
    double* base = pyr + (size_t)blockIdx.z * pyr_stride;
    base[coarse_off + i] = flow_down(base + fine_off, 2 * cw, x, y);
}

__global__ __launch_bounds__(FLOW_THREADS) void flow_smooth_kernel(const double* __restrict__ pyr, size_t level_off, size_t pyr_stride,
                                                                   double* __restrict__ smooth, size_t smooth_stride, int h, int w, int wrap) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    smooth[(size_t)blockIdx.z * smooth_stride + i] = flow_smooth(pyr + (size_t)blockIdx.z * pyr_stride + level_off, h, w, wrap, x, y);
}

// coarse == nullptr: the coarsest level starts at zero
__global__ __launch_bounds__(FLOW_THREADS) void flow_upsample_kernel(const FlowUV* __restrict__ coarse, FlowUV* __restrict__ fine, int h, int w,
                                                                     int wrap, size_t pair_stride) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    FlowUV r;
    r.u = 0.; r.v = 0.;
    if (coarse) r = flow_upsample(coarse + (size_t)blockIdx.z * pair_stride, h / 2, w / 2, wrap, x, y);
    fine[(size_t)blockIdx.z * pair_stride + i] = r;
}

// pair k: frames k and k + 1 of `smooth`
__global__ __launch_bounds__(FLOW_THREADS) void flow_deriv_kernel(const double* __restrict__ smooth, size_t smooth_stride,
                                                                  const FlowUV* __restrict__ flow, FlowCoef* __restrict__ coef,
                                                                  FlowUV* __restrict__ flow0, int h, int w, int wrap, size_t pair_stride) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i - y * w;
    const size_t k = blockIdx.z;
    const FlowUV* f = flow + k * pair_stride;
    coef[k * pair_stride + i] = flow_derivs(smooth + k * smooth_stride, smooth + (k + 1) * smooth_stride, f, h, w, wrap, x, y);
    flow0[k * pair_stride + i] = f[i];
}

template <int F>
__global__ __launch_bounds__(FLOW_THREADS) void flow_jacobi_kernel(const FlowCoef* __restrict__ coef, const FlowUV* __restrict__ flow0,
                                                                   const FlowUV* __restrict__ in, FlowUV* __restrict__ out, int h, int w, int wrap,
                                                                   double alpha2, size_t pair_stride) {
    constexpr int RW = JT_X + 2 * F, RH = JT_Y + 2 * F, N = RW * RH, K = (N + FLOW_THREADS - 1) / FLOW_THREADS;
    __shared__ double su[N], sv[N];
    const int x0 = blockIdx.x * JT_X - F, y0 = blockIdx.y * JT_Y - F;
    const size_t base = (size_t)blockIdx.z * pair_stride;
    FlowCoef c[K];
    FlowUV f0[K], nw[K];
    // per region pixel: bits 0-3 say which neighbour offsets are NOT zero (north, south, west, east), bits 4.. hold margin + 1, the
    // pixel's distance from the region's edge; 0: not a pixel of the image (or past the region), never computed and never read
    int meta[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int p = threadIdx.x + k * FLOW_THREADS;
        const int ry = p / RW, rx = p - ry * RW;
        const int gy = y0 + ry, gxr = x0 + rx;
        const bool live = p < N && gy >= 0 && gy < h && (wrap || (gxr >= 0 && gxr < w));
        meta[k] = 0;
        c[k].ix = c[k].iy = c[k].it = 0.;
        f0[k].u = f0[k].v = 0.;
        nw[k].u = nw[k].v = 0.;
        if (live) {
            const int gx = flow_ix(gxr, w, wrap);
            const size_t g = base + (size_t)gy * w + gx;
            c[k] = coef[g];
            f0[k] = flow0[g];
            const FlowUV f = in[g];
            su[p] = f.u;
            sv[p] = f.v;
            const int mx = rx < RW - 1 - rx ? rx : RW - 1 - rx, my = ry < RH - 1 - ry ? ry : RH - 1 - ry;
            // the neighbour rule by index: a row offset of zero on the first / last row, a column offset of zero on the first /
            // last column when the frame does not wrap
            meta[k] = (((mx < my ? mx : my) + 1) << 4) | (gy > 0 ? 1 : 0) | (gy < h - 1 ? 2 : 0) | ((wrap || gx > 0) ? 4 : 0) |
                      ((wrap || gx < w - 1) ? 8 : 0);
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 1; s <= F; ++s) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((meta[k] >> 4) > s) {             // margin >= s: its eight neighbours are >= s - 1 inside the region, exact after sweep s - 1
                const int p = threadIdx.x + k * FLOW_THREADS;
                const int pn = p - ((meta[k] & 1) ? RW : 0), ps = p + ((meta[k] & 2) ? RW : 0);
                const int dw = (meta[k] & 4) ? -1 : 0, de = (meta[k] & 8) ? 1 : 0;
                const double ub = flow_average(su[pn], su[ps], su[p + dw], su[p + de], su[pn + dw], su[pn + de], su[ps + dw], su[ps + de]);
                const double vb = flow_average(sv[pn], sv[ps], sv[p + dw], sv[p + de], sv[pn + dw], sv[pn + de], sv[ps + dw], sv[ps + de]);
                nw[k] = flow_hs_update(ub, vb, c[k], f0[k], alpha2);
            }
        }
        if (s == F) break;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if ((meta[k] >> 4) > s) {
                const int p = threadIdx.x + k * FLOW_THREADS;
                su[p] = nw[k].u;
                sv[p] = nw[k].v;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if ((meta[k] >> 4) > F) {                 // margin >= F: a pixel of the tile, exact after F sweeps
            const int p = threadIdx.x + k * FLOW_THREADS;
            const int ry = p / RW, rx = p - ry * RW;
            const int gy = y0 + ry, gxr = x0 + rx;
            if (gxr < w) out[base + (size_t)gy * w + gxr] = nw[k];      // (under wrap a tile may reach past the last column)
        }
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void flow_store_kernel(const FlowUV* __restrict__ flow, float* __restrict__ out, int hw,
                                                                  size_t pair_stride) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= hw) return;
    const FlowUV f = flow[(size_t)blockIdx.z * pair_stride + i];
    float* o = out + ((size_t)blockIdx.z * hw + i) * 2;
    o[0] = (float)f.u;
    o[1] = (float)f.v;
}

// ---- the byte coding ----------------------------------------------------------------------------------------------------------------
template <bool MAX, int M = 1>
__device__ __forceinline__ float wave_extreme(float v) {       // every lane ends with the wave's minimum / maximum
    if constexpr (M < 64) {
        int a, b;
        lane_pair<M>(__float_as_int(v), a, b);
        const float fa = __int_as_float(a), fb = __int_as_float(b);
        return wave_extreme<MAX, M * 2>(MAX ? (fa > fb ? fa : fb) : (fa < fb ? fa : fb));
    } else {
        return v;
    }
}

// grid (FLOW_ENC_PARTS, 1, n): part j of frame f -> parts[f][j] = (min, max) of its share of the magnitudes
__global__ __launch_bounds__(FLOW_THREADS) void flow_minmax_kernel(const float* __restrict__ flow, float* __restrict__ parts, int hw) {
    __shared__ float wl[FLOW_THREADS / 64], wh[FLOW_THREADS / 64];
    const float* f = flow + (size_t)blockIdx.z * hw * 2;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < hw; i += FLOW_ENC_PARTS * FLOW_THREADS) {
        const float m = flow_mag(f[2 * i], f[2 * i + 1]);
        lo = m < lo ? m : lo;
        hi = m > hi ? m : hi;
    }
    lo = wave_extreme<false>(lo);
    hi = wave_extreme<true>(hi);
    if ((threadIdx.x & 63) == 0) {
        wl[threadIdx.x >> 6] = lo;
        wh[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < FLOW_THREADS / 64; ++k) {
            lo = wl[k] < lo ? wl[k] : lo;
            hi = wh[k] > hi ? wh[k] : hi;
        }
        float* o = parts + ((size_t)blockIdx.z * FLOW_ENC_PARTS + blockIdx.x) * 2;
        o[0] = lo;
        o[1] = hi;
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void flow_encode_kernel(const float* __restrict__ flow, const float* __restrict__ parts,
                                                                   uint8_t* __restrict__ rgb, float* __restrict__ limits, int hw) {
    static_assert(FLOW_ENC_PARTS == 64, "one partial per lane");
    const float* pp = parts + ((size_t)blockIdx.z * FLOW_ENC_PARTS + (threadIdx.x & 63)) * 2;
    float lim[2];
    flow_limits(wave_extreme<false>(pp[0]), wave_extreme<true>(pp[1]), lim);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        limits[(size_t)blockIdx.z * 2] = lim[0];
        limits[(size_t)blockIdx.z * 2 + 1] = lim[1];
    }
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= hw) return;
    const size_t g = (size_t)blockIdx.z * hw + i;
    uint8_t b[3];
    flow_bytes(flow[2 * g], flow[2 * g + 1], lim[0], lim[1], b);
    rgb[3 * g] = b[0];
    rgb[3 * g + 1] = b[1];
    rgb[3 * g + 2] = b[2];
}

template <int F>
void jacobi_launch(const FlowCoef* coef, const FlowUV* f0, const FlowUV* in, FlowUV* out, int h, int w, int pairs, const FlowArgs& a,
                   size_t pair_stride, hipStream_t s) {
    hipLaunchKernelGGL(flow_jacobi_kernel<F>, dim3(cdiv(w, JT_X), cdiv(h, JT_Y), pairs), dim3(FLOW_THREADS), 0, s, coef, f0, in, out, h, w, a.wrap,
                       a.alpha2, pair_stride);
}

void jacobi_dispatch(int depth, const FlowCoef* coef, const FlowUV* f0, const FlowUV* in, FlowUV* out, int h, int w, int pairs,
                     const FlowArgs& a, size_t pair_stride, hipStream_t s) {
    switch (depth) {
        case 1: jacobi_launch<1>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 2: jacobi_launch<2>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 3: jacobi_launch<3>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 4: jacobi_launch<4>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 5: jacobi_launch<5>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 6: jacobi_launch<6>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        case 7: jacobi_launch<7>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
        default: jacobi_launch<8>(coef, f0, in, out, h, w, pairs, a, pair_stride, s); break;
    }
}

}  // namespace

int flow_auto_fuse() { return FLOW_AUTO_FUSE; }

int run_optical_flow(const uint8_t* frames, const FlowArgs& a, float* flow, void* scratch, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const int n = a.n_frames, pairs = n - 1, hw = a.h * a.w;
    const size_t pair_stride = (size_t)hw, pyr_stride = flow_level_pixels(a.h, a.w, a.levels), smooth_stride = (size_t)hw;
    // the (u, v) fields first: they are read and written in 16-byte pieces
    FlowUV* cur = (FlowUV*)scratch;
    FlowUV* oth = cur + pairs * pair_stride;
    FlowUV* flow0 = oth + pairs * pair_stride;
    FlowCoef* coef = (FlowCoef*)(flow0 + pairs * pair_stride);
    double* pyr = (double*)(coef + pairs * pair_stride);
    double* smooth = pyr + (size_t)n * pyr_stride;
    size_t off[FLOW_MAX_LEVELS];
    off[0] = 0;
    for (int l = 1; l < a.levels; ++l) off[l] = off[l - 1] + (size_t)(a.h >> (l - 1)) * (a.w >> (l - 1));

    hipLaunchKernelGGL(flow_luma_kernel, dim3(cdiv(hw, FLOW_THREADS), 1, n), dim3(FLOW_THREADS), 0, s, frames, pyr, hw, pyr_stride);
    SAGEN_LAUNCH_CHECK();
    for (int l = 1; l < a.levels; ++l) {
        const int ch = a.h >> l, cw = a.w >> l;
        hipLaunchKernelGGL(flow_down_kernel, dim3(cdiv(ch * cw, FLOW_THREADS), 1, n), dim3(FLOW_THREADS), 0, s, pyr, off[l - 1], off[l], ch, cw,
                           pyr_stride);
        SAGEN_LAUNCH_CHECK();
    }
    const int depth = a.fuse > 0 ? a.fuse : FLOW_AUTO_FUSE;
    for (int l = a.levels - 1; l >= 0; --l) {
        const int h = a.h >> l, w = a.w >> l;
        const dim3 pix(cdiv(h * w, FLOW_THREADS), 1, pairs);
        hipLaunchKernelGGL(flow_smooth_kernel, dim3(cdiv(h * w, FLOW_THREADS), 1, n), dim3(FLOW_THREADS), 0, s, pyr, off[l], pyr_stride, smooth,
                           smooth_stride, h, w, a.wrap);
        SAGEN_LAUNCH_CHECK();
        hipLaunchKernelGGL(flow_upsample_kernel, pix, dim3(FLOW_THREADS), 0, s, l == a.levels - 1 ? (const FlowUV*)nullptr : cur, oth, h, w, a.wrap,
                           pair_stride);
        SAGEN_LAUNCH_CHECK();
        std::swap(cur, oth);
        for (int wp = 0; wp < a.warps; ++wp) {
            hipLaunchKernelGGL(flow_deriv_kernel, pix, dim3(FLOW_THREADS), 0, s, smooth, smooth_stride, cur, coef, flow0, h, w, a.wrap, pair_stride);
            SAGEN_LAUNCH_CHECK();
            for (int it = 0; it < a.iters; it += depth) {
                jacobi_dispatch(a.iters - it < depth ? a.iters - it : depth, coef, flow0, cur, oth, h, w, pairs, a, pair_stride, s);
                SAGEN_LAUNCH_CHECK();
                std::swap(cur, oth);
            }
        }
    }
    hipLaunchKernelGGL(flow_store_kernel, dim3(cdiv(hw, FLOW_THREADS), 1, pairs), dim3(FLOW_THREADS), 0, s, cur, flow, hw, pair_stride);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_flow_encode(const float* flow, int n, int h, int w, uint8_t* rgb, float* limits, void* scratch, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const int hw = h * w;
    float* parts = (float*)scratch;
    hipLaunchKernelGGL(flow_minmax_kernel, dim3(FLOW_ENC_PARTS, 1, n), dim3(FLOW_THREADS), 0, s, flow, parts, hw);
    SAGEN_LAUNCH_CHECK();
    hipLaunchKernelGGL(flow_encode_kernel, dim3(cdiv(hw, FLOW_THREADS), 1, n), dim3(FLOW_THREADS), 0, s, flow, parts, rgb, limits, hw);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
