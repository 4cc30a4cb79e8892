// Dense optical flow between consecutive frames (include/sagen.h: sagen_optical_flow, sagen_flow_encode): the per-pixel arithmetic
// of a pyramidal Horn-Schunck estimator with warping, and of the polar byte coding the reference stores its flow in
// (scraping/preprocess.py:183-196).  The reference computes the flow itself offline with FlowNet2 under caffe (scraping/flow.py);
// this is a classical estimator of our own, not a port of that network.
//
// The same code runs on the device (flow.hip) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).  Everything up to the last
// rounding of the flow to fp32 is fp64; it is compiled WITHOUT contraction so that both builds round alike.
//
// Neighbour and fetch rule, used by every function here: a row index is clamped into [0, h - 1]; a column index wraps modulo w
// when wrap = 1 (an equirectangular frame closes on itself in x) and is clamped into [0, w - 1] when wrap = 0.  A bilinear fetch
// at (fx, fy) takes floor() of each coordinate and applies the rule to each of its four taps, which is the same as clamping the
// coordinate where the rule clamps.  Coordinates are held within +-2^20 before floor(), far outside anything a frame of <= 4096
// pixels can ask for, so that the conversion to an index is defined whatever the flow holds.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define FLOW_FN __host__ __device__ __forceinline__
#else
#define FLOW_FN inline
#endif
#if defined(__clang__)
#define FLOW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FLOW_NO_CONTRACT                       // g++ has no such pragma: the twin's build line passes -ffp-contract=off
#endif

namespace sagen {

constexpr int FLOW_MAX_DIM = 4096;
constexpr int FLOW_MAX_FRAMES = 65535;
constexpr int FLOW_MAX_LEVELS = 8;
constexpr int FLOW_MAX_WARPS = 16;
constexpr int FLOW_MAX_ITERS = 1000;
constexpr int FLOW_MAX_FUSE = 8;
constexpr int FLOW_MIN_COARSEST = 4;
constexpr int FLOW_ENC_PARTS = 64;             // partial (min, max) pairs per frame of the coding: one per lane of a wave
constexpr double FLOW_PI = 3.14159265358979323846;

struct FlowUV {
    double u, v;                               // pixels to the right, pixels down
};

// What a checked call works with, by value in the kernel arguments.
struct FlowArgs {
    int n_frames, h, w;                        // level 0
    int levels, warps, iters, wrap, fuse;
    double alpha2;                             // alpha^2, in (0..255 levels)^2
};

FLOW_FN int flow_iy(int y, int h) { return y < 0 ? 0 : (y > h - 1 ? h - 1 : y); }

FLOW_FN int flow_ix(int x, int w, int wrap) {
    if (wrap) {
        const int m = x % w;
        return m < 0 ? m + w : m;
    }
    return x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
}

FLOW_FN double flow_luma(const uint8_t* rgb) {
    FLOW_NO_CONTRACT
    return 0.299 * (double)rgb[0] + 0.587 * (double)rgb[1] + 0.114 * (double)rgb[2];
}

// pixel (x, y) of the next coarser level: the mean of a 2 x 2 block of `fine`, whose rows hold fw values
FLOW_FN double flow_down(const double* fine, int fw, int x, int y) {
    FLOW_NO_CONTRACT
    const double* p = fine + (size_t)(2 * y) * fw + 2 * x;
    return 0.25 * ((p[0] + p[1]) + (p[fw] + p[fw + 1]));
}

// one row of the binomial [1 4 6 4 1] / 16 at column x
FLOW_FN double flow_smooth_row(const double* row, int w, int wrap, int x) {
    FLOW_NO_CONTRACT
    const double a = row[flow_ix(x - 2, w, wrap)], b = row[flow_ix(x - 1, w, wrap)], c = row[x], d = row[flow_ix(x + 1, w, wrap)],
                 e = row[flow_ix(x + 2, w, wrap)];
    return ((a + e) + 4. * (b + d) + 6. * c) / 16.;
}

// the separable binomial, rows first: the five row results of rows y - 2 .. y + 2, then the same weights down the column
FLOW_FN double flow_smooth(const double* img, int h, int w, int wrap, int x, int y) {
    FLOW_NO_CONTRACT
    const double a = flow_smooth_row(img + (size_t)flow_iy(y - 2, h) * w, w, wrap, x);
    const double b = flow_smooth_row(img + (size_t)flow_iy(y - 1, h) * w, w, wrap, x);
    const double c = flow_smooth_row(img + (size_t)y * w, w, wrap, x);
    const double d = flow_smooth_row(img + (size_t)flow_iy(y + 1, h) * w, w, wrap, x);
    const double e = flow_smooth_row(img + (size_t)flow_iy(y + 2, h) * w, w, wrap, x);
    return ((a + e) + 4. * (b + d) + 6. * c) / 16.;
}

FLOW_FN double flow_hold(double c) {
    const double lim = 1048576.;
    return !(c >= -lim) ? -lim : (c > lim ? lim : c);      // a NaN lands on the lower limit
}

// taps and weights of a bilinear fetch at (fx, fy)
struct FlowTaps {
    int x0, x1, y0, y1;
    double ax, ay;
};

FLOW_FN FlowTaps flow_taps(int h, int w, int wrap, double fx, double fy) {
    FLOW_NO_CONTRACT
    FlowTaps t;
    fx = flow_hold(fx);
    fy = flow_hold(fy);
    const double bx = floor(fx), by = floor(fy);
    t.ax = fx - bx;
    t.ay = fy - by;
    const int ix = (int)bx, iy = (int)by;
    t.x0 = flow_ix(ix, w, wrap);
    t.x1 = flow_ix(ix + 1, w, wrap);
    t.y0 = flow_iy(iy, h);
    t.y1 = flow_iy(iy + 1, h);
    return t;
}

FLOW_FN double flow_blend(const FlowTaps& t, double v00, double v01, double v10, double v11) {
    FLOW_NO_CONTRACT
    const double top = (1. - t.ax) * v00 + t.ax * v01, bot = (1. - t.ax) * v10 + t.ax * v11;
    return (1. - t.ay) * top + t.ay * bot;
}

FLOW_FN double flow_bilinear(const double* img, int h, int w, int wrap, double fx, double fy) {
    const FlowTaps t = flow_taps(h, w, wrap, fx, fy);
    const double* r0 = img + (size_t)t.y0 * w;
    const double* r1 = img + (size_t)t.y1 * w;
    return flow_blend(t, r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1]);
}

// the start of a finer level: twice the coarser flow (ch x cw) at the fine pixel's centre, (x + 0.5) / 2 - 0.5
FLOW_FN FlowUV flow_upsample(const FlowUV* coarse, int ch, int cw, int wrap, int x, int y) {
    FLOW_NO_CONTRACT
    const FlowTaps t = flow_taps(ch, cw, wrap, ((double)x + 0.5) / 2. - 0.5, ((double)y + 0.5) / 2. - 0.5);
    const FlowUV a = coarse[(size_t)t.y0 * cw + t.x0], b = coarse[(size_t)t.y0 * cw + t.x1], c = coarse[(size_t)t.y1 * cw + t.x0],
                 d = coarse[(size_t)t.y1 * cw + t.x1];
    FlowUV r;
    r.u = 2. * flow_blend(t, a.u, b.u, c.u, d.u);
    r.v = 2. * flow_blend(t, a.v, b.v, c.v, d.v);
    return r;
}

// the second image, warped by the flow, at pixel (x, y): I2w = I2(x + u0, y + v0)
FLOW_FN double flow_warped(const double* s2, const FlowUV* flow, int h, int w, int wrap, int x, int y) {
    FLOW_NO_CONTRACT
    const FlowUV f = flow[(size_t)y * w + x];
    return flow_bilinear(s2, h, w, wrap, (double)x + f.u, (double)y + f.v);
}

// what one warp linearises around, per pixel: the derivatives of both images averaged, and the residual
struct FlowCoef {
    double ix, iy, it;
};

FLOW_FN FlowCoef flow_derivs(const double* s1, const double* s2, const FlowUV* flow, int h, int w, int wrap, int x, int y) {
    FLOW_NO_CONTRACT
    const int xl = flow_ix(x - 1, w, wrap), xr = flow_ix(x + 1, w, wrap), yu = flow_iy(y - 1, h), yd = flow_iy(y + 1, h);
    const double wl = flow_warped(s2, flow, h, w, wrap, xl, y), wr = flow_warped(s2, flow, h, w, wrap, xr, y);
    const double wu = flow_warped(s2, flow, h, w, wrap, x, yu), wd = flow_warped(s2, flow, h, w, wrap, x, yd);
    const double wc = flow_warped(s2, flow, h, w, wrap, x, y);
    const double* r = s1 + (size_t)y * w;
    FlowCoef c;
    c.ix = ((wr - wl) + (r[xr] - r[xl])) / 4.;
    c.iy = ((wd - wu) + (s1[(size_t)yd * w + x] - s1[(size_t)yu * w + x])) / 4.;
    c.it = wc - r[x];
    return c;
}

// the Horn-Schunck average: edge neighbours at 1/6, diagonal neighbours at 1/12
FLOW_FN double flow_average(double n, double s, double wst, double e, double nw, double ne, double sw, double se) {
    FLOW_NO_CONTRACT
    return ((n + s) + (wst + e)) / 6. + ((nw + ne) + (sw + se)) / 12.;
}

// ONE Jacobi update of a pixel from the averages of the previous iterate: the only place this arithmetic exists, whatever the
// fusion depth and on either side
FLOW_FN FlowUV flow_hs_update(double ubar, double vbar, const FlowCoef& c, const FlowUV& f0, double alpha2) {
    FLOW_NO_CONTRACT
    const double t = (c.ix * (ubar - f0.u) + c.iy * (vbar - f0.v) + c.it) / (alpha2 + c.ix * c.ix + c.iy * c.iy);
    FlowUV r;
    r.u = ubar - c.ix * t;
    r.v = vbar - c.iy * t;
    return r;
}

// ---- the byte coding (scraping/preprocess.py:183-196) -----------------------------------------------------------------------------
FLOW_FN float flow_mag(float u, float v) {
    FLOW_NO_CONTRACT
    return (float)sqrt((double)u * (double)u + (double)v * (double)v);
}

FLOW_FN void flow_limits(float lo, float hi, float* out) {
    FLOW_NO_CONTRACT
    if (hi - lo < 1.f) hi = lo + 1.f;                       // "avoid 0 division", in fp32: the stored limits are the ones used
    out[0] = lo;
    out[1] = hi;
}

FLOW_FN void flow_bytes(float u, float v, float lo, float hi, uint8_t* rgb) {
    FLOW_NO_CONTRACT
    const float mag = flow_mag(u, v);
    const double ang = mag < 0.005f ? 0. : atan2((double)v, (double)u) + FLOW_PI;
    rgb[0] = (uint8_t)(int)(ang * 255. / (FLOW_PI * 2.));
    rgb[1] = 0;
    rgb[2] = (uint8_t)(int)(((double)mag - (double)lo) / ((double)hi - (double)lo) * 255.);
}

// ---- argument checks shared by both libraries ---------------------------------------------------------------------------------------
inline size_t flow_level_pixels(int h, int w, int levels) {           // pixels of one frame's pyramid
    size_t s = 0;
    for (int l = 0; l < levels; ++l) s += (size_t)(h >> l) * (size_t)(w >> l);
    return s;
}

// scratch layout in doubles: pyramid [n][levels], smoothed [n] and per pair three coefficient planes + three (u, v) fields, all of
// the finest level's size
inline size_t flow_scratch_doubles(int n_frames, int h, int w, int levels) {
    const size_t hw = (size_t)h * w, pairs = (size_t)(n_frames - 1);
    return (size_t)n_frames * (flow_level_pixels(h, w, levels) + hw) + pairs * hw * 9;
}

inline int flow_check_sizes(int n_frames, int h, int w, int levels, const char** why) {
    if (n_frames < 0) { *why = "n_frames is negative"; return SAGEN_ERR_SHAPE; }
    if (h < 1 || w < 1) { *why = "h and w must be positive"; return SAGEN_ERR_SHAPE; }
    if (levels < 1 || levels > FLOW_MAX_LEVELS) { *why = "levels takes 1..8"; return SAGEN_ERR_UNSUPPORTED; }
    if (h > FLOW_MAX_DIM || w > FLOW_MAX_DIM) { *why = "h and w take at most 4096"; return SAGEN_ERR_UNSUPPORTED; }
    if (n_frames > FLOW_MAX_FRAMES) { *why = "n_frames takes at most 65535"; return SAGEN_ERR_UNSUPPORTED; }
    const int k = 1 << (levels - 1);
    if (h % k || w % k) { *why = "h and w must be divisible by 2^(levels-1)"; return SAGEN_ERR_SHAPE; }
    if (h / k < FLOW_MIN_COARSEST || w / k < FLOW_MIN_COARSEST) { *why = "the coarsest level of levels must keep 4 pixels in h and w"; return SAGEN_ERR_UNSUPPORTED; }
    return SAGEN_OK;
}

inline int flow_args_fill(FlowArgs& a, int n_frames, int h, int w, const sagen_flow_params* p, const char** why) {
    if (p->warps < 1 || p->warps > FLOW_MAX_WARPS) { *why = "warps takes 1..16"; return SAGEN_ERR_UNSUPPORTED; }
    if (p->iters < 1 || p->iters > FLOW_MAX_ITERS) { *why = "iters takes 1..1000"; return SAGEN_ERR_UNSUPPORTED; }
    if (p->fuse < 0 || p->fuse > FLOW_MAX_FUSE) { *why = "fuse takes 0..8"; return SAGEN_ERR_UNSUPPORTED; }
    if (!(p->alpha > 0.) || !std::isfinite(p->alpha)) { *why = "alpha must be positive and finite"; return SAGEN_ERR_UNSUPPORTED; }
    const int rc = flow_check_sizes(n_frames, h, w, p->levels, why);
    if (rc != SAGEN_OK) return rc;
    a.n_frames = n_frames; a.h = h; a.w = w;
    a.levels = p->levels; a.warps = p->warps; a.iters = p->iters; a.wrap = p->wrap != 0; a.fuse = p->fuse;
    a.alpha2 = p->alpha * p->alpha;
    return SAGEN_OK;
}

inline int flow_encode_check(int n, int h, int w, const char** why) {
    if (n < 0) { *why = "n is negative"; return SAGEN_ERR_SHAPE; }
    if (h < 1 || w < 1) { *why = "h and w must be positive"; return SAGEN_ERR_SHAPE; }
    if (h > FLOW_MAX_DIM || w > FLOW_MAX_DIM) { *why = "h and w take at most 4096"; return SAGEN_ERR_UNSUPPORTED; }
    if (n > FLOW_MAX_FRAMES) { *why = "n takes at most 65535"; return SAGEN_ERR_UNSUPPORTED; }
    return SAGEN_OK;
}

}  // namespace sagen
