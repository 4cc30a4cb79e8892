// Reprojection of 360-degree frames (include/sagen.h: sagen_reproject): the geometry that is the same for every output pixel - the
// direction of a destination sub-sample (equirectangular, cube face, equi-angular cube face, pinhole view), its rotation, the source
// pixel that direction lands on (equirectangular or one face of a cube layout) and the bilinear fetch.  It replaces what the
// reference does offline: scraping/utils.py:91-144 (unwarp_eac, gen_eac2eqr_maps), the cube <-> equirect step of
// 3rd-party/vrProjector (CubemapProjection.py:68-121, EquirectangularProjection.py:23-42) and the crop of scraping/preprocess.py:51-52.
//
// The same code runs on the device (project.hip, one thread per output pixel) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).
// Coordinates, weights and the sum are fp64; it is compiled WITHOUT contraction so that both builds round alike.
//
// World frame (ambisonics.py): x front, y left, z up.  vrProjector's frame is x front, y RIGHT, z DOWN (its equirectangular row
// grows with phi = asin(z), its column with theta = atan2(y, x): EquirectangularProjection.py:29-31), so a vector (x, y, z) there is
// (x, -y, -z) here.  Its six face images read, in OUR frame (CubemapProjection.py, u = column / n, v = row / n):
//     face     axis     column grows along   row grows along      lines
//     front    +x       -y                   -z                   :82-87    u = .5 + t y,  v = .5 + t z
//     back     -x       +y                   -z                   :88-93    u = .5 - t y,  v = .5 + t z
//     right    -y       -x                   -z                   :96-101   u = .5 - t x,  v = .5 + t z
//     left     +y       +x                   -z                   :102-107  u = .5 + t x,  v = .5 + t z
//     bottom   -z       -y                   -x                   :110-115  u = .5 + t y,  v = .5 - t x
//     top      +z       -y                   +x                   :116-121  u = .5 + t y,  v = .5 + t x
// These are the CANONICAL face frames (orientation 0).  A layout stores, per face, where its cell sits in the frame and how the cell
// is turned against the canonical image: see proj_face_frame.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define PROJ_FN __host__ __device__ __forceinline__
#else
#define PROJ_FN inline
#endif
#if defined(__clang__)
#define PROJ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PROJ_NO_CONTRACT
#endif

namespace sagen {

constexpr int PROJ_MAX_DIM = 16384;
constexpr int PROJ_MAX_FRAMES = 65535;
constexpr int PROJ_MAX_SS = 8;
constexpr double PROJ_PI = 3.14159265358979323846;

// One face of a layout, ready for the kernel: rectangle, and the world vectors along which the CELL's column and row grow.
struct ProjFaceGeom {
    int x0, y0, n;                 // square cell of n x n pixels
    signed char R[3], D[3];        // cell column / row direction; the axis is face f's: +x -x +y -y +z -z
};

// One side (source or destination) of a call, by value in the kernel arguments.
struct ProjSide {
    int kind;                      // SAGEN_PROJ_*
    int x0, y0, w, h;              // ER / VIEW: the rectangle that holds the image
    int fh, fw;                    // the frame that holds the rectangles
    double t;                      // VIEW: tan(hfov / 2)
    ProjFaceGeom face[6];
};

struct ProjArgs {
    ProjSide src, dst;
    int n, n_rot, S;
};

// Axis, column and row vectors of face f (0..5: +x -x +y -y +z -z) whose cell is stored with orientation `orient` (0..7).  The
// canonical frame (Rc, Dc) is the table at the top of this file.  With (p, q) the canonical and (pc, qc) the cell coordinates:
//     bit 2 set: the cell is mirrored left-right first, p -> -p
//     turns 0: (pc, qc) = ( p,  q)
//     turns 1: (pc, qc) = ( q, -p)     canonical = np.rot90(cell, -1)   (utils.py:133 'bottom', :135 'top')
//     turns 2: (pc, qc) = (-p, -q)
//     turns 3: (pc, qc) = (-q,  p)     canonical = np.rot90(cell)       (utils.py:134 'back')
PROJ_FN void proj_face_frame(int f, int orient, int A[3], int R[3], int D[3]) {
    const int canon[6][6] = {{0, -1, 0, 0, 0, -1},     // +x front
                             {0, 1, 0, 0, 0, -1},      // -x back
                             {1, 0, 0, 0, 0, -1},      // +y left
                             {-1, 0, 0, 0, 0, -1},     // -y right
                             {0, -1, 0, 1, 0, 0},      // +z top
                             {0, -1, 0, -1, 0, 0}};    // -z bottom
    int rc[3], dc[3];
    for (int k = 0; k < 3; ++k) {
        A[k] = k == f / 2 ? (f & 1 ? -1 : 1) : 0;
        rc[k] = (orient & 4) ? -canon[f][k] : canon[f][k];
        dc[k] = canon[f][3 + k];
    }
    for (int k = 0; k < 3; ++k) {
        switch (orient & 3) {
            case 0: R[k] = rc[k]; D[k] = dc[k]; break;
            case 1: R[k] = dc[k]; D[k] = -rc[k]; break;
            case 2: R[k] = -rc[k]; D[k] = -dc[k]; break;
            default: R[k] = -dc[k]; D[k] = rc[k]; break;
        }
    }
}

// host: one sagen_projection, checked against its frame, into a ProjSide.  Returns SAGEN_OK or the error code, *why naming the fault.
inline int proj_side_fill(ProjSide& s, const sagen_projection* p, int fh, int fw, bool is_source, const char** why) {
    *why = "";
    if (p->kind != SAGEN_PROJ_ER && p->kind != SAGEN_PROJ_CUBE && p->kind != SAGEN_PROJ_EAC && p->kind != SAGEN_PROJ_VIEW)
        return *why = "unknown projection kind", SAGEN_ERR_UNSUPPORTED;
    if (p->kind == SAGEN_PROJ_VIEW && is_source) return *why = "a perspective view cannot be a source", SAGEN_ERR_UNSUPPORTED;
    s.kind = p->kind; s.fh = fh; s.fw = fw; s.t = 0.;
    s.x0 = 0; s.y0 = 0; s.w = fw; s.h = fh;
    for (int f = 0; f < 6; ++f) {
        s.face[f].x0 = s.face[f].y0 = 0; s.face[f].n = 1;
        for (int k = 0; k < 3; ++k) s.face[f].R[k] = s.face[f].D[k] = 0;
    }
    if (p->kind == SAGEN_PROJ_ER || p->kind == SAGEN_PROJ_VIEW) {
        if (p->w != 0 || p->h != 0) {
            if (p->w < 1 || p->h < 1 || p->x0 < 0 || p->y0 < 0 || p->x0 > fw - p->w || p->y0 > fh - p->h)
                return *why = "the rectangle does not lie inside the frame", SAGEN_ERR_SHAPE;
            s.x0 = p->x0; s.y0 = p->y0; s.w = p->w; s.h = p->h;
        }
        if (p->kind == SAGEN_PROJ_VIEW) {
            if (!(p->hfov > 0. && p->hfov < PROJ_PI)) return *why = "0 < hfov < pi expected", SAGEN_ERR_SHAPE;
            s.t = tan(p->hfov / 2.);
        }
        return SAGEN_OK;
    }
    for (int f = 0; f < 6; ++f) {
        const sagen_proj_face& c = p->face[f];
        if (c.w != c.h) return *why = "a cube face must be square", SAGEN_ERR_SHAPE;
        if (c.w < 1 || c.x0 < 0 || c.y0 < 0 || c.x0 > fw - c.w || c.y0 > fh - c.h)
            return *why = "a face rectangle does not lie inside the frame", SAGEN_ERR_SHAPE;
        if (c.orient < 0 || c.orient > 7) return *why = "a face orientation outside 0..7", SAGEN_ERR_SHAPE;
        int A[3], R[3], D[3];
        proj_face_frame(f, c.orient, A, R, D);
        s.face[f].x0 = c.x0; s.face[f].y0 = c.y0; s.face[f].n = c.w;
        for (int k = 0; k < 3; ++k) {
            s.face[f].R[k] = (signed char)R[k];
            s.face[f].D[k] = (signed char)D[k];
        }
    }
    return SAGEN_OK;
}

// host: every check of sagen_reproject that needs no pointer to be followed but the two descriptors
inline int proj_args_fill(ProjArgs& a, int n, int src_h, int src_w, const sagen_projection* sp, int dst_h, int dst_w,
                          const sagen_projection* dp, int n_rot, int supersample, const char** why) {
    *why = "";
    if (supersample < 1 || supersample > PROJ_MAX_SS) return *why = "supersample outside 1..8", SAGEN_ERR_UNSUPPORTED;
    if (src_h > PROJ_MAX_DIM || src_w > PROJ_MAX_DIM || dst_h > PROJ_MAX_DIM || dst_w > PROJ_MAX_DIM)
        return *why = "a frame dimension above 16384", SAGEN_ERR_UNSUPPORTED;
    if (n > PROJ_MAX_FRAMES) return *why = "more than 65535 frames in one call", SAGEN_ERR_UNSUPPORTED;
    if (n_rot != 0 && n_rot != 1 && n_rot != n) return *why = "n_rot must be 0, 1 or n", SAGEN_ERR_SHAPE;
    int rc = proj_side_fill(a.src, sp, src_h, src_w, true, why);
    if (rc != SAGEN_OK) return rc;
    rc = proj_side_fill(a.dst, dp, dst_h, dst_w, false, why);
    if (rc != SAGEN_OK) return rc;
    a.n = n; a.n_rot = n_rot; a.S = supersample;
    return SAGEN_OK;
}

// The cell of the destination that holds frame pixel (px, py): false where the pixel belongs to no rectangle (it is left alone).
// (cx, cy) are the pixel's coordinates inside the cell, (cw, ch) the cell's size, f the face.
template <int DK>
PROJ_FN bool proj_dst_cell(const ProjSide& d, int px, int py, int& f, int& cx, int& cy, int& cw, int& ch) {
    if (DK == SAGEN_PROJ_ER || DK == SAGEN_PROJ_VIEW) {
        f = 0; cx = px - d.x0; cy = py - d.y0; cw = d.w; ch = d.h;
        return cx >= 0 && cx < cw && cy >= 0 && cy < ch;
    }
    for (int k = 0; k < 6; ++k) {
        const int x = px - d.face[k].x0, y = py - d.face[k].y0, n = d.face[k].n;
        if (x >= 0 && x < n && y >= 0 && y < n) {
            f = k; cx = x; cy = y; cw = n; ch = n;
            return true;
        }
    }
    return false;
}

// head-frame direction (any length) of the sub-sample at fractions (xf, yf) of the destination cell
template <int DK>
PROJ_FN void proj_dst_dir(const ProjSide& d, int f, double xf, double yf, int cw, int ch, double v[3]) {
    PROJ_NO_CONTRACT
    if (DK == SAGEN_PROJ_ER) {
        const double az = PROJ_PI - 2. * PROJ_PI * xf, el = PROJ_PI / 2. - PROJ_PI * yf;
        const double ce = cos(el);
        v[0] = ce * cos(az); v[1] = ce * sin(az); v[2] = sin(el);
    } else if (DK == SAGEN_PROJ_VIEW) {
        v[0] = 1.;
        v[1] = d.t * (1. - 2. * xf);
        v[2] = d.t * ((double)ch / (double)cw) * (1. - 2. * yf);
    } else {
        double p = 2. * xf - 1., q = 2. * yf - 1.;
        if (DK == SAGEN_PROJ_EAC) {
            p = tan(PROJ_PI * p / 4.);
            q = tan(PROJ_PI * q / 4.);
        }
        const ProjFaceGeom& g = d.face[f];
        for (int k = 0; k < 3; ++k) v[k] = (k == f / 2 ? (f & 1 ? -1. : 1.) : 0.) + p * (double)g.R[k] + q * (double)g.D[k];
    }
}

PROJ_FN void proj_rotate(const double* rot, const double v[3], double w[3]) {
    PROJ_NO_CONTRACT
    for (int k = 0; k < 3; ++k) w[k] = rot[k * 3] * v[0] + rot[k * 3 + 1] * v[1] + rot[k * 3 + 2] * v[2];
}

PROJ_FN int proj_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The four taps of direction w in the source frame: byte offsets of the pixels (row-major, 3 bytes each) and the two weights.  Every
// index is clamped into its rectangle after the conversion to int, so whatever w holds (a NaN of a bad matrix included) the taps stay
// inside the frame.
template <int SK>
PROJ_FN void proj_src_taps(const ProjSide& s, const double w[3], long long off[4], double& fx, double& fy) {
    PROJ_NO_CONTRACT
    int x0, y0, cw, ch, ix0, ix1;
    double x, y;
    if (SK == SAGEN_PROJ_ER) {
        const double az = atan2(w[1], w[0]), el = atan2(w[2], hypot(w[0], w[1]));
        x0 = s.x0; y0 = s.y0; cw = s.w; ch = s.h;
        x = (PROJ_PI - az) / (2. * PROJ_PI) * (double)cw - 0.5;
        y = (PROJ_PI / 2. - el) / PROJ_PI * (double)ch - 0.5;
        const double xl = floor(x);
        fx = x - xl;
        ix0 = xl >= 0. ? (xl < (double)cw ? (int)xl : cw - 1) : -1;      // -1 .. cw - 1: wraps (a NaN takes the last branch)
        if (ix0 < 0) ix0 += cw;
        ix1 = ix0 + 1;
        if (ix1 >= cw) ix1 -= cw;
    } else {
        const double ax = fabs(w[0]), ay = fabs(w[1]), az = fabs(w[2]);
        const int axis = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
        const int f = axis * 2 + (w[axis] < 0. ? 1 : 0);
        const ProjFaceGeom& g = s.face[f];
        const double a = fabs(w[axis]);
        double p = ((double)g.R[0] * w[0] + (double)g.R[1] * w[1] + (double)g.R[2] * w[2]) / a;
        double q = ((double)g.D[0] * w[0] + (double)g.D[1] * w[1] + (double)g.D[2] * w[2]) / a;
        if (SK == SAGEN_PROJ_EAC) {
            p = atan(p) * (4. / PROJ_PI);
            q = atan(q) * (4. / PROJ_PI);
        }
        x0 = g.x0; y0 = g.y0; cw = g.n; ch = g.n;
        x = (p + 1.) / 2. * (double)cw - 0.5;
        x = fmin(fmax(x, 0.), (double)(cw - 1));   // clamped inside the face: no filtering across faces
        const double xl = floor(x);
        fx = x - xl;
        ix0 = (int)xl;
        ix1 = ix0 + 1;
        y = (q + 1.) / 2. * (double)ch - 0.5;
    }
    y = fmin(fmax(y, 0.), (double)(ch - 1));
    const double yl = floor(y);
    fy = y - yl;
    int iy0 = (int)yl, iy1 = iy0 + 1;
    ix0 = proj_clampi(ix0, 0, cw - 1); ix1 = proj_clampi(ix1, 0, cw - 1);
    iy0 = proj_clampi(iy0, 0, ch - 1); iy1 = proj_clampi(iy1, 0, ch - 1);
    if (!(fx >= 0. && fx <= 1.)) fx = 0.;
    if (!(fy >= 0. && fy <= 1.)) fy = 0.;
    const long long r0 = (long long)(y0 + iy0) * s.fw, r1 = (long long)(y0 + iy1) * s.fw;
    off[0] = (r0 + x0 + ix0) * 3; off[1] = (r0 + x0 + ix1) * 3;
    off[2] = (r1 + x0 + ix0) * 3; off[3] = (r1 + x0 + ix1) * 3;
}

// One output pixel: the mean of the S x S bilinear samples per channel, floor(mean + 0.5).  `frame` is the source frame, (cx, cy) the
// pixel inside its destination cell; rot is null (identity) or 9 doubles.
template <int SK, int DK>
PROJ_FN void proj_pixel(const ProjArgs& a, const uint8_t* frame, const double* rot, int f, int cx, int cy, int cw, int ch, uint8_t out[3]) {
    PROJ_NO_CONTRACT
    double sum[3] = {0., 0., 0.};
    const double S = (double)a.S;
    for (int b = 0; b < a.S; ++b) {
        const double yf = ((double)cy + ((double)b + 0.5) / S) / (double)ch;
        for (int c = 0; c < a.S; ++c) {
            const double xf = ((double)cx + ((double)c + 0.5) / S) / (double)cw;
            double v[3], w[3];
            proj_dst_dir<DK>(a.dst, f, xf, yf, cw, ch, v);
            if (rot) proj_rotate(rot, v, w);
            else { w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; }
            long long off[4];
            double fx, fy;
            proj_src_taps<SK>(a.src, w, off, fx, fy);
            for (int k = 0; k < 3; ++k) {
                const double top = (1. - fx) * (double)frame[off[0] + k] + fx * (double)frame[off[1] + k];
                const double bot = (1. - fx) * (double)frame[off[2] + k] + fx * (double)frame[off[3] + k];
                sum[k] += (1. - fy) * top + fy * bot;
            }
        }
    }
    for (int k = 0; k < 3; ++k) {
        const double m = floor(sum[k] / (S * S) + 0.5);
        out[k] = (uint8_t)(m < 0. ? 0 : (m > 255. ? 255 : (int)m));
    }
}

}  // namespace sagen
