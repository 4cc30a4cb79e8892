// Moving point sources (include/sagen.h: sagen_source_track / sagen_encode_sources / sagen_binauralize_sources): the fp64 part that
// is the same for every sample of every source - where the source is (MovingSource.tic, pyutils/ambisonics/position.py:73-102),
// the direction that leaves behind (Position.set_polar -> calc_cartesian -> calc_polar, :24-37), the harmonics of that direction
// (common.py:136-157 at orders 1 and 2, in cartesian closed form) and the closest direction of a set (hrir.py:35-41 under the tie
// rule of render.py: HrirSet.closest).
//
// The same code runs on the device (sources.hip, one thread per sample) and on the host (csrc_cpu/sagen_cpu.cpp, plain loops).  It
// is compiled WITHOUT contraction: a delay is int(dist / 343 * rate) and a nearest index an argmax, and neither may depend on
// whether a multiply and an add were fused.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/sagen.h"

#if defined(__HIPCC__)
#define SRC_FN __host__ __device__ __forceinline__
#else
#define SRC_FN inline
#endif
#if defined(__clang__)
#define SRC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SRC_NO_CONTRACT
#endif

namespace sagen {

constexpr int SRC_MAX_SOURCES = 64;
constexpr int SRC_MAX_DIRS = 4096;
constexpr int SRC_MAX_TAPS = 512;
constexpr int64_t SRC_MAX_N = (int64_t)1 << 31;  // samples per call (the device's grid is n / 256 workgroups)
constexpr double SRC_SPEED_OF_SOUND = 343.;      // binauralizer.py:9, encoder.py:49
constexpr double SRC_EAR_Y = 0.1;                // VirtualStereoMic: ears at (0, +-0.1, 0) (binauralizer.py:13-16)
constexpr double SRC_TIE = 1e-12;                // HrirSet.closest: every candidate this close to the maximum ties

// The sources of one call.  The per-source scalars travel by value (kernel arguments on the device); ctrl is a device array.
struct SourceSet {
    int n_sources;
    int pt_off[SRC_MAX_SOURCES + 1];             // control points of source s: ctrl rows pt_off[s] .. pt_off[s + 1] - 1
    long long nframes[SRC_MAX_SOURCES];          // int(duration * rate)
    double duration[SRC_MAX_SOURCES];            // N / float(rate)
    double rate;
};

// (phi, nu, r) of sample i < nframes of a source with P >= 1 control points cp [P][3]  (position.py:78-101)
SRC_FN void source_polar(const double* cp, int P, long long nframes, double duration, double rate, long long i, double& phi, double& nu,
                         double& r) {
    SRC_NO_CONTRACT
    long long idx = P - 1;
    if (P > 1 && i != nframes - 1) {
        idx = (long long)floor((double)i * ((double)(P - 1) / (double)(nframes - 1)));      // floor(linspace(0, P - 1, nframes))[i]
        if (idx > P - 1) idx = P - 1;
        if (idx < 0) idx = 0;
    }
    if (idx == P - 1) {
        phi = cp[idx * 3]; nu = cp[idx * 3 + 1]; r = cp[idx * 3 + 2];
        return;
    }
    // pts_t = linspace(0, duration, P): j * step, the last one the stop itself
    const double step = duration / (double)(P - 1);
    const double ta = (double)idx * step;
    const double tb = idx + 1 == P - 1 ? duration : (double)(idx + 1) * step;
    const double al = ((double)i * (1. / rate) - ta) / (tb - ta), be = 1. - al;
    const double* a = cp + idx * 3;
    phi = al * a[3] + be * a[0];
    nu = al * a[4] + be * a[1];
    r = al * a[5] + be * a[2];
}

// the unit direction set_polar leaves behind: sgn(r) (cos phi cos nu, sin phi cos nu, sin nu); (1, 0, 0) at r == 0 (atan2(0, 0) = 0)
SRC_FN void source_unit(double phi, double nu, double r, double u[3]) {
    SRC_NO_CONTRACT
    if (r == 0.) {
        u[0] = 1.; u[1] = 0.; u[2] = 0.;
        return;
    }
    const double sg = r < 0. ? -1. : 1., cn = cos(nu);
    u[0] = sg * (cos(phi) * cn);
    u[1] = sg * (sin(phi) * cn);
    u[2] = sg * sin(nu);
}

// ACN / SN3D harmonics of a unit direction: W Y Z X | V T R S U
template <int C>
SRC_FN void source_harmonics(const double u[3], double Y[C]) {
    SRC_NO_CONTRACT
    const double x = u[0], y = u[1], z = u[2];
    Y[0] = 1.; Y[1] = y; Y[2] = z; Y[3] = x;
    if (C == 9) {
        const double s3 = 1.7320508075688772;
        Y[4] = s3 * x * y;
        Y[5] = s3 * y * z;
        Y[6] = (3. * z * z - 1.) / 2.;
        Y[7] = s3 * x * z;
        Y[8] = (s3 / 2.) * (x * x - y * y);
    }
}

SRC_FN double source_dot(const double* d, const double u[3]) {
    SRC_NO_CONTRACT
    return d[0] * u[0] + d[1] * u[1] + d[2] * u[2];
}

// the closest direction in two sweeps over dirs [count][3] (or over its chunks, in order): the maximum dot product, then the first
// index whose dot product is >= maximum - SRC_TIE
SRC_FN double nearest_max(const double* dirs, int count, const double u[3], double mx) {
    for (int j = 0; j < count; ++j) {
        const double d = source_dot(dirs + j * 3, u);
        mx = d > mx ? d : mx;
    }
    return mx;
}
SRC_FN int nearest_first(const double* dirs, int base, int count, const double u[3], double mx, int found) {
    SRC_NO_CONTRACT
    const double thr = mx - SRC_TIE;
    for (int j = 0; j < count; ++j)
        if (found < 0 && source_dot(dirs + j * 3, u) >= thr) found = base + j;
    return found;
}

// delay in samples and distance gain of a path of `dist` metres: int(dist / 343. * rate), 1 / (1 + dist); false where the delay
// cannot be a sample index
SRC_FN bool source_delay(double dist, double rate, long long& d) {
    SRC_NO_CONTRACT
    const double dd = dist / SRC_SPEED_OF_SOUND * rate;
    if (!(dd > -9e15 && dd < 9e15)) return false;
    d = (long long)dd;                           // int(): towards zero
    return true;
}

// host: the flat arrays of the header into a SourceSet, checked; t_last = the largest sample index the call evaluates.  Returns
// SAGEN_OK or the error code, *why naming what was wrong.
inline int source_set_fill(SourceSet& ss, const double* ctrl, const int32_t* pt_off, const int64_t* nframes, const double* duration,
                           int n_sources, double rate, int64_t t_first, int64_t t_last, const char** why) {
    *why = "";
    if (!ctrl || !pt_off || !nframes || !duration) return *why = "null source array", SAGEN_ERR_NULL;
    if (n_sources < 1 || !(rate > 0.) || t_first < 0 || t_last < t_first) return *why = "n_sources >= 1, rate > 0, t0 >= 0, n >= 1 expected", SAGEN_ERR_SHAPE;
    if (n_sources > SRC_MAX_SOURCES) return *why = "more than 64 sources", SAGEN_ERR_UNSUPPORTED;
    ss.n_sources = n_sources;
    ss.rate = rate;
    if (pt_off[0] < 0) return *why = "pt_off[0] < 0", SAGEN_ERR_SHAPE;
    for (int s = 0; s < n_sources; ++s) {
        if (pt_off[s + 1] <= pt_off[s]) return *why = "a source without control points (pt_off must increase)", SAGEN_ERR_SHAPE;
        if (nframes[s] < 1 || !(duration[s] > 0.)) return *why = "nframes >= 1 and duration > 0 expected", SAGEN_ERR_SHAPE;
        if (t_last >= nframes[s]) return *why = "the requested samples reach past the shortest source (t < min nframes)", SAGEN_ERR_SHAPE;
        ss.pt_off[s] = pt_off[s];
        ss.nframes[s] = nframes[s];
        ss.duration[s] = duration[s];
    }
    ss.pt_off[n_sources] = pt_off[n_sources];
    return SAGEN_OK;
}

}  // namespace sagen
