// Moving point sources (gfx950): the front end of the reference's ambisonics toolbox - AmbiEncoder.encode / encode_frame / encode_v2
// (pyutils/ambisonics/encoder.py:10-55), SourceBinauralizer over VirtualStereoMic and Convolvotron (binauralizer.py:12-121) and the
// positions behind SphericalSourceVisualizer (distance.py:62-97), all over MovingSource.tic (position.py:73-102) - see include/sagen.h.
// The reference walks these in a Python loop per audio sample; every sample is independent, so here a thread owns a sample:
//
//   sources_track_kernel     thread = (sample, source): the unit direction and, optionally, the closest direction of a set
//   sources_encode_kernel    thread = sample, loop over the sources: ambi[t][c] = sum_s g_s sig_s[t - d_s] Y_c(u_s(t))
//   sources_mic_kernel       thread = sample, loop over the sources and the two ears
//   sources_hrir_kernel      workgroup = 256 consecutive samples; per source the K - 1 + 256 signal samples they reach are staged in
//                            LDS once, the direction set is staged in LDS for the search (in chunks of SRC_DCHUNK), and the taps of
//                            each thread's closest response are read from global memory - neighbouring samples nearly always
//                            share the index, so these are broadcast loads
//
// Where, which way and how far is fp64 (sources_core.h, shared with the CPU twin, no contraction).  The sample sums are fp32: one
// accumulator per output, sources outermost, taps ascending, one fmaf each - a pure function of the absolute sample index, so a
// stream rendered in pieces gives the bits of the one-call result.
#include "kernels.h"
#include "sources_core.h"

namespace sagen {

namespace {

constexpr int SRC_T = 256;                // samples per workgroup
constexpr int SRC_DCHUNK = 2048;          // directions staged at a time: 48 KiB of LDS beside <= 3 KiB of signal

struct SourcePoint {
    double phi, nu, r, u[3];
};

__device__ __forceinline__ SourcePoint source_at(const double* __restrict__ ctrl, const SourceSet& ss, int s, long long t) {
    SourcePoint p;
    const int p0 = ss.pt_off[s];
    source_polar(ctrl + (long long)p0 * 3, ss.pt_off[s + 1] - p0, ss.nframes[s], ss.duration[s], ss.rate, t, p.phi, p.nu, p.r);
    source_unit(p.phi, p.nu, p.r, p.u);
    return p;
}

__global__ __launch_bounds__(256) void sources_track_kernel(const double* __restrict__ ctrl, const SourceSet ss, long long t0, long long n,
                                                            long long stride, const double* __restrict__ dirs, int D,
                                                            double* __restrict__ unit,        // [n][S][3] or null
                                                            int* __restrict__ nearest) {      // [n][S] or null
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int S = ss.n_sources;
    if (e >= n * S) return;
    const long long i = e / S;
    const int s = (int)(e - i * S);
    const SourcePoint p = source_at(ctrl, ss, s, t0 + i * stride);
    if (unit) {
        unit[e * 3] = p.u[0];
        unit[e * 3 + 1] = p.u[1];
        unit[e * 3 + 2] = p.u[2];
    }
    if (nearest) {
        const double mx = nearest_max(dirs, D, p.u, -INFINITY);
        const int f = nearest_first(dirs, 0, D, p.u, mx, -1);
        nearest[e] = f < 0 ? 0 : f;          // (a non-finite direction matches nothing)
    }
}

template <int C>
__global__ __launch_bounds__(256) void sources_encode_kernel(const float* __restrict__ signals, long long ld, const double* __restrict__ ctrl,
                                                             const SourceSet ss, int distance_model, double radius, long long t0,
                                                             long long n, float* __restrict__ ambi) {        // [n][C]
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long t = t0 + i;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (int s = 0; s < ss.n_sources; ++s) {
        const SourcePoint p = source_at(ctrl, ss, s, t);
        double Y[C];
        source_harmonics<C>(p.u, Y);
        double g = 1.;
        long long d = 0;
        bool ok = true;
        if (distance_model) {                // encode_v2 (encoder.py:46-52), per sample
            const double dist = fabs(p.r) - radius;
            ok = source_delay(dist, ss.rate, d);
            g = 1. / (1. + dist);
        }
        const long long j = t - d;
        if (ok && j >= 0 && j < ss.nframes[s]) {
            const float x = signals[s * ld + j];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = fmaf((float)(g * Y[c]), x, acc[c]);
        }
    }
    if (C == 4) {
        *(float4*)(ambi + i * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) ambi[i * C + c] = acc[c];
    }
}

// VirtualStereoMic.binauralize_frame (binauralizer.py:38-55)
__global__ __launch_bounds__(256) void sources_mic_kernel(const float* __restrict__ signals, long long ld, const double* __restrict__ ctrl,
                                                          const SourceSet ss, long long t0, long long n, float* __restrict__ y) {      // [n][2]
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long t = t0 + i;
    float acc[2] = {0.f, 0.f};
    const double inv_s = 1. / (double)ss.n_sources;
    for (int s = 0; s < ss.n_sources; ++s) {
        const SourcePoint p = source_at(ctrl, ss, s, t);
        const double ar = fabs(p.r), px = ar * p.u[0], py = ar * p.u[1], pz = ar * p.u[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double dy = py - (e == 0 ? SRC_EAR_Y : -SRC_EAR_Y);
            const double dist = sqrt(px * px + dy * dy + pz * pz);
            long long d;
            if (!source_delay(dist, ss.rate, d)) continue;
            const long long j = t - d;
            if (j >= 0 && j < ss.nframes[s]) acc[e] = fmaf((float)(inv_s / (1. + dist)), signals[s * ld + j], acc[e]);
        }
    }
    *(float2*)(y + i * 2) = make_float2(acc[0], acc[1]);
}

// Convolvotron (binauralizer.py:63-90) with the response re-chosen per sample.  V4: K % 4 == 0 and a 16-byte aligned table - four taps
// per load, the same order of the sum
template <bool V4>
__global__ __launch_bounds__(SRC_T) void sources_hrir_kernel(const float* __restrict__ signals, long long ld, const double* __restrict__ ctrl,
                                                             const SourceSet ss, const double* __restrict__ dirs,
                                                             const float* __restrict__ hrir,      // [D][2][K]
                                                             int D, int K, long long zero_before, long long t0, long long n,
                                                             float* __restrict__ y) {             // [n][2]
    extern __shared__ double sources_lds[];
    const int dc = D < SRC_DCHUNK ? D : SRC_DCHUNK;
    double* ldirs = sources_lds;                       // [dc][3]
    float* lsig = (float*)(sources_lds + dc * 3);      // slot q holds sig[tb - (K - 1) + q], q < K - 1 + SRC_T
    const int tid = threadIdx.x;
    const long long tb = t0 + (long long)blockIdx.x * SRC_T;      // the workgroup's first sample
    const bool active = (long long)blockIdx.x * SRC_T + tid < n;
    const long long t = active ? tb + tid : t0;        // (an idle thread tracks a valid sample and stores nothing)
    const bool one_chunk = D <= SRC_DCHUNK;
    if (one_chunk)
        for (int q = tid; q < D * 3; q += SRC_T) ldirs[q] = dirs[q];
    float accl = 0.f, accr = 0.f;
    for (int s = 0; s < ss.n_sources; ++s) {
        __syncthreads();                               // the previous source's taps loop has read lsig
        const long long nf = ss.nframes[s];
        for (int q = tid; q < K - 1 + SRC_T; q += SRC_T) {
            const long long j = tb - (K - 1) + q;
            lsig[q] = j >= 0 && j < nf ? signals[s * ld + j] : 0.f;
        }
        const SourcePoint p = source_at(ctrl, ss, s, t);
        int near = -1;
        if (one_chunk) {
            __syncthreads();
            near = nearest_first(ldirs, 0, D, p.u, nearest_max(ldirs, D, p.u, -INFINITY), -1);
        } else {
            double mx = -INFINITY;
            for (int sweep = 0; sweep < 2; ++sweep)
                for (int c0 = 0; c0 < D; c0 += SRC_DCHUNK) {
                    const int cnt = D - c0 < SRC_DCHUNK ? D - c0 : SRC_DCHUNK;
                    __syncthreads();
                    for (int q = tid; q < cnt * 3; q += SRC_T) ldirs[q] = dirs[(long long)c0 * 3 + q];
                    __syncthreads();
                    if (sweep == 0)
                        mx = nearest_max(ldirs, cnt, p.u, mx);
                    else
                        near = nearest_first(ldirs, c0, cnt, p.u, mx, near);
                }
        }
        near = near < 0 ? 0 : near;
        const float* hl = hrir + (long long)near * 2 * K;
        const float* hr = hl + K;
        const float* x = lsig + tid + K - 1;           // x[-k] = sig[t - k]; zero where the stream has no sample
        if (V4) {
            for (int k = 0; k < K; k += 4) {
                const float4 a = *(const float4*)(hl + k), b = *(const float4*)(hr + k);
                const float x0 = x[-k], x1 = x[-k - 1], x2 = x[-k - 2], x3 = x[-k - 3];
                accl = fmaf(a.x, x0, accl); accr = fmaf(b.x, x0, accr);
                accl = fmaf(a.y, x1, accl); accr = fmaf(b.y, x1, accr);
                accl = fmaf(a.z, x2, accl); accr = fmaf(b.z, x2, accr);
                accl = fmaf(a.w, x3, accl); accr = fmaf(b.w, x3, accr);
            }
        } else {
            for (int k = 0; k < K; ++k) {
                const float xk = x[-k];
                accl = fmaf(hl[k], xk, accl);
                accr = fmaf(hr[k], xk, accr);
            }
        }
    }
    if (active) {
        const bool z = t < zero_before;
        *(float2*)(y + (t - t0) * 2) = make_float2(z ? 0.f : accl, z ? 0.f : accr);
    }
}

}  // namespace

// ---- the backends of the entry points (op_entries.h), which have checked every argument and filled the SourceSet ----
int run_source_track(const double* ctrl, const SourceSet& ss, int64_t t0, int64_t n, int64_t stride, const double* dirs, int n_dirs,
                     double* unit, int32_t* nearest, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sources_track_kernel, dim3(cdiv(n * ss.n_sources, 256)), dim3(256), 0, s, ctrl, ss, (long long)t0, (long long)n,
                       (long long)stride, dirs, n_dirs, unit, (int*)nearest);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_encode_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int channels, int distance_model,
                       double radius, int64_t t0, int64_t n, float* ambi, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(n, 256));
    if (channels == 4)
        hipLaunchKernelGGL(sources_encode_kernel<4>, grid, dim3(256), 0, s, signals, (long long)ld, ctrl, ss, distance_model, radius,
                           (long long)t0, (long long)n, ambi);
    else
        hipLaunchKernelGGL(sources_encode_kernel<9>, grid, dim3(256), 0, s, signals, (long long)ld, ctrl, ss, distance_model, radius,
                           (long long)t0, (long long)n, ambi);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_binauralize_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int mode, const double* dirs,
                            const float* hrir, int n_dirs, int ntaps, int64_t zero_before, int64_t t0, int64_t n, float* y, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (mode == SAGEN_SOURCES_MIC) {
        hipLaunchKernelGGL(sources_mic_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, signals, (long long)ld, ctrl, ss, (long long)t0, (long long)n, y);
    } else {
        const int dc = n_dirs < SRC_DCHUNK ? n_dirs : SRC_DCHUNK;
        const size_t lds = (size_t)dc * 3 * sizeof(double) + (size_t)(ntaps - 1 + SRC_T) * sizeof(float);      // <= 49 152 + 3 068 bytes
        const dim3 grid(cdiv(n, SRC_T));
        if (ntaps % 4 == 0 && ((uintptr_t)hrir) % 16 == 0)
            hipLaunchKernelGGL(sources_hrir_kernel<true>, grid, dim3(SRC_T), lds, s, signals, (long long)ld, ctrl, ss, dirs, hrir, n_dirs, ntaps,
                               (long long)zero_before, (long long)t0, (long long)n, y);
        else
            hipLaunchKernelGGL(sources_hrir_kernel<false>, grid, dim3(SRC_T), lds, s, signals, (long long)ld, ctrl, ss, dirs, hrir, n_dirs, ntaps,
                               (long long)zero_before, (long long)t0, (long long)n, y);
    }
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
