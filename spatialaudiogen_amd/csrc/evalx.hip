// The metrics of the reference's eval.py that it computes on the host (eval.py:172-193), on the device:
//
//  * env_mse (myutils.py:109-116): envelope |hilbert(x)| of pred and gt per channel, N = 4800 (scipy's circular analytic signal),
//    e = sqrt(x^2 + (Hx)^2) with (Hx)[n] = sum_m g[(n - m) mod N] x[m], g[k] = (2/N) cot(pi k / N) for odd k, 0 for even k;
//    env_mse = sqrt(mean_n (e_gt - e_pred)^2).  evalx_env_kernel: the circulant product directly (2400 odd taps), pred and gt of one
//    channel in one LDS ring shared by 10 waves (one per 512 outputs), 8 outputs per lane in registers (each tap step reuses 6 of
//    the 8 window samples).
//  * mel_lsd (myutils.py:96-106): librosa 0.6.0 melspectrogram(sr=48000, n_mels=128, fmax=12000): reflect pad 1024, 10 frames of
//    2048 at hop 512, periodic Hann, |rfft|^2 of bins 0..512 (the Slaney / norm=1 mel basis is 0 above 12 kHz = bin 512),
//    L = 10 log10(W S + 0.01), mel_lsd = sqrt(mean over 128 x 10 of (L_gt - L_pred)^2).  evalx_mel_kernel: one workgroup per
//    (window, channel, frame); pred and gt as the real and imaginary part of ONE 2048-point complex radix-2 FFT in LDS, split by
//    Hermitian symmetry; the mel weights are evaluated in fp64 from the edge formula (no basis in memory).
//  * emd/dir, emd/dir2 (distance.py:100-130): exact EMD-hat between directional RMS maps (emd_core.h), one wave per (map pair,
//    normalisation).
#include "kernels.h"
#include "emd_core.h"

namespace sagen {

constexpr int XN = 4800, XH = XN / 2;                   // window length, odd Hilbert taps
constexpr int ENV_R = 8, ENV_SPAN = ENV_R * 64, ENV_CHUNKS = (XN + ENV_SPAN - 1) / ENV_SPAN, ENV_THREADS = ENV_CHUNKS * 64;
constexpr int ENV_LO = 8;                               // ring: x[(i) mod N] at i + N + ENV_LO, i in [-N - ENV_LO, N)
constexpr int MEL_NFFT = 2048, MEL_HOP = 512, MEL_FRAMES = 1 + XN / MEL_HOP, MEL_BANDS = 128,
              MEL_BINS = 513;
static_assert(MEL_FRAMES == 10, "librosa frame count for 4800 samples, center=True");
static_assert(XN % ENV_R == 0, "whole output blocks");

// ---- envelope ---------------------------------------------------------------------------------------------------------------
// grid B*C x ENV_THREADS (a wave per chunk of 512 outputs; the 86 KB ring allows one workgroup per CU, so its waves are what
// hides the LDS latency): partial sum of (e_gt - e_pred)^2 over each chunk's outputs -> part[bc * ENV_CHUNKS + chunk]
__global__ __launch_bounds__(ENV_THREADS) void evalx_env_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int C,
                                                       float* __restrict__ part) {
    __shared__ float2 ring[2 * XN + ENV_LO];            // (pred, gt)
    __shared__ float4 taps[XH / 4];                      // g[1], g[3], ...
    const int bc = blockIdx.x, chunk = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = bc / C, c = bc - (bc / C) * C;
    const float* p = pred + (long)b * XN * C + c;
    const float* g = gt + (long)b * XN * C + c;
    for (int t = threadIdx.x; t < 2 * XN + ENV_LO; t += ENV_THREADS) {
        int i = t - ENV_LO;
        i = i < 0 ? i + XN : (i >= XN ? i - XN : i);
        ring[t] = make_float2(p[(long)i * C], g[(long)i * C]);
    }
    float* tapf = (float*)taps;
    for (int j = threadIdx.x; j < XH; j += ENV_THREADS) {
        double s, co;
        sincospi((double)(2 * j + 1) / (double)XN, &s, &co);
        tapf[j] = (float)(2.0 / XN * co / s);
    }
    __syncthreads();
    const int n0 = chunk * ENV_SPAN + lane * ENV_R;
    float d2 = 0.f;
    if (n0 < XN) {
        const float2* x = ring + XN + ENV_LO;           // x[i] for i in [-N - ENV_LO, N)
        float ap[ENV_R], ag[ENV_R];
        float2 w[ENV_R];                                // x[base + r], base = n0 - 1 - 2j
#pragma unroll
        for (int r = 0; r < ENV_R; ++r) { ap[r] = 0.f; ag[r] = 0.f; w[r] = x[n0 - 1 + r]; }
        for (int j = 0; j < XH; j += 4) {
            const float4 g4 = taps[j >> 2];
            const int base = n0 - 1 - 2 * j;
            float2 v[2 * ENV_R];                        // x[base - 8 .. base + 7]
#pragma unroll
            for (int r = 0; r < ENV_R; ++r) { v[r] = x[base - ENV_R + r]; v[ENV_R + r] = w[r]; }
            const float gu[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int r = 0; r < ENV_R; ++r) {       // tap k = 2(j+u)+1 on x[n0 + r - k] = v[8 - 2u + r]
                    ap[r] = fmaf(gu[u], v[ENV_R - 2 * u + r].x, ap[r]);
                    ag[r] = fmaf(gu[u], v[ENV_R - 2 * u + r].y, ag[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < ENV_R; ++r) w[r] = v[r];
        }
#pragma unroll
        for (int r = 0; r < ENV_R; ++r) {
            const float2 xv = x[n0 + r];
            const float ep = sqrtf(xv.x * xv.x + ap[r] * ap[r]), eg = sqrtf(xv.y * xv.y + ag[r] * ag[r]);
            d2 += (eg - ep) * (eg - ep);
        }
    }
    d2 = wave_sum(d2);
    if (lane == 0) part[bc * ENV_CHUNKS + chunk] = d2;
}

// ---- mel-LSD ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double slaney_hz(double m) {          // librosa mel_to_hz, htk=False
    return m < 15.0 ? m * (200.0 / 3.0) : 1000.0 * exp(log(6.4) / 27.0 * (m - 15.0));
}

// grid (B*C, MEL_FRAMES) x 256: sum over the 128 bands of (L_gt - L_pred)^2 of this frame -> part[bc * MEL_FRAMES + t]
__global__ __launch_bounds__(256) void evalx_mel_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int C,
                                                        float* __restrict__ part) {
    __shared__ float2 z[MEL_NFFT];
    __shared__ float2 tw[MEL_NFFT / 2];
    __shared__ float sp[MEL_BINS], sg[MEL_BINS];
    __shared__ float red[2];
    const int bc = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int b = bc / C, c = bc - (bc / C) * C;
    const float* p = pred + (long)b * XN * C + c;
    const float* g = gt + (long)b * XN * C + c;
    for (int k = tid; k < MEL_NFFT / 2; k += 256) {
        double s, co;
        sincospi(2.0 * k / MEL_NFFT, &s, &co);
        tw[k] = make_float2((float)co, (float)-s);                 // e^{-2 pi i k / 2048}
    }
    for (int n = tid; n < MEL_NFFT; n += 256) {
        int i = t * MEL_HOP + n - MEL_NFFT / 2;                    // numpy 'reflect' (edge sample not repeated)
        i = i < 0 ? -i : (i >= XN ? 2 * (XN - 1) - i : i);
        const float h = (float)(0.5 - 0.5 * cospi(2.0 * n / MEL_NFFT));
        z[__brev((unsigned)n) >> 21] = make_float2(h * p[(long)i * C], h * g[(long)i * C]);
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 11; ++s) {                                 // radix-2 DIT, span 2^s
        const int half = 1 << s;
        for (int q = tid; q < MEL_NFFT / 2; q += 256) {
            const int pos = q & (half - 1);
            const int i0 = ((q >> s) << (s + 1)) + pos, i1 = i0 + half;
            const float2 w = tw[pos << (10 - s)], a = z[i0], bb = z[i1];
            const float2 m = make_float2(w.x * bb.x - w.y * bb.y, w.x * bb.y + w.y * bb.x);
            z[i0] = make_float2(a.x + m.x, a.y + m.y);
            z[i1] = make_float2(a.x - m.x, a.y - m.y);
        }
        __syncthreads();
    }
    for (int f = tid; f < MEL_BINS; f += 256) {                    // Z = P + iG  ->  P_f = (Z_f + conj Z_-f) / 2, G_f = (Z_f - conj Z_-f) / 2i
        const float2 a = z[f], r = z[(MEL_NFFT - f) & (MEL_NFFT - 1)];
        const float pr = a.x + r.x, pi = a.y - r.y, gr = a.y + r.y, gi = a.x - r.x;
        sp[f] = 0.25f * (pr * pr + pi * pi);
        sg[f] = 0.25f * (gr * gr + gi * gi);
    }
    __syncthreads();
    float d2 = 0.f;
    if (tid < MEL_BANDS) {
        const double mtop = 15.0 + log(12000.0 / 1000.0) / (log(6.4) / 27.0);
        const double f0 = slaney_hz(mtop * tid / (MEL_BANDS + 1)), f1 = slaney_hz(mtop * (tid + 1) / (MEL_BANDS + 1)),
                     f2 = slaney_hz(mtop * (tid + 2) / (MEL_BANDS + 1));
        const double df = 48000.0 / MEL_NFFT, enorm = 2.0 / (f2 - f0);
        const int lo = max(0, (int)floor(f0 / df)), hi = min(MEL_BINS - 1, (int)ceil(f2 / df));
        double mp = 0.0, mg = 0.0;
        for (int f = lo; f <= hi; ++f) {
            const double nu = f * df;
            const double wgt = fmax(0.0, fmin((nu - f0) / (f1 - f0), (f2 - nu) / (f2 - f1))) * enorm;
            mp += wgt * sp[f];
            mg += wgt * sg[f];
        }
        const double d = 10.0 * log10(mg + 0.01) - 10.0 * log10(mp + 0.01);
        d2 = (float)(d * d);
    }
    if (tid < MEL_BANDS) {
        d2 = wave_sum(d2);
        if ((tid & 63) == 0) red[tid >> 6] = d2;
    }
    __syncthreads();
    if (tid == 0) part[bc * MEL_FRAMES + t] = red[0] + red[1];
}

// one lane per (window, channel): the per-sample values from the partial sums, in a fixed order
__global__ __launch_bounds__(64) void evalx_finish_kernel(const float* __restrict__ env_part, const float* __restrict__ mel_part, int n,
                                                          float* __restrict__ mel_lsd, float* __restrict__ env_mse) {
    const int bc = blockIdx.x * 64 + threadIdx.x;
    if (bc >= n) return;
    double se = 0.0, sm = 0.0;
    for (int k = 0; k < ENV_CHUNKS; ++k) se += env_part[bc * ENV_CHUNKS + k];
    for (int k = 0; k < MEL_FRAMES; ++k) sm += mel_part[bc * MEL_FRAMES + k];
    env_mse[bc] = (float)sqrt(se / XN);
    mel_lsd[bc] = (float)sqrt(sm / (MEL_BANDS * MEL_FRAMES));
}

size_t evalx_scratch_floats(int B, int C) { return (size_t)B * C * (ENV_CHUNKS + MEL_FRAMES); }

int evalx_mel_env_launch(const float* pred, const float* gt, int B, int C, float* mel_lsd, float* env_mse, float* scratch,
                         hipStream_t s) {
    float* env_part = scratch;
    float* mel_part = scratch + (size_t)B * C * ENV_CHUNKS;
    hipLaunchKernelGGL(evalx_env_kernel, dim3(B * C), dim3(ENV_THREADS), 0, s, pred, gt, C, env_part);
    SAGEN_LAUNCH_CHECK();
    hipLaunchKernelGGL(evalx_mel_kernel, dim3(B * C, MEL_FRAMES), dim3(256), 0, s, pred, gt, C, mel_part);
    SAGEN_LAUNCH_CHECK();
    hipLaunchKernelGGL(evalx_finish_kernel, dim3(cdiv((long)B * C, 64)), dim3(64), 0, s, env_part, mel_part, B * C, mel_lsd, env_mse);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// ---- EMD ----------------------------------------------------------------------------------------------------------------------
// the device "wave" of emd_core.h: 64 lanes, DPP / permlane butterflies, ballots for the ordered lists
struct EmdWave {
    static constexpr int WIDTH = 64;
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void argmin(double& d, int& i) const { wave_argmin_f64(d, i); }
    __device__ double sum(double v) const { return wave_sum_f64(v); }
    __device__ double max(double v) const { return wave_max_f64(v); }
    __device__ int any(bool b) const { return __ballot(b) != 0ull; }
    __device__ int prefix(bool f, int& count) const {
        const unsigned long long m = __ballot(f);
        const int p = count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        count += __popcll(m);
        return p;
    }
};

// grid (n_maps, 2) x 64: variant 0 = dir (P = p / nodes), 1 = dir2 (P = p / (sum p + 0.01))  (distance.py:128-129)
__global__ __launch_bounds__(64) void evalx_emd_kernel(const float* __restrict__ pm, const float* __restrict__ qm, int nodes,
                                                       const double* __restrict__ cost, double* __restrict__ out,
                                                       unsigned int* __restrict__ not_converged) {
    __shared__ EmdState st;
    __shared__ double P[EMD_MAX_NODES], Q[EMD_MAX_NODES];
    const EmdWave w;
    const int m = blockIdx.x, var = blockIdx.y, lane = threadIdx.x;
    const float* p = pm + (long)m * nodes;
    const float* q = qm + (long)m * nodes;
    double sp = 0.0, sq = 0.0;
    for (int v = lane; v < nodes; v += 64) { sp += (double)p[v]; sq += (double)q[v]; }
    sp = w.sum(sp); sq = w.sum(sq);
    const double np_ = var == 0 ? (double)nodes : sp + 0.01, nq = var == 0 ? (double)nodes : sq + 0.01;
    for (int v = lane; v < nodes; v += 64) { P[v] = (double)p[v] / np_; Q[v] = (double)q[v] / nq; }
    __syncthreads();
    int conv = 1;
    const double r = emd_hat(w, st, P, Q, nodes, cost, &conv);
    if (lane == 0) {
        out[m * 2 + var] = r;
        if (!conv) atomicAdd(not_converged, 1u);
    }
}

int run_eval_emd(const float* p, const float* q, int n_maps, int nodes, const double* cost, double* out, uint32_t* not_converged, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(evalx_emd_kernel, dim3(n_maps, 2), dim3(64), 0, s, p, q, nodes, cost, out, not_converged);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
