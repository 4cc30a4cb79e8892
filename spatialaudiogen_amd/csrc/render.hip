// Ambisonic rendering (gfx950): one rotated FIR matrix serves every rendering of the reference's output stage - the W+-Y
// fold-down (myutils.py:289), AmbiDecoder.decode (decoder.py:24-28), DirectAmbisonicBinauralizer (binauralizer.py:156-166),
// VirtualStereoMic (:18-36) and Convolvotron (:63-76) behind AmbisonicBinauralizer (:124-153) - see include/sagen.h.
//
//   x'[s]   = M(s) . x[s],   M(s) = (1 - a) R[m] + a R[min(m + 1, n_rot - 1)]   (R absent: the identity)
//   y[t, o] = sum_c sum_k H[o, c, k] x'[t - k, c]
//
// A workgroup takes RENDER_T consecutive output samples for all outputs.  It stages them and the K - 1 rows before
// them into LDS (zero where the stream has no row), one plane per channel, applying M(s) on the way in.  One work item = (output o, 512 consecutive samples): a wave
// per item, a lane per 8 consecutive samples, the taps wave-uniform (scalar operands).  A lane keeps a window of 12 consecutive
// samples of the current plane in registers: four taps x eight samples = 32 FMAs per 16-byte LDS read.
//
// ORDER OF THE SUM, fixed per output sample whatever tile or call it falls into: one fp32 accumulator, channels outermost
// (c = 0 .. C-1), taps ascending inside (k = 0 .. 4 * ceil(K / 4) - 1, the taps past K - 1 being zeros), one fmaf each.  A stream
// rendered in pieces therefore gives the bits of the one-call result.
#include "kernels.h"

namespace sagen {

namespace {

constexpr int RENDER_T = 1024;            // output samples per workgroup
constexpr int RENDER_J = 8;               // consecutive output samples per lane
constexpr int RENDER_ITEM = 64 * RENDER_J;    // output samples per work item (one wave)
constexpr int RENDER_NB = RENDER_T / RENDER_ITEM;

struct RenderArgs {
    long long n_hist, n, pos0, zero_before;
    int outputs, ntaps, n_rot, rot_hop;
};

// acc[j] += h[d] * x[t0 + j - (k0 + d)], d = 0..3 ascending: w[i] = x[t0 - 3 - k0 + i]
__device__ __forceinline__ void fir_block(float (&acc)[RENDER_J], const float (&w)[12], float h0, float h1, float h2, float h3) {
#pragma unroll
    for (int j = 0; j < RENDER_J; ++j) {
        float a = acc[j];
        a = fmaf(h0, w[j + 3], a);
        a = fmaf(h1, w[j + 2], a);
        a = fmaf(h2, w[j + 1], a);
        a = fmaf(h3, w[j], a);
        acc[j] = a;
    }
}

template <int C>
__global__ __launch_bounds__(256) void render_fir_kernel(const float* __restrict__ x,        // [n_hist + n][C]
                                                         const float* __restrict__ taps,     // [O][C][K]: wave-uniform, read by scalar loads
                                                         const float* __restrict__ rot,      // [n_rot][C][C] or null
                                                         float* __restrict__ y,              // [n][O]
                                                         const RenderArgs a) {
    extern __shared__ float4 render_lds4[];
    float* lds = (float*)render_lds4;
    const int K = a.ntaps, Kb = (K + 3) >> 2;
    const int OFF = 4 * Kb + 3;              // plane index of the tile's first output sample (OFF % 4 == 3: every window read is 16-byte aligned)
    const int PS = 4 * Kb + 8 + RENDER_T;    // plane stride: four zero slots in front (the read-ahead of the last tap block), zeros up to the
                                             // first row the taps reach, the rows, four more slots (the last one read into a window, never used)
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * RENDER_T;     // of the tile, among the n new rows
    const long long n_rows = a.n_hist + a.n;

    // ---- stage: plane c, slot i holds x'[s][c] of the absolute position s = pos0 + row0 + i - OFF; zero where the stream has no row
    for (int i = tid; i < PS; i += 256) {
        const int q = i - OFF;
        const long long s = a.pos0 + row0 + q;
        const long long r = a.n_hist + row0 + q;                 // row of the x buffer
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.f;
        if (q >= -(K - 1) && q < RENDER_T && s >= 0 && r >= 0 && r < n_rows) {
            if (C == 4) {
                const float4 t = *(const float4*)(x + r * 4);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = x[r * C + c];
            }
            if (rot) {
                long long m = s / a.rot_hop;
                if (m > a.n_rot - 1) m = a.n_rot - 1;
                const long long m1 = m + 1 < a.n_rot ? m + 1 : m;
                // at and past the last control point the last matrix is HELD: a = 0 there, so that M = R[n_rot - 1] exactly (the unclamped
                // (s - m hop) / hop would grow with the stream position and with it the fp32 error of (1 - a) R + a R)
                const float al = m1 == m ? 0.f : (float)(s - m * a.rot_hop) / (float)a.rot_hop, be = 1.f - al;
                const float* r0 = rot + m * (C * C);
                const float* r1 = rot + m1 * (C * C);
                float u[C];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float acc = 0.f;
#pragma unroll
                    for (int e = 0; e < C; ++e) acc = fmaf(fmaf(al, r1[c * C + e], be * r0[c * C + e]), v[e], acc);
                    u[c] = acc;
                }
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = u[c];
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) lds[c * PS + i] = v[c];
    }
    __syncthreads();

    // ---- contract: wave w takes the items w, w + 4, ...
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n_items = a.outputs * RENDER_NB;
    const int full = K >> 2;                 // tap blocks without a tap past K - 1
    for (int item = wave; item < n_items; item += 4) {
        const int o = item / RENDER_NB, t0 = (item % RENDER_NB) * RENDER_ITEM + lane * RENDER_J;
        if (row0 + (item % RENDER_NB) * RENDER_ITEM >= a.n) continue;       // (wave-uniform) nothing of this item is stored
        float acc[RENDER_J];
#pragma unroll
        for (int j = 0; j < RENDER_J; ++j) acc[j] = 0.f;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            const float4* p = (const float4*)(lds + c * PS + t0) + Kb;            // window of tap block 0: slots t0 + 4 Kb .. t0 + 4 Kb + 11
            const float* h = taps + ((long)o * C + c) * K;
            float w[12];
            {
                const float4 w0 = p[0], w1 = p[1], w2 = p[2];
                w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w;
                w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
                w[8] = w2.x; w[9] = w2.y; w[10] = w2.z; w[11] = w2.w;
            }
            // three tap blocks per step, software-pipelined: the 12 taps and the 12 window samples of the NEXT step are requested before
            // the 96 FMAs of this one, so neither the scalar loads nor the LDS reads are waited for with nothing to do
            const int n3 = full / 3;
            float hc[12];
            if (n3 > 0) {
#pragma unroll
                for (int i = 0; i < 12; ++i) hc[i] = h[i];
            }
#pragma unroll 2
            for (int g = 0; g < n3; ++g) {
                const int kb = 3 * g;
                const float4 n0 = p[-(kb + 1)], n1 = p[-(kb + 2)], n2 = p[-(kb + 3)];
                float hn[12];
                const float* hp = h + (g + 1 < n3 ? 12 * (g + 1) : 0);       // (the last step re-reads the first taps: no branch, never used)
#pragma unroll
                for (int i = 0; i < 12; ++i) hn[i] = hp[i];
                fir_block(acc, w, hc[0], hc[1], hc[2], hc[3]);
                const float w1[12] = {n0.x, n0.y, n0.z, n0.w, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
                fir_block(acc, w1, hc[4], hc[5], hc[6], hc[7]);
                const float w2[12] = {n1.x, n1.y, n1.z, n1.w, n0.x, n0.y, n0.z, n0.w, w[0], w[1], w[2], w[3]};
                fir_block(acc, w2, hc[8], hc[9], hc[10], hc[11]);
                w[0] = n2.x; w[1] = n2.y; w[2] = n2.z; w[3] = n2.w;
                w[4] = n1.x; w[5] = n1.y; w[6] = n1.z; w[7] = n1.w;
                w[8] = n0.x; w[9] = n0.y; w[10] = n0.z; w[11] = n0.w;
#pragma unroll
                for (int i = 0; i < 12; ++i) hc[i] = hn[i];
            }
            for (int kb = 3 * n3; kb < full; ++kb) {
                const float4 nx = p[-(kb + 1)];          // the four samples tap block kb + 1 adds to the window
                fir_block(acc, w, h[4 * kb], h[4 * kb + 1], h[4 * kb + 2], h[4 * kb + 3]);
#pragma unroll
                for (int i = 11; i >= 4; --i) w[i] = w[i - 4];
                w[0] = nx.x; w[1] = nx.y; w[2] = nx.z; w[3] = nx.w;
            }
            if (full < Kb) {                 // the last block: taps past K - 1 are zeros
                const int k0 = 4 * full;
                fir_block(acc, w, h[k0], k0 + 1 < K ? h[k0 + 1] : 0.f, k0 + 2 < K ? h[k0 + 2] : 0.f, 0.f);
            }
        }
        const long long t_abs = a.pos0 + row0 + t0;
#pragma unroll
        for (int j = 0; j < RENDER_J; ++j) {
            const long long row = row0 + t0 + j;
            if (row < a.n) y[row * a.outputs + o] = t_abs + j < a.zero_before ? 0.f : acc[j];
        }
    }
}

size_t render_fir_lds_bytes(int channels, int ntaps) {
    return (size_t)channels * (4 * ((ntaps + 3) / 4) + 8 + RENDER_T) * sizeof(float);
}

}  // namespace

int run_render_fir(const float* x, int64_t n_hist, int64_t n, int channels, const float* taps, int outputs, int ntaps, const float* rot,
                   int n_rot, int rot_hop, int64_t pos0, int64_t zero_before, float* y, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    RenderArgs a;
    a.n_hist = n_hist; a.n = n; a.pos0 = pos0; a.zero_before = zero_before;
    a.outputs = outputs; a.ntaps = ntaps; a.n_rot = n_rot; a.rot_hop = rot_hop;
    const dim3 grid(cdiv(n, RENDER_T));
    const size_t lds = render_fir_lds_bytes(channels, ntaps);      // <= 9 * (512 + 8 + 1024) * 4 = 55 584 bytes
    if (channels == 4)
        hipLaunchKernelGGL(render_fir_kernel<4>, grid, dim3(256), lds, s, x, taps, rot, y, a);
    else
        hipLaunchKernelGGL(render_fir_kernel<9>, grid, dim3(256), lds, s, x, taps, rot, y, a);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
