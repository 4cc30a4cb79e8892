// HBM-bound kernels of the path: batch-norm statistics finalisation, BN+ReLU(+residual),
// BN+ReLU+max-pool, input padding, ambisonic power map, output assembly.  All are
// 16-byte-per-lane coalesced NHWC streams (channels innermost, C % 4 == 0).
#include "kernels.h"

namespace sagen {

// -----------------------------------------------------------------------------------------
// contrib batch_norm, training mode (core.py:6,209-210): per-tile partial (sum, sumsq) ->
// scale = gamma / sqrt(var + eps), shift = beta - mean * scale; biased variance.
// The producers (conv epilogue / split-K reduce) accumulate per-channel (sum, sumsq) with fp64 atomics.
// -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void bn_finalize_kernel(const double* __restrict__ acc, double inv_count, int C,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double mean = acc[c] * inv_count;
    double var = acc[C + c] * inv_count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double sc = (double)gamma[c] / sqrt(var + (double)eps);
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - mean * sc);
}

int bn_finalize_launch(const double* stats, long count, int C, const float* gamma, const float* beta, float eps,
                       float* scale, float* shift, hipStream_t s) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, stats, 1.0 / (double)count, C, gamma, beta, eps,
                       scale, shift);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// scale/shift of 4 consecutive channels: from arrays, or derived from a producer's fp64 (sum, sumsq) accumulators
__device__ __forceinline__ void bn_coeffs4(const float4* scale, const float4* shift, const BnRef& bn, int C4, int c4,
                                           float4& sc, float4& sh) {
    if (bn.acc != nullptr) {
        float s4[4], h4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * c4 + k;
            const double mean = bn.acc[c] * bn.inv_count;
            double var = bn.acc[4 * C4 + c] * bn.inv_count - mean * mean;
            var = var < 0.0 ? 0.0 : var;
            const double a = (double)bn.gamma[c] / sqrt(var + (double)bn.eps);
            s4[k] = (float)a;
            h4[k] = (float)((double)bn.beta[c] - mean * a);
        }
        sc = make_float4(s4[0], s4[1], s4[2], s4[3]);
        sh = make_float4(h4[0], h4[1], h4[2], h4[3]);
    } else if (scale != nullptr) {
        sc = scale[c4];
        sh = shift[c4];
    } else {
        sc = make_float4(1.f, 1.f, 1.f, 1.f);
        sh = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// y = relu(x*scale[c] + shift[c] (+ residual))   (resnet.py:221,235)
__global__ __launch_bounds__(256) void bn_apply_relu_kernel(const float4* __restrict__ x, const float4* __restrict__ scale,
                                                            const float4* __restrict__ shift, const BnRef bn,
                                                            const float4* __restrict__ res, float4* __restrict__ y,
                                                            long n4, int C4) {
    // the grid stride is a multiple of C4 (launcher), so a thread always sees the same 4 channels
    float4 sc, sh;
    bn_coeffs4(scale, shift, bn, C4, (int)(((long)blockIdx.x * 256 + threadIdx.x) % C4), sc, sh);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = x[i];
        v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
        v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
        if (res) {
            const float4 r = res[i];
            v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
        }
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        y[i] = v;
    }
}

// grid whose stride (grid*256 threads) is a multiple of C4, so per-thread channel groups are loop-invariant
static int channel_aligned_grid(long n4, int C4) {
    long g = std::min<long>(cdiv(n4, 256), 256L * 16);
    if ((g * 256) % C4) {
        long unit = C4;                       // smallest g with (g*256) % C4 == 0 is C4 / gcd(256, C4)
        for (long a = 256, b = C4; b;) { const long t = a % b; a = b; b = t; unit = C4 / a; }
        g = std::max<long>(unit, g / unit * unit);
    }
    return (int)g;
}

int bn_apply_relu_launch(const float* x, const float* scale, const float* shift, const BnRef& bn, const float* residual,
                         float* y, long n_pixels, int C, hipStream_t s) {
    if (C % 4) return fail(SAGEN_ERR_UNSUPPORTED, "bn_apply_relu: C=%d must be a multiple of 4", C);
    const long n4 = n_pixels * (C / 4);
    const int grid = channel_aligned_grid(n4, C / 4);
    hipLaunchKernelGGL(bn_apply_relu_kernel, dim3(grid), dim3(256), 0, s, (const float4*)x, (const float4*)scale,
                       (const float4*)shift, bn, (const float4*)residual, (float4*)y, n4, C / 4);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// tf.nn.max_pool(x,[1,3,3,1],[1,2,2,1],'SAME') (resnet.py:135) of relu(bn(x)); TF SAME pads
// (0 before, 1 after) for even H/W -> window rows 2*ho .. 2*ho+2 clipped at the border (-inf pad).
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float4* __restrict__ x, const float4* __restrict__ scale,
                                                           const float4* __restrict__ shift, const BnRef bn,
                                                           float4* __restrict__ y,
                                                           int B, int H, int W, int C4, int Ho, int Wo, int pt, int pl) {
    const long total = (long)B * Ho * Wo * C4;
    float4 sc, sh;
    bn_coeffs4(scale, shift, bn, C4, (int)(((long)blockIdx.x * 256 + threadIdx.x) % C4), sc, sh);
    const bool has_bn = scale != nullptr || bn.acc != nullptr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % Wo); p /= Wo;
        const int ho = (int)(p % Ho);
        const int b = (int)(p / Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int h = ho * 2 + dy - pt;
            if ((unsigned)h >= (unsigned)H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int w = wo * 2 + dx - pl;
                if ((unsigned)w >= (unsigned)W) continue;
                float4 v = x[(((long)b * H + h) * W + w) * C4 + c];
                v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
                v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        if (has_bn) {   // relu commutes with max
            m.x = fmaxf(m.x, 0.f); m.y = fmaxf(m.y, 0.f); m.z = fmaxf(m.z, 0.f); m.w = fmaxf(m.w, 0.f);
        }
        y[i] = m;
    }
}

int maxpool3x3s2_launch(const float* x, const float* scale, const float* shift, const BnRef& bn, float* y, int B, int H,
                        int W, int C, hipStream_t s) {
    if (C % 4) return fail(SAGEN_ERR_UNSUPPORTED, "maxpool: C=%d must be a multiple of 4", C);
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const int pth = std::max((Ho - 1) * 2 + 3 - H, 0), ptw = std::max((Wo - 1) * 2 + 3 - W, 0);
    const long total = (long)B * Ho * Wo * (C / 4);
    const int grid = channel_aligned_grid(total, C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid), dim3(256), 0, s, (const float4*)x, (const float4*)scale,
                       (const float4*)shift, bn, (float4*)y, B, H, W, C / 4, Ho, Wo, pth / 2, ptw / 2);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// [B,H,W,3] -> [B,H+pt+pb,W+pl+pr,4] with zero border and zero 4th channel: the 7x7/2 SAME conv of
// ResNet18 (resnet.py:133) then runs as a VALID conv over 16-byte pixels.
__global__ __launch_bounds__(256) void pad_nhwc3to4_kernel(const float* __restrict__ x, float4* __restrict__ y, int B, int H,
                                                           int W, int Hp, int Wp, int pt, int pl) {
    const long total = (long)B * Hp * Wp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long p = i;
        const int w = (int)(p % Wp) - pl; p /= Wp;
        const int h = (int)(p % Hp) - pt;
        const int b = (int)(p / Hp);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
            const float* src = x + (((long)b * H + h) * W + w) * 3;
            v.x = src[0]; v.y = src[1]; v.z = src[2];
        }
        y[i] = v;
    }
}

// the same from uint8 frames, with the reference's pixel normalisation x / 255. - 0.5 (myutils.py:88-89, applied by the feeder to
// the decoded uint8 frame in double precision and stored as float32) fused in: the host ships 1 byte per sample instead of 4
__global__ __launch_bounds__(256) void pad_u8_nhwc3to4_kernel(const unsigned char* __restrict__ x, float4* __restrict__ y, int B, int H,
                                                              int W, int Hp, int Wp, int pt, int pl) {
    const long total = (long)B * Hp * Wp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long p = i;
        const int w = (int)(p % Wp) - pl; p /= Wp;
        const int h = (int)(p % Hp) - pt;
        const int b = (int)(p / Hp);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
            const unsigned char* src = x + (((long)b * H + h) * W + w) * 3;
            v.x = (float)((double)src[0] / 255.0 - 0.5); v.y = (float)((double)src[1] / 255.0 - 0.5); v.z = (float)((double)src[2] / 255.0 - 0.5);
        }
        y[i] = v;
    }
}

int pad_u8_nhwc3to4_launch(const unsigned char* x, float* y, int B, int H, int W, int pt, int pb, int pl, int pr, hipStream_t s) {
    const int Hp = H + pt + pb, Wp = W + pl + pr;
    const long total = (long)B * Hp * Wp;
    const int grid = (int)std::min<long>(cdiv(total, 256), 256L * 16);
    hipLaunchKernelGGL(pad_u8_nhwc3to4_kernel, dim3(grid), dim3(256), 0, s, x, (float4*)y, B, H, W, Hp, Wp, pt, pl);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int pad_nhwc3to4_launch(const float* x, float* y, int B, int H, int W, int pt, int pb, int pl, int pr, hipStream_t s) {
    const int Hp = H + pt + pb, Wp = W + pl + pr;
    const long total = (long)B * Hp * Wp;
    const int grid = (int)std::min<long>(cdiv(total, 256), 256L * 16);
    hipLaunchKernelGGL(pad_nhwc3to4_kernel, dim3(grid), dim3(256), 0, s, x, (float4*)y, B, H, W, Hp, Wp, pt, pl);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// deploy.py:143-152: [mono[b, snd_contx/2 + n] | Y Z X]
__global__ __launch_bounds__(256) void assemble_wyzx_kernel(const float* __restrict__ audio, const float* __restrict__ yzx,
                                                            float4* __restrict__ out, int B, int snd_size, int ss,
                                                            int snd_dur) {
    const long total = (long)B * snd_dur;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int b = (int)(i / snd_dur), n = (int)(i - (long)b * snd_dur);
        const float* p = yzx + i * 3;
        out[i] = make_float4(audio[(long)b * snd_size + ss + n], p[0], p[1], p[2]);
    }
}

int assemble_wyzx_launch(const float* audio, const float* yzx, float* out, int B, int snd_size, int snd_contx,
                         int snd_dur, hipStream_t s) {
    const long total = (long)B * snd_dur;
    hipLaunchKernelGGL(assemble_wyzx_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, audio, yzx, (float4*)out, B,
                       snd_size, snd_contx / 2, snd_dur);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// NO_SEPARATION (model.py:274-280, 430): x_sep = mono crop; one track
__global__ __launch_bounds__(256) void nosep_mix_kernel(const float* __restrict__ audio, const float* __restrict__ coeffs,
                                                        float* __restrict__ out, int B, int snd_size, int ss, int snd_dur,
                                                        int num_out) {
    const long total = (long)B * snd_dur * num_out;
    const int step_len = snd_dur / 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int o = (int)(i % num_out);
        long p = i / num_out;
        const int n = (int)(p % snd_dur);
        const int b = (int)(p / snd_dur);
        const float* cf = coeffs + (((long)b * 3 + n / step_len) * num_out + o) * 2;   // [B,3,o,(w,bias)]
        out[i] = fmaf(cf[0], audio[(long)b * snd_size + ss + n], cf[1]);
    }
}

int nosep_mix_launch(const float* audio, const float* coeffs, float* out, int B, int snd_size, int snd_contx,
                     int snd_dur, int num_out, hipStream_t s) {
    const long total = (long)B * snd_dur * num_out;
    hipLaunchKernelGGL(nosep_mix_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, audio, coeffs, out, B, snd_size,
                       snd_contx / 2, snd_dur, num_out);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// 'none' separation at NIN > 1 input channels (model.py:274-280, 428-430): x_sep = mono[:, :, ss:ss+dur] gets a new axis 1, i.e.
// [B, 1 track, NIN, dur], and after the transpose of model.py:421 the decoder's product broadcasts the NIN audio channels against
// the ONE track axis of the weights [B, dur, NOUT, NIN, 1]:  out[b,n,o] = (sum_i w[b,s,o,i,0]) * (sum_c audio[b,ss+n,c]) + w[b,s,o,0,1].
// coeffs [B, 3, NOUT, NIN, 2]; audio [B, snd_size, NIN] interleaved.
__global__ __launch_bounds__(256) void nosep_mix_multi_kernel(const float* __restrict__ audio, const float* __restrict__ coeffs,
                                                              float* __restrict__ out, int B, int snd_size, int ss, int snd_dur,
                                                              int nin, int num_out) {
    const long total = (long)B * snd_dur * num_out;
    const int step_len = snd_dur / 3;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int o = (int)(idx % num_out);
        const long p = idx / num_out;
        const int n = (int)(p % snd_dur);
        const int b = (int)(p / snd_dur);
        const float* cf = coeffs + (((long)b * 3 + n / step_len) * num_out + o) * nin * 2;
        const float* a = audio + ((long)b * snd_size + ss + n) * nin;
        float ws = 0.f, as = 0.f;
        for (int i = 0; i < nin; ++i) { ws += cf[2 * i]; as += a[i]; }
        out[idx] = fmaf(ws, as, cf[1]);
    }
}

int nosep_mix_multi_launch(const float* audio, const float* coeffs, float* out, int B, int snd_size, int snd_contx,
                           int snd_dur, int nin, int num_out, hipStream_t s) {
    const long total = (long)B * snd_dur * num_out;
    hipLaunchKernelGGL(nosep_mix_multi_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, audio, coeffs, out, B, snd_size,
                       snd_contx / 2, snd_dur, nin, num_out);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// Ambisonic power map (decoder.py:24-28 'projection', distance.py:41-52):
// rms[p] = sqrt(mean_t (sum_c ambi[t,c] * sh[p,c])^2).  Expanded as the 4x4 second-moment matrix
// S = sum_t ambi^T ambi (one wavefront-reduced pass over the audio, DPP/shuffle tree), then
// rms[p] = sqrt(sh[p] S sh[p]^T / T) — the audio is read exactly once whatever the mesh size.
// The ten moments are summed in fp64 from the first addition on (products of float32 values are exact there): the quadratic form
// cancels to zero opposite a plane wave, and float32 sums left 1e-4 of the map's maximum at that null
// ("The evaluation side op by op"; overlay_moments_kernel sums the same way).
__device__ __forceinline__ void moments_add(double (&m)[10], const float4 a4) {
    const double a[4] = {a4.x, a4.y, a4.z, a4.w};
    m[0] += a[0] * a[0]; m[1] += a[0] * a[1]; m[2] += a[0] * a[2]; m[3] += a[0] * a[3];
    m[4] += a[1] * a[1]; m[5] += a[1] * a[2]; m[6] += a[1] * a[3];
    m[7] += a[2] * a[2]; m[8] += a[2] * a[3]; m[9] += a[3] * a[3];
}

// sum of the 256 threads' moments, in one fixed order (wave butterflies, then the four waves): moment threadIdx.x in threads 0..9
__device__ __forceinline__ double moments_block_sum(const double (&m)[10]) {
    __shared__ double red[4][10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const double v = wave_sum_f64(m[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    return threadIdx.x < 10 ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : 0.0;
}

__global__ __launch_bounds__(256) void power_moments_kernel(const float4* __restrict__ ambi, long T, double* __restrict__ S) {
    double m[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = 0.0;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < T; t += (long)gridDim.x * 256) moments_add(m, ambi[t]);
    const double v = moments_block_sum(m);
    if (threadIdx.x < 10) atomicAdd(&S[threadIdx.x], v);
}

__global__ __launch_bounds__(256) void power_map_kernel(const double* __restrict__ S, double inv_T, const float4* __restrict__ sh,
                                                        int P, float* __restrict__ rms) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 y = sh[p];
    const double v[4] = {y.x, y.y, y.z, y.w};
    const double s[4][4] = {{S[0], S[1], S[2], S[3]}, {S[1], S[4], S[5], S[6]}, {S[2], S[5], S[7], S[8]}, {S[3], S[6], S[8], S[9]}};
    double e = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) e += v[i] * s[i][j] * v[j];
    rms[p] = (float)sqrt(fmax(e, 0.0) * inv_T);
}

// One map per chunk of T samples, `nchunks` chunks back to back (SphericalAmbisonicsVisualizer.loop_frames,
// distance.py:41-59: one RMS map per 0.1 s window): block b reduces the second moments of chunk b (no atomics).
__global__ __launch_bounds__(256) void power_moments_batched_kernel(const float4* __restrict__ ambi, long T, double* __restrict__ S) {
    const float4* a4 = ambi + (long)blockIdx.x * T;
    double m[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) m[k] = 0.0;
    for (long t = threadIdx.x; t < T; t += 256) moments_add(m, a4[t]);
    const double v = moments_block_sum(m);
    if (threadIdx.x < 10) S[(long)blockIdx.x * 10 + threadIdx.x] = v;
}

__global__ __launch_bounds__(256) void power_map_batched_kernel(const double* __restrict__ Sall, double inv_T, const float4* __restrict__ sh,
                                                                int P, float* __restrict__ rms) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double* S = Sall + (long)blockIdx.y * 10;
    const float4 y = sh[p];
    const double v[4] = {y.x, y.y, y.z, y.w};
    const double s[4][4] = {{S[0], S[1], S[2], S[3]}, {S[1], S[4], S[5], S[6]}, {S[2], S[5], S[7], S[8]}, {S[3], S[6], S[8], S[9]}};
    double e = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) e += v[i] * s[i][j] * v[j];
    rms[(long)blockIdx.y * P + p] = (float)sqrt(fmax(e, 0.0) * inv_T);
}

int power_map_batched_launch(const float* ambi, int nchunks, long T, const float* sh, int P, float* rms, double* moments, hipStream_t s) {
    hipLaunchKernelGGL(power_moments_batched_kernel, dim3(nchunks), dim3(256), 0, s, (const float4*)ambi, T, moments);
    SAGEN_LAUNCH_CHECK();
    hipLaunchKernelGGL(power_map_batched_kernel, dim3(cdiv(P, 256), nchunks), dim3(256), 0, s, moments, 1.0 / (double)T, (const float4*)sh, P, rms);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// scratch for the moments lives at the head of rms' caller-provided buffer? No: keep it explicit.
int power_map_launch(const float* ambi, long T, const float* sh, int P, float* rms, hipStream_t s) {
    // 10 doubles of scratch are taken from a static per-device buffer allocated lazily would break
    // the "no allocation" rule; instead the caller's rms buffer must hold P floats + 32 extra floats
    // (documented in sagen.h): the moments are accumulated in rms[P .. P+20).
    double* S = reinterpret_cast<double*>(rms + ((P + 1) / 2) * 2);
    SAGEN_HIP_CHECK(hipMemsetAsync(S, 0, 10 * sizeof(double), s));
    const int grid = (int)std::min<long>(cdiv(T, 256), 1024L);
    hipLaunchKernelGGL(power_moments_kernel, dim3(grid), dim3(256), 0, s, (const float4*)ambi, T, S);
    SAGEN_LAUNCH_CHECK();
    hipLaunchKernelGGL(power_map_kernel, dim3(cdiv(P, 256)), dim3(256), 0, s, S, 1.0 / (double)T, (const float4*)sh, P, rms);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
