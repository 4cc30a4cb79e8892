// conv3h_kernel: conv3p_kernel (dense 3x3 stride-1 SAME convolution over pre-split activation planes; reference op tf.nn.convolution,
// core.py:206, as the ResNet18 trunk uses it: resnet.py:141-190 / 215-235) on TWO fp16 planes per operand instead of three bf16
// planes - three matrix products per fp32 product instead of six, 4 instead of 6 bytes per operand element.
//
// Arithmetic ("fp16x2").  An fp32 value v with |v| in fp16's NORMAL range splits as
//     hi = rne_f16(v),  lo = rne_f16(v - hi)            (v - hi is exact in fp32)
// into 11 + 11 significant bits plus the sign of the residual: |v - hi - lo| <= 2^-23.5 |v| - fp32's own resolution.  The product
// a*b is evaluated as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation; the dropped lo*lo is below 2^-22
// relative.  bf16 was chosen for the general kernels because it has fp32's EXPONENT range; fp16 does not (normal range 6.1e-5 ..
// 65504, below that the absolute resolution stays at 2^-25 - v_mfma honours fp16 subnormals: tools/probe/f16_denorm.hip), so this
// kernel is used only where the operands' magnitudes are known, and both are scaled into the middle of that range by exact powers
// of two:
//   * filters: per layer, 2^kw with max |w| 2^kw in [512, 1024) (h2_filter_pack: absmax on the device, planes [K/16][2][N][16]);
//   * activations: the plane-writing pass (p3.hip, format 1) derives 2^ka from STATISTICS the forward already holds - channel c of
//     relu(bn(y)) has mean beta_c and standard deviation |gamma_c| sqrt(var_c / (var_c + eps)); the residual branch of a block merge adds
//     the bound of the block input (tracked from pass to pass) or, behind a 1x1 projection, |mean| + 8 sigma of the projection's output
//     (its conv accumulates (sum, sumsq) like the batch-norm convs do): bound = max_c(|beta_c| + 8 std_c) [+ residual bound] is scaled
//     into [512, 1024) and the planes saturate at +-65000 - 64 times beyond eight standard deviations; exact zeros (ReLU) stay exact.
// The epilogue multiplies the tile by 2^-(ka + kw) (exact).  Measured against an fp64 evaluation of the network this path is as accurate as the
// six-product bf16x3 path (fewer products = fewer fp32 accumulation roundings): DESIGN.md 3.2, profiles/r04_accuracy_modes.jsonl.
//
// Everything else is conv3p_kernel: P layout [Cin/16][NP][2 planes][16 ch] fp16 (64 B per pixel and chunk), NP = B*H*(W+1) with one
// zero pixel closing every image row; K order (dh, chunk, dw): per group the workgroup stages the activation tile once (with one
// halo pixel either side) and the three dw filter tiles by LDS-DMA; fragments by ds_read_b128; two-stage ring; one barrier per
// group.  The LDS image of a slot is 64 B = four 16-byte units (plane, half); unit u of slot s sits at position u ^ ((s >> 2) & 3):
// the 16 lanes of one ds_read_b128 group then cover all 64 banks for ANY slot base (with 96-byte slots conv3p_kernel needs only the
// half swap).  40 KiB of LDS per 128x64 workgroup: three per CU.
#include "conv3h_body.h"

namespace sagen {

template <int BM, int BN, int WM, int WN, int KC>
__global__ __launch_bounds__(256, conv3h_wgs_per_cu(BM, BN, KC, 2)) void conv3h_kernel(const IgemmDesc d_in) {
    IgemmDesc d = d_in;
    if (d.grp.G > 1) igemm_relocate(d, (int)blockIdx.z);              // grouped launch (common.h)
    conv3h_body<BM, BN, WM, WN, KC, 2>(d);
}
// ... with the three-deep activation ring
template <int BM, int BN, int WM, int WN, int KC>
__global__ __launch_bounds__(256, conv3h_wgs_per_cu(BM, BN, KC, 3)) void conv3hr_kernel(const IgemmDesc d_in) {
    IgemmDesc d = d_in;
    if (d.grp.G > 1) igemm_relocate(d, (int)blockIdx.z);              // grouped launch (common.h)
    conv3h_body<BM, BN, WM, WN, KC, 3>(d);
}

template <int BM, int BN, int WM, int WN, int KC, int AR = 2>
static int launch_conv3h(const IgemmDesc& d, hipStream_t s) {
    if ((d.Cin / 16) % KC) return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: %d channel chunks are not a multiple of %d per group", d.Cin / 16, KC);
    const int per = (cdiv(d.p3_np, BM - 2) + 7) / 8;
    const int grid = 8 * per * cdiv(d.N, BN);
    if constexpr (AR == 3) {
        if (d.splitk != 1) return fail(SAGEN_ERR_UNSUPPORTED, "conv3hr: no dh-split (the three-deep ring needs three groups)");
        hipLaunchKernelGGL((conv3hr_kernel<BM, BN, WM, WN, KC>), dim3(grid, 1, d.grp.G), dim3(256), 0, s, d);
    } else hipLaunchKernelGGL((conv3h_kernel<BM, BN, WM, WN, KC>), dim3(grid, d.splitk, d.grp.G), dim3(256), 0, s, d);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

#ifdef SAGEN_TRACE
static void* g_trace_buf = nullptr;
static int g_trace_nth = -1;
// arms the trace of the nth conv3h launch from now (0 = the next one); buf: 8 x 8 bytes per workgroup, zeroed by the caller
extern "C" void sagen_debug_trace_conv3h(void* buf, int nth) { g_trace_buf = buf; g_trace_nth = nth; }
#endif

int conv3h_dispatch(const IgemmDesc& d_in, IgemmTile tile, hipStream_t s) {
    IgemmDesc d = d_in;
#ifdef SAGEN_TRACE
    if (g_trace_nth >= 0 && g_trace_nth-- == 0) d.trace = g_trace_buf;
#endif
    if (!d.xp3 || d.p3_np <= 0 || d.xp3_fmt != 1) return fail(SAGEN_ERR_NULL, "conv3h: the fp16x2 activation planes are missing");
    if (!d.wh2 || !d.h2_a_inv || !d.h2_w_inv) return fail(SAGEN_ERR_NULL, "conv3h: the fp16x2 filter planes / scales are missing");
    if (d.splitk != 1 && d.splitk != 3) return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: split-K only as the dh-split (3), got %d", d.splitk);
    if (d.splitk == 3) {             // partials [dh][M][N] (dense rows): the reducer applies bias / ReLU / statistics
        if (!d.splitk_ws || d.bias || d.relu_out || d.stats) return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: the dh-split writes raw partials (no bias / ReLU / statistics)");
        d.y = d.splitk_ws;
        d.ldy = d.N;
    }
    if ((long)(d.p3_np + 512) * (d.Win + 1) >= (1L << 32) || ((long)(d.p3_np + 512) / (d.Win + 1) + 1) * d.Hin >= (1L << 32))
        return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: too many pixels for 32-bit index arithmetic");
    if ((long)d.p3_np * 64 >= (1L << 31) || (long)d.xp3_cstride * (d.Cin / 16) >= (1L << 31) || d.xp3_bytes == 0)
        return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: the activation planes exceed 2 GiB buffer addressing (use a smaller batch)");
    const long y_bytes = ((long)(d.M - 1) * d.ldy + d.N) * 4;
    if (y_bytes >= (1L << 31)) return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: the output exceeds 2 GiB buffer addressing (use a smaller batch)");
    d.y_bytes = (unsigned)y_bytes;
    d.p3_magic_wp = (unsigned)((1UL << 32) / (unsigned)(d.Win + 1)) + 1u;
    d.p3_magic_h = (unsigned)((1UL << 32) / (unsigned)d.Hin) + 1u;
#define SAGEN_TILE_HAS_P3H ,
#define SAGEN_TILE_HAS_P3HR ,
    switch (tile) {
        SAGEN_TILES(SAGEN_TILE_CASE)
        default: return fail(SAGEN_ERR_UNSUPPORTED, "conv3h: bad tile id %d", (int)tile);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// filter planes for conv3h_kernel: fp32 packed filter [N][Kpad] -> max |w| -> 2^kw -> fp16 (hi, lo) of w 2^kw, [Kpad/16][2][N][16]
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void h2_absmax_kernel(const float* __restrict__ wp, long total, unsigned* __restrict__ amax_bits) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(wp[i]));
    __shared__ unsigned s_m;
    if (threadIdx.x == 0) s_m = 0u;
    __syncthreads();
    atomicMax(&s_m, __builtin_bit_cast(unsigned, m));            // non-negative floats order like their bit patterns
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(amax_bits, s_m);
}

// 2^k with bound * 2^k in [512, 1024) (k from the exponent field; bound == 0 or not finite -> 1)
__device__ __forceinline__ float h2_scale_for(float bound) {
    const unsigned b = __builtin_bit_cast(unsigned, bound);
    const int e = (int)((b >> 23) & 0xff);
    if (e == 0 || e == 255) return 1.f;
    int k = 127 + 9 - e;                                         // bound in [2^(e-127), 2^(e-126)) -> bound 2^k in [512, 1024)
    k = max(-60, min(60, k));
    return __builtin_bit_cast(float, (unsigned)(127 + k) << 23);
}

__global__ __launch_bounds__(256) void h2_filter_pack_kernel(const float* __restrict__ wp, long total, int N, int Kpad,
                                                             const unsigned* __restrict__ amax_bits, _Float16* __restrict__ w2,
                                                             float* __restrict__ w_inv) {
    const float sc = h2_scale_for(__builtin_bit_cast(float, amax_bits[0]));
    if (blockIdx.x == 0 && threadIdx.x == 0) w_inv[0] = 1.f / sc;                // exact: a power of two
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long n = idx / Kpad;
    const int k = (int)(idx - n * Kpad);
    const float v = wp[idx] * sc;
    const _Float16 h = (_Float16)v;
    const _Float16 l = (_Float16)(v - (float)h);
    const long o = ((long)(k >> 4) * 2 * N + n) * 16 + (k & 15);          // plane 0 of K tile k/16
    w2[o] = h;
    w2[o + (long)N * 16] = l;
}

// wp: fp32 packed filter [N][Kpad]; w2: N*Kpad*2 fp16; scratch: one unsigned (zeroed here); w_inv: where 2^-kw is written
int h2_filter_pack_launch(const float* wp, int N, int Kpad, void* w2, unsigned* scratch, float* w_inv, hipStream_t s) {
    if (!wp || !w2 || !scratch || !w_inv) return fail(SAGEN_ERR_NULL, "h2_filter_pack: null argument");
    const long total = (long)N * Kpad;
    SAGEN_HIP_CHECK(hipMemsetAsync(scratch, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(h2_absmax_kernel, dim3((int)std::min<long>(cdiv(total, 256), 1024)), dim3(256), 0, s, wp, total, scratch);
    hipLaunchKernelGGL(h2_filter_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, wp, total, N, Kpad, scratch,
                       reinterpret_cast<_Float16*>(w2), w_inv);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}


// ---- the same for MANY layers in two launches (bind; and once per training step, after the optimiser rewrote the variables) ----
// max |w| per job WITHOUT atomics: one partial per workgroup, then one workgroup per job folds its partials (11 k workgroups each
// ending in a same-address atomicMax took 109 us for 44 MB in the training step's trace - the L2 serialises them; an atomic-load
// guard in front of the atomicMax made it 188 us)
__global__ __launch_bounds__(256) void h2_absmax_multi_kernel(const H2Job* __restrict__ jobs, int njobs, float* __restrict__ part) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].first_block) ++j;
    const H2Job job = jobs[j];
    const unsigned total = (unsigned)job.N * (unsigned)job.Kpad;            // (a multiple of 16)
    const unsigned i = ((unsigned)((int)blockIdx.x - job.first_block) * 256 + threadIdx.x) * 4;
    float m = 0.f;
    if (i < total) {
        const float4 v = *reinterpret_cast<const float4*>(job.wp + i);
        m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    m = wave_max_f(m);
    __shared__ float s_m[4];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}
__global__ __launch_bounds__(256) void h2_absmax_finish_kernel(const H2Job* __restrict__ jobs, int njobs, int nblocks, const float* __restrict__ part,
                                                               unsigned* __restrict__ amax) {
    const int j = blockIdx.x;
    const int b0 = jobs[j].first_block, b1 = j + 1 < njobs ? jobs[j + 1].first_block : nblocks;
    float m = 0.f;
    for (int b = b0 + threadIdx.x; b < b1; b += 256) m = fmaxf(m, part[b]);
    m = wave_max_f(m);
    __shared__ float s_m[4];
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) amax[j] = __builtin_bit_cast(unsigned, fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3])));
}

__global__ __launch_bounds__(256) void h2_filter_pack_multi_kernel(const H2Job* __restrict__ jobs, int njobs, const unsigned* __restrict__ amax) {
    int j = 0;
    while (j + 1 < njobs && (int)blockIdx.x >= jobs[j + 1].first_block) ++j;
    const H2Job job = jobs[j];
    const float sc = h2_scale_for(__builtin_bit_cast(float, amax[j]));
    if ((int)blockIdx.x == job.first_block && threadIdx.x == 0) job.w_inv[0] = 1.f / sc;
    const long total = (long)job.N * job.Kpad;
    const long i0 = ((long)blockIdx.x - job.first_block) * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long idx = i0 + 256 * k;
        if (idx >= total) continue;
        const long n = idx / job.Kpad;
        const int kk = (int)(idx - n * job.Kpad);
        const float v = job.wp[idx] * sc;
        const _Float16 h = (_Float16)v;
        const _Float16 l = (_Float16)(v - (float)h);
        const long o = ((long)(kk >> 4) * 2 * job.N + n) * 16 + (kk & 15);
        reinterpret_cast<_Float16*>(job.w2)[o] = h;
        reinterpret_cast<_Float16*>(job.w2)[o + (long)job.N * 16] = l;
    }
}

int h2_filter_pack_multi_launch(const H2Job* jobs_dev, int njobs, int nblocks, unsigned* amax, hipStream_t s) {
    if (njobs <= 0) return SAGEN_OK;
    if (!jobs_dev || !amax) return fail(SAGEN_ERR_NULL, "h2_filter_pack_multi: null argument");
    float* part = reinterpret_cast<float*>(amax + njobs);        // amax holds njobs + nblocks words
    hipLaunchKernelGGL(h2_absmax_multi_kernel, dim3(nblocks), dim3(256), 0, s, jobs_dev, njobs, part);
    hipLaunchKernelGGL(h2_absmax_finish_kernel, dim3(njobs), dim3(256), 0, s, jobs_dev, njobs, nblocks, (const float*)part, amax);
    hipLaunchKernelGGL(h2_filter_pack_multi_kernel, dim3(nblocks), dim3(256), 0, s, jobs_dev, njobs, amax);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
