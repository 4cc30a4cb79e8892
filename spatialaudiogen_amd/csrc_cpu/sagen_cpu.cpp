// libsagen_cpu.so - the CPU twin of the OP LEVEL of include/sagen.h ("the same header is implemented twice").
//
// Plain C++, one thread, straightforward loops with double accumulation: every op-level entry point of the HIP library
// (sagen_stft_mag, sagen_conv2d, sagen_bn_finalize, sagen_bn_apply_relu, sagen_maxpool3x3s2, sagen_fc, sagen_deconv2d,
// sagen_mask_istft_mix, sagen_power_map[_batched], sagen_assemble_wyzx and their scratch-size queries) with the same
// signatures, layouts and argument meaning, on HOST pointers (the `stream` argument is ignored).  What it is for: the
// op-level parity cases of tests/test_gpu_ops.py run in a container WITHOUT a GPU against the same fp64 checker
// (tests/test_cpu_twin_ops.py), i.e. the header's semantics are pinned independently of the device code.
// What it is NOT: a fallback.  It is never loaded unless SAGEN_LIB names it explicitly, the context / forward / training
// entry points do not exist here (the Python binding refuses them), and it shares no code with the test checker.
// Each function cites the reference it follows, like the header.
//
// Two halves.  The network's op level above is an independent restatement, entry points and checks included.  The media ops
// (rendering, overlay, sources, reprojection, flow, resampling, JPEG, EMD) share with the device library their arithmetic
// (csrc/*_core.h) AND their entry points (csrc/op_entries.h, included here): what is refused, with which code and message, is
// the device library's by construction, and this file keeps only the loops, as the backends sagen::run_<op> of that header.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../csrc/op_entries.h"
#include "../csrc/op_entries_feed.h"
#include "../csrc/op_entries_audio.h"
#include "../csrc/op_entries_png.h"
#include "../csrc/op_entries_jpeg_rst.h"
#include "../csrc/op_entries_jpeg_split.h"
#include "../csrc/stft_frames.h"

namespace {
thread_local char g_err[512] = "";
}

int sagen::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

namespace {

typedef std::complex<double> cd;

// in-place radix-2 FFT of 1024 points (sign -1 forward, +1 inverse; unnormalised)
void fft1024(cd* a, int sign) {
    const int N = 1024;
    for (int i = 1, j = 0; i < N; ++i) {
        int bit = N >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= N; len <<= 1) {
        const double ang = sign * 2.0 * M_PI / len;
        const cd wl(std::cos(ang), std::sin(ang));
        for (int i = 0; i < N; i += len) {
            cd w(1.0, 0.0);
            for (int k = 0; k < len / 2; ++k) {
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
                w *= wl;
            }
        }
    }
}

// TF 'SAME': pad_total = max((ceil(in / s) - 1) * s + k - in, 0), pad_before = pad_total / 2
void same_pad(int in, int k, int s, int* out, int* before) {
    *out = (in + s - 1) / s;
    const int total = std::max((*out - 1) * s + k - in, 0);
    *before = total / 2;
}

}  // namespace

extern "C" {

int sagen_version(void) { return 100; }
const char* sagen_build_info(void) { return "cpu-twin (op level only; plain C++, double accumulation)"; }
const char* sagen_source_digest(void) { return "cpu-twin"; }
const char* sagen_last_error(void) { return g_err; }

/* myutils.stft (myutils.py:119-147) + crop + tf.abs (model.py:166-178): frame t = samples [256 t, 256 t + 1024) x periodic Hann */
int sagen_stft_mag(const float* audio, int batch, int n_samples, int f0, int f1, float* mag, int c0, int c1, float* spec, void*) {
    if (!audio || (!mag && !spec)) return fail(SAGEN_ERR_NULL, "sagen_stft_mag: null argument");
    if (batch <= 0) return fail(SAGEN_ERR_SHAPE, "sagen_stft_mag: batch=%d", batch);
    const int rc = sagen::stft_frames_check(n_samples, f0, f1, spec != nullptr, c0, c1);      // the device library's rule (csrc/stft_frames.h)
    if (rc) return rc;
    std::vector<double> hann(1024);
    for (int n = 0; n < 1024; ++n) hann[n] = (double)(float)(0.5 - 0.5 * std::cos(2.0 * M_PI / 1024 * n));     // (the reference rounds the window to float32, myutils.py:134)
    std::vector<cd> buf(1024);
    for (int b = 0; b < batch; ++b) {
        for (int t = f0; t < f1; ++t) {                  // (the spec window lies inside [f0, f1))
            const bool want_m = mag && t >= f0 && t < f1, want_s = spec && t >= c0 && t < c1;
            if (!want_m && !want_s) continue;
            for (int n = 0; n < 1024; ++n) buf[n] = cd((double)audio[(size_t)b * n_samples + 256 * t + n] * hann[n], 0.0);
            fft1024(buf.data(), -1);
            if (want_m)
                for (int k = 0; k < 1024; ++k) mag[((size_t)b * (f1 - f0) + (t - f0)) * 1024 + k] = (float)std::abs(buf[k]);
            if (want_s)
                for (int k = 0; k <= 512; ++k) {
                    float* o = spec + (((size_t)b * (c1 - c0) + (t - c0)) * 513 + k) * 2;
                    o[0] = (float)buf[k].real(); o[1] = (float)buf[k].imag();
                }
        }
    }
    return SAGEN_OK;
}

size_t sagen_conv2d_scratch_bytes(int, int, int, int, int, int, int) { return 256; }
size_t sagen_bn_stats_floats(int, int, int, int cout) { return (size_t)4 * cout; }     /* 2 * cout doubles */

/* tfw.conv_2d (core.py:156-220) = tf.nn.convolution NHWC / HWIO + bias + optional ReLU; input prologue relu(x * scale + shift) */
int sagen_conv2d(const float* x, int batch, int h, int w, int cin, const float* w_hwio, int kh, int kw, int cout, int sh, int sw,
                 int padding, const float* bias, int relu, const float* in_scale, const float* in_shift, float* y, float* bn_stats,
                 void*, size_t, void*) {
    if (!x || !w_hwio || !y) return fail(SAGEN_ERR_NULL, "sagen_conv2d: null argument");
    int ho, wo, pt = 0, pl = 0;
    if (padding) { same_pad(h, kh, sh, &ho, &pt); same_pad(w, kw, sw, &wo, &pl); }
    else { ho = (h - kh) / sh + 1; wo = (w - kw) / sw + 1; }
    double* st = reinterpret_cast<double*>(bn_stats);
    if (st) std::fill(st, st + 2 * cout, 0.0);
    std::vector<double> acc(cout);
    std::vector<float> xin(cin);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < ho; ++i)
            for (int j = 0; j < wo; ++j) {
                std::fill(acc.begin(), acc.end(), 0.0);
                for (int p = 0; p < kh; ++p) {
                    const int hi = i * sh + p - pt;
                    if (hi < 0 || hi >= h) continue;
                    for (int q = 0; q < kw; ++q) {
                        const int wi = j * sw + q - pl;
                        if (wi < 0 || wi >= w) continue;
                        const float* px = x + (((size_t)b * h + hi) * w + wi) * cin;
                        for (int c = 0; c < cin; ++c) xin[c] = in_scale ? std::max(px[c] * in_scale[c] + in_shift[c], 0.f) : px[c];
                        const float* pw = w_hwio + ((size_t)(p * kw + q) * cin) * cout;
                        for (int c = 0; c < cin; ++c) {
                            const double xv = xin[c];
                            if (xv == 0.0) continue;
                            const float* row = pw + (size_t)c * cout;
                            for (int o = 0; o < cout; ++o) acc[o] += xv * (double)row[o];
                        }
                    }
                }
                float* py = y + (((size_t)b * ho + i) * wo + j) * cout;
                for (int o = 0; o < cout; ++o) {
                    if (st) { st[o] += acc[o]; st[cout + o] += acc[o] * acc[o]; }      /* statistics of the RAW output */
                    double v = acc[o] + (bias ? (double)bias[o] : 0.0);
                    if (relu) v = std::max(v, 0.0);
                    py[o] = (float)v;
                }
            }
    return SAGEN_OK;
}

/* contrib batch_norm, is_training (core.py:6,209-210): biased variance, eps as given */
int sagen_bn_finalize(const float* bn_stats, int batch, int hout, int wout, int cout, const float* gamma, const float* beta, float eps,
                      float* scale, float* shift, void*) {
    if (!bn_stats || !gamma || !beta || !scale || !shift) return fail(SAGEN_ERR_NULL, "sagen_bn_finalize: null argument");
    const double* st = reinterpret_cast<const double*>(bn_stats);
    const double n = (double)batch * hout * wout;
    for (int c = 0; c < cout; ++c) {
        const double mean = st[c] / n, var = std::max(st[cout + c] / n - mean * mean, 0.0);
        const double s = (double)gamma[c] / std::sqrt(var + (double)eps);
        scale[c] = (float)s;
        shift[c] = (float)((double)beta[c] - mean * s);
    }
    return SAGEN_OK;
}

/* y = relu(x * scale + shift (+ residual)) (resnet.py:221,235) */
int sagen_bn_apply_relu(const float* x, const float* scale, const float* shift, const float* residual, float* y, int64_t n_pixels, int c, void*) {
    if (!x || !y) return fail(SAGEN_ERR_NULL, "sagen_bn_apply_relu: null argument");
    for (int64_t i = 0; i < n_pixels; ++i)
        for (int k = 0; k < c; ++k) {
            float v = scale ? std::fmaf(x[i * c + k], scale[k], shift[k]) : x[i * c + k];
            if (residual) v += residual[i * c + k];
            y[i * c + k] = std::max(v, 0.f);
        }
    return SAGEN_OK;
}

/* tf.nn.max_pool 3x3 s2 'SAME' (resnet.py:135) of relu(x * scale + shift); scale NULL: of x itself; -inf padding */
int sagen_maxpool3x3s2(const float* x, const float* scale, const float* shift, float* y, int batch, int h, int w, int c, void*) {
    if (!x || !y) return fail(SAGEN_ERR_NULL, "sagen_maxpool3x3s2: null argument");
    int ho, wo, pt, pl;
    same_pad(h, 3, 2, &ho, &pt); same_pad(w, 3, 2, &wo, &pl);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < ho; ++i)
            for (int j = 0; j < wo; ++j)
                for (int k = 0; k < c; ++k) {
                    float m = -INFINITY;
                    for (int p = 0; p < 3; ++p) {
                        const int hi = 2 * i + p - pt;
                        if (hi < 0 || hi >= h) continue;
                        for (int q = 0; q < 3; ++q) {
                            const int wi = 2 * j + q - pl;
                            if (wi < 0 || wi >= w) continue;
                            float v = x[(((size_t)b * h + hi) * w + wi) * c + k];
                            if (scale) v = std::max(std::fmaf(v, scale[k], shift[k]), 0.f);
                            m = std::max(m, v);
                        }
                    }
                    y[(((size_t)b * ho + i) * wo + j) * c + k] = m;
                }
    return SAGEN_OK;
}

size_t sagen_fc_scratch_bytes(int, int, int) { return 256; }
/* tfw.fully_connected (core.py:43-93) */
int sagen_fc(const float* x, int m, int k, const float* w_kn, int n, const float* bias, int relu, float* y, void*, size_t, void*) {
    if (!x || !w_kn || !y) return fail(SAGEN_ERR_NULL, "sagen_fc: null argument");
    std::vector<double> acc(n);
    for (int i = 0; i < m; ++i) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int kk = 0; kk < k; ++kk) {
            const double xv = x[(size_t)i * k + kk];
            const float* row = w_kn + (size_t)kk * n;
            for (int j = 0; j < n; ++j) acc[j] += xv * (double)row[j];
        }
        for (int j = 0; j < n; ++j) {
            double v = acc[j] + (bias ? (double)bias[j] : 0.0);
            y[(size_t)i * n + j] = (float)(relu ? std::max(v, 0.0) : v);
        }
    }
    return SAGEN_OK;
}

size_t sagen_deconv2d_scratch_bytes(int, int, int, int, int, int) { return 256; }
/* tfw.deconv_2d (core.py:96-153) = tf.nn.conv2d_transpose VALID: out[b, i sh + p, j sw + q, o] += x[b, i, j, c] w[p, q, o, c] */
int sagen_deconv2d(const float* x, int batch, int h, int w, int cin, const float* w_hwoi, int kh, int kw, int cout, int sh, int sw,
                   const float* bias, int relu, float* y, void*, size_t, void*) {
    if (!x || !w_hwoi || !y) return fail(SAGEN_ERR_NULL, "sagen_deconv2d: null argument");
    const int ho = h * sh + kh - sh, wo = w * sw + kw - sw;
    std::vector<double> acc((size_t)ho * wo * cout);
    for (int b = 0; b < batch; ++b) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int i = 0; i < h; ++i)
            for (int j = 0; j < w; ++j) {
                const float* px = x + (((size_t)b * h + i) * w + j) * cin;
                for (int p = 0; p < kh; ++p)
                    for (int q = 0; q < kw; ++q) {
                        double* po = acc.data() + ((size_t)(i * sh + p) * wo + (j * sw + q)) * cout;
                        const float* pw = w_hwoi + (size_t)(p * kw + q) * cout * cin;
                        for (int o = 0; o < cout; ++o) {
                            double s = 0.0;
                            for (int c = 0; c < cin; ++c) s += (double)px[c] * (double)pw[(size_t)o * cin + c];
                            po[o] += s;
                        }
                    }
            }
        for (size_t e = 0; e < acc.size(); ++e) {
            double v = acc[e] + (bias ? (double)bias[e % cout] : 0.0);
            y[(size_t)b * acc.size() + e] = (float)(relu ? std::max(v, 0.0) : v);
        }
    }
    return SAGEN_OK;
}

size_t sagen_mask_istft_mix_scratch_bytes(int) { return 256; }      /* not used here; asked for as the device library asks for its own */
/* model.py:326-347 (sigmoid mask x STFT), myutils.istft (myutils.py:181-211: plain average of the four overlaps, no synthesis
 * window), crop [448, 5248), decoder sum (model.py:421-434): out[b, n, o] = sum_k w[b, n / 1600, o, k] s_k[n] + bias */
int sagen_mask_istft_mix(const float* dmask, const float* spec, const float* coeffs, int batch, int ntracks, float* ambi_yzx, void* scratch,
                         size_t scratch_bytes, void*) {
    if (!dmask || !spec || !coeffs || !ambi_yzx || !scratch) return fail(SAGEN_ERR_NULL, "sagen_mask_istft_mix: null argument");
    if (batch <= 0) return fail(SAGEN_ERR_SHAPE, "sagen_mask_istft_mix: batch=%d", batch);
    if (scratch_bytes < sagen_mask_istft_mix_scratch_bytes(batch)) return fail(SAGEN_ERR_WORKSPACE, "sagen_mask_istft_mix: scratch too small");
    if (ntracks != 16 && ntracks != 32 && ntracks != 64)
        return fail(SAGEN_ERR_UNSUPPORTED, "mask_istft: num_sep_tracks=%d (supported: 16, 32, 64)", ntracks);
    const int NF = 28;
    std::vector<cd> buf(1024);
    std::vector<double> frames((size_t)NF * 1024), sep(4800);
    std::vector<double> out((size_t)4800 * 3);
    for (int b = 0; b < batch; ++b) {
        const float* cf = coeffs + (size_t)b * 3 * 3 * (ntracks + 1);
        for (int n = 0; n < 4800; ++n)
            for (int o = 0; o < 3; ++o) out[(size_t)n * 3 + o] = cf[((n / 1600) * 3 + o) * (ntracks + 1) + ntracks];
        for (int k = 0; k < ntracks; ++k) {
            for (int f = 0; f < NF; ++f) {
                const float* ps = spec + ((size_t)b * NF + f) * 513 * 2;
                const float* pm = dmask + (((size_t)b * NF + f) * 1024) * ntracks + k;
                for (int bin = 0; bin < 1024; ++bin) {
                    const int kb = bin <= 512 ? bin : 1024 - bin;
                    const cd X((double)ps[2 * kb], bin <= 512 ? (double)ps[2 * kb + 1] : -(double)ps[2 * kb + 1]);   // Hermitian mirror
                    const double m = 1.0 / (1.0 + std::exp(-(double)pm[(size_t)bin * ntracks]));
                    buf[bin] = X * m;
                }
                fft1024(buf.data(), +1);
                for (int n = 0; n < 1024; ++n) frames[(size_t)f * 1024 + n] = buf[n].real() / 1024.0;
            }
            /* istft sample q <-> time q + 768 from the start of frame 0; the crop keeps q in [448, 5248) */
            for (int n = 0; n < 4800; ++n) {
                const int t = n + 448 + 768;
                double s = 0.0;
                for (int f = 0; f < NF; ++f) {
                    const int p = t - 256 * f;
                    if (p >= 0 && p < 1024) s += frames[(size_t)f * 1024 + p];
                }
                sep[n] = s / 4.0;
            }
            for (int n = 0; n < 4800; ++n)
                for (int o = 0; o < 3; ++o) out[(size_t)n * 3 + o] += (double)cf[((n / 1600) * 3 + o) * (ntracks + 1) + k] * sep[n];
        }
        for (size_t e = 0; e < out.size(); ++e) ambi_yzx[(size_t)b * out.size() + e] = (float)out[e];
    }
    return SAGEN_OK;
}

/* AmbiDecoder.decode('projection') + RMS (decoder.py:24-28, distance.py:41-52) */
int sagen_power_map(const float* ambi_wyzx, int64_t t, const float* sh, int p, float* rms, void*) {
    if (!ambi_wyzx || !sh || !rms) return fail(SAGEN_ERR_NULL, "sagen_power_map: null argument");
    for (int d = 0; d < p; ++d) {
        double s = 0.0;
        for (int64_t i = 0; i < t; ++i) {
            double v = 0.0;
            for (int c = 0; c < 4; ++c) v += (double)ambi_wyzx[i * 4 + c] * (double)sh[d * 4 + c];
            s += v * v;
        }
        rms[d] = (float)std::sqrt(s / (double)t);
    }
    return SAGEN_OK;
}
int sagen_power_map_batched(const float* ambi_wyzx, int nchunks, int64_t t, const float* sh, int p, float* rms, double*, void* stream) {
    for (int c = 0; c < nchunks; ++c) {
        const int rc = sagen_power_map(ambi_wyzx + (size_t)c * t * 4, t, sh, p, rms + (size_t)c * p, stream);
        if (rc) return rc;
    }
    return SAGEN_OK;
}

/* deploy.py:143-152: W = mono[snd_contx / 2 : snd_contx / 2 + snd_dur], then Y, Z, X */
int sagen_assemble_wyzx(const float* audio, const float* ambi_yzx, float* out_wyzx, int batch, int snd_size, int snd_contx, int snd_dur, void*) {
    if (!audio || !ambi_yzx || !out_wyzx) return fail(SAGEN_ERR_NULL, "sagen_assemble_wyzx: null argument");
    for (int b = 0; b < batch; ++b)
        for (int n = 0; n < snd_dur; ++n) {
            float* o = out_wyzx + ((size_t)b * snd_dur + n) * 4;
            o[0] = audio[(size_t)b * snd_size + snd_contx / 2 + n];
            for (int c = 0; c < 3; ++c) o[1 + c] = ambi_yzx[((size_t)b * snd_dur + n) * 3 + c];
        }
    return SAGEN_OK;
}

}  // extern "C"

/* ---- the media ops: the backends of csrc/op_entries.h, which has checked every argument ---- */
namespace sagen {

/* The rotated FIR matrix of the renderings (include/sagen.h: sagen_render_fir; binauralizer.py:18-36, 63-76, 124-166, decoder.py:24-28,
 * myutils.py:289): rotate every row by the matrix interpolated at its absolute position, then the direct-form sum in double */
int run_render_fir(const float* x, int64_t n_hist, int64_t n, int channels, const float* taps, int outputs, int ntaps, const float* rot,
                   int n_rot, int rot_hop, int64_t pos0, int64_t zero_before, float* y, void*) {
    const int C = channels;
    const int64_t rows = n_hist + n;
    std::vector<double> xr((size_t)rows * C);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t s = pos0 - n_hist + r;
        for (int c = 0; c < C; ++c) {
            if (!rot) {
                xr[r * C + c] = x[r * C + c];
                continue;
            }
            const int64_t m = std::min<int64_t>(s / rot_hop, n_rot - 1), m1 = std::min<int64_t>(m + 1, n_rot - 1);
            const double al = m1 == m ? 0.0 : (double)(s - m * rot_hop) / (double)rot_hop;      // the last matrix is held
            double v = 0.0;
            for (int e = 0; e < C; ++e)
                v += ((1.0 - al) * (double)rot[(m * C + c) * C + e] + al * (double)rot[(m1 * C + c) * C + e]) * (double)x[r * C + e];
            xr[r * C + c] = v;
        }
    }
    for (int64_t i = 0; i < n; ++i)
        for (int o = 0; o < outputs; ++o) {
            double acc = 0.0;
            for (int c = 0; c < C; ++c)
                for (int k = 0; k < ntaps; ++k) {
                    const int64_t r = n_hist + i - k;
                    if (r < 0) break;
                    acc += (double)taps[((size_t)o * C + c) * ntaps + k] * xr[r * C + c];
                }
            y[i * outputs + o] = pos0 + i < zero_before ? 0.f : (float)acc;
        }
    return SAGEN_OK;
}

/* The maps of a strided stream (include/sagen.h: sagen_power_map_windows; distance.py:41-52 over myutils.py:252's ambix[::5]): the
 * definition itself, every node's projection squared and averaged in double */
int run_power_map_windows(const float* ambi, int channels, int stride, int64_t window, int n_maps, const float* sh, int p, float* rms,
                          double*, void*) {
    for (int64_t m = 0; m < n_maps; ++m)
        for (int d = 0; d < p; ++d) {
            double s = 0.0;
            for (int64_t k = 0; k < window; ++k) {
                const float* row = ambi + (m * window + k) * stride * channels;
                double v = 0.0;
                for (int c = 0; c < channels; ++c) v += (double)row[c] * (double)sh[(size_t)d * channels + c];
                s += v * v;
            }
            rms[m * p + d] = (float)std::sqrt(s / (double)window);
        }
    return SAGEN_OK;
}

/* myutils.py:255-279 for a run of frames (include/sagen.h: sagen_overlay_blend): whole arrays at a time, the way the reference's
 * numpy does it - normalise the maps, mix, colour, resize (the header's restatement of scikit-image 0.13.1), blend, truncate */
namespace {
// resize of one [mh][mw][nc] array to [h][w][nc]
std::vector<double> resize_bilinear(const std::vector<double>& a, int mh, int mw, int nc, int h, int w) {
    const double lo = *std::min_element(a.begin(), a.end()), hi = *std::max_element(a.begin(), a.end());
    const bool spans_zero = lo <= 0.0 && 0.0 <= hi;
    auto get = [&](double i, double j, int k) { return i < 0 || i >= mh || j < 0 || j >= mw ? 0.0 : a[((size_t)i * mw + (size_t)j) * nc + k]; };
    std::vector<double> o((size_t)h * w * nc);
    for (int y = 0; y < h; ++y) {
        const double r = (y + 0.5) * ((double)mh / h) - 0.5, r0 = std::floor(r), r1 = std::ceil(r), dr = r - r0;
        for (int x = 0; x < w; ++x) {
            const double c = (x + 0.5) * ((double)mw / w) - 0.5, c0 = std::floor(c), c1 = std::ceil(c), dc = c - c0;
            for (int k = 0; k < nc; ++k) {
                const double top = (1 - dc) * get(r0, c0, k) + dc * get(r0, c1, k);
                const double bot = (1 - dc) * get(r1, c0, k) + dc * get(r1, c1, k);
                double val = (1 - dr) * top + dr * bot;
                if (spans_zero || val != 0.0) val = std::min(std::max(val, lo), hi);
                o[((size_t)y * w + x) * nc + k] = val;
            }
        }
    }
    return o;
}
}  // namespace
int run_overlay_blend(const float* maps, int64_t map0, int mh, int mw, const double* lut, const uint8_t* frames, int n_frames,
                      int64_t frame0, int h, int w, int frames_per_map, uint8_t* out, void*, void*) {
    const int N = mh * mw;
    const int n_maps = (int)((frame0 + n_frames - 1) / frames_per_map + 1 - map0) + 1;      // up to the last frame's `cur` map
    std::vector<double> norm((size_t)n_maps * N);
    for (int m = 0; m < n_maps; ++m) {
        const float* r = maps + (size_t)m * N;
        const double lo = *std::min_element(r, r + N), hi = *std::max_element(r, r + N);
        for (int n = 0; n < N; ++n) norm[(size_t)m * N + n] = ((double)r[n] - lo) / (hi - lo + 0.005);
    }
    std::vector<double> v(N), colour((size_t)N * 3);
    for (int f = 0; f < n_frames; ++f) {
        const int64_t F = frame0 + f, prev = F / frames_per_map - map0, cur = prev + 1;
        const double beta = (double)(F % frames_per_map) / (double)frames_per_map;
        for (int n = 0; n < N; ++n) {
            double t = (1 - beta) * norm[(size_t)prev * N + n] + beta * norm[(size_t)cur * N + n];
            t = t * 2. - 0.7;
            v[n] = t < 0 ? 0.0 : t;
            const int idx = std::min((int)(v[n] * 255), 255);
            for (int k = 0; k < 3; ++k) colour[(size_t)n * 3 + k] = lut[idx * 3 + k];
        }
        const std::vector<double> dir = resize_bilinear(colour, mh, mw, 3, h, w), al = resize_bilinear(v, mh, mw, 1, h, w);
        for (size_t px = 0; px < (size_t)h * w; ++px) {
            const double alpha = al[px] * 0.6;
            for (int k = 0; k < 3; ++k) {
                const size_t e = ((size_t)f * h * w + px) * 3 + k;
                out[e] = (uint8_t)(int)(alpha * (dir[px * 3 + k] * 255) + (1 - alpha) * (double)frames[e]);
            }
        }
    }
    return SAGEN_OK;
}

// emd/dir, emd/dir2 (distance.py:100-143): the solver core of the device kernel (csrc/emd_core.h) run by one host "lane"
int run_eval_emd(const float* p, const float* q, int n_maps, int nodes, const double* cost, double* emd, uint32_t* not_converged, void*) {
    std::vector<sagen::EmdState> st(1);
    std::vector<double> P(nodes), Q(nodes);
    const sagen::EmdSerial w;
    for (int m = 0; m < n_maps; ++m)
        for (int var = 0; var < 2; ++var) {
            double sp = 0.0, sq = 0.0;
            for (int v = 0; v < nodes; ++v) { sp += p[(size_t)m * nodes + v]; sq += q[(size_t)m * nodes + v]; }
            const double np_ = var == 0 ? (double)nodes : sp + 0.01, nq = var == 0 ? (double)nodes : sq + 0.01;
            for (int v = 0; v < nodes; ++v) { P[v] = p[(size_t)m * nodes + v] / np_; Q[v] = q[(size_t)m * nodes + v] / nq; }
            int conv = 1;
            emd[m * 2 + var] = sagen::emd_hat(w, st[0], P.data(), Q.data(), nodes, cost, &conv);
            if (!conv) ++*not_converged;
        }
    return SAGEN_OK;
}

/* Moving point sources (include/sagen.h; encoder.py:10-55, binauralizer.py:12-121, distance.py:62-97 over position.py:73-102): a loop
 * per sample and source over the fp64 core the device uses (csrc/sources_core.h), the sample sums in double */
namespace {
struct SrcPoint { double r, u[3]; };
SrcPoint src_at(const double* ctrl, const sagen::SourceSet& ss, int s, int64_t t) {
    SrcPoint p;
    double phi, nu;
    const int p0 = ss.pt_off[s];
    sagen::source_polar(ctrl + (size_t)p0 * 3, ss.pt_off[s + 1] - p0, ss.nframes[s], ss.duration[s], ss.rate, t, phi, nu, p.r);
    sagen::source_unit(phi, nu, p.r, p.u);
    return p;
}
int src_nearest(const double* dirs, int D, const double u[3]) {
    const int f = sagen::nearest_first(dirs, 0, D, u, sagen::nearest_max(dirs, D, u, -INFINITY), -1);
    return f < 0 ? 0 : f;
}
}  // namespace

int run_source_track(const double* ctrl, const SourceSet& ss, int64_t t0, int64_t n, int64_t stride, const double* dirs, int n_dirs,
                     double* unit, int32_t* nearest, void*) {
    const int n_sources = ss.n_sources;
    for (int64_t i = 0; i < n; ++i)
        for (int s = 0; s < n_sources; ++s) {
            const SrcPoint p = src_at(ctrl, ss, s, t0 + i * stride);
            if (unit)
                for (int k = 0; k < 3; ++k) unit[(i * n_sources + s) * 3 + k] = p.u[k];
            if (nearest) nearest[i * n_sources + s] = src_nearest(dirs, n_dirs, p.u);
        }
    return SAGEN_OK;
}

int run_encode_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int channels, int distance_model,
                       double radius, int64_t t0, int64_t n, float* ambi, void*) {
    const int n_sources = ss.n_sources;
    const double rate = ss.rate;
    const long long* nframes = ss.nframes;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t t = t0 + i;
        double acc[9] = {0.};
        for (int s = 0; s < n_sources; ++s) {
            const SrcPoint p = src_at(ctrl, ss, s, t);
            double Y[9];
            if (channels == 4) sagen::source_harmonics<4>(p.u, Y); else sagen::source_harmonics<9>(p.u, Y);
            double g = 1.;
            long long d = 0;
            if (distance_model) {
                const double dist = std::fabs(p.r) - radius;
                if (!sagen::source_delay(dist, rate, d)) continue;
                g = 1. / (1. + dist);
            }
            const int64_t j = t - d;
            if (j < 0 || j >= nframes[s]) continue;
            for (int c = 0; c < channels; ++c) acc[c] += g * Y[c] * (double)signals[s * ld + j];
        }
        for (int c = 0; c < channels; ++c) ambi[i * channels + c] = (float)acc[c];
    }
    return SAGEN_OK;
}

int run_binauralize_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int mode, const double* dirs,
                            const float* hrir, int n_dirs, int ntaps, int64_t zero_before, int64_t t0, int64_t n, float* y, void*) {
    const bool h = mode == SAGEN_SOURCES_HRIR;
    const int n_sources = ss.n_sources;
    const double rate = ss.rate;
    const long long* nframes = ss.nframes;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t t = t0 + i;
        double acc[2] = {0., 0.};
        for (int s = 0; s < n_sources; ++s) {
            const SrcPoint p = src_at(ctrl, ss, s, t);
            const float* sig = signals + s * ld;
            if (h) {
                const float* hp = hrir + (size_t)src_nearest(dirs, n_dirs, p.u) * 2 * ntaps;
                for (int e = 0; e < 2; ++e)
                    for (int k = 0; k < ntaps && t - k >= 0; ++k) acc[e] += (double)hp[e * ntaps + k] * (double)sig[t - k];
                continue;
            }
            const double ar = std::fabs(p.r);
            for (int e = 0; e < 2; ++e) {
                const double dx = ar * p.u[0], dy = ar * p.u[1] - (e == 0 ? sagen::SRC_EAR_Y : -sagen::SRC_EAR_Y), dz = ar * p.u[2];
                const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
                long long d;
                if (!sagen::source_delay(dist, rate, d) || t - d < 0 || t - d >= nframes[s]) continue;
                acc[e] += (double)sig[t - d] / (1. + dist) / (double)n_sources;
            }
        }
        const bool z = h && t < zero_before;
        y[i * 2] = z ? 0.f : (float)acc[0];
        y[i * 2 + 1] = z ? 0.f : (float)acc[1];
    }
    return SAGEN_OK;
}

/* Reprojection of 360-degree frames (include/sagen.h: sagen_reproject; scraping/utils.py:91-144, preprocess.py:51-52, vrProjector's
 * CubemapProjection.py:68-121): a loop per frame and destination pixel over the fp64 core the device uses (csrc/project_core.h) */
namespace {
template <int SK, int DK>
void reproject_frames(const uint8_t* src, uint8_t* dst, const double* rot, const sagen::ProjArgs& a) {
    const size_t src_bytes = (size_t)a.src.fh * a.src.fw * 3, dst_bytes = (size_t)a.dst.fh * a.dst.fw * 3;
    for (int fr = 0; fr < a.n; ++fr) {
        const double* rp = a.n_rot == 0 ? nullptr : rot + (a.n_rot == 1 ? 0 : (size_t)fr * 9);
        for (int py = 0; py < a.dst.fh; ++py)
            for (int px = 0; px < a.dst.fw; ++px) {
                int f, cx, cy, cw, ch;
                if (!sagen::proj_dst_cell<DK>(a.dst, px, py, f, cx, cy, cw, ch)) continue;
                sagen::proj_pixel<SK, DK>(a, src + fr * src_bytes, rp, f, cx, cy, cw, ch, dst + fr * dst_bytes + ((size_t)py * a.dst.fw + px) * 3);
            }
    }
}
template <int SK>
void reproject_dst(const uint8_t* src, uint8_t* dst, const double* rot, const sagen::ProjArgs& a) {
    switch (a.dst.kind) {
        case SAGEN_PROJ_ER: reproject_frames<SK, SAGEN_PROJ_ER>(src, dst, rot, a); break;
        case SAGEN_PROJ_CUBE: reproject_frames<SK, SAGEN_PROJ_CUBE>(src, dst, rot, a); break;
        case SAGEN_PROJ_EAC: reproject_frames<SK, SAGEN_PROJ_EAC>(src, dst, rot, a); break;
        default: reproject_frames<SK, SAGEN_PROJ_VIEW>(src, dst, rot, a); break;
    }
}
}  // namespace

int run_reproject(const uint8_t* src, uint8_t* dst, const double* rot, const ProjArgs& a, void*) {
    switch (a.src.kind) {
        case SAGEN_PROJ_ER: reproject_dst<SAGEN_PROJ_ER>(src, dst, rot, a); break;
        case SAGEN_PROJ_CUBE: reproject_dst<SAGEN_PROJ_CUBE>(src, dst, rot, a); break;
        default: reproject_dst<SAGEN_PROJ_EAC>(src, dst, rot, a); break;
    }
    return SAGEN_OK;
}

/* Dense optical flow and its byte coding (include/sagen.h: sagen_optical_flow, sagen_flow_encode): plain loops per pair over the fp64
 * core the device uses (csrc/flow_core.h).  Every Jacobi sweep covers the whole level: `fuse` is checked and otherwise ignored, which
 * is what "the result does not depend on it" means on this side. */
namespace {
void flow_pair(const double* p1, const double* p2, const sagen::FlowArgs& a, float* out, double* s1, double* s2, sagen::FlowUV* cur,
               sagen::FlowUV* oth, sagen::FlowUV* f0, sagen::FlowCoef* coef) {
    using namespace sagen;
    size_t off[FLOW_MAX_LEVELS];
    off[0] = 0;
    for (int l = 1; l < a.levels; ++l) off[l] = off[l - 1] + (size_t)(a.h >> (l - 1)) * (a.w >> (l - 1));
    for (int l = a.levels - 1; l >= 0; --l) {
        const int h = a.h >> l, w = a.w >> l;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                s1[(size_t)y * w + x] = flow_smooth(p1 + off[l], h, w, a.wrap, x, y);
                s2[(size_t)y * w + x] = flow_smooth(p2 + off[l], h, w, a.wrap, x, y);
                FlowUV r;
                r.u = 0.; r.v = 0.;
                if (l != a.levels - 1) r = flow_upsample(cur, h / 2, w / 2, a.wrap, x, y);
                oth[(size_t)y * w + x] = r;
            }
        std::swap(cur, oth);
        for (int wp = 0; wp < a.warps; ++wp) {
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    coef[(size_t)y * w + x] = flow_derivs(s1, s2, cur, h, w, a.wrap, x, y);
                    f0[(size_t)y * w + x] = cur[(size_t)y * w + x];
                }
            for (int it = 0; it < a.iters; ++it) {
                for (int y = 0; y < h; ++y) {
                    const FlowUV* rn = cur + (size_t)flow_iy(y - 1, h) * w;
                    const FlowUV* rc = cur + (size_t)y * w;
                    const FlowUV* rs = cur + (size_t)flow_iy(y + 1, h) * w;
                    for (int x = 0; x < w; ++x) {
                        const int xw = flow_ix(x - 1, w, a.wrap), xe = flow_ix(x + 1, w, a.wrap);
                        const double ub = flow_average(rn[x].u, rs[x].u, rc[xw].u, rc[xe].u, rn[xw].u, rn[xe].u, rs[xw].u, rs[xe].u);
                        const double vb = flow_average(rn[x].v, rs[x].v, rc[xw].v, rc[xe].v, rn[xw].v, rn[xe].v, rs[xw].v, rs[xe].v);
                        oth[(size_t)y * w + x] = flow_hs_update(ub, vb, coef[(size_t)y * w + x], f0[(size_t)y * w + x], a.alpha2);
                    }
                }
                std::swap(cur, oth);
            }
        }
    }
    for (size_t i = 0; i < (size_t)a.h * a.w; ++i) {
        out[2 * i] = (float)cur[i].u;
        out[2 * i + 1] = (float)cur[i].v;
    }
}
}  // namespace

int run_optical_flow(const uint8_t* frames, const FlowArgs& a, float* flow, void* scratch, void*) {
    const int n_frames = a.n_frames, h = a.h, w = a.w;
    // the device's layout: three (u, v) fields and the coefficients per pair, the pyramids, the smoothed level (two frames used here)
    const size_t hw = (size_t)h * w, pyr = flow_level_pixels(h, w, a.levels);
    FlowUV* cur = (FlowUV*)scratch;
    FlowUV* oth = cur + (size_t)(n_frames - 1) * hw;
    FlowUV* f0 = oth + (size_t)(n_frames - 1) * hw;
    FlowCoef* coef = (FlowCoef*)(f0 + (size_t)(n_frames - 1) * hw);
    double* pyramid = (double*)(coef + (size_t)(n_frames - 1) * hw);
    double* smooth = pyramid + (size_t)n_frames * pyr;
    for (int f = 0; f < n_frames; ++f) {
        double* g = pyramid + (size_t)f * pyr;
        for (size_t i = 0; i < hw; ++i) g[i] = flow_luma(frames + ((size_t)f * hw + i) * 3);
        size_t fine = 0;
        for (int l = 1; l < a.levels; ++l) {
            const int ch = h >> l, cw = w >> l;
            const size_t coarse = fine + (size_t)(2 * ch) * (2 * cw);
            for (int y = 0; y < ch; ++y)
                for (int x = 0; x < cw; ++x) g[coarse + (size_t)y * cw + x] = flow_down(g + fine, 2 * cw, x, y);
            fine = coarse;
        }
    }
    for (int k = 0; k + 1 < n_frames; ++k)
        flow_pair(pyramid + (size_t)k * pyr, pyramid + (size_t)(k + 1) * pyr, a, flow + (size_t)k * hw * 2, smooth, smooth + hw, cur, oth, f0, coef);
    return SAGEN_OK;
}

int run_flow_encode(const float* flow, int n, int h, int w, uint8_t* rgb, float* limits, void*, void*) {
    const size_t hw = (size_t)h * w;
    for (int f = 0; f < n; ++f) {
        const float* p = flow + (size_t)f * hw * 2;
        float lo = INFINITY, hi = -INFINITY;
        for (size_t i = 0; i < hw; ++i) {
            const float m = flow_mag(p[2 * i], p[2 * i + 1]);
            lo = m < lo ? m : lo;
            hi = m > hi ? m : hi;
        }
        float* lim = limits + (size_t)f * 2;
        flow_limits(lo, hi, lim);
        for (size_t i = 0; i < hw; ++i) flow_bytes(p[2 * i], p[2 * i + 1], lim[0], lim[1], rgb + ((size_t)f * hw + i) * 3);
    }
    return SAGEN_OK;
}

/* Polyphase FIR resampling and windowed RMS (include/sagen.h: sagen_resample_fir, sagen_window_rms; pyutils/iolib/audio.py:23,
 * scraping/preprocess.py:14-34 and :146-153, pyutils/ambisonics/common.py:34-59): plain loops per output over the fp64 core the
 * device uses (csrc/resample_core.h).  The rows an output reaches are mixed into a small buffer, zeros where the x buffer has none. */
int run_resample_fir(const float* x, const double* taps, const double* mix, float* y, const ResampleArgs& a, const char**, void*) {
    const int c_in = a.c_in, c_out = a.c_out, L = a.L, M = a.M, H = a.H, T = a.T;
    std::vector<double> z((size_t)T * c_out);
    for (long long j = 0; j < a.n; ++j) {
        const long long nn = a.n0 + j, m0 = rs_first_row(nn, L, M, H);
        for (int t = 0; t < T; ++t) {
            const long long r = m0 + t - a.x0;
            for (int o = 0; o < c_out; ++o) z[(size_t)t * c_out + o] = (r >= 0 && r < a.n_in) ? rs_mix_row(x, r, c_in, mix, o) : 0.;
        }
        const double* row = taps + (long long)rs_phase(nn, L, M) * T;
        for (int o = 0; o < c_out; ++o) y[j * c_out + o] = (float)rs_dot(row, z.data() + o, c_out, T);
    }
    return SAGEN_OK;
}

int run_window_rms(const float* x, int channels, int channel, int64_t first, int64_t hop, int64_t length, int64_t count, double* rms,
                   void*) {
    for (long long i = 0; i < count; ++i) {
        double p[RMS_LANES];
        for (int l = 0; l < RMS_LANES; ++l) p[l] = rms_partial(x, first + i * hop, channels, channel, length, l);
        rms[i] = rms_finish_host(p, length);
    }
    return SAGEN_OK;
}

/* Baseline JPEG decode (include/sagen.h: sagen_jpeg_decode; PIL / libjpeg behind feeder.py:18-23 in the reference): the five stages
 * of csrc/jpeg.hip as plain loops over the integer core the device uses (csrc/jpeg_core.h: jpeg_decode_host) */
int run_jpeg_decode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                    const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out,
                    int32_t* status, void* scratch, void*) {
    jpeg_decode_host(bytes, total_bytes, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch);
    return SAGEN_OK;
}

/* The same with the entropy stage of a segment on many lanes (include/sagen.h: sagen_jpeg_decode_split): the stages of
 * csrc/jpeg_split.hip in their order as plain loops (csrc/jpeg_split_core.h: jpeg_split_decode_host), the same rounds, the same path */
int run_jpeg_decode_split(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                          const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out, int32_t* status,
                          void* scratch, void*, int chunk_bytes, int rounds, int64_t max_chunks, int32_t* path) {
    jpeg_split_decode_host(bytes, total_bytes, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch, chunk_bytes,
                           rounds, max_chunks, path);
    return SAGEN_OK;
}

/* Baseline JPEG encode (include/sagen.h: sagen_jpeg_encode; ffmpeg's "%06d.jpg" behind scraping/preprocess.py:183-196 in the
 * reference, PIL / libjpeg behind the frame writers here): frame by frame, block by block, bit by bit over the integer core the device
 * uses (csrc/jpeg_enc_core.h: jpeg_encode_host).  The scratch is not used. */
int run_jpeg_encode(const uint8_t* frames, const JpegEncGeom& g, const uint16_t* qtabs, uint8_t* out, int32_t* sizes, int32_t* status, void*,
                    void*) {
    jpeg_encode_host(frames, g, qtabs, out, sizes, status);
    return SAGEN_OK;
}

/* Lossless re-segmenting (include/sagen.h: sagen_jpeg_transcode): the decoder's entropy loop into coefficients, the encoder's bit loop
 * out of them (csrc/jpeg_enc_core.h: jpeg_transcode_host).  The scratch is used as the device uses it. */
int run_jpeg_transcode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                       const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& d, const JpegEncGeom& g, uint8_t* out, int32_t* sizes, int32_t* status,
                       void* scratch, void*) {
    jpeg_transcode_host(bytes, total_bytes, frames, segments, n_segments, hufftabs, n_hufftabs, d, g, out, sizes, status, scratch);
    return SAGEN_OK;
}

/* Frame batches from a resident clip (include/sagen.h: sagen_assemble_frames; the stacking, rolling and flow un-coding of
 * feeder.py:106-161 in the reference): item by item, pixel by pixel over the core the device uses (csrc/feed_core.h). */
int run_assemble_frames(const uint8_t* frames, int n_frames, int h, int w, const int32_t* index, const int32_t* shift, int n_out, int mode,
                        const float* table, const double* scale_lo, void* out, void*) {
    const size_t hw = (size_t)h * w;
    for (int i = 0; i < n_out; ++i) {
        uint8_t* ob = (uint8_t*)out + (size_t)i * hw * 3;
        float* of = (float*)out + (size_t)i * hw * 3;
        const int f = index[i];
        if (f < 0 || f >= n_frames) {
            if (mode == FEED_BYTES) memset(ob, 0, hw * 3);
            else for (size_t k = 0; k < hw * 3; ++k) of[k] = 0.f;
            continue;
        }
        const int s = feed_roll(shift[i], w);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const uint8_t* p = frames + ((size_t)f * hw + (size_t)y * w + feed_src_x(x, s, w)) * 3;
                const size_t o = ((size_t)y * w + x) * 3;
                if (mode == FEED_BYTES) {
                    ob[o] = p[0]; ob[o + 1] = p[1]; ob[o + 2] = p[2];
                } else if (mode == FEED_TABLE) {
                    of[o] = table[p[0]]; of[o + 1] = table[p[1]]; of[o + 2] = table[p[2]];
                } else {
                    feed_flow_pixel(p[0], p[2], table, table + 256, scale_lo[2 * (size_t)f], scale_lo[2 * (size_t)f + 1], of + o);
                }
            }
    }
    return SAGEN_OK;
}

/* Audio windows from a resident clip (include/sagen.h: sagen_assemble_audio; the cutting, padding and rotating of feeder.py:50-103 in
 * the reference and the slicing of train.py:107-111): item by item, row by row over the core the device uses (csrc/audio_feed_core.h). */
namespace {
template <typename T>
void assemble_audio_rows(const T* samples, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from, const int32_t* count,
                         const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono, float* target) {
    for (int i = 0; i < n_out; ++i)
        for (int j = 0; j < size; ++j) {
            double v[AUDIO_FEED_MAX_CHANNELS];
            float o[AUDIO_FEED_MAX_CHANNELS];
            int64_t src = 0;
            const bool live = audio_feed_src_row(j, lead[i], read_from[i], count[i], n_samples, &src);
            for (int c = 0; c < channels; ++c) v[c] = live ? audio_feed_value(samples[src * channels + c]) : 0.0;
            if (live && rot) audio_feed_rotate(v, rot[2 * (size_t)i], rot[2 * (size_t)i + 1]);
            for (int c = 0; c < channels; ++c) o[c] = live ? (float)v[c] : 0.f;
            const size_t row = (size_t)i * size + j;
            if (full) for (int c = 0; c < channels; ++c) full[row * channels + c] = o[c];
            if (mono) mono[row] = o[0];
            if (target && j >= t_off && j - t_off < t_len)
                for (int c = 1; c < channels; ++c) target[((size_t)i * t_len + (j - t_off)) * (channels - 1) + (c - 1)] = o[c];
        }
}
}  // namespace

int run_assemble_audio(const void* samples, int sample_type, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from,
                       const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono,
                       float* target, void*) {
    if (sample_type == AUDIO_I16) assemble_audio_rows((const int16_t*)samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target);
    else if (sample_type == AUDIO_F32) assemble_audio_rows((const float*)samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target);
    else assemble_audio_rows((const double*)samples, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono, target);
    return SAGEN_OK;
}

/* PNG frames (include/sagen.h: sagen_png_filter, sagen_deflate; the host's zlib behind the lossless frames of myutils.py:246-279 in
 * the reference, PIL's save behind the overlay writers here): row by row, and frame by frame, block by block, chunk by chunk over the
 * integer core the device uses (csrc/png_core.h: png_filter_host, deflate_host).  The scratch is used as the device uses it. */
int run_png_filter(const uint8_t* frames, int n, int w, int h, int components, uint8_t* rows, void*) {
    png_filter_host(frames, n, w, h, components, rows);
    return SAGEN_OK;
}

int run_deflate(const uint8_t* data, const DeflateGeom& g, uint8_t* out, int32_t* sizes, int32_t* status, void* scratch, void*) {
    deflate_host(data, g, out, sizes, status, scratch);
    return SAGEN_OK;
}

}  // namespace sagen
