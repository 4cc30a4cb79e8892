// The extern "C" entry points of the media ops of include/sagen.h, written ONCE for both libraries: libsagen_hip.so (api.hip) and the
// CPU twin (csrc_cpu/sagen_cpu.cpp) each include this file in exactly one translation unit.  An entry is the whole refusal half of
// the header's contract - null operands, sizes, support limits, scratch size, pointer alignment, the empty call, in that order - and
// ends in one call to its backend, sagen::run_<op> (op_backends.h), which sees validated arguments only.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.  The network's op level (sagen_conv2d and the
// rest, tied to IgemmDesc and tile choice) is not here: the twin restates it independently on purpose.
#pragma once
#include "op_backends.h"
#include "host_sizes.h"
#include "emd_core.h"
#include "sources_core.h"
#include "project_core.h"
#include "flow_core.h"
#include "resample_core.h"
#include "jpeg_core.h"
#include "jpeg_enc_core.h"

namespace sagen {

static inline int source_fill(const char* who, SourceSet& ss, const double* ctrl, const int32_t* pt_off, const int64_t* nframes,
                              const double* duration, int n_sources, double rate, int64_t t_first, int64_t t_last) {
    const char* why;
    const int rc = source_set_fill(ss, ctrl, pt_off, nframes, duration, n_sources, rate, t_first, t_last, &why);
    return rc == SAGEN_OK ? rc : fail(rc, "%s: %s", who, why);
}

static inline long long source_longest(const SourceSet& ss) {
    long long m = 0;
    for (int s = 0; s < ss.n_sources; ++s) m = ss.nframes[s] > m ? ss.nframes[s] : m;
    return m;
}

}  // namespace sagen

using namespace sagen;

extern "C" {

int sagen_eval_emd(const float* p, const float* q, int n_maps, int nodes, const double* cost, double* emd, uint32_t* not_converged,
                   void* stream) {
    if (!p || !q || !cost || !emd || !not_converged) return fail(SAGEN_ERR_NULL, "sagen_eval_emd: null argument");
    if (n_maps <= 0 || nodes <= 0) return fail(SAGEN_ERR_SHAPE, "sagen_eval_emd: n_maps=%d nodes=%d", n_maps, nodes);
    if (nodes > EMD_MAX_NODES) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_eval_emd: nodes=%d (supported: <= %d)", nodes, EMD_MAX_NODES);
    if (((uintptr_t)cost) % 8 || ((uintptr_t)emd) % 8 || ((uintptr_t)not_converged) % 4)
        return fail(SAGEN_ERR_SHAPE, "sagen_eval_emd: cost / emd must be 8-byte aligned, not_converged 4-byte aligned");
    return run_eval_emd(p, q, n_maps, nodes, cost, emd, not_converged, stream);
}

int sagen_render_fir(const float* x, int64_t n_hist, int64_t n, int channels, const float* taps, int outputs, int ntaps, const float* rot,
                     int n_rot, int rot_hop, int64_t pos0, int64_t zero_before, float* y, void* stream) {
    if (!x || !taps || !y) return fail(SAGEN_ERR_NULL, "sagen_render_fir: null argument");
    if (n_hist < 0 || n <= 0 || channels <= 0 || outputs <= 0 || ntaps <= 0 || pos0 < 0)
        return fail(SAGEN_ERR_SHAPE, "sagen_render_fir: n_hist=%ld n=%ld channels=%d outputs=%d ntaps=%d pos0=%ld", (long)n_hist, (long)n,
                    channels, outputs, ntaps, (long)pos0);
    if (n_hist > pos0) return fail(SAGEN_ERR_SHAPE, "sagen_render_fir: %ld rows of history before position %ld", (long)n_hist, (long)pos0);
    if (rot && (n_rot <= 0 || rot_hop <= 0)) return fail(SAGEN_ERR_SHAPE, "sagen_render_fir: n_rot=%d rot_hop=%d", n_rot, rot_hop);
    if (channels != 4 && channels != 9)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_render_fir: channels=%d (supported: 4 and 9, ambisonic orders 1 and 2)", channels);
    if (outputs > 32) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_render_fir: outputs=%d (supported: <= 32)", outputs);
    if (ntaps > 512) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_render_fir: ntaps=%d (supported: <= 512)", ntaps);
    if (n > ((int64_t)1 << 40)) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_render_fir: n=%ld rows in one call", (long)n);
    if (channels == 4 && ((uintptr_t)x) % 16) return fail(SAGEN_ERR_SHAPE, "sagen_render_fir: a 4-channel x must be 16-byte aligned");
    return run_render_fir(x, n_hist, n, channels, taps, outputs, ntaps, rot, n_rot, rot_hop, pos0, zero_before, y, stream);
}

size_t sagen_power_map_windows_scratch_bytes(int n_maps, int channels) {
    if (n_maps <= 0 || (channels != 4 && channels != 9)) return 0;
    return (size_t)n_maps * (channels * (channels + 1) / 2) * sizeof(double);
}

int sagen_power_map_windows(const float* ambi, int64_t n_rows, int channels, int stride, int64_t window, const float* sh, int p, float* rms,
                            void* scratch, size_t scratch_bytes, void* stream) {
    if (n_rows < 0 || stride <= 0 || window <= 0 || p <= 0)
        return fail(SAGEN_ERR_SHAPE, "sagen_power_map_windows: n_rows=%ld stride=%d window=%ld p=%d", (long)n_rows, stride, (long)window, p);
    if (channels != 4 && channels != 9)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_power_map_windows: channels=%d (supported: 4 and 9, ambisonic orders 1 and 2)", channels);
    const int64_t n_maps = overlay_n_maps(n_rows, stride, window);
    if (n_maps == 0) return SAGEN_OK;                  // (before the pointers are looked at: an empty stream has none)
    if (!ambi || !sh || !rms) return fail(SAGEN_ERR_NULL, "sagen_power_map_windows: null argument");
    if (n_maps * ((p + 255) / 256) > (int64_t)0x7fffffff)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_power_map_windows: %ld maps of %d nodes in one call", (long)n_maps, p);
    if (!scratch || scratch_bytes < sagen_power_map_windows_scratch_bytes((int)n_maps, channels))
        return fail(SAGEN_ERR_WORKSPACE, "sagen_power_map_windows: scratch too small (%ld maps)", (long)n_maps);
    if (((uintptr_t)scratch) % 8 || (channels == 4 && ((uintptr_t)ambi) % 16))
        return fail(SAGEN_ERR_SHAPE, "sagen_power_map_windows: scratch must be 8-byte aligned, a 4-channel ambi 16-byte aligned");
    return run_power_map_windows(ambi, channels, stride, window, (int)n_maps, sh, p, rms, (double*)scratch, stream);
}

size_t sagen_overlay_blend_scratch_bytes(int n_maps, int mh, int mw, int n_frames) {
    if (n_maps <= 0 || mh <= 0 || mw <= 0 || n_frames <= 0) return 0;
    return overlay_blend_grid_bytes(mh, mw, n_frames) + (size_t)n_frames * 4 * sizeof(double);
}

int sagen_overlay_blend(const float* maps, int n_maps, int64_t map0, int mh, int mw, const double* lut, const uint8_t* frames, int n_frames,
                        int64_t frame0, int h, int w, int frames_per_map, uint8_t* out, void* scratch, size_t scratch_bytes, void* stream) {
    if (n_maps < 0 || map0 < 0 || mh <= 0 || mw <= 0 || n_frames < 0 || frame0 < 0 || h <= 0 || w <= 0 || frames_per_map <= 0)
        return fail(SAGEN_ERR_SHAPE, "sagen_overlay_blend: n_maps=%d map0=%ld map %dx%d n_frames=%d frame0=%ld frame %dx%d frames_per_map=%d", n_maps,
                    (long)map0, mh, mw, n_frames, (long)frame0, h, w, frames_per_map);
    if (n_frames == 0) return SAGEN_OK;
    if (!maps || !lut || !frames || !out) return fail(SAGEN_ERR_NULL, "sagen_overlay_blend: null argument");
    // prev = F / frames_per_map grows with F: the first and the last frame decide
    const int64_t first = frame0 / frames_per_map, last = (frame0 + n_frames - 1) / frames_per_map + 1;
    if (first < map0 || last >= map0 + n_maps)
        return fail(SAGEN_ERR_SHAPE, "sagen_overlay_blend: frames %ld..%ld need the maps %ld..%ld, given %ld..%ld", (long)frame0,
                    (long)(frame0 + n_frames - 1), (long)first, (long)last, (long)map0, (long)(map0 + n_maps - 1));
    if (mw > 1000 || mh > 4096 || h > 65535 || w > (1 << 20) || n_frames > 65535)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_overlay_blend: map %dx%d frame %dx%d n_frames=%d (supported: map <= 4096 x 1000, h, n_frames <= 65535, w <= 1048576)",
                    mh, mw, h, w, n_frames);
    if (!scratch || scratch_bytes < sagen_overlay_blend_scratch_bytes(n_maps, mh, mw, n_frames))
        return fail(SAGEN_ERR_WORKSPACE, "sagen_overlay_blend: scratch too small");
    if (((uintptr_t)scratch) % 16 || ((uintptr_t)lut) % 8)
        return fail(SAGEN_ERR_SHAPE, "sagen_overlay_blend: scratch must be 16-byte aligned, lut 8-byte aligned");
    return run_overlay_blend(maps, map0, mh, mw, lut, frames, n_frames, frame0, h, w, frames_per_map, out, scratch, stream);
}

int sagen_source_track(const double* ctrl, const int32_t* pt_off, const int64_t* nframes, const double* duration, int n_sources, double rate,
                       int64_t t0, int64_t n, int64_t stride, const double* dirs, int n_dirs, double* unit, int32_t* nearest, void* stream) {
    if (!unit && !nearest) return fail(SAGEN_ERR_NULL, "sagen_source_track: null argument (unit and nearest)");
    if (nearest && !dirs) return fail(SAGEN_ERR_NULL, "sagen_source_track: nearest needs dirs");
    if (n < 1 || stride < 1 || (nearest && n_dirs < 1)) return fail(SAGEN_ERR_SHAPE, "sagen_source_track: n=%ld stride=%ld n_dirs=%d", (long)n, (long)stride, n_dirs);
    if (nearest && n_dirs > SRC_MAX_DIRS) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_source_track: n_dirs=%d (supported: <= %d)", n_dirs, SRC_MAX_DIRS);
    if (n > SRC_MAX_N / SRC_MAX_SOURCES) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_source_track: n=%ld samples in one call", (long)n);
    SourceSet ss;
    const int rc = source_fill("sagen_source_track", ss, ctrl, pt_off, nframes, duration, n_sources, rate, t0, t0 + (n - 1) * stride);
    if (rc != SAGEN_OK) return rc;
    return run_source_track(ctrl, ss, t0, n, stride, dirs, n_dirs, unit, nearest, stream);
}

int sagen_encode_sources(const float* signals, int64_t ld, const double* ctrl, const int32_t* pt_off, const int64_t* nframes,
                         const double* duration, int n_sources, double rate, int channels, int distance_model, double radius, int64_t t0,
                         int64_t n, float* ambi, void* stream) {
    if (!signals || !ambi) return fail(SAGEN_ERR_NULL, "sagen_encode_sources: null argument");
    if (n < 1 || ld < 1 || channels < 1) return fail(SAGEN_ERR_SHAPE, "sagen_encode_sources: n=%ld ld=%ld channels=%d", (long)n, (long)ld, channels);
    if (channels != 4 && channels != 9)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_encode_sources: channels=%d (supported: 4 and 9, ambisonic orders 1 and 2)", channels);
    if (n > SRC_MAX_N) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_encode_sources: n=%ld samples in one call", (long)n);
    if (distance_model != 0 && !(distance_model == 1 && radius > 0.))
        return fail(SAGEN_ERR_SHAPE, "sagen_encode_sources: distance_model=%d radius=%g (0, or 1 with radius > 0)", distance_model, radius);
    SourceSet ss;
    const int rc = source_fill("sagen_encode_sources", ss, ctrl, pt_off, nframes, duration, n_sources, rate, t0, t0 + n - 1);
    if (rc != SAGEN_OK) return rc;
    if (ld < source_longest(ss)) return fail(SAGEN_ERR_SHAPE, "sagen_encode_sources: ld=%ld is shorter than a source's nframes", (long)ld);
    if (channels == 4 && ((uintptr_t)ambi) % 16) return fail(SAGEN_ERR_SHAPE, "sagen_encode_sources: a 4-channel ambi must be 16-byte aligned");
    return run_encode_sources(signals, ld, ctrl, ss, channels, distance_model, radius, t0, n, ambi, stream);
}

int sagen_binauralize_sources(const float* signals, int64_t ld, const double* ctrl, const int32_t* pt_off, const int64_t* nframes,
                              const double* duration, int n_sources, double rate, int mode, const double* dirs, const float* hrir, int n_dirs,
                              int ntaps, int64_t zero_before, int64_t t0, int64_t n, float* y, void* stream) {
    if (!signals || !y) return fail(SAGEN_ERR_NULL, "sagen_binauralize_sources: null argument");
    if (mode != SAGEN_SOURCES_MIC && mode != SAGEN_SOURCES_HRIR) return fail(SAGEN_ERR_SHAPE, "sagen_binauralize_sources: mode=%d", mode);
    if (mode == SAGEN_SOURCES_HRIR && (!dirs || !hrir)) return fail(SAGEN_ERR_NULL, "sagen_binauralize_sources: the hrir mode needs dirs and hrir");
    if (n < 1 || ld < 1 || (mode == SAGEN_SOURCES_HRIR && (n_dirs < 1 || ntaps < 1)))
        return fail(SAGEN_ERR_SHAPE, "sagen_binauralize_sources: n=%ld ld=%ld n_dirs=%d ntaps=%d", (long)n, (long)ld, n_dirs, ntaps);
    if (mode == SAGEN_SOURCES_HRIR && (n_dirs > SRC_MAX_DIRS || ntaps > SRC_MAX_TAPS))
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_binauralize_sources: n_dirs=%d ntaps=%d (supported: <= %d, <= %d)", n_dirs, ntaps, SRC_MAX_DIRS, SRC_MAX_TAPS);
    if (n > SRC_MAX_N) return fail(SAGEN_ERR_UNSUPPORTED, "sagen_binauralize_sources: n=%ld samples in one call", (long)n);
    SourceSet ss;
    const int rc = source_fill("sagen_binauralize_sources", ss, ctrl, pt_off, nframes, duration, n_sources, rate, t0, t0 + n - 1);
    if (rc != SAGEN_OK) return rc;
    if (ld < source_longest(ss)) return fail(SAGEN_ERR_SHAPE, "sagen_binauralize_sources: ld=%ld is shorter than a source's nframes", (long)ld);
    if (((uintptr_t)y) % 8) return fail(SAGEN_ERR_SHAPE, "sagen_binauralize_sources: y must be 8-byte aligned");
    return run_binauralize_sources(signals, ld, ctrl, ss, mode, dirs, hrir, n_dirs, ntaps, zero_before, t0, n, y, stream);
}

size_t sagen_reproject_scratch_bytes(int n, int dst_h, int dst_w, int supersample) {
    (void)n; (void)dst_h; (void)dst_w; (void)supersample;
    return 0;                                          // the kernel is fused: nothing is staged between passes
}

int sagen_reproject(const uint8_t* src, int n, int src_h, int src_w, const sagen_projection* src_proj, uint8_t* dst, int dst_h, int dst_w,
                    const sagen_projection* dst_proj, const double* rot, int n_rot, int supersample, void* scratch, size_t scratch_bytes,
                    void* stream) {
    (void)scratch; (void)scratch_bytes;
    if (n < 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0)
        return fail(SAGEN_ERR_SHAPE, "sagen_reproject: n=%d source %dx%d destination %dx%d", n, src_h, src_w, dst_h, dst_w);
    if (n == 0) return SAGEN_OK;
    if (!src || !dst || !src_proj || !dst_proj || (n_rot != 0 && !rot)) return fail(SAGEN_ERR_NULL, "sagen_reproject: null argument");
    ProjArgs a;
    const char* why;
    const int rc = proj_args_fill(a, n, src_h, src_w, src_proj, dst_h, dst_w, dst_proj, n_rot, supersample, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_reproject: %s (n=%d n_rot=%d supersample=%d source %dx%d kind %d, destination %dx%d kind %d)", why, n, n_rot,
                    supersample, src_h, src_w, src_proj->kind, dst_h, dst_w, dst_proj->kind);
    if (n_rot != 0 && ((uintptr_t)rot) % 8) return fail(SAGEN_ERR_SHAPE, "sagen_reproject: rot must be 8-byte aligned");
    return run_reproject(src, dst, rot, a, stream);
}

size_t sagen_optical_flow_scratch_bytes(int n_frames, int h, int w, int levels) {
    const char* why;
    if (n_frames <= 1 || flow_check_sizes(n_frames, h, w, levels, &why) != SAGEN_OK) return 0;
    return flow_scratch_doubles(n_frames, h, w, levels) * sizeof(double);
}

int sagen_optical_flow(const uint8_t* frames, int n_frames, int h, int w, const sagen_flow_params* p, float* flow, void* scratch,
                       size_t scratch_bytes, void* stream) {
    if (n_frames < 0) return fail(SAGEN_ERR_SHAPE, "sagen_optical_flow: n_frames=%d", n_frames);
    if (n_frames <= 1) return SAGEN_OK;
    if (!frames || !p || !flow || !scratch) return fail(SAGEN_ERR_NULL, "sagen_optical_flow: null argument");
    FlowArgs a;
    const char* why;
    const int rc = flow_args_fill(a, n_frames, h, w, p, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_optical_flow: %s (n_frames=%d h=%d w=%d levels=%d warps=%d iters=%d fuse=%d alpha=%g)", why, n_frames, h, w,
                    p->levels, p->warps, p->iters, p->fuse, p->alpha);
    const size_t need = flow_scratch_doubles(n_frames, h, w, a.levels) * sizeof(double);
    if (scratch_bytes < need) return fail(SAGEN_ERR_SHAPE, "sagen_optical_flow: scratch_bytes=%zu, %zu needed", scratch_bytes, need);
    if (((uintptr_t)scratch) % 8) return fail(SAGEN_ERR_SHAPE, "sagen_optical_flow: scratch must be 8-byte aligned");
    return run_optical_flow(frames, a, flow, scratch, stream);
}

size_t sagen_flow_encode_scratch_bytes(int n, int h, int w) {
    (void)h; (void)w;
    return n > 0 ? (size_t)n * FLOW_ENC_PARTS * 2 * sizeof(float) : 0;
}

int sagen_flow_encode(const float* flow, int n, int h, int w, uint8_t* rgb, float* limits, void* scratch, size_t scratch_bytes,
                      void* stream) {
    if (n < 0) return fail(SAGEN_ERR_SHAPE, "sagen_flow_encode: n=%d", n);
    if (n == 0) return SAGEN_OK;
    const char* why;
    const int rc = flow_encode_check(n, h, w, &why);
    if (rc != SAGEN_OK) return fail(rc, "sagen_flow_encode: %s (n=%d h=%d w=%d)", why, n, h, w);
    if (!flow || !rgb || !limits || !scratch) return fail(SAGEN_ERR_NULL, "sagen_flow_encode: null argument");
    const size_t need = sagen_flow_encode_scratch_bytes(n, h, w);
    if (scratch_bytes < need) return fail(SAGEN_ERR_SHAPE, "sagen_flow_encode: scratch_bytes=%zu, %zu needed", scratch_bytes, need);
    if (((uintptr_t)scratch) % 4) return fail(SAGEN_ERR_SHAPE, "sagen_flow_encode: scratch must be 4-byte aligned");
    return run_flow_encode(flow, n, h, w, rgb, limits, scratch, stream);
}

int sagen_resample_fir(const float* x, int64_t x0, int64_t n_in, int c_in, const double* taps, int L, int M, int H, int T, const double* mix,
                       int c_out, int64_t n0, int64_t n, float* y, void* stream) {
    if (n < 0) return fail(SAGEN_ERR_SHAPE, "sagen_resample_fir: n=%ld", (long)n);
    if (n == 0) return SAGEN_OK;
    if (!taps || !y || (!x && n_in != 0)) return fail(SAGEN_ERR_NULL, "sagen_resample_fir: null argument");
    ResampleArgs a;
    const char* why;
    int rc = resample_args_fill(a, x0, n_in, c_in, L, M, H, T, mix != nullptr, c_out, n0, n, &why);
    if (rc == SAGEN_OK) rc = run_resample_fir(x, taps, mix, y, a, &why, stream);
    if (rc != SAGEN_OK && rc != SAGEN_ERR_HIP)
        return fail(rc, "sagen_resample_fir: %s (x0=%ld n_in=%ld c_in=%d L=%d M=%d H=%d T=%d c_out=%d n0=%ld n=%ld)", why, (long)x0, (long)n_in,
                    c_in, L, M, H, T, c_out, (long)n0, (long)n);
    return rc;
}

size_t sagen_jpeg_decode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs) {
    JpegGeom g;
    const char* why;
    if (n <= 0 || n_hufftabs < 1 || n_hufftabs > 65536 || jpeg_geom_fill(g, n, w, h, components, hs, vs, &why) != SAGEN_OK) return 0;
    return jpeg_scratch_layout(g, n_hufftabs).total;
}

int sagen_jpeg_decode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments,
                      int n_segments, const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, int w, int h,
                      int components, int hs, int vs, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    if (n == 0) return SAGEN_OK;
    JpegGeom g;
    const char* why;
    const int rc = jpeg_args_check(g, bytes, total_bytes, frames, n, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, w, h, components,
                                   hs, vs, out, status, scratch, scratch_bytes, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_jpeg_decode: %s (n=%d %dx%d components=%d sampling %dx%d total_bytes=%ld n_segments=%d n_qtabs=%d n_hufftabs=%d "
                    "scratch_bytes=%zu)", why, n, w, h, components, hs, vs, (long)total_bytes, n_segments, n_qtabs, n_hufftabs, scratch_bytes);
    return run_jpeg_decode(bytes, total_bytes, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch, stream);
}

size_t sagen_jpeg_encode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int64_t stride) {
    JpegEncGeom g;
    const char* why;
    if (n <= 0 || jpeg_enc_geom_fill(g, n, w, h, components, hs, vs, stride, &why) != SAGEN_OK) return 0;
    return jpeg_enc_scratch_layout(g).total;
}

int64_t sagen_jpeg_encode_max_bytes(int w, int h, int components, int hs, int vs) {
    JpegEncGeom g;
    const char* why;
    if (jpeg_enc_geom_fill(g, 1, w, h, components, hs, vs, 4, &why) != SAGEN_OK) return 0;
    return jpeg_enc_max_bytes(g.blocks);
}

int sagen_jpeg_encode(const uint8_t* frames, int n, int w, int h, int components, int hs, int vs, const uint16_t* qtabs, uint8_t* out,
                      int64_t stride, int32_t* sizes, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    if (n == 0) return SAGEN_OK;
    JpegEncGeom g;
    const char* why;
    const int rc = jpeg_enc_args_check(g, frames, n, w, h, components, hs, vs, qtabs, out, stride, sizes, status, scratch, scratch_bytes, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_jpeg_encode: %s (n=%d %dx%d components=%d sampling %dx%d stride=%ld scratch_bytes=%zu)", why, n, w, h, components, hs,
                    vs, (long)stride, scratch_bytes);
    return run_jpeg_encode(frames, g, qtabs, out, sizes, status, scratch, stream);
}

int sagen_window_rms(const float* x, int64_t n, int channels, int channel, int64_t first, int64_t hop, int64_t length, int64_t count,
                     double* rms, void* stream) {
    if (count < 0) return fail(SAGEN_ERR_SHAPE, "sagen_window_rms: count=%ld", (long)count);
    if (count == 0) return SAGEN_OK;
    if (!x || !rms) return fail(SAGEN_ERR_NULL, "sagen_window_rms: null argument");
    const char* why;
    const int rc = window_rms_check(n, channels, channel, first, hop, length, count, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_window_rms: %s (n=%ld channels=%d channel=%d first=%ld hop=%ld length=%ld count=%ld)", why, (long)n, channels,
                    channel, (long)first, (long)hop, (long)length, (long)count);
    return run_window_rms(x, channels, channel, first, hop, length, count, rms, stream);
}

}  // extern "C"
