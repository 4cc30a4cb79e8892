// What each library puts behind the shared entry points of the media ops (op_entries.h): sagen::fail and one backend per op, which
// is called with validated arguments only - the launcher of the op's .hip file in libsagen_hip.so, plain loops in the CPU twin
// (csrc_cpu/sagen_cpu.cpp), which ignores `stream` and whatever scratch it does not need.  Declarations only, no HIP header: every
// file that defines a backend sees this (the device's through kernels.h), so a signature cannot drift from its call.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sagen.h"

namespace sagen {

struct SourceSet;       // sources_core.h, filled by source_set_fill
struct ProjArgs;        // project_core.h, filled by proj_args_fill
struct FlowArgs;        // flow_core.h, filled by flow_args_fill
struct ResampleArgs;    // resample_core.h, filled by resample_args_fill
struct JpegGeom;        // jpeg_core.h, filled by jpeg_args_check; scratch as jpeg_scratch_layout carves it
struct JpegEncGeom;     // jpeg_enc_core.h, filled by jpeg_enc_args_check; scratch as jpeg_enc_scratch_layout carves it
struct DeflateGeom;     // png_core.h, filled by deflate_args_check; scratch as deflate_scratch_layout carves it

int fail(int code, const char* fmt, ...);      // writes the message sagen_last_error() returns, returns code

int run_eval_emd(const float* p, const float* q, int n_maps, int nodes, const double* cost, double* emd, uint32_t* not_converged, void* stream);
int run_render_fir(const float* x, int64_t n_hist, int64_t n, int channels, const float* taps, int outputs, int ntaps, const float* rot,
                   int n_rot, int rot_hop, int64_t pos0, int64_t zero_before, float* y, void* stream);
int run_power_map_windows(const float* ambi, int channels, int stride, int64_t window, int n_maps, const float* sh, int p, float* rms,
                          double* moments, void* stream);
int run_overlay_blend(const float* maps, int64_t map0, int mh, int mw, const double* lut, const uint8_t* frames, int n_frames,
                      int64_t frame0, int h, int w, int frames_per_map, uint8_t* out, void* scratch, void* stream);
int run_source_track(const double* ctrl, const SourceSet& ss, int64_t t0, int64_t n, int64_t stride, const double* dirs, int n_dirs,
                     double* unit, int32_t* nearest, void* stream);
int run_encode_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int channels, int distance_model,
                       double radius, int64_t t0, int64_t n, float* ambi, void* stream);
int run_binauralize_sources(const float* signals, int64_t ld, const double* ctrl, const SourceSet& ss, int mode, const double* dirs,
                            const float* hrir, int n_dirs, int ntaps, int64_t zero_before, int64_t t0, int64_t n, float* y, void* stream);
int run_reproject(const uint8_t* src, uint8_t* dst, const double* rot, const ProjArgs& a, void* stream);
int run_optical_flow(const uint8_t* frames, const FlowArgs& a, float* flow, void* scratch, void* stream);
int run_flow_encode(const float* flow, int n, int h, int w, uint8_t* rgb, float* limits, void* scratch, void* stream);
// may itself refuse: an error code other than SAGEN_ERR_HIP with *why set
int run_resample_fir(const float* x, const double* taps, const double* mix, float* y, const ResampleArgs& a, const char** why, void* stream);
int run_window_rms(const float* x, int channels, int channel, int64_t first, int64_t hop, int64_t length, int64_t count, double* rms,
                   void* stream);
int run_jpeg_decode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                    const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out,
                    int32_t* status, void* scratch, void* stream);
int run_jpeg_encode(const uint8_t* frames, const JpegEncGeom& g, const uint16_t* qtabs, uint8_t* out, int32_t* sizes, int32_t* status,
                    void* scratch, void* stream);
int run_assemble_frames(const uint8_t* frames, int n_frames, int h, int w, const int32_t* index, const int32_t* shift, int n_out, int mode,
                        const float* table, const double* scale_lo, void* out, void* stream);
int run_assemble_audio(const void* samples, int sample_type, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from,
                       const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono,
                       float* target, void* stream);
int run_png_filter(const uint8_t* frames, int n, int w, int h, int components, uint8_t* rows, void* stream);
int run_deflate(const uint8_t* data, const DeflateGeom& g, uint8_t* out, int32_t* sizes, int32_t* status, void* scratch, void* stream);

}  // namespace sagen
