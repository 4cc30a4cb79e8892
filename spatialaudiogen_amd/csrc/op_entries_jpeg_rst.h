// The extern "C" entry points of sagen_jpeg_encode_rst and sagen_jpeg_transcode, written ONCE for both libraries in the manner of op_entries.h and
// op_entries_png.h and included next to them, in the same translation unit of each library (api.hip, csrc_cpu/sagen_cpu.cpp).  It is a
// file of its own because the tests of those headers pin them against recorded fixtures, fail for fail;
// tests/test_jpeg_rst_host.py and tests/golden/op_refusals_jpeg_rst_v1.txt do the same for this one.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.  It reads no device memory.
#pragma once
#include "op_backends.h"
#include "jpeg_enc_core.h"

namespace sagen {
// the backend of sagen_jpeg_transcode (jpeg_enc.hip; csrc_cpu/sagen_cpu.cpp), after jpeg_transcode_args_check
int run_jpeg_transcode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                       const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& d, const JpegEncGeom& g, uint8_t* out, int32_t* sizes, int32_t* status,
                       void* scratch, void* stream);
}  // namespace sagen

extern "C" {

size_t sagen_jpeg_encode_rst_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int restart_interval, int64_t stride) {
    using namespace sagen;
    JpegEncGeom g;
    const char* why;
    if (n <= 0 || jpeg_enc_geom_fill(g, n, w, h, components, hs, vs, stride, &why) != SAGEN_OK) return 0;
    if (jpeg_enc_geom_rst(g, restart_interval, &why) != SAGEN_OK) return 0;
    return jpeg_enc_scratch_layout(g).total;
}

int64_t sagen_jpeg_encode_rst_max_bytes(int w, int h, int components, int hs, int vs, int restart_interval) {
    using namespace sagen;
    JpegEncGeom g;
    const char* why;
    if (jpeg_enc_geom_fill(g, 1, w, h, components, hs, vs, 4, &why) != SAGEN_OK) return 0;
    if (jpeg_enc_geom_rst(g, restart_interval, &why) != SAGEN_OK) return 0;
    return jpeg_enc_rst_max_bytes(g.blocks, g.nseg);
}

int sagen_jpeg_encode_rst(const uint8_t* frames, int n, int w, int h, int components, int hs, int vs, int restart_interval, const uint16_t* qtabs,
                          uint8_t* out, int64_t stride, int32_t* sizes, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    using namespace sagen;
    if (n == 0) return SAGEN_OK;
    JpegEncGeom g;
    const char* why;
    const int rc = jpeg_enc_args_check(g, frames, n, w, h, components, hs, vs, qtabs, out, stride, sizes, status, scratch, scratch_bytes, &why,
                                       restart_interval);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_jpeg_encode_rst: %s (n=%d %dx%d components=%d sampling %dx%d restart_interval=%d stride=%ld scratch_bytes=%zu)", why, n,
                    w, h, components, hs, vs, restart_interval, (long)stride, scratch_bytes);
    return run_jpeg_encode(frames, g, qtabs, out, sizes, status, scratch, stream);
}

size_t sagen_jpeg_transcode_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs, int restart_interval, int64_t stride) {
    using namespace sagen;
    JpegGeom d;
    JpegEncGeom g;
    const char* why;
    if (n <= 0 || jpeg_transcode_geom_fill(d, g, n, w, h, components, hs, vs, restart_interval, stride, n_hufftabs, &why) != SAGEN_OK) return 0;
    return jpeg_transcode_scratch_layout(d, g, n_hufftabs).total;
}

int64_t sagen_jpeg_transcode_max_bytes(int w, int h, int components, int hs, int vs, int restart_interval) {
    using namespace sagen;
    JpegGeom d;
    JpegEncGeom g;
    const char* why;
    if (jpeg_transcode_geom_fill(d, g, 1, w, h, components, hs, vs, restart_interval, 4, 1, &why) != SAGEN_OK) return 0;
    return jpeg_transcode_max_bytes(g.blocks, g.nseg);
}

int sagen_jpeg_transcode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments, int n_segments,
                         const uint8_t* hufftabs, int n_hufftabs, int w, int h, int components, int hs, int vs, int restart_interval, uint8_t* out,
                         int64_t stride, int32_t* sizes, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    using namespace sagen;
    if (n == 0) return SAGEN_OK;
    JpegGeom d;
    JpegEncGeom g;
    const char* why;
    const int rc = jpeg_transcode_args_check(d, g, bytes, total_bytes, frames, n, segments, n_segments, hufftabs, n_hufftabs, w, h, components, hs, vs,
                                             restart_interval, out, stride, sizes, status, scratch, scratch_bytes, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_jpeg_transcode: %s (n=%d %dx%d components=%d sampling %dx%d total_bytes=%ld n_segments=%d n_hufftabs=%d "
                    "restart_interval=%d stride=%ld scratch_bytes=%zu)", why, n, w, h, components, hs, vs, (long)total_bytes, n_segments, n_hufftabs,
                    restart_interval, (long)stride, scratch_bytes);
    return run_jpeg_transcode(bytes, total_bytes, frames, segments, n_segments, hufftabs, n_hufftabs, d, g, out, sizes, status, scratch, stream);
}

}  // extern "C"
