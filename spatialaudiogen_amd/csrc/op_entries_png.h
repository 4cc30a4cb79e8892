// The extern "C" entry points of sagen_png_filter and sagen_deflate, written ONCE for both libraries in the manner of op_entries.h,
// op_entries_feed.h and op_entries_audio.h and included next to them, in the same translation unit of each library (api.hip,
// csrc_cpu/sagen_cpu.cpp).  It is a file of its own because the tests of those headers pin them against recorded fixtures, fail for
// fail; tests/test_png_host.py and tests/golden/op_refusals_png_v1.txt do the same for this one.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.  It reads no device memory.
#pragma once
#include "op_backends.h"
#include "png_core.h"

extern "C" {

int sagen_png_filter(const uint8_t* frames, int n, int w, int h, int components, uint8_t* rows, void* stream) {
    using namespace sagen;
    if (n == 0) return SAGEN_OK;
    const char* why;
    const int rc = png_filter_args_check(frames, n, w, h, components, rows, &why);
    if (rc != SAGEN_OK) return fail(rc, "sagen_png_filter: %s (n=%d %dx%d components=%d)", why, n, w, h, components);
    return run_png_filter(frames, n, w, h, components, rows, stream);
}

int64_t sagen_deflate_max_bytes(int64_t length) {
    using namespace sagen;
    if (length < 0 || length > PNG_MAX_LENGTH) return 0;
    return deflate_max_bytes(length);
}

size_t sagen_deflate_scratch_bytes(int n, int64_t length, int64_t stride) {
    using namespace sagen;
    DeflateGeom g;
    const char* why;
    if (n <= 0 || deflate_geom_fill(g, n, length, stride, &why) != SAGEN_OK) return 0;
    return deflate_scratch_layout(g).total;
}

int sagen_deflate(const uint8_t* data, int n, int64_t length, uint8_t* out, int64_t stride, int32_t* sizes, int32_t* status, void* scratch,
                  size_t scratch_bytes, void* stream) {
    using namespace sagen;
    if (n == 0) return SAGEN_OK;
    DeflateGeom g;
    const char* why;
    const int rc = deflate_args_check(g, data, n, length, out, stride, sizes, status, scratch, scratch_bytes, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_deflate: %s (n=%d length=%ld stride=%ld scratch_bytes=%zu)", why, n, (long)length, (long)stride, scratch_bytes);
    return run_deflate(data, g, out, sizes, status, scratch, stream);
}

}  // extern "C"
