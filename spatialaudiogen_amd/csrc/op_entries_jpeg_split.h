// The extern "C" entry points of sagen_jpeg_decode_split, written ONCE for both libraries in the manner of op_entries_jpeg_rst.h and included
// next to it, in the same translation unit of each library (api.hip, csrc_cpu/sagen_cpu.cpp).  tests/test_jpeg_split_host.py and
// tests/golden/op_refusals_jpeg_split_v1.txt pin what it refuses, fail for fail.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.  It reads no device memory.
#pragma once
#include "op_backends.h"
#include "jpeg_split_core.h"

namespace sagen {
// the backend (jpeg_split.hip; csrc_cpu/sagen_cpu.cpp), after jpeg_args_check and jpeg_split_args_check
int run_jpeg_decode_split(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                          const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out, int32_t* status,
                          void* scratch, void* stream, int chunk_bytes, int rounds, int64_t max_chunks, int32_t* path);
}  // namespace sagen

extern "C" {

size_t sagen_jpeg_decode_split_scratch_bytes(int n, int w, int h, int components, int hs, int vs, int n_hufftabs, int n_segments, int64_t max_chunks) {
    using namespace sagen;
    JpegGeom g;
    const char* why;
    if (n <= 0 || n_hufftabs < 1 || n_hufftabs > 65536 || jpeg_geom_fill(g, n, w, h, components, hs, vs, &why) != SAGEN_OK) return 0;
    if (n_segments < n || max_chunks < n_segments || max_chunks > 0x7fffffffLL) return 0;
    return jpeg_split_scratch_layout(g, n_hufftabs, n_segments, max_chunks).total;
}

int sagen_jpeg_decode_split(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, int n, const int32_t* segments, int n_segments,
                            const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, int w, int h, int components, int hs, int vs,
                            uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes, void* stream, int chunk_bytes, int rounds,
                            int64_t max_chunks, int32_t* path) {
    using namespace sagen;
    if (n == 0) return SAGEN_OK;
    JpegGeom g;
    const char* why;
    // (the one-lane call's own scratch is a prefix of this one's: its size check cannot fail where the split's passes)
    int rc = jpeg_args_check(g, bytes, total_bytes, frames, n, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, w, h, components, hs, vs, out,
                             status, scratch, (size_t)-1, &why);
    if (rc == SAGEN_OK) rc = jpeg_split_args_check(g, n_hufftabs, n_segments, chunk_bytes, rounds, max_chunks, path, scratch_bytes, &why);
    if (rc != SAGEN_OK)
        return fail(rc, "sagen_jpeg_decode_split: %s (n=%d %dx%d components=%d sampling %dx%d total_bytes=%ld n_segments=%d n_qtabs=%d n_hufftabs=%d "
                    "chunk_bytes=%d rounds=%d max_chunks=%ld scratch_bytes=%zu)", why, n, w, h, components, hs, vs, (long)total_bytes, n_segments, n_qtabs,
                    n_hufftabs, chunk_bytes, rounds, (long)max_chunks, scratch_bytes);
    return run_jpeg_decode_split(bytes, total_bytes, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch, stream,
                                 chunk_bytes, rounds, max_chunks, path);
}

}  // extern "C"
