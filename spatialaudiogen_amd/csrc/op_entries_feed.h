// The extern "C" entry point of sagen_assemble_frames, written ONCE for both libraries in the manner of op_entries.h and included
// next to it, in the same translation unit of each library (api.hip, csrc_cpu/sagen_cpu.cpp).  It is a file of its own only because
// tests/test_op_refusals_host.py pins op_entries.h against a recorded fixture, fail for fail; tests/test_op_refusals_feed_host.py and
// tests/golden/op_refusals_feed_v1.txt do the same for this one.  The two headers can be folded when that test is next revised.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.
#pragma once
#include "op_backends.h"
#include "feed_core.h"

extern "C" {

int sagen_assemble_frames(const uint8_t* frames, int n_frames, int h, int w, const int32_t* index, const int32_t* shift, int n_out, int mode,
                          const float* table, const double* scale_lo, void* out, void* stream) {
    using namespace sagen;
    if (n_out < 0 || n_frames < 0) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: n_out=%d n_frames=%d", n_out, n_frames);
    if (n_out == 0) return SAGEN_OK;                   // (before the pointers are looked at: an empty batch has none)
    if (h < 1 || w < 1) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: h=%d w=%d", h, w);
    if (h > FEED_MAX_DIM || w > FEED_MAX_DIM)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_assemble_frames: frame %dx%d (supported: <= %d)", h, w, FEED_MAX_DIM);
    if (mode != FEED_BYTES && mode != FEED_TABLE && mode != FEED_FLOW)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: mode=%d (0: bytes, 1: table[byte], 2: flow)", mode);
    if ((!frames && n_frames > 0) || !index || !shift || !out) return fail(SAGEN_ERR_NULL, "sagen_assemble_frames: null argument");
    if (mode != FEED_BYTES && !table) return fail(SAGEN_ERR_NULL, "sagen_assemble_frames: mode %d needs a table", mode);
    if (mode == FEED_FLOW && n_frames > 0 && !scale_lo) return fail(SAGEN_ERR_NULL, "sagen_assemble_frames: the flow mode needs scale_lo");
    if (mode != FEED_BYTES && (((uintptr_t)out) % 4 || ((uintptr_t)table) % 4))
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: a float out and the table must be 4-byte aligned");
    if (((uintptr_t)scale_lo) % 8) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: scale_lo must be 8-byte aligned");
    if (((uintptr_t)index) % 4 || ((uintptr_t)shift) % 4)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_frames: index and shift must be 4-byte aligned");
    return run_assemble_frames(frames, n_frames, h, w, index, shift, n_out, mode, table, scale_lo, out, stream);
}

}  // extern "C"
