// The extern "C" entry point of sagen_assemble_audio, written ONCE for both libraries in the manner of op_entries.h and
// op_entries_feed.h and included next to them, in the same translation unit of each library (api.hip, csrc_cpu/sagen_cpu.cpp).  It is
// a file of its own because the tests of those two headers pin them against recorded fixtures, fail for fail;
// tests/test_op_refusals_audio_host.py and tests/golden/op_refusals_audio_v1.txt do the same for this one.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.  It reads no device memory.
#pragma once
#include "op_backends.h"
#include "audio_feed_core.h"

extern "C" {

int sagen_assemble_audio(const void* samples, int sample_type, int64_t n_samples, int channels, const int32_t* lead, const int64_t* read_from,
                         const int32_t* count, const double* rot, int n_out, int size, int t_off, int t_len, float* full, float* mono,
                         float* target, void* stream) {
    using namespace sagen;
    if (n_out < 0 || n_samples < 0)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: n_out=%d n_samples=%ld", n_out, (long)n_samples);
    if (n_out == 0) return SAGEN_OK;                   // (before the pointers are looked at: an empty batch has none)
    if (size < 1 || channels < 1) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: size=%d channels=%d", size, channels);
    if (sample_type != AUDIO_I16 && sample_type != AUDIO_F32 && sample_type != AUDIO_F64)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: sample_type=%d (0: int16, 1: float32, 2: float64)", sample_type);
    if (channels > AUDIO_FEED_MAX_CHANNELS)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_assemble_audio: %d channels (supported: <= %d)", channels, AUDIO_FEED_MAX_CHANNELS);
    if (size > AUDIO_FEED_MAX_SIZE)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_assemble_audio: windows of %d rows (supported: <= %d)", size, AUDIO_FEED_MAX_SIZE);
    if ((!samples && n_samples > 0) || !lead || !read_from || !count) return fail(SAGEN_ERR_NULL, "sagen_assemble_audio: null argument");
    if (!full && !mono && !target) return fail(SAGEN_ERR_NULL, "sagen_assemble_audio: no output asked for (full, mono and target are null)");
    if (rot && channels != 4)
        return fail(SAGEN_ERR_UNSUPPORTED, "sagen_assemble_audio: a rotation needs the 4 first-order channels, not %d", channels);
    if (target && channels == 1) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: a target needs channels >= 2");
    if (target && (t_off < 0 || t_len < 1 || t_off > size - t_len))
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: target rows t_off=%d t_len=%d of windows of %d", t_off, t_len, size);
    if (((uintptr_t)samples) % (uintptr_t)audio_feed_elem_bytes(sample_type))
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: samples must be %d-byte aligned", audio_feed_elem_bytes(sample_type));
    if (((uintptr_t)lead) % 4 || ((uintptr_t)count) % 4 || ((uintptr_t)read_from) % 8)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: lead and count must be 4-byte aligned, read_from 8-byte");
    if (((uintptr_t)rot) % 8) return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: rot must be 8-byte aligned");
    if (((uintptr_t)full) % 4 || ((uintptr_t)mono) % 4 || ((uintptr_t)target) % 4)
        return fail(SAGEN_ERR_SHAPE, "sagen_assemble_audio: full, mono and target must be 4-byte aligned");
    return run_assemble_audio(samples, sample_type, n_samples, channels, lead, read_from, count, rot, n_out, size, t_off, t_len, full, mono,
                              target, stream);
}

}  // extern "C"
