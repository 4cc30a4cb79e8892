// Which STFT frames may be asked for (include/sagen.h: sagen_stft_mag), written ONCE for both libraries: the launchers of fft.hip and
// the CPU twin (csrc_cpu/sagen_cpu.cpp) call this before anything is read, so what is refused, with which code and which message,
// cannot differ between them (the host tests call one table of refused calls against both).
//
// The rule is the reference's own frame count: myutils.stft (myutils.py:119-147) cuts n_samples / 1024 windows and, at hop 256, keeps
// 4 * (n_samples / 1024 - 1) frames; frame t covers samples [256 t, 256 t + 1024).  The last legal frame therefore ends at
// 1024 * (n_samples / 1024) - 256 <= n_samples: every legal frame fits, and the frames that merely fit behind them (200..202 of
// 52799 samples, or the one frame of 1024 samples) are refused because the reference never produces them.
//
// Host code only: no HIP header, compiles under hipcc and under plain g++ -std=c++17.
#pragma once
#include "op_backends.h"

namespace sagen {

inline int stft_frame_count(int n_samples) { return n_samples >= 1024 ? 4 * (n_samples / 1024 - 1) : 0; }

// SAGEN_OK, or SAGEN_ERR_SHAPE with the message set.  has_spec: a spec output is given, so [c0, c1) counts.
inline int stft_frames_check(int n_samples, int f0, int f1, bool has_spec, int c0, int c1) {
    const int nframes = stft_frame_count(n_samples);
    if (f0 < 0 || f1 <= f0 || f1 > nframes)
        return fail(SAGEN_ERR_SHAPE, "stft: frames [%d,%d) are not among the %d frames of %d samples", f0, f1, nframes, n_samples);
    if (has_spec && (c0 < f0 || c1 > f1 || c1 <= c0))
        return fail(SAGEN_ERR_SHAPE, "stft: spec frames [%d,%d) must lie in [%d,%d)", c0, c1, f0, f1);
    return SAGEN_OK;
}

}  // namespace sagen
