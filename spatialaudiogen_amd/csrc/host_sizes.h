// Size arithmetic that the entry points (op_entries.h) check and the launchers carve by: plain host code, no HIP header, so that
// libsagen_hip.so and the CPU twin (csrc_cpu/sagen_cpu.cpp) compute the same numbers from the same lines.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sagen {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// power-map overlay (overlay.hip): the windows that fit into a strided stream; the blend's scratch starts with per-node
// (r, g, b, v) of every frame, then 4 doubles of clip bounds per frame
static inline int64_t overlay_n_maps(int64_t n_rows, int stride, int64_t window) { return ((n_rows + stride - 1) / stride) / window; }
static inline size_t overlay_blend_grid_bytes(int mh, int mw, int n_frames) { return align_up((size_t)n_frames * mh * mw * 4 * sizeof(double), 256); }

}  // namespace sagen
