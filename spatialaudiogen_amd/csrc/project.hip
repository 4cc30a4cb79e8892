// Reprojection of 360-degree frames (gfx950): equirectangular, cube-map and equi-angular cube-map frames into one another and
// into the pinhole view of a turned head - include/sagen.h: sagen_reproject; the geometry is csrc/project_core.h, shared with the
// CPU twin.  It replaces the reference's offline conversion (scraping/utils.py:91-144, scraping/preprocess.py:51-52, vrProjector).
//
//   project_kernel<SK, DK>   one thread per destination pixel, consecutive threads along a row; a workgroup row of the grid per
//                            frame, striding over the frames (n may exceed what gridDim.y takes).  The thread walks its S x S
//                            sub-samples: direction (fp64 sin / cos / tan of the destination kind), rotation, source coordinates
//                            (fp64 atan2 / atan of the source kind), four taps of three bytes each, fp64 sum; then three byte
//                            stores.  Rows are 3 W bytes and rectangles start anywhere, so every load and store is a byte: nothing
//                            here assumes an alignment.  The taps are clamped into their rectangle in proj_src_taps, whatever the
//                            rotation matrix holds.
//
// The kernel is fused: the coordinates are recomputed per frame even when all frames share one rotation.  tools/project_rate.py
// measures it; DESIGN.md 3.12 says what bounds each shape and why no precomputed-coordinate pass exists.
#include "kernels.h"
#include "project_core.h"

#pragma clang fp contract(off)

namespace sagen {

namespace {

constexpr int PROJ_THREADS = 256;
constexpr int PROJ_GRID_FRAMES = 1024;

template <int SK, int DK>
__global__ __launch_bounds__(PROJ_THREADS) void project_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const double* __restrict__ rot, const ProjArgs a) {
    const long long pix = (long long)blockIdx.x * PROJ_THREADS + threadIdx.x;
    if (pix >= (long long)a.dst.fh * a.dst.fw) return;
    const int py = (int)(pix / a.dst.fw), px = (int)(pix - (long long)py * a.dst.fw);
    int f, cx, cy, cw, ch;
    if (!proj_dst_cell<DK>(a.dst, px, py, f, cx, cy, cw, ch)) return;
    const long long src_bytes = (long long)a.src.fh * a.src.fw * 3, dst_bytes = (long long)a.dst.fh * a.dst.fw * 3;
    for (int fr = blockIdx.y; fr < a.n; fr += gridDim.y) {
        // the identity stands in for "no rotation": 1 x + 0 y + 0 z is x exactly, and the matrix stays in registers
        double r[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        if (a.n_rot > 0) {
            const double* g = rot + (a.n_rot == 1 ? 0 : (long long)fr * 9);
#pragma unroll
            for (int k = 0; k < 9; ++k) r[k] = g[k];
        }
        uint8_t out[3];
        proj_pixel<SK, DK>(a, src + fr * src_bytes, r, f, cx, cy, cw, ch, out);
        uint8_t* o = dst + fr * dst_bytes + pix * 3;
        o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    }
}

template <int SK>
void launch_dst(const uint8_t* src, uint8_t* dst, const double* rot, const ProjArgs& a, dim3 grid, hipStream_t s) {
    switch (a.dst.kind) {
        case SAGEN_PROJ_ER: hipLaunchKernelGGL((project_kernel<SK, SAGEN_PROJ_ER>), grid, dim3(PROJ_THREADS), 0, s, src, dst, rot, a); break;
        case SAGEN_PROJ_CUBE: hipLaunchKernelGGL((project_kernel<SK, SAGEN_PROJ_CUBE>), grid, dim3(PROJ_THREADS), 0, s, src, dst, rot, a); break;
        case SAGEN_PROJ_EAC: hipLaunchKernelGGL((project_kernel<SK, SAGEN_PROJ_EAC>), grid, dim3(PROJ_THREADS), 0, s, src, dst, rot, a); break;
        default: hipLaunchKernelGGL((project_kernel<SK, SAGEN_PROJ_VIEW>), grid, dim3(PROJ_THREADS), 0, s, src, dst, rot, a); break;
    }
}

}  // namespace

int run_reproject(const uint8_t* src, uint8_t* dst, const double* rot, const ProjArgs& a, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv((long)a.dst.fh * a.dst.fw, PROJ_THREADS), a.n < PROJ_GRID_FRAMES ? a.n : PROJ_GRID_FRAMES);
    switch (a.src.kind) {
        case SAGEN_PROJ_ER: launch_dst<SAGEN_PROJ_ER>(src, dst, rot, a, grid, s); break;
        case SAGEN_PROJ_CUBE: launch_dst<SAGEN_PROJ_CUBE>(src, dst, rot, a, grid, s); break;
        default: launch_dst<SAGEN_PROJ_EAC>(src, dst, rot, a, grid, s); break;
    }
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

}  // namespace sagen
