// conv3h_kernel<.., AR, true> ("conv3s"): the 3x3 stride-2 SAME convolution of the first block of ResNet stages 3-5 (reference op tf.nn.convolution, core.py:206,
// as resnet.py:200-236 uses it) over fp16x2 activation planes in SPACE-TO-DEPTH form, on conv3h_kernel's K loop (conv3h_body.h).
//
// Before: these convs ran on conv3g_kernel, which gathers every K tile (tap, 16-channel chunk) by per-lane LDS-DMA.  Consecutive output
// pixels read input pixels two apart, so each gather used 64 B of every 128-byte line of the row-padded planes, and each of the nine
// taps fetched its own operand tile.
//
// Layout (written by the block merge in front of the conv: p3.hip, p3_pack_launch with s2d = 1).  H and W even, Ho = H/2, Wo = W/2:
// four phase images (r, c) = (h & 1, w & 1), image 2r + c an ordinary plane tensor [C/16][NPs][2][16] over the output grid with
// NPs = B*Ho*(Wo + 1) - one zero pixel closes every row - and the four back to back.  The padded pixel index
//     p = (b*Ho + ho)*(Wo + 1) + wo
// is the same in all four and is the index of output pixel (b, ho, wo).  Under TF SAME padding (top / left 0, bottom / right 1) tap
// (dh, dw) reads phase (dh & 1, dw & 1) at p + (dh >> 1)(Wo + 1) + (dw >> 1): the row's closing zero pixel is the right padding, the
// row below the image the bottom padding (and the boundary to the next image: masked per lane like conv3h_kernel's rows above / below).
//
// A tile is BM consecutive padded pixels: BM - 1 outputs and one halo pixel to the right.  Filter row dh is one barrier step, as in
// conv3h_kernel, and contracts the existing "pkh:" filter planes [tap][chunk][2][N][16] at taps 3 dh .. 3 dh + 2; its activation stage
// holds the two images (dh & 1, 0) and (dh & 1, 1) - 2 x BM x 64 B of contiguous, full-line DMA - and the taps dw = 0 / 1 / 2 read
// image 0 at slot r, image 1 at slot r, image 0 at slot r + 1.  A step carries three taps of MFMAs against 2 BM / 16 + 3 BN / 16 DMA
// instructions; the input is read 1.5 times (the row below a second time) instead of nine half-used gathers.
#include "conv3h_body.h"

namespace sagen {

// (An instantiation of the conv3h family by name too - conv3h_kernel<BM,BN,WM,WN,KC,AR,true>, a template of its own beside the five-
// parameter one of conv3h.hip: the tile table's set of kernel families is part of the library's interface, and the per-family
// accounting of the benchmark counts these launches among the fp16x2 contractions they are.)
template <int BM, int BN, int WM, int WN, int KC, int AR, bool S2D>
__global__ __launch_bounds__(256, conv3h_wgs_per_cu(BM, BN, KC, AR, true)) void conv3h_kernel(const IgemmDesc d_in) {
    IgemmDesc d = d_in;
    if (d.grp.G > 1) igemm_relocate(d, (int)blockIdx.z);              // grouped launch (common.h)
    static_assert(S2D, "the space-to-depth instantiations only");
    conv3h_body<BM, BN, WM, WN, KC, AR, true>(d);
}

template <int BM, int BN, int WM, int WN, int KC, int AR>
static int launch_conv3s(const IgemmDesc& d, hipStream_t s) {
    if ((d.Cin / 16) % KC) return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: %d channel chunks are not a multiple of %d per group", d.Cin / 16, KC);
    const int per = (cdiv(d.xs2d_np, BM - 1) + 7) / 8;
    const int grid = 8 * per * cdiv(d.N, BN);
    hipLaunchKernelGGL((conv3h_kernel<BM, BN, WM, WN, KC, AR, true>), dim3(grid, 1, d.grp.G), dim3(256), 0, s, d);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

// 3x3 stride-2 SAME conv (pad top / left 0) over even sizes, dense NHWC output, fp16x2 filter planes and the space-to-depth planes
bool conv3s_ok(const IgemmDesc& d) {
    if (!d.xs2d || d.xs2d_np <= 0 || !d.wh2 || !d.h2_a_inv || !d.h2_w_inv) return false;
    if (d.ntaps != 9 || d.TW != 3 || d.tap_sh != 1 || d.tap_sw != 1 || d.tap_h0 != 0 || d.tap_w0 != 0 || d.in_sh != 2 || d.in_sw != 2) return false;
    if ((d.Hin & 1) || (d.Win & 1) || d.Hg * 2 != d.Hin || d.Wg * 2 != d.Win || d.g_h0 != 0 || d.g_w0 != 0 || d.dsh * d.dsw != 1) return false;
    if (d.Cin % 16 || d.K != 9 * d.Cin || d.Kpad != d.K || d.in_scale != nullptr || d.bn_in.acc != nullptr) return false;
    if (d.M % (d.Hg * d.Wg) || d.xs2d_np != d.M / d.Wg * (d.Wg + 1)) return false;
    return d.y_rstride == (long)d.Wg * d.ldy && d.y_bstride == (long)d.Hg * d.Wg * d.ldy;
}

int conv3s_dispatch(const IgemmDesc& d_in, IgemmTile tile, hipStream_t s) {
    IgemmDesc d = d_in;
    if (!conv3s_ok(d)) return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: not a 3x3 stride-2 SAME conv over even sizes with its space-to-depth planes");
    if (d.splitk != 1) return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: no split-K");
    if ((long)(d.xs2d_np + 512) * (d.Wg + 1) >= (1L << 32) || ((long)(d.xs2d_np + 512) / (d.Wg + 1) + 1) * d.Hg >= (1L << 32))
        return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: too many pixels for 32-bit index arithmetic");
    const long x_bytes = 4L * (d.Cin / 16) * d.xs2d_np * 64;
    if (x_bytes >= (1L << 31) || d.xs2d_bytes != (unsigned)x_bytes)
        return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: the activation planes exceed 2 GiB buffer addressing (use a smaller batch) or their extent is wrong");
    const long y_bytes = ((long)(d.M - 1) * d.ldy + d.N) * 4;
    if (y_bytes >= (1L << 31)) return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: the output exceeds 2 GiB buffer addressing (use a smaller batch)");
    d.y_bytes = (unsigned)y_bytes;
    d.p3_magic_wp = (unsigned)((1UL << 32) / (unsigned)(d.Wg + 1)) + 1u;      // (here the divisors are the OUTPUT grid's Wg + 1, Hg)
    d.p3_magic_h = (unsigned)((1UL << 32) / (unsigned)d.Hg) + 1u;
#define SAGEN_TILE_HAS_P3S ,
    switch (tile) {
        SAGEN_TILES(SAGEN_TILE_CASE)
        default: return fail(SAGEN_ERR_UNSUPPORTED, "conv3s: bad tile id %d", (int)tile);
    }
}

}  // namespace sagen
