// Baseline JPEG decode on the device (gfx950): file bytes in, [n][h][w][3] uint8 RGB out - include/sagen.h: sagen_jpeg_decode; the
// arithmetic is csrc/jpeg_core.h, shared with the CPU twin.  It replaces the host decode (PIL / libjpeg) in front of every frame
// consumer of the library, byte for byte.
//
//   jpeg_tables_kernel    one thread per Huffman table: counts + symbols -> the 8-bit lookahead table, the per-length largest code
//                         and the symbol offsets, in the scratch (global memory; frames of one folder share a handful of tables,
//                         which then sit in the L1 / L2 of every CU that decodes)
//   jpeg_check_kernel     one thread per frame: the descriptor and its segment rows against the buffer and the tables; writes the
//                         frame's initial status.  Nothing of a frame that fails here is touched by the later stages
//   jpeg_entropy_kernel   one LANE per restart segment (per frame where there is no restart interval): a 32-bit register bit
//                         window refilled from one cached aligned word, lookahead decode with a code-length search behind it, and
//                         int16 stores of the non-zero coefficients, undequantised and in natural order, straight into the
//                         coefficient buffer (zeroed by hipMemsetAsync ahead of the launch; no per-lane coefficient array).  The
//                         lanes of a wave walk different bitstreams and diverge by construction, so a launch with few segments
//                         spreads them thin: JPEG_ENTROPY_WAVES waves are filled one lane at a time before any wave gets a second
//   jpeg_idct_kernel      one thread per 8 x 8 block: dequantise, the islow inverse DCT with the block in statically indexed
//                         registers, eight 8-byte stores into the padded component plane
//   jpeg_pixel_kernel     one thread per output pixel: triangle upsampling of the two chroma planes, colour conversion, three byte
//                         stores (rows are 3 w bytes: nothing assumes an alignment)
//
// tools/jpeg_rate.py measures the stages; DESIGN.md says what is known about what bounds them.
#include "kernels.h"
#include "jpeg_core.h"

namespace sagen {

namespace {

constexpr int JPEG_THREADS = 256;
constexpr int JPEG_ENTROPY_WAVES = 2048;       // 256 CUs x 4 SIMDs x 2
constexpr int JPEG_GRID_FRAMES = 1024;

__global__ __launch_bounds__(64) void jpeg_tables_kernel(const uint8_t* __restrict__ specs, JpegHuff* __restrict__ huff, int n_hufftabs) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < n_hufftabs) jpeg_huff_build(specs + (size_t)t * JPEG_HUFF_SPEC, huff[t]);
}

__global__ __launch_bounds__(64) void jpeg_check_kernel(const sagen_jpeg_frame* __restrict__ frames, const int32_t* __restrict__ segments,
                                                        int n_segments, long long total_bytes, int n_qtabs, int n_hufftabs, const JpegGeom g,
                                                        const JpegHuff* __restrict__ huff, int32_t* __restrict__ status) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < g.n) status[f] = (int32_t)jpeg_check_frame(frames[f], f, segments, n_segments, total_bytes, n_qtabs, n_hufftabs, g, huff);
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* __restrict__ bytes, const sagen_jpeg_frame* __restrict__ frames,
                                                          const int32_t* __restrict__ segments, int n_segments, int lanes, const JpegGeom g,
                                                          const JpegHuff* __restrict__ huff, int16_t* __restrict__ coef, int32_t* status) {
    if ((int)threadIdx.x >= lanes) return;
    const long long s = (long long)blockIdx.x * lanes + threadIdx.x;
    if (s >= n_segments) return;
    const int f = segments[2 * s];
    if (f < 0 || f >= g.n) return;                                     // a row of no frame: nobody waits for it
    // (status[f] was written by jpeg_check_kernel, a launch ago; lanes of this launch only ever OR bits into it)
    if (__hip_atomic_load(&status[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE)) return;
    const sagen_jpeg_frame& fr = frames[f];                              // (by reference: a copy indexed by component would leave the registers)
    const long long k = s - fr.first_segment;
    if (k < 0 || k >= fr.n_segments) return;
    const uint32_t st = jpeg_decode_segment(bytes, fr, segments, (int)k, g, huff, coef + (size_t)f * g.blocks * 64);
    if (st) atomicOr(&status[f], (int32_t)st);
}

// the same for the frames sagen_jpeg_decode_split decodes again (jpeg_split.hip): gate[f] != 0, written launches ago and zeroed since
__global__ __launch_bounds__(64) void jpeg_entropy_redo_kernel(const uint8_t* __restrict__ bytes, const sagen_jpeg_frame* __restrict__ frames,
                                                               const int32_t* __restrict__ segments, int n_segments, int lanes, const JpegGeom g,
                                                               const JpegHuff* __restrict__ huff, int16_t* __restrict__ coef, int32_t* status,
                                                               const int32_t* __restrict__ gate) {
    if ((int)threadIdx.x >= lanes) return;
    const long long s = (long long)blockIdx.x * lanes + threadIdx.x;
    if (s >= n_segments) return;
    const int f = segments[2 * s];
    if (f < 0 || f >= g.n || !gate[f]) return;
    if (__hip_atomic_load(&status[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE)) return;
    const sagen_jpeg_frame& fr = frames[f];
    const long long k = s - fr.first_segment;
    if (k < 0 || k >= fr.n_segments) return;
    const uint32_t st = jpeg_decode_segment(bytes, fr, segments, (int)k, g, huff, coef + (size_t)f * g.blocks * 64);
    if (st) atomicOr(&status[f], (int32_t)st);
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const sagen_jpeg_frame* __restrict__ frames,
                                                                 const uint16_t* __restrict__ qtabs, const JpegGeom g,
                                                                 const int32_t* __restrict__ status, uint8_t* __restrict__ planes) {
    const long long id = (long long)blockIdx.x * JPEG_THREADS + threadIdx.x;
    if (id >= (long long)g.n * g.blocks) return;
    const int f = (int)(id / g.blocks), b = (int)(id - (long long)f * g.blocks);
    if (status[f] & SAGEN_JPEG_ST_DESC) return;                        // its table indices were never checked
    int comp, stride, x0, y0;
    size_t plane;
    jpeg_block_place(g, b / g.bpm, b % g.bpm, comp, plane, stride, x0, y0);
    const int qi = comp == 0 ? frames[f].qtab[0] : (comp == 1 ? frames[f].qtab[1] : frames[f].qtab[2]);
    uint8_t px[64];
    jpeg_idct_block(coef + id * 64, qtabs + (size_t)qi * 64, px);
    uint8_t* dst = planes + (size_t)f * g.plane_bytes + plane + (size_t)y0 * stride + x0;      // 8-byte aligned: every term is a multiple of 8
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = px[8 * r] | (px[8 * r + 1] << 8) | (px[8 * r + 2] << 16) | ((uint32_t)px[8 * r + 3] << 24);
        v.y = px[8 * r + 4] | (px[8 * r + 5] << 8) | (px[8 * r + 6] << 16) | ((uint32_t)px[8 * r + 7] << 24);
        *(uint2*)(dst + (size_t)r * stride) = v;
    }
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_pixel_kernel(const uint8_t* __restrict__ planes, const JpegGeom g,
                                                                  uint8_t* __restrict__ out) {
    const int pix = blockIdx.x * JPEG_THREADS + threadIdx.x;           // w h <= 2^28
    if (pix >= g.w * g.h) return;
    const int y = pix / g.w, x = pix - y * g.w;
    for (int f = blockIdx.y; f < g.n; f += gridDim.y) {
        uint8_t rgb[3];
        jpeg_pixel(g, planes + (size_t)f * g.plane_bytes, x, y, rgb);
        uint8_t* o = out + ((size_t)f * g.w * g.h + pix) * 3;
        o[0] = rgb[0], o[1] = rgb[1], o[2] = rgb[2];
    }
}

}  // namespace

// The first stages: zeroed coefficients, the derived tables, every frame's initial status.
int jpeg_front_launch(int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, int n_qtabs, const uint8_t* hufftabs,
                      int n_hufftabs, const JpegGeom& g, JpegHuff* huff, int16_t* coef, int32_t* status, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    SAGEN_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)g.n * g.blocks * 64 * sizeof(int16_t), s));
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3(cdiv(n_hufftabs, 64)), dim3(64), 0, s, hufftabs, huff, n_hufftabs);
    hipLaunchKernelGGL(jpeg_check_kernel, dim3(cdiv(g.n, 64)), dim3(64), 0, s, frames, segments, n_segments, total_bytes, n_qtabs, n_hufftabs, g,
                       huff, status);
    return SAGEN_OK;
}

// The three stages in front of the inverse DCT: the tables, the check and the entropy decode into the natural-order coefficients (zeroed
// here).  sagen_jpeg_transcode (jpeg_enc.hip) stops behind them; n_qtabs bounds the descriptors' table indices and nothing else.
int jpeg_coefficients_launch(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                             int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, JpegHuff* huff, int16_t* coef, int32_t* status,
                             void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const int rc = jpeg_front_launch(total_bytes, frames, segments, n_segments, n_qtabs, hufftabs, n_hufftabs, g, huff, coef, status, stream);
    if (rc != SAGEN_OK) return rc;
    int lanes = cdiv(n_segments, JPEG_ENTROPY_WAVES);
    lanes = lanes > 64 ? 64 : lanes;
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(cdiv(n_segments, lanes)), dim3(64), 0, s, bytes, frames, segments, n_segments, lanes, g, huff,
                       coef, status);
    return SAGEN_OK;
}

// one lane per segment of the frames with gate[f] != 0 (sagen_jpeg_decode_split's redo)
int jpeg_entropy_redo_launch(const uint8_t* bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments, const JpegGeom& g,
                             const JpegHuff* huff, int16_t* coef, int32_t* status, const int32_t* gate, void* stream) {
    int lanes = cdiv(n_segments, JPEG_ENTROPY_WAVES);
    lanes = lanes > 64 ? 64 : lanes;
    hipLaunchKernelGGL(jpeg_entropy_redo_kernel, dim3(cdiv(n_segments, lanes)), dim3(64), 0, (hipStream_t)stream, bytes, frames, segments, n_segments,
                       lanes, g, huff, coef, status, gate);
    return SAGEN_OK;
}

// the inverse DCT into the planes, upsampling and colour into out
int jpeg_back_launch(const sagen_jpeg_frame* frames, const uint16_t* qtabs, const JpegGeom& g, const int16_t* coef, const int32_t* status, uint8_t* planes,
                     uint8_t* out, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv((long)g.n * g.blocks, JPEG_THREADS)), dim3(JPEG_THREADS), 0, s, coef, frames, qtabs, g, status,
                       planes);
    hipLaunchKernelGGL(jpeg_pixel_kernel, dim3(cdiv((long)g.w * g.h, JPEG_THREADS), g.n < JPEG_GRID_FRAMES ? g.n : JPEG_GRID_FRAMES),
                       dim3(JPEG_THREADS), 0, s, planes, g, out);
    SAGEN_LAUNCH_CHECK();
    return SAGEN_OK;
}

int run_jpeg_decode(const uint8_t* bytes, int64_t total_bytes, const sagen_jpeg_frame* frames, const int32_t* segments, int n_segments,
                    const uint16_t* qtabs, int n_qtabs, const uint8_t* hufftabs, int n_hufftabs, const JpegGeom& g, uint8_t* out,
                    int32_t* status, void* scratch, void* stream) {
    const JpegScratch lay = jpeg_scratch_layout(g, n_hufftabs);
    JpegHuff* huff = (JpegHuff*)((char*)scratch + lay.huff);
    int16_t* coef = (int16_t*)((char*)scratch + lay.coef);
    uint8_t* planes = (uint8_t*)scratch + lay.planes;
    const int rc = jpeg_coefficients_launch(bytes, total_bytes, frames, segments, n_segments, n_qtabs, hufftabs, n_hufftabs, g, huff, coef, status, stream);
    if (rc != SAGEN_OK) return rc;
    return jpeg_back_launch(frames, qtabs, g, coef, status, planes, out, stream);
}

}  // namespace sagen
