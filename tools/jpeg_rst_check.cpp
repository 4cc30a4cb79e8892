// The host loops of sagen_jpeg_encode_rst and sagen_jpeg_transcode (csrc/jpeg_enc_core.h, what csrc_cpu/sagen_cpu.cpp calls) as
// a stand-alone program for a sanitizer build (tests/test_cpu_twin_jpeg_rst.py), in the manner of tools/jpeg_encode_check.cpp:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_rst_check.cpp -o jpeg_rst_check
//     ./jpeg_rst_check cases.bin
//
// cases.bin: int32 count, then per case int32 {w, h, components, hs, vs, restart interval, stream bytes}, uint16 qtabs[128] (zigzag
// order), the image and the stream PIL wrote (restart markers included).  Every array lives in a heap block of its exact size, and each
// case runs at strides of 4, 64, exactly what it needs (rounded up to 4) and the bound of sagen_jpeg_encode_rst_max_bytes: sizes must be
// exact at all of them and never above the bound, the bytes wherever they fit, and nothing may be written past a row.  Each case's
// plain stream (interval 0) then goes through the transcode path (jpeg_transcode_host) at the case's interval and must come out as
// PIL's stream, at the exact stride and at a stride of 4.  Then every
// interval 0..70 and 65535 over one frame: the segment count of the geometry, and interval 0 against the plain geometry.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../spatialaudiogen_amd/csrc/jpeg_enc_core.h"

using namespace sagen;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: jpeg_rst_check cases.bin\n"), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    int32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    int runs = 0, transcodes = 0;
    const char* why;
    for (int c = 0; c < count; ++c) {
        int32_t head[7];
        uint16_t q[128];
        if (!read_exact(f, head, sizeof head) || !read_exact(f, q, sizeof q)) return fprintf(stderr, "case %d: short file\n", c), 2;
        const int w = head[0], h = head[1], comps = head[2], hs = head[3], vs = head[4], rst = head[5], want_bytes = head[6];
        const size_t image_bytes = (size_t)w * h * comps;
        uint8_t* image = (uint8_t*)malloc(image_bytes);
        uint8_t* want = (uint8_t*)malloc(want_bytes);
        uint16_t* qtabs = (uint16_t*)malloc((comps == 1 ? 64 : 128) * sizeof(uint16_t));
        if (!read_exact(f, image, image_bytes) || !read_exact(f, want, want_bytes)) return fprintf(stderr, "case %d: short file\n", c), 2;
        memcpy(qtabs, q, (comps == 1 ? 64 : 128) * sizeof(uint16_t));
        JpegEncGeom g;
        if (jpeg_enc_geom_fill(g, 1, w, h, comps, hs, vs, 4, &why) != SAGEN_OK || jpeg_enc_geom_rst(g, rst, &why) != SAGEN_OK)
            return fprintf(stderr, "case %d: %s\n", c, why), 1;
        const long long bound = jpeg_enc_rst_max_bytes(g.blocks, g.nseg);
        if (want_bytes > bound) return fprintf(stderr, "case %d: %d bytes above the bound %lld\n", c, want_bytes, bound), 1;
        const long long strides[4] = {4, 64, (want_bytes + 3) / 4 * 4, (bound + 3) / 4 * 4};
        for (long long stride : strides) {
            if (jpeg_enc_geom_fill(g, 1, w, h, comps, hs, vs, stride, &why) != SAGEN_OK || jpeg_enc_geom_rst(g, rst, &why) != SAGEN_OK)
                return fprintf(stderr, "case %d: %s\n", c, why), 1;
            uint8_t* out = (uint8_t*)malloc((size_t)stride);
            int32_t* sizes = (int32_t*)malloc(sizeof(int32_t));
            int32_t* status = (int32_t*)malloc(sizeof(int32_t));
            memset(out, 0xA5, (size_t)stride);
            jpeg_encode_host(image, g, qtabs, out, sizes, status);
            const int fits = want_bytes <= stride;
            if (sizes[0] != want_bytes || status[0] != (fits ? 0 : SAGEN_JPEG_ENC_ST_CAPACITY) || (fits && memcmp(out, want, want_bytes) != 0))
                return fprintf(stderr, "case %d at stride %lld: sizes %d (want %d) status %d\n", c, stride, sizes[0], want_bytes, status[0]), 1;
            free(out), free(sizes), free(status);
            ++runs;
        }
        // the transcode path: the plain stream of the same pixels (interval 0, at the bound) through jpeg_transcode_host at this interval
        // is the stream PIL wrote; heap blocks of exact sizes again, the scratch at what the layout asks for
        {
            JpegEncGeom plain;
            if (jpeg_enc_geom_fill(plain, 1, w, h, comps, hs, vs, (jpeg_enc_max_bytes(g.blocks) + 3) / 4 * 4, &why) != SAGEN_OK) return 1;
            uint8_t* src = (uint8_t*)malloc((size_t)plain.stride);
            int32_t sz = 0, st = 0;
            jpeg_encode_host(image, plain, qtabs, src, &sz, &st);
            if (st) return fprintf(stderr, "case %d: plain status %d\n", c, st), 1;
            const long long total_bytes = ((long long)sz + 3) / 4 * 4;
            uint8_t* bytes = (uint8_t*)calloc((size_t)total_bytes + 4, 1) ;
            memcpy(bytes, src, (size_t)sz);
            const JpegEncSpec* specs[4] = {&JPEG_ENC_DC_LUMA, &JPEG_ENC_AC_LUMA, &JPEG_ENC_DC_CHROMA, &JPEG_ENC_AC_CHROMA};
            uint8_t* huff = (uint8_t*)calloc(4 * JPEG_HUFF_SPEC, 1);
            for (int t = 0; t < 4; ++t) {
                memcpy(huff + t * JPEG_HUFF_SPEC, specs[t]->counts, 16);
                memcpy(huff + t * JPEG_HUFF_SPEC + 16, specs[t]->symbols, (size_t)specs[t]->n);
            }
            sagen_jpeg_frame* fr = (sagen_jpeg_frame*)calloc(1, sizeof(sagen_jpeg_frame));
            fr->scan_bytes = sz, fr->n_segments = 1;
            fr->dctab[1] = fr->dctab[2] = 2, fr->actab[0] = 1, fr->actab[1] = fr->actab[2] = 3;
            int32_t* segs = (int32_t*)calloc(2, sizeof(int32_t));
            const long long strides2[2] = {(want_bytes + 3) / 4 * 4, 4};
            for (long long stride : strides2) {
                JpegGeom d;
                JpegEncGeom tg;
                if (jpeg_transcode_geom_fill(d, tg, 1, w, h, comps, hs, vs, rst, stride, 4, &why) != SAGEN_OK) return fprintf(stderr, "case %d: %s\n", c, why), 1;
                if (want_bytes > jpeg_transcode_max_bytes(tg.blocks, tg.nseg)) return 1;
                const size_t need = jpeg_transcode_scratch_layout(d, tg, 4).total;
                void* scratch = aligned_alloc(16, need);
                uint8_t* out = (uint8_t*)malloc((size_t)stride);
                memset(out, 0xA5, (size_t)stride);
                int32_t* sizes = (int32_t*)malloc(4);
                int32_t* status = (int32_t*)malloc(4);
                jpeg_transcode_host(bytes, total_bytes, fr, segs, 1, huff, 4, d, tg, out, sizes, status, scratch);
                const int fits = want_bytes <= stride;
                if (sizes[0] != want_bytes || status[0] != (fits ? 0 : SAGEN_JPEG_ENC_ST_CAPACITY << 8) || (fits && memcmp(out, want, want_bytes) != 0))
                    return fprintf(stderr, "case %d transcode at stride %lld: sizes %d (want %d) status %d\n", c, stride, sizes[0], want_bytes, status[0]), 1;
                free(scratch), free(out), free(sizes), free(status);
                ++transcodes;
            }
            free(src), free(bytes), free(huff), free(fr), free(segs);
        }
        free(image), free(want), free(qtabs);
    }
    fclose(f);
    // 40 x 72 at 4:2:0: 3 x 5 MCUs of 6 blocks
    JpegEncGeom plain, g;
    if (jpeg_enc_geom_fill(plain, 1, 40, 72, 3, 2, 2, 4096, &why) != SAGEN_OK) return 1;
    for (int rst = 0; rst <= 71; ++rst) {
        const int r = rst == 71 ? 65535 : rst;
        if (jpeg_enc_geom_fill(g, 1, 40, 72, 3, 2, 2, 4096, &why) != SAGEN_OK || jpeg_enc_geom_rst(g, r, &why) != SAGEN_OK) return 1;
        const int nseg = r == 0 || r >= 15 ? 1 : (15 + r - 1) / r;
        if (g.nseg != nseg || g.seg_blocks != (nseg == 1 ? 90 : 6 * r) || g.cap < plain.cap || (nseg == 1 && g.cap != plain.cap) || g.cap % 16)
            return fprintf(stderr, "interval %d: nseg %d seg_blocks %d cap %lld\n", r, g.nseg, g.seg_blocks, g.cap), 1;
        if (jpeg_enc_scratch_layout(g).total < jpeg_enc_scratch_layout(plain).total) return 1;
        if (nseg == 1 && jpeg_enc_scratch_layout(g).total != jpeg_enc_scratch_layout(plain).total) return 1;
        for (int b = 0; b < g.blocks; ++b) {
            const int p = jpeg_enc_pred_block(g, b);
            if (p >= b || (p >= 0 && p / g.seg_blocks != b / g.seg_blocks)) return fprintf(stderr, "interval %d: block %d predicted by %d\n", r, b, p), 1;
        }
    }
    if (jpeg_enc_geom_rst(g, -1, &why) != SAGEN_ERR_UNSUPPORTED || jpeg_enc_geom_rst(g, 65536, &why) != SAGEN_ERR_UNSUPPORTED) return 1;
    printf("jpeg_rst_check: %d cases, %d runs, %d transcodes\n", count, runs, transcodes);
    return 0;
}
