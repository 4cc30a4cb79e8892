// The host loop of sagen_jpeg_encode (csrc/jpeg_enc_core.h: jpeg_encode_host, what csrc_cpu/sagen_cpu.cpp calls) as a stand-alone program
// for a sanitizer build (tests/test_cpu_twin_jpeg_enc.py):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_check.cpp -o jpeg_encode_check
//     ./jpeg_encode_check cases.bin
//
// cases.bin: int32 count, then per case int32 {w, h, components, hs, vs, stream bytes}, uint16 qtabs[128] (zigzag order), the image and
// the stream PIL wrote.  Every array lives in a heap block of its exact size (the grey cases get 64 table entries, not 128), and each
// case runs at strides of 4, 64, exactly what it needs (rounded up to 4) and the bound: sizes must be exact at all of them, the bytes
// wherever they fit, and nothing may be written past a row.  Then the category function over |v| <= 2^15.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../spatialaudiogen_amd/csrc/jpeg_enc_core.h"

using namespace sagen;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: jpeg_encode_check cases.bin\n"), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    int32_t count = 0;
    if (!read_exact(f, &count, 4)) return 2;
    int runs = 0;
    for (int c = 0; c < count; ++c) {
        int32_t head[6];
        uint16_t q[128];
        if (!read_exact(f, head, sizeof head) || !read_exact(f, q, sizeof q)) return fprintf(stderr, "case %d: short file\n", c), 2;
        const int w = head[0], h = head[1], comps = head[2], hs = head[3], vs = head[4], want_bytes = head[5];
        const size_t image_bytes = (size_t)w * h * comps;
        uint8_t* image = (uint8_t*)malloc(image_bytes);
        uint8_t* want = (uint8_t*)malloc(want_bytes);
        uint16_t* qtabs = (uint16_t*)malloc((comps == 1 ? 64 : 128) * sizeof(uint16_t));
        if (!read_exact(f, image, image_bytes) || !read_exact(f, want, want_bytes)) return fprintf(stderr, "case %d: short file\n", c), 2;
        memcpy(qtabs, q, (comps == 1 ? 64 : 128) * sizeof(uint16_t));
        JpegEncGeom g;
        const char* why;
        if (jpeg_enc_geom_fill(g, 1, w, h, comps, hs, vs, 4, &why) != SAGEN_OK) return fprintf(stderr, "case %d: %s\n", c, why), 1;
        const long long strides[4] = {4, 64, (want_bytes + 3) / 4 * 4, (jpeg_enc_max_bytes(g.blocks) + 3) / 4 * 4};
        for (long long stride : strides) {
            if (jpeg_enc_geom_fill(g, 1, w, h, comps, hs, vs, stride, &why) != SAGEN_OK) return fprintf(stderr, "case %d: %s\n", c, why), 1;
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
        free(image), free(want), free(qtabs);
    }
    fclose(f);
    for (int v = -(1 << 15); v <= (1 << 15); ++v) {
        int n = 0;
        for (int a = v < 0 ? -v : v; a; a >>= 1) ++n;
        if (jpeg_enc_category(v) != n) return fprintf(stderr, "category(%d) = %d, want %d\n", v, jpeg_enc_category(v), n), 1;
        static const JpegEncHuff huff = jpeg_enc_huff_make();
        uint64_t bits;
        bool dc_range = false, ac_range = false;
        const int dc_len = jpeg_enc_code(huff, v & 1, true, 0, v, bits, dc_range);
        const int ac_len = v ? jpeg_enc_code(huff, v & 1, false, (v & 63) % 63, v, bits, ac_range) : 0;
        if (dc_range != (n > 11) || ac_range != (n > 10) || dc_len < 2 || dc_len > 22 || ac_len > 59)
            return fprintf(stderr, "code(%d): range %d %d, lengths %d %d\n", v, (int)dc_range, (int)ac_range, dc_len, ac_len), 1;
    }
    printf("jpeg_encode_check: %d cases, %d runs\n", count, runs);
    return 0;
}
