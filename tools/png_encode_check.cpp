// The host loops of sagen_png_filter and sagen_deflate (csrc/png_core.h: png_filter_host and deflate_host, what csrc_cpu/sagen_cpu.cpp
// calls) as a stand-alone program for a sanitizer build (tests/test_png_host.py):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_encode_check.cpp -o png_encode_check
//     ./png_encode_check cases.bin
//
// cases.bin: int32 count, then per deflate case int32 {n, length}, the n strings, and per string int32 bytes and the recorded stream;
// then int32 count and per filter case int32 {n, w, h, components}, the frames and the recorded rows.  Every array lives in a heap
// block of its exact size.  A deflate case runs with all its strings at strides of 4 and the bound, and each string alone at exactly
// what it needs (rounded up to 4): sizes must be exact at all of them, the bytes wherever they fit, and nothing may be written past a
// row.  Then the length symbols over 3..258 and the token rule over every (k, rem).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../spatialaudiogen_amd/csrc/png_core.h"

using namespace sagen;

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// one call on exact heap blocks; returns 0 when every frame's size, status and (where it fits) bytes are the recorded ones
static int run(const uint8_t* data, int n, long long length, long long stride, uint8_t* const* want, const int32_t* want_bytes) {
    DeflateGeom g;
    const char* why;
    if (deflate_geom_fill(g, n, length, stride, &why) != SAGEN_OK) return fprintf(stderr, "%s\n", why), 1;
    const size_t scratch_bytes = deflate_scratch_layout(g).total;
    uint8_t* out = (uint8_t*)malloc((size_t)n * stride);
    int32_t* sizes = (int32_t*)malloc(n * sizeof(int32_t));
    int32_t* status = (int32_t*)malloc(n * sizeof(int32_t));
    void* scratch = aligned_alloc(16, scratch_bytes);
    memset(out, 0xA5, (size_t)n * stride);
    if (deflate_args_check(g, data, n, length, out, stride, sizes, status, scratch, scratch_bytes, &why) != SAGEN_OK) return fprintf(stderr, "%s\n", why), 1;
    deflate_host(data, g, out, sizes, status, scratch);
    int bad = 0;
    for (int f = 0; f < n; ++f) {
        const bool fits = want_bytes[f] <= stride;
        if (sizes[f] != want_bytes[f] || status[f] != (fits ? 0 : SAGEN_DEFLATE_ST_CAPACITY) || sizes[f] > deflate_max_bytes(length)) bad = 1;
        if (fits && memcmp(out + (size_t)f * stride, want[f], want_bytes[f]) != 0) bad = 1;
        for (long long i = fits ? want_bytes[f] : stride; i < stride; ++i) bad |= out[(size_t)f * stride + i] != 0xA5;
        if (bad) return fprintf(stderr, "frame %d at stride %lld: sizes %d (want %d) status %d\n", f, stride, sizes[f], want_bytes[f], status[f]), 1;
    }
    free(out), free(sizes), free(status), free(scratch);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: png_encode_check cases.bin\n"), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    int32_t count = 0, filters = 0;
    if (!read_exact(f, &count, 4)) return 2;
    int runs = 0;
    for (int c = 0; c < count; ++c) {
        int32_t head[2];
        if (!read_exact(f, head, sizeof head)) return fprintf(stderr, "case %d: short file\n", c), 2;
        const int n = head[0];
        const long long length = head[1];
        uint8_t* data = length ? (uint8_t*)malloc((size_t)n * length) : nullptr;
        if (!read_exact(f, data, (size_t)n * length)) return 2;
        uint8_t** want = (uint8_t**)malloc(n * sizeof(uint8_t*));
        int32_t* want_bytes = (int32_t*)malloc(n * sizeof(int32_t));
        for (int i = 0; i < n; ++i) {
            if (!read_exact(f, want_bytes + i, 4)) return 2;
            want[i] = (uint8_t*)malloc(want_bytes[i]);
            if (!read_exact(f, want[i], want_bytes[i])) return 2;
        }
        const long long bound = (deflate_max_bytes(length) + 3) / 4 * 4;
        if (run(data, n, length, 4, want, want_bytes) || run(data, n, length, bound, want, want_bytes)) return fprintf(stderr, "case %d\n", c), 1;
        runs += 2;
        for (int i = 0; i < n; ++i, ++runs)
            if (run(data ? data + (size_t)i * length : nullptr, 1, length, (want_bytes[i] + 3) / 4 * 4, want + i, want_bytes + i)) return fprintf(stderr, "case %d\n", c), 1;
        for (int i = 0; i < n; ++i) free(want[i]);
        free(want), free(want_bytes), free(data);
    }
    if (!read_exact(f, &filters, 4)) return 2;
    for (int c = 0; c < filters; ++c) {
        int32_t head[4];
        if (!read_exact(f, head, sizeof head)) return 2;
        const int n = head[0], w = head[1], h = head[2], comps = head[3];
        const size_t in_bytes = (size_t)n * h * w * comps, out_bytes = (size_t)n * h * (1 + (size_t)w * comps);
        uint8_t* frames = (uint8_t*)malloc(in_bytes);
        uint8_t* want = (uint8_t*)malloc(out_bytes);
        uint8_t* rows = (uint8_t*)malloc(out_bytes);
        if (!read_exact(f, frames, in_bytes) || !read_exact(f, want, out_bytes)) return 2;
        const char* why;
        if (png_filter_args_check(frames, n, w, h, comps, rows, &why) != SAGEN_OK) return fprintf(stderr, "filter case %d: %s\n", c, why), 1;
        png_filter_host(frames, n, w, h, comps, rows);
        if (memcmp(rows, want, out_bytes) != 0) return fprintf(stderr, "filter case %d: other rows\n", c), 1;
        free(frames), free(want), free(rows);
    }
    fclose(f);
    for (int len = 3; len <= 258; ++len) {                               // RFC 1951, 3.2.5: the base lengths and extra bits of 257..285
        static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        static const int ebit[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
        int sym, ebits, extra, code = 28;
        while (base[code] > len) --code;
        png_length_symbol(len, sym, ebits, extra);
        if (sym != 257 + code || ebits != ebit[code] || extra != len - base[code] || png_length_extra_bits(sym) != ebits)
            return fprintf(stderr, "length %d: symbol %d, %d extra bits of value %d\n", len, sym, ebits, extra), 1;
    }
    for (int m = 1; m <= 1200; ++m) {                                    // a run of m bytes: its tokens cover it exactly
        int covered = 0;
        for (int k = 0; k < m; ++k) {
            int len;
            const int kind = png_token(k, m - k, len);
            if (kind == 1) covered += 1;
            if (kind == 2) covered += len;
            if (kind == 2 && (len < 3 || len > 258 || len > m - k)) return fprintf(stderr, "run %d: a match of %d at %d\n", m, len, k), 1;
        }
        if (covered != m) return fprintf(stderr, "run %d: %d bytes covered\n", m, covered), 1;
    }
    printf("png_encode_check: %d deflate cases, %d runs, %d filter cases\n", count, runs, filters);
    return 0;
}
