// A stand-alone runner of damaged JPEG streams through the host decode loop of csrc/jpeg_core.h (jpeg_decode_host: the loop the CPU
// twin runs, the arithmetic the kernels run), meant to be built with -fsanitize=address,undefined and run on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_mutate.cpp -o jpeg_mutate
//     ./jpeg_mutate cases.bin
//
// tests/test_cpu_twin_jpeg.py writes cases.bin (fixture streams truncated, with a Huffman symbol replaced, with a restart marker
// moved) and runs this.  Every array of a case is copied into a heap block of exactly its size, so a read or write one byte outside
// what include/sagen.h promises ends the run.  Per case: the call returns, every damaged frame has a status, every other frame has
// status 0 and exactly the expected pixels.  Nothing here touches a device.
//
// cases.bin: int32 count; per case int32 {n, n_segments, n_qtabs, n_hufftabs, w, h, components, hs, vs, total_bytes}, then
// frames [n][64 bytes], segments [n_segments][2] int32, qtabs [n_qtabs][64] uint16, hufftabs [n_hufftabs][272] uint8,
// bytes [total_bytes], damaged [n] int32, expected [n][h][w][3] uint8.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../spatialaudiogen_amd/csrc/jpeg_core.h"

namespace {

template <class T>
T* read_block(FILE* f, size_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (!p || fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "jpeg_mutate: short read\n");
        exit(2);
    }
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: jpeg_mutate cases.bin\n"), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "jpeg_mutate: cannot open %s\n", argv[1]), 2;
    int32_t* count = read_block<int32_t>(f, 1);
    int flagged = 0, kept = 0;
    for (int c = 0; c < *count; ++c) {
        int32_t* hd = read_block<int32_t>(f, 10);
        const int n = hd[0], n_segments = hd[1], n_qtabs = hd[2], n_hufftabs = hd[3], w = hd[4], h = hd[5];
        const long long total = hd[9];
        sagen_jpeg_frame* frames = read_block<sagen_jpeg_frame>(f, n);
        int32_t* segments = read_block<int32_t>(f, 2 * (size_t)n_segments);
        uint16_t* qtabs = read_block<uint16_t>(f, 64 * (size_t)n_qtabs);
        uint8_t* hufftabs = read_block<uint8_t>(f, 272 * (size_t)n_hufftabs);
        uint8_t* bytes = read_block<uint8_t>(f, (size_t)total);
        int32_t* damaged = read_block<int32_t>(f, n);
        const size_t frame_bytes = (size_t)h * w * 3;
        uint8_t* expected = read_block<uint8_t>(f, n * frame_bytes);
        uint8_t* out = (uint8_t*)malloc(n * frame_bytes);
        int32_t* status = (int32_t*)malloc(n * sizeof(int32_t));
        memset(out, 0, n * frame_bytes);
        sagen::JpegGeom g;
        const char* why;
        const size_t need = sagen::jpeg_scratch_layout((sagen::jpeg_geom_fill(g, n, w, h, hd[6], hd[7], hd[8], &why), g), n_hufftabs).total;
        void* scratch = malloc(need);
        const int rc = sagen::jpeg_args_check(g, bytes, total, frames, n, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, w, h, hd[6], hd[7],
                                              hd[8], out, status, scratch, need, &why);
        if (rc != SAGEN_OK) return fprintf(stderr, "jpeg_mutate: case %d refused: %s\n", c, why), 1;
        sagen::jpeg_decode_host(bytes, total, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch);
        for (int k = 0; k < n; ++k) {
            if (damaged[k]) {
                if (!status[k]) return fprintf(stderr, "jpeg_mutate: case %d: damaged frame %d has status 0\n", c, k), 1;
                ++flagged;
            } else {
                if (status[k] || memcmp(out + k * frame_bytes, expected + k * frame_bytes, frame_bytes))
                    return fprintf(stderr, "jpeg_mutate: case %d: intact frame %d has status %d or other pixels\n", c, k, status[k]), 1;
                ++kept;
            }
        }
        free(scratch), free(status), free(out), free(expected), free(damaged), free(bytes), free(hufftabs), free(qtabs), free(segments), free(frames), free(hd);
    }
    printf("jpeg_mutate: %d cases, %d damaged frames flagged, %d intact frames exact\n", *count, flagged, kept);
    free(count);
    fclose(f);
    return 0;
}
