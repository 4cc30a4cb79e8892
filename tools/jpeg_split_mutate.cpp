// A stand-alone runner of damaged JPEG streams through the host loop of the split decode (csrc/jpeg_split_core.h: jpeg_split_decode_host,
// the loop the CPU twin runs, the arithmetic the kernels of csrc/jpeg_split.hip run), meant to be built with
// -fsanitize=address,undefined and run on the CPU:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_split_mutate.cpp -o jpeg_split_mutate
//     ./jpeg_split_mutate cases.bin
//
// tests/test_cpu_twin_jpeg_split.py writes cases.bin in the format of tools/jpeg_mutate.cpp (the same mutations) and runs this.  Every
// array of a case is copied into a heap block of exactly its size - the scratch at exactly what the size query names for the exact
// chunk count - so a read or write one byte outside what include/sagen.h promises ends the run.  Per case, at chunk_bytes 16 and 64
// and rounds 1 and 8: status equals the one-lane host loop's for every frame; the pixels of every frame some stage decoded are equal;
// path is 0 for a frame the descriptor check refused, non-zero for every other frame with a status, and 0 or UNSETTLED for a frame
// without one.  Nothing here touches a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../spatialaudiogen_amd/csrc/jpeg_split_core.h"

namespace {

template <class T>
T* read_block(FILE* f, size_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (!p || fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "jpeg_split_mutate: short read\n");
        exit(2);
    }
    return p;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: jpeg_split_mutate cases.bin\n"), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "jpeg_split_mutate: cannot open %s\n", argv[1]), 2;
    int32_t* count = read_block<int32_t>(f, 1);
    long runs = 0, redone = 0;
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
        uint8_t* ref = (uint8_t*)malloc(n * frame_bytes);
        uint8_t* out = (uint8_t*)malloc(n * frame_bytes);
        int32_t* ref_status = (int32_t*)malloc(n * sizeof(int32_t));
        int32_t* status = (int32_t*)malloc(n * sizeof(int32_t));
        int32_t* path = (int32_t*)malloc(n * sizeof(int32_t));
        sagen::JpegGeom g;
        const char* why;
        if (sagen::jpeg_geom_fill(g, n, w, h, hd[6], hd[7], hd[8], &why) != SAGEN_OK) return fprintf(stderr, "jpeg_split_mutate: case %d: %s\n", c, why), 1;
        const size_t plain = sagen::jpeg_scratch_layout(g, n_hufftabs).total;
        void* scratch = malloc(plain);
        memset(ref, 0, n * frame_bytes);
        sagen::jpeg_decode_host(bytes, total, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, ref, ref_status, scratch);
        free(scratch);
        for (int chunk_bytes = 16; chunk_bytes <= 64; chunk_bytes *= 4) {
            // the exact chunk count, from the descriptors as the caller knows them (a refused frame's rows count too: a capacity, no promise)
            long long max_chunks = 0;
            for (int k = 0; k < n; ++k) {
                const int32_t* rows = segments + 2 * (size_t)frames[k].first_segment;
                for (int s = 0; s < frames[k].n_segments; ++s) {
                    const long long len = (s + 1 < frames[k].n_segments ? rows[2 * s + 3] - 2 : frames[k].scan_bytes) - rows[2 * s + 1];
                    max_chunks += len <= 0 ? 1 : (len + chunk_bytes - 1) / chunk_bytes;
                }
            }
            if (max_chunks < n_segments) max_chunks = n_segments;
            for (int rounds = 1; rounds <= 8; rounds *= 8) {
                const size_t need = sagen::jpeg_split_scratch_layout(g, n_hufftabs, n_segments, max_chunks).total;
                scratch = malloc(need);
                int rc = sagen::jpeg_args_check(g, bytes, total, frames, n, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, w, h, hd[6], hd[7], hd[8],
                                                out, status, scratch, (size_t)-1, &why);
                if (rc == SAGEN_OK) rc = sagen::jpeg_split_args_check(g, n_hufftabs, n_segments, chunk_bytes, rounds, max_chunks, path, need, &why);
                if (rc != SAGEN_OK) return fprintf(stderr, "jpeg_split_mutate: case %d refused: %s\n", c, why), 1;
                memset(out, 0, n * frame_bytes);
                sagen::jpeg_split_decode_host(bytes, total, frames, segments, n_segments, qtabs, n_qtabs, hufftabs, n_hufftabs, g, out, status, scratch,
                                              chunk_bytes, rounds, max_chunks, path);
                free(scratch);
                ++runs;
                for (int k = 0; k < n; ++k) {
                    const bool refused = status[k] & (SAGEN_JPEG_ST_DESC | SAGEN_JPEG_ST_TABLE);
                    if (status[k] != ref_status[k]) return fprintf(stderr, "jpeg_split_mutate: case %d frame %d: status %d, one lane %d\n", c, k, status[k], ref_status[k]), 1;
                    if (!(status[k] & SAGEN_JPEG_ST_DESC) && memcmp(out + k * frame_bytes, ref + k * frame_bytes, frame_bytes))
                        return fprintf(stderr, "jpeg_split_mutate: case %d frame %d: other pixels than one lane (path %d)\n", c, k, path[k]), 1;
                    if (refused ? path[k] != 0 : (status[k] ? path[k] == 0 : (path[k] != 0 && path[k] != SAGEN_JPEG_PATH_UNSETTLED)))
                        return fprintf(stderr, "jpeg_split_mutate: case %d frame %d: path %d with status %d\n", c, k, path[k], status[k]), 1;
                    if (!damaged[k] && (status[k] || memcmp(out + k * frame_bytes, expected + k * frame_bytes, frame_bytes)))
                        return fprintf(stderr, "jpeg_split_mutate: case %d: intact frame %d has status %d or other pixels\n", c, k, status[k]), 1;
                    redone += path[k] != 0;
                }
            }
        }
        free(path), free(status), free(ref_status), free(out), free(ref), free(expected), free(damaged), free(bytes), free(hufftabs), free(qtabs), free(segments);
        free(frames), free(hd);
    }
    printf("jpeg_split_mutate: %d cases, %ld runs, %ld frames decoded again by one lane\n", *count, runs, redone);
    free(count);
    fclose(f);
    return 0;
}
