// Exclusive prefix sums over a wavefront and over a workgroup of 256 threads, on the butterfly of wave_reduce.h (DPP inside a row,
// v_permlane swaps across rows: no LDS crossbar).  The JPEG encoder's bit and stuffing scans (jpeg_enc.hip) and the split decoder's
// chunk, block and DC scans (jpeg_split.hip) use them.  Every lane of the wave / every thread of the workgroup must call.
#pragma once
#include "wave_reduce.h"

namespace sagen {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;

// exclusive prefix sum over the 64 lanes (pre) and the wave's sum (tot), by the butterfly of wave_reduce.h: after the step of mask M
// tot is the sum of the lane's aligned group of 2 M lanes, and the lanes of its upper half have added the lower half's sum
template <int M = 1>
__device__ __forceinline__ void wave_scan(int lane, int& pre, int& tot) {
    if constexpr (M < 64) {
        int a, b;
        lane_pair<M>(tot, a, b);
        const int other = a + b - tot;
        if (lane & M) pre += other;
        tot = a + b;
        wave_scan<M * 2>(lane, pre, tot);
    }
}

// the same over the 256 threads of a workgroup; lds: SCAN_WAVES ints, free again on return
__device__ __forceinline__ int group_scan(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pre = 0, tot = v;
    wave_scan(lane, pre, tot);
    if (lane == 0) lds[wave] = tot;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < SCAN_WAVES; ++i) {
        const int t = lds[i];
        base += i < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return base + pre;
}

// the same for 0 <= v < 2^43 (256 of them stay below 2^51): the low 20 bits and the rest are scanned apart
__device__ __forceinline__ long long group_scan64(long long v, int* lds, long long& total) {
    int tl, th;
    const int lo = group_scan((int)(v & 0xFFFFF), lds, tl);
    const int hi = group_scan((int)(v >> 20), lds, th);
    total = ((long long)th << 20) + tl;
    return ((long long)hi << 20) + lo;
}

}  // namespace sagen
