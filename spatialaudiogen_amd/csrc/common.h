// Shared host-side helpers of libsagen_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../include/sagen.h"
#include "switches.h"
#include "host_sizes.h"

namespace sagen {

char* err_buf();                       // thread-local message buffer (api.hip)
int   fail(int code, const char* fmt, ...);

#define SAGEN_HIP_CHECK(expr)                                                                   \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return ::sagen::fail(SAGEN_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,    \
                                 hipGetErrorString(e_));                                        \
    } while (0)

#define SAGEN_LAUNCH_CHECK() SAGEN_HIP_CHECK(hipGetLastError())

// ---- grouped launch (round 6: sagen_forward_grouped) ------------------------------------------------------------------------
// G INDEPENDENT batches of B windows run as ONE launch per layer: every kernel of the inference path takes the group index from
// its grid (blockIdx.z; igemm_kernel / igemm3_kernel: blockIdx.z / splitk) and sees exactly the single-batch problem - same tiles,
// same statistics, same scales, hence bit-identical results per group.  What differs per group is WHERE its tensors live: the
// workspace holds the per-batch region (activations, batch-norm accumulators, plane scales, split-K scratch, ...) G times at a
// constant stride, and a pointer that falls into group 0's copy [lo, lo + span) is moved g * stride further on (grp_ptr).  Pointers
// outside that range - packed filters, the caller's variables, null - are shared and stay.  The caller's own arrays (audio, frames,
// output) hold the G batches back to back and are moved by the explicit element strides of the three kernels that touch them.
struct GroupInfo {
    const char* lo = nullptr;
    unsigned long long span = 0, stride = 0;       // bytes
    int G = 1;
};
template <class T>
__device__ __forceinline__ T* grp_ptr(T* p, const GroupInfo& gi, int g) {
    const unsigned long long d = (unsigned long long)((const char*)p - gi.lo);
    return d < gi.span ? (T*)((char*)p + (unsigned long long)g * gi.stride) : p;
}
// in a kernel with a `const GroupInfo gi` parameter: pointer p of THIS workgroup's group (blockIdx.z)
#define SAGEN_GRP(p) (gi.G > 1 ? ::sagen::grp_ptr((p), gi, (int)blockIdx.z) : (p))
// On the host the group is an ARGUMENT like every other operand of a launch, never ambient state: a launcher whose kernel takes a
// group dimension has a required `const GroupInfo&` parameter, a contraction carries it in IgemmDesc::grp.  Fwd (model.h) holds the
// group of its context and passes it on; the op level, the training step and the weight gradients pass a default-constructed one
// (G = 1) in plain sight.  Launchers without the parameter run one group: Fwd refuses them in a grouped context (Fwd::timed_no_group).

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int ilog2_exact(int x) {   // -1 if not a power of two
    if (x <= 0 || (x & (x - 1))) return -1;
    int l = 0;
    while ((1 << l) < x) ++l;
    return l;
}

}  // namespace sagen
