// blake3_cv.h -- chaining values between lanes: 32-byte CV moves, the level-wise LDS merge and the
// in-register CV stack that the hashing kernels of cas_kernels.hip and cdc.hip share.  Header-only;
// every translation unit that includes it gets its own copies (as sliced.h's k_iota).
#pragma once
#include <hip/hip_runtime.h>

#include "blake3_device.h"

namespace {

using namespace sdb3;

__device__ __forceinline__ void store_cv(uint32_t* dst, const uint32_t (&cv)[8]) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    d[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}
__device__ __forceinline__ void load_cv(uint32_t (&cv)[8], const uint32_t* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4 a = s[0], b = s[1];
    cv[0] = a.x; cv[1] = a.y; cv[2] = a.z; cv[3] = a.w;
    cv[4] = b.x; cv[5] = b.y; cv[6] = b.z; cv[7] = b.w;
}

// Level-wise merge of n (1..blockDim) CVs held in lds[0..n) -> lds[0].  ROOT goes on the
// final parent when `root`.  Every thread of the workgroup must call it.
template <bool W, bool SDWA16 = rotr16_sdwa(W)>
__device__ void lds_reduce(uint32_t (*lds)[8], uint32_t n, bool root) {
    const uint32_t t = threadIdx.x;
    while (n > 1) {
        const uint32_t P = n >> 1;
        const bool carry = n & 1u;
        uint32_t res[8];
        bool have = false;
        if (t < P) {
            uint32_t l[8], r[8];
            load_cv(l, lds[2 * t]);
            load_cv(r, lds[2 * t + 1]);
            parent<W, SDWA16>(res, l, r, (root && n == 2) ? ROOT : 0u);
            have = true;
        } else if (carry && t == P) {
            load_cv(res, lds[n - 1]);
            have = true;
        }
        __syncthreads();
        if (have) store_cv(lds[t], res);
        __syncthreads();
        n = P + (carry ? 1u : 0u);
    }
}

}  // namespace

// CvStack: the pending subtree CVs, top first, in registers with static indices only (a
// push shifts every entry down one slot), so a loop that is not unrolled can drive it.
template <int D>
struct CvStack {
    uint32_t s[D][8];
    __device__ __forceinline__ void push(const uint32_t (&c)[8]) {
#pragma unroll
        for (int d = D - 1; d > 0; d--)
#pragma unroll
            for (int i = 0; i < 8; i++) s[d][i] = s[d - 1][i];
#pragma unroll
        for (int i = 0; i < 8; i++) s[0][i] = c[i];
    }
    // c <- parent(top, c), and the top popped
    template <bool W>
    __device__ __forceinline__ void merge_top(uint32_t (&c)[8], uint32_t flags) {
        uint32_t r[8];
        sdb3::parent<W>(r, s[0], c, flags);
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = r[i];
#pragma unroll
        for (int d = 0; d + 1 < D; d++)
#pragma unroll
            for (int i = 0; i < 8; i++) s[d][i] = s[d + 1][i];
    }
};

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }
