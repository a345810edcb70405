// sliced.h -- the sliced pass: ordered compaction on the device without atomics on the data path.
//
// A fixed grid of at most BLOCKS workgroups of TILE lanes runs, and workgroup b owns the
// contiguous slice b of the input, in whole tiles.  A pass over the slices leaves one count per
// workgroup (block_count); a later pass takes the sum of the counts before its slice (block_base,
// slice_bases) and ranks the flagged lanes of every tile in order (tile_slot: ballot / popcount
// inside a wave, LDS counts across the four waves), which hands every position its slot.  Two
// kernel skeletons hold that arithmetic for the passes that are a predicate and an emit:
//   sliced_flag     a predicate per position -> flags[i] and one count per workgroup
//   sliced_compact  each workgroup takes the sum of the counts before it, ranks its flags in
//                   order and hands every position its slot
// Kernels that use the slices in ways of their own (object_index.hip, dedup_confirm.hip) call the
// primitives.  Header-only; every translation unit that includes it gets its own k_iota.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "sd_internal.h"

namespace sliced {

constexpr uint32_t TILE = 256;     // lanes of a workgroup = positions of a tile
constexpr uint32_t BLOCKS = 1024;  // most workgroups of a sliced pass (= the count slots per counter)
static_assert(sdk::OI_COUNT_SLOTS == BLOCKS, "the index's count slots are one per workgroup of a sliced pass");

struct slice { uint64_t lo, hi; };
__device__ __forceinline__ slice slice_of(uint64_t n) {
    const uint64_t per = ((n + gridDim.x - 1) / gridDim.x + TILE - 1) / TILE * TILE;  // whole tiles
    uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
    return {lo, hi};
}

// one lane per position, grid-stride past 4096 workgroups
inline uint32_t flat_grid(uint64_t n) {
    uint64_t g = (n + TILE - 1) / TILE;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (uint32_t)g;
}

inline uint32_t sliced_grid(uint64_t n) { return std::min<uint32_t>(flat_grid(n), BLOCKS); }

// The one workgroup reduction: v[k] <- the sum of v[k] over the 256 lanes, k < K, in every lane.
// Every lane calls it.  The first barrier also orders what the caller wrote to LDS before the
// call; the trailing one lets the next call reuse ws.
template <class T, int K>
__device__ __forceinline__ void block_sum(T (&v)[K]) {
    __shared__ T ws[4][K];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < K; k++) v[k] += __shfl_xor(v[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) ws[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ws[0][k] + ws[1][k] + ws[2][k] + ws[3][k];
    __syncthreads();
}

// workgroup total of `mine` -> counts[blockIdx.x], by lane 0
__device__ __forceinline__ void block_count(uint32_t mine, uint64_t* __restrict__ counts) {
    uint32_t v[1] = {mine};
    block_sum(v);
    if (threadIdx.x == 0) counts[blockIdx.x] = v[0];
}

// The prefix: base[c] <- the sum of counts[c * stride + k] over the slices k before this
// workgroup's, c < NC, in every lane.  ALL: all[c] <- the sum over every slice as well; the
// workgroup then reads gridDim.x counts per counter, not only the blockIdx.x before it.
template <int NC, bool ALL>
__device__ __forceinline__ void slice_bases(const uint64_t* __restrict__ counts, uint32_t stride,
                                            uint64_t (&base)[NC], uint64_t* __restrict__ all) {
    uint64_t v[ALL ? 2 * NC : NC];
#pragma unroll
    for (int c = 0; c < (ALL ? 2 * NC : NC); c++) v[c] = 0;
    const uint32_t end = ALL ? gridDim.x : blockIdx.x;
    for (uint32_t k = threadIdx.x; k < end; k += blockDim.x) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const uint64_t x = counts[c * stride + k];
            if (ALL) v[NC + c] += x;
            if (!ALL || k < blockIdx.x) v[c] += x;
        }
    }
    block_sum(v);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        base[c] = v[c];
        if (ALL) all[c] = v[NC + c];
    }
}

// sum of counts[0 .. blockIdx.x) for every lane; the last workgroup also writes the total
__device__ __forceinline__ uint64_t block_base(const uint64_t* __restrict__ counts, uint64_t* __restrict__ total) {
    uint64_t base[1];
    slice_bases<1, false>(counts, 0, base, nullptr);
    if (threadIdx.x == 0 && blockIdx.x + 1 == gridDim.x && total) *total = base[0] + counts[blockIdx.x];
    return base[0];
}

// this lane's output slot among the flagged lanes of the tile, in lane order; `run` (the
// slot of the tile's first flagged lane) advances by the tile's count.  A kernel may call it
// more than once per tile with the one wcnt: the second barrier comes after the last read of
// wcnt, so the next call's write cannot overtake it.
__device__ __forceinline__ uint64_t tile_slot(bool flag, uint64_t& run) {
    __shared__ uint32_t wcnt[4];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t bal = __ballot(flag);
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint64_t slot = run + __popcll(bal & ((1ull << lane) - 1));
    for (uint32_t k = 0; k < w; k++) slot += wcnt[k];
    const uint32_t all = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
    run += all;
    return slot;
}

// The flagging skeleton: workgroup b passes every position i of its slice of [0, n) and n to the
// functor, stores the answer at flags[i] (unless flags is null: a count-only pass) and leaves
// its count of true answers at counts[b].  n is *d_n if d_n is set (a count the host never
// waited for), else the value.  The functor may write side outputs of its own.
template <class F>
__global__ __launch_bounds__(256) void sliced_flag(F f, const uint64_t* __restrict__ d_n, uint64_t n,
                                                   uint8_t* __restrict__ flags, uint64_t* __restrict__ counts) {
    if (d_n) n = *d_n;
    const slice sl = slice_of(n);
    uint32_t mine = 0;
    for (uint64_t i = sl.lo + threadIdx.x; i < sl.hi; i += blockDim.x) {
        const bool flag = f(i, n);
        if (flags) flags[i] = flag ? 1 : 0;
        mine += flag;
    }
    block_count(mine, counts);
}

// The compaction skeleton over the same slices: slot = the flagged positions before i (counts[]
// of the flagging pass before this workgroup, tile_slot inside it), which is a flagged
// position's row of the output, and taken from i an unflagged position's rank among the
// unflagged.  Whole tiles: every lane of the workgroup makes the same trips (tile_slot has
// barriers); the lanes past the slice's end are unflagged and emit nothing.  f.flag(i) says
// whether i is flagged, f.emit(i, flag, slot, n) writes; *total (may be null) takes the count.
template <class F>
__global__ __launch_bounds__(256) void sliced_compact(F f, const uint64_t* __restrict__ d_n, uint64_t n,
                                                      const uint64_t* __restrict__ counts,
                                                      uint64_t* __restrict__ total) {
    uint64_t run = block_base(counts, total);
    if (d_n) n = *d_n;
    const slice sl = slice_of(n);
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi;
        const bool flag = act && f.flag(i);
        const uint64_t slot = tile_slot(flag, run);
        if (act) f.emit(i, flag, slot, n);
    }
}

// the flags of a sliced_flag pass, for the compactions that read them
struct from_flags {
    const uint8_t* __restrict__ flags;
    __device__ bool flag(uint64_t i) const { return flags[i] != 0; }
};

template <class F>
void launch_flag(uint32_t grid, hipStream_t s, F f, const uint64_t* d_n, uint64_t n, uint8_t* flags,
                 uint64_t* counts) {
    hipLaunchKernelGGL(sliced_flag<F>, dim3(grid), dim3(256), 0, s, f, d_n, n, flags, counts);
}

template <class F>
void launch_compact(uint32_t grid, hipStream_t s, F f, const uint64_t* d_n, uint64_t n, const uint64_t* counts,
                    uint64_t* total) {
    hipLaunchKernelGGL(sliced_compact<F>, dim3(grid), dim3(256), 0, s, f, d_n, n, counts, total);
}

static __global__ __launch_bounds__(256) void k_iota(uint64_t* __restrict__ p, uint64_t m) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = i;
}

inline size_t round256(size_t b) { return (b + 255) & ~size_t(255); }

// the temporary bytes of a u64 / u64 radix_sort_pairs of m
inline size_t sort_pairs_bytes(uint64_t m, hipStream_t s) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, b, nul, nul, nul, nul, (size_t)m, 0, 64, s) != hipSuccess) return 0;
    return round256(b);
}

}  // namespace sliced
