// dedup_confirm.hip -- confirm duplicate groups by full checksum (sd_dedup_confirm).
//
// Reference semantics: a cas_id samples files over 100 KiB (core/src/object/cas.rs:30-58), so
// files of one cas_id are candidates; file_checksum (core/src/object/validation/hash.rs:10-24)
// hashes every byte.  Per valid file i, group(i) = the valid files of its cas key, class(i) =
// those of them with the same 32 checksum bytes (include/sd_cas.h, sd_dedup_confirm).
//
// The permutation of the files by (invalid, key, checksum, position) comes from stable radix
// sorts of one 64-bit word each, least significant word first, every word gathered through the
// permutation so far (positions start ascending, so they stay ascending inside a run):
//   prefix path      h0 (checksum bytes 0..7 read as a big-endian number), key, invalid bit
//   full-width path  checksum words 3, 2, 1, 0, key, invalid bit
// The invalid files end up behind every valid one and are never a neighbour that counts.  One
// pass over the sorted order flags group heads (the key changes) and class heads (the key or any
// of the 32 bytes changes) and, on the prefix path, raises `tie` when two neighbours of one (key,
// h0) run differ in their last 24 bytes: adjacency then proves nothing (tails A, B, A), the later
// kernels of that pass write nothing and the host runs the full-width path.
//
// After the heads, sliced passes (sliced.h: a fixed grid in which workgroup b owns the contiguous
// slice b of the sorted order, in whole tiles): the heads before a position are the counts of the
// slices before it (slice_bases) plus its rank inside the tile (tile_slot), which gives every
// position its class and group slot and every head its row in cpos / gpos.  The kernels stand
// alone on that header's primitives: three counters per pass, the tie early-out and the capacity
// early-out do not fit its two skeletons.  A
// class's size is the distance to the next class head, its representative the position at its
// head.  One pass scatters rep, class_size and verdict to file order and reduces the totals (the
// only atomics: a few adds per workgroup); one more compacts the confirmed classes in order.
#include <hip/hip_runtime.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "sd_internal.h"
#include "sliced.h"

using namespace sliced;

namespace {

// flags[j] of sorted position j
constexpr uint8_t DC_VALID = 1, DC_GHEAD = 2, DC_CHEAD = 4;
// state (device u64): the eight stats, then
constexpr uint32_t DC_ST_TIE = 8;  // a (key, h0) run with unequal tails (prefix path only)

__device__ __forceinline__ uint64_t be64(uint64_t v) { return __builtin_bswap64(v); }

// the sort word of every position of the permutation: 0..3 = that checksum word as a big-endian
// number (the byte-swapped load: memcmp order), 4 = the key, 5 = 1 for an invalid file
__global__ __launch_bounds__(256) void k_dc_word(const uint64_t* __restrict__ keys,
                                                 const uint64_t* __restrict__ hash, const uint8_t* __restrict__ valid,
                                                 const uint64_t* __restrict__ perm, uint64_t m, int which,
                                                 uint64_t* __restrict__ out) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = perm[j];
        out[j] = which < 4 ? be64(hash[4 * p + which]) : which == 4 ? keys[p] : (valid && !valid[p] ? 1u : 0u);
    }
}

// Heads of the sorted order -> flags[j]; per slice the valid files, group heads and class heads
// -> counts[{0, 1, 2} * BLOCKS + blockIdx.x].  A valid position's predecessor is valid (the
// invalid files sort last).  `detect`: raise st[DC_ST_TIE] on unequal tails inside a (key, h0) run.
__global__ __launch_bounds__(256) void k_dc_heads(const uint64_t* __restrict__ keys,
                                                  const uint64_t* __restrict__ hash, const uint8_t* __restrict__ valid,
                                                  const uint64_t* __restrict__ perm, uint64_t m, int detect,
                                                  uint8_t* __restrict__ flags, uint64_t* __restrict__ counts,
                                                  uint64_t* __restrict__ st) {
    const slice sl = slice_of(m);
    uint32_t v[4] = {0, 0, 0, 0};  // valid files, group heads, class heads, ties
    for (uint64_t j = sl.lo + threadIdx.x; j < sl.hi; j += blockDim.x) {
        const uint64_t p = perm[j];
        uint8_t f = 0;
        if (!valid || valid[p]) {
            f = DC_VALID;
            bool ghead = j == 0, chead = ghead;
            if (!ghead) {
                const uint64_t q = perm[j - 1];
                ghead = keys[q] != keys[p];
                const bool h0_eq = hash[4 * q] == hash[4 * p];
                const bool tail_eq = hash[4 * q + 1] == hash[4 * p + 1] && hash[4 * q + 2] == hash[4 * p + 2] &&
                                     hash[4 * q + 3] == hash[4 * p + 3];
                chead = ghead || !h0_eq || !tail_eq;
                v[3] += !ghead && h0_eq && !tail_eq;
            }
            f |= (ghead ? DC_GHEAD : 0) | (chead ? DC_CHEAD : 0);
            v[0]++;
            v[1] += ghead;
            v[2] += chead;
        }
        flags[j] = f;
    }
    block_sum(v);
    if (threadIdx.x != 0) return;
    for (int c = 0; c < 3; c++) counts[c * BLOCKS + blockIdx.x] = v[c];
    if (detect && v[3]) st[DC_ST_TIE] = 1;  // same value from all
}

// Every valid position's class and group slot (the heads at or before it, less one) -> cslot,
// gslot; every head's position -> cpos[class slot], gpos[group slot]; the totals -> st[0] (valid
// files), st[1] (groups), st[3] (classes).  Whole tiles: every lane makes the same trips.
__global__ __launch_bounds__(256) void k_dc_rank(const uint8_t* __restrict__ flags, uint64_t m,
                                                 const uint64_t* __restrict__ counts, uint64_t* __restrict__ cslot,
                                                 uint64_t* __restrict__ gslot, uint64_t* __restrict__ cpos,
                                                 uint64_t* __restrict__ gpos, uint64_t* __restrict__ st) {
    uint64_t base[3], all[3];
    slice_bases<3, true>(counts, BLOCKS, base, all);
    if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = all[0], st[1] = all[1], st[3] = all[2];
    uint64_t grun = base[1], crun = base[2];
    const slice sl = slice_of(m);
    for (uint64_t b = sl.lo; b < sl.hi; b += blockDim.x) {
        const uint64_t j = b + threadIdx.x;
        const uint8_t f = j < sl.hi ? flags[j] : 0;
        const uint64_t gs = tile_slot(f & DC_GHEAD, grun);
        const uint64_t cs = tile_slot(f & DC_CHEAD, crun);
        if (!(f & DC_VALID)) continue;
        // position 0 is a head of both kinds: a follower has a head before it
        gslot[j] = (f & DC_GHEAD) ? gs : gs - 1;
        cslot[j] = (f & DC_CHEAD) ? cs : cs - 1;
        if (f & DC_GHEAD) gpos[gs] = j;
        if (f & DC_CHEAD) cpos[cs] = j;
    }
}

__device__ __forceinline__ uint64_t dc_run_size(const uint64_t* __restrict__ hpos, uint64_t slot, uint64_t heads,
                                                uint64_t nvalid) {
    return (slot + 1 < heads ? hpos[slot + 1] : nvalid) - hpos[slot];
}

// rep, class_size and verdict to file order (each may be null); the confirmed classes per slice
// -> counts[3 * BLOCKS + blockIdx.x]; st[2], [4], [5], [6], [7] by one add per workgroup each.
// Nothing happens once `tie` is up: the full-width pass follows.
__global__ __launch_bounds__(256) void k_dc_scatter(const uint64_t* __restrict__ perm,
                                                    const uint8_t* __restrict__ flags, uint64_t m,
                                                    const uint64_t* __restrict__ cslot,
                                                    const uint64_t* __restrict__ gslot,
                                                    const uint64_t* __restrict__ cpos,
                                                    const uint64_t* __restrict__ gpos, uint64_t* __restrict__ rep,
                                                    uint64_t* __restrict__ class_size, uint8_t* __restrict__ verdict,
                                                    uint64_t* __restrict__ counts, uint64_t* __restrict__ st) {
    if (st[DC_ST_TIE]) return;
    const uint64_t nvalid = st[0], groups = st[1], classes = st[3];
    const slice sl = slice_of(m);
    uint64_t v[5] = {0, 0, 0, 0, 0};  // candidate groups, confirmed classes, their files, refuted files, lying groups
    for (uint64_t j = sl.lo + threadIdx.x; j < sl.hi; j += blockDim.x) {
        const uint64_t p = perm[j];
        const uint8_t f = flags[j];
        if (!(f & DC_VALID)) {
            if (rep) rep[p] = ~0ull;
            if (class_size) class_size[p] = 0;
            if (verdict) verdict[p] = SD_CONFIRM_INVALID;
            continue;
        }
        const uint64_t cs = cslot[j];
        const uint64_t csize = dc_run_size(cpos, cs, classes, nvalid);
        const uint64_t gsize = dc_run_size(gpos, gslot[j], groups, nvalid);
        const uint8_t vd = gsize == 1 ? SD_CONFIRM_SINGLE : csize >= 2 ? SD_CONFIRM_CONFIRMED : SD_CONFIRM_REFUTED;
        if (rep) rep[p] = perm[cpos[cs]];
        if (class_size) class_size[p] = csize;
        if (verdict) verdict[p] = vd;
        if ((f & DC_GHEAD) && gsize >= 2) v[0]++, v[4] += csize < gsize;  // the head's class is not the whole group
        if ((f & DC_CHEAD) && csize >= 2) v[1]++, v[2] += csize;
        v[3] += vd == SD_CONFIRM_REFUTED;
    }
    block_sum(v);
    if (threadIdx.x != 0) return;
    counts[3 * BLOCKS + blockIdx.x] = v[1];
    const int at[5] = {2, 4, 5, 6, 7};
    for (int k = 0; k < 5; k++)
        if (v[k]) atomicAdd(reinterpret_cast<unsigned long long*>(st + at[k]), (unsigned long long)v[k]);
}

// One row (key, rep, size) per confirmed class in sorted order: ascending key, then ascending
// checksum.  Nothing is written when `tie` is up or the rows exceed `capacity`.
__global__ __launch_bounds__(256) void k_dc_sets(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ perm,
                                                 const uint8_t* __restrict__ flags, uint64_t m,
                                                 const uint64_t* __restrict__ cslot, const uint64_t* __restrict__ cpos,
                                                 const uint64_t* __restrict__ counts, const uint64_t* __restrict__ st,
                                                 uint64_t* __restrict__ sets, uint64_t capacity) {
    if (st[DC_ST_TIE]) return;
    uint64_t base[1], all[1];
    slice_bases<1, true>(counts + 3 * BLOCKS, 0, base, all);
    if (all[0] > capacity) return;
    const uint64_t nvalid = st[0], classes = st[3];
    uint64_t run = base[0];
    const slice sl = slice_of(m);
    for (uint64_t b = sl.lo; b < sl.hi; b += blockDim.x) {
        const uint64_t j = b + threadIdx.x;
        const uint8_t f = j < sl.hi ? flags[j] : 0;
        uint64_t csize = 0;
        if (f & DC_CHEAD) csize = dc_run_size(cpos, cslot[j], classes, nvalid);
        const uint64_t slot = tile_slot(csize >= 2, run);
        if (csize < 2) continue;
        const uint64_t p = perm[j];
        sets[3 * slot] = keys[p];
        sets[3 * slot + 1] = p;
        sets[3 * slot + 2] = csize;
    }
}

// scratch: a[6][m] u64 (perm, perm2, word / cpos, word2 / gpos, cslot, gslot), flags[m] u8,
// counts[4 * BLOCKS] u64, then the radix sort's temporary storage
struct dc_scratch {
    uint64_t *perm, *perm2, *word, *word2, *cslot, *gslot, *counts;
    uint8_t* flags;
    void* tmp;
};

dc_scratch dc_scratch_at(void* base, uint64_t m) {
    dc_scratch x;
    uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 255) & ~uintptr_t(255));
    uint64_t* u = reinterpret_cast<uint64_t*>(p);
    x.perm = u, x.perm2 = u + m, x.word = u + 2 * m, x.word2 = u + 3 * m, x.cslot = u + 4 * m, x.gslot = u + 5 * m;
    p += round256(6 * m * sizeof(uint64_t));
    x.flags = p;
    p += round256(m);
    x.counts = reinterpret_cast<uint64_t*>(p);
    p += round256(4 * BLOCKS * sizeof(uint64_t));
    x.tmp = p;
    return x;
}

}  // namespace

namespace sdk {

size_t dedup_confirm_scratch(uint64_t m) {
    return 256 + round256(6 * m * sizeof(uint64_t)) + round256(m) + round256(4 * BLOCKS * sizeof(uint64_t)) +
           sort_pairs_bytes(m, nullptr) + 256;
}

// One pass, queued on s: state[0..7] = the stats, state[8] = tie (prefix path only; then the
// outputs of this pass were not written and the caller runs it again with full = true).  m > 0.
hipError_t dedup_confirm(const uint64_t* keys, const uint8_t* hash32, const uint8_t* valid, uint64_t m, bool full,
                         uint64_t* rep, uint64_t* class_size, uint8_t* verdict, uint64_t* sets, uint64_t capacity,
                         uint64_t* state, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (m == 0 || scratch_bytes < dedup_confirm_scratch(m)) return hipErrorInvalidValue;
    const dc_scratch x = dc_scratch_at(scratch, m);
    const uint64_t* hash = reinterpret_cast<const uint64_t*>(hash32);
    hipError_t e = hipMemsetAsync(state, 0, DEDUP_CONFIRM_STATE * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    uint64_t *perm = x.perm, *perm2 = x.perm2;
    hipLaunchKernelGGL(k_iota, dim3(flat_grid(m)), dim3(256), 0, s, perm, m);
    const int prefix_words[] = {0, 4, 5}, full_words[] = {3, 2, 1, 0, 4, 5};
    const int* words = full ? full_words : prefix_words;
    const int nwords = full ? 6 : 3;
    const size_t temp = sort_pairs_bytes(m, s);
    for (int k = 0; k < nwords; k++) {
        if (words[k] == 5 && !valid) continue;  // every file is valid
        hipLaunchKernelGGL(k_dc_word, dim3(flat_grid(m)), dim3(256), 0, s, keys, hash, valid, perm, m, words[k],
                           x.word);
        size_t tb = temp;
        e = rocprim::radix_sort_pairs(x.tmp, tb, x.word, x.word2, perm, perm2, (size_t)m, 0, words[k] == 5 ? 1 : 64, s);
        if (e != hipSuccess) return e;
        std::swap(perm, perm2);
    }
    const uint32_t g = sliced_grid(m);
    uint64_t *cpos = x.word, *gpos = x.word2;  // the sort words are done with
    hipLaunchKernelGGL(k_dc_heads, dim3(g), dim3(256), 0, s, keys, hash, valid, perm, m, full ? 0 : 1, x.flags,
                       x.counts, state);
    hipLaunchKernelGGL(k_dc_rank, dim3(g), dim3(256), 0, s, x.flags, m, x.counts, x.cslot, x.gslot, cpos, gpos, state);
    hipLaunchKernelGGL(k_dc_scatter, dim3(g), dim3(256), 0, s, perm, x.flags, m, x.cslot, x.gslot, cpos, gpos, rep,
                       class_size, verdict, x.counts, state);
    if (sets)
        hipLaunchKernelGGL(k_dc_sets, dim3(g), dim3(256), 0, s, keys, perm, x.flags, m, x.cslot, cpos, x.counts, state,
                           sets, capacity);
    return hipGetLastError();
}

}  // namespace sdk
