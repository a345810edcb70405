// cas_kernels.hip -- gfx950 kernels for Spacedrive's content-addressing hot path.
//
//   k_cas_sampled_lanes  generate_cas_id, size > 102400 (cas.rs:30-58): every message is
//   k_cas_sampled_merge  the same 57 352 B = 56 full chunks + one 8-byte chunk, so one lane
//                   per aligned 8-chunk group (7 per file) hashes its subtree, and one lane
//                   per file merges the 7 subtree CVs and the tail chunk.  No work lists.
//   k_whole_items   generate_cas_id, size <= 102400 (cas.rs:27-29): host-built work lists
//   k_whole_merge8  of aligned chunk pairs (full pairs of multi-pair messages, then the
//                   cost-sorted partial / short pairs), then two level-wise merge passes of
//                   <= 8 pair nodes per lane.
//   k_ck_leaf       file_checksum (hash.rs:10-24), and whole-file cas messages longer than
//   k_ck_reduce     the work-list path takes: 256 lanes per 1 MiB block of a message, two
//                   blocks per workgroup, 4 consecutive chunks per lane merged in-lane, each
//                   block's 256 lane CVs merged in LDS (both trees packed into the lowest
//                   lanes); then 256-way LDS reductions over the block CVs.
//   k_ck_leaf_tree  k_ck_leaf's body, also storing the LDS tree's level at 128 KiB .. 1 MiB
//                   granularity: the checksum trees (checksum_tree.hip).
//   k_ck_blocks     the nodes of listed blocks of at most 128 KiB .. 1 MiB that sit anywhere in a
//                   buffer: the leaf's lanes, 16 .. 2 items per workgroup, one item table.
//
// Tree shape: every merge is the level-wise pairwise merge with the odd node carried up
// unchanged, over power-of-two aligned groups.  It is the BLAKE3 tree (left subtree =
// largest power of two); tests/test_oracle.py checks the equivalence for 1..600 chunks.
#include <hip/hip_runtime.h>

#include "blake3_cv.h"
#include "blake3_device.h"
#include "sd_internal.h"

using namespace sdb3;

// ------------------------------------------------------------------------ sampled cas
// Every sampled message is the same 57 352 B = 56 full chunks + one 8-byte chunk (message
// bytes 57344..57351, chunk 56), so the launch shape needs no work lists:
constexpr int S_FULL = 56;  // full chunks per sampled message (57344 bytes)
#ifndef SD_SAMPLED_LANE_CHUNKS
#define SD_SAMPLED_LANE_CHUNKS 8  // chunks per lane (2, 4 or 8; scripts/sampled_ab.py)
#endif
constexpr int S_U = SD_SAMPLED_LANE_CHUNKS;
constexpr int S_K = S_FULL / S_U;  // nodes per file after the lanes kernel (7)
static_assert(S_U == 2 || S_U == 4 || S_U == 8, "chunks per lane");

// Two kernels, and no in-workgroup tree phase (round 2 measured a one-kernel design -- 16
// files per 7-wave workgroup, the 29 lane CVs of each merged level-wise in LDS -- 3.4%
// slower: the LDS rounds, barriers and partly-filled waves of its tree phase cost more than
// a second launch; profiles/r2/r2z_sampled_ab.json):
//   k_cas_sampled_lanes<U>  one lane per (file, aligned group of U chunks): 56/U lanes per
//                           file, 256-lane workgroups, no LDS, no barrier; the group's
//                           subtree CV -> node row j of the file, rows stored node-major
//                           (row (j, f) at (j * n + f) * 32 B) so the merge reads coalesce;
//   k_cas_sampled_merge<U>  one lane per file: the 56/U node CVs merged with BLAKE3's CV
//                           stack, then the 8-byte tail chunk (chunk 56) and the stack folded
//                           into the root.
// CvStack (blake3_cv.h) holds the pending subtree CVs of the merges below.

// CV of U (a power of two) consecutive full non-root chunks c0.. : U = 2 is full_chunks_cv's
// unrolled pair; larger groups merge each chunk into the stack as it completes.
// c0 is a chunk index of a sampled message (< 57) and 32 bits wide: as a uint64_t it and c0 + u
// each held a second register through the loops, and with the windows the lanes kernel took 81
// VGPRs, one over the 80 at which a sixth wave shares the SIMD.  Now 79 and 6 waves/SIMD, no
// scratch, no instruction added (profiles/g_rotr16/resource_usage.md; registers only, 5 -> 6
// waves is 61.8 -> 66.1 T lane-ops/s, profiles/g_rotr16/probe.txt).
template <int U, bool W>
__device__ __forceinline__ void group_cv(uint32_t (&out)[8], const uint8_t* __restrict__ p, uint32_t c0) {
    // sampled messages only: a caller with chunk indices of long messages needs full_chunks_cv's 64-bit counter
    static_assert((long long)S_FULL + 1 < (1ll << 32), "group_cv counts a sampled message's chunks in 32 bits");
    if constexpr (U <= 2) {
        full_chunks_cv<U, W>(out, p, c0);
    } else {
        CvStack<ilog2(U)> st;
        uint32_t ma[16], mb[16];
#pragma unroll 1
        for (uint32_t u = 0; u < (uint32_t)U; u++) {
            // chi = 0 holds for sampled messages only; the 64-bit counter of the long-message path is held by
            // tests/test_gpu_high_counter.py (test_split_leaves_past_2_32)
            const uint32_t clo = c0 + u, chi = 0u;
            const uint8_t* q = p + (size_t)u * CHUNK_LEN;
            set_iv(out);
#pragma unroll 1
            for (uint32_t b = 0; b < 16; b += 2) {
                load_block(ma, q + 64u * b);
                load_block(mb, q + 64u * (b + 1));
                compress<W>(out, ma, clo, chi, BLOCK_LEN, b == 0 ? CHUNK_START : 0u);
                compress<W>(out, mb, clo, chi, BLOCK_LEN, b + 1 == 15 ? CHUNK_END : 0u);
            }
#pragma unroll 1
            for (uint32_t t = u + 1; (t & 1u) == 0; t >>= 1) st.template merge_top<W>(out, 0u);
            if (u + 1 < (uint32_t)U) st.push(out);
        }
    }
}

template <int U, bool W>
__global__ __launch_bounds__(256) void k_cas_sampled_lanes(const uint8_t* __restrict__ staged,
                                                           const uint64_t* __restrict__ soff, uint32_t n,
                                                           uint32_t* __restrict__ rows) {
    constexpr uint32_t K = S_FULL / U;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (uint64_t)n * K) return;
    const uint32_t f = (uint32_t)(g / K), j = (uint32_t)(g - (uint64_t)f * K);
    uint32_t cv[8];
    group_cv<U, W>(cv, staged + soff[f] + (size_t)j * U * CHUNK_LEN, j * U);
    store_cv(rows + ((size_t)j * n + f) * 8, cv);
}

template <int U, bool W>
__global__ __launch_bounds__(256) void k_cas_sampled_merge(const uint8_t* __restrict__ staged,
                                                           const uint64_t* __restrict__ soff,
                                                           const uint32_t* __restrict__ idx, uint32_t n,
                                                           const uint32_t* __restrict__ rows, uint32_t* __restrict__ out) {
    constexpr uint32_t K = S_FULL / U;
    constexpr int D = ilog2(K + 1);  // after node k the stack holds popcount(k + 1) subtrees
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    CvStack<D> st;
    uint32_t cur[8], nxt[8];
    load_cv(nxt, rows + (size_t)f * 8);
#pragma unroll 1
    for (uint32_t k = 0; k < K; k++) {
#pragma unroll
        for (int i = 0; i < 8; i++) cur[i] = nxt[i];
        if (k + 1 < K) load_cv(nxt, rows + ((size_t)(k + 1) * n + f) * 8);  // in flight during the merges
#pragma unroll 1
        for (uint32_t t = k + 1; (t & 1u) == 0; t >>= 1) st.template merge_top<W>(cur, 0u);
        st.push(cur);
    }
    // the tail chunk is the rightmost node; the stack's subtrees fold onto it, ROOT last
    chunk_cv<W>(cur, staged + soff[f] + (size_t)S_FULL * CHUNK_LEN, SD_SAMPLED_MSG_LEN - S_FULL * CHUNK_LEN, S_FULL,
             false);
    constexpr int P = __builtin_popcount(K);  // subtrees on the stack after K nodes
#pragma unroll 1
    for (int d = 0; d < P; d++) st.template merge_top<W>(cur, d + 1 == P ? ROOT : 0u);
    store_cv(out + (size_t)idx[f] * 8, cur);
}

// Small batches (latency): the kernels above trade per-file latency for throughput -- one
// lane walks 8 chunks (135 dependent compressions) and the merge adds 8 more, fine when
// tens of thousands of files fill the chip, but a watcher event or a 100-file identifier
// step then waits for that whole chain.  k_cas_sampled_wave: one 64-lane wave per file,
// one full chunk per lane (lanes 0..55; the next line pair in flight while the current one
// is compressed), lane 56 the 8-byte tail chunk, then the 57 chunk CVs merged level-wise
// in LDS (6 levels): 16 + 6 dependent compressions per file.
// Full 1 KiB non-root chunk, the next line pair in flight while the current one is
// compressed: latency kernels (one chunk per lane, few waves) that cannot hide the load
// of each line pair behind other waves.
template <bool W, bool SDWA16 = rotr16_sdwa(W)>
__device__ __forceinline__ void full_chunk_cv_prefetch(uint32_t (&cv)[8], const uint8_t* __restrict__ q,
                                                       uint32_t counter) {
    set_iv(cv);
    uint32_t ma[16], mb[16], na[16], nb[16];
    load_block(ma, q);
    load_block(mb, q + 64);
#pragma unroll
    for (uint32_t b = 0; b < 16; b += 2) {
        if (b + 2 < 16) {
            load_block(na, q + 64u * (b + 2));
            load_block(nb, q + 64u * (b + 3));
        }
        compress<W, SDWA16>(cv, ma, counter, 0u, BLOCK_LEN, b == 0 ? CHUNK_START : 0u);
        compress<W, SDWA16>(cv, mb, counter, 0u, BLOCK_LEN, b + 1 == 15 ? CHUNK_END : 0u);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            ma[i] = na[i];
            mb[i] = nb[i];
        }
    }
}

// With or without the windows this kernel keeps rotr16 as the SDWA pair: its prefetching chunk loop
// is unrolled whole, and with xor + alignbit under the windows the compiler lets it grow from 91 to
// 179 VGPRs (2 waves/SIMD), or spills when held to 5 waves (profiles/g_rotr16/resource_usage.md).
template <bool W>
__global__ __launch_bounds__(64) void k_cas_sampled_wave(const uint8_t* __restrict__ staged,
                                                         const uint64_t* __restrict__ soff,
                                                         const uint32_t* __restrict__ idx, uint32_t n,
                                                         uint32_t* __restrict__ out) {
    constexpr bool S16 = rotr16_sdwa(false);
    __shared__ __attribute__((aligned(16))) uint32_t lds[64][8];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    const uint8_t* msg = staged + soff[f];
    uint32_t cv[8];
    if (t < (uint32_t)S_FULL) {
        full_chunk_cv_prefetch<W, S16>(cv, msg + (size_t)t * CHUNK_LEN, t);
        store_cv(lds[t], cv);
    } else if (t == (uint32_t)S_FULL) {
        chunk_cv<W, S16>(cv, msg + (size_t)S_FULL * CHUNK_LEN, SD_SAMPLED_MSG_LEN - S_FULL * CHUNK_LEN, S_FULL, false);
        store_cv(lds[t], cv);
    }
    __syncthreads();
    lds_reduce<W, S16>(lds, S_FULL + 1, true);
    if (t < 8) out[(size_t)idx[f] * 8 + t] = lds[0][t];
}

// Small batches of whole-kind messages (latency; see k_cas_sampled_wave): one 128-lane
// workgroup per message of <= 101 chunks (SD_WHOLE_ITEMS_MAX), lane c hashes chunk c, the
// chunk CVs merge level-wise in LDS: at most 16 + 7 dependent compressions, against the
// work-list path's 33 (a chunk pair per lane) + two merge launches.  Row = (u64 message
// offset, message length, output row).
__global__ __launch_bounds__(128) void k_whole_wave(const uint8_t* __restrict__ staged, const uint4* __restrict__ rows,
                                                    uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[128][8];
    const uint4 r = rows[blockIdx.x];
    const uint32_t t = threadIdx.x, L = r.z;
    const uint8_t* msg = staged + ((uint64_t)r.x | ((uint64_t)r.y << 32));
    const uint32_t C = L == 0 ? 1u : (L + CHUNK_LEN - 1) / CHUNK_LEN;
    if (t < C) {
        const uint32_t len = L == 0 ? 0u : (L - t * CHUNK_LEN < CHUNK_LEN ? L - t * CHUNK_LEN : CHUNK_LEN);
        uint32_t cv[8];
        if (len == CHUNK_LEN && C > 1) full_chunk_cv_prefetch<false>(cv, msg + (size_t)t * CHUNK_LEN, t);
        else chunk_cv<false>(cv, msg + (size_t)t * CHUNK_LEN, len, t, C == 1);
        store_cv(lds[t], cv);
    }
    __syncthreads();
    lds_reduce<false>(lds, C, C > 1);  // one chunk: its last block already carried ROOT
    if (t < 8) out[(size_t)r.w * 8 + t] = lds[0][t];
}

// ------------------------------------------------------------------ whole-file cas
// Work items built on the host (sd_cas_api.cpp, plan_whole_items), 16 bytes each:
//   full-pair item  (u64 pair offset, CV slot, first chunk index): an aligned chunk pair
//                   lying wholly inside a message of >= 3 chunks -- 32 full blocks and one
//                   parent, never ROOT; the sampled kernel's branch-free line-pair loop.
//   tail item       (u64 offset, CV slot or file, glen | c0 << 12 | root << 31): a
//                   message's partial last pair, or the whole message when it has <= 2
//                   chunks (then ROOT).  Sorted on the host by compression count, so the
//                   lanes of a wave have equal trip counts.
// Workgroups [0, wf) take full-pair items, the rest tail items (a workgroup-uniform
// branch); the tail path hashes its chunks one after the other without the second message
// buffer, so the kernel keeps the full path's register budget, and its latency-bound
// lanes run while the last full-pair waves drain.
template <bool W>
__global__ __launch_bounds__(256) void k_whole_items(const uint8_t* __restrict__ staged,
                                                     const uint4* __restrict__ full, uint32_t n_full, uint32_t wf,
                                                     const uint4* __restrict__ tail, uint32_t n_tail,
                                                     uint32_t* __restrict__ cvbuf, uint32_t* __restrict__ out) {
    if (blockIdx.x < wf) {
        const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
        if (g >= n_full) return;
        const uint4 it = full[g];
        const uint64_t off = (uint64_t)it.x | ((uint64_t)it.y << 32);
        uint32_t cv[8];
        full_chunks_cv<2, W>(cv, staged + off, it.w);
        store_cv(cvbuf + (size_t)it.z * 8, cv);
        return;
    }
    const uint32_t g = (blockIdx.x - wf) * blockDim.x + threadIdx.x;
    if (g >= n_tail) return;
    const uint4 it = tail[g];
    const uint8_t* p = staged + ((uint64_t)it.x | ((uint64_t)it.y << 32));
    const uint32_t glen = it.w & 0xFFFu, c0 = (it.w >> 12) & 0x7FFFFu;
    const bool root = (it.w >> 31) != 0u;
    uint32_t cv[8];
    if (glen <= CHUNK_LEN) {
        chunk_cv<W>(cv, p, glen, c0, root);
    } else {
        uint32_t l[8], r[8];
        chunk_cv<W>(l, p, CHUNK_LEN, c0, false);
        // Hold l here (the empty asm emits nothing).  With rotr16 in its plain form no op of G is an
        // asm, and the compiler sank the whole last compression of l out of its windows, past r, to
        // parent() where l is first read.
        if constexpr (W) {
#pragma unroll
            for (int k = 0; k < 8; k++) asm volatile("" : "+v"(l[k]));
        }
        chunk_cv<W>(r, p + CHUNK_LEN, glen - CHUNK_LEN, c0 + 1, false);
        parent<W>(cv, l, r, root ? ROOT : 0u);
    }
    store_cv((root ? out : cvbuf) + (size_t)it.z * 8, cv);
}

// Item = (first node slot in src, m | root << 31, dst slot or file): merges nodes
// src[first .. first + m), m in 1..8, an aligned group of one file's node list (every node
// but the last a full subtree of one size), into one CV, level-wise (below).  ROOT on the
// final parent when the group is the whole file.  Two passes (<= 8 pair nodes, then <= 8 of
// those) cover messages of up to 128 chunks.  (Round 5: every node loaded up front, 4 %
// faster than merging each into a CV stack as it arrived, profiles/r5/r5w_merge8_trace.md;
// the stack version is in e9a97a5.)
template <bool W>
__global__ __launch_bounds__(256) void k_whole_merge8(const uint4* __restrict__ items, uint32_t n,
                                                      const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                      uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const uint4 it = items[g];
    const uint32_t m = it.y & 0xFu;
    const bool root = (it.y >> 31) != 0u;
    // All m node CVs are loaded at once (they were written by another XCD's workgroups, so
    // each load is a trip past this XCD's L2: one round trip per lane instead of m), then
    // merged level-wise with static register indices -- pairs (2k, 2k+1), the odd node
    // carried up -- the BLAKE3 tree of an aligned group.  The lanes of a wave hold items
    // sorted by node count, so the guarded parents rarely diverge.
    uint32_t nd[8][8];
#pragma unroll
    for (int k = 0; k < 8; k++)
        if ((uint32_t)k < m) load_cv(nd[k], src + (size_t)(it.x + k) * 8);
    uint32_t cnt = m;
#pragma unroll
    for (int lvl = 0; lvl < 3; lvl++) {
        const uint32_t flags = (root && cnt == 2u) ? ROOT : 0u;
#pragma unroll
        for (int k = 0; k < 4 >> lvl; k++) {
            if ((uint32_t)(2 * k + 1) < cnt) {
                uint32_t r[8];
                parent<W>(r, nd[2 * k], nd[2 * k + 1], flags);
#pragma unroll
                for (int i = 0; i < 8; i++) nd[k][i] = r[i];
            } else if ((uint32_t)(2 * k) < cnt) {
#pragma unroll
                for (int i = 0; i < 8; i++) nd[k][i] = nd[2 * k][i];
            }
        }
        cnt = (cnt + 1u) >> 1;
    }
    store_cv((root ? out : dst) + (size_t)it.z * 8, nd[0]);
}

// 32-byte hash rows src[i] -> out[idx[i]] (whole-file cas messages hashed by the checksum
// kernels land in their batch's output order)
__global__ __launch_bounds__(256) void k_scatter_hash(const uint32_t* __restrict__ src, const uint32_t* __restrict__ idx,
                                                      uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n * 8u) return;
    out[(size_t)idx[g >> 3] * 8 + (g & 7u)] = src[g];
}

// ------------------------------------------------------------------------ checksums
// Leaf: 1 MiB blocks = 1024 chunks of one message, CK_WG_BLOCKS (2) blocks per workgroup of
// 256 lanes each.  Lane l of a block hashes its chunks [4l, 4l+4) one after the other
// (line-pair loads) and merges them in-lane with the CV stack; then the lane CVs of each
// block merge level-wise in LDS with the blocks' trees packed together: at tree level L the
// parents of both blocks sit in the lowest lanes, so the workgroup's waves run partly masked
// only at the top levels, once per two blocks (round 5: with one block per workgroup its
// 8-level tree left 321 lane-compressions of every 17 728 masked, 1.8 %; two blocks leave
// 129 per block -- 0.3-1.2 % faster, profiles/r5/r5zk_ck_leaf_ab/; 16- or 8-chunk lanes
// with 4 or 2 blocks per 256-lane workgroup lost it again to 4x / 2x longer workgroups, and
// 4 blocks of 256 lanes per workgroup to occupancy, r5zk1 and r5zk).  Block number =
// wg_map[i].y + blk_base for entry i = CK_WG_BLOCKS x workgroup + (lane / 256); `shift` is
// subtracted from the message's byte offset (a streamed window holds message bytes
// [shift, shift + window)).
#ifndef SD_CK_LANE_CHUNKS
#define SD_CK_LANE_CHUNKS 4
#endif
#ifndef SD_CK_WG_BLOCKS
#define SD_CK_WG_BLOCKS 2
#endif
constexpr uint32_t CK_BLOCK_CHUNKS = 1024;
constexpr uint32_t CK_LANE_CHUNKS = SD_CK_LANE_CHUNKS;
constexpr uint32_t CK_BLOCK_LANES = CK_BLOCK_CHUNKS / CK_LANE_CHUNKS;
constexpr uint32_t CK_WG_BLOCKS = SD_CK_WG_BLOCKS;
constexpr uint32_t CK_WG_THREADS = CK_BLOCK_LANES * CK_WG_BLOCKS;
constexpr uint32_t CK_TREE_LEVELS = ilog2(CK_BLOCK_LANES);
static_assert((CK_LANE_CHUNKS & (CK_LANE_CHUNKS - 1)) == 0 && CK_LANE_CHUNKS >= 2 && CK_LANE_CHUNKS <= 16, "lane chunks");
static_assert(CK_WG_THREADS >= 64 && CK_WG_THREADS <= 1024 && CK_WG_THREADS % 64 == 0, "workgroup size");

// The leaf's body, shared by k_ck_leaf and k_ck_leaf_tree.
// T (k_ck_leaf_tree, the checksum tree's level at 2^k-byte granularity, 17 <= k <= 20): the
// LDS tree after iteration L holds the CVs of aligned 2^(13+L)-byte groups, so after iteration
// node_level = k - 13 the first ceil(block bytes / 2^k) slots of a leaf block are its nodes; the
// lanes that just computed them also store them to nodes[node_base[file] + blk 2^(20-k) + j].
// A file of one node has its root there (ROOT went on in the lane or at the nb == 2 merge below
// that level and is only carried since); a longer file's nodes are plain CVs.
template <bool W, bool T>
__device__ __forceinline__ void ck_leaf_body(
    const uint8_t* __restrict__ data, uint64_t shift, uint32_t blk_base, const ck_file* __restrict__ files,
    const uint2* __restrict__ wg_map, uint32_t n_blocks, uint32_t* __restrict__ cvbuf, uint32_t* __restrict__ out,
    const uint64_t* __restrict__ node_base, uint32_t node_level, uint32_t* __restrict__ nodes) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[CK_WG_THREADS][8];
    __shared__ uint32_t s_lanes[CK_WG_BLOCKS], s_root[CK_WG_BLOCKS];
    __shared__ uint64_t s_dst[CK_WG_BLOCKS];  // output row: file (root) or CV slot, | 1 << 63 for out
    __shared__ uint64_t s_node[CK_WG_BLOCKS];  // T: the block's first node
    const uint32_t t = threadIdx.x, wv = t / CK_BLOCK_LANES, lane = t % CK_BLOCK_LANES;
    const uint32_t bi = blockIdx.x * CK_WG_BLOCKS + wv;  // this lane's block entry
    uint32_t lanes_b = 0, root_b = 0;
    uint64_t dst_b = 0, node_b = 0;
    if (bi < n_blocks) {
        const uint2 wm = wg_map[bi];  // (file, block)
        const uint32_t blk = wm.y + blk_base;
        const ck_file fi = files[wm.x];
        if constexpr (T) node_b = node_base[wm.x] + ((uint64_t)blk << (CK_TREE_LEVELS - 1 - node_level));
        const uint64_t nchunks = fi.len == 0 ? 1 : (fi.len + CHUNK_LEN - 1) / CHUNK_LEN;
        const uint64_t blk0 = (uint64_t)blk * CK_BLOCK_CHUNKS;
        const uint32_t blk_chunks = (uint32_t)(nchunks - blk0 < CK_BLOCK_CHUNKS ? nchunks - blk0 : CK_BLOCK_CHUNKS);
        const bool file_is_block = nchunks <= CK_BLOCK_CHUNKS;
        const bool file_is_lane = nchunks <= CK_LANE_CHUNKS;  // the whole message inside lane 0
        lanes_b = (blk_chunks + CK_LANE_CHUNKS - 1) / CK_LANE_CHUNKS;
        root_b = file_is_block && !file_is_lane;
        dst_b = file_is_block ? ((uint64_t)wm.x | (1ull << 63)) : fi.cv_base + blk;
        const uint32_t c0 = lane * CK_LANE_CHUNKS;
        if (c0 < blk_chunks) {
            const uint32_t nch = blk_chunks - c0 < CK_LANE_CHUNKS ? blk_chunks - c0 : CK_LANE_CHUNKS;
            const uint8_t* p = data + (fi.offset - shift);
            CvStack<ilog2(CK_LANE_CHUNKS)> st;  // after chunk j it holds popcount(j + 1) subtrees
            uint32_t cv[8];
#pragma unroll 1
            for (uint32_t j = 0; j < nch; j++) {
                // 64 bits: the chunk counter passes 2^32 at 4 TiB of a message, and both words reach compress
                // (tests/test_gpu_high_counter.py::test_split_leaves_past_2_32 fails on a narrower one)
                const uint64_t ci = blk0 + c0 + j;
                const uint64_t rem = fi.len - ci * CHUNK_LEN;
                const uint32_t len = fi.len == 0 ? 0u : (rem < CHUNK_LEN ? (uint32_t)rem : CHUNK_LEN);
                if (len == CHUNK_LEN && nchunks > 1) full_chunk_cv_lp<W>(cv, p + ci * CHUNK_LEN, ci);
                else chunk_cv<W>(cv, p + ci * CHUNK_LEN, len, ci, nchunks == 1);
                if (j + 1 < nch) {  // an aligned group that ends here merges, then waits on the stack
#pragma unroll 1
                    for (uint32_t g = j + 1; (g & 1u) == 0; g >>= 1) st.template merge_top<W>(cv, 0u);
                    st.push(cv);
                } else {  // the lane's last chunk: its aligned merges and the fold, one run of
                          // popcount(nch - 1) merges; ROOT on the last when the file is this lane
                    const uint32_t ops = (uint32_t)__builtin_popcount(nch - 1);
#pragma unroll 1
                    for (uint32_t k = ops; k > 0; k--) st.template merge_top<W>(cv, (file_is_lane && k == 1) ? ROOT : 0u);
                }
            }
            store_cv(lds[t], cv);
        }
    }
    if (lane == 0) {
        s_lanes[wv] = lanes_b;
        s_root[wv] = root_b;
        s_dst[wv] = dst_b;
        if constexpr (T) s_node[wv] = node_b;
    }
    __syncthreads();
    // the blocks' trees, level-wise with the odd node carried up (CK_BLOCK_LANES -> 1); block
    // b's level-L nodes at lds[CK_BLOCK_LANES b .. + n_b(L))
#pragma unroll 1
    for (uint32_t L = 0; L < CK_TREE_LEVELS; L++) {
        const uint32_t P = (CK_BLOCK_LANES / 2) >> L;  // parent slots per block at this level
        uint32_t res[8];
        bool have = false;
        uint32_t to = 0;
        if (t < CK_WG_BLOCKS * P) {
            const uint32_t b = t / P, j = t - b * P;
            uint32_t nb = s_lanes[b];
            for (uint32_t l = 0; l < L; l++) nb = (nb + 1) >> 1;
            if (2 * j + 1 < nb) {
                uint32_t l8[8], r8[8];
                load_cv(l8, lds[CK_BLOCK_LANES * b + 2 * j]);
                load_cv(r8, lds[CK_BLOCK_LANES * b + 2 * j + 1]);
                parent<W>(res, l8, r8, (s_root[b] && nb == 2) ? ROOT : 0u);
                have = true;
            } else if (2 * j + 1 == nb) {  // the odd last node
                load_cv(res, lds[CK_BLOCK_LANES * b + 2 * j]);
                have = true;
            }
            to = CK_BLOCK_LANES * b + j;
        }
        __syncthreads();
        if (have) store_cv(lds[to], res);
        if constexpr (T) {
            if (have && L == node_level) {  // to = CK_BLOCK_LANES b + j: node j of leaf block b
                const uint32_t b = to / CK_BLOCK_LANES;
                store_cv(nodes + (s_node[b] + (to - CK_BLOCK_LANES * b)) * 8, res);
            }
        }
        __syncthreads();
    }
    if (t < 8 * CK_WG_BLOCKS) {
        const uint32_t b = t >> 3, w = t & 7u;
        if (s_lanes[b]) {
            const uint64_t d = s_dst[b];
            if (d >> 63) out[(d & ~(1ull << 63)) * 8 + w] = lds[CK_BLOCK_LANES * b][w];
            else cvbuf[d * 8 + w] = lds[CK_BLOCK_LANES * b][w];
        }
    }
}

template <bool W>
__global__ __launch_bounds__(CK_WG_THREADS) void k_ck_leaf(
    const uint8_t* __restrict__ data, uint64_t shift, uint32_t blk_base, const ck_file* __restrict__ files,
    const uint2* __restrict__ wg_map, uint32_t n_blocks, uint32_t* __restrict__ cvbuf, uint32_t* __restrict__ out) {
    ck_leaf_body<W, false>(data, shift, blk_base, files, wg_map, n_blocks, cvbuf, out, nullptr, 0, nullptr);
}

// the same pass that also leaves the level at 2^(13 + node_level)-byte granularity in `nodes`
// (16-byte aligned, as cvbuf)
template <bool W>
__global__ __launch_bounds__(CK_WG_THREADS) void k_ck_leaf_tree(
    const uint8_t* __restrict__ data, const ck_file* __restrict__ files, const uint2* __restrict__ wg_map,
    uint32_t n_blocks, uint32_t* __restrict__ cvbuf, uint32_t* __restrict__ out,
    const uint64_t* __restrict__ node_base, uint32_t node_level, uint32_t* __restrict__ nodes) {
    ck_leaf_body<W, true>(data, 0, 0, files, wg_map, n_blocks, cvbuf, out, node_base, node_level, nodes);
}

// Listed blocks (include/sd_cas.h; checksum_tree.hip): the node of item bi = ck_block_item
// {src, chunk0, len, root, dst} -- at most 2^k bytes (17 <= k <= 20) that sit anywhere in `data`,
// chunk counters from chunk0 (64 bits), ROOT only when the item's file has one node.  No file
// table and no block map: the item is all a workgroup reads.  An item takes 2^il_log2 = 2^(k-12)
// lanes of CK_LANE_CHUNKS chunks, the leaf's in-lane path, and the workgroup's CK_WG_THREADS lanes
// hold 512 >> il_log2 items (16 at k = 17 down to 2 at k = 20, the leaf's own shape) whose LDS
// trees of il_log2 levels are packed into the lowest lanes level by level, as the leaf packs its
// two.  ROOT, when the item asks: inside the lane for <= CK_LANE_CHUNKS chunks, else on the
// item's last parent; an item of a longer file never has it (a 1-byte trailing block, a one-chunk
// block at a counter > 0 are plain CVs).  The lane that holds an item's top after the last level
// stores it from registers (two 16-byte stores): to row bi of `nodes` (list order), or, `scatter`,
// to row item.dst (the level layout).
template <bool W>
__global__ __launch_bounds__(CK_WG_THREADS) void k_ck_blocks(const uint8_t* __restrict__ data,
                                                             const ck_block_item* __restrict__ items,
                                                             uint32_t n_items, uint32_t il_log2, uint32_t scatter,
                                                             uint32_t* __restrict__ nodes) {
    constexpr uint32_t MAX_ITEMS = CK_WG_THREADS >> 5;  // il_log2 >= 5
    __shared__ __attribute__((aligned(16))) uint32_t lds[CK_WG_THREADS][8];
    __shared__ uint32_t s_lanes[MAX_ITEMS], s_root[MAX_ITEMS];
    __shared__ uint64_t s_dst[MAX_ITEMS];
    const uint32_t t = threadIdx.x, wi = t >> il_log2, lane = t & ((1u << il_log2) - 1);
    const uint32_t per_wg = CK_WG_THREADS >> il_log2;
    const uint32_t bi = blockIdx.x * per_wg + wi;  // this lane's item
    uint32_t lanes_b = 0, root_b = 0;
    uint64_t dst_b = 0;
    if (bi < n_items) {
        const uint4* q = reinterpret_cast<const uint4*>(items + bi);
        const uint4 a = q[0], b = q[1];
        const uint64_t src = (uint64_t)a.x | ((uint64_t)a.y << 32), chunk0 = (uint64_t)a.z | ((uint64_t)a.w << 32);
        const uint32_t ilen = b.x;
        const bool root = b.y != 0u;
        dst_b = scatter ? ((uint64_t)b.z | ((uint64_t)b.w << 32)) : (uint64_t)bi;
        const uint32_t nchunks = ilen == 0 ? 1u : (ilen + CHUNK_LEN - 1) / CHUNK_LEN;
        const bool item_is_lane = nchunks <= CK_LANE_CHUNKS;  // the whole item inside lane 0
        lanes_b = (nchunks + CK_LANE_CHUNKS - 1) / CK_LANE_CHUNKS;
        root_b = root && !item_is_lane;
        const uint32_t c0 = lane * CK_LANE_CHUNKS;
        if (c0 < nchunks) {
            const uint32_t nch = nchunks - c0 < CK_LANE_CHUNKS ? nchunks - c0 : CK_LANE_CHUNKS;
            const uint8_t* p = data + src;
            CvStack<ilog2(CK_LANE_CHUNKS)> st;  // after chunk j it holds popcount(j + 1) subtrees
            uint32_t cv[8];
#pragma unroll 1
            for (uint32_t j = 0; j < nch; j++) {
                const uint32_t ci = c0 + j;  // the chunk inside the item; its counter is 64 bits wide
                const uint32_t rem = ilen - ci * CHUNK_LEN;
                const uint32_t len = ilen == 0 ? 0u : (rem < CHUNK_LEN ? rem : CHUNK_LEN);
                const bool root_chunk = root && nchunks == 1;
                if (len == CHUNK_LEN && !root_chunk) full_chunk_cv_lp<W>(cv, p + (size_t)ci * CHUNK_LEN, chunk0 + ci);
                else chunk_cv<W>(cv, p + (size_t)ci * CHUNK_LEN, len, chunk0 + ci, root_chunk);
                if (j + 1 < nch) {  // an aligned group that ends here merges, then waits on the stack
#pragma unroll 1
                    for (uint32_t g = j + 1; (g & 1u) == 0; g >>= 1) st.template merge_top<W>(cv, 0u);
                    st.push(cv);
                } else {  // the lane's last chunk: ROOT on the last merge when the file is this lane
                    const uint32_t ops = (uint32_t)__builtin_popcount(nch - 1);
#pragma unroll 1
                    for (uint32_t k = ops; k > 0; k--)
                        st.template merge_top<W>(cv, (root && item_is_lane && k == 1) ? ROOT : 0u);
                }
            }
            store_cv(lds[t], cv);
        }
    }
    if (lane == 0) {
        s_lanes[wi] = lanes_b;
        s_root[wi] = root_b;
        s_dst[wi] = dst_b;
    }
    __syncthreads();
    // the items' trees, level-wise with the odd node carried up (2^il_log2 -> 1); item b's level-L
    // nodes at lds[(b << il_log2) .. + n_b(L)); the last level's result leaves from registers
#pragma unroll 1
    for (uint32_t L = 0; L < il_log2; L++) {
        const uint32_t p_log2 = il_log2 - 1 - L;  // parent slots per item at this level, log2
        uint32_t res[8];
        bool have = false;
        uint32_t to = 0, b = 0;
        if (t < (per_wg << p_log2)) {
            b = t >> p_log2;
            const uint32_t j = t & ((1u << p_log2) - 1);
            uint32_t nb = s_lanes[b];
            for (uint32_t l = 0; l < L; l++) nb = (nb + 1) >> 1;
            const uint32_t at = (b << il_log2) + 2 * j;
            if (2 * j + 1 < nb) {
                uint32_t l8[8], r8[8];
                load_cv(l8, lds[at]);
                load_cv(r8, lds[at + 1]);
                parent<W>(res, l8, r8, (s_root[b] && nb == 2) ? ROOT : 0u);
                have = true;
            } else if (2 * j + 1 == nb) {  // the odd last node
                load_cv(res, lds[at]);
                have = true;
            }
            to = (b << il_log2) + j;
        }
        if (L + 1 == il_log2) {  // one slot per item: its node
            if (have) store_cv(nodes + s_dst[b] * 8, res);
            break;
        }
        __syncthreads();
        if (have) store_cv(lds[to], res);
        __syncthreads();
    }
}

// Reduce: workgroup = up to 256 consecutive CVs of one message's level; writes one CV to
// the next level, or the root hash when the level fits one group.
__global__ __launch_bounds__(256) void k_ck_reduce(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                   const ck_reduce_wg* __restrict__ wgs, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[256][8];
    const ck_reduce_wg w = wgs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    if (t < w.count) {
        uint32_t cv[8];
        load_cv(cv, src + (w.src_base + t) * 8);
        store_cv(lds[t], cv);
    }
    __syncthreads();
    lds_reduce<false>(lds, w.count, w.is_root != 0);
    if (t < 8) {
        if (w.is_root) out[(size_t)w.file * 8 + t] = lds[0][t];
        else dst[w.dst_index * 8 + t] = lds[0][t];
    }
}

// --------------------------------------------------------------------- launchers
namespace sdk {

// Priority windows (blake3_device.h, SD_G_PRIO) for a launch of `waves` waves?  They steer the
// arbiter between the waves of one SIMD, so they need more waves than the device has SIMDs;
// below that a wave only pays for the s_setprio (profiles/g_prio/small_batch.md).  The count is
// the launch's own: what else runs on the device at the time is not considered.  k_whole_wave
// (<= 512 workgroups of two waves) and k_ck_reduce (an LDS tree of a few waves) never have them.
static bool g_windows(uint64_t waves) {
    static const uint64_t simds = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return (uint64_t)cus * 4;
    }();
    return SD_G_PRIO != 0 && waves > simds;
}
// K<W> on `wgs` workgroups of `threads` lanes, W = g_windows(the launch's waves)
#define SD_LAUNCH_W(K_TRUE, K_FALSE, wgs, threads, s, ...)                                           \
    do {                                                                                             \
        if (g_windows((uint64_t)(wgs) * ((threads) / 64)))                                           \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(K_TRUE), dim3(wgs), dim3(threads), 0, s, __VA_ARGS__);  \
        else                                                                                         \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(K_FALSE), dim3(wgs), dim3(threads), 0, s, __VA_ARGS__); \
    } while (0)

uint64_t cas_sampled_rows_bytes(uint32_t n) { return (uint64_t)n * S_K * 32; }

// rows >= cas_sampled_rows_bytes(n)
hipError_t launch_cas_sampled(const uint8_t* staged, const uint64_t* soff, const uint32_t* idx, uint32_t n,
                              uint32_t* rows, uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t lanes_wg = (uint32_t)(((uint64_t)n * S_K + 255) / 256), merge_wg = (n + 255) / 256;
    SD_LAUNCH_W((k_cas_sampled_lanes<S_U, true>), (k_cas_sampled_lanes<S_U, false>), lanes_wg, 256, s, staged, soff, n, rows);
    SD_LAUNCH_W((k_cas_sampled_merge<S_U, true>), (k_cas_sampled_merge<S_U, false>), merge_wg, 256, s, staged, soff, idx, n,
                rows, out);
    return hipGetLastError();
}

hipError_t launch_whole_wave(const uint8_t* staged, const uint4* rows, uint32_t n, uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_whole_wave, dim3(n), dim3(128), 0, s, staged, rows, out);
    return hipGetLastError();
}

hipError_t launch_cas_sampled_wave(const uint8_t* staged, const uint64_t* soff, const uint32_t* idx, uint32_t n,
                                   uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    SD_LAUNCH_W(k_cas_sampled_wave<true>, k_cas_sampled_wave<false>, n, 64, s, staged, soff, idx, n, out);
    return hipGetLastError();
}

hipError_t launch_whole_items(const uint8_t* staged, const uint4* full, uint32_t n_full, const uint4* tail,
                              uint32_t n_tail, const uint4* merge_a, uint32_t n_a, const uint4* merge_b, uint32_t n_b,
                              uint32_t* cvbuf, uint32_t* cv2, uint32_t* out, hipStream_t s) {
    const uint32_t wf = (n_full + 255) / 256, wt = (n_tail + 255) / 256;
    if (wf + wt)
        SD_LAUNCH_W(k_whole_items<true>, k_whole_items<false>, wf + wt, 256, s, staged, full, n_full, wf, tail, n_tail,
                    cvbuf, out);
    if (n_a)
        SD_LAUNCH_W(k_whole_merge8<true>, k_whole_merge8<false>, (n_a + 255) / 256, 256, s, merge_a, n_a,
                    (const uint32_t*)cvbuf, cv2, out);
    if (n_b)
        SD_LAUNCH_W(k_whole_merge8<true>, k_whole_merge8<false>, (n_b + 255) / 256, 256, s, merge_b, n_b,
                    (const uint32_t*)cv2, (uint32_t*)nullptr, out);
    return hipGetLastError();
}

hipError_t launch_scatter_hash(const uint32_t* src, const uint32_t* idx, uint32_t n, uint32_t* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_hash, dim3((n * 8 + 255) / 256), dim3(256), 0, s, src, idx, n, out);
    return hipGetLastError();
}

hipError_t launch_ck_leaf(const uint8_t* data, uint64_t shift, uint32_t blk_base, const ck_file* files,
                          const uint2* wg_map, uint32_t n_wg, uint32_t* cvbuf, uint32_t* out, hipStream_t s) {
    if (n_wg == 0) return hipSuccess;
    SD_LAUNCH_W(k_ck_leaf<true>, k_ck_leaf<false>, (n_wg + CK_WG_BLOCKS - 1) / CK_WG_BLOCKS, CK_WG_THREADS, s, data, shift,
                blk_base, files, wg_map, n_wg, cvbuf, out);
    return hipGetLastError();
}

// block_log2 in [SD_TREE_BLOCK_LOG2_MIN, SD_TREE_BLOCK_LOG2_MAX] (the caller checked)
hipError_t launch_ck_leaf_tree(const uint8_t* data, const ck_file* files, const uint2* wg_map, uint32_t n_wg,
                               uint32_t* cvbuf, uint32_t* out, const uint64_t* node_base, uint32_t block_log2,
                               uint32_t* nodes, hipStream_t s) {
    static_assert(CK_BLOCK_CHUNKS * CHUNK_LEN == (1u << SD_TREE_BLOCK_LOG2_MAX), "the leaf block is the largest tree block");
    if (n_wg == 0) return hipSuccess;
    const uint32_t lane_log2 = SD_TREE_BLOCK_LOG2_MAX - CK_TREE_LEVELS;  // bytes of a lane, log2
    if (block_log2 <= lane_log2 || block_log2 > SD_TREE_BLOCK_LOG2_MAX) return hipErrorInvalidValue;
    SD_LAUNCH_W(k_ck_leaf_tree<true>, k_ck_leaf_tree<false>, (n_wg + CK_WG_BLOCKS - 1) / CK_WG_BLOCKS, CK_WG_THREADS, s,
                data, files, wg_map, n_wg, cvbuf, out, node_base, block_log2 - lane_log2 - 1, nodes);
    return hipGetLastError();
}

// block_log2 in [SD_TREE_BLOCK_LOG2_MIN, SD_TREE_BLOCK_LOG2_MAX] (the caller checked)
hipError_t launch_ck_blocks(const uint8_t* data, const ck_block_item* items, uint32_t n_items, uint32_t block_log2,
                            bool scatter, uint32_t* nodes, hipStream_t s) {
    if (n_items == 0) return hipSuccess;
    const uint32_t lane_log2 = SD_TREE_BLOCK_LOG2_MAX - CK_TREE_LEVELS;  // bytes of a lane, log2
    if (block_log2 < lane_log2 + 5 || block_log2 > SD_TREE_BLOCK_LOG2_MAX) return hipErrorInvalidValue;
    const uint32_t il_log2 = block_log2 - lane_log2, per_wg = CK_WG_THREADS >> il_log2;
    if (per_wg == 0) return hipErrorInvalidValue;
    SD_LAUNCH_W(k_ck_blocks<true>, k_ck_blocks<false>, (n_items + per_wg - 1) / per_wg, CK_WG_THREADS, s, data, items,
                n_items, il_log2, scatter ? 1u : 0u, nodes);
    return hipGetLastError();
}

hipError_t launch_ck_reduce(const uint32_t* src, uint32_t* dst, const ck_reduce_wg* wgs, uint32_t n_wg,
                            uint32_t* out, hipStream_t s) {
    if (n_wg == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ck_reduce, dim3(n_wg), dim3(256), 0, s, src, dst, wgs, out);
    return hipGetLastError();
}

#undef SD_LAUNCH_W

}  // namespace sdk
