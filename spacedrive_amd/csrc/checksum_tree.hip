// checksum_tree.hip -- the checksum trees of the C ABI (include/sd_cas.h): every file's BLAKE3
// tree cut at block granularity beside its root, the roots from levels alone, and a verify that
// names the blocks that differ.
//
// Reference: validator_job.rs:138-141 ("we can also compare old and new checksums here"),
// p2p/src/spaceblock/block.rs:6,10 (a block to resend needs a checksum) and block_size.rs:20-23
// (128 KiB blocks); file_checksum is validation/hash.rs:10-24.
//
// The level is what k_ck_leaf's LDS tree holds on its way to the 1 MiB CV
// (k_ck_leaf_tree, cas_kernels.hip), and a level's root is k_ck_reduce run with the level as its
// level 0 (plan_reduce_passes takes any count per file).  Here: the plan, the copy of one-node
// files' roots, and the verify's compare / compact on sliced.h's two skeletons.  The listed blocks
// (sd_checksum_tree_blocks_*) are k_ck_blocks over an item table planned on the host
// (plan_tree_blocks): its nodes in list order (_run, and _verify's scratch, compared and compacted
// by the same two skeletons) or scattered into a level that the same reduce then roots (_update).
// The block proofs (_prove, _verify_proofs) are the only BLAKE3 here, blake3_device.h's parent:
// k_tree_levels stores the interior levels a reduce passes through, k_tree_proof_gather packs the
// siblings, and proof_climb, a predicate of the flag skeleton, climbs a row's node to its root.
// The range proofs (_prove_ranges, _verify_range_proofs) take a run of rows at once:
// k_tree_range_gather packs the run's two flanks, and k_tree_range_climb, the reduce's LDS tree
// with flanks, climbs the run's nodes to the root they claim, which range_differs compares.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "blake3_device.h"
#include "sd_api_impl.h"
#include "sliced.h"

using namespace sliced;
using namespace sdi;

namespace {

// the file of node i: the last f with node_base[f] <= i (node_base ascends strictly, i < node_base[n])
__device__ __forceinline__ uint64_t tree_file_of(const uint64_t* __restrict__ node_base, uint64_t n, uint64_t i) {
    uint64_t lo = 0, hi = n;  // node_base[lo] <= i < node_base[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (node_base[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a file of one node: the node is its root
__global__ __launch_bounds__(256) void k_tree_single_roots(const uint64_t* __restrict__ node_base, uint64_t n,
                                                           const uint32_t* __restrict__ nodes,
                                                           uint32_t* __restrict__ out) {
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < 8 * n; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = g >> 3, b = node_base[i];
        if (node_base[i + 1] - b == 1) out[g] = nodes[8 * b + (g & 7u)];
    }
}

// node i differs from the expected one; its file is marked (the same value from every writer)
struct tree_differs {
    const uint4* __restrict__ got;
    const uint4* __restrict__ want;
    const uint64_t* __restrict__ node_base;
    uint64_t n_files;
    uint8_t* __restrict__ file_bad;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint4 a0 = got[2 * i], a1 = got[2 * i + 1], b0 = want[2 * i], b1 = want[2 * i + 1];
        const bool d = a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y ||
                       a1.z != b1.z || a1.w != b1.w;
        if (d) file_bad[tree_file_of(node_base, n_files, i)] = 1;
        return d;
    }
};

struct tree_file_marked {
    const uint8_t* __restrict__ file_bad;
    __device__ bool operator()(uint64_t i, uint64_t) const { return file_bad[i] != 0; }
};

// one row (file, block) per flagged node, in order
struct tree_rows : from_flags {
    const uint64_t* __restrict__ node_base;
    uint64_t n_files;
    uint64_t* __restrict__ rows;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        const uint64_t f = tree_file_of(node_base, n_files, i);
        rows[2 * slot] = f;
        rows[2 * slot + 1] = i - node_base[f];
    }
};

// the verify's scratch in a pooled slot: the level, the roots the leaf pass writes anyway, the
// flags when the caller wants none, the files' marks, two rows of per-workgroup counts
struct verify_scratch {
    uint8_t *nodes, *roots, *flags, *file_bad;
    uint64_t* counts;
    static size_t bytes(uint64_t total, uint64_t n) {
        return 256 + round256(32 * total) + round256(32 * n) + round256(total) + round256(n) +
               round256(2 * BLOCKS * sizeof(uint64_t));
    }
    verify_scratch(void* base, uint64_t total, uint64_t n) {
        uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 255) & ~uintptr_t(255));
        nodes = p, p += round256(32 * total);
        roots = p, p += round256(32 * n);
        flags = p, p += round256(total);
        file_bad = p, p += round256(n);
        counts = reinterpret_cast<uint64_t*>(p);
    }
};

// listed blocks: row i's node (list order) differs from the expected level's node at the item's
// slot; its file is marked
struct blocks_differ {
    const uint4* __restrict__ got;
    const uint4* __restrict__ want;
    const ck_block_item* __restrict__ items;
    const uint64_t* __restrict__ list;
    uint8_t* __restrict__ file_bad;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t q = items[i].dst;
        const uint4 a0 = got[2 * i], a1 = got[2 * i + 1], b0 = want[2 * q], b1 = want[2 * q + 1];
        const bool d = a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y ||
                       a1.z != b1.z || a1.w != b1.w;
        if (d) file_bad[list[2 * i]] = 1;
        return d;
    }
};

// the list's row (file, block) per flagged row, in list order
struct blocks_rows : from_flags {
    const uint64_t* __restrict__ list;
    uint64_t* __restrict__ rows;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        rows[2 * slot] = list[2 * i];
        rows[2 * slot + 1] = list[2 * i + 1];
    }
};

// the list verify's scratch in a pooled slot: the rows' nodes, the flags when the caller wants
// none, the files' marks, two rows of per-workgroup counts
struct blocks_scratch {
    uint8_t *nodes, *flags, *file_bad;
    uint64_t* counts;
    static size_t bytes(uint64_t m, uint64_t n) {
        return 256 + round256(32 * m) + round256(m) + round256(n) + round256(2 * BLOCKS * sizeof(uint64_t));
    }
    blocks_scratch(void* base, uint64_t m, uint64_t n) {
        uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 255) & ~uintptr_t(255));
        nodes = p, p += round256(32 * m);
        flags = p, p += round256(m);
        file_bad = p, p += round256(n);
        counts = reinterpret_cast<uint64_t*>(p);
    }
};

// ------------------------------------------------------------------------------------ proofs
// Block proofs (include/sd_cas.h): the siblings on a block's way up, and the climb back to the root.
__device__ __forceinline__ void put_cv(uint32_t* dst, const uint32_t (&cv)[8]) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    d[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}
__device__ __forceinline__ void get_cv(uint32_t (&cv)[8], const uint32_t* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    const uint4 a = s[0], b = s[1];
    cv[0] = a.x; cv[1] = a.y; cv[2] = a.z; cv[3] = a.w;
    cv[4] = b.x; cv[5] = b.y; cv[6] = b.z; cv[7] = b.w;
}

// Interior levels: k_ck_reduce's LDS tree over up to 256 consecutive nodes of one file's level, but
// every level it passes through is stored, the carried odd node included: node t of the group's
// level l goes to slot lvl_off[lvl_tab + l - 1] + (first >> l) + t of the scratch.  An aligned group
// of 256 is a complete subtree under the level-wise rule, and in a file's last, short group the
// local carry (2t + 1 >= the group's count) is the file's own, so the slots are the file's levels.
// No ROOT: the levels stored end below the root.  src is the caller's level (pass 0) or the scratch
// itself (a level an earlier pass stored), so neither pointer is __restrict__.
__global__ __launch_bounds__(256) void k_tree_levels(const uint32_t* src, uint32_t* scratch,
                                                     const ck_levels_wg* __restrict__ wgs,
                                                     const uint64_t* __restrict__ lvl_off) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[256][8];
    const ck_levels_wg w = wgs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    if (t < w.count) {
        uint32_t cv[8];
        get_cv(cv, src + (w.src_base + t) * 8);
        put_cv(lds[t], cv);
    }
    __syncthreads();
    uint32_t n = w.count;
    for (uint32_t l = 1; l <= w.levels; l++) {
        const uint32_t P = n >> 1;
        const bool carry = n & 1u;
        uint32_t res[8];
        bool have = false;
        if (t < P) {
            uint32_t a[8], b[8];
            get_cv(a, lds[2 * t]);
            get_cv(b, lds[2 * t + 1]);
            sdb3::parent<false>(res, a, b, 0u);
            have = true;
        } else if (carry && t == P) {
            get_cv(res, lds[n - 1]);
            have = true;
        }
        __syncthreads();
        if (have) {
            put_cv(lds[t], res);
            put_cv(scratch + (lvl_off[w.lvl_tab + l - 1] + (w.first >> l) + t) * 8, res);
        }
        __syncthreads();
        n = P + (carry ? 1u : 0u);
    }
}

// Proof gather: one lane per row copies the siblings that exist, bottom-up, to the row's place
// among the packed proofs: level 0's from the caller's level, the others from the scratch.
__global__ __launch_bounds__(256) void k_tree_proof_gather(const ck_proof_row* __restrict__ prow,
                                                           const uint64_t* __restrict__ list, uint64_t m,
                                                           const uint4* __restrict__ nodes,
                                                           const uint4* __restrict__ scratch,
                                                           const uint64_t* __restrict__ lvl_off,
                                                           uint4* __restrict__ out) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (uint64_t)gridDim.x * blockDim.x) {
        const ck_proof_row w = prow[r];
        uint64_t j = list[2 * r + 1];
        uint4* o = out + 2 * w.pbase;
        uint32_t L = 0;
        for (uint64_t n = w.nb; n > 1; n = (n + 1) >> 1, j >>= 1, L++) {
            const uint64_t s = j ^ 1;
            if (s >= n) continue;  // the node was carried: this level contributes nothing
            const uint4* p = L == 0 ? nodes + 2 * (w.node0 + s) : scratch + 2 * (lvl_off[w.lvl_tab + L - 1] + s);
            o[0] = p[0];
            o[1] = p[1];
            o += 2;
        }
    }
}

// Climb: row i's node (list order) climbed through its proof differs from its file's root; the
// file is marked.  A lane makes as many dependent compressions as its row has entries, so the
// lanes of one wave leave the loop at different depths (nb = 1: none).
struct proof_climb {
    const uint32_t* __restrict__ got;
    const uint32_t* __restrict__ proofs;
    const uint32_t* __restrict__ roots;
    const ck_proof_row* __restrict__ prow;
    const uint64_t* __restrict__ list;
    uint8_t* __restrict__ file_bad;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const ck_proof_row w = prow[i];
        uint64_t j = list[2 * i + 1];
        uint32_t cv[8];
        get_cv(cv, got + 8 * i);
        const uint32_t* e = proofs + 8 * w.pbase;
        for (uint64_t n = w.nb; n > 1; n = (n + 1) >> 1, j >>= 1) {
            if ((j ^ 1) >= n) continue;
            uint32_t s[8], a[8], b[8];
            get_cv(s, e);
            e += 8;
            const bool odd = j & 1;
#pragma unroll
            for (int k = 0; k < 8; k++) a[k] = odd ? s[k] : cv[k], b[k] = odd ? cv[k] : s[k];
            sdb3::parent<false>(cv, a, b, n == 2 ? (uint32_t)sdb3::ROOT : 0u);
        }
        uint32_t want[8];
        get_cv(want, roots + 8 * (uint64_t)w.file);
        bool d = false;
#pragma unroll
        for (int k = 0; k < 8; k++) d |= cv[k] != want[k];
        if (d) file_bad[w.file] = 1;
        return d;
    }
};

// ------------------------------------------------------------------------------------ ranges
// Range proofs (include/sd_cas.h): a run of blocks climbed as a tree reduce, its two flanks the
// only siblings that are not its own.
//
// Range climb: k_ck_reduce's 256-node LDS tree with flanks.  A workgroup holds the nodes of one
// range that fall into one 256-aligned group of the file's level 8p, node i at slot i & 255, so a
// pair of the file is a pair of slots at every level of the pass and a node's sibling is always in
// its group.  Before level l's parents are formed, the range's first group puts the left entry
// beside its first node when that node's index is odd, and its last group the right entry beside
// its last node when that index is even and the file has a node after it (both from the masks the
// host planned; the two may be one workgroup).  A last node still unpaired is the file's own
// carry.  ROOT goes on the last level of the pass that reaches level h.  The group's top goes to
// the scratch the next pass reads, or to top[range].  src is the rows' nodes (pass 0) or the
// scratch itself, so neither pointer is __restrict__.
__global__ __launch_bounds__(256) void k_tree_range_climb(const uint32_t* src, uint32_t* scratch,
                                                          const uint32_t* __restrict__ proofs,
                                                          const ck_range_wg* __restrict__ wgs,
                                                          uint32_t* __restrict__ top) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[256][8];
    const ck_range_wg w = wgs[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const bool first = w.flags & CK_RANGE_FIRST, last = w.flags & CK_RANGE_LAST, fin = w.flags & CK_RANGE_FINAL;
    uint32_t s = w.start, e = w.start + w.count - 1u;  // the present slots of the current level
    uint64_t at = w.pbase;                             // the current level's first entry
    if (t >= s && t <= e) {
        uint32_t cv[8];
        get_cv(cv, src + (w.src_base + (t - s)) * 8);
        put_cv(lds[t], cv);
    }
    // level l's flanks into the slots beside [s, e]: lanes that hold no node of that level
    auto flanks = [&](uint32_t l) {
        const uint32_t lb = (w.lmask >> l) & 1u, rb = (w.rmask >> l) & 1u;
        uint32_t cv[8];
        if (first && lb && t + 1 == s) {
            get_cv(cv, proofs + at * 8);
            put_cv(lds[t], cv);
        }
        if (last && rb && t == e + 1) {
            get_cv(cv, proofs + (at + lb) * 8);
            put_cv(lds[t], cv);
        }
        at += lb + rb;
    };
    if (w.levels) flanks(0);
    __syncthreads();
    for (uint32_t l = 0; l < w.levels; l++) {
        const uint32_t e2 = e + ((last && ((w.rmask >> l) & 1u)) ? 1u : 0u);  // the last slot with the right entry
        s >>= 1, e >>= 1;  // the parents' slots: pairs start at the even slot at or below the first
        uint32_t res[8];
        bool have = false;
        if (t >= s && t <= e) {
            if (2 * t + 1 <= e2) {
                uint32_t a[8], b[8];
                get_cv(a, lds[2 * t]);
                get_cv(b, lds[2 * t + 1]);
                sdb3::parent<false>(res, a, b, fin && l + 1 == w.levels ? (uint32_t)sdb3::ROOT : 0u);
            } else {
                get_cv(res, lds[2 * t]);  // the file's carried odd node
            }
            have = true;
        }
        __syncthreads();
        if (have) put_cv(lds[t], res);
        if (l + 1 < w.levels) flanks(l + 1);
        __syncthreads();
    }
    if (t == 0) {
        uint32_t cv[8];
        get_cv(cv, lds[0]);
        put_cv((fin ? top : scratch) + w.dst * 8, cv);
    }
}

// Range gather: one lane per range copies the flanks that exist, bottom-up and left before right,
// to the range's place among the packed proofs: level 0's from the caller's level, the others from
// the scratch k_tree_levels filled.
__global__ __launch_bounds__(256) void k_tree_range_gather(const ck_range_row* __restrict__ rrow, uint64_t q,
                                                           const uint4* __restrict__ nodes,
                                                           const uint4* __restrict__ scratch,
                                                           const uint64_t* __restrict__ lvl_off,
                                                           uint4* __restrict__ out) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < q; r += (uint64_t)gridDim.x * blockDim.x) {
        const ck_range_row w = rrow[r];
        uint64_t lo = w.first, hi = w.first + w.count - 1;
        uint4* o = out + 2 * w.pbase;
        uint32_t L = 0;
        for (uint64_t n = w.nb; n > 1; n = (n + 1) >> 1, lo >>= 1, hi >>= 1, L++) {
            const uint4* lvl = L == 0 ? nodes + 2 * w.node0 : scratch + 2 * lvl_off[w.lvl_tab + L - 1];
            if (lo & 1) {
                o[0] = lvl[2 * (lo - 1)];
                o[1] = lvl[2 * (lo - 1) + 1];
                o += 2;
            }
            if (!(hi & 1) && hi + 1 < n) {
                o[0] = lvl[2 * (hi + 1)];
                o[1] = lvl[2 * (hi + 1) + 1];
                o += 2;
            }
        }
    }
}

// range i's claimed root differs from its file's; the file is marked
struct range_differs {
    const uint4* __restrict__ top;
    const uint4* __restrict__ roots;
    const ck_range_row* __restrict__ rrow;
    uint8_t* __restrict__ file_bad;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t f = rrow[i].file;
        const uint4 a0 = top[2 * i], a1 = top[2 * i + 1], b0 = roots[2 * f], b1 = roots[2 * f + 1];
        const bool d = a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y ||
                       a1.z != b1.z || a1.w != b1.w;
        if (d) file_bad[f] = 1;
        return d;
    }
};

// (file, first block, blocks) per flagged range, in range order
struct range_rows : from_flags {
    const ck_range_row* __restrict__ rrow;
    uint64_t* __restrict__ rows;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        rows[3 * slot] = rrow[i].file;
        rows[3 * slot + 1] = rrow[i].first;
        rows[3 * slot + 2] = rrow[i].count;
    }
};

// the range verify's scratch in a pooled slot: the rows' nodes, the ranges' claimed roots, the
// flags when the caller wants none, the files' marks, two rows of per-workgroup counts
struct ranges_scratch {
    uint8_t *nodes, *top, *flags, *file_bad;
    uint64_t* counts;
    static size_t bytes(uint64_t m, uint64_t q, uint64_t n) {
        return 256 + round256(32 * m) + round256(32 * q) + round256(q) + round256(n) +
               round256(2 * BLOCKS * sizeof(uint64_t));
    }
    ranges_scratch(void* base, uint64_t m, uint64_t q, uint64_t n) {
        uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)base + 255) & ~uintptr_t(255));
        nodes = p, p += round256(32 * m);
        top = p, p += round256(32 * q);
        flags = p, p += round256(q);
        file_bad = p, p += round256(n);
        counts = reinterpret_cast<uint64_t*>(p);
    }
};

void need_ranges(const sd_checksum_tree_blocks* b) {
    if (!b->ranges.set) throw sd_failure(SD_ERR_INVALID, "sd_checksum_tree_blocks_set_ranges has not been called");
}

// the first range call after _set_ranges: the ranges' rows, the climb passes and their scratch
void upload_blocks_ranges(sd_checksum_tree_blocks* b) {
    if (b->ranges_up) return;
    b->gtab.begin();
    b->o_rrow = b->gtab.add(b->ranges.rrow);
    b->o_gpass.clear();
    for (const auto& ps : b->ranges.passes) b->o_gpass.push_back(b->gtab.add(ps));
    b->gtab.upload(nullptr);
    b->tops.ensure(32 * b->ranges.scratch_nodes);
    b->ranges_up = true;
}

// the first _prove_ranges': the level offsets, k_tree_levels' passes and the interior levels' scratch
void plan_blocks_range_levels(sd_checksum_tree_blocks* b) {
    TreeProofPlan& lv = b->ranges.levels;
    if (lv.levels) return;
    plan_tree_proofs(lv, b->plan.node_base, b->ranges.firsts.data(), b->ranges.q(), true);
    b->gltab.begin();
    b->o_rlvl = b->gltab.add(lv.lvl_off);
    b->o_rlpass.clear();
    for (const auto& ps : lv.passes) b->o_rlpass.push_back(b->gltab.add(ps));
    b->gltab.upload(nullptr);
    b->rlevels.ensure(32 * lv.scratch_nodes);
}

// the first proof call's tables: the rows' and the listed files' level offsets
void plan_blocks_proof_rows(sd_checksum_tree_blocks* b) {
    plan_tree_proofs(b->proofs, b->plan.node_base, b->rows.data(), b->m(), false);
    b->ptab.begin();
    b->o_prow = b->ptab.add(b->proofs.prow);
    b->o_lvl = b->ptab.add(b->proofs.lvl_off);
    b->ptab.upload(nullptr);
}

// the first _prove's: the passes' tables and the scratch of the interior levels
void plan_blocks_proof_levels(sd_checksum_tree_blocks* b) {
    if (b->proofs.levels) return;
    plan_tree_proofs(b->proofs, b->plan.node_base, b->rows.data(), b->m(), true);
    b->ltab.begin();
    b->o_lpass.clear();
    for (const auto& ps : b->proofs.passes) b->o_lpass.push_back(b->ltab.add(ps));
    b->ltab.upload(nullptr);
    b->levels.ensure(32 * b->proofs.scratch_nodes);
}

// _update's roots: the reduce passes over the whole level layout, as plan_tree's
void plan_blocks_roots(sd_checksum_tree_blocks* b) {
    const size_t n = b->n_files;
    const std::vector<uint64_t>& nb = b->plan.node_base;
    std::vector<uint64_t> level_n(n), base(nb.begin(), nb.end() - 1);
    for (size_t i = 0; i < n; i++) level_n[i] = nb[i + 1] - nb[i];
    b->roots.lvl_cap[0] = b->roots.lvl_cap[1] = 0;
    plan_reduce_passes(b->roots, std::move(level_n), std::move(base));
    b->rtab.begin();
    b->o_base = b->rtab.add(nb);
    b->o_pass.clear();
    for (const auto& ps : b->roots.passes) b->o_pass.push_back(b->rtab.add(ps));
    b->rtab.upload(nullptr);
    b->lvl[0].ensure(b->roots.lvl_cap[0] * 32);
    b->lvl[1].ensure(b->roots.lvl_cap[1] * 32);
    b->roots_planned = true;
}

void plan_tree(sd_checksum_tree* t, const uint64_t* offsets, const uint64_t* lens, size_t n, uint32_t block_log2) {
    plan_tree_layout(lens, n, block_log2, t->node_base);  // refuses a bad block_log2 before anything is allocated
    plan_checksum_batch(&t->ck, offsets, lens, n, nullptr);
    t->block_log2 = block_log2;
    std::vector<uint64_t> level_n(n), base(t->node_base.begin(), t->node_base.end() - 1);
    for (size_t i = 0; i < n; i++) level_n[i] = t->node_base[i + 1] - t->node_base[i];
    t->roots.lvl_cap[0] = t->roots.lvl_cap[1] = 0;
    plan_reduce_passes(t->roots, std::move(level_n), std::move(base));
    t->tab.begin();
    t->o_base = t->tab.add(t->node_base);
    t->o_pass.clear();
    for (const auto& ps : t->roots.passes) t->o_pass.push_back(t->tab.add(ps));
    t->tab.upload(nullptr);
    t->lvl[0].ensure(t->roots.lvl_cap[0] * 32);
    t->lvl[1].ensure(t->roots.lvl_cap[1] * 32);
}

// leaf pass with the level -> nodes; roots of files of at most 1 MiB -> out, longer files' 1 MiB CVs
// -> the batch's level 0
void run_tree_leaf(const sd_checksum_tree* t, const uint8_t* d_data, uint8_t* nodes, uint8_t* out, hipStream_t s) {
    HIP_CHECK(sdk::launch_ck_leaf_tree(d_data, t->ck.d_files(), t->ck.d_map(), (uint32_t)t->ck.plan.wg_map.size(),
                                       t->ck.lvl[0].as<uint32_t>(), reinterpret_cast<uint32_t*>(out), t->d_base(),
                                       t->block_log2, reinterpret_cast<uint32_t*>(nodes), s));
}

// every file's root from a level buffer: the one-node files' copied, the others' reduced with the
// level as the reduce's level 0 (T: a tree or a block list, which plan the same passes)
template <class T>
void run_level_roots(const T* t, uint64_t n, const uint8_t* d_nodes, uint8_t* d_hash32, hipStream_t s) {
    uint32_t* out = reinterpret_cast<uint32_t*>(d_hash32);
    hipLaunchKernelGGL(k_tree_single_roots, dim3(flat_grid(8 * n)), dim3(256), 0, s, t->d_base(), n,
                       reinterpret_cast<const uint32_t*>(d_nodes), out);
    HIP_CHECK(hipGetLastError());
    for (size_t k = 0; k < t->roots.passes.size(); k++) {
        const uint32_t* src = k == 0 ? reinterpret_cast<const uint32_t*>(d_nodes) : t->lvl[k & 1].template as<uint32_t>();
        HIP_CHECK(sdk::launch_ck_reduce(src, t->lvl[1 - (k & 1)].template as<uint32_t>(), t->d_pass(k),
                                        (uint32_t)t->roots.passes[k].size(), out, s));
    }
}

void check_aligned16(const void* p, const char* what) {
    if (reinterpret_cast<uintptr_t>(p) % 16) throw sd_failure(SD_ERR_INVALID, std::string(what) + " must be 16-byte aligned");
}

}  // namespace

extern "C" {

int sd_checksum_tree_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                            uint32_t block_log2, sd_checksum_tree** out) {
    SD_GUARD_BEGIN
    if (!ctx || !out || (n && (!offsets || !lens))) throw sd_failure(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    ctx->bind();
    auto t = std::make_unique<sd_checksum_tree>();
    plan_tree(t.get(), offsets, lens, n, block_log2);
    *out = t.release();
    return SD_OK;
    SD_GUARD_END
}

void sd_checksum_tree_destroy(sd_checksum_tree* t) {
    try {
        delete t;
    } catch (...) {
    }
}

int sd_checksum_tree_layout(const sd_checksum_tree* t, uint64_t* node_base) {
    SD_GUARD_BEGIN
    if (!t || !node_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::copy(t->node_base.begin(), t->node_base.end(), node_base);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_stats(const sd_checksum_tree* t, uint64_t out[4]) {
    SD_GUARD_BEGIN
    if (!t || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    out[0] = t->ck.n; out[1] = t->ck.plan.total_bytes; out[2] = t->ck.plan.compressions; out[3] = t->total();
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_run(sd_cas_ctx* ctx, const sd_checksum_tree* t, const uint8_t* d_data, uint8_t* d_nodes,
                         uint8_t* d_hash32, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !t || (t->ck.n && (!d_data || !d_nodes || !d_hash32))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes, "d_nodes");
    if (t->ck.n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    run_tree_leaf(t, d_data, d_nodes, d_hash32, s);
    run_checksum_reduce(&t->ck, reinterpret_cast<uint32_t*>(d_hash32), s);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_roots(sd_cas_ctx* ctx, const sd_checksum_tree* t, const uint8_t* d_nodes, uint8_t* d_hash32,
                           void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !t || (t->ck.n && (!d_nodes || !d_hash32))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes, "d_nodes");
    const uint64_t n = t->ck.n;
    if (n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    run_level_roots(t, n, d_nodes, d_hash32, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_verify(sd_cas_ctx* ctx, const sd_checksum_tree* t, const uint8_t* d_data,
                            const uint8_t* d_expected, uint8_t* d_bad, uint64_t* d_rows_out, uint64_t capacity,
                            uint64_t* count, uint64_t stats[4], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !t || (t->ck.n && (!d_data || !d_expected))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_expected, "d_expected");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const uint64_t n = t->ck.n, total = t->total();
    if (n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    auto slot = ctx->acquire();
    struct Rel {
        sd_cas_ctx* c;
        std::unique_ptr<Slot>* s;
        ~Rel() { c->release(std::move(*s)); }
    } rel{ctx, &slot};
    slot->staged.ensure(verify_scratch::bytes(total, n));
    slot->host_hashes.ensure(2 * BLOCKS * sizeof(uint64_t));
    const verify_scratch x(slot->staged.p, total, n);
    run_tree_leaf(t, d_data, x.nodes, x.roots, s);
    HIP_CHECK(hipMemsetAsync(x.file_bad, 0, n, s));
    uint8_t* flags = d_bad ? d_bad : x.flags;
    const uint32_t g_nodes = sliced_grid(total), g_files = sliced_grid(n);
    launch_flag(g_nodes, s,
                tree_differs{reinterpret_cast<const uint4*>(x.nodes), reinterpret_cast<const uint4*>(d_expected),
                             t->d_base(), n, x.file_bad},
                nullptr, total, flags, x.counts);
    launch_flag(g_files, s, tree_file_marked{x.file_bad}, nullptr, n, nullptr, x.counts + BLOCKS);
    HIP_CHECK(hipGetLastError());
    const uint64_t* h = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, x.counts, 2 * BLOCKS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t bad_blocks = 0, bad_files = 0;
    for (uint32_t b = 0; b < g_nodes; b++) bad_blocks += h[b];
    for (uint32_t b = 0; b < g_files; b++) bad_files += h[BLOCKS + b];
    if (bad_blocks > total || bad_files > n || bad_files > bad_blocks)
        throw sd_failure(SD_ERR_INTERNAL, "verify: inconsistent totals");
    if (count) *count = bad_blocks;
    if (stats) stats[0] = n, stats[1] = total, stats[2] = bad_blocks, stats[3] = bad_files;
    if (!d_rows_out) return SD_OK;
    if (capacity < bad_blocks)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing blocks");
    if (bad_blocks == 0) return SD_OK;
    tree_rows rows{{flags}, t->d_base(), n, d_rows_out};
    launch_compact(g_nodes, s, rows, nullptr, total, x.counts, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_create(sd_cas_ctx* ctx, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                   const uint64_t* rows, const uint64_t* data_offsets, size_t m,
                                   sd_checksum_tree_blocks** out) {
    SD_GUARD_BEGIN
    if (!ctx || !out || (n_files && !lens) || (m && (!rows || !data_offsets)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n_files >= (1ull << 31) || m >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "list too large");
    auto b = std::make_unique<sd_checksum_tree_blocks>();
    plan_tree_blocks(b->plan, lens, n_files, block_log2, rows, data_offsets, m);  // refuses before any allocation
    b->block_log2 = block_log2;
    b->n_files = n_files;
    b->rows.assign(rows, rows + 2 * m);
    if (m) {
        ctx->bind();
        b->tab.begin();
        b->o_items = b->tab.add(b->plan.items);
        b->o_rows = b->tab.add(b->rows);
        b->tab.upload(nullptr);
    }
    *out = b.release();
    return SD_OK;
    SD_GUARD_END
}

void sd_checksum_tree_blocks_destroy(sd_checksum_tree_blocks* b) {
    try {
        delete b;
    } catch (...) {
    }
}

int sd_checksum_tree_blocks_stats(const sd_checksum_tree_blocks* b, uint64_t out[4]) {
    SD_GUARD_BEGIN
    if (!b || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    out[0] = b->n_files; out[1] = b->m(); out[2] = b->plan.bytes; out[3] = b->plan.compressions;
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_run(sd_cas_ctx* ctx, const sd_checksum_tree_blocks* b, const uint8_t* d_data,
                                uint8_t* d_nodes_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && (!d_data || !d_nodes_out))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes_out, "d_nodes_out");
    if (b->m() == 0) return SD_OK;
    ctx->bind();
    HIP_CHECK(sdk::launch_ck_blocks(d_data, b->d_items(), (uint32_t)b->m(), b->block_log2, false,
                                    reinterpret_cast<uint32_t*>(d_nodes_out), ctx->pick(stream)));
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_verify(sd_cas_ctx* ctx, const sd_checksum_tree_blocks* b, const uint8_t* d_data,
                                   const uint8_t* d_expected, uint8_t* d_bad, uint64_t* d_rows_out,
                                   uint64_t capacity, uint64_t* count, uint64_t stats[4], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && (!d_data || !d_expected))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_expected, "d_expected");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const uint64_t n = b->n_files, m = b->m();
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    auto slot = ctx->acquire();
    struct Rel {
        sd_cas_ctx* c;
        std::unique_ptr<Slot>* s;
        ~Rel() { c->release(std::move(*s)); }
    } rel{ctx, &slot};
    slot->staged.ensure(blocks_scratch::bytes(m, n));
    slot->host_hashes.ensure(2 * BLOCKS * sizeof(uint64_t));
    const blocks_scratch x(slot->staged.p, m, n);
    HIP_CHECK(sdk::launch_ck_blocks(d_data, b->d_items(), (uint32_t)m, b->block_log2, false,
                                    reinterpret_cast<uint32_t*>(x.nodes), s));
    HIP_CHECK(hipMemsetAsync(x.file_bad, 0, n, s));
    uint8_t* flags = d_bad ? d_bad : x.flags;
    const uint32_t g_rows = sliced_grid(m), g_files = sliced_grid(n);
    launch_flag(g_rows, s,
                blocks_differ{reinterpret_cast<const uint4*>(x.nodes), reinterpret_cast<const uint4*>(d_expected),
                              b->d_items(), b->d_rows(), x.file_bad},
                nullptr, m, flags, x.counts);
    launch_flag(g_files, s, tree_file_marked{x.file_bad}, nullptr, n, nullptr, x.counts + BLOCKS);
    HIP_CHECK(hipGetLastError());
    const uint64_t* h = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, x.counts, 2 * BLOCKS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t bad_rows = 0, bad_files = 0;
    for (uint32_t g = 0; g < g_rows; g++) bad_rows += h[g];
    for (uint32_t g = 0; g < g_files; g++) bad_files += h[BLOCKS + g];
    if (bad_rows > m || bad_files > n || bad_files > bad_rows)
        throw sd_failure(SD_ERR_INTERNAL, "verify: inconsistent totals");
    if (count) *count = bad_rows;
    if (stats) stats[0] = n, stats[1] = m, stats[2] = bad_rows, stats[3] = bad_files;
    if (!d_rows_out) return SD_OK;
    if (capacity < bad_rows) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing rows");
    if (bad_rows == 0) return SD_OK;
    blocks_rows rows{{flags}, b->d_rows(), d_rows_out};
    launch_compact(g_rows, s, rows, nullptr, m, x.counts, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_update(sd_cas_ctx* ctx, sd_checksum_tree_blocks* b, const uint8_t* d_data,
                                   uint8_t* d_nodes, uint8_t* d_hash32, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && (!d_data || !d_nodes || !d_hash32))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes, "d_nodes");
    if (b->plan.repeats) throw sd_failure(SD_ERR_INVALID, "a (file, block) is listed twice: two writers of one node");
    if (b->m() == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    if (!b->roots_planned) plan_blocks_roots(b);
    HIP_CHECK(sdk::launch_ck_blocks(d_data, b->d_items(), (uint32_t)b->m(), b->block_log2, true,
                                    reinterpret_cast<uint32_t*>(d_nodes), s));
    run_level_roots(b, b->n_files, d_nodes, d_hash32, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_proof_layout(sd_checksum_tree_blocks* b, uint64_t* proof_base) {
    SD_GUARD_BEGIN
    if (!b || !proof_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (b->proofs.proof_base.empty()) plan_tree_proofs(b->proofs, b->plan.node_base, b->rows.data(), b->m(), false);
    std::copy(b->proofs.proof_base.begin(), b->proofs.proof_base.end(), proof_base);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_prove(sd_cas_ctx* ctx, sd_checksum_tree_blocks* b, const uint8_t* d_nodes,
                                  uint8_t* d_proofs_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && !d_nodes)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes, "d_nodes");
    check_aligned16(d_proofs_out, "d_proofs_out");
    const uint64_t m = b->m();
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    if (!b->ptab.bytes) plan_blocks_proof_rows(b);
    if (b->proofs.proof_base[m] == 0) return SD_OK;  // one-node files only: every proof is empty
    if (!d_proofs_out) throw sd_failure(SD_ERR_INVALID, "null argument");
    plan_blocks_proof_levels(b);
    uint32_t* scratch = b->levels.as<uint32_t>();
    for (size_t k = 0; k < b->proofs.passes.size(); k++) {
        hipLaunchKernelGGL(k_tree_levels, dim3((uint32_t)b->proofs.passes[k].size()), dim3(256), 0, s,
                           k == 0 ? reinterpret_cast<const uint32_t*>(d_nodes) : scratch, scratch, b->d_lpass(k),
                           b->d_lvl_off());
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tree_proof_gather, dim3(flat_grid(m)), dim3(256), 0, s, b->d_prow(), b->d_rows(), m,
                       reinterpret_cast<const uint4*>(d_nodes), reinterpret_cast<const uint4*>(scratch), b->d_lvl_off(),
                       reinterpret_cast<uint4*>(d_proofs_out));
    HIP_CHECK(hipGetLastError());
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_verify_proofs(sd_cas_ctx* ctx, sd_checksum_tree_blocks* b, const uint8_t* d_data,
                                          const uint8_t* d_proofs, const uint8_t* d_roots, uint8_t* d_nodes_out,
                                          uint8_t* d_bad, uint64_t* d_rows_out, uint64_t capacity, uint64_t* count,
                                          uint64_t stats[4], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && (!d_data || !d_roots))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_proofs, "d_proofs");
    check_aligned16(d_roots, "d_roots");
    check_aligned16(d_nodes_out, "d_nodes_out");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const uint64_t n = b->n_files, m = b->m();
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    if (!b->ptab.bytes) plan_blocks_proof_rows(b);
    if (b->proofs.proof_base[m] && !d_proofs) throw sd_failure(SD_ERR_INVALID, "null argument");
    auto slot = ctx->acquire();
    struct Rel {
        sd_cas_ctx* c;
        std::unique_ptr<Slot>* s;
        ~Rel() { c->release(std::move(*s)); }
    } rel{ctx, &slot};
    slot->staged.ensure(blocks_scratch::bytes(m, n));
    slot->host_hashes.ensure(2 * BLOCKS * sizeof(uint64_t));
    const blocks_scratch x(slot->staged.p, m, n);
    uint8_t* nodes = d_nodes_out ? d_nodes_out : x.nodes;
    HIP_CHECK(sdk::launch_ck_blocks(d_data, b->d_items(), (uint32_t)m, b->block_log2, false,
                                    reinterpret_cast<uint32_t*>(nodes), s));
    HIP_CHECK(hipMemsetAsync(x.file_bad, 0, n, s));
    uint8_t* flags = d_bad ? d_bad : x.flags;
    const uint32_t g_rows = sliced_grid(m), g_files = sliced_grid(n);
    launch_flag(g_rows, s,
                proof_climb{reinterpret_cast<const uint32_t*>(nodes), reinterpret_cast<const uint32_t*>(d_proofs),
                            reinterpret_cast<const uint32_t*>(d_roots), b->d_prow(), b->d_rows(), x.file_bad},
                nullptr, m, flags, x.counts);
    launch_flag(g_files, s, tree_file_marked{x.file_bad}, nullptr, n, nullptr, x.counts + BLOCKS);
    HIP_CHECK(hipGetLastError());
    const uint64_t* h = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, x.counts, 2 * BLOCKS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t bad_rows = 0, bad_files = 0;
    for (uint32_t g = 0; g < g_rows; g++) bad_rows += h[g];
    for (uint32_t g = 0; g < g_files; g++) bad_files += h[BLOCKS + g];
    if (bad_rows > m || bad_files > n || bad_files > bad_rows)
        throw sd_failure(SD_ERR_INTERNAL, "verify_proofs: inconsistent totals");
    if (count) *count = bad_rows;
    if (stats) stats[0] = n, stats[1] = m, stats[2] = bad_rows, stats[3] = bad_files;
    if (!d_rows_out) return SD_OK;
    if (capacity < bad_rows) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing rows");
    if (bad_rows == 0) return SD_OK;
    blocks_rows rows{{flags}, b->d_rows(), d_rows_out};
    launch_compact(g_rows, s, rows, nullptr, m, x.counts, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_set_ranges(sd_checksum_tree_blocks* b, const uint64_t* range_base, size_t q) {
    SD_GUARD_BEGIN
    if (!b || (q && !range_base)) throw sd_failure(SD_ERR_INVALID, "null argument");
    plan_tree_ranges(b->ranges, b->plan.node_base, b->rows.data(), b->m(), range_base, q);  // throws: nothing changed
    b->ranges_up = false;
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_range_proof_layout(sd_checksum_tree_blocks* b, uint64_t* proof_base) {
    SD_GUARD_BEGIN
    if (!b || !proof_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (b->m() == 0) {
        proof_base[0] = 0;
        return SD_OK;
    }
    need_ranges(b);
    std::copy(b->ranges.proof_base.begin(), b->ranges.proof_base.end(), proof_base);
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_prove_ranges(sd_cas_ctx* ctx, sd_checksum_tree_blocks* b, const uint8_t* d_nodes,
                                         uint8_t* d_proofs_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && !d_nodes)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_nodes, "d_nodes");
    check_aligned16(d_proofs_out, "d_proofs_out");
    if (b->m() == 0) return SD_OK;
    need_ranges(b);
    const uint64_t q = b->ranges.q();
    if (b->ranges.proof_base[q] == 0) return SD_OK;  // whole files and one-node files only: every proof is empty
    if (!d_proofs_out) throw sd_failure(SD_ERR_INVALID, "null argument");
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    upload_blocks_ranges(b);
    plan_blocks_range_levels(b);
    const TreeProofPlan& lv = b->ranges.levels;
    uint32_t* scratch = b->rlevels.as<uint32_t>();
    for (size_t k = 0; k < lv.passes.size(); k++) {
        hipLaunchKernelGGL(k_tree_levels, dim3((uint32_t)lv.passes[k].size()), dim3(256), 0, s,
                           k == 0 ? reinterpret_cast<const uint32_t*>(d_nodes) : scratch, scratch, b->d_rlpass(k),
                           b->d_rlvl_off());
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tree_range_gather, dim3(flat_grid(q)), dim3(256), 0, s, b->d_rrow(), q,
                       reinterpret_cast<const uint4*>(d_nodes), reinterpret_cast<const uint4*>(scratch), b->d_rlvl_off(),
                       reinterpret_cast<uint4*>(d_proofs_out));
    HIP_CHECK(hipGetLastError());
    return SD_OK;
    SD_GUARD_END
}

int sd_checksum_tree_blocks_verify_range_proofs(sd_cas_ctx* ctx, sd_checksum_tree_blocks* b, const uint8_t* d_data,
                                                const uint8_t* d_proofs, const uint8_t* d_roots, uint8_t* d_nodes_out,
                                                uint8_t* d_bad, uint64_t* d_ranges_out, uint64_t capacity,
                                                uint64_t* count, uint64_t stats[4], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->m() && (!d_data || !d_roots))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_aligned16(d_proofs, "d_proofs");
    check_aligned16(d_roots, "d_roots");
    check_aligned16(d_nodes_out, "d_nodes_out");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    const uint64_t n = b->n_files, m = b->m();
    if (m == 0) return SD_OK;
    need_ranges(b);
    const uint64_t q = b->ranges.q();
    if (b->ranges.proof_base[q] && !d_proofs) throw sd_failure(SD_ERR_INVALID, "null argument");
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    upload_blocks_ranges(b);
    auto slot = ctx->acquire();
    struct Rel {
        sd_cas_ctx* c;
        std::unique_ptr<Slot>* s;
        ~Rel() { c->release(std::move(*s)); }
    } rel{ctx, &slot};
    slot->staged.ensure(ranges_scratch::bytes(m, q, n));
    slot->host_hashes.ensure(2 * BLOCKS * sizeof(uint64_t));
    const ranges_scratch x(slot->staged.p, m, q, n);
    uint8_t* nodes = d_nodes_out ? d_nodes_out : x.nodes;
    HIP_CHECK(sdk::launch_ck_blocks(d_data, b->d_items(), (uint32_t)m, b->block_log2, false,
                                    reinterpret_cast<uint32_t*>(nodes), s));
    HIP_CHECK(hipMemsetAsync(x.file_bad, 0, n, s));
    uint32_t* tops = b->tops.as<uint32_t>();
    for (size_t k = 0; k < b->ranges.passes.size(); k++) {
        hipLaunchKernelGGL(k_tree_range_climb, dim3((uint32_t)b->ranges.passes[k].size()), dim3(256), 0, s,
                           k == 0 ? reinterpret_cast<const uint32_t*>(nodes) : tops, tops,
                           reinterpret_cast<const uint32_t*>(d_proofs), b->d_gpass(k), reinterpret_cast<uint32_t*>(x.top));
        HIP_CHECK(hipGetLastError());
    }
    uint8_t* flags = d_bad ? d_bad : x.flags;
    const uint32_t g_ranges = sliced_grid(q), g_files = sliced_grid(n);
    launch_flag(g_ranges, s,
                range_differs{reinterpret_cast<const uint4*>(x.top), reinterpret_cast<const uint4*>(d_roots), b->d_rrow(),
                              x.file_bad},
                nullptr, q, flags, x.counts);
    launch_flag(g_files, s, tree_file_marked{x.file_bad}, nullptr, n, nullptr, x.counts + BLOCKS);
    HIP_CHECK(hipGetLastError());
    const uint64_t* h = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, x.counts, 2 * BLOCKS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t bad_ranges = 0, bad_files = 0;
    for (uint32_t g = 0; g < g_ranges; g++) bad_ranges += h[g];
    for (uint32_t g = 0; g < g_files; g++) bad_files += h[BLOCKS + g];
    if (bad_ranges > q || bad_files > n || bad_files > bad_ranges)
        throw sd_failure(SD_ERR_INTERNAL, "verify_range_proofs: inconsistent totals");
    if (count) *count = bad_ranges;
    if (stats) stats[0] = n, stats[1] = q, stats[2] = bad_ranges, stats[3] = bad_files;
    if (!d_ranges_out) return SD_OK;
    if (capacity < bad_ranges)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing ranges");
    if (bad_ranges == 0) return SD_OK;
    range_rows rows{{flags}, b->d_rrow(), d_ranges_out};
    launch_compact(g_ranges, s, rows, nullptr, q, x.counts, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
