// object_index.hip -- the device-resident Object index: lookup, the indexed owner rule with
// its compacted list of new group heads, insertion (merge by rank + directory rebuild) and
// removal by key or by Object (flag, two-way ordered compaction, directory rebuild); and the
// owners mode (one entry per (key, Object id) with a link count): the same passes over (key,
// id), after a batch of pairs has been aggregated to distinct pairs with multiplicities; and
// apply, that mode's removal with ids and insert in one flagging pass and one fused
// merge-compaction; and that mode's read-only view by Object: the link totals of listed ids and
// the orphans among them, in one pass over the entries; and its read-only view by key: the
// duplicate groups (the runs of equal keys) with their link and owner totals, selected by
// thresholds and compacted in order; and merge Objects, which relabels the owners by a map and
// coalesces the pairs that meet, in apply's rewrite.
//
// Reference semantics: identifier_job_step joins a step's cas_ids against the Objects the
// library already has (core/src/object/file_identifier/mod.rs:168-175), links each file to
// the first of them (:189-225) and creates Objects for the rest (:229-333).  Layout and
// lookup: object_index.h (shared with the host mirror, object_index_host.cpp).
//
// Ordered compaction (new heads; an insert's surviving pairs; a removal's survivors and its
// dropped entries; distinct pairs, ids and groups) without atomics on the data path: a fixed
// grid in which workgroup b owns the contiguous slice b of the input.  sliced.h holds the slice
// and tile arithmetic and the two kernel skeletons over it (sliced_flag, sliced_compact); every
// such pass here is a functor of a few lines over one of them.
// k_apply_merge (apply's and the merge's rewrite), k_group_totals, k_entry_flag, k_object_totals, k_key_links and k_group_stats use
// the slices in ways of their own and stand alone, on that header's primitives.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "object_index.h"
#include "sd_internal.h"
#include "sliced.h"

using namespace sliced;

namespace {

// the first of a run of equal values in a sorted array: the listed ids by Object, the groups
// (runs of equal keys) of the index
struct run_head {
    const uint64_t* __restrict__ a;
    __device__ bool operator()(uint64_t i, uint64_t) const { return i == 0 || a[i - 1] != a[i]; }
};

// bytes already written, counted per slice: the marks of k_remove_mark (0 or 1), apply's
// leaving entries (mark 1)
struct marked {
    const uint8_t* __restrict__ mark;
    __device__ bool operator()(uint64_t i, uint64_t) const { return mark[i] == 1; }
};

__global__ __launch_bounds__(256) void k_index_lookup(const uint64_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ vals,
                                                      const uint64_t* __restrict__ dir, uint32_t bits,
                                                      const uint64_t* __restrict__ q, uint64_t m,
                                                      uint64_t* __restrict__ out, uint8_t* __restrict__ found) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t at;
        const bool f = oi_find(keys, dir, bits, q[i], &at);
        found[i] = f ? 1 : 0;
        out[i] = f ? vals[at] : 0;
    }
}

// The indexed owner rule per grouped record (sorted by (key, index): neighbouring lanes read
// neighbouring index lines).  existing[i] = 1 if owner[i] is an Object id of the index, else
// owner[i] is what k_owners writes; bit 1 of existing[i] carries the new-head flag (a group's
// first record whose key the index does not have) to heads_out, which clears it.
struct owners_indexed_rule {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ dir;
    uint32_t bits;
    const uint64_t *__restrict__ rec, *__restrict__ rep;
    uint64_t chunk;
    uint64_t* __restrict__ owner;
    uint8_t* __restrict__ existing;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t key = rec[2 * i], idx = rec[2 * i + 1], r = rep[i];
        uint64_t at;
        const bool f = oi_find(keys, dir, bits, key, &at);
        const bool head = !f && (i == 0 || rec[2 * (i - 1)] != key);
        owner[i] = f ? vals[at] : (idx / chunk == r / chunk ? idx : r);
        existing[i] = (uint8_t)((f ? 1 : 0) | (head ? 2 : 0));
        return head;
    }
};

// (key, index) of the flagged heads, in record order = ascending key order
struct heads_out {
    const uint64_t* __restrict__ rec;
    uint8_t* __restrict__ existing;
    uint64_t* __restrict__ new_out;
    __device__ bool flag(uint64_t i) const { return (existing[i] & 2) != 0; }
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        new_out[2 * slot] = rec[2 * i];
        new_out[2 * slot + 1] = rec[2 * i + 1];
        existing[i] = 0;  // a head's key is not in the index: bit 0 is clear
    }
};

// an insert's pairs sorted by (key, position): a pair survives if it is its key's first, its
// key belongs to this shard and the index does not have it
struct insert_keep {
    const uint64_t *__restrict__ keys, *__restrict__ dir;
    uint32_t bits;
    int nparts, part;
    const uint64_t* __restrict__ sk;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t k = sk[i];
        if ((i != 0 && sk[i - 1] == k) || oi_dest_of(k, nparts) != (uint32_t)part) return false;
        uint64_t at;
        return !oi_find(keys, dir, bits, k, &at);
    }
};

struct insert_out : from_flags {
    const uint64_t *__restrict__ sk, *__restrict__ spos, *__restrict__ in_vals;
    uint64_t *__restrict__ nk, *__restrict__ nv;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        nk[slot] = sk[i];
        nv[slot] = in_vals[spos[i]];
    }
};

// Merge by rank of two sorted runs without common keys: lanes [0, r) place the new entries
// (rank + the old keys below, through the old directory), lanes [r, r + n) the old ones
// (position + the new keys below).
__global__ __launch_bounds__(256) void k_index_merge(const uint64_t* __restrict__ keys,
                                                     const uint64_t* __restrict__ vals,
                                                     const uint64_t* __restrict__ dir, uint32_t bits, uint64_t n,
                                                     const uint64_t* __restrict__ nk, const uint64_t* __restrict__ nv,
                                                     uint64_t r, uint64_t* __restrict__ out_keys,
                                                     uint64_t* __restrict__ out_vals) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n + r; t += (uint64_t)gridDim.x * blockDim.x) {
        if (t < r) {
            const uint64_t k = nk[t], at = t + oi_rank(keys, dir, bits, k);
            out_keys[at] = k;
            out_vals[at] = nv[t];
        } else {
            const uint64_t i = t - r, k = keys[i], at = i + oi_lower_bound(nk, 0, r, k);
            out_keys[at] = k;
            out_vals[at] = vals[i];
        }
    }
}

// dir[q] = i for q in (prefix(key[i-1]), prefix(key[i])]; the last position fills the tail with n
__global__ __launch_bounds__(256) void k_index_dir(const uint64_t* __restrict__ keys, uint64_t n, uint32_t bits,
                                                   uint64_t* __restrict__ dir) {
    const uint64_t nb = 1ull << bits;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t first = i == 0 ? 0 : oi_prefix(keys[i - 1], bits) + 1;
        const uint64_t cur = oi_prefix(keys[i], bits);
        for (uint64_t q = first; q <= cur; q++) dir[q] = i;
        if (i + 1 == n)
            for (uint64_t q = cur + 1; q <= nb; q++) dir[q] = n;
    }
}

// ---- removal (orphan_remover.rs:57-95 deletes Objects; watcher/utils.rs:410-494 moves a
// file_path to another cas_id).  flags[n], one byte per entry of the index: 1 = dropped.
// By key: every input pair marks the entry it removes (oi_remove_hit); pairs that hit the same
// entry all write the same byte, so the flags do not depend on the order the lanes ran in.
__global__ __launch_bounds__(256) void k_remove_mark(const uint64_t* __restrict__ keys,
                                                     const uint64_t* __restrict__ vals,
                                                     const uint64_t* __restrict__ dir, uint32_t bits,
                                                     const uint64_t* __restrict__ rk, const uint64_t* __restrict__ rid,
                                                     uint64_t m, uint8_t* __restrict__ flags) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t id = rid ? rid[i] : 0;
        uint64_t at;
        if (oi_remove_hit(keys, vals, dir, bits, rk[i], rid ? &id : nullptr, &at)) flags[at] = 1;
    }
}

// By Object: an entry goes if its value is among the ids (sorted ascending)
struct listed {
    const uint64_t *__restrict__ vals, *__restrict__ sorted_ids;
    uint64_t m;
    __device__ bool operator()(uint64_t i, uint64_t) const { return oi_id_listed(sorted_ids, m, vals[i]); }
};

// Two-way ordered compaction: the slot is the number of dropped entries before the position,
// which is a dropped entry's row of rm_out (may be null) and, taken from its position, a
// survivor's place in the other buffer pair.
struct remove_out : from_flags {
    const uint64_t *__restrict__ keys, *__restrict__ vals;
    uint64_t *__restrict__ out_keys, *__restrict__ out_vals, *__restrict__ rm_out;
    const uint64_t *__restrict__ links, *__restrict__ asked;
    uint64_t* __restrict__ out_links;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        const uint64_t k = keys[i], v = vals[i];
        if (!flag) {
            out_keys[i - slot] = k;
            out_vals[i - slot] = v;
            // owners mode: the third array, less the links a removal with ids asked for
            if (out_links) out_links[i - slot] = links[i] - (asked ? asked[i] : 0);
        } else if (rm_out) {
            rm_out[2 * slot] = k;
            rm_out[2 * slot + 1] = v;
        }
    }
};

// ---- owners mode (object_index.h): one entry per (key, Object id) and links[n].
// A batch of pairs is first aggregated: two stable radix sorts (by id, then by key) leave it
// in (key, id) order; the heads of the runs of equal pairs are flagged and compacted in order
// with their positions, so a distinct pair's multiplicity is the distance to the next head
// (the last one's to m): no lane walks a run, however many copies of one pair there are.
struct pair_head {
    const uint64_t *__restrict__ sk, *__restrict__ sv;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        return i == 0 || sk[i - 1] != sk[i] || sv[i - 1] != sv[i];
    }
};

struct pair_out : from_flags {
    const uint64_t *__restrict__ sk, *__restrict__ sv;
    uint64_t *__restrict__ dk, *__restrict__ dv, *__restrict__ dpos;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        dk[slot] = sk[i];
        dv[slot] = sv[i];
        dpos[slot] = i;
    }
};

// the multiplicity of distinct pair i of d: from its run's head to the next one's (the last
// one's to m, the pairs of the batch)
__device__ __forceinline__ uint64_t run_length(const uint64_t* __restrict__ dpos, uint64_t i, uint64_t d, uint64_t m) {
    return (i + 1 < d ? dpos[i + 1] : m) - dpos[i];
}

// Insert: every distinct pair (d of them, the pass's bound) takes its (key, id) rank in the
// index and its state: 0 = another shard's key, 1 = absent (merges in at its rank), 2 = present
// (adds its multiplicity to the entry at its rank).  Flags the absent ones.  MARK (apply): a
// present pair also marks its entry 2.
template <bool MARK>
struct pair_state {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ dir;
    uint32_t bits;
    int nparts, part;
    const uint64_t *__restrict__ dk, *__restrict__ dv, *__restrict__ dpos;
    uint64_t m;
    uint64_t *__restrict__ dcnt, *__restrict__ drank;
    uint8_t *__restrict__ dstate, *__restrict__ mark;
    __device__ bool operator()(uint64_t i, uint64_t d) const {
        const uint64_t k = dk[i], v = dv[i];
        uint64_t at = 0;
        uint8_t st = 0;
        if (oi_dest_of(k, nparts) == (uint32_t)part) st = oi_find_pair(keys, vals, dir, bits, k, v, &at) ? 2 : 1;
        dcnt[i] = run_length(dpos, i, d, m);
        drank[i] = at;
        dstate[i] = st;
        if (MARK && st == 2) mark[at] = 2;
        return st == 1;
    }
};

// the absent pairs in order; RANK (apply): with their ranks in the index as it stands
// (non-decreasing)
template <bool RANK>
struct enter_out {
    const uint64_t *__restrict__ dk, *__restrict__ dv, *__restrict__ dcnt, *__restrict__ drank;
    const uint8_t* __restrict__ dstate;
    uint64_t *__restrict__ nk, *__restrict__ nv, *__restrict__ nl, *__restrict__ nrank;
    __device__ bool flag(uint64_t i) const { return dstate[i] == 1; }
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        nk[slot] = dk[i];
        nv[slot] = dv[i];
        nl[slot] = dcnt[i];
        if (RANK) nrank[slot] = drank[i];
    }
};

// k_index_merge over (key, id): two sorted runs without common pairs
__global__ __launch_bounds__(256) void k_owners_merge(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ links,
    const uint64_t* __restrict__ dir, uint32_t bits, uint64_t n, const uint64_t* __restrict__ nk,
    const uint64_t* __restrict__ nv, const uint64_t* __restrict__ nl, uint64_t r, uint64_t* __restrict__ out_keys,
    uint64_t* __restrict__ out_vals, uint64_t* __restrict__ out_links) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n + r; t += (uint64_t)gridDim.x * blockDim.x) {
        if (t < r) {
            const uint64_t k = nk[t], v = nv[t], at = t + oi_rank_pair(keys, vals, dir, bits, k, v);
            out_keys[at] = k;
            out_vals[at] = v;
            out_links[at] = nl[t];
        } else {
            const uint64_t i = t - r, k = keys[i], v = vals[i], at = i + oi_lower_bound_pair(nk, nv, 0, r, k, v);
            out_keys[at] = k;
            out_vals[at] = v;
            out_links[at] = links[i];
        }
    }
}

// the present pairs add their multiplicity to their entry, which the merge of r new entries
// moved up by the new pairs below it; distinct pairs name distinct entries: one writer each
__global__ __launch_bounds__(256) void k_owners_add_links(
    const uint64_t* __restrict__ dk, const uint64_t* __restrict__ dv, const uint64_t* __restrict__ dcnt,
    const uint64_t* __restrict__ drank, const uint8_t* __restrict__ dstate, const uint64_t* __restrict__ d_total,
    const uint64_t* __restrict__ nk, const uint64_t* __restrict__ nv, uint64_t r, uint64_t* __restrict__ links) {
    const uint64_t d = *d_total;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (uint64_t)gridDim.x * blockDim.x) {
        if (dstate[i] != 2) continue;
        const uint64_t at = drank[i] + (r ? oi_lower_bound_pair(nk, nv, 0, r, dk[i], dv[i]) : 0);
        links[at] += dcnt[i];
    }
}

// Removal with ids: every distinct pair leaves the links asked at its entry (asked[n], zeroed
// before; one writer per entry), then the entries asked for at least what they hold are flagged
__global__ __launch_bounds__(256) void k_owners_remove_ask(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ dir,
    uint32_t bits, const uint64_t* __restrict__ dk, const uint64_t* __restrict__ dv,
    const uint64_t* __restrict__ dpos, const uint64_t* __restrict__ d_total, uint64_t m,
    uint64_t* __restrict__ asked) {
    const uint64_t d = *d_total;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t at;
        if (oi_find_pair(keys, vals, dir, bits, dk[i], dv[i], &at))
            asked[at] = run_length(dpos, i, d, m);
    }
}

struct links_drop {
    const uint64_t *__restrict__ links, *__restrict__ asked;
    __device__ bool operator()(uint64_t i, uint64_t) const { return oi_links_drop(links[i], asked[i]); }
};

// A removal with ids after which no entry leaves: every distinct pair takes its multiplicity
// from its entry in place (less than the entry holds, or it would have been flagged); distinct
// pairs name distinct entries: one writer each
__global__ __launch_bounds__(256) void k_owners_take_links(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ dir,
    uint32_t bits, const uint64_t* __restrict__ dk, const uint64_t* __restrict__ dv,
    const uint64_t* __restrict__ dpos, const uint64_t* __restrict__ d_total, uint64_t m,
    uint64_t* __restrict__ links) {
    const uint64_t d = *d_total;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t at;
        if (oi_find_pair(keys, vals, dir, bits, dk[i], dv[i], &at))
            links[at] -= run_length(dpos, i, d, m);
    }
}

__global__ __launch_bounds__(256) void k_index_links(const uint64_t* __restrict__ keys,
                                                     const uint64_t* __restrict__ vals,
                                                     const uint64_t* __restrict__ links,
                                                     const uint64_t* __restrict__ dir, uint32_t bits,
                                                     const uint64_t* __restrict__ qk, const uint64_t* __restrict__ qv,
                                                     uint64_t m, uint64_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t at;
        out[i] = oi_find_pair(keys, vals, dir, bits, qk[i], qv[i], &at) ? links[at] : 0;
    }
}

// ---- apply (owners mode): a removal list and an insertion list in one call, one rewrite.
// Both lists are aggregated (above).  A pair absent from the index is untouched by the
// removal list, so the two lists meet only at present entries: mark[n], one byte per entry,
//   0 = no pair names it, 1 = it leaves (oi_links_after == 0), 2 = it stays and only the
//   insertion list names it, 3 = it stays and the removal list names it,
// and the absent pairs of the insertion list enter at their (key, id) rank.  An entry is named
// by at most one distinct pair of each list, and the pass over the removal list runs after the
// pass over the insertion list: one writer per byte per pass, the later pass decides.

// the multiplicity of (key, id) in an aggregated batch (d distinct pairs in (key, id) order
// with the head positions of their runs among m pairs), 0 if it is not there
__device__ __forceinline__ uint64_t pair_multiplicity(const uint64_t* __restrict__ dk, const uint64_t* __restrict__ dv,
                                                      const uint64_t* __restrict__ dpos, uint64_t d, uint64_t m,
                                                      uint64_t key, uint64_t id) {
    const uint64_t j = oi_lower_bound_pair(dk, dv, 0, d, key, id);
    if (j >= d || dk[j] != key || dv[j] != id) return 0;
    return run_length(dpos, j, d, m);
}

// (The insertion list's pass is pair_state<true>, its compaction enter_out<true>: the insert's
// own instantiations carry neither the mark nor the rank.)

// every distinct pair of the removal list that names an entry decides it: leaving or staying
__global__ __launch_bounds__(256) void k_apply_mark_removals(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ links,
    const uint64_t* __restrict__ dir, uint32_t bits, const uint64_t* __restrict__ rk, const uint64_t* __restrict__ rv,
    const uint64_t* __restrict__ rpos, const uint64_t* __restrict__ r_total, uint64_t m_rm,
    const uint64_t* __restrict__ ik, const uint64_t* __restrict__ iv, const uint64_t* __restrict__ ipos,
    const uint64_t* __restrict__ i_total, uint64_t m_in, uint8_t* __restrict__ mark) {
    const uint64_t d = *r_total, di = *i_total;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = rk[i], v = rv[i];
        uint64_t at;
        if (!oi_find_pair(keys, vals, dir, bits, k, v, &at)) continue;
        const uint64_t asked = run_length(rpos, i, d, m_rm);
        const uint64_t added = pair_multiplicity(ik, iv, ipos, di, m_in, k, v);
        mark[at] = oi_links_after(links[at], asked, added) == 0 ? 1 : 3;
    }
}

// Nothing leaves and nothing enters: the links change at their entries.  Lanes [0, d_rm) take
// the entries the removal list names (mark 3: both lists' multiplicities), lanes [d_rm, d_rm +
// d_in) those only the insertion list names (mark 2); one writer per entry.
__global__ __launch_bounds__(256) void k_apply_links_in_place(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ dir,
    uint32_t bits, const uint64_t* __restrict__ rk, const uint64_t* __restrict__ rv,
    const uint64_t* __restrict__ rpos, const uint64_t* __restrict__ r_total, uint64_t m_rm,
    const uint64_t* __restrict__ ik, const uint64_t* __restrict__ iv, const uint64_t* __restrict__ ipos,
    const uint64_t* __restrict__ icnt, const uint64_t* __restrict__ irank, const uint8_t* __restrict__ istate,
    const uint64_t* __restrict__ i_total, uint64_t m_in, const uint8_t* __restrict__ mark,
    uint64_t* __restrict__ links) {
    const uint64_t d = *r_total, di = *i_total;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < d + di; t += (uint64_t)gridDim.x * blockDim.x) {
        if (t < d) {
            const uint64_t k = rk[t], v = rv[t];
            uint64_t at;
            if (!oi_find_pair(keys, vals, dir, bits, k, v, &at)) continue;
            const uint64_t asked = run_length(rpos, t, d, m_rm);
            links[at] = oi_links_after(links[at], asked, pair_multiplicity(ik, iv, ipos, di, m_in, k, v));
        } else {
            const uint64_t j = t - d;
            if (istate[j] == 2 && mark[irank[j]] == 2) links[irank[j]] += icnt[j];
        }
    }
}

// the links afterwards of a staying entry that apply's lists name (mark 2: the insertion list
// alone, 3: the removal list too)
struct apply_links {
    const uint64_t *__restrict__ rk, *__restrict__ rv, *__restrict__ rpos, *__restrict__ r_total;
    uint64_t m_rm;
    const uint64_t *__restrict__ ik, *__restrict__ iv, *__restrict__ ipos, *__restrict__ i_total;
    uint64_t m_in;
    __device__ uint64_t operator()(uint8_t mk, uint64_t k, uint64_t v, uint64_t l) const {
        return oi_links_after(l, mk == 3 ? pair_multiplicity(rk, rv, rpos, *r_total, m_rm, k, v) : 0,
                              pair_multiplicity(ik, iv, ipos, *i_total, m_in, k, v));
    }
};

// The one rewrite: k_owners_merge and the owners branch of remove_out in one sliced pass
// over the entries.  With L(i) the leaving entries before position i (block_base + tile_slot)
// and E(i) the entering pairs ranked at or before i (a search of nrank[r]):
//   a staying entry i      -> out[i - L(i) + E(i)], with oi_links_after where a pair names it
//   a leaving entry i      -> row L(i) of rm_out (may be null)
//   the entering pair j    -> out[q - L(q) + j], q = nrank[j]: the tile that holds position q
//                             places it (L inside a tile from LDS); the tile that holds the
//                             last entry also places the pairs ranked at n
// n == 0: workgroup 0 copies the entering pairs.
// A staying entry that a pair names (mark >= 2) takes its links from `after` (apply_links above,
// merge_links below).  r is *d_r if d_r is set (a count the host never waited for), else the value.
template <class After>
__global__ __launch_bounds__(256) void k_apply_merge(
    const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const uint64_t* __restrict__ links,
    uint64_t n, const uint8_t* __restrict__ mark, const uint64_t* __restrict__ counts, After after,
    const uint64_t* __restrict__ nk, const uint64_t* __restrict__ nv, const uint64_t* __restrict__ nl,
    const uint64_t* __restrict__ nrank, const uint64_t* __restrict__ d_r, uint64_t r,
    uint64_t* __restrict__ out_keys, uint64_t* __restrict__ out_vals, uint64_t* __restrict__ out_links,
    uint64_t* __restrict__ rm_out) {
    __shared__ uint32_t before[257];  // leaving entries of the tile before each lane; [256] = all
    if (d_r) r = *d_r;
    if (n == 0) {
        if (blockIdx.x == 0)
            for (uint64_t j = threadIdx.x; j < r; j += blockDim.x) {
                out_keys[j] = nk[j];
                out_vals[j] = nv[j];
                out_links[j] = nl[j];
            }
        return;
    }
    uint64_t run = block_base(counts, nullptr);
    const slice sl = slice_of(n);
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi;
        const uint8_t mk = act ? mark[i] : 0;
        const bool leave = mk == 1;
        const uint64_t tile_run = run;
        const uint64_t slot = tile_slot(leave, run);
        const uint64_t end = base + blockDim.x < sl.hi ? base + blockDim.x : sl.hi;
        // the entering pairs this tile places: ranks in [base, end), and n with the last entry
        const uint64_t e_lo = oi_lower_bound(nrank, 0, r, base);
        const uint64_t e_hi = end == n ? r : oi_lower_bound(nrank, e_lo, r, end);
        if (e_hi > e_lo) {  // the same for every lane
            before[threadIdx.x] = (uint32_t)(slot - tile_run);
            if (threadIdx.x == 255) before[256] = (uint32_t)(slot - tile_run) + (leave ? 1 : 0);
            __syncthreads();
            for (uint64_t j = e_lo + threadIdx.x; j < e_hi; j += blockDim.x) {
                const uint64_t q = nrank[j], at = q - (tile_run + before[q - base]) + j;
                out_keys[at] = nk[j];
                out_vals[at] = nv[j];
                out_links[at] = nl[j];
            }
            __syncthreads();
        }
        if (!act) continue;
        const uint64_t k = keys[i], v = vals[i];
        if (leave) {
            if (rm_out) {
                rm_out[2 * slot] = k;
                rm_out[2 * slot + 1] = v;
            }
            continue;
        }
        const uint64_t at = i - slot + (e_hi > e_lo ? oi_lower_bound(nrank, e_lo, e_hi, i + 1) : e_lo);
        uint64_t l = links[i];
        if (mk >= 2) l = after(mk, k, v, l);
        out_keys[at] = k;
        out_vals[at] = v;
        out_links[at] = l;
    }
}

// ---- merge Objects (object_index.h oi_relabel / oi_map_contradicts; mod.rs:229-333 gives
// same-step duplicates an Object each): the map sorted by `from`; one pass over its rows counts
// the contradictions, one sliced pass over the entries marks those whose id phi changes (mark 1,
// apply's leaving entries).  The host reads both counts in its one wait.  First mode: the marked
// entries are relabelled in place.  Owners mode: the leaving entries are compacted in order into
// rows (key, phi(id), links), put into (key, id) order by two stable sorts of their positions,
// and coalesced: the heads of the runs of equal pairs are compacted as aggregate_pairs does, and a
// run's links are the difference of two elements of the rows' inclusive scan, so no lane walks a
// run however many ids of one key go to one.  A coalesced pair that meets an entry that stays adds
// its sum there (mark 2); one that meets a leaving entry, or none, enters at its rank.  The
// rewrite is k_apply_merge with merge_links.
struct map_contradiction {
    const uint64_t *__restrict__ sf, *__restrict__ st;
    __device__ bool operator()(uint64_t i, uint64_t) const { return oi_map_contradicts(sf, st, i); }
};

struct relabelled {
    const uint64_t *__restrict__ vals, *__restrict__ sf, *__restrict__ st;
    uint64_t m;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t v = vals[i];
        return oi_relabel(sf, st, m, v) != v;
    }
};

// first mode: one entry per key, so the marked entries take phi(id) where they stand
__global__ __launch_bounds__(256) void k_relabel_in_place(const uint8_t* __restrict__ mark,
                                                          const uint64_t* __restrict__ sf,
                                                          const uint64_t* __restrict__ st, uint64_t m, uint64_t n,
                                                          uint64_t* __restrict__ vals) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (mark[i]) vals[i] = oi_relabel(sf, st, m, vals[i]);
}

struct leaving_rows : from_flags {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ links, *__restrict__ sf, *__restrict__ st;
    uint64_t m;
    uint64_t *__restrict__ rk, *__restrict__ rv, *__restrict__ rl;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        rk[slot] = keys[i];
        rv[slot] = oi_relabel(sf, st, m, vals[i]);
        rl[slot] = links[i];
    }
};

// out[i] = a[pos[i]] (and outb[i] = b[pos[i]] where b is given): the rows behind sorted positions
__global__ __launch_bounds__(256) void k_gather_rows(const uint64_t* __restrict__ pos, uint64_t m,
                                                     const uint64_t* __restrict__ a, uint64_t* __restrict__ out,
                                                     const uint64_t* __restrict__ b, uint64_t* __restrict__ outb) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = pos[i];
        out[i] = a[p];
        if (b) outb[i] = b[p];
    }
}

// Every coalesced pair (d of them, the pass's bound) takes the links of its run (pre = the
// inclusive scan of the m rows' links in (key, id) order; u64 sums wrap alike on both sides of the
// difference), its (key, id) rank in the index and its state: 2 = it meets an entry that stays
// and marks it 2 (distinct pairs name distinct entries: one reader and one writer per byte), 1 =
// it enters.  Flags the entering ones.
struct merged_pair_state {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ dir;
    uint32_t bits;
    const uint64_t *__restrict__ dk, *__restrict__ dv, *__restrict__ dpos, *__restrict__ pre;
    uint64_t m;
    uint64_t *__restrict__ dcnt, *__restrict__ drank;
    uint8_t *__restrict__ dstate, *mark;
    __device__ bool operator()(uint64_t i, uint64_t d) const {
        uint64_t at;
        const bool stays = oi_find_pair(keys, vals, dir, bits, dk[i], dv[i], &at) && mark[at] == 0;
        const uint64_t lo = dpos[i], hi = i + 1 < d ? dpos[i + 1] : m;
        dcnt[i] = pre[hi - 1] - (lo ? pre[lo - 1] : 0);
        drank[i] = at;
        dstate[i] = stays ? 2 : 1;
        if (stays) mark[at] = 2;
        return !stays;
    }
};

// the links afterwards of a staying entry that a coalesced pair met (mark 2)
struct merge_links {
    const uint64_t *__restrict__ dk, *__restrict__ dv, *__restrict__ dcnt, *__restrict__ d_total;
    __device__ uint64_t operator()(uint8_t, uint64_t k, uint64_t v, uint64_t l) const {
        return l + dcnt[oi_lower_bound_pair(dk, dv, 0, *d_total, k, v)];
    }
};

// ---- by Object, read-only (owners mode): per-Object link totals and the orphans among listed
// ids (object_index.h oi_object_slot / oi_unowned; orphan_remover.rs:57-95 asks the DB which
// Objects have no file_path).  The listed ids are sorted with their positions (the strided
// read is the sort's input iterator), the heads of the runs of equal ids compacted in order to
// the distinct ids u[d], and every position keeps its run's slot, so repeats share one answer.
struct strided_ids {
    const uint64_t* p;
    uint64_t stride;
    __host__ __device__ uint64_t operator()(uint64_t j) const { return p[j * stride]; }
};

// (The heads are run_head over the sorted ids.)  u[slot] = the run's id; pslot[position] = the
// slot of the position's id: the slot counts the heads before a position, which is a head's own
// slot and one more than a follower's
struct ids_out : from_flags {
    const uint64_t *__restrict__ sid, *__restrict__ spos;
    uint64_t *__restrict__ u, *__restrict__ pslot;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (flag) u[slot] = sid[i];
        pslot[spos[i]] = flag ? slot : slot - 1;  // position 0 is a head: a follower has one before it
    }
};

// The one pass over the entries, from the entry side: vals[i] (8 B per entry, coalesced) is
// searched among the distinct ids -- staged in LDS when the list is at most OI_LDS_IDS ids -- and
// only a hit reads links[i].  tot[2 * slot] = links, tot[2 * slot + 1] = entries, zeroed before.
// SUMS: a lane keeps the totals of the slot it hit last in registers (one Object owning a large
// share of the entries adds up there, not at one address); lanes that meet another slot first
// add what they hold combined by equal slot within the wave (wave_flush).  With the ids in LDS
// those adds go to per-slot totals of the workgroup in LDS (16 KB), which leave for global
// memory once, at the end of the slice: one pair of global adds per workgroup and slot, however
// many heavy Objects alternate along the entries.  Without (more than OI_LDS_IDS ids) they go to
// global memory, and what the lanes hold at the end of the slice is combined by equal slot
// across the workgroup (two rounds: the slots most lanes hold; the rest add alone).  Integer
// sums: any order is exact.
// !SUMS (orphans): a hit stores 1 at tot[2 * slot + 1]; every writer writes the same value.
constexpr uint32_t OI_LDS_IDS = 1024;

__device__ __forceinline__ void add_totals(uint64_t* __restrict__ tot, uint64_t slot, uint64_t links, uint64_t entries) {
    atomicAdd(reinterpret_cast<unsigned long long*>(tot + 2 * slot), (unsigned long long)links);
    atomicAdd(reinterpret_cast<unsigned long long*>(tot + 2 * slot + 1), (unsigned long long)entries);
}

// The lanes of one wave with `pend` add (sum, cnt) to their slot `cur` and clear them: twice the
// lanes that hold the slot of the first pending lane add as one (a shuffle reduction, one lane
// adds), the rest add alone.  `tot` is global memory or the workgroup's table in LDS.  Called
// by every lane of the wave.
__device__ __forceinline__ void wave_flush(uint64_t* __restrict__ tot, bool pend, uint64_t cur, uint64_t& sum,
                                           uint64_t& cnt) {
    const uint32_t lane = threadIdx.x & 63;
    for (int round = 0; round < 2; round++) {
        const uint64_t bal = __ballot(pend);
        if (!bal) return;  // the same for every lane
        const int leader = __ffsll((unsigned long long)bal) - 1;
        const uint64_t chosen = __shfl(cur, leader);
        const bool same = pend && cur == chosen;
        uint64_t l = same ? sum : 0, e = same ? cnt : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l += __shfl_xor(l, o);
            e += __shfl_xor(e, o);
        }
        if (lane == (uint32_t)leader) add_totals(tot, chosen, l, e);
        if (same) sum = cnt = 0;
        pend = pend && !same;
    }
    if (pend) {
        add_totals(tot, cur, sum, cnt);
        sum = cnt = 0;
    }
}

template <bool LDS, bool SUMS>
__global__ __launch_bounds__(256) void k_object_totals(const uint64_t* __restrict__ vals,
                                                       const uint64_t* __restrict__ links, uint64_t n,
                                                       const uint64_t* __restrict__ u,
                                                       const uint64_t* __restrict__ d_total,
                                                       uint64_t* __restrict__ tot) {
    __shared__ uint64_t su[LDS ? OI_LDS_IDS : 1];
    __shared__ uint64_t lt[LDS && SUMS ? 2 * OI_LDS_IDS : 1];  // the workgroup's totals per slot
    __shared__ uint64_t pick;
    const uint64_t d = *d_total;  // <= the listed count, which chose LDS
    if (LDS) {
        for (uint64_t j = threadIdx.x; j < d && j < OI_LDS_IDS; j += blockDim.x) {
            su[j] = u[j];
            if (SUMS) lt[2 * j] = lt[2 * j + 1] = 0;
        }
        __syncthreads();
    }
    const uint64_t* ids = LDS ? su : u;
    uint64_t* acc = LDS && SUMS ? lt : tot;  // where a lane that changes slots adds what it holds
    const slice sl = slice_of(n);
    bool have = false;
    uint64_t cur = 0, sum = 0, cnt = 0;
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {  // whole tiles: the same trips for every lane
        const uint64_t i = base + threadIdx.x;
        uint64_t slot = 0;
        const bool hit = i < sl.hi && oi_object_slot(ids, d, vals[i], &slot);
        if (!SUMS) {
            if (hit) tot[2 * slot + 1] = 1;
            continue;
        }
        // lanes that meet another slot give up what they hold, combined by equal slot in the wave
        const bool change = hit && have && slot != cur;
        if (__any(change)) wave_flush(acc, change, cur, sum, cnt);
        if (hit) {
            have = true;
            cur = slot;
            sum += links[i];
            cnt++;
        }
    }
    if (!SUMS) return;
    if (LDS) {  // the workgroup's totals leave LDS once: one pair of global adds per slot it hit
        wave_flush(acc, have, cur, sum, cnt);
        __syncthreads();
        for (uint64_t j = threadIdx.x; j < d && j < OI_LDS_IDS; j += blockDim.x)
            if (lt[2 * j + 1]) add_totals(tot, j, lt[2 * j], lt[2 * j + 1]);
        return;
    }
    bool pend = have;
    for (int round = 0; round < 2; round++) {
        if (!__syncthreads_or(pend)) break;  // the same for every lane
        if (pend) pick = cur;                // any one of the pending slots
        __syncthreads();
        const uint64_t chosen = pick;
        const bool same = pend && cur == chosen;
        uint64_t le[2] = {same ? sum : 0, same ? cnt : 0};
        block_sum(le);
        if (threadIdx.x == 0) add_totals(tot, chosen, le[0], le[1]);
        pend = pend && !same;
    }
    if (pend) add_totals(tot, cur, sum, cnt);
}

// the totals of every position's slot, to the caller's order (either output may be null)
__global__ __launch_bounds__(256) void k_object_scatter(const uint64_t* __restrict__ pslot,
                                                        const uint64_t* __restrict__ tot, uint64_t m,
                                                        uint64_t* __restrict__ links_out,
                                                        uint64_t* __restrict__ entries_out) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t slot = pslot[j];
        if (links_out) links_out[j] = tot[2 * slot];
        if (entries_out) entries_out[j] = tot[2 * slot + 1];
    }
}

// orphans: the distinct ids without an entry, flagged and counted per slice, then compacted in
// order (ascending, as u is) once the host has checked the count against the capacity
struct unowned {
    const uint64_t* __restrict__ tot;
    __device__ bool operator()(uint64_t i, uint64_t) const { return oi_unowned(tot[2 * i + 1]); }
};

struct orphans_out : from_flags {
    const uint64_t* __restrict__ u;
    uint64_t* __restrict__ out;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (flag) out[slot] = u[i];
    }
};

// ---- by key, read-only (owners mode): the duplicate groups (object_index.h oi_key_run /
// oi_qualifies; mod.rs:189-225 links later copies to an Object, :229-333 gives same-step
// duplicates an Object each).  The index is sorted, so a group is a run of equal keys and its
// slot is the number of heads before it (block_base + tile_slot over the head flags).
//
// key_links: per listed key the run's bounds by two searches in its bucket.  A run of at most
// OI_RUN_SERIAL entries is summed by its lane; longer ones are summed by the whole wave, one run
// after the other (64 * OI_RUN_LOADS consecutive links per step, OI_RUN_LOADS loads in flight per
// lane: one wave is bound by the memory's latency, not its bandwidth), so RUN owners of one key
// cost RUN / 512 steps.
constexpr uint64_t OI_RUN_SERIAL = 64;
constexpr uint32_t OI_RUN_LOADS = 8;

template <bool SUMS>
__global__ __launch_bounds__(256) void k_key_links(const uint64_t* __restrict__ keys,
                                                   const uint64_t* __restrict__ links,
                                                   const uint64_t* __restrict__ dir, uint32_t bits,
                                                   const uint64_t* __restrict__ q, uint64_t m,
                                                   uint64_t* __restrict__ links_out,
                                                   uint64_t* __restrict__ owners_out) {
    const uint32_t lane = threadIdx.x & 63;
    // whole tiles: the same trips for every lane of a wave
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < m;
        uint64_t lo = 0, hi = 0;
        if (act) oi_key_run(keys, dir, bits, q[i], &lo, &hi);
        if (act && owners_out) owners_out[i] = hi - lo;
        if (!SUMS) continue;
        uint64_t sum = 0;
        const bool wide = hi - lo > OI_RUN_SERIAL;
        if (!wide)
            for (uint64_t j = lo; j < hi; j++) sum += links[j];
        uint64_t todo = __ballot(wide);
        while (todo) {  // the same for every lane
            const int leader = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t l0 = __shfl(lo, leader), h0 = __shfl(hi, leader);
            uint64_t p[OI_RUN_LOADS] = {};  // that many loads in flight per lane
            for (uint64_t j = l0 + lane; j < h0; j += 64 * OI_RUN_LOADS) {
                // every load is issued before the first add waits for one: a lane past the run's end
                // reads the run's last link and adds 0
                uint64_t v[OI_RUN_LOADS];
#pragma unroll
                for (uint32_t u = 0; u < OI_RUN_LOADS; u++) v[u] = links[j + 64 * u < h0 ? j + 64 * u : h0 - 1];
#pragma unroll
                for (uint32_t u = 0; u < OI_RUN_LOADS; u++) p[u] += j + 64 * u < h0 ? v[u] : 0;
            }
            uint64_t part = 0;
#pragma unroll
            for (uint32_t u = 0; u < OI_RUN_LOADS; u++) part += p[u];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
            if (lane == (uint32_t)leader) sum = part;
        }
        if (act) links_out[i] = sum;
    }
}

// (The heads of the runs of equal keys are counted per workgroup slice by run_head.)
// Group totals.  Every entry learns its group's slot; a head stores its position at hpos[slot],
// so owners(slot) = hpos[slot + 1] - hpos[slot] (the last one's from n) with no sum at all.
// links: a segmented sum by slot inside the wave (the lanes of one run are neighbours; each step
// takes the partial sum `o` lanes down unless that lane lies before the run's first lane in this
// wave), which leaves the run's sum over this wave at the run's last lane here.  A run that
// begins and ends inside the wave -- most do -- costs one plain store; a run that crosses a wave,
// tile or slice border costs one u64 add per wave it touches into gl[slot] (zeroed before;
// integer sums are exact in any order), so a run of many slices combines across workgroups and no
// lane walks anything.  A slot is written either by one store or by adds, never both.
__global__ __launch_bounds__(256) void k_group_totals(const uint64_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ links, uint64_t n,
                                                      const uint64_t* __restrict__ counts,
                                                      uint64_t* __restrict__ hpos, uint64_t* __restrict__ gl,
                                                      uint64_t* __restrict__ g_total) {
    uint64_t run = block_base(counts, g_total);
    const slice sl = slice_of(n);
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi;
        const uint64_t key = act ? keys[i] : 0;
        const bool head = act && (i == 0 || keys[i - 1] != key);
        const uint64_t slot = tile_slot(head, run);
        if (head) hpos[slot] = i;
        // a segment of the wave begins at lane 0, at a head and at every inactive lane
        const uint64_t starts = __ballot(lane == 0 || head || !act);
        const uint64_t heads = __ballot(head);
        const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1;
        const uint32_t first = 63 - (uint32_t)__clzll((long long)(starts & upto));  // bit 0 is set
        uint64_t sum = act ? links[i] : 0;
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint64_t below = __shfl_up(sum, o);
            if (lane >= first + o) sum += below;
        }
        const bool last = act && (lane == 63 || ((starts >> (lane + 1)) & 1));
        if (!last) continue;
        const uint64_t gs = head ? slot : slot - 1;  // position 0 is a head: a follower has one before it
        const bool opens = (heads >> first) & 1;
        const bool closes = i + 1 == n || keys[i + 1] != key;
        if (opens && closes) gl[gs] = sum;
        else atomicAdd(reinterpret_cast<unsigned long long*>(gl + gs), (unsigned long long)sum);
    }
}

__device__ __forceinline__ uint64_t group_owners(const uint64_t* __restrict__ hpos, uint64_t g, uint64_t groups,
                                                 uint64_t n) {
    return (g + 1 < groups ? hpos[g + 1] : n) - hpos[g];
}

// Selection per group (the pass's bound is the groups): gflags[g] = the group qualifies
struct group_ok {
    const uint64_t *__restrict__ hpos, *__restrict__ gl;
    uint64_t n, min_links, min_owners;
    __device__ bool operator()(uint64_t g, uint64_t groups) const {
        return oi_qualifies(gl[g], group_owners(hpos, g, groups, n), min_links, min_owners);
    }
};

// one row per qualifying group in group order = ascending key order; key and first owner are
// read at the head's position (every output may be null)
struct group_out : from_flags {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ hpos, *__restrict__ gl;
    uint64_t n;
    uint64_t *__restrict__ keys_out, *__restrict__ first_out, *__restrict__ links_out, *__restrict__ owners_out;
    __device__ void emit(uint64_t g, bool flag, uint64_t slot, uint64_t groups) const {
        if (!flag) return;
        const uint64_t at = hpos[g];
        if (keys_out) keys_out[slot] = keys[at];
        if (first_out) first_out[slot] = vals[at];
        if (links_out) links_out[slot] = gl[g];
        if (owners_out) owners_out[slot] = group_owners(hpos, g, groups, n);
    }
};

// Selection per entry: an entry is selected iff its group is.  The group's slot is found again as
// in k_group_totals (the head counts per slice are still there); eflags[i] and the selected
// entries per slice are left for the compaction.
__global__ __launch_bounds__(256) void k_entry_flag(const uint64_t* __restrict__ keys, uint64_t n,
                                                    const uint64_t* __restrict__ head_counts,
                                                    const uint8_t* __restrict__ gflags,
                                                    uint8_t* __restrict__ eflags, uint64_t* __restrict__ counts) {
    uint64_t run = block_base(head_counts, nullptr);
    const slice sl = slice_of(n);
    uint32_t mine = 0;
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi;
        const bool head = act && (i == 0 || keys[i - 1] != keys[i]);
        const uint64_t slot = tile_slot(head, run);
        if (!act) continue;
        const bool sel = gflags[head ? slot : slot - 1] != 0;
        eflags[i] = sel ? 1 : 0;
        mine += sel;
    }
    block_count(mine, counts);
}

struct entry_out : from_flags {
    const uint64_t *__restrict__ keys, *__restrict__ vals, *__restrict__ links;
    uint64_t *__restrict__ keys_out, *__restrict__ ids_out, *__restrict__ links_out;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        if (keys_out) keys_out[slot] = keys[i];
        if (ids_out) ids_out[slot] = vals[i];
        if (links_out) links_out[slot] = links[i];
    }
};

// Stats: one reduction over the group totals.  A lane sums its groups in registers, the wave by
// shuffles, the workgroup through LDS; one workgroup adds seven sums and one maximum to st[8]
// (zeroed before).  st[0] (the groups) and st[1] (the entries) are known and set by workgroup 0.
__global__ __launch_bounds__(256) void k_group_stats(const uint64_t* __restrict__ hpos,
                                                     const uint64_t* __restrict__ gl,
                                                     const uint64_t* __restrict__ g_total, uint64_t n,
                                                     uint64_t* __restrict__ st) {
    __shared__ uint64_t wmax[4];
    const uint64_t groups = *g_total;
    const slice sl = slice_of(groups);
    uint64_t v[5] = {0, 0, 0, 0, 0}, big = 0;  // v[k] is st[2 + k]; big = the largest links(k)
    for (uint64_t g = sl.lo + threadIdx.x; g < sl.hi; g += blockDim.x) {
        const uint64_t l = gl[g], o = group_owners(hpos, g, groups, n);
        v[0] += l;
        if (l >= 2) v[1] += 1, v[2] += l;
        if (o >= 2) v[3] += 1, v[4] += o;
        if (l > big) big = l;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t other = __shfl_xor(big, o);
        if (other > big) big = other;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = big;
    block_sum(v);  // its first barrier is wmax's too
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 5; k++)
        if (v[k]) atomicAdd(reinterpret_cast<unsigned long long*>(st + 2 + k), (unsigned long long)v[k]);
    uint64_t mx = wmax[0];
    for (int w = 1; w < 4; w++) mx = wmax[w] > mx ? wmax[w] : mx;
    if (mx) atomicMax(reinterpret_cast<unsigned long long*>(st + 7), (unsigned long long)mx);
    if (blockIdx.x == 0) st[0] = groups, st[1] = n;
}

size_t remove_sort_bytes(uint64_t m, hipStream_t s) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (rocprim::radix_sort_keys(nullptr, b, nul, nul, (size_t)m, 0, 64, s) != hipSuccess) return 0;
    return round256(b);
}

// An aggregated batch of m pairs in scratch: a[5][m] u64 (the first sort's ids and keys, later
// the distinct pairs dk, dv; the second sort's sk, sv, later an insert's nk, nv; dpos), an
// insert's dcnt, drank, nl [m] u64, heads[m] and dstate[m] u8, the distinct count and an
// insert's count (u64, 256 bytes apart), then the radix sort's temporary storage.
struct pair_batch {
    uint64_t *t0, *t1, *sk, *sv, *dpos, *dcnt, *drank, *nl, *d_total, *r_total;
    uint8_t *heads, *dstate;
    void* tmp;
};

size_t pair_batch_bytes(uint64_t m, bool insert) {
    return round256((insert ? 8 : 5) * m * sizeof(uint64_t)) + round256(2 * m) + 512 + sort_pairs_bytes(m, nullptr) +
           256;
}

pair_batch pair_batch_at(void* base, uint64_t m, bool insert) {
    pair_batch b;
    uint64_t* u = reinterpret_cast<uint64_t*>(base);
    b.t0 = u, b.t1 = u + m, b.sk = u + 2 * m, b.sv = u + 3 * m, b.dpos = u + 4 * m;
    b.dcnt = insert ? u + 5 * m : nullptr, b.drank = insert ? u + 6 * m : nullptr, b.nl = insert ? u + 7 * m : nullptr;
    uint8_t* p = reinterpret_cast<uint8_t*>(base) + round256((insert ? 8 : 5) * m * sizeof(uint64_t));
    b.heads = p, b.dstate = p + m;
    p += round256(2 * m);
    b.d_total = reinterpret_cast<uint64_t*>(p), b.r_total = reinterpret_cast<uint64_t*>(p + 256);
    b.tmp = p + 512;
    return b;
}

// (key, id) order by two stable sorts, then the distinct pairs (t0 = keys, t1 = ids) with the
// positions of their runs' heads and their count
hipError_t aggregate_pairs(const pair_batch& b, const uint64_t* in_keys, const uint64_t* in_ids, uint64_t m,
                           uint64_t* counts, hipStream_t s) {
    size_t tb = sort_pairs_bytes(m, s);
    hipError_t e = rocprim::radix_sort_pairs(b.tmp, tb, in_ids, b.t0, in_keys, b.t1, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(b.tmp, tb, b.t1, b.sk, b.t0, b.sv, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    const uint32_t g = sliced_grid(m);
    launch_flag(g, s, pair_head{b.sk, b.sv}, nullptr, m, b.heads, counts);
    launch_compact(g, s, pair_out{{b.heads}, b.sk, b.sv, b.t0, b.t1, b.dpos}, nullptr, m, counts, b.d_total);
    return hipGetLastError();
}

}  // namespace

namespace sdk {

uint32_t index_slots(uint64_t n) { return sliced_grid(n); }

hipError_t index_lookup(const oi_view& x, const uint64_t* q, uint64_t m, uint64_t* out, uint8_t* found,
                        hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_index_lookup, dim3(flat_grid(m)), dim3(256), 0, s, x.keys, x.vals, x.dir, x.bits, q, m, out,
                       found);
    return hipGetLastError();
}

hipError_t owners_indexed(const oi_view& x, const uint64_t* records, uint64_t m, const uint64_t* rep, uint64_t chunk,
                          uint64_t* owner, uint8_t* existing, uint64_t* new_out, uint64_t* n_new, uint64_t* counts,
                          hipStream_t s) {
    if (m == 0) return hipMemsetAsync(n_new, 0, sizeof(uint64_t), s);
    const uint32_t g = sliced_grid(m);
    launch_flag(g, s, owners_indexed_rule{x.keys, x.vals, x.dir, x.bits, records, rep, chunk, owner, existing}, nullptr,
                m, nullptr, counts);
    launch_compact(g, s, heads_out{records, existing, new_out}, nullptr, m, counts, n_new);
    return hipGetLastError();
}

// scratch: sk[m], spos[m], pos[m], nk[m], nv[m] (u64), flags[m] (u8), total (u64), then the
// radix sort's temporary storage
size_t index_insert_scratch(uint64_t m) {
    return round256(5 * m * sizeof(uint64_t) + m) + 256 + sort_pairs_bytes(m, nullptr) + 256;
}

hipError_t index_insert_select(const oi_view& x, int nparts, int part, const uint64_t* in_keys,
                               const uint64_t* in_vals, uint64_t m, void* scratch, uint64_t* counts,
                               const uint64_t** nk_out, const uint64_t** nv_out, const uint64_t** total_out,
                               hipStream_t s) {
    uint64_t* sk = reinterpret_cast<uint64_t*>(scratch);
    uint64_t* spos = sk + m;
    uint64_t* pos = spos + m;
    uint64_t* nk = pos + m;
    uint64_t* nv = nk + m;
    uint8_t* flags = reinterpret_cast<uint8_t*>(nv + m);
    uint64_t* total = reinterpret_cast<uint64_t*>(round256((uintptr_t)(flags + m)));
    void* tmp = reinterpret_cast<uint8_t*>(total) + 256;
    size_t tb = sort_pairs_bytes(m, s);
    hipLaunchKernelGGL(k_iota, dim3(flat_grid(m)), dim3(256), 0, s, pos, m);
    // a stable sort by key leaves equal keys in ascending position: (key, position) order
    hipError_t e = rocprim::radix_sort_pairs(tmp, tb, in_keys, sk, pos, spos, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    const uint32_t g = sliced_grid(m);
    launch_flag(g, s, insert_keep{x.keys, x.dir, x.bits, nparts, part, sk}, nullptr, m, flags, counts);
    launch_compact(g, s, insert_out{{flags}, sk, spos, in_vals, nk, nv}, nullptr, m, counts, total);
    *nk_out = nk;
    *nv_out = nv;
    *total_out = total;
    return hipGetLastError();
}

hipError_t index_merge(const oi_view& x, const uint64_t* nk, const uint64_t* nv, uint64_t r, uint64_t* out_keys,
                       uint64_t* out_vals, hipStream_t s) {
    if (x.n + r == 0) return hipSuccess;
    hipLaunchKernelGGL(k_index_merge, dim3(flat_grid(x.n + r)), dim3(256), 0, s, x.keys, x.vals, x.dir, x.bits, x.n, nk,
                       nv, r, out_keys, out_vals);
    return hipGetLastError();
}

// scratch: flags[n] (u8), then for a removal by Object the sorted ids[m_ids] (u64) and the
// radix sort's temporary storage
size_t index_remove_scratch(uint64_t n, uint64_t m_ids) {
    size_t b = round256(n) + 256;
    if (m_ids) b += round256(m_ids * sizeof(uint64_t)) + remove_sort_bytes(m_ids, nullptr) + 256;
    return b;
}

hipError_t index_remove_flag_keys(const oi_view& x, const uint64_t* rm_keys, const uint64_t* rm_ids, uint64_t m,
                                  void* scratch, uint64_t* counts, hipStream_t s) {
    uint8_t* flags = reinterpret_cast<uint8_t*>(scratch);
    hipError_t e = hipMemsetAsync(flags, 0, x.n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_remove_mark, dim3(flat_grid(m)), dim3(256), 0, s, x.keys, x.vals, x.dir, x.bits, rm_keys,
                       rm_ids, m, flags);
    launch_flag(sliced_grid(x.n), s, marked{flags}, nullptr, x.n, nullptr, counts);
    return hipGetLastError();
}

namespace {
// the entries whose `field` (values by Object; keys in the owners mode) is among the m listed,
// which are sorted into the scratch behind flags[n]
hipError_t remove_flag_listed(const oi_view& x, const uint64_t* field, const uint64_t* list, uint64_t m, void* scratch,
                              uint64_t* counts, hipStream_t s) {
    uint8_t* flags = reinterpret_cast<uint8_t*>(scratch);
    uint64_t* sorted = reinterpret_cast<uint64_t*>(flags + round256(x.n));
    void* tmp = reinterpret_cast<uint8_t*>(sorted) + round256(m * sizeof(uint64_t));
    size_t tb = remove_sort_bytes(m, s);
    hipError_t e = rocprim::radix_sort_keys(tmp, tb, list, sorted, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    launch_flag(sliced_grid(x.n), s, listed{field, sorted, m}, nullptr, x.n, flags, counts);
    return hipGetLastError();
}
}  // namespace

hipError_t index_remove_flag_objects(const oi_view& x, const uint64_t* ids, uint64_t m, void* scratch,
                                     uint64_t* counts, hipStream_t s) {
    return remove_flag_listed(x, x.vals, ids, m, scratch, counts, s);
}

hipError_t index_remove_compact(const oi_view& x, const void* scratch, const uint64_t* counts, uint64_t* out_keys,
                                uint64_t* out_vals, uint64_t* rm_out, hipStream_t s) {
    return index_owners_remove_compact(x, scratch, nullptr, counts, out_keys, out_vals, nullptr, rm_out, s);
}

// ---- owners mode
size_t index_owners_insert_scratch(uint64_t m) { return pair_batch_bytes(m, true); }

hipError_t index_owners_insert_select(const oi_view& x, int nparts, int part, const uint64_t* in_keys,
                                      const uint64_t* in_vals, uint64_t m, void* scratch, uint64_t* counts,
                                      const uint64_t** nk_out, const uint64_t** nv_out, const uint64_t** nl_out,
                                      const uint64_t** total_out, hipStream_t s) {
    const pair_batch b = pair_batch_at(scratch, m, true);
    hipError_t e = aggregate_pairs(b, in_keys, in_vals, m, counts, s);
    if (e != hipSuccess) return e;
    const uint32_t g = sliced_grid(m);
    launch_flag(g, s,
                pair_state<false>{x.keys, x.vals, x.dir, x.bits, nparts, part, b.t0, b.t1, b.dpos, m, b.dcnt, b.drank,
                                  b.dstate, nullptr},
                b.d_total, 0, nullptr, counts);
    launch_compact(g, s, enter_out<false>{b.t0, b.t1, b.dcnt, b.drank, b.dstate, b.sk, b.sv, b.nl, nullptr}, b.d_total,
                   0, counts, b.r_total);
    *nk_out = b.sk;
    *nv_out = b.sv;
    *nl_out = b.nl;
    *total_out = b.r_total;
    return hipGetLastError();
}

hipError_t index_owners_merge(const oi_view& x, const uint64_t* nk, const uint64_t* nv, const uint64_t* nl, uint64_t r,
                              uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, hipStream_t s) {
    if (x.n + r == 0) return hipSuccess;
    hipLaunchKernelGGL(k_owners_merge, dim3(flat_grid(x.n + r)), dim3(256), 0, s, x.keys, x.vals, x.links, x.dir, x.bits,
                       x.n, nk, nv, nl, r, out_keys, out_vals, out_links);
    return hipGetLastError();
}

hipError_t index_owners_add_links(const void* scratch, uint64_t m, const uint64_t* nk, const uint64_t* nv, uint64_t r,
                                  uint64_t* links, hipStream_t s) {
    const pair_batch b = pair_batch_at(const_cast<void*>(scratch), m, true);
    hipLaunchKernelGGL(k_owners_add_links, dim3(flat_grid(m)), dim3(256), 0, s, b.t0, b.t1, b.dcnt, b.drank, b.dstate,
                       b.d_total, nk, nv, r, links);
    return hipGetLastError();
}

// scratch: flags[n] (u8), asked[n] (u64), then the aggregated batch
size_t index_owners_remove_scratch(uint64_t n, uint64_t m) {
    return round256(n) + round256(n * sizeof(uint64_t)) + pair_batch_bytes(m, false);
}

const uint64_t* index_owners_asked(const void* scratch, uint64_t n) {
    return reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(scratch) + round256(n));
}

hipError_t index_owners_remove_flag_pairs(const oi_view& x, const uint64_t* rm_keys, const uint64_t* rm_ids,
                                          uint64_t m, void* scratch, uint64_t* counts, hipStream_t s) {
    uint8_t* flags = reinterpret_cast<uint8_t*>(scratch);
    uint64_t* asked = const_cast<uint64_t*>(index_owners_asked(scratch, x.n));
    const pair_batch b =
        pair_batch_at(reinterpret_cast<uint8_t*>(asked) + round256(x.n * sizeof(uint64_t)), m, false);
    hipError_t e = hipMemsetAsync(asked, 0, x.n * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    e = aggregate_pairs(b, rm_keys, rm_ids, m, counts, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_owners_remove_ask, dim3(flat_grid(m)), dim3(256), 0, s, x.keys, x.vals, x.dir, x.bits, b.t0,
                       b.t1, b.dpos, b.d_total, m, asked);
    launch_flag(sliced_grid(x.n), s, links_drop{x.links, asked}, nullptr, x.n, flags, counts);
    return hipGetLastError();
}

hipError_t index_owners_take_links(const oi_view& x, const void* scratch, uint64_t m, uint64_t* links, hipStream_t s) {
    const uint8_t* asked = reinterpret_cast<const uint8_t*>(index_owners_asked(scratch, x.n));
    const pair_batch b = pair_batch_at(const_cast<uint8_t*>(asked) + round256(x.n * sizeof(uint64_t)), m, false);
    hipLaunchKernelGGL(k_owners_take_links, dim3(flat_grid(m)), dim3(256), 0, s, x.keys, x.vals, x.dir, x.bits, b.t0,
                       b.t1, b.dpos, b.d_total, m, links);
    return hipGetLastError();
}

hipError_t index_owners_remove_flag_keys(const oi_view& x, const uint64_t* rm_keys, uint64_t m, void* scratch,
                                         uint64_t* counts, hipStream_t s) {
    // the entry side searches the sorted keys, as it searches the sorted ids by Object
    return remove_flag_listed(x, x.keys, rm_keys, m, scratch, counts, s);
}

hipError_t index_owners_remove_compact(const oi_view& x, const void* scratch, const uint64_t* asked,
                                       const uint64_t* counts, uint64_t* out_keys, uint64_t* out_vals,
                                       uint64_t* out_links, uint64_t* rm_out, hipStream_t s) {
    launch_compact(sliced_grid(x.n), s,
                   remove_out{{reinterpret_cast<const uint8_t*>(scratch)}, x.keys, x.vals, out_keys, out_vals, rm_out,
                              x.links, asked, out_links},
                   nullptr, x.n, counts, nullptr);
    return hipGetLastError();
}

// ---- apply.  scratch: mark[n] (u8); the per-slice counts of leaving entries, then of entering
// pairs (u64, index_slots(n) then index_slots(m_in), side by side for the host's one copy); the removal
// list's aggregated batch; the insertion list's, as an insert's; nrank[m_in] (u64)
namespace {
struct apply_scratch {
    uint8_t* mark;
    uint64_t *leaving, *entering, *nrank;
    pair_batch rm, in;
};

apply_scratch apply_scratch_at(void* base, uint64_t n, uint64_t m_rm, uint64_t m_in) {
    apply_scratch a;
    uint8_t* p = reinterpret_cast<uint8_t*>(base);
    a.mark = p;
    p += round256(n);
    a.leaving = reinterpret_cast<uint64_t*>(p);
    a.entering = a.leaving + sliced_grid(n);
    p += 2 * BLOCKS * sizeof(uint64_t);
    a.rm = pair_batch_at(p, m_rm, false);
    p += pair_batch_bytes(std::max<uint64_t>(m_rm, 1), false);
    a.in = pair_batch_at(p, m_in, true);
    p += pair_batch_bytes(std::max<uint64_t>(m_in, 1), true);
    a.nrank = reinterpret_cast<uint64_t*>(p);
    return a;
}
}  // namespace

size_t index_apply_scratch(uint64_t n, uint64_t m_rm, uint64_t m_in) {
    return round256(n) + 2 * BLOCKS * sizeof(uint64_t) + pair_batch_bytes(std::max<uint64_t>(m_rm, 1), false) +
           pair_batch_bytes(std::max<uint64_t>(m_in, 1), true) + round256(m_in * sizeof(uint64_t)) + 256;
}

const uint64_t* index_apply_counts(const void* scratch, uint64_t n) {
    return apply_scratch_at(const_cast<void*>(scratch), n, 0, 0).leaving;
}

hipError_t index_apply_flag(const oi_view& x, int nparts, int part, const uint64_t* rm_keys, const uint64_t* rm_ids,
                            uint64_t m_rm, const uint64_t* in_keys, const uint64_t* in_ids, uint64_t m_in,
                            void* scratch, uint64_t* counts, hipStream_t s) {
    const apply_scratch a = apply_scratch_at(scratch, x.n, m_rm, m_in);
    hipError_t e = hipSuccess;
    if (x.n && (e = hipMemsetAsync(a.mark, 0, x.n, s)) != hipSuccess) return e;
    // an empty list has no distinct pairs; its arrays are never read
    if (m_rm) e = aggregate_pairs(a.rm, rm_keys, rm_ids, m_rm, counts, s);
    else e = hipMemsetAsync(a.rm.d_total, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    if (m_in) e = aggregate_pairs(a.in, in_keys, in_ids, m_in, counts, s);
    else e = hipMemsetAsync(a.in.d_total, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    launch_flag(sliced_grid(m_in), s,
                pair_state<true>{x.keys, x.vals, x.dir, x.bits, nparts, part, a.in.t0, a.in.t1, a.in.dpos, m_in,
                                 a.in.dcnt, a.in.drank, a.in.dstate, a.mark},
                a.in.d_total, 0, nullptr, a.entering);
    if (m_rm)
        hipLaunchKernelGGL(k_apply_mark_removals, dim3(flat_grid(m_rm)), dim3(256), 0, s, x.keys, x.vals, x.links, x.dir,
                           x.bits, a.rm.t0, a.rm.t1, a.rm.dpos, a.rm.d_total, m_rm, a.in.t0, a.in.t1, a.in.dpos,
                           a.in.d_total, m_in, a.mark);
    launch_flag(sliced_grid(x.n), s, marked{a.mark}, nullptr, x.n, nullptr, a.leaving);
    return hipGetLastError();
}

hipError_t index_apply_in_place(const oi_view& x, const void* scratch, uint64_t m_rm, uint64_t m_in, uint64_t* links,
                                hipStream_t s) {
    const apply_scratch a = apply_scratch_at(const_cast<void*>(scratch), x.n, m_rm, m_in);
    hipLaunchKernelGGL(k_apply_links_in_place, dim3(flat_grid(m_rm + m_in)), dim3(256), 0, s, x.keys, x.vals, x.dir,
                       x.bits, a.rm.t0, a.rm.t1, a.rm.dpos, a.rm.d_total, m_rm, a.in.t0, a.in.t1, a.in.dpos, a.in.dcnt,
                       a.in.drank, a.in.dstate, a.in.d_total, m_in, a.mark, links);
    return hipGetLastError();
}

hipError_t index_apply_merge(const oi_view& x, const void* scratch, uint64_t m_rm, uint64_t m_in, uint64_t r_in,
                             uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, uint64_t* rm_out,
                             hipStream_t s) {
    const apply_scratch a = apply_scratch_at(const_cast<void*>(scratch), x.n, m_rm, m_in);
    if (r_in)
        launch_compact(sliced_grid(m_in), s,
                       enter_out<true>{a.in.t0, a.in.t1, a.in.dcnt, a.in.drank, a.in.dstate, a.in.sk, a.in.sv, a.in.nl,
                                       a.nrank},
                       a.in.d_total, 0, a.entering, nullptr);
    const apply_links after{a.rm.t0, a.rm.t1, a.rm.dpos, a.rm.d_total, m_rm,
                            a.in.t0, a.in.t1, a.in.dpos, a.in.d_total, m_in};
    hipLaunchKernelGGL(k_apply_merge<apply_links>, dim3(sliced_grid(x.n)), dim3(256), 0, s, x.keys, x.vals, x.links, x.n,
                       a.mark, a.leaving, after, a.in.sk, a.in.sv, a.in.nl, a.nrank, nullptr, r_in, out_keys, out_vals,
                       out_links, rm_out);
    return hipGetLastError();
}

// ---- merge Objects.  scratch: mark[n] (u8); the per-slice counts of contradictions, of leaving
// entries and of entering pairs (BLOCKS u64 each; the first two side by side for the host's one
// copy); the sorted map sf[m], st[m] and its sort's temporary storage.  Behind that, sized once
// the host knows the leaving entries L: nine u64 arrays of L that the passes hand on to each other
// (merge_rows below), heads[L] and dstate[L] (u8), the coalesced and the entering count (u64, 256
// bytes apart), then the temporary storage of the sorts and the scan.
namespace {
struct merge_scratch {
    uint8_t* mark;
    uint64_t *contra, *leaving, *entering, *sf, *st;
    void* map_tmp;
    uint8_t* rows;
};

size_t merge_flag_bytes(uint64_t n, uint64_t m) {
    return round256(n) + 3 * BLOCKS * sizeof(uint64_t) + 2 * round256(m * sizeof(uint64_t)) + sort_pairs_bytes(m, nullptr) +
           256;
}

merge_scratch merge_scratch_at(void* base, uint64_t n, uint64_t m) {
    merge_scratch q;
    uint8_t* p = reinterpret_cast<uint8_t*>(base);
    q.mark = p;
    p += round256(n);
    q.contra = reinterpret_cast<uint64_t*>(p);
    q.leaving = q.contra + BLOCKS, q.entering = q.contra + 2 * BLOCKS;
    p += 3 * BLOCKS * sizeof(uint64_t);
    q.sf = reinterpret_cast<uint64_t*>(p);
    q.st = reinterpret_cast<uint64_t*>(p + round256(m * sizeof(uint64_t)));
    q.map_tmp = p + 2 * round256(m * sizeof(uint64_t));
    q.rows = reinterpret_cast<uint8_t*>(base) + merge_flag_bytes(n, m);
    return q;
}

size_t scan_bytes(uint64_t m) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (rocprim::inclusive_scan(nullptr, b, nul, nul, (size_t)m, rocprim::plus<uint64_t>(), nullptr) != hipSuccess) return 0;
    return round256(b);
}

// The arrays of L rows, by the pass that writes them; a later pass takes over an array whose
// last reader ran before it:
//   compaction   rk, rv, rl     the leaving entries' (key, phi(id), links), in entry order
//   sort by id   p0 -> p1       positions 0 .. L in phi(id) order (the sorted ids go to sk, unread)
//   sort by key  gk = rk[p1], p1 -> sk, p2     the rows' keys and positions in (key, id) order
//   gather       sv = rv[p2], sl = rl[p2]; scan sl -> pre
//   heads        dk, dv, dpos   the coalesced pairs and their runs' first rows (over rk, rv, rl)
//   state        dcnt, drank    (over p2, sl)
//   entering     nk, nv, nl, nrank   (over sv, sk, pre; nrank its own)
struct merge_rows {
    uint64_t *rk, *rv, *rl, *p0, *p1, *gk, *sk, *p2, *sv, *sl, *pre, *dk, *dv, *dpos, *dcnt, *drank, *nk, *nv, *nl, *nrank;
    uint64_t *d_total, *r_total;
    uint8_t *heads, *dstate;
    void* tmp;
};

size_t merge_rows_bytes(uint64_t L) {
    return 9 * round256(L * sizeof(uint64_t)) + round256(2 * L) + 512 +
           std::max(sort_pairs_bytes(L, nullptr), scan_bytes(L)) + 256;
}

merge_rows merge_rows_at(uint8_t* base, uint64_t L) {
    merge_rows r;
    uint64_t* a[9];
    for (int k = 0; k < 9; k++) a[k] = reinterpret_cast<uint64_t*>(base + k * round256(L * sizeof(uint64_t)));
    r.rk = a[0], r.rv = a[1], r.rl = a[2], r.p0 = a[3], r.sk = a[4], r.p1 = a[5], r.p2 = a[6], r.pre = a[7];
    r.gk = a[3], r.sv = a[3], r.sl = a[5];
    r.dk = a[0], r.dv = a[1], r.dpos = a[2], r.dcnt = a[6], r.drank = a[5];
    r.nk = a[3], r.nv = a[4], r.nl = a[7], r.nrank = a[8];
    uint8_t* p = base + 9 * round256(L * sizeof(uint64_t));
    r.heads = p, r.dstate = p + L;
    p += round256(2 * L);
    r.d_total = reinterpret_cast<uint64_t*>(p), r.r_total = reinterpret_cast<uint64_t*>(p + 256);
    r.tmp = p + 512;
    return r;
}
}  // namespace

size_t index_relabel_scratch(uint64_t n, uint64_t m, uint64_t leaving) {
    return merge_flag_bytes(n, m) + (leaving ? merge_rows_bytes(leaving) : 0);
}

const uint64_t* index_relabel_counts(const void* scratch, uint64_t n) {
    return reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(scratch) + round256(n));
}

hipError_t index_relabel_flag(const oi_view& x, const uint64_t* from, const uint64_t* to, uint64_t m, void* scratch,
                              hipStream_t s) {
    const merge_scratch q = merge_scratch_at(scratch, x.n, m);
    size_t tb = sort_pairs_bytes(m, s);
    hipError_t e = rocprim::radix_sort_pairs(q.map_tmp, tb, from, q.sf, to, q.st, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    launch_flag(sliced_grid(m), s, map_contradiction{q.sf, q.st}, nullptr, m, nullptr, q.contra);
    if (x.n) launch_flag(sliced_grid(x.n), s, relabelled{x.vals, q.sf, q.st, m}, nullptr, x.n, q.mark, q.leaving);
    return hipGetLastError();
}

hipError_t index_relabel_in_place(const oi_view& x, uint64_t m, const void* scratch, uint64_t* vals, hipStream_t s) {
    const merge_scratch q = merge_scratch_at(const_cast<void*>(scratch), x.n, m);
    hipLaunchKernelGGL(k_relabel_in_place, dim3(flat_grid(x.n)), dim3(256), 0, s, q.mark, q.sf, q.st, m, x.n, vals);
    return hipGetLastError();
}

hipError_t index_relabel_rewrite(const oi_view& x, uint64_t m, uint64_t leaving, void* scratch, uint64_t* counts,
                                 uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, const uint64_t** entered,
                                 hipStream_t s) {
    const merge_scratch q = merge_scratch_at(scratch, x.n, m);
    const uint64_t L = leaving;
    const merge_rows r = merge_rows_at(q.rows, L);
    const uint32_t gn = sliced_grid(x.n), gl = sliced_grid(L);
    const dim3 flat(flat_grid(L)), b(256);
    launch_compact(gn, s, leaving_rows{{q.mark}, x.keys, x.vals, x.links, q.sf, q.st, m, r.rk, r.rv, r.rl}, nullptr, x.n,
                   q.leaving, nullptr);
    // (key, id) order: the positions sorted by phi(id), then, stably, by the key behind them
    hipLaunchKernelGGL(k_iota, flat, b, 0, s, r.p0, L);
    size_t tb = sort_pairs_bytes(L, s);
    hipError_t e = rocprim::radix_sort_pairs(r.tmp, tb, r.rv, r.sk, r.p0, r.p1, (size_t)L, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gather_rows, flat, b, 0, s, r.p1, L, r.rk, r.gk, nullptr, nullptr);
    e = rocprim::radix_sort_pairs(r.tmp, tb, r.gk, r.sk, r.p1, r.p2, (size_t)L, 0, 64, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gather_rows, flat, b, 0, s, r.p2, L, r.rv, r.sv, r.rl, r.sl);
    size_t sb = scan_bytes(L);
    e = rocprim::inclusive_scan(r.tmp, sb, r.sl, r.pre, (size_t)L, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return e;
    launch_flag(gl, s, pair_head{r.sk, r.sv}, nullptr, L, r.heads, counts);
    launch_compact(gl, s, pair_out{{r.heads}, r.sk, r.sv, r.dk, r.dv, r.dpos}, nullptr, L, counts, r.d_total);
    launch_flag(gl, s,
                merged_pair_state{x.keys, x.vals, x.dir, x.bits, r.dk, r.dv, r.dpos, r.pre, L, r.dcnt, r.drank, r.dstate,
                                  q.mark},
                r.d_total, 0, nullptr, q.entering);
    launch_compact(gl, s, enter_out<true>{r.dk, r.dv, r.dcnt, r.drank, r.dstate, r.nk, r.nv, r.nl, r.nrank}, r.d_total, 0,
                   q.entering, r.r_total);
    hipLaunchKernelGGL(k_apply_merge<merge_links>, dim3(gn), b, 0, s, x.keys, x.vals, x.links, x.n, q.mark, q.leaving,
                       merge_links{r.dk, r.dv, r.dcnt, r.d_total}, r.nk, r.nv, r.nl, r.nrank, r.r_total, 0, out_keys,
                       out_vals, out_links, nullptr);
    *entered = r.r_total;
    return hipGetLastError();
}

hipError_t index_links(const oi_view& x, const uint64_t* q_keys, const uint64_t* q_ids, uint64_t m, uint64_t* out,
                       hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_index_links, dim3(flat_grid(m)), dim3(256), 0, s, x.keys, x.vals, x.links, x.dir, x.bits, q_keys,
                       q_ids, m, out);
    return hipGetLastError();
}

// ---- by Object, read-only.  scratch: sid[m], spos[m], u[m], pslot[m], tot[2 * m] (u64),
// flags[m] (u8), the distinct count (u64), the per-slice counts of the two ordered compactions
// (BLOCKS u64: the calls by Object share no count slot with sd_dedup_owners_indexed, which
// uses the index's own), then the radix sort's temporary storage
namespace {
struct objects_scratch {
    uint64_t *sid, *spos, *u, *pslot, *tot, *d_total, *counts;
    uint8_t* flags;
    void* tmp;
};

// the sort of (listed id, position): the ids read through their stride, the positions counted
hipError_t objects_sort(void* tmp, size_t& bytes, const uint64_t* ids, uint64_t stride, uint64_t m, uint64_t* sid,
                        uint64_t* spos, hipStream_t s) {
    const rocprim::counting_iterator<uint64_t> pos(0);
    return rocprim::radix_sort_pairs(tmp, bytes, rocprim::make_transform_iterator(pos, strided_ids{ids, stride}), sid,
                                     pos, spos, (size_t)m, 0, 64, s);
}

size_t objects_sort_bytes(uint64_t m) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (objects_sort(nullptr, b, nul, 1, m, nul, nul, nullptr) != hipSuccess) return 0;
    return round256(b);
}

objects_scratch objects_scratch_at(void* base, uint64_t m) {
    objects_scratch q;
    uint64_t* p = reinterpret_cast<uint64_t*>(base);
    q.sid = p, q.spos = p + m, q.u = p + 2 * m, q.pslot = p + 3 * m, q.tot = p + 4 * m;
    uint8_t* b = reinterpret_cast<uint8_t*>(base) + round256(6 * m * sizeof(uint64_t));
    q.flags = b;
    b += round256(m);
    q.d_total = reinterpret_cast<uint64_t*>(b);
    q.counts = reinterpret_cast<uint64_t*>(b + 256);
    q.tmp = b + 256 + BLOCKS * sizeof(uint64_t);
    return q;
}
}  // namespace

size_t index_objects_scratch(uint64_t m) {
    return round256(6 * m * sizeof(uint64_t)) + round256(m) + 256 + BLOCKS * sizeof(uint64_t) + objects_sort_bytes(m) + 256;
}

// m > 0.  After it tot[2 * slot], tot[2 * slot + 1] hold links and entries of the distinct ids
// (sums), or 0 and entries != 0 (!sums: what the orphans need).  Nothing of the index is written.
hipError_t index_objects_totals(const oi_view& x, const uint64_t* ids, uint64_t stride, uint64_t m, bool sums,
                                void* scratch, hipStream_t s) {
    const objects_scratch q = objects_scratch_at(scratch, m);
    size_t tb = objects_sort_bytes(m);
    hipError_t e = objects_sort(q.tmp, tb, ids, stride, m, q.sid, q.spos, s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(q.tot, 0, 2 * m * sizeof(uint64_t), s)) != hipSuccess) return e;
    const uint32_t g = sliced_grid(m);
    launch_flag(g, s, run_head{q.sid}, nullptr, m, q.flags, q.counts);
    launch_compact(g, s, ids_out{{q.flags}, q.sid, q.spos, q.u, q.pslot}, nullptr, m, q.counts, q.d_total);
    if (x.n) {
        const dim3 ge(sliced_grid(x.n)), b(256);
        if (m <= OI_LDS_IDS) {
            if (sums) hipLaunchKernelGGL((k_object_totals<true, true>), ge, b, 0, s, x.vals, x.links, x.n, q.u, q.d_total, q.tot);
            else hipLaunchKernelGGL((k_object_totals<true, false>), ge, b, 0, s, x.vals, x.links, x.n, q.u, q.d_total, q.tot);
        } else {
            if (sums) hipLaunchKernelGGL((k_object_totals<false, true>), ge, b, 0, s, x.vals, x.links, x.n, q.u, q.d_total, q.tot);
            else hipLaunchKernelGGL((k_object_totals<false, false>), ge, b, 0, s, x.vals, x.links, x.n, q.u, q.d_total, q.tot);
        }
    }
    return hipGetLastError();
}

hipError_t index_objects_scatter(const void* scratch, uint64_t m, uint64_t* links_out, uint64_t* entries_out,
                                 hipStream_t s) {
    const objects_scratch q = objects_scratch_at(const_cast<void*>(scratch), m);
    hipLaunchKernelGGL(k_object_scatter, dim3(flat_grid(m)), dim3(256), 0, s, q.pslot, q.tot, m, links_out, entries_out);
    return hipGetLastError();
}

// the orphans counted per slice in index_objects_counts(scratch, m)[0 .. index_slots(m)),
// then compacted
const uint64_t* index_objects_counts(const void* scratch, uint64_t m) {
    return objects_scratch_at(const_cast<void*>(scratch), m).counts;
}

hipError_t index_orphans_flag(const void* scratch, uint64_t m, hipStream_t s) {
    const objects_scratch q = objects_scratch_at(const_cast<void*>(scratch), m);
    launch_flag(sliced_grid(m), s, unowned{q.tot}, q.d_total, 0, q.flags, q.counts);
    return hipGetLastError();
}

hipError_t index_orphans_compact(const void* scratch, uint64_t m, uint64_t* out, hipStream_t s) {
    const objects_scratch q = objects_scratch_at(const_cast<void*>(scratch), m);
    launch_compact(sliced_grid(m), s, orphans_out{{q.flags}, q.u, out}, q.d_total, 0, q.counts, nullptr);
    return hipGetLastError();
}

// ---- by key, read-only
hipError_t index_key_links(const oi_view& x, const uint64_t* q_keys, uint64_t m, uint64_t* links_out,
                           uint64_t* owners_out, hipStream_t s) {
    if (m == 0 || (!links_out && !owners_out)) return hipSuccess;
    if (x.n == 0) {  // no run to search: every answer is 0
        hipError_t e = links_out ? hipMemsetAsync(links_out, 0, m * sizeof(uint64_t), s) : hipSuccess;
        if (e == hipSuccess && owners_out) e = hipMemsetAsync(owners_out, 0, m * sizeof(uint64_t), s);
        return e;
    }
    const dim3 g(flat_grid(m)), b(256);
    if (links_out) hipLaunchKernelGGL((k_key_links<true>), g, b, 0, s, x.keys, x.links, x.dir, x.bits, q_keys, m, links_out, owners_out);
    else hipLaunchKernelGGL((k_key_links<false>), g, b, 0, s, x.keys, x.links, x.dir, x.bits, q_keys, m, links_out, owners_out);
    return hipGetLastError();
}

// The group calls' scratch for n entries: hpos[n], gl[n] (u64), gflags[n], eflags[n] (u8), the
// group count and the eight stats (u64, 256 bytes apart), the head counts and the selection
// counts per slice (BLOCKS u64 each): 18 B per entry and 17 KiB.
namespace {
struct groups_scratch {
    uint64_t *hpos, *gl, *g_total, *stats, *head_counts, *sel_counts;
    uint8_t *gflags, *eflags;
};

groups_scratch groups_scratch_at(void* base, uint64_t n) {
    groups_scratch q;
    uint64_t* p = reinterpret_cast<uint64_t*>(base);
    q.hpos = p, q.gl = p + n;
    uint8_t* b = reinterpret_cast<uint8_t*>(base) + round256(2 * n * sizeof(uint64_t));
    q.gflags = b, q.eflags = b + round256(n);
    b += 2 * round256(n);
    q.g_total = reinterpret_cast<uint64_t*>(b);
    q.stats = reinterpret_cast<uint64_t*>(b + 256);
    q.head_counts = reinterpret_cast<uint64_t*>(b + 512);
    q.sel_counts = q.head_counts + BLOCKS;
    return q;
}
}  // namespace

size_t index_groups_scratch(uint64_t n) {
    return round256(2 * n * sizeof(uint64_t)) + 2 * round256(n) + 512 + 2 * BLOCKS * sizeof(uint64_t);
}

// n > 0.  After it hpos[g] and gl[g] hold the head position and links of every group g, and
// *g_total the groups.  Nothing of the index is written.
hipError_t index_groups_totals(const oi_view& x, void* scratch, hipStream_t s) {
    const groups_scratch q = groups_scratch_at(scratch, x.n);
    hipError_t e = hipMemsetAsync(q.gl, 0, x.n * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const dim3 g(sliced_grid(x.n)), b(256);
    launch_flag(g.x, s, run_head{x.keys}, nullptr, x.n, nullptr, q.head_counts);
    hipLaunchKernelGGL(k_group_totals, g, b, 0, s, x.keys, x.links, x.n, q.head_counts, q.hpos, q.gl, q.g_total);
    return hipGetLastError();
}

// the qualifying groups, or (entries) the entries of the qualifying groups, counted per slice in
// index_groups_counts(scratch, n)[0 .. index_slots(n))
hipError_t index_groups_flag(const oi_view& x, void* scratch, uint64_t min_links, uint64_t min_owners, bool entries,
                             hipStream_t s) {
    const groups_scratch q = groups_scratch_at(scratch, x.n);
    const dim3 g(sliced_grid(x.n)), b(256);  // groups <= n: the slices past the groups are empty
    launch_flag(g.x, s, group_ok{q.hpos, q.gl, x.n, min_links, min_owners}, q.g_total, 0, q.gflags, q.sel_counts);
    if (entries)
        hipLaunchKernelGGL(k_entry_flag, g, b, 0, s, x.keys, x.n, q.head_counts, q.gflags, q.eflags, q.sel_counts);
    return hipGetLastError();
}

const uint64_t* index_groups_counts(const void* scratch, uint64_t n) {
    return groups_scratch_at(const_cast<void*>(scratch), n).sel_counts;
}

hipError_t index_groups_compact(const oi_view& x, const void* scratch, uint64_t* keys_out, uint64_t* first_out,
                                uint64_t* links_out, uint64_t* owners_out, hipStream_t s) {
    const groups_scratch q = groups_scratch_at(const_cast<void*>(scratch), x.n);
    launch_compact(sliced_grid(x.n), s,
                   group_out{{q.gflags}, x.keys, x.vals, q.hpos, q.gl, x.n, keys_out, first_out, links_out, owners_out},
                   q.g_total, 0, q.sel_counts, nullptr);
    return hipGetLastError();
}

hipError_t index_groups_compact_entries(const oi_view& x, const void* scratch, uint64_t* keys_out, uint64_t* ids_out,
                                        uint64_t* links_out, hipStream_t s) {
    const groups_scratch q = groups_scratch_at(const_cast<void*>(scratch), x.n);
    launch_compact(sliced_grid(x.n), s, entry_out{{q.eflags}, x.keys, x.vals, x.links, keys_out, ids_out, links_out},
                   nullptr, x.n, q.sel_counts, nullptr);
    return hipGetLastError();
}

// the eight stats of sd_object_index_duplicate_stats in index_groups_stats_at(scratch, n)
hipError_t index_groups_stats(const oi_view& x, void* scratch, hipStream_t s) {
    const groups_scratch q = groups_scratch_at(scratch, x.n);
    hipError_t e = hipMemsetAsync(q.stats, 0, 8 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_stats, dim3(sliced_grid(x.n)), dim3(256), 0, s, q.hpos, q.gl, q.g_total, x.n, q.stats);
    return hipGetLastError();
}

const uint64_t* index_groups_stats_at(const void* scratch, uint64_t n) {
    return groups_scratch_at(const_cast<void*>(scratch), n).stats;
}

hipError_t index_build_dir(const uint64_t* keys, uint64_t n, uint32_t bits, uint64_t* dir, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(dir, 0, 2 * sizeof(uint64_t), s);
    hipLaunchKernelGGL(k_index_dir, dim3(flat_grid(n)), dim3(256), 0, s, keys, n, bits, dir);
    return hipGetLastError();
}

}  // namespace sdk
