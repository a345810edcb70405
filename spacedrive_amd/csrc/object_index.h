// object_index.h -- the Object index's layout and lookup, stated once for the host code
// (object_index_host.cpp, g++) and the kernels (object_index.hip, hipcc).
//
// Reference semantics: identifier_job_step first finds the Objects the library already has
// for a step's cas_ids (core/src/object/file_identifier/mod.rs:168-175) and links each file
// to the first of them (:189-225).  The index is that join's table: keys[n] strictly
// ascending (the big-endian u64 of the cas_id, dedup.hip cas_key; one entry per key -- the
// owners mode below keeps one per (key, Object id) instead), vals[n] the Object ids,
// and a prefix directory dir[2^bits + 1]: dir[p] = the first position whose key's top
// `bits` bits are >= p (dir[2^bits] = n).  cas_ids are uniform hash bits, so a bucket
// [dir[p], dir[p + 1]) holds ~8-16 keys; the search inside it is a binary search bounded by
// the bucket, so keys that all share a prefix cost O(log n), never a scan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SD_OI_HD __host__ __device__ __forceinline__
#else
#define SD_OI_HD inline
#endif

SD_OI_HD uint64_t oi_prefix(uint64_t key, uint32_t bits) { return bits ? key >> (64 - bits) : 0; }

// the rank that owns a key among nparts: its top 16 bits scaled (dedup.hip dest_of, k_part_*)
SD_OI_HD uint32_t oi_dest_of(uint64_t key, int nparts) { return (uint32_t)(((key >> 48) * (uint64_t)nparts) >> 16); }

// first position in [lo, hi) whose key is >= key (hi if none); unsigned comparisons
SD_OI_HD uint64_t oi_lower_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// lower bound of `key` over the whole index through the directory: every key before the
// bucket is smaller and every key after it larger, so the bucket's bound is the global one
SD_OI_HD uint64_t oi_rank(const uint64_t* keys, const uint64_t* dir, uint32_t bits, uint64_t key) {
    const uint64_t p = oi_prefix(key, bits);
    return oi_lower_bound(keys, dir[p], dir[p + 1], key);
}

// position of `key` in the index, or false
SD_OI_HD bool oi_find(const uint64_t* keys, const uint64_t* dir, uint32_t bits, uint64_t key, uint64_t* pos) {
    const uint64_t p = oi_prefix(key, bits);
    const uint64_t hi = dir[p + 1];
    const uint64_t at = oi_lower_bound(keys, dir[p], hi, key);
    *pos = at;
    return at < hi && keys[at] == key;
}

// ---- removal (orphan_remover.rs:57-95; watcher/utils.rs:410-494), stated once for both paths
// By key: the position of the entry a pair (key, *id) removes, or false: the key is in the
// index (keys of other shards never are) and, where an id is given, the entry still names it.
SD_OI_HD bool oi_remove_hit(const uint64_t* keys, const uint64_t* vals, const uint64_t* dir, uint32_t bits,
                            uint64_t key, const uint64_t* id, uint64_t* pos) {
    return oi_find(keys, dir, bits, key, pos) && (!id || vals[*pos] == *id);
}

// By Object: is `id` among the m ids sorted ascending (unsigned)?
SD_OI_HD bool oi_id_listed(const uint64_t* sorted_ids, uint64_t m, uint64_t id) {
    const uint64_t at = oi_lower_bound(sorted_ids, 0, m, id);
    return at < m && sorted_ids[at] == id;
}

// By Object, read-only (owners mode; sd_object_index_object_links, sd_object_index_orphans): the
// orphan remover asks the DB which Objects have no file_path (orphan_remover.rs:57-95).  For an
// Object id o and one index (one shard), ids compared unsigned:
//   entries(o) = the number of entries with vals[i] == o
//   links(o)   = the sum of links[i] over those entries, in u64
//   o is UNOWNED IN THIS SHARD iff entries(o) == 0
// Both paths search the listed ids, sorted and made distinct, from the entry side: the slot of
// vals[i] among them, or false; an entry adds (links[i], 1) to its slot's two totals.
SD_OI_HD bool oi_object_slot(const uint64_t* distinct_ids, uint64_t d, uint64_t id, uint64_t* slot) {
    const uint64_t at = oi_lower_bound(distinct_ids, 0, d, id);
    *slot = at;
    return at < d && distinct_ids[at] == id;
}
SD_OI_HD bool oi_unowned(uint64_t entries) { return entries == 0; }

// ---- owners mode (SD_OBJECT_INDEX_OWNERS), stated once for both paths.  One entry per (key,
// Object id) pair: keys[n] ascending, no longer strictly; vals[n] strictly ascending (unsigned)
// within equal keys; links[n] >= 1, the file_paths that link the pair; the same directory over
// keys.  The FIRST owner of a key is its smallest Object id (mod.rs:168-210: find over a
// find_many in id order), and oi_find returns a lower bound over keys, so it lands on exactly
// that entry: lookup, the indexed owner rule, the new heads, the directory and the multi-GPU
// step serve this mode through the functions above, with no change of rule.  Every entry of a
// key lies in the key's bucket, so the (key, id) bound inside the bucket is the global one and
// a run of thousands of owners costs O(log), never a walk.
// first position in [lo, hi) whose (key, id) is >= (key, id) (hi if none)
SD_OI_HD uint64_t oi_lower_bound_pair(const uint64_t* keys, const uint64_t* vals, uint64_t lo, uint64_t hi,
                                      uint64_t key, uint64_t id) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t k = keys[mid];
        if (k < key || (k == key && vals[mid] < id)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// (key, id) lower bound over the whole index through the directory
SD_OI_HD uint64_t oi_rank_pair(const uint64_t* keys, const uint64_t* vals, const uint64_t* dir, uint32_t bits,
                               uint64_t key, uint64_t id) {
    const uint64_t p = oi_prefix(key, bits);
    return oi_lower_bound_pair(keys, vals, dir[p], dir[p + 1], key, id);
}

// position of the entry (key, id), or false (*pos = its rank either way)
SD_OI_HD bool oi_find_pair(const uint64_t* keys, const uint64_t* vals, const uint64_t* dir, uint32_t bits,
                           uint64_t key, uint64_t id, uint64_t* pos) {
    const uint64_t p = oi_prefix(key, bits);
    const uint64_t hi = dir[p + 1];
    const uint64_t at = oi_lower_bound_pair(keys, vals, dir[p], hi, key, id);
    *pos = at;
    return at < hi && keys[at] == key && vals[at] == id;
}

// removal with ids: an entry asked for at least as many links as it holds is dropped (asking
// for more is not an error); asked 0 = no pair named it
SD_OI_HD bool oi_links_drop(uint64_t held, uint64_t asked) { return asked != 0 && asked >= held; }

// apply (removals, then insertions, in one call): the links of a pair afterwards.  held = its
// links before (0 = absent), asked / added = its multiplicity in the removal / insertion list.
//   kept  = 0 if held == 0 or oi_links_drop(held, asked), else held - asked
//   after = kept + added
// after == 0 with held > 0: the entry leaves; after > 0 with held == 0: the pair enters.  A pair
// whose last link is taken and that gains one in the same call stays, with links = added.
SD_OI_HD uint64_t oi_links_after(uint64_t held, uint64_t asked, uint64_t added) {
    const uint64_t kept = (held == 0 || oi_links_drop(held, asked)) ? 0 : held - asked;
    return kept + added;
}

// ---- by key, read-only (owners mode; sd_object_index_key_links, _duplicates, _duplicate_entries,
// _duplicate_stats): the duplicates the library exists to find -- content that more than one
// file_path has (mod.rs:189-225 links later copies to an existing Object) and content split over
// several Objects (mod.rs:229-333 gives same-step duplicates an Object each).  For one index (one
// shard) and a key k that has at least one entry -- the entries of a key are adjacent:
//   owners(k) = the number of entries with key k
//   links(k)  = the sum of their link counts, in u64
//   first(k)  = the smallest Object id among them: the run's first entry, which lookup answers with
//   k QUALIFIES under (min_links, min_owners) iff links(k) >= min_links and owners(k) >= min_owners;
//   0 means 1 for both, so every key qualifies.
// first position in [lo, hi) whose key is > key (hi if none): the run's end without key + 1,
// since 2^64 - 1 is a legal key
SD_OI_HD uint64_t oi_upper_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the run [*lo, *hi) of `key` (empty if absent): two binary searches inside the key's bucket
SD_OI_HD void oi_key_run(const uint64_t* keys, const uint64_t* dir, uint32_t bits, uint64_t key, uint64_t* lo,
                         uint64_t* hi) {
    const uint64_t p = oi_prefix(key, bits);
    const uint64_t end = dir[p + 1];
    *lo = oi_lower_bound(keys, dir[p], end, key);
    *hi = oi_upper_bound(keys, *lo, end, key);
}

SD_OI_HD bool oi_qualifies(uint64_t links, uint64_t owners, uint64_t min_links, uint64_t min_owners) {
    return links >= (min_links ? min_links : 1) && owners >= (min_owners ? min_owners : 1);
}

// ---- merge Objects (sd_object_index_merge_objects): same-step duplicates each get an Object
// (mod.rs:229-333), so one cas_id is split over several; once the host has decided that Object
// `from` IS Object `to`, the index follows in one call.  The m pairs (from[j], to[j]) -- ids
// compared unsigned, any u64 legal -- define
//   phi(v) = to[j] if some from[j] == v, else v
// applied ONCE and SIMULTANEOUSLY to the ids as they stand before the call: a -> b, b -> c sends
// a's entries to b and b's to c; a -> b, b -> a is a swap (chains are the host's to resolve).
// Repeated pairs, from == to and a `from` the index does not hold are no-ops.  One `from` with two
// different `to` ((a -> a) with (a -> b) is one) is a CONTRADICTION: the call is refused with the
// index untouched.
//   owners mode: after(k, w) = the sum, in u64, of links(k, v) over every v with phi(v) = w; an
//     entry exists iff that sum is >= 1.  Keys never change: entries move inside their key's run,
//     and entries of one key that now share an id coalesce into one.
//   first mode:  vals[i] = phi(vals[i]) in place.
//   moved = the entries, before the call, whose id phi changes; coalesced = the count before less
//   the count after (0 in the first mode).
// Both paths sort the map by `from` (sf[m] with its st[m]) and search an entry's id among sf: a
// lower bound lands on the first row of a run of equal `from`, and without a contradiction every
// row of the run carries the same `to`.
SD_OI_HD bool oi_map_contradicts(const uint64_t* sf, const uint64_t* st, uint64_t i) {
    return i != 0 && sf[i - 1] == sf[i] && st[i - 1] != st[i];
}
SD_OI_HD uint64_t oi_relabel(const uint64_t* sf, const uint64_t* st, uint64_t m, uint64_t id) {
    uint64_t slot;
    return oi_object_slot(sf, m, id, &slot) ? st[slot] : id;
}

// ---- policies (object_index_host.cpp; the device path calls the same functions)
// directory bits for n entries: ~log2(n / 8), 0 for tiny indexes, at most 24
uint32_t oi_dir_bits(uint64_t n);
// grow-only capacity: `cap` while `need` fits, else at least need and 1.5 x cap
uint64_t oi_grow_capacity(uint64_t need, uint64_t cap);
// 16 lower-case hex digits -> the key (false on any other character)
bool oi_key_from_hex(const char* hex16, uint64_t* key);
