// object_index_host.cpp -- the GPU-free half of the Object index (include/sd_cas.h): the
// directory-size and growth policies the device path shares, and the sd_cpu_object_index_*
// / sd_cpu_dedup_owners_indexed entry points over host arrays, with the device path's layout
// (object_index.h) and semantics.
//
// Reference: the join of a step's cas_ids against the Objects the library already has
// (core/src/object/file_identifier/mod.rs:168-175) and the link to the first of them
// (:189-225); removal as Objects are deleted (core/src/object/orphan_remover.rs:57-95) and
// files change (location/manager/watcher/utils.rs:410-494).  No HIP: built with g++ under
// the sanitizers too (object_index_selftest.cpp, object_index_remove_selftest.cpp,
// object_index_owners_selftest.cpp, object_index_apply_selftest.cpp,
// object_index_orphans_selftest.cpp, object_index_duplicates_selftest.cpp,
// object_index_merge_selftest.cpp; `make sanitize-object-index-merge`, `make
// sanitize-object-index`, `make sanitize-object-index-remove`, `make
// sanitize-object-index-owners`, `make sanitize-object-index-apply`, `make
// sanitize-object-index-orphans`, `make sanitize-object-index-duplicates`).  The owners mode
// (sd_cpu_object_index_create_ex with SD_OBJECT_INDEX_OWNERS) keeps one entry per (key, Object
// id) with its link count; its rules are those of object_index.h, as the kernels'.
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "object_index.h"
#include "sd_host.h"

uint32_t oi_dir_bits(uint64_t n) {
    const int cap = tuning_get(SD_TUNE_INDEX_DIR_MAX_BITS);  // "index_dir_max_bits" (24)
    const uint32_t most = cap < 0 ? 0u : cap > 24 ? 24u : (uint32_t)cap;
    uint32_t b = 0;
    while (b < most && ((uint64_t)16 << b) <= n) b++;  // 2^b <= n / 8 < 2^(b+1): 8-16 keys per bucket
    return b;
}

uint64_t oi_grow_capacity(uint64_t need, uint64_t cap) {
    if (need <= cap) return cap;
    return std::max<uint64_t>({need, cap + cap / 2, 16});
}

bool oi_key_from_hex(const char* hex16, uint64_t* key) {
    uint64_t k = 0;
    for (int i = 0; i < 16; i++) {
        const char c = hex16[i];
        uint64_t d;
        if (c >= '0' && c <= '9') d = (uint64_t)(c - '0');
        else if (c >= 'a' && c <= 'f') d = (uint64_t)(c - 'a' + 10);
        else return false;
        k = (k << 4) | d;
    }
    *key = k;
    return true;
}

struct sd_cpu_object_index {
    int nparts = 1, part = 0;
    int flags = 0;  // SD_OBJECT_INDEX_OWNERS: one entry per (key, Object id) and links[]
    uint64_t n = 0, cap = 0;
    uint32_t bits = 0;
    std::vector<uint64_t> keys, vals, keys2, vals2;  // two buffers of `cap`, swapped by an insert or a removal
    std::vector<uint64_t> links, links2;             // owners mode: the third array beside them
    bool owners() const { return (flags & SD_OBJECT_INDEX_OWNERS) != 0; }
    std::vector<uint64_t> dir{0, 0};
};

namespace {

// dir[q] = i for q in (prefix(key[i-1]), prefix(key[i])], the tail filled with n (k_index_dir)
void build_dir(sd_cpu_object_index* x) {
    x->bits = oi_dir_bits(x->n);
    const uint64_t nb = 1ull << x->bits;
    x->dir.assign(nb + 1, x->n);
    if (x->n == 0) x->dir[0] = 0;
    for (uint64_t i = 0; i < x->n; i++) {
        const uint64_t first = i == 0 ? 0 : oi_prefix(x->keys[i - 1], x->bits) + 1;
        const uint64_t cur = oi_prefix(x->keys[i], x->bits);
        for (uint64_t q = first; q <= cur; q++) x->dir[q] = i;
    }
}

// The second half of both removals (object_index.cpp finish_remove): the count against
// `capacity` before anything is written, the dropped entries in order into removed_out, the
// survivors in order into the other buffer pair, the swap and the directory.
// Owners mode: links[] travels with the survivors, less asked[i] (the links a removal with ids
// takes; null otherwise); nothing is decremented before the capacity check.
void finish_remove(sd_cpu_object_index* x, const std::vector<uint8_t>& flags, uint64_t* removed_out, uint64_t capacity,
                   uint64_t* removed, const uint64_t* asked = nullptr) {
    const uint64_t r = (uint64_t)std::count(flags.begin(), flags.end(), (uint8_t)1);
    if (removed) *removed = r;
    if (r == 0) {  // no entry leaves: the links asked are taken in place, the rest stands
        if (asked)
            for (uint64_t i = 0; i < x->n; i++) x->links[i] -= asked[i];
        return;
    }
    if (removed_out && capacity < r)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of removed entries");
    uint64_t kept = 0, gone = 0;
    for (uint64_t i = 0; i < x->n; i++) {
        if (!flags[i]) {
            x->keys2[kept] = x->keys[i];
            x->vals2[kept] = x->vals[i];
            if (x->owners()) x->links2[kept] = x->links[i] - (asked ? asked[i] : 0);
            kept++;
        } else {
            if (removed_out) {
                removed_out[2 * gone] = x->keys[i];
                removed_out[2 * gone + 1] = x->vals[i];
            }
            gone++;
        }
    }
    x->keys.swap(x->keys2);
    x->vals.swap(x->vals2);
    x->links.swap(x->links2);
    x->n = kept;
    build_dir(x);
}

// A batch of pairs aggregated (object_index.hip aggregate_pairs): ordered by (key, id), each
// distinct pair once with its multiplicity
struct pair_batch {
    std::vector<uint64_t> k, v, cnt;
};
pair_batch aggregate_pairs(const uint64_t* keys, const uint64_t* ids, uint64_t m) {
    std::vector<uint64_t> pos(m);
    std::iota(pos.begin(), pos.end(), 0);
    std::sort(pos.begin(), pos.end(), [&](uint64_t a, uint64_t b) {
        return keys[a] != keys[b] ? keys[a] < keys[b] : ids[a] < ids[b];
    });
    pair_batch b;
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t k = keys[pos[j]], v = ids[pos[j]];
        if (j && b.k.back() == k && b.v.back() == v) b.cnt.back()++;
        else b.k.push_back(k), b.v.push_back(v), b.cnt.push_back(1);
    }
    return b;
}

void grow(sd_cpu_object_index* x, uint64_t need) {
    const uint64_t cap = oi_grow_capacity(need, x->cap);
    if (cap == x->cap) return;
    x->keys.resize(cap), x->vals.resize(cap), x->keys2.resize(cap), x->vals2.resize(cap);
    if (x->owners()) x->links.resize(cap), x->links2.resize(cap);
    x->cap = cap;
}

// Owners-mode insert: every distinct pair of this shard takes its (key, id) rank; the absent
// ones merge in by rank with their multiplicity as links, the present ones add theirs
void insert_owners(sd_cpu_object_index* x, const uint64_t* keys, const uint64_t* ids, uint64_t m, uint64_t* taken) {
    const pair_batch b = aggregate_pairs(keys, ids, m);
    std::vector<uint64_t> nk, nv, nl, at_old, add;
    for (size_t j = 0; j < b.k.size(); j++) {
        if (oi_dest_of(b.k[j], x->nparts) != (uint32_t)x->part) continue;
        uint64_t at;
        if (oi_find_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, b.k[j], b.v[j], &at))
            at_old.push_back(at), add.push_back(b.cnt[j]);
        else
            nk.push_back(b.k[j]), nv.push_back(b.v[j]), nl.push_back(b.cnt[j]);
    }
    const uint64_t r = nk.size();
    if (taken) *taken = r;
    if (r == 0) {
        for (size_t j = 0; j < at_old.size(); j++) x->links[at_old[j]] += add[j];
        return;
    }
    grow(x, x->n + r);
    for (uint64_t j = 0; j < r; j++) {
        const uint64_t at = j + oi_rank_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, nk[j], nv[j]);
        x->keys2[at] = nk[j], x->vals2[at] = nv[j], x->links2[at] = nl[j];
    }
    for (uint64_t i = 0; i < x->n; i++) {
        const uint64_t at = i + oi_lower_bound_pair(nk.data(), nv.data(), 0, r, x->keys[i], x->vals[i]);
        x->keys2[at] = x->keys[i], x->vals2[at] = x->vals[i], x->links2[at] = x->links[i];
    }
    for (size_t j = 0; j < at_old.size(); j++) {
        const uint64_t i = at_old[j];
        x->links2[i + oi_lower_bound_pair(nk.data(), nv.data(), 0, r, x->keys[i], x->vals[i])] += add[j];
    }
    x->keys.swap(x->keys2);
    x->vals.swap(x->vals2);
    x->links.swap(x->links2);
    x->n += r;
    build_dir(x);
}


// The view by Object of object_index.cpp over host arrays (orphan_remover.rs:57-95): the listed
// ids sorted and made distinct, one pass over the entries from the entry side (oi_object_slot),
// the two totals per distinct id.
struct object_totals {
    std::vector<uint64_t> u, links, entries;
};
object_totals totals_by_object(const sd_cpu_object_index* x, const uint64_t* object_ids, uint64_t id_stride, uint64_t m) {
    if (!x || (m && !object_ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!x->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
    if (id_stride != 1 && id_stride != 2) throw sd_failure(SD_ERR_INVALID, "id_stride is 1 or 2 (u64 units)");
    object_totals t;
    t.u.resize(m);
    for (uint64_t j = 0; j < m; j++) t.u[j] = object_ids[j * id_stride];
    std::sort(t.u.begin(), t.u.end());
    t.u.erase(std::unique(t.u.begin(), t.u.end()), t.u.end());
    t.links.assign(t.u.size(), 0), t.entries.assign(t.u.size(), 0);
    for (uint64_t i = 0; i < x->n; i++) {
        uint64_t slot;
        if (oi_object_slot(t.u.data(), t.u.size(), x->vals[i], &slot)) t.links[slot] += x->links[i], t.entries[slot]++;
    }
    return t;
}

// The groups of an owners-mode index (object_index.h, by key): head[s] = the position of run s's
// first entry, links[s] = links(k); owners = the distance to the next head.
struct groups_of {
    std::vector<uint64_t> head, links;
    uint64_t n = 0;
    explicit groups_of(const sd_cpu_object_index* x) {
        if (!x) throw sd_failure(SD_ERR_INVALID, "null argument");
        if (!x->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
        n = x->n;
        for (uint64_t i = 0; i < n; i++) {
            if (i == 0 || x->keys[i - 1] != x->keys[i]) head.push_back(i), links.push_back(0);
            links.back() += x->links[i];
        }
    }
    uint64_t owners(size_t s) const { return (s + 1 < head.size() ? head[s + 1] : n) - head[s]; }
};
}  // namespace

extern "C" {

int sd_cpu_object_index_create(int nparts, int part, sd_cpu_object_index** out) {
    return sd_cpu_object_index_create_ex(nparts, part, 0, out);
}

int sd_cpu_object_index_create_ex(int nparts, int part, int flags, sd_cpu_object_index** out) {
    SD_GUARD_BEGIN
    if (!out) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (nparts < 1 || nparts > 64 || part < 0 || part >= nparts)
        throw sd_failure(SD_ERR_INVALID, "part / nparts out of range (1..64 parts)");
    if (flags & ~SD_OBJECT_INDEX_OWNERS) throw sd_failure(SD_ERR_INVALID, "unknown flags");
    auto* x = new sd_cpu_object_index();
    x->nparts = nparts;
    x->part = part;
    x->flags = flags;
    *out = x;
    return SD_OK;
    SD_GUARD_END
}

void sd_cpu_object_index_destroy(sd_cpu_object_index* index) { delete index; }

int sd_cpu_object_index_flags(const sd_cpu_object_index* index, int* flags) {
    SD_GUARD_BEGIN
    if (!index || !flags) throw sd_failure(SD_ERR_INVALID, "null argument");
    *flags = index->flags;
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_count(const sd_cpu_object_index* index, uint64_t* n) {
    SD_GUARD_BEGIN
    if (!index || !n) throw sd_failure(SD_ERR_INVALID, "null argument");
    *n = index->n;
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_insert(sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids, uint64_t m,
                               uint64_t* taken) {
    SD_GUARD_BEGIN
    if (!index || (m && (!keys || !object_ids))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (taken) *taken = 0;
    if (m == 0) return SD_OK;
    sd_cpu_object_index* x = index;
    if (x->owners()) {
        insert_owners(x, keys, object_ids, m, taken);
        return SD_OK;
    }
    // keep first: order the pairs by (key, position), keep each key's first pair, drop the
    // other shards' keys and those the index already has
    std::vector<uint64_t> pos(m);
    std::iota(pos.begin(), pos.end(), 0);
    std::stable_sort(pos.begin(), pos.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> nk, nv;
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t k = keys[pos[j]];
        if (j && keys[pos[j - 1]] == k) continue;
        if (oi_dest_of(k, x->nparts) != (uint32_t)x->part) continue;
        uint64_t at;
        if (oi_find(x->keys.data(), x->dir.data(), x->bits, k, &at)) continue;
        nk.push_back(k);
        nv.push_back(object_ids[pos[j]]);
    }
    const uint64_t r = nk.size();
    if (taken) *taken = r;
    if (r == 0) return SD_OK;
    grow(x, x->n + r);
    // merge by rank: a new entry goes to its rank + the old keys below it, an old entry to its
    // position + the new keys below it
    for (uint64_t j = 0; j < r; j++) {
        const uint64_t at = j + oi_rank(x->keys.data(), x->dir.data(), x->bits, nk[j]);
        x->keys2[at] = nk[j];
        x->vals2[at] = nv[j];
    }
    for (uint64_t i = 0; i < x->n; i++) {
        const uint64_t at = i + oi_lower_bound(nk.data(), 0, r, x->keys[i]);
        x->keys2[at] = x->keys[i];
        x->vals2[at] = x->vals[i];
    }
    x->keys.swap(x->keys2);
    x->vals.swap(x->vals2);
    x->n += r;
    build_dir(x);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_remove(sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids, uint64_t m,
                               uint64_t* removed_out, uint64_t capacity, uint64_t* removed) {
    SD_GUARD_BEGIN
    if (!index || (m && !keys)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (removed) *removed = 0;
    sd_cpu_object_index* x = index;
    if (m == 0 || x->n == 0) return SD_OK;
    std::vector<uint8_t> flags(x->n, 0);
    if (x->owners() && object_ids) {  // each pair takes one link; an entry leaves at zero
        const pair_batch b = aggregate_pairs(keys, object_ids, m);
        std::vector<uint64_t> asked(x->n, 0);
        for (size_t j = 0; j < b.k.size(); j++) {
            uint64_t at;
            if (oi_find_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, b.k[j], b.v[j], &at))
                asked[at] = b.cnt[j];
        }
        for (uint64_t i = 0; i < x->n; i++) flags[i] = oi_links_drop(x->links[i], asked[i]) ? 1 : 0;
        finish_remove(x, flags, removed_out, capacity, removed, asked.data());
        return SD_OK;
    }
    if (x->owners()) {  // every entry of each listed key: the entry side searches the sorted keys
        std::vector<uint64_t> sorted(keys, keys + m);
        std::sort(sorted.begin(), sorted.end());
        for (uint64_t i = 0; i < x->n; i++) flags[i] = oi_id_listed(sorted.data(), m, x->keys[i]) ? 1 : 0;
        finish_remove(x, flags, removed_out, capacity, removed);
        return SD_OK;
    }
    for (uint64_t i = 0; i < m; i++) {
        uint64_t at;
        if (oi_remove_hit(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, keys[i],
                          object_ids ? &object_ids[i] : nullptr, &at))
            flags[at] = 1;
    }
    finish_remove(x, flags, removed_out, capacity, removed);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_remove_objects(sd_cpu_object_index* index, const uint64_t* object_ids, uint64_t m,
                                       uint64_t* removed_out, uint64_t capacity, uint64_t* removed) {
    SD_GUARD_BEGIN
    if (!index || (m && !object_ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (removed) *removed = 0;
    sd_cpu_object_index* x = index;
    if (m == 0 || x->n == 0) return SD_OK;
    std::vector<uint64_t> sorted(object_ids, object_ids + m);
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint8_t> flags(x->n);
    for (uint64_t i = 0; i < x->n; i++) flags[i] = oi_id_listed(sorted.data(), m, x->vals[i]) ? 1 : 0;
    finish_remove(x, flags, removed_out, capacity, removed);
    return SD_OK;
    SD_GUARD_END
}

// sd_object_index_apply over host arrays (object_index.cpp): both lists aggregated, asked[] and
// added[] per entry and the entering pairs with their ranks, the counts against `capacity`
// before anything is written, then the links in place or one merge into the other buffers.
int sd_cpu_object_index_apply(sd_cpu_object_index* index, const uint64_t* rm_keys, const uint64_t* rm_ids, uint64_t m_rm,
                              const uint64_t* in_keys, const uint64_t* in_ids, uint64_t m_in, uint64_t* removed_out,
                              uint64_t capacity, uint64_t* removed, uint64_t* taken) {
    SD_GUARD_BEGIN
    if (!index || (m_rm && !rm_keys) || (m_in && (!in_keys || !in_ids)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    if (removed) *removed = 0;
    if (taken) *taken = 0;
    sd_cpu_object_index* x = index;
    if (!x->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
    if (m_rm && !rm_ids)
        throw sd_failure(SD_ERR_INVALID, "apply takes links of (key, id) pairs; every owner of a key: sd_cpu_object_index_remove");
    if (x->n == 0) m_rm = 0;
    if (m_rm == 0 && m_in == 0) return SD_OK;
    const pair_batch rm = aggregate_pairs(rm_keys, rm_ids, m_rm), in = aggregate_pairs(in_keys, in_ids, m_in);
    std::vector<uint64_t> asked(x->n, 0), added(x->n, 0), nk, nv, nl, nrank;
    for (size_t j = 0; j < rm.k.size(); j++) {
        uint64_t at;
        if (oi_find_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, rm.k[j], rm.v[j], &at))
            asked[at] = rm.cnt[j];
    }
    for (size_t j = 0; j < in.k.size(); j++) {
        if (oi_dest_of(in.k[j], x->nparts) != (uint32_t)x->part) continue;
        uint64_t at;
        if (oi_find_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, in.k[j], in.v[j], &at))
            added[at] = in.cnt[j];
        else
            nk.push_back(in.k[j]), nv.push_back(in.v[j]), nl.push_back(in.cnt[j]), nrank.push_back(at);
    }
    uint64_t r_out = 0;
    for (uint64_t i = 0; i < x->n; i++) r_out += oi_links_after(x->links[i], asked[i], added[i]) == 0;
    const uint64_t r_in = nk.size();
    if (removed) *removed = r_out;
    if (removed_out && capacity < r_out)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of removed entries");
    if (taken) *taken = r_in;
    if (r_out == 0 && r_in == 0) {  // keys, values and directory stand
        for (uint64_t i = 0; i < x->n; i++) x->links[i] = oi_links_after(x->links[i], asked[i], added[i]);
        return SD_OK;
    }
    grow(x, x->n - r_out + r_in);
    uint64_t o = 0, gone = 0, j = 0;
    for (uint64_t i = 0; i <= x->n; i++) {
        for (; j < r_in && nrank[j] == i; j++, o++)  // the entering pairs ranked at i go before entry i
            x->keys2[o] = nk[j], x->vals2[o] = nv[j], x->links2[o] = nl[j];
        if (i == x->n) break;
        const uint64_t after = oi_links_after(x->links[i], asked[i], added[i]);
        if (after == 0) {
            if (removed_out) removed_out[2 * gone] = x->keys[i], removed_out[2 * gone + 1] = x->vals[i];
            gone++;
        } else {
            x->keys2[o] = x->keys[i], x->vals2[o] = x->vals[i], x->links2[o] = after;
            o++;
        }
    }
    x->keys.swap(x->keys2);
    x->vals.swap(x->vals2);
    x->links.swap(x->links2);
    x->n = o;
    build_dir(x);
    return SD_OK;
    SD_GUARD_END
}

// sd_object_index_merge_objects over host arrays (object_index.h, merge Objects): the map sorted
// by `from` and refused on a contradiction before the index is read; the entries phi changes
// flagged; their rows (key, phi(id), links) put into (key, id) order and coalesced; a coalesced
// pair that meets an entry that stays adds its sum there, every other one enters at its rank; one
// rewrite into the other buffers, as apply's.
int sd_cpu_object_index_merge_objects(sd_cpu_object_index* index, const uint64_t* from, const uint64_t* to, uint64_t m,
                                      uint64_t* moved, uint64_t* coalesced) {
    SD_GUARD_BEGIN
    if (!index || (m && (!from || !to))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (moved) *moved = 0;
    if (coalesced) *coalesced = 0;
    if (m == 0) return SD_OK;
    sd_cpu_object_index* x = index;
    std::vector<uint64_t> pos(m), sf(m), st(m);
    std::iota(pos.begin(), pos.end(), 0);
    std::sort(pos.begin(), pos.end(), [&](uint64_t a, uint64_t b) { return from[a] < from[b]; });
    for (uint64_t j = 0; j < m; j++) sf[j] = from[pos[j]], st[j] = to[pos[j]];
    for (uint64_t j = 0; j < m; j++)
        if (oi_map_contradicts(sf.data(), st.data(), j))
            throw sd_failure(SD_ERR_INVALID, "merge: one `from` id is sent to two different `to` ids");
    std::vector<uint64_t> at_old;  // the positions of the entries whose id phi changes
    for (uint64_t i = 0; i < x->n; i++)
        if (oi_relabel(sf.data(), st.data(), m, x->vals[i]) != x->vals[i]) at_old.push_back(i);
    const uint64_t r_out = at_old.size();
    if (moved) *moved = r_out;
    if (r_out == 0) return SD_OK;  // nothing is written
    if (!x->owners()) {
        for (uint64_t i : at_old) x->vals[i] = oi_relabel(sf.data(), st.data(), m, x->vals[i]);
        return SD_OK;
    }
    // the leaving entries' rows in (key, phi(id)) order; equal pairs are adjacent and add up
    std::vector<uint64_t> rv(r_out);
    for (uint64_t j = 0; j < r_out; j++) rv[j] = oi_relabel(sf.data(), st.data(), m, x->vals[at_old[j]]);
    std::vector<uint64_t> row(r_out);
    std::iota(row.begin(), row.end(), 0);
    std::sort(row.begin(), row.end(), [&](uint64_t a, uint64_t b) {
        const uint64_t ka = x->keys[at_old[a]], kb = x->keys[at_old[b]];
        return ka != kb ? ka < kb : rv[a] < rv[b];
    });
    std::vector<uint8_t> leaves(x->n, 0);
    for (uint64_t i : at_old) leaves[i] = 1;
    std::vector<uint64_t> gain(x->n, 0), nk, nv, nl, nrank;
    for (uint64_t j = 0; j < r_out;) {
        const uint64_t k = x->keys[at_old[row[j]]], v = rv[row[j]];
        uint64_t sum = 0;
        for (; j < r_out && x->keys[at_old[row[j]]] == k && rv[row[j]] == v; j++) sum += x->links[at_old[row[j]]];
        uint64_t at;
        if (oi_find_pair(x->keys.data(), x->vals.data(), x->dir.data(), x->bits, k, v, &at) && !leaves[at]) gain[at] = sum;
        else nk.push_back(k), nv.push_back(v), nl.push_back(sum), nrank.push_back(at);
    }
    const uint64_t r_in = nk.size();
    if (coalesced) *coalesced = r_out - r_in;
    uint64_t o = 0, j = 0;  // the count cannot grow: the other buffers hold it
    for (uint64_t i = 0; i <= x->n; i++) {
        for (; j < r_in && nrank[j] == i; j++, o++)  // the entering pairs ranked at i go before entry i
            x->keys2[o] = nk[j], x->vals2[o] = nv[j], x->links2[o] = nl[j];
        if (i == x->n || leaves[i]) continue;
        x->keys2[o] = x->keys[i], x->vals2[o] = x->vals[i], x->links2[o] = x->links[i] + gain[i];
        o++;
    }
    x->keys.swap(x->keys2);
    x->vals.swap(x->vals2);
    x->links.swap(x->links2);
    x->n = o;
    build_dir(x);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_lookup(const sd_cpu_object_index* index, const uint64_t* keys, uint64_t m, uint64_t* object_ids,
                               uint8_t* found) {
    SD_GUARD_BEGIN
    if (!index || (m && (!keys || !object_ids || !found))) throw sd_failure(SD_ERR_INVALID, "null argument");
    for (uint64_t i = 0; i < m; i++) {
        uint64_t at;
        const bool f = oi_find(index->keys.data(), index->dir.data(), index->bits, keys[i], &at);
        found[i] = f ? 1 : 0;
        object_ids[i] = f ? index->vals[at] : 0;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_export(const sd_cpu_object_index* index, uint64_t* keys_out, uint64_t* object_ids_out,
                               uint64_t capacity) {
    SD_GUARD_BEGIN
    if (!index || (index->n && (!keys_out || !object_ids_out))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (capacity < index->n) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the index's count");
    if (index->n) {
        memcpy(keys_out, index->keys.data(), index->n * sizeof(uint64_t));
        memcpy(object_ids_out, index->vals.data(), index->n * sizeof(uint64_t));
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_links(const sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids,
                              uint64_t m, uint64_t* links_out) {
    SD_GUARD_BEGIN
    if (!index || (m && (!keys || !object_ids || !links_out))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!index->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
    for (uint64_t i = 0; i < m; i++) {
        uint64_t at;
        links_out[i] = oi_find_pair(index->keys.data(), index->vals.data(), index->dir.data(), index->bits, keys[i],
                                    object_ids[i], &at)
                           ? index->links[at]
                           : 0;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_export_links(const sd_cpu_object_index* index, uint64_t* keys_out, uint64_t* ids_out,
                                     uint64_t* links_out, uint64_t capacity) {
    SD_GUARD_BEGIN
    if (!index) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!index->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
    if (index->n && (!keys_out || !ids_out || !links_out)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (capacity < index->n) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the index's count");
    if (index->n) {
        memcpy(keys_out, index->keys.data(), index->n * sizeof(uint64_t));
        memcpy(ids_out, index->vals.data(), index->n * sizeof(uint64_t));
        memcpy(links_out, index->links.data(), index->n * sizeof(uint64_t));
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_object_links(const sd_cpu_object_index* index, const uint64_t* object_ids, uint64_t id_stride,
                                     uint64_t m, uint64_t* links_out, uint64_t* entries_out) {
    SD_GUARD_BEGIN
    const object_totals t = totals_by_object(index, object_ids, id_stride, m);
    for (uint64_t j = 0; j < m; j++) {
        uint64_t slot = 0;
        (void)oi_object_slot(t.u.data(), t.u.size(), object_ids[j * id_stride], &slot);  // every listed id has one
        if (links_out) links_out[j] = t.links[slot];
        if (entries_out) entries_out[j] = t.entries[slot];
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_orphans(const sd_cpu_object_index* index, const uint64_t* object_ids, uint64_t id_stride,
                                uint64_t m, uint64_t* orphans_out, uint64_t capacity, uint64_t* count) {
    SD_GUARD_BEGIN
    if (count) *count = 0;
    const object_totals t = totals_by_object(index, object_ids, id_stride, m);
    uint64_t r = 0;
    for (size_t s = 0; s < t.u.size(); s++) r += oi_unowned(t.entries[s]);
    if (count) *count = r;
    if (!orphans_out || r == 0) return SD_OK;
    if (capacity < r) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of orphans");
    uint64_t o = 0;
    for (size_t s = 0; s < t.u.size(); s++)
        if (oi_unowned(t.entries[s])) orphans_out[o++] = t.u[s];
    return SD_OK;
    SD_GUARD_END
}

// The view by key of object_index.cpp over host arrays (mod.rs:189-225, :229-333): the runs of
// equal keys walked once (oi_qualifies), key_links through the directory (oi_key_run).
int sd_cpu_object_index_key_links(const sd_cpu_object_index* index, const uint64_t* keys, uint64_t m,
                                  uint64_t* links_out, uint64_t* owners_out) {
    SD_GUARD_BEGIN
    if (!index || (m && !keys)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!index->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
    for (uint64_t j = 0; j < m; j++) {
        uint64_t lo, hi, sum = 0;
        oi_key_run(index->keys.data(), index->dir.data(), index->bits, keys[j], &lo, &hi);
        for (uint64_t i = lo; i < hi; i++) sum += index->links[i];
        if (links_out) links_out[j] = sum;
        if (owners_out) owners_out[j] = hi - lo;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_duplicates(const sd_cpu_object_index* index, uint64_t min_links, uint64_t min_owners,
                                   uint64_t* keys_out, uint64_t* first_out, uint64_t* links_out, uint64_t* owners_out,
                                   uint64_t capacity, uint64_t* count) {
    SD_GUARD_BEGIN
    if (count) *count = 0;
    const groups_of g(index);
    uint64_t r = 0;
    for (size_t s = 0; s < g.head.size(); s++) r += oi_qualifies(g.links[s], g.owners(s), min_links, min_owners);
    if (count) *count = r;
    if ((!keys_out && !first_out && !links_out && !owners_out) || r == 0) return SD_OK;
    if (capacity < r) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of rows");
    uint64_t o = 0;
    for (size_t s = 0; s < g.head.size(); s++) {
        if (!oi_qualifies(g.links[s], g.owners(s), min_links, min_owners)) continue;
        if (keys_out) keys_out[o] = index->keys[g.head[s]];
        if (first_out) first_out[o] = index->vals[g.head[s]];
        if (links_out) links_out[o] = g.links[s];
        if (owners_out) owners_out[o] = g.owners(s);
        o++;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_duplicate_entries(const sd_cpu_object_index* index, uint64_t min_links, uint64_t min_owners,
                                          uint64_t* keys_out, uint64_t* ids_out, uint64_t* links_out,
                                          uint64_t capacity, uint64_t* count) {
    SD_GUARD_BEGIN
    if (count) *count = 0;
    const groups_of g(index);
    uint64_t r = 0;
    for (size_t s = 0; s < g.head.size(); s++)
        if (oi_qualifies(g.links[s], g.owners(s), min_links, min_owners)) r += g.owners(s);
    if (count) *count = r;
    if ((!keys_out && !ids_out && !links_out) || r == 0) return SD_OK;
    if (capacity < r) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of rows");
    uint64_t o = 0;
    for (size_t s = 0; s < g.head.size(); s++) {
        if (!oi_qualifies(g.links[s], g.owners(s), min_links, min_owners)) continue;
        for (uint64_t i = g.head[s]; i < g.head[s] + g.owners(s); i++, o++) {
            if (keys_out) keys_out[o] = index->keys[i];
            if (ids_out) ids_out[o] = index->vals[i];
            if (links_out) links_out[o] = index->links[i];
        }
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_object_index_duplicate_stats(const sd_cpu_object_index* index, uint64_t out[8]) {
    SD_GUARD_BEGIN
    if (!out) throw sd_failure(SD_ERR_INVALID, "null argument");
    const groups_of g(index);
    for (int k = 0; k < 8; k++) out[k] = 0;
    out[0] = g.head.size(), out[1] = index->n;
    for (size_t s = 0; s < g.head.size(); s++) {
        const uint64_t l = g.links[s], o = g.owners(s);
        out[2] += l;
        if (l >= 2) out[3] += 1, out[4] += l;
        if (o >= 2) out[5] += 1, out[6] += o;
        if (l > out[7]) out[7] = l;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_dedup_owners_indexed(const sd_cpu_object_index* index, const uint64_t* records, uint64_t m,
                                const uint64_t* rep, uint64_t chunk_size, uint64_t* owner, uint8_t* existing,
                                uint64_t* new_out, uint64_t* n_new) {
    SD_GUARD_BEGIN
    if (m && (!records || !rep || !owner)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (index && (!n_new || (m && (!existing || !new_out)))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (chunk_size == 0) throw sd_failure(SD_ERR_INVALID, "chunk_size must be positive");
    uint64_t heads = 0;
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t key = records[2 * i], idx = records[2 * i + 1], r = rep[i];
        uint64_t at = 0;
        const bool f = index && oi_find(index->keys.data(), index->dir.data(), index->bits, key, &at);
        owner[i] = f ? index->vals[at] : (idx / chunk_size == r / chunk_size ? idx : r);
        if (!index) continue;
        existing[i] = f ? 1 : 0;
        if (!f && (i == 0 || records[2 * (i - 1)] != key)) {
            new_out[2 * heads] = key;
            new_out[2 * heads + 1] = idx;
            heads++;
        }
    }
    if (index) *n_new = heads;
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
