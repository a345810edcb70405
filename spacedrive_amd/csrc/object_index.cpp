// object_index.cpp -- the device-resident Object index behind the C ABI (include/sd_cas.h):
// which Object already owns a cas_id, the join identifier_job_step does per 100-row step
// through the DB (core/src/object/file_identifier/mod.rs:168-175) before it links each file
// to the first such Object (:189-225), and the removals that keep it true while Objects are
// deleted (core/src/object/orphan_remover.rs:57-95) and files change
// (location/manager/watcher/utils.rs:410-494), in the owners mode also both at once
// (sd_object_index_apply), and that mode's read-only view by Object, which answers the orphan
// remover's own query (sd_object_index_object_links, sd_object_index_orphans), and its view by
// key, the duplicate groups per cas_id (sd_object_index_key_links, _duplicates,
// _duplicate_entries, _duplicate_stats), and the call that acts on that view's answer
// (sd_object_index_merge_objects).  Kernels:
// object_index.hip; layout, lookup,
// the removal rules and the directory / growth policies: object_index.h,
// object_index_host.cpp (shared with the sd_cpu_object_index_* mirror).
#include <vector>

#include "object_index.h"
#include "sd_api_impl.h"

namespace {

void check_index(const sd_cas_ctx* ctx, const sd_object_index* index) {
    if (index->ctx != ctx) throw sd_failure(SD_ERR_INVALID, "the index belongs to another context");
}

void require_owners(const sd_object_index* index) {
    if (!index->owners()) throw sd_failure(SD_ERR_INVALID, "the index was not created with SD_OBJECT_INDEX_OWNERS");
}

// m cas_ids of 17 bytes each as keys; `what` names the list in the error ("cas_id", ...)
void keys_from_hex(const char* hex17, uint64_t m, const char* what, uint64_t* keys) {
    for (uint64_t i = 0; i < m; i++)
        if (!oi_key_from_hex(hex17 + 17 * i, &keys[i]))
            throw sd_failure(SD_ERR_INVALID, std::string(what) + " " + std::to_string(i) + " is not 16 lower-case hex digits");
}

// the per-slice counts of a flagging pass in one copy and one sync, summed
uint64_t sum_slots(const uint64_t* dev_counts, uint32_t slots, const sdi::PinnedBuf& host_buf, hipStream_t s) {
    HIP_CHECK(hipMemcpyAsync(host_buf.p, dev_counts, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t* c = reinterpret_cast<const uint64_t*>(host_buf.p);
    uint64_t r = 0;
    for (uint32_t k = 0; k < slots; k++) r += c[k];
    return r;
}

// Every rewrite goes into the other buffer pair (triple in the owners mode) and swaps: before
// the kernel, grow_other makes that side hold `cap` entries (grow-only); after it, swap_in waits
// for the kernel (it read the old buffers and the old directory), grows the old side too, swaps,
// and rebuilds the directory for the new count (bits re-chosen; rebuilt even at an unchanged
// count: the keys moved; the directory's buffer never shrinks).
void grow_other(sd_object_index* x, uint64_t cap) {
    const int to = 1 - x->cur;
    x->keys[to].ensure(cap * sizeof(uint64_t));
    x->vals[to].ensure(cap * sizeof(uint64_t));
    if (x->owners()) x->links[to].ensure(cap * sizeof(uint64_t));
}

void swap_in(sd_object_index* x, int to, uint64_t cap, uint64_t n_new, hipStream_t s) {
    HIP_CHECK(hipStreamSynchronize(s));
    x->keys[x->cur].ensure(cap * sizeof(uint64_t));
    x->vals[x->cur].ensure(cap * sizeof(uint64_t));
    if (x->owners()) x->links[x->cur].ensure(cap * sizeof(uint64_t));
    x->cap = cap;
    x->cur = to;
    x->n = n_new;
    x->bits = oi_dir_bits(x->n);
    x->dir.ensure(((1ull << x->bits) + 1) * sizeof(uint64_t));
    HIP_CHECK(sdk::index_build_dir(x->keys[to].as<uint64_t>(), x->n, x->bits, x->dir.as<uint64_t>(), s));
    HIP_CHECK(hipStreamSynchronize(s));
}

// the checks both reads by Object share; the index comes back writable for its scratch alone:
// keys, values, links and directory are only read
sd_object_index* objects_query(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_object_ids,
                               uint64_t id_stride, uint64_t m) {
    if (!ctx || !index || (m && !d_object_ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    require_owners(index);
    if (id_stride != 1 && id_stride != 2) throw sd_failure(SD_ERR_INVALID, "id_stride is 1 or 2 (u64 units)");
    return const_cast<sd_object_index*>(index);
}

// the checks the three group calls share; the index comes back writable for its scratch alone
sd_object_index* groups_query(sd_cas_ctx* ctx, const sd_object_index* index) {
    if (!ctx || !index) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    require_owners(index);
    return const_cast<sd_object_index*>(index);
}

// Both selections after the group totals: flag, the count in one copy and one sync, the capacity
// checked BEFORE anything is written, then the ordered compaction.
template <class Compact>
void groups_select(sd_object_index* x, uint64_t min_links, uint64_t min_owners, bool entries, bool any_output,
                   uint64_t capacity, uint64_t* count, hipStream_t s, Compact compact) {
    if (count) *count = 0;
    if (x->n == 0) return;
    x->scratch.ensure(sdk::index_groups_scratch(x->n));
    const sdk::oi_view v = x->view();
    HIP_CHECK(sdk::index_groups_totals(v, x->scratch.p, s));
    HIP_CHECK(sdk::index_groups_flag(v, x->scratch.p, min_links, min_owners, entries, s));
    x->objects_host.ensure(sdk::OI_COUNT_SLOTS * sizeof(uint64_t));
    const uint64_t r =
        sum_slots(sdk::index_groups_counts(x->scratch.p, x->n), sdk::index_slots(x->n), x->objects_host, s);
    if (r > x->n) throw sd_failure(SD_ERR_INTERNAL, "duplicates: more rows than entries");
    if (count) *count = r;
    if (!any_output || r == 0) return;
    if (capacity < r) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of rows");
    HIP_CHECK(compact(v, x->scratch.p));
    HIP_CHECK(hipStreamSynchronize(s));
}

// The second half of both removals, after the flagging pass: the per-slice counts give the
// number of dropped entries; it is checked against `capacity` BEFORE anything is written, so
// a short d_removed_out leaves the index (and d_removed_out) as they were.  Then the two-way
// compaction into the other buffer pair, the swap, and the directory for the new count.
// Owners mode: the compaction also carries links[], less `asked` (the links a removal with ids
// takes from each entry; null otherwise) for the survivors -- written into the other buffer
// only, after the capacity check, so a refused call leaves every link count as it was.  When no
// entry leaves (the commonest deletion: the pair keeps other links) nothing is compacted: the
// links are taken in place, O(log n) per distinct pair, and capacity cannot be short of 0 rows.
void finish_remove(sd_object_index* x, uint64_t* d_removed_out, uint64_t capacity, uint64_t* removed, hipStream_t s,
                   const uint64_t* asked = nullptr, uint64_t m = 0) {
    const uint64_t r = sum_slots(x->counts.as<uint64_t>(), sdk::index_slots(x->n), x->host, s);
    if (r > x->n) throw sd_failure(SD_ERR_INTERNAL, "remove: more dropped entries than entries");
    if (removed) *removed = r;
    if (r == 0) {  // no entry leaves: keys, values and directory stand; a removal with ids (of m
                   // pairs) takes its links from the index's own array, a pair without an entry none
        if (asked) {
            HIP_CHECK(sdk::index_owners_take_links(x->view(), x->scratch.p, m, x->links[x->cur].as<uint64_t>(), s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        return;
    }
    if (d_removed_out && capacity < r)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of removed entries");
    const int to = 1 - x->cur;  // both pairs hold `cap` entries since the insert that grew them
    if (x->owners())
        HIP_CHECK(sdk::index_owners_remove_compact(x->view(), x->scratch.p, asked, x->counts.as<uint64_t>(),
                                                   x->keys[to].as<uint64_t>(), x->vals[to].as<uint64_t>(),
                                                   x->links[to].as<uint64_t>(), d_removed_out, s));
    else
        HIP_CHECK(sdk::index_remove_compact(x->view(), x->scratch.p, x->counts.as<uint64_t>(),
                                            x->keys[to].as<uint64_t>(), x->vals[to].as<uint64_t>(), d_removed_out, s));
    swap_in(x, to, x->cap, x->n - r, s);
}

// Owners-mode insert: aggregate the batch, select the absent pairs, merge them in by (key, id)
// rank with the links beside keys and values, then add the present pairs' multiplicities to
// their entries (in place when nothing merges).
void insert_owners(sd_object_index* x, const uint64_t* d_keys, const uint64_t* d_object_ids, uint64_t m,
                   uint64_t* taken, hipStream_t s) {
    x->scratch.ensure(sdk::index_owners_insert_scratch(m));
    const uint64_t *nk = nullptr, *nv = nullptr, *nl = nullptr, *d_total = nullptr;
    HIP_CHECK(sdk::index_owners_insert_select(x->view(), x->nparts, x->part, d_keys, d_object_ids, m, x->scratch.p,
                                              x->counts.as<uint64_t>(), &nk, &nv, &nl, &d_total, s));
    HIP_CHECK(hipMemcpyAsync(x->host.p, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t r = *reinterpret_cast<const uint64_t*>(x->host.p);
    if (r > m) throw sd_failure(SD_ERR_INTERNAL, "insert: more new entries than pairs");
    if (taken) *taken = r;
    if (r == 0) {
        if (x->n)
            HIP_CHECK(sdk::index_owners_add_links(x->scratch.p, m, nk, nv, 0, x->links[x->cur].as<uint64_t>(), s));
        HIP_CHECK(hipStreamSynchronize(s));
        return;
    }
    const uint64_t cap = oi_grow_capacity(x->n + r, x->cap);
    const int to = 1 - x->cur;
    grow_other(x, cap);
    HIP_CHECK(sdk::index_owners_merge(x->view(), nk, nv, nl, r, x->keys[to].as<uint64_t>(), x->vals[to].as<uint64_t>(),
                                      x->links[to].as<uint64_t>(), s));
    HIP_CHECK(sdk::index_owners_add_links(x->scratch.p, m, nk, nv, r, x->links[to].as<uint64_t>(), s));
    swap_in(x, to, cap, x->n + r, s);
}

}  // namespace

extern "C" {

int sd_object_index_create(sd_cas_ctx* ctx, int nparts, int part, sd_object_index** out) {
    return sd_object_index_create_ex(ctx, nparts, part, 0, out);
}

int sd_object_index_create_ex(sd_cas_ctx* ctx, int nparts, int part, int flags, sd_object_index** out) {
    SD_GUARD_BEGIN
    if (!ctx || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (nparts < 1 || nparts > 64 || part < 0 || part >= nparts)
        throw sd_failure(SD_ERR_INVALID, "part / nparts out of range (1..64 parts)");
    if (flags & ~SD_OBJECT_INDEX_OWNERS) throw sd_failure(SD_ERR_INVALID, "unknown flags");
    *out = nullptr;
    ctx->bind();
    auto x = std::make_unique<sd_object_index>();
    x->ctx = ctx;
    x->nparts = nparts;
    x->part = part;
    x->flags = flags;
    for (int k = 0; k < 2; k++) {
        x->keys[k].alloc(0);
        x->vals[k].alloc(0);
        if (x->owners()) x->links[k].alloc(0);
    }
    x->dir.alloc(2 * sizeof(uint64_t));
    HIP_CHECK(hipMemset(x->dir.p, 0, 2 * sizeof(uint64_t)));
    x->counts.alloc((sdk::OI_COUNT_SLOTS + 1) * sizeof(uint64_t));  // + sd_cas_dedup_mgpu_indexed's count
    x->host.ensure(sdk::OI_COUNT_SLOTS * sizeof(uint64_t));  // an insert's count; a removal's per-slice counts
    *out = x.release();
    return SD_OK;
    SD_GUARD_END
}

void sd_object_index_destroy(sd_object_index* index) {
    try {
        if (index) (void)hipSetDevice(index->ctx->device);
        delete index;
    } catch (...) {
    }
}

int sd_object_index_flags(const sd_object_index* index, int* flags) {
    SD_GUARD_BEGIN
    if (!index || !flags) throw sd_failure(SD_ERR_INVALID, "null argument");
    *flags = index->flags;
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_count(const sd_object_index* index, uint64_t* n) {
    SD_GUARD_BEGIN
    if (!index || !n) throw sd_failure(SD_ERR_INVALID, "null argument");
    *n = index->n;
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_insert(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_keys,
                           const uint64_t* d_object_ids, uint64_t m, uint64_t* taken, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && (!d_keys || !d_object_ids))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (taken) *taken = 0;
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    sd_object_index* x = index;
    if (x->owners()) {
        insert_owners(x, d_keys, d_object_ids, m, taken, s);
        return SD_OK;
    }
    x->scratch.ensure(sdk::index_insert_scratch(m));
    const uint64_t *nk = nullptr, *nv = nullptr, *d_total = nullptr;
    HIP_CHECK(sdk::index_insert_select(x->view(), x->nparts, x->part, d_keys, d_object_ids, m, x->scratch.p,
                                       x->counts.as<uint64_t>(), &nk, &nv, &d_total, s));
    HIP_CHECK(hipMemcpyAsync(x->host.p, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t r = *reinterpret_cast<const uint64_t*>(x->host.p);
    if (r > m) throw sd_failure(SD_ERR_INTERNAL, "insert: more survivors than pairs");
    if (taken) *taken = r;
    if (r == 0) return SD_OK;
    // merge into the other buffer pair (grown first if short; grow-only), then swap
    const uint64_t cap = oi_grow_capacity(x->n + r, x->cap);
    const int to = 1 - x->cur;
    grow_other(x, cap);
    HIP_CHECK(sdk::index_merge(x->view(), nk, nv, r, x->keys[to].as<uint64_t>(), x->vals[to].as<uint64_t>(), s));
    swap_in(x, to, cap, x->n + r, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_insert_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* hex17, const uint64_t* object_ids,
                               uint64_t m, uint64_t* taken) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && (!hex17 || !object_ids))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (taken) *taken = 0;
    if (m == 0) return SD_OK;
    std::vector<uint64_t> keys(m);
    keys_from_hex(hex17, m, "cas_id", keys.data());
    ctx->bind();
    sdi::DevBuf dk, dv;
    dk.alloc(m * sizeof(uint64_t));
    dv.alloc(m * sizeof(uint64_t));
    HIP_CHECK(hipMemcpy(dk.p, keys.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dv.p, object_ids, m * sizeof(uint64_t), hipMemcpyHostToDevice));
    return sd_object_index_insert(ctx, index, dk.as<uint64_t>(), dv.as<uint64_t>(), m, taken, nullptr);
    SD_GUARD_END
}

int sd_object_index_remove(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_keys,
                           const uint64_t* d_object_ids, uint64_t m, uint64_t* d_removed_out, uint64_t capacity,
                           uint64_t* removed, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && !d_keys)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (removed) *removed = 0;
    sd_object_index* x = index;
    if (m == 0 || x->n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    if (x->owners() && d_object_ids) {  // each pair takes one link; an entry leaves at zero
        x->scratch.ensure(sdk::index_owners_remove_scratch(x->n, m));
        HIP_CHECK(sdk::index_owners_remove_flag_pairs(x->view(), d_keys, d_object_ids, m, x->scratch.p,
                                                      x->counts.as<uint64_t>(), s));
        finish_remove(x, d_removed_out, capacity, removed, s, sdk::index_owners_asked(x->scratch.p, x->n), m);
        return SD_OK;
    }
    if (x->owners()) {  // every entry of each listed key
        x->scratch.ensure(sdk::index_remove_scratch(x->n, m));
        HIP_CHECK(sdk::index_owners_remove_flag_keys(x->view(), d_keys, m, x->scratch.p, x->counts.as<uint64_t>(), s));
        finish_remove(x, d_removed_out, capacity, removed, s);
        return SD_OK;
    }
    x->scratch.ensure(sdk::index_remove_scratch(x->n, 0));
    HIP_CHECK(sdk::index_remove_flag_keys(x->view(), d_keys, d_object_ids, m, x->scratch.p, x->counts.as<uint64_t>(),
                                          s));
    finish_remove(x, d_removed_out, capacity, removed, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_remove_objects(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_object_ids, uint64_t m,
                                   uint64_t* d_removed_out, uint64_t capacity, uint64_t* removed, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && !d_object_ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (removed) *removed = 0;
    sd_object_index* x = index;
    if (m == 0 || x->n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_remove_scratch(x->n, m));
    HIP_CHECK(sdk::index_remove_flag_objects(x->view(), d_object_ids, m, x->scratch.p, x->counts.as<uint64_t>(), s));
    finish_remove(x, d_removed_out, capacity, removed, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_remove_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* hex17, const uint64_t* object_ids,
                               uint64_t m, uint64_t* removed) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && !hex17)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (removed) *removed = 0;
    if (m == 0) return SD_OK;
    std::vector<uint64_t> keys(m);
    keys_from_hex(hex17, m, "cas_id", keys.data());
    ctx->bind();
    sdi::DevBuf dk, dv;
    dk.alloc(m * sizeof(uint64_t));
    HIP_CHECK(hipMemcpy(dk.p, keys.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (object_ids) {
        dv.alloc(m * sizeof(uint64_t));
        HIP_CHECK(hipMemcpy(dv.p, object_ids, m * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    return sd_object_index_remove(ctx, index, dk.as<uint64_t>(), object_ids ? dv.as<uint64_t>() : nullptr, m, nullptr,
                                  0, removed, nullptr);
    SD_GUARD_END
}

// Removals, then insertions, of an owners-mode index in one call (object_index.h
// oi_links_after): both lists aggregated and every entry and pair classed (nothing of the index
// written); the per-slice counts of leaving entries and entering pairs in one copy and one
// sync; `capacity` checked; then either the links in place (nothing leaves or enters) or ONE
// merge-compaction into the other buffer triple, the swap and the directory.
int sd_object_index_apply(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_rm_keys, const uint64_t* d_rm_ids,
                          uint64_t m_rm, const uint64_t* d_in_keys, const uint64_t* d_in_ids, uint64_t m_in,
                          uint64_t* d_removed_out, uint64_t capacity, uint64_t* removed, uint64_t* taken,
                          void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m_rm && !d_rm_keys) || (m_in && (!d_in_keys || !d_in_ids)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (removed) *removed = 0;
    if (taken) *taken = 0;
    sd_object_index* x = index;
    require_owners(x);
    if (m_rm && !d_rm_ids)
        throw sd_failure(SD_ERR_INVALID, "apply takes links of (key, id) pairs; every owner of a key: sd_object_index_remove");
    if (x->n == 0) m_rm = 0;  // nothing to take from
    if (m_rm == 0 && m_in == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_apply_scratch(x->n, m_rm, m_in));
    HIP_CHECK(sdk::index_apply_flag(x->view(), x->nparts, x->part, d_rm_keys, d_rm_ids, m_rm, d_in_keys, d_in_ids, m_in,
                                    x->scratch.p, x->counts.as<uint64_t>(), s));
    const uint32_t slots_out = sdk::index_slots(x->n), slots_in = sdk::index_slots(m_in);
    x->host.ensure(2 * sdk::OI_COUNT_SLOTS * sizeof(uint64_t));
    HIP_CHECK(hipMemcpyAsync(x->host.p, sdk::index_apply_counts(x->scratch.p, x->n),
                             (slots_out + slots_in) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t* c = reinterpret_cast<const uint64_t*>(x->host.p);
    uint64_t r_out = 0, r_in = 0;
    for (uint32_t k = 0; k < slots_out; k++) r_out += c[k];
    for (uint32_t k = 0; k < slots_in; k++) r_in += c[slots_out + k];
    if (r_out > x->n || r_in > m_in) throw sd_failure(SD_ERR_INTERNAL, "apply: more leaving or entering than there are");
    if (removed) *removed = r_out;
    if (d_removed_out && capacity < r_out)
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of removed entries");
    if (taken) *taken = r_in;
    if (r_out == 0 && r_in == 0) {  // keys, values and directory stand
        HIP_CHECK(sdk::index_apply_in_place(x->view(), x->scratch.p, m_rm, m_in, x->links[x->cur].as<uint64_t>(), s));
        HIP_CHECK(hipStreamSynchronize(s));
        return SD_OK;
    }
    const uint64_t n_new = x->n - r_out + r_in;
    const uint64_t cap = oi_grow_capacity(n_new, x->cap);
    const int to = 1 - x->cur;
    grow_other(x, cap);
    HIP_CHECK(sdk::index_apply_merge(x->view(), x->scratch.p, m_rm, m_in, r_in, x->keys[to].as<uint64_t>(),
                                     x->vals[to].as<uint64_t>(), x->links[to].as<uint64_t>(), d_removed_out, s));
    swap_in(x, to, cap, n_new, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_apply_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* rm_hex17, const uint64_t* rm_ids,
                              uint64_t m_rm, const char* in_hex17, const uint64_t* in_ids, uint64_t m_in,
                              uint64_t* removed, uint64_t* taken) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m_rm && !rm_hex17) || (m_in && (!in_hex17 || !in_ids)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (removed) *removed = 0;
    if (taken) *taken = 0;
    require_owners(index);
    if (m_rm && !rm_ids)
        throw sd_failure(SD_ERR_INVALID, "apply takes links of (key, id) pairs; every owner of a key: sd_object_index_remove_hex");
    if (m_rm == 0 && m_in == 0) return SD_OK;
    // both lists are parsed before anything is uploaded: a malformed cas_id changes nothing
    std::vector<uint64_t> host(2 * (m_rm + m_in));
    uint64_t *rk = host.data(), *rv = rk + m_rm, *ik = rv + m_rm, *iv = ik + m_in;
    keys_from_hex(rm_hex17, m_rm, "removed cas_id", rk);
    keys_from_hex(in_hex17, m_in, "inserted cas_id", ik);
    for (uint64_t i = 0; i < m_rm; i++) rv[i] = rm_ids[i];
    for (uint64_t i = 0; i < m_in; i++) iv[i] = in_ids[i];
    ctx->bind();
    sdi::DevBuf d;
    d.alloc(host.size() * sizeof(uint64_t));
    HIP_CHECK(hipMemcpy(d.p, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    uint64_t* p = d.as<uint64_t>();
    return sd_object_index_apply(ctx, index, p, p + m_rm, m_rm, p + 2 * m_rm, p + 2 * m_rm + m_in, m_in, nullptr, 0,
                                 removed, taken, nullptr);
    SD_GUARD_END
}

// Object `from` is Object `to` (object_index.h, merge Objects): the map sorted and every entry
// whose id changes marked (nothing of the index written); the per-slice counts of contradictions
// and of leaving entries in one copy and one sync -- the only wait before the rewrite; then the
// ids in place (first mode) or the leaving entries' rows coalesced and ONE merge-compaction into
// the other buffer triple, the swap and the directory, as apply's.  The count cannot grow, so
// both triples hold it; the entering pairs are counted on the device and read once the rewrite
// is queued.
int sd_object_index_merge_objects(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_from,
                                  const uint64_t* d_to, uint64_t m, uint64_t* moved, uint64_t* coalesced,
                                  void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && (!d_from || !d_to))) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (moved) *moved = 0;
    if (coalesced) *coalesced = 0;
    if (m == 0) return SD_OK;
    sd_object_index* x = index;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_relabel_scratch(x->n, m, 0));
    HIP_CHECK(sdk::index_relabel_flag(x->view(), d_from, d_to, m, x->scratch.p, s));
    const uint32_t slots_map = sdk::index_slots(m), slots_out = x->n ? sdk::index_slots(x->n) : 0;
    x->host.ensure(2 * sdk::OI_COUNT_SLOTS * sizeof(uint64_t));
    HIP_CHECK(hipMemcpyAsync(x->host.p, sdk::index_relabel_counts(x->scratch.p, x->n),
                             (sdk::OI_COUNT_SLOTS + slots_out) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t* c = reinterpret_cast<const uint64_t*>(x->host.p);
    uint64_t contradictions = 0, r_out = 0;
    for (uint32_t k = 0; k < slots_map; k++) contradictions += c[k];
    for (uint32_t k = 0; k < slots_out; k++) r_out += c[sdk::OI_COUNT_SLOTS + k];
    if (contradictions) throw sd_failure(SD_ERR_INVALID, "merge: one `from` id is sent to two different `to` ids");
    if (r_out > x->n) throw sd_failure(SD_ERR_INTERNAL, "merge: more leaving entries than entries");
    if (moved) *moved = r_out;
    if (r_out == 0) return SD_OK;  // nothing is written
    if (!x->owners()) {
        HIP_CHECK(sdk::index_relabel_in_place(x->view(), m, x->scratch.p, x->vals[x->cur].as<uint64_t>(), s));
        HIP_CHECK(hipStreamSynchronize(s));
        return SD_OK;
    }
    x->scratch.grow_preserve(sdk::index_relabel_scratch(x->n, m, r_out));  // the stream is idle: the marks stay
    const int to = 1 - x->cur;  // both triples hold `cap` entries since the insert that grew them
    const uint64_t* d_entered = nullptr;
    HIP_CHECK(sdk::index_relabel_rewrite(x->view(), m, r_out, x->scratch.p, x->counts.as<uint64_t>(),
                                         x->keys[to].as<uint64_t>(), x->vals[to].as<uint64_t>(),
                                         x->links[to].as<uint64_t>(), &d_entered, s));
    HIP_CHECK(hipMemcpyAsync(x->host.p, d_entered, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t r_in = *reinterpret_cast<const uint64_t*>(x->host.p);
    if (r_in > r_out) throw sd_failure(SD_ERR_INTERNAL, "merge: more entering pairs than leaving entries");
    if (coalesced) *coalesced = r_out - r_in;
    swap_in(x, to, x->cap, x->n - r_out + r_in, s);
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_lookup(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys, uint64_t m,
                           uint64_t* d_object_ids, uint8_t* d_found, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && (!d_keys || !d_object_ids || !d_found)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (m == 0) return SD_OK;
    ctx->bind();
    HIP_CHECK(sdk::index_lookup(index->view(), d_keys, m, d_object_ids, d_found, ctx->pick(stream)));
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_export(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t* d_keys_out,
                           uint64_t* d_object_ids_out, uint64_t capacity, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (index->n && (!d_keys_out || !d_object_ids_out)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    if (capacity < index->n) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the index's count");
    if (index->n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    const sdk::oi_view v = index->view();
    HIP_CHECK(hipMemcpyAsync(d_keys_out, v.keys, v.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_object_ids_out, v.vals, v.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys,
                          const uint64_t* d_object_ids, uint64_t m, uint64_t* d_links_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && (!d_keys || !d_object_ids || !d_links_out)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    require_owners(index);
    if (m == 0) return SD_OK;
    ctx->bind();
    HIP_CHECK(sdk::index_links(index->view(), d_keys, d_object_ids, m, d_links_out, ctx->pick(stream)));
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_export_links(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t* d_keys_out,
                                 uint64_t* d_ids_out, uint64_t* d_links_out, uint64_t capacity, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    require_owners(index);
    if (index->n && (!d_keys_out || !d_ids_out || !d_links_out)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (capacity < index->n) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the index's count");
    if (index->n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    const sdk::oi_view v = index->view();
    HIP_CHECK(hipMemcpyAsync(d_keys_out, v.keys, v.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ids_out, v.vals, v.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_links_out, v.links, v.n * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    return SD_OK;
    SD_GUARD_END
}

// The view by Object of an owners-mode index (object_index.h oi_object_slot / oi_unowned): what
// the orphan remover asks the DB with `object().find_many(file_paths::none)` per 512 Objects
// (core/src/object/orphan_remover.rs:57-95).  The entries are only read; the sorted ids and the
// totals, the per-slice counts and the host's copy of them are the index's own but belong to these
// two calls alone (not `counts` and `host`, which sd_dedup_owners_indexed and
// sd_cas_dedup_mgpu_indexed use): they may run beside every other read, and one at a time.
int sd_object_index_object_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_object_ids,
                                 uint64_t id_stride, uint64_t m, uint64_t* d_links_out, uint64_t* d_entries_out,
                                 void* stream) {
    SD_GUARD_BEGIN
    sd_object_index* x = objects_query(ctx, index, d_object_ids, id_stride, m);
    if (m == 0 || (!d_links_out && !d_entries_out)) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_objects_scratch(m));
    HIP_CHECK(sdk::index_objects_totals(x->view(), d_object_ids, id_stride, m, true, x->scratch.p, s));
    HIP_CHECK(sdk::index_objects_scatter(x->scratch.p, m, d_links_out, d_entries_out, s));
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_orphans(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_object_ids,
                            uint64_t id_stride, uint64_t m, uint64_t* d_orphans_out, uint64_t capacity,
                            uint64_t* count, void* stream) {
    SD_GUARD_BEGIN
    sd_object_index* x = objects_query(ctx, index, d_object_ids, id_stride, m);
    if (count) *count = 0;
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_objects_scratch(m));
    HIP_CHECK(sdk::index_objects_totals(x->view(), d_object_ids, id_stride, m, false, x->scratch.p, s));
    HIP_CHECK(sdk::index_orphans_flag(x->scratch.p, m, s));
    // the count in one copy and one sync, checked against `capacity` before anything is written
    x->objects_host.ensure(sdk::OI_COUNT_SLOTS * sizeof(uint64_t));
    const uint64_t r = sum_slots(sdk::index_objects_counts(x->scratch.p, m), sdk::index_slots(m), x->objects_host, s);
    if (r > m) throw sd_failure(SD_ERR_INTERNAL, "orphans: more orphans than listed ids");
    if (count) *count = r;
    if (!d_orphans_out || r == 0) return SD_OK;
    if (capacity < r) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of orphans");
    HIP_CHECK(sdk::index_orphans_compact(x->scratch.p, m, d_orphans_out, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return SD_OK;
    SD_GUARD_END
}

// The view by key of an owners-mode index (object_index.h oi_key_run / oi_qualifies): which
// content exists more than once (later duplicates link to an Object, mod.rs:189-225) and which is
// split over several Objects (same-step duplicates, mod.rs:229-333).  key_links is a plain read.
// The three group calls keep the group totals, flags and per-slice counts in the index's scratch
// and use the by-Object calls' host buffer: ONE call by Object or of this view per index.
int sd_object_index_key_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys, uint64_t m,
                              uint64_t* d_links_out, uint64_t* d_owners_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !index || (m && !d_keys)) throw sd_failure(SD_ERR_INVALID, "null argument");
    check_index(ctx, index);
    require_owners(index);
    if (m == 0) return SD_OK;
    ctx->bind();
    HIP_CHECK(sdk::index_key_links(index->view(), d_keys, m, d_links_out, d_owners_out, ctx->pick(stream)));
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_duplicates(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t min_links, uint64_t min_owners,
                               uint64_t* d_keys_out, uint64_t* d_first_out, uint64_t* d_links_out,
                               uint64_t* d_owners_out, uint64_t capacity, uint64_t* count, void* stream) {
    SD_GUARD_BEGIN
    sd_object_index* x = groups_query(ctx, index);
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    groups_select(x, min_links, min_owners, false, d_keys_out || d_first_out || d_links_out || d_owners_out, capacity,
                  count, s, [&](const sdk::oi_view& v, const void* scratch) {
                      return sdk::index_groups_compact(v, scratch, d_keys_out, d_first_out, d_links_out, d_owners_out, s);
                  });
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_duplicate_entries(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t min_links,
                                      uint64_t min_owners, uint64_t* d_keys_out, uint64_t* d_ids_out,
                                      uint64_t* d_links_out, uint64_t capacity, uint64_t* count, void* stream) {
    SD_GUARD_BEGIN
    sd_object_index* x = groups_query(ctx, index);
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    groups_select(x, min_links, min_owners, true, d_keys_out || d_ids_out || d_links_out, capacity, count, s,
                  [&](const sdk::oi_view& v, const void* scratch) {
                      return sdk::index_groups_compact_entries(v, scratch, d_keys_out, d_ids_out, d_links_out, s);
                  });
    return SD_OK;
    SD_GUARD_END
}

int sd_object_index_duplicate_stats(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t out[8], void* stream) {
    SD_GUARD_BEGIN
    if (!out) throw sd_failure(SD_ERR_INVALID, "null argument");
    sd_object_index* x = groups_query(ctx, index);
    for (int k = 0; k < 8; k++) out[k] = 0;
    if (x->n == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    x->scratch.ensure(sdk::index_groups_scratch(x->n));
    const sdk::oi_view v = x->view();
    HIP_CHECK(sdk::index_groups_totals(v, x->scratch.p, s));
    HIP_CHECK(sdk::index_groups_stats(v, x->scratch.p, s));
    x->objects_host.ensure(sdk::OI_COUNT_SLOTS * sizeof(uint64_t));
    HIP_CHECK(hipMemcpyAsync(x->objects_host.p, sdk::index_groups_stats_at(x->scratch.p, x->n), 8 * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 8; k++) out[k] = reinterpret_cast<const uint64_t*>(x->objects_host.p)[k];
    return SD_OK;
    SD_GUARD_END
}

int sd_dedup_owners_indexed(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_records, uint64_t m,
                            const uint64_t* d_rep, uint64_t chunk_size, uint64_t* d_owner, uint8_t* d_existing,
                            uint64_t* d_new_out, uint64_t* d_n_new, void* stream) {
    SD_GUARD_BEGIN
    if (!index) return sd_dedup_owners(ctx, d_records, m, d_rep, chunk_size, d_owner, stream);
    if (!ctx || !d_n_new || (m && (!d_records || !d_rep || !d_owner || !d_existing || !d_new_out)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    if (chunk_size == 0) throw sd_failure(SD_ERR_INVALID, "chunk_size must be positive");
    check_index(ctx, index);
    ctx->bind();
    HIP_CHECK(sdk::owners_indexed(index->view(), d_records, m, d_rep, chunk_size, d_owner, d_existing, d_new_out,
                                  d_n_new, index->counts.as<uint64_t>(), ctx->pick(stream)));
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
