// sd_internal.h -- types shared between the host-side C ABI and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sd_cas.h"
#include "sd_host.h"

// the device a context was created on
int sd_ctx_device(const sd_cas_ctx* ctx);
// sd_dedup_group followed by sd_dedup_owners (owner_chunk > 0) with a single host sync
void dedup_group_owners(sd_cas_ctx* ctx, uint64_t* d_records, uint64_t m, int flags, uint64_t* d_rep,
                        uint64_t owner_chunk, uint64_t* d_owner, uint64_t* n_groups, hipStream_t s);
// the block partition of a split-file checksum object
const SplitPlan& sd_split_plan_of(const sd_split_checksum* x);
namespace sdk {
// soff[i] = msg_offset of sampled file i, idx[i] = its index in the batch (the output slot)
// sampled cas (two kernels: lanes of 8 chunks, then the per-file merge) through `rows`
uint64_t cas_sampled_rows_bytes(uint32_t n);
hipError_t launch_cas_sampled(const uint8_t* staged, const uint64_t* soff, const uint32_t* idx, uint32_t n,
                              uint32_t* rows, uint32_t* out, hipStream_t s);
// the same for small batches: one wave per file, 16 + 6 dependent compressions (latency)
hipError_t launch_cas_sampled_wave(const uint8_t* staged, const uint64_t* soff, const uint32_t* idx, uint32_t n,
                                   uint32_t* out, hipStream_t s);
// whole-kind messages of <= 101 chunks, small batches: one workgroup per message (latency);
// rows = (u64 message offset, length, output row)
hipError_t launch_whole_wave(const uint8_t* staged, const uint4* rows, uint32_t n, uint32_t* out, hipStream_t s);
// whole-file work lists: full-pair items, cost-sorted tail items, two merge8 passes (cv2 =
// pass-A output)
hipError_t launch_whole_items(const uint8_t* staged, const uint4* full, uint32_t n_full, const uint4* tail,
                              uint32_t n_tail, const uint4* merge_a, uint32_t n_a, const uint4* merge_b, uint32_t n_b,
                              uint32_t* cvbuf, uint32_t* cv2, uint32_t* out, hipStream_t s);
hipError_t launch_scatter_hash(const uint32_t* src, const uint32_t* idx, uint32_t n, uint32_t* out, hipStream_t s);
hipError_t launch_ck_leaf(const uint8_t* data, uint64_t shift, uint32_t blk_base, const ck_file* files,
                          const uint2* wg_map, uint32_t n_wg, uint32_t* cvbuf, uint32_t* out, hipStream_t s);
// launch_ck_leaf over whole resident messages that also stores every message's level at
// 2^block_log2-byte granularity (17..20): message i's nodes from nodes[8 * node_base[i]], 16-byte aligned
hipError_t launch_ck_leaf_tree(const uint8_t* data, const ck_file* files, const uint2* wg_map, uint32_t n_wg,
                               uint32_t* cvbuf, uint32_t* out, const uint64_t* node_base, uint32_t block_log2,
                               uint32_t* nodes, hipStream_t s);
// the nodes of n_items listed blocks of at most 2^block_log2 bytes (17..20): item i's node to
// nodes[8 * i], or (scatter) to nodes[8 * items[i].dst]; nodes 16-byte aligned
hipError_t launch_ck_blocks(const uint8_t* data, const ck_block_item* items, uint32_t n_items, uint32_t block_log2,
                            bool scatter, uint32_t* nodes, hipStream_t s);
hipError_t launch_ck_reduce(const uint32_t* src, uint32_t* dst, const ck_reduce_wg* wgs, uint32_t n_wg,
                            uint32_t* out, hipStream_t s);
hipError_t launch_synth_stage_cas(const uint64_t* sizes, const uint64_t* cids, const uint32_t* twins,
                                  const sd_extent* ext, uint32_t n, uint8_t* staged, hipStream_t s);
hipError_t launch_synth_fill(uint64_t cid, uint32_t twin, uint64_t offset, uint64_t len, uint8_t* out,
                             hipStream_t s);
// cas messages of the files of a fingerprint batch, from their resident bytes (gather.hip;
// rows / tile_first: sd_host.h GatherPlan)
hipError_t launch_cas_gather(const uint8_t* data, const gather_row* rows, const uint32_t* tile_first,
                             uint64_t total_units, uint8_t* staged, hipStream_t s);
hipError_t launch_read_probe(const uint8_t* buf, uint64_t bytes, int pattern, hipStream_t s);
constexpr uint32_t VALU_PEAK_OPS_PER_ITER = 384;  // k_valu_peak: VALU instructions per wave per iteration
hipError_t launch_valu_peak(uint32_t* sink, uint32_t iters, uint32_t grid, hipStream_t s);
// dedup
// the rest of an exchange row (sd_host.h, SD_EXCHANGE_ROW_EXTRA) behind its nparts counts: with
// `row`, the partition's scan writes counts[nparts .. nparts + 3] = base, n, capacity and the
// valid-record total, or ~0 in its place when bad_index is set
struct part_row {
    uint64_t base, n, capacity;
    uint32_t bad_index;
};
hipError_t dedup_partition(const uint8_t* hash32, const uint8_t* valid, uint64_t n, uint64_t base, int nparts,
                           uint64_t* counts, uint64_t* records, uint64_t* scratch, hipStream_t s,
                           const part_row* row = nullptr);
// device scratch bytes dedup_partition needs; the valid-record total is its last u64
size_t dedup_partition_scratch(int nparts);
hipError_t dedup_group(uint64_t* records, uint64_t m, int flags, uint64_t* rep, uint64_t* n_groups_dev,
                       void* scratch, size_t* scratch_bytes, hipStream_t s);
// bucket grouping (dedup_variant 1): same outputs as dedup_group for m < 2^31 unless
// state[1] (overflow) comes back nonzero -- then records hold a permutation of the input
// and dedup_group (without SD_DEDUP_INDEX_SORTED) must run.  state: 6 device u64, state[0]
// = the group count.
size_t dedup_group_buckets_scratch(uint64_t m);
hipError_t dedup_group_buckets(uint64_t* records, uint64_t m, uint64_t* rep, uint64_t* state, void* scratch,
                               size_t scratch_bytes, hipStream_t s);
hipError_t dedup_owners(const uint64_t* records, uint64_t m, const uint64_t* rep, uint64_t chunk, uint64_t* owner,
                        hipStream_t s);
// sd_dedup_confirm (dedup_confirm.hip), one pass queued on s: the prefix path, or (full) the
// full-width path.  state: DEDUP_CONFIRM_STATE device u64, [0..7] = the stats, [8] = nonzero when
// the prefix path met a (key, h0) run with unequal tails -- then this pass wrote no output and
// the pass with full = true must run.  Every output may be null; m > 0.
constexpr uint32_t DEDUP_CONFIRM_STATE = 16;
size_t dedup_confirm_scratch(uint64_t m);
hipError_t dedup_confirm(const uint64_t* keys, const uint8_t* hash32, const uint8_t* valid, uint64_t m, bool full,
                         uint64_t* rep, uint64_t* class_size, uint8_t* verdict, uint64_t* sets, uint64_t capacity,
                         uint64_t* state, void* scratch, size_t scratch_bytes, hipStream_t s);
// Object index (object_index.hip; layout in object_index.h): the current device arrays
struct oi_view {
    const uint64_t *keys, *vals, *dir;
    uint64_t n;
    uint32_t bits;
    const uint64_t* links = nullptr;  // owners mode only: the link count per entry
};
// u64 per-workgroup counts of an ordered compaction: sliced.h's BLOCKS (a static_assert there; that
// header is device code, this one is also the host sources')
constexpr uint32_t OI_COUNT_SLOTS = 1024;
// the count slots a sliced pass over n positions fills: one per workgroup, at most OI_COUNT_SLOTS
uint32_t index_slots(uint64_t n);
hipError_t index_lookup(const oi_view& x, const uint64_t* q, uint64_t m, uint64_t* out, uint8_t* found,
                        hipStream_t s);
// the indexed owner rule + the compacted new heads (2 x u64 each, ascending key) and their
// count (device u64); counts: OI_COUNT_SLOTS device u64 of scratch
hipError_t owners_indexed(const oi_view& x, const uint64_t* records, uint64_t m, const uint64_t* rep, uint64_t chunk,
                          uint64_t* owner, uint8_t* existing, uint64_t* new_out, uint64_t* n_new, uint64_t* counts,
                          hipStream_t s);
// insert, first half: the pairs that survive (first of their key, this shard's, not in the
// index), sorted by key, left in `scratch` with their count (device u64); m > 0
size_t index_insert_scratch(uint64_t m);
hipError_t index_insert_select(const oi_view& x, int nparts, int part, const uint64_t* in_keys,
                               const uint64_t* in_vals, uint64_t m, void* scratch, uint64_t* counts,
                               const uint64_t** nk_out, const uint64_t** nv_out, const uint64_t** total_out,
                               hipStream_t s);
// second half: merge the r survivors with the index into out_keys / out_vals (n + r entries)
hipError_t index_merge(const oi_view& x, const uint64_t* nk, const uint64_t* nv, uint64_t r, uint64_t* out_keys,
                       uint64_t* out_vals, hipStream_t s);
// removal, first half: flags[n] in `scratch` (1 = the entry goes) and one count per workgroup
// slice in counts[0 .. index_slots(n)); n > 0, m > 0.  By key (rm_ids may be null:
// unconditional) or by Object (m_ids = m sizes the scratch for the sorted ids).
size_t index_remove_scratch(uint64_t n, uint64_t m_ids);
hipError_t index_remove_flag_keys(const oi_view& x, const uint64_t* rm_keys, const uint64_t* rm_ids, uint64_t m,
                                  void* scratch, uint64_t* counts, hipStream_t s);
hipError_t index_remove_flag_objects(const oi_view& x, const uint64_t* ids, uint64_t m, void* scratch,
                                     uint64_t* counts, hipStream_t s);
// second half: the survivors in order into out_keys / out_vals, the dropped entries (key,
// Object id) in order into rm_out (may be null)
hipError_t index_remove_compact(const oi_view& x, const void* scratch, const uint64_t* counts, uint64_t* out_keys,
                                uint64_t* out_vals, uint64_t* rm_out, hipStream_t s);
// ---- owners mode (object_index.h): one entry per (key, Object id) with its link count
// A batch of m pairs aggregated in `scratch`: ordered by (key, id), each distinct pair once
// with its multiplicity.  Insert, first half: the distinct pairs this shard lacks (nk, nv, nl =
// multiplicity) with their count (device u64); the present ones are remembered in `scratch`
// for index_owners_add_links.  m > 0.
size_t index_owners_insert_scratch(uint64_t m);
hipError_t index_owners_insert_select(const oi_view& x, int nparts, int part, const uint64_t* in_keys,
                                      const uint64_t* in_vals, uint64_t m, void* scratch, uint64_t* counts,
                                      const uint64_t** nk_out, const uint64_t** nv_out, const uint64_t** nl_out,
                                      const uint64_t** total_out, hipStream_t s);
// second half: merge the r new entries with the index x into out_* (n + r entries) ...
hipError_t index_owners_merge(const oi_view& x, const uint64_t* nk, const uint64_t* nv, const uint64_t* nl, uint64_t r,
                              uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, hipStream_t s);
// ... and add the present pairs' multiplicities to their entries' links, at their places after
// the merge of r new entries (r == 0: in the index's own array); one writer per entry
hipError_t index_owners_add_links(const void* scratch, uint64_t m, const uint64_t* nk, const uint64_t* nv, uint64_t r,
                                  uint64_t* links, hipStream_t s);
// removal with ids, first half: asked[n] (the links each entry is asked to give up), flags[n]
// and the per-slice counts; n > 0, m > 0.  Nothing of the index is written.
size_t index_owners_remove_scratch(uint64_t n, uint64_t m);
hipError_t index_owners_remove_flag_pairs(const oi_view& x, const uint64_t* rm_keys, const uint64_t* rm_ids,
                                          uint64_t m, void* scratch, uint64_t* counts, hipStream_t s);
// a removal with ids that drops no entry (the counts say so): the links asked leave their
// entries in place, `links` being the index's own array; keys, values and directory stand
hipError_t index_owners_take_links(const oi_view& x, const void* scratch, uint64_t m, uint64_t* links, hipStream_t s);
// removal without ids: every entry whose key is among the m keys (sorted in `scratch`, sized by
// index_remove_scratch(n, m))
hipError_t index_owners_remove_flag_keys(const oi_view& x, const uint64_t* rm_keys, uint64_t m, void* scratch,
                                         uint64_t* counts, hipStream_t s);
// second half of every owners-mode removal: index_remove_compact carrying the links; `asked`
// (null except after index_owners_remove_flag_pairs) is taken from the survivors' links
const uint64_t* index_owners_asked(const void* scratch, uint64_t n);
hipError_t index_owners_remove_compact(const oi_view& x, const void* scratch, const uint64_t* asked,
                                       const uint64_t* counts, uint64_t* out_keys, uint64_t* out_vals,
                                       uint64_t* out_links, uint64_t* rm_out, hipStream_t s);
// apply: a removal list (with ids) and an insertion list in one call (object_index.h
// oi_links_after).  First half: both lists aggregated in `scratch`, every entry marked leaving /
// staying, every distinct pair of the insertion list classed entering / present / another
// shard's; index_apply_counts(scratch, n) then holds the per-slice counts of leaving entries
// (index_slots(n)) followed by those of entering pairs (index_slots(m_in)).  Nothing of the
// index is written.  m_rm + m_in > 0; either may be 0; `counts`: OI_COUNT_SLOTS u64 of scratch.
size_t index_apply_scratch(uint64_t n, uint64_t m_rm, uint64_t m_in);
const uint64_t* index_apply_counts(const void* scratch, uint64_t n);
hipError_t index_apply_flag(const oi_view& x, int nparts, int part, const uint64_t* rm_keys, const uint64_t* rm_ids,
                            uint64_t m_rm, const uint64_t* in_keys, const uint64_t* in_ids, uint64_t m_in,
                            void* scratch, uint64_t* counts, hipStream_t s);
// nothing leaves or enters: the new link counts at their entries, `links` being the index's own
hipError_t index_apply_in_place(const oi_view& x, const void* scratch, uint64_t m_rm, uint64_t m_in, uint64_t* links,
                                hipStream_t s);
// otherwise: the staying entries (with their new links) and the r_in entering pairs merged into
// out_* (n - leaving + r_in entries), the leaving entries in order into rm_out (may be null)
hipError_t index_apply_merge(const oi_view& x, const void* scratch, uint64_t m_rm, uint64_t m_in, uint64_t r_in,
                             uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, uint64_t* rm_out,
                             hipStream_t s);
// merge Objects (object_index.h oi_relabel): relabel the owners by the m pairs (from, to), m > 0.
// First half: the map sorted in `scratch`, every entry whose id changes marked;
// index_relabel_counts(scratch, n) then holds the per-slice counts of contradictions
// (index_slots(m)) and, OI_COUNT_SLOTS further, of leaving entries (index_slots(n); unset when n
// == 0).  Nothing of the index is written.  The scratch is index_relabel_scratch(n, m, 0) bytes
// for the first half and, its contents kept, index_relabel_scratch(n, m, leaving) for the rewrite.
size_t index_relabel_scratch(uint64_t n, uint64_t m, uint64_t leaving);
const uint64_t* index_relabel_counts(const void* scratch, uint64_t n);
hipError_t index_relabel_flag(const oi_view& x, const uint64_t* from, const uint64_t* to, uint64_t m, void* scratch,
                              hipStream_t s);
// first mode: the marked entries' ids in place, `vals` being the index's own
hipError_t index_relabel_in_place(const oi_view& x, uint64_t m, const void* scratch, uint64_t* vals, hipStream_t s);
// owners mode, leaving > 0: the leaving entries' rows coalesced, the staying entries (with the
// links they gain) and the entering pairs merged into out_* (n - leaving + **entered entries;
// *entered is a device count); `counts`: OI_COUNT_SLOTS u64 of scratch
hipError_t index_relabel_rewrite(const oi_view& x, uint64_t m, uint64_t leaving, void* scratch, uint64_t* counts,
                                 uint64_t* out_keys, uint64_t* out_vals, uint64_t* out_links, const uint64_t** entered,
                                 hipStream_t s);
// the link count per (key, id) pair, 0 if absent
hipError_t index_links(const oi_view& x, const uint64_t* q_keys, const uint64_t* q_ids, uint64_t m, uint64_t* out,
                       hipStream_t s);
// By Object, read-only (owners mode; object_index.h oi_object_slot): the m listed ids (element j at
// ids[j * stride]) sorted and made distinct in `scratch` (index_objects_scratch(m) bytes), then
// one pass over the entries that leaves, per distinct id, its links and entries (`sums`) or only
// whether it has an entry (the orphans).  m > 0.  The per-slice counts of their ordered
// compactions live in `scratch` too, not in the index's count slots.
size_t index_objects_scratch(uint64_t m);
hipError_t index_objects_totals(const oi_view& x, const uint64_t* ids, uint64_t stride, uint64_t m, bool sums,
                                void* scratch, hipStream_t s);
// the totals to the m listed positions (either output may be null)
hipError_t index_objects_scatter(const void* scratch, uint64_t m, uint64_t* links_out, uint64_t* entries_out,
                                 hipStream_t s);
// the distinct ids without an entry: counted per slice in index_objects_counts(scratch, m)[0 ..
// index_slots(m)), then written ascending to `out` (as many as the counts add up to)
const uint64_t* index_objects_counts(const void* scratch, uint64_t m);
hipError_t index_orphans_flag(const void* scratch, uint64_t m, hipStream_t s);
hipError_t index_orphans_compact(const void* scratch, uint64_t m, uint64_t* out, hipStream_t s);
// By key, read-only (owners mode; object_index.h oi_key_run / oi_qualifies).  links(k) and
// owners(k) per listed key, 0 and 0 for a key the index does not hold (either output may be
// null); no scratch.
hipError_t index_key_links(const oi_view& x, const uint64_t* q_keys, uint64_t m, uint64_t* links_out,
                           uint64_t* owners_out, hipStream_t s);
// The duplicate groups of an index of n > 0 entries in `scratch` (index_groups_scratch(n) bytes,
// 18 B per entry and 17 KiB): the totals of every run of equal keys; then the qualifying groups
// (or, `entries`, the entries of the qualifying groups) flagged and counted per slice in
// index_groups_counts(scratch, n)[0 .. index_slots(n)); then, once the host has checked
// the count, one row per flagged group / entry in order (every output may be null); or the
// eight stats of sd_object_index_duplicate_stats at index_groups_stats_at(scratch, n).
size_t index_groups_scratch(uint64_t n);
hipError_t index_groups_totals(const oi_view& x, void* scratch, hipStream_t s);
hipError_t index_groups_flag(const oi_view& x, void* scratch, uint64_t min_links, uint64_t min_owners, bool entries,
                             hipStream_t s);
const uint64_t* index_groups_counts(const void* scratch, uint64_t n);
hipError_t index_groups_compact(const oi_view& x, const void* scratch, uint64_t* keys_out, uint64_t* first_out,
                                uint64_t* links_out, uint64_t* owners_out, hipStream_t s);
hipError_t index_groups_compact_entries(const oi_view& x, const void* scratch, uint64_t* keys_out, uint64_t* ids_out,
                                        uint64_t* links_out, hipStream_t s);
hipError_t index_groups_stats(const oi_view& x, void* scratch, hipStream_t s);
const uint64_t* index_groups_stats_at(const void* scratch, uint64_t n);
hipError_t index_build_dir(const uint64_t* keys, uint64_t n, uint32_t bits, uint64_t* dir, hipStream_t s);
}  // namespace sdk
