//! Raw FFI mirror of `include/sd_cas.h` (ABI version 2) plus a small safe layer used by
//! `core/src/object/cas.rs`, `core/src/object/validation/hash.rs`, the batched identifier
//! step (`file_identifier_step.rs`) and the batched validator step (`validator_step.rs`).
//!
//! Conventions follow the reference's own FFI (`apps/mobile/modules/sd-core/ios/crate/
//! src/lib.rs:36-86`): plain pointers and sizes, no panics across the boundary.  Behind
//! the ABI, libsdcas catches every C++ exception and returns a negative `sd_rc`.
//!
//! Routing: with a gfx950 device, batches go to the GPU entry points and single files to
//! `sd_cas_id_path` / `sd_file_checksum_path` (the library's latency policy: CPU while few
//! calls are in flight, coalesced GPU batches beyond).  Without one, [`ctx`] returns an
//! error (it never panics) and every call takes the library's CPU path (`sd_cpu_*`): the
//! same results from the host cores.
#![allow(non_camel_case_types)]
use std::ffi::{CStr, CString};
use std::io;
use std::os::raw::{c_char, c_int, c_void};
use std::os::unix::ffi::OsStrExt;
use std::path::Path;
use std::sync::{Arc, OnceLock};

#[repr(C)]
pub struct sd_cas_ctx {
    _p: [u8; 0],
}

#[repr(C)]
pub struct sd_comm {
    _p: [u8; 0],
}
#[repr(C)]
pub struct sd_comm_group {
    _p: [u8; 0],
}

#[repr(C)]
pub struct sd_split_checksum {
    _p: [u8; 0],
}

#[repr(C)]
pub struct sd_fingerprint_batch {
    _p: [u8; 0],
}
#[repr(C)]
pub struct sd_object_index {
    _p: [u8; 0],
}
#[repr(C)]
pub struct sd_cpu_object_index {
    _p: [u8; 0],
}
#[repr(C)]
pub struct sd_checksum_tree {
    _p: [u8; 0],
}
#[repr(C)]
pub struct sd_checksum_tree_blocks {
    _p: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct sd_extent {
    pub size: u64,
    pub msg_offset: u64,
    pub msg_len: u32,
    pub kind: u32,
}

pub const SD_CAS_ABI_VERSION: c_int = 2;
pub const SD_OK: c_int = 0;
pub const SD_ERR_DEVICE: c_int = -2;
pub const SD_ERR_CAPACITY: c_int = -6;
pub const SD_FILE_OK: i32 = 0;
pub const SD_FILE_SKIPPED_EMPTY: i32 = 1;
pub const SD_FILE_IO_ERROR: i32 = 2;
pub const SD_FILE_SHORT_READ: i32 = 3;
pub const SD_FILE_CHANGED: i32 = 4;
pub const SD_COMM_ID_BYTES: usize = 128;
pub const SD_OBJECT_INDEX_OWNERS: c_int = 1;
// checksum trees: block_log2 of the level (128 KiB .. 1 MiB)
pub const SD_TREE_BLOCK_LOG2_MIN: u32 = 17;
pub const SD_TREE_BLOCK_LOG2_MAX: u32 = 20;
// sd_dedup_confirm's verdict per file
pub const SD_CONFIRM_INVALID: u8 = 0;
pub const SD_CONFIRM_SINGLE: u8 = 1;
pub const SD_CONFIRM_CONFIRMED: u8 = 2;
pub const SD_CONFIRM_REFUTED: u8 = 3;

extern "C" {
    pub fn sd_cas_abi_version() -> c_int;
    pub fn sd_cas_last_error() -> *const c_char;
    // the host thread budget every call is capped by; "host_cpu_budget" sets it
    pub fn sd_host_cpu_budget(out: *mut c_int) -> c_int;
    // where the library's own threads run (the device's NUMA node; tuning "numa_pin")
    pub fn sd_host_numa(out: *mut c_int) -> c_int;
    pub fn sd_cas_set_tuning(key: *const c_char, value: c_int) -> c_int;
    pub fn sd_cas_ctx_create(device: c_int, out: *mut *mut sd_cas_ctx) -> c_int;
    pub fn sd_cas_ctx_destroy(ctx: *mut sd_cas_ctx);
    pub fn sd_cas_stage_plan(sizes: *const u64, n: usize, ext: *mut sd_extent, total: *mut u64) -> c_int;
    pub fn sd_cas_ids_files(ctx: *mut sd_cas_ctx, paths: *const *const c_char, sizes: *const u64, n: usize,
                            out_hex17: *mut c_char, status: *mut i32, nthreads: c_int) -> c_int;
    pub fn sd_cas_hashes_files(ctx: *mut sd_cas_ctx, paths: *const *const c_char, sizes: *const u64, n: usize,
                               d_hash32: *mut u8, d_valid: *mut u8, status: *mut i32, nthreads: c_int) -> c_int;
    pub fn sd_cas_id_path(ctx: *mut sd_cas_ctx, path: *const c_char, size: u64, out_hex17: *mut c_char,
                          status: *mut i32) -> c_int;
    pub fn sd_file_checksums(ctx: *mut sd_cas_ctx, paths: *const *const c_char, n: usize,
                             out_hex65: *mut c_char, status: *mut i32) -> c_int;
    pub fn sd_file_checksum_path(ctx: *mut sd_cas_ctx, path: *const c_char, out_hex65: *mut c_char,
                                 status: *mut i32) -> c_int;
    pub fn sd_checksums(ctx: *mut sd_cas_ctx, data: *const u8, offsets: *const u64, lens: *const u64, n: usize,
                        out_hex65: *mut c_char) -> c_int;
    // the validator's split: bytes the GPU route and the CPU path hashed
    pub fn sd_file_checksums_bytes(ctx: *mut sd_cas_ctx, out: *mut u64) -> c_int;
    // what the context learned for the split vs the CPU path ("checksum_split_adapt")
    pub fn sd_file_checksums_learned(ctx: *mut sd_cas_ctx, out: *mut f64) -> c_int;
    // what the context learned for sd_checksums' co-hashed calls vs the CPU path alone
    pub fn sd_checksums_learned(ctx: *mut sd_cas_ctx, out: *mut f64) -> c_int;
    // fingerprints: cas_id and checksum of resident files from one copy of their bytes
    // (watcher/utils.rs:393,438-446); device-resident batches, the host drop-in, the CPU sibling
    pub fn sd_fingerprint_batch_create(ctx: *mut sd_cas_ctx, offsets: *const u64, lens: *const u64, n: usize,
                                       out: *mut *mut sd_fingerprint_batch) -> c_int;
    pub fn sd_fingerprint_batch_destroy(batch: *mut sd_fingerprint_batch);
    pub fn sd_fingerprint_batch_stats(batch: *const sd_fingerprint_batch, out: *mut u64) -> c_int;
    pub fn sd_fingerprint_batch_extents(batch: *const sd_fingerprint_batch, extents_out: *mut sd_extent) -> c_int;
    pub fn sd_fingerprint_batch_gather(ctx: *mut sd_cas_ctx, batch: *const sd_fingerprint_batch, d_data: *const u8,
                                       d_staged: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_fingerprint_batch_run(ctx: *mut sd_cas_ctx, batch: *const sd_fingerprint_batch, d_data: *const u8,
                                    d_cas_hash32: *mut u8, d_checksum32: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_fingerprints(ctx: *mut sd_cas_ctx, data: *const u8, offsets: *const u64, lens: *const u64, n: usize,
                           out_hex17: *mut c_char, out_hex65: *mut c_char) -> c_int;
    pub fn sd_fingerprints_stats(ctx: *mut sd_cas_ctx, out: *mut u64) -> c_int;
    pub fn sd_cpu_fingerprints(data: *const u8, offsets: *const u64, lens: *const u64, n: usize,
                               out_hex17: *mut c_char, out_hex65: *mut c_char, nthreads: c_int) -> c_int;
    // the CPU path (no device)
    pub fn sd_cpu_simd_lanes() -> c_int;
    pub fn sd_cpu_cas_ids_files(paths: *const *const c_char, sizes: *const u64, n: usize, out_hex17: *mut c_char,
                                status: *mut i32, nthreads: c_int) -> c_int;
    pub fn sd_cpu_file_checksums(paths: *const *const c_char, n: usize, out_hex65: *mut c_char, status: *mut i32,
                                 nthreads: c_int) -> c_int;
    pub fn sd_cpu_cas_id_path(path: *const c_char, size: u64, out_hex17: *mut c_char, status: *mut i32) -> c_int;
    pub fn sd_cpu_file_checksum_path(path: *const c_char, out_hex65: *mut c_char, status: *mut i32) -> c_int;
    // multi-GPU dedup over RCCL (one process per GPU)
    pub fn sd_comm_id(out_id: *mut u8) -> c_int;
    pub fn sd_comm_create(ctx: *mut sd_cas_ctx, id: *const u8, nranks: c_int, rank: c_int,
                          out: *mut *mut sd_comm) -> c_int;
    pub fn sd_comm_destroy(comm: *mut sd_comm);
    pub fn sd_comm_rccl_info(version: *mut c_int, path_out: *mut c_char, path_cap: usize) -> c_int;
    // the same collectives with the ranks as threads of one process (several GPUs, one process)
    pub fn sd_comm_group_create(nranks: c_int, out: *mut *mut sd_comm_group) -> c_int;
    pub fn sd_comm_group_destroy(group: *mut sd_comm_group);
    pub fn sd_comm_create_local(ctx: *mut sd_cas_ctx, group: *mut sd_comm_group, rank: c_int,
                                out: *mut *mut sd_comm) -> c_int;
    pub fn sd_cas_dedup_mgpu(ctx: *mut sd_cas_ctx, comm: *mut sd_comm, d_hash32: *const u8, d_valid: *const u8,
                             n: u64, global_index_base: u64, chunk_size: u64, d_records_out: *mut u64,
                             d_rep_out: *mut u64, d_owner_out: *mut u64, capacity: u64, m_out: *mut u64,
                             n_groups_out: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_cas_dedup_mgpu_indexed(ctx: *mut sd_cas_ctx, comm: *mut sd_comm, d_hash32: *const u8,
                                     d_valid: *const u8, n: u64, global_index_base: u64, chunk_size: u64,
                                     d_records_out: *mut u64, d_rep_out: *mut u64, d_owner_out: *mut u64,
                                     capacity: u64, m_out: *mut u64, n_groups_out: *mut u64, stream: *mut c_void,
                                     index: *const sd_object_index, d_existing_out: *mut u8, d_new_out: *mut u64,
                                     n_new_out: *mut u64) -> c_int;
    // the Object index: which Object already owns a cas_id (file_identifier/mod.rs:168-225)
    pub fn sd_object_index_create(ctx: *mut sd_cas_ctx, nparts: c_int, part: c_int,
                                  out: *mut *mut sd_object_index) -> c_int;
    pub fn sd_object_index_destroy(index: *mut sd_object_index);
    pub fn sd_object_index_insert(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, d_keys: *const u64,
                                  d_object_ids: *const u64, m: u64, taken: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_insert_hex(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, hex17: *const c_char,
                                      object_ids: *const u64, m: u64, taken: *mut u64) -> c_int;
    // removal: Objects deleted (orphan_remover.rs:57-95), file_paths deleted or moved to another
    // cas_id (watcher/utils.rs:410-494)
    pub fn sd_object_index_remove(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, d_keys: *const u64,
                                  d_object_ids: *const u64, m: u64, d_removed_out: *mut u64, capacity: u64,
                                  removed: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_remove_objects(ctx: *mut sd_cas_ctx, index: *mut sd_object_index,
                                          d_object_ids: *const u64, m: u64, d_removed_out: *mut u64, capacity: u64,
                                          removed: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_remove_hex(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, hex17: *const c_char,
                                      object_ids: *const u64, m: u64, removed: *mut u64) -> c_int;
    pub fn sd_object_index_count(index: *const sd_object_index, n: *mut u64) -> c_int;
    pub fn sd_object_index_lookup(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_keys: *const u64, m: u64,
                                  d_object_ids: *mut u64, d_found: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_export(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_keys_out: *mut u64,
                                  d_object_ids_out: *mut u64, capacity: u64, stream: *mut c_void) -> c_int;
    // the owners mode (SD_OBJECT_INDEX_OWNERS): one entry per (cas_id, Object) with its link count
    pub fn sd_object_index_create_ex(ctx: *mut sd_cas_ctx, nparts: c_int, part: c_int, flags: c_int,
                                     out: *mut *mut sd_object_index) -> c_int;
    pub fn sd_object_index_flags(index: *const sd_object_index, flags: *mut c_int) -> c_int;
    pub fn sd_object_index_links(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_keys: *const u64,
                                 d_object_ids: *const u64, m: u64, d_links_out: *mut u64,
                                 stream: *mut c_void) -> c_int;
    pub fn sd_object_index_export_links(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_keys_out: *mut u64,
                                        d_ids_out: *mut u64, d_links_out: *mut u64, capacity: u64,
                                        stream: *mut c_void) -> c_int;
    pub fn sd_cpu_object_index_create_ex(nparts: c_int, part: c_int, flags: c_int,
                                         out: *mut *mut sd_cpu_object_index) -> c_int;
    pub fn sd_cpu_object_index_flags(index: *const sd_cpu_object_index, flags: *mut c_int) -> c_int;
    pub fn sd_cpu_object_index_links(index: *const sd_cpu_object_index, keys: *const u64, object_ids: *const u64,
                                     m: u64, links_out: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_export_links(index: *const sd_cpu_object_index, keys_out: *mut u64,
                                            ids_out: *mut u64, links_out: *mut u64, capacity: u64) -> c_int;
    // apply: the links that went, then the links that came, of an owners-mode index in one call
    pub fn sd_object_index_apply(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, d_rm_keys: *const u64,
                                 d_rm_ids: *const u64, m_rm: u64, d_in_keys: *const u64, d_in_ids: *const u64,
                                 m_in: u64, d_removed_out: *mut u64, capacity: u64, removed: *mut u64,
                                 taken: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_apply_hex(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, rm_hex17: *const c_char,
                                     rm_ids: *const u64, m_rm: u64, in_hex17: *const c_char, in_ids: *const u64,
                                     m_in: u64, removed: *mut u64, taken: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_apply(index: *mut sd_cpu_object_index, rm_keys: *const u64, rm_ids: *const u64,
                                     m_rm: u64, in_keys: *const u64, in_ids: *const u64, m_in: u64,
                                     removed_out: *mut u64, capacity: u64, removed: *mut u64,
                                     taken: *mut u64) -> c_int;
    // the view by Object of an owners-mode index: per-Object link totals and the orphans among
    // listed ids, without the DB scan of orphan_remover.rs:57-95
    pub fn sd_object_index_object_links(ctx: *mut sd_cas_ctx, index: *const sd_object_index,
                                        d_object_ids: *const u64, id_stride: u64, m: u64, d_links_out: *mut u64,
                                        d_entries_out: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_orphans(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_object_ids: *const u64,
                                   id_stride: u64, m: u64, d_orphans_out: *mut u64, capacity: u64, count: *mut u64,
                                   stream: *mut c_void) -> c_int;
    pub fn sd_cpu_object_index_object_links(index: *const sd_cpu_object_index, object_ids: *const u64,
                                            id_stride: u64, m: u64, links_out: *mut u64,
                                            entries_out: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_orphans(index: *const sd_cpu_object_index, object_ids: *const u64, id_stride: u64,
                                       m: u64, orphans_out: *mut u64, capacity: u64, count: *mut u64) -> c_int;
    // the view by key of an owners-mode index: the duplicate groups per cas_id (mod.rs:189-225,
    // :229-333), without a GROUP BY over file_path
    pub fn sd_object_index_key_links(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_keys: *const u64, m: u64,
                                     d_links_out: *mut u64, d_owners_out: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_duplicates(ctx: *mut sd_cas_ctx, index: *const sd_object_index, min_links: u64,
                                      min_owners: u64, d_keys_out: *mut u64, d_first_out: *mut u64,
                                      d_links_out: *mut u64, d_owners_out: *mut u64, capacity: u64,
                                      count: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_object_index_duplicate_entries(ctx: *mut sd_cas_ctx, index: *const sd_object_index, min_links: u64,
                                             min_owners: u64, d_keys_out: *mut u64, d_ids_out: *mut u64,
                                             d_links_out: *mut u64, capacity: u64, count: *mut u64,
                                             stream: *mut c_void) -> c_int;
    pub fn sd_object_index_duplicate_stats(ctx: *mut sd_cas_ctx, index: *const sd_object_index, out: *mut u64,
                                           stream: *mut c_void) -> c_int;
    // merge Objects: "Object from IS Object to" (mod.rs:229-333 gave same-step duplicates an
    // Object each); every id relabelled once and simultaneously, equal pairs of a key coalesced
    pub fn sd_object_index_merge_objects(ctx: *mut sd_cas_ctx, index: *mut sd_object_index, d_from: *const u64,
                                         d_to: *const u64, m: u64, moved: *mut u64, coalesced: *mut u64,
                                         stream: *mut c_void) -> c_int;
    pub fn sd_cpu_object_index_merge_objects(index: *mut sd_cpu_object_index, from: *const u64, to: *const u64,
                                             m: u64, moved: *mut u64, coalesced: *mut u64) -> c_int;
    // a duplicate group is a candidate set (cas.rs:30-58 samples): split by full checksum
    // (hash.rs:10-24) on the device, or over host arrays without one
    pub fn sd_dedup_confirm(ctx: *mut sd_cas_ctx, d_keys: *const u64, d_hash32: *const u8, d_valid: *const u8,
                            m: u64, d_rep: *mut u64, d_class_size: *mut u64, d_verdict: *mut u8,
                            d_sets_out: *mut u64, capacity: u64, n_sets: *mut u64, stats: *mut u64,
                            stream: *mut c_void) -> c_int;
    pub fn sd_dedup_confirm_stats(ctx: *mut sd_cas_ctx, out: *mut u64) -> c_int;
    pub fn sd_cpu_dedup_confirm(keys: *const u64, hash32: *const u8, valid: *const u8, m: u64, rep: *mut u64,
                                class_size: *mut u64, verdict: *mut u8, sets_out: *mut u64, capacity: u64,
                                n_sets: *mut u64, stats: *mut u64) -> c_int;
    // checksum trees: a file's level (one 32-byte node per 2^block_log2 bytes) beside its checksum,
    // the roots from levels alone, and a verify that names the (file, block) rows that differ
    // (validator_job.rs:138-141; spaceblock's 128 KiB blocks, block_size.rs:20-23)
    pub fn sd_checksum_tree_nodes(len: u64, block_log2: u32, n_nodes: *mut u64) -> c_int;
    pub fn sd_checksum_tree_create(ctx: *mut sd_cas_ctx, offsets: *const u64, lens: *const u64, n: usize,
                                   block_log2: u32, out: *mut *mut sd_checksum_tree) -> c_int;
    pub fn sd_checksum_tree_destroy(tree: *mut sd_checksum_tree);
    pub fn sd_checksum_tree_layout(tree: *const sd_checksum_tree, node_base: *mut u64) -> c_int;
    pub fn sd_checksum_tree_stats(tree: *const sd_checksum_tree, out: *mut u64) -> c_int;
    pub fn sd_checksum_tree_run(ctx: *mut sd_cas_ctx, tree: *const sd_checksum_tree, d_data: *const u8,
                                d_nodes: *mut u8, d_hash32: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_roots(ctx: *mut sd_cas_ctx, tree: *const sd_checksum_tree, d_nodes: *const u8,
                                  d_hash32: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_verify(ctx: *mut sd_cas_ctx, tree: *const sd_checksum_tree, d_data: *const u8,
                                   d_expected: *const u8, d_bad: *mut u8, d_rows_out: *mut u64, capacity: u64,
                                   count: *mut u64, stats: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_cpu_checksum_tree(data: *const u8, offsets: *const u64, lens: *const u64, n: usize, block_log2: u32,
                                nodes: *mut u8, hash32: *mut u8, nthreads: c_int) -> c_int;
    pub fn sd_cpu_checksum_tree_roots(nodes: *const u8, lens: *const u64, n: usize, block_log2: u32,
                                      hash32: *mut u8) -> c_int;
    pub fn sd_cpu_checksum_tree_verify(data: *const u8, offsets: *const u64, lens: *const u64, n: usize,
                                       block_log2: u32, expected: *const u8, bad: *mut u8, rows_out: *mut u64,
                                       capacity: u64, count: *mut u64, stats: *mut u64, nthreads: c_int) -> c_int;
    // listed blocks: rows = m x (file, block), data_offsets = where each row's bytes sit
    pub fn sd_checksum_tree_blocks_create(ctx: *mut sd_cas_ctx, lens: *const u64, n_files: usize, block_log2: u32,
                                          rows: *const u64, data_offsets: *const u64, m: usize,
                                          out: *mut *mut sd_checksum_tree_blocks) -> c_int;
    pub fn sd_checksum_tree_blocks_destroy(blocks: *mut sd_checksum_tree_blocks);
    pub fn sd_checksum_tree_blocks_stats(blocks: *const sd_checksum_tree_blocks, out: *mut u64) -> c_int;
    pub fn sd_checksum_tree_blocks_run(ctx: *mut sd_cas_ctx, blocks: *const sd_checksum_tree_blocks,
                                       d_data: *const u8, d_nodes_out: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_blocks_verify(ctx: *mut sd_cas_ctx, blocks: *const sd_checksum_tree_blocks,
                                          d_data: *const u8, d_expected: *const u8, d_bad: *mut u8,
                                          d_rows_out: *mut u64, capacity: u64, count: *mut u64, stats: *mut u64,
                                          stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_blocks_update(ctx: *mut sd_cas_ctx, blocks: *mut sd_checksum_tree_blocks,
                                          d_data: *const u8, d_nodes: *mut u8, d_hash32: *mut u8,
                                          stream: *mut c_void) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks(data: *const u8, lens: *const u64, n_files: usize, block_log2: u32,
                                       rows: *const u64, data_offsets: *const u64, m: usize, nodes_out: *mut u8,
                                       nthreads: c_int) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_verify(data: *const u8, lens: *const u64, n_files: usize, block_log2: u32,
                                              rows: *const u64, data_offsets: *const u64, m: usize,
                                              expected: *const u8, bad: *mut u8, rows_out: *mut u64, capacity: u64,
                                              count: *mut u64, stats: *mut u64, nthreads: c_int) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_update(data: *const u8, lens: *const u64, n_files: usize, block_log2: u32,
                                              rows: *const u64, data_offsets: *const u64, m: usize, nodes: *mut u8,
                                              hash32: *mut u8, nthreads: c_int) -> c_int;
    // block proofs: a listed block against the file's checksum and length alone
    pub fn sd_checksum_tree_proof_entries(len: u64, block_log2: u32, block: u64, entries: *mut u32) -> c_int;
    pub fn sd_checksum_tree_blocks_proof_layout(blocks: *mut sd_checksum_tree_blocks, proof_base: *mut u64) -> c_int;
    pub fn sd_checksum_tree_blocks_prove(ctx: *mut sd_cas_ctx, blocks: *mut sd_checksum_tree_blocks,
                                         d_nodes: *const u8, d_proofs_out: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_blocks_verify_proofs(ctx: *mut sd_cas_ctx, blocks: *mut sd_checksum_tree_blocks,
                                                 d_data: *const u8, d_proofs: *const u8, d_roots: *const u8,
                                                 d_nodes_out: *mut u8, d_bad: *mut u8, d_rows_out: *mut u64,
                                                 capacity: u64, count: *mut u64, stats: *mut u64,
                                                 stream: *mut c_void) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_prove(nodes: *const u8, lens: *const u64, n_files: usize, block_log2: u32,
                                             rows: *const u64, m: usize, proofs_out: *mut u8) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_verify_proofs(data: *const u8, lens: *const u64, n_files: usize,
                                                     block_log2: u32, rows: *const u64, data_offsets: *const u64,
                                                     m: usize, proofs: *const u8, roots: *const u8,
                                                     nodes_out: *mut u8, bad: *mut u8, rows_out: *mut u64,
                                                     capacity: u64, count: *mut u64, stats: *mut u64,
                                                     nthreads: c_int) -> c_int;
    // range proofs: a run of blocks (Range::Partial) against the checksum and length alone, two flanks per level
    pub fn sd_checksum_tree_range_proof_entries(len: u64, block_log2: u32, first: u64, count: u64,
                                                entries: *mut u32) -> c_int;
    pub fn sd_checksum_tree_blocks_set_ranges(blocks: *mut sd_checksum_tree_blocks, range_base: *const u64,
                                              q: usize) -> c_int;
    pub fn sd_checksum_tree_blocks_range_proof_layout(blocks: *mut sd_checksum_tree_blocks,
                                                      proof_base: *mut u64) -> c_int;
    pub fn sd_checksum_tree_blocks_prove_ranges(ctx: *mut sd_cas_ctx, blocks: *mut sd_checksum_tree_blocks,
                                                d_nodes: *const u8, d_proofs_out: *mut u8,
                                                stream: *mut c_void) -> c_int;
    pub fn sd_checksum_tree_blocks_verify_range_proofs(ctx: *mut sd_cas_ctx, blocks: *mut sd_checksum_tree_blocks,
                                                       d_data: *const u8, d_proofs: *const u8, d_roots: *const u8,
                                                       d_nodes_out: *mut u8, d_bad: *mut u8, d_ranges_out: *mut u64,
                                                       capacity: u64, count: *mut u64, stats: *mut u64,
                                                       stream: *mut c_void) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_prove_ranges(nodes: *const u8, lens: *const u64, n_files: usize,
                                                    block_log2: u32, rows: *const u64, m: usize,
                                                    range_base: *const u64, q: usize, proofs_out: *mut u8) -> c_int;
    pub fn sd_cpu_checksum_tree_blocks_verify_range_proofs(data: *const u8, lens: *const u64, n_files: usize,
                                                           block_log2: u32, rows: *const u64,
                                                           data_offsets: *const u64, m: usize,
                                                           range_base: *const u64, q: usize, proofs: *const u8,
                                                           roots: *const u8, nodes_out: *mut u8, bad: *mut u8,
                                                           ranges_out: *mut u64, capacity: u64, count: *mut u64,
                                                           stats: *mut u64, nthreads: c_int) -> c_int;
    // shared blocks: which blocks of a batch of levels are there more than once (aligned blocks only)
    pub fn sd_checksum_tree_shared(ctx: *mut sd_cas_ctx, lens: *const u64, n: usize, block_log2: u32,
                                   d_nodes: *const u8, min_blocks: u64, d_rep: *mut u64, d_class_size: *mut u64,
                                   d_files_out: *mut u64, d_pairs_out: *mut u64, capacity: u64, n_pairs: *mut u64,
                                   stats: *mut u64, stream: *mut c_void) -> c_int;
    pub fn sd_cpu_checksum_tree_shared(lens: *const u64, n: usize, block_log2: u32, nodes: *const u8,
                                       min_blocks: u64, rep: *mut u64, class_size: *mut u64, files_out: *mut u64,
                                       pairs_out: *mut u64, capacity: u64, n_pairs: *mut u64,
                                       stats: *mut u64) -> c_int;
    // device buffers for callers that hold their lists on the host (sd_memcpy syncs `stream`)
    pub fn sd_device_malloc(ctx: *mut sd_cas_ctx, bytes: u64, out: *mut *mut c_void) -> c_int;
    pub fn sd_device_free(ctx: *mut sd_cas_ctx, p: *mut c_void);
    pub fn sd_memcpy(ctx: *mut sd_cas_ctx, dst: *mut c_void, src: *const c_void, bytes: u64,
                     stream: *mut c_void) -> c_int;
    pub fn sd_dedup_owners_indexed(ctx: *mut sd_cas_ctx, index: *const sd_object_index, d_records: *const u64,
                                   m: u64, d_rep: *const u64, chunk_size: u64, d_owner: *mut u64,
                                   d_existing: *mut u8, d_new_out: *mut u64, d_n_new: *mut u64,
                                   stream: *mut c_void) -> c_int;
    pub fn sd_cpu_object_index_create(nparts: c_int, part: c_int, out: *mut *mut sd_cpu_object_index) -> c_int;
    pub fn sd_cpu_object_index_destroy(index: *mut sd_cpu_object_index);
    pub fn sd_cpu_object_index_insert(index: *mut sd_cpu_object_index, keys: *const u64, object_ids: *const u64,
                                      m: u64, taken: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_remove(index: *mut sd_cpu_object_index, keys: *const u64, object_ids: *const u64,
                                      m: u64, removed_out: *mut u64, capacity: u64, removed: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_remove_objects(index: *mut sd_cpu_object_index, object_ids: *const u64, m: u64,
                                              removed_out: *mut u64, capacity: u64, removed: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_lookup(index: *const sd_cpu_object_index, keys: *const u64, m: u64,
                                      object_ids: *mut u64, found: *mut u8) -> c_int;
    pub fn sd_cpu_object_index_count(index: *const sd_cpu_object_index, n: *mut u64) -> c_int;
    pub fn sd_cpu_object_index_export(index: *const sd_cpu_object_index, keys_out: *mut u64,
                                      object_ids_out: *mut u64, capacity: u64) -> c_int;
    pub fn sd_cpu_dedup_owners_indexed(index: *const sd_cpu_object_index, records: *const u64, m: u64,
                                       rep: *const u64, chunk_size: u64, owner: *mut u64, existing: *mut u8,
                                       new_out: *mut u64, n_new: *mut u64) -> c_int;
    pub fn sd_shard_plan(sizes: *const u64, n: usize, nranks: c_int, bounds_out: *mut u64) -> c_int;
    // one file's checksum over many GPUs (its 1 MiB blocks sharded by rank)
    pub fn sd_split_range(total_len: u64, nranks: c_int, rank: c_int, offset: *mut u64, len: *mut u64,
                          cv_bytes: *mut u64) -> c_int;
    pub fn sd_split_checksum_create(ctx: *mut sd_cas_ctx, total_len: u64, nranks: c_int, rank: c_int,
                                    out: *mut *mut sd_split_checksum) -> c_int;
    pub fn sd_split_checksum_destroy(split: *mut sd_split_checksum);
    pub fn sd_split_checksum_mgpu(ctx: *mut sd_cas_ctx, comm: *mut sd_comm, split: *mut sd_split_checksum,
                                  d_slice: *const u8, d_cvs: *mut u8, d_hash32: *mut u8, stream: *mut c_void) -> c_int;
    pub fn sd_cpu_split_leaves(slice: *const u8, total_len: u64, nranks: c_int, rank: c_int, cvs: *mut u8,
                               nthreads: c_int) -> c_int;
    pub fn sd_cpu_split_root(cvs: *const u8, total_len: u64, out_hash32: *mut u8) -> c_int;
}

/// One context per process on device 0 (the job system's 5 concurrent jobs, watcher and
/// non_indexed tasks all share it: every entry point is thread-safe).
pub struct Ctx(*mut sd_cas_ctx);
unsafe impl Send for Ctx {}
unsafe impl Sync for Ctx {}

/// The process's GPU context, or the reason there is none (no gfx950 device, driver
/// error, ABI mismatch) -- callers then take the CPU path.  Never panics.
pub fn ctx() -> Result<&'static Ctx, io::Error> {
    static CTX: OnceLock<Result<Ctx, String>> = OnceLock::new();
    CTX.get_or_init(|| {
        let abi = unsafe { sd_cas_abi_version() };
        if abi != SD_CAS_ABI_VERSION {
            return Err(format!("libsdcas ABI {abi}, this binding expects {SD_CAS_ABI_VERSION}"));
        }
        let mut p = std::ptr::null_mut();
        match unsafe { sd_cas_ctx_create(0, &mut p) } {
            SD_OK => Ok(Ctx(p)),
            _ => Err(last_error()),
        }
    })
    .as_ref()
    .map_err(|e| io::Error::new(io::ErrorKind::Unsupported, e.clone()))
}

pub fn last_error() -> String {
    unsafe { CStr::from_ptr(sd_cas_last_error()) }.to_string_lossy().into_owned()
}

/// sd_file_status -> the io::Error the reference's reads would have produced.
pub fn status_to_io(st: i32) -> io::Error {
    match st & 0xFFFF {
        SD_FILE_SHORT_READ => io::ErrorKind::UnexpectedEof.into(), // read_exact (cas.rs:36,43,56)
        SD_FILE_IO_ERROR => io::Error::from_raw_os_error((st >> 16) & 0xFFFF),
        _ => io::Error::new(io::ErrorKind::Other, format!("sd_cas status {st}")),
    }
}

fn cpath(p: &Path) -> Result<CString, io::Error> {
    CString::new(p.as_os_str().as_bytes()).map_err(|e| io::Error::new(io::ErrorKind::InvalidInput, e))
}

fn hex_at(buf: &[c_char], i: usize, stride: usize, len: usize) -> String {
    buf[stride * i..stride * i + len].iter().map(|&b| b as u8 as char).collect()
}

fn per_file(rc: c_int, status: &[i32], hex: &[c_char], stride: usize, len: usize) -> Vec<Result<String, io::Error>> {
    (0..status.len())
        .map(|i| {
            if rc != SD_OK {
                Err(io::Error::new(io::ErrorKind::Other, last_error()))
            } else if status[i] != SD_FILE_OK {
                Err(status_to_io(status[i]))
            } else {
                Ok(hex_at(hex, i, stride, len))
            }
        })
        .collect()
}

/// Batched generate_cas_id (cas.rs:23-62): one result per (path, size), in order.  On the
/// GPU the library reads the windows on its stager pool and overlaps them with the
/// kernels; without a device, the CPU path on 16 host threads.
pub fn cas_ids_blocking(files: &[(&Path, u64)]) -> Vec<Result<String, io::Error>> {
    let n = files.len();
    let c: Vec<CString> = match files.iter().map(|f| cpath(f.0)).collect() {
        Ok(v) => v,
        Err(e) => return (0..n).map(|_| Err(io::Error::new(e.kind(), e.to_string()))).collect(),
    };
    let ptrs: Vec<*const c_char> = c.iter().map(|s| s.as_ptr()).collect();
    let sizes: Vec<u64> = files.iter().map(|f| f.1).collect();
    let mut hex = vec![0 as c_char; 17 * n];
    let mut status = vec![0i32; n];
    let rc = unsafe {
        match ctx() {
            Ok(g) => sd_cas_ids_files(g.0, ptrs.as_ptr(), sizes.as_ptr(), n, hex.as_mut_ptr(), status.as_mut_ptr(), 16),
            Err(_) => sd_cpu_cas_ids_files(ptrs.as_ptr(), sizes.as_ptr(), n, hex.as_mut_ptr(), status.as_mut_ptr(), 16),
        }
    };
    per_file(rc, &status, &hex, 17, 16)
}

/// Single-file generate_cas_id for the latency callers (watcher, non_indexed).
pub fn cas_id_blocking(path: &Path, size: u64) -> Result<String, io::Error> {
    let c = cpath(path)?;
    let mut hex = [0 as c_char; 17];
    let mut st = 0i32;
    let rc = unsafe {
        match ctx() {
            Ok(g) => sd_cas_id_path(g.0, c.as_ptr(), size, hex.as_mut_ptr(), &mut st),
            Err(_) => sd_cpu_cas_id_path(c.as_ptr(), size, hex.as_mut_ptr(), &mut st),
        }
    };
    per_file(rc, &[st], &hex, 17, 16).pop().expect("one result")
}

/// Batched file_checksum (hash.rs:10-24).
pub fn checksums_blocking(paths: &[&Path]) -> Vec<Result<String, io::Error>> {
    let n = paths.len();
    let c: Vec<CString> = match paths.iter().map(|p| cpath(p)).collect() {
        Ok(v) => v,
        Err(e) => return (0..n).map(|_| Err(io::Error::new(e.kind(), e.to_string()))).collect(),
    };
    let ptrs: Vec<*const c_char> = c.iter().map(|s| s.as_ptr()).collect();
    let mut hex = vec![0 as c_char; 65 * n];
    let mut status = vec![0i32; n];
    let rc = unsafe {
        match ctx() {
            Ok(g) => sd_file_checksums(g.0, ptrs.as_ptr(), n, hex.as_mut_ptr(), status.as_mut_ptr()),
            Err(_) => sd_cpu_file_checksums(ptrs.as_ptr(), n, hex.as_mut_ptr(), status.as_mut_ptr(), 16),
        }
    };
    per_file(rc, &status, &hex, 65, 64)
}

/// Single-file file_checksum (the watcher's recompute, watcher/utils.rs:438-446).
pub fn checksum_blocking(path: &Path) -> Result<String, io::Error> {
    let c = cpath(path)?;
    let mut hex = [0 as c_char; 65];
    let mut st = 0i32;
    let rc = unsafe {
        match ctx() {
            Ok(g) => sd_file_checksum_path(g.0, c.as_ptr(), hex.as_mut_ptr(), &mut st),
            Err(_) => sd_cpu_file_checksum_path(c.as_ptr(), hex.as_mut_ptr(), &mut st),
        }
    };
    per_file(rc, &[st], &hex, 65, 64).pop().expect("one result")
}

/// cas_id and checksum of files already read into one buffer (`ranges`: (offset, len), offsets
/// 16-byte aligned), every byte sent to the device once: what `inner_update_file` computes per
/// file (watcher/utils.rs:393 and :438-446).  Equal to generate_cas_id(path, len) and
/// file_checksum(path) for files holding exactly `len` bytes; empty ranges are hashed, the
/// caller applies FileMetadata::new's skip.  Without a device: the CPU path on 16 threads.
pub fn fingerprints_blocking(data: &[u8], ranges: &[(u64, u64)]) -> Result<Vec<(String, String)>, io::Error> {
    let n = ranges.len();
    if ranges.iter().any(|r| r.0 % 16 != 0 || r.0.checked_add(r.1).map_or(true, |e| e > data.len() as u64)) {
        return Err(io::Error::new(io::ErrorKind::InvalidInput, "range misaligned or beyond the buffer"));
    }
    let offs: Vec<u64> = ranges.iter().map(|r| r.0).collect();
    let lens: Vec<u64> = ranges.iter().map(|r| r.1).collect();
    let mut h17 = vec![0 as c_char; 17 * n];
    let mut h65 = vec![0 as c_char; 65 * n];
    let rc = unsafe {
        match ctx() {
            Ok(g) => sd_fingerprints(g.0, data.as_ptr(), offs.as_ptr(), lens.as_ptr(), n, h17.as_mut_ptr(), h65.as_mut_ptr()),
            Err(_) => sd_cpu_fingerprints(data.as_ptr(), offs.as_ptr(), lens.as_ptr(), n, h17.as_mut_ptr(), h65.as_mut_ptr(), 16),
        }
    };
    if rc != SD_OK {
        return Err(io::Error::new(io::ErrorKind::Other, last_error()));
    }
    Ok((0..n).map(|i| (hex_at(&h17, i, 17, 16), hex_at(&h65, i, 65, 64))).collect())
}

// Keeping the Object index true while the library changes.  The invariant:
// index[c] = the first live Object, in DB order, that owns a file_path with cas_id c.  Remove
// and insert are two calls, because the DB query sits between them; both are exclusive on the
// index.  (The owners mode further down has them as one call, OwnersIndex::apply.)
//
// The orphan remover's hook (orphan_remover.rs:57-95), after its delete_many of <= 512 ids:
//
//     let mut removed = 0u64;
//     sd_object_index_remove_objects(ctx, index, d_ids, ids.len() as u64, d_removed, capacity, &mut removed, stream);
//     // d_removed holds (key, Object id) of the entries that went; usually nobody else owns those
//     // cas_ids, but a same-chunk duplicate's own Object may (mod.rs:233-333):
//     let rows = db.file_path().find_many(vec![cas_id::in_vec(hex(&d_removed, removed))]).order_by(object_id).exec();
//     sd_object_index_insert_hex(ctx, index, hex17(&rows), object_ids(&rows), rows.len() as u64, &mut taken);
//
// The watcher's update hook (watcher/utils.rs:410-494), file_path of Object O: cas_id A -> B:
//
//     sd_object_index_remove_hex(ctx, index, hex17(&[a]), [o].as_ptr(), 1, &mut removed);   // A -> O only if it still says O
//     if lookup(b).map_or(false, |owner| db_order(owner) > db_order(o)) {
//         sd_object_index_remove_hex(ctx, index, hex17(&[b]), std::ptr::null(), 1, &mut removed);
//     }
//     let rows = db.file_path().find_many(vec![cas_id::in_vec(vec![a, b])]).order_by(object_id).exec();
//     sd_object_index_insert_hex(ctx, index, hex17(&rows), object_ids(&rows), rows.len() as u64, &mut taken);
//
// A deleted file_path (c, O) is the first and the last line of that hook with c for A.
//
// With an owners-mode index (sd_object_index_create_ex(.., SD_OBJECT_INDEX_OWNERS, ..)) none of
// the hooks asks the DB for owners: the index holds every (cas_id, Object) pair with its count
// of file_paths, and the first owner of a cas_id is its smallest Object id.
//
//     // after a scan: ONE insert of (cas_id, Object id) for every record, linked and created alike
//     sd_object_index_insert(ctx, index, d_keys, d_object_ids, m, &mut taken, stream);
//     // a deleted file_path (c, O): one link less; the entry leaves at zero
//     sd_object_index_remove_hex(ctx, index, hex17(&[c]), [o].as_ptr(), 1, &mut removed);
//     // the watcher's update hook, A -> B on O
//     sd_object_index_remove_hex(ctx, index, hex17(&[a]), [o].as_ptr(), 1, &mut removed);
//     sd_object_index_insert_hex(ctx, index, hex17(&[b]), [o].as_ptr(), 1, &mut taken);
//     // the orphan remover's hook, after a DB scan for the ids (orphan_remover.rs:57-95)
//     sd_object_index_remove_objects(ctx, index, d_ids, ids.len() as u64, std::ptr::null_mut(), 0, &mut removed, stream);
//     // ... or without that scan: the candidates are the Object ids of the (key, id) rows the calls
//     // above reported in d_removed_out, plus the Objects that lost a file_path without a cas_id;
//     // the orphans among them own nothing in the index and need no remove_objects call
//     sd_object_index_orphans(ctx, index, d_removed.add(1), 2, removed, d_orphans, capacity, &mut count, stream);
//     // delete from the DB those whose count of cas-less file_paths (kept by the host) is zero
//
// The update hook and a burst of watcher events are ONE call with `OwnersIndex::apply` below: the
// links that went, then the links that came, one rewrite of the index and no state in between.

/// An owners-mode Object index on the process's GPU context.
pub struct OwnersIndex(*mut sd_object_index);
unsafe impl Send for OwnersIndex {}

impl OwnersIndex {
    pub fn new(nparts: i32, part: i32) -> Result<Self, io::Error> {
        let g = ctx()?;
        let mut p = std::ptr::null_mut();
        match unsafe { sd_object_index_create_ex(g.0, nparts, part, SD_OBJECT_INDEX_OWNERS, &mut p) } {
            SD_OK => Ok(OwnersIndex(p)),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }

    /// sd_object_index_apply_hex: `gone` and `came` are (cas_id as 16 lower-case hex digits,
    /// Object id) of the file_path links that left and that entered since the last call -- a
    /// content change A -> B on O is `gone = [(A, O)]`, `came = [(B, O)]`; a deleted file_path has
    /// an empty `came`; a burst passes its coalesced lists (a link that came and went again
    /// inside the burst is struck from `came`, not added to `gone`).  Returns (entries that
    /// left the index, entries that entered it): the net effect, not the two lists' lengths.
    pub fn apply(&mut self, gone: &[(&str, u64)], came: &[(&str, u64)]) -> Result<(u64, u64), io::Error> {
        fn hex17(rows: &[(&str, u64)]) -> Result<Vec<u8>, io::Error> {
            let mut buf = Vec::with_capacity(17 * rows.len());
            for r in rows {
                if r.0.len() != 16 {
                    return Err(io::Error::new(io::ErrorKind::InvalidInput, "a cas_id is not 16 characters"));
                }
                buf.extend_from_slice(r.0.as_bytes());
                buf.push(0);
            }
            Ok(buf)
        }
        let g = ctx()?;
        let (rm_hex, in_hex) = (hex17(gone)?, hex17(came)?);
        let rm_ids: Vec<u64> = gone.iter().map(|r| r.1).collect();
        let in_ids: Vec<u64> = came.iter().map(|r| r.1).collect();
        let (mut removed, mut taken) = (0u64, 0u64);
        let rc = unsafe {
            sd_object_index_apply_hex(g.0, self.0, rm_hex.as_ptr() as *const c_char, rm_ids.as_ptr(), gone.len() as u64,
                                      in_hex.as_ptr() as *const c_char, in_ids.as_ptr(), came.len() as u64,
                                      &mut removed, &mut taken)
        };
        match rc {
            SD_OK => Ok((removed, taken)),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }

    /// sd_object_index_orphans: the distinct Objects among `candidates` that own nothing in the
    /// index any more, ascending -- the orphan remover's query (orphan_remover.rs:57-95) without
    /// its scan of the Object table.  `candidates` are the Object ids of the pairs that left the
    /// index since the last pass (the reports of apply and remove) and every Object that lost a
    /// file_path without a cas_id.  The index knows only links that have a cas_id: the caller
    /// deletes an Object iff it is returned here AND its count of file_paths without a cas_id
    /// (kept by the host) is zero.  No remove_objects call follows: an orphan
    /// holds no entry.
    pub fn orphans(&self, candidates: &[u64]) -> Result<Vec<u64>, io::Error> {
        let m = candidates.len();
        if m == 0 {
            return Ok(Vec::new());
        }
        let g = ctx()?;
        let fail = || io::Error::new(io::ErrorKind::Other, last_error());
        let bytes = (8 * m) as u64;
        let mut buf: *mut c_void = std::ptr::null_mut();
        // ids in the first half, the orphans (m at most) in the second
        if unsafe { sd_device_malloc(g.0, 2 * bytes, &mut buf) } != SD_OK {
            return Err(fail());
        }
        let d_ids = buf as *mut u64;
        let d_out = unsafe { d_ids.add(m) };
        let mut out = vec![0u64; m];
        let mut count = 0u64;
        let null = std::ptr::null_mut();
        let rc = unsafe {
            let mut rc = sd_memcpy(g.0, buf, candidates.as_ptr() as *const c_void, bytes, null);
            if rc == SD_OK {
                rc = sd_object_index_orphans(g.0, self.0, d_ids, 1, m as u64, d_out, m as u64, &mut count, null);
            }
            if rc == SD_OK && count > 0 {
                rc = sd_memcpy(g.0, out.as_mut_ptr() as *mut c_void, d_out as *const c_void, 8 * count, null);
            }
            rc
        };
        let res = if rc == SD_OK { Ok(()) } else { Err(fail()) };
        unsafe { sd_device_free(g.0, buf) };
        res?;
        out.truncate(count as usize);
        Ok(out)
    }
}

impl Drop for OwnersIndex {
    fn drop(&mut self) {
        unsafe { sd_object_index_destroy(self.0) }
    }
}

/// libsdcas's RCCL communicator for a multi-GPU library scan (one process per GPU).
/// A member of an in-process group holds a reference to the group, so the group is
/// destroyed only after its last member (sd_comm_destroy writes to the group).
pub struct Comm {
    raw: *mut sd_comm,
    _group: Option<Arc<GroupHandle>>,
}
unsafe impl Send for Comm {}

impl Comm {
    /// On rank 0: the 128-byte id every rank passes to [`Comm::join`] (out of band).
    pub fn unique_id() -> Result<[u8; SD_COMM_ID_BYTES], io::Error> {
        let mut id = [0u8; SD_COMM_ID_BYTES];
        match unsafe { sd_comm_id(id.as_mut_ptr()) } {
            SD_OK => Ok(id),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }
    /// Collective over all ranks (ncclCommInitRank on the context's device).
    pub fn join(id: &[u8; SD_COMM_ID_BYTES], nranks: i32, rank: i32) -> Result<Comm, io::Error> {
        let g = ctx()?;
        let mut p = std::ptr::null_mut();
        match unsafe { sd_comm_create(g.0, id.as_ptr(), nranks, rank, &mut p) } {
            SD_OK => Ok(Comm { raw: p, _group: None }),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }
    /// One rank of an in-process group: the ranks are threads of this process, each with its
    /// own context (`ctx`, e.g. one per device from sd_cas_ctx_create); every collective has
    /// the RCCL communicator's semantics.  The member keeps the group alive: dropping the
    /// `CommGroup` first only releases the caller's handle.
    pub fn join_local(group: &CommGroup, ctx: *mut sd_cas_ctx, rank: i32) -> Result<Comm, io::Error> {
        let mut p = std::ptr::null_mut();
        match unsafe { sd_comm_create_local(ctx, group.0.0, rank, &mut p) } {
            SD_OK => Ok(Comm { raw: p, _group: Some(Arc::clone(&group.0)) }),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }
    pub fn raw(&self) -> *mut sd_comm {
        self.raw
    }
}

impl Drop for Comm {
    fn drop(&mut self) {
        // the communicator first; then the field drops release the group reference
        unsafe { sd_comm_destroy(self.raw) }
    }
}

/// The owned sd_comm_group; destroyed when the group handle and every member are gone.
pub struct GroupHandle(*mut sd_comm_group);
unsafe impl Send for GroupHandle {}
unsafe impl Sync for GroupHandle {}

impl Drop for GroupHandle {
    fn drop(&mut self) {
        unsafe { sd_comm_group_destroy(self.0) }
    }
}

/// The rendezvous of an in-process group of `nranks` ranks (sd_comm_group_create).
pub struct CommGroup(Arc<GroupHandle>);

impl CommGroup {
    pub fn new(nranks: i32) -> Result<CommGroup, io::Error> {
        let mut p = std::ptr::null_mut();
        match unsafe { sd_comm_group_create(nranks, &mut p) } {
            SD_OK => Ok(CommGroup(Arc::new(GroupHandle(p)))),
            _ => Err(io::Error::new(io::ErrorKind::Other, last_error())),
        }
    }
}

