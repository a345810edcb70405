/*
 * sd_cas.h -- C ABI of the MI355X content-addressing library (libsdcas.so).
 *
 * Drop-in boundary for Spacedrive's content-addressing hot path:
 *   generate_cas_id  /root/reference/core/src/object/cas.rs:23
 *       pub async fn generate_cas_id(path: impl AsRef<Path>, size: u64) -> Result<String, io::Error>
 *   file_checksum    /root/reference/core/src/object/validation/hash.rs:10
 *       pub async fn file_checksum(path: impl AsRef<Path>) -> Result<String, io::Error>
 * The Rust signatures stay as they are; a thin shim crate calls these
 * entry points inside tokio::task::spawn_blocking, and a batched sibling replaces the
 * per-file join_all of identifier_job_step (core/src/object/file_identifier/mod.rs:107-134).
 *
 * Conventions:
 *   - plain pointers and sizes only; the caller owns every buffer; nothing is retained
 *     after a call returns (batches are explicit objects the caller destroys);
 *   - every entry point is thread-safe and re-entrant: a context hands each call its own
 *     stream and scratch from an internal pool; no C++ exception crosses the ABI (the
 *     analogue of the reference FFI's panic::catch_unwind fence,
 *     apps/mobile/modules/sd-core/ios/crate/src/lib.rs:36-86);
 *   - return value: SD_OK (0) or a negative sd_rc for the whole call; per-file outcomes go
 *     to an int32 status array (sd_file_status);
 *   - `stream` arguments are hipStream_t passed as void*; NULL is HIP's null (default)
 *     stream, as everywhere in HIP.  Device-pointer entry points only enqueue work on it
 *     and do not synchronise (the dedup calls return host counts and so do sync it);
 *   - the GPU entry points need a gfx950 device (sd_cas_ctx_create fails with SD_ERR_DEVICE
 *     otherwise); the sd_cpu_* entry points are the library's CPU path:
 *     the same results from the host cores, for a node without the device and for the
 *     latency path's single-file callers.  No GPU entry point falls back to them silently;
 *     sd_cas_id_path / sd_file_checksum_path route a call to the CPU by a documented,
 *     tunable policy ("latency_cpu_max") and count it in sd_coalescer_stats.
 *
 * File-read semantics (the reference's, whatever the file's length): a whole-kind cas
 * message is le64(size) || every byte fs::read returns (cas.rs:25,29) -- the file may be
 * shorter or longer than `size`; a sampled message reads head and samples with read_exact
 * at their traced offsets and the tail at seek(End(-8192)), the file's real end (cas.rs:
 * 31-58); a checksum hashes what 1 MiB read calls return until one returns fewer
 * (hash.rs:14-20).
 */
#ifndef SD_CAS_H
#define SD_CAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_CAS_ABI_VERSION 2

/* cas.rs:10-15 */
#define SD_SAMPLE_COUNT 4u
#define SD_SAMPLE_SIZE 10240u
#define SD_HEADER_OR_FOOTER_SIZE 8192u
#define SD_MINIMUM_FILE_SIZE 102400u
/* le64 header + head + 4 samples + tail */
#define SD_SAMPLED_MSG_LEN 57352u
/* sd_cas_stage_plan starts staged messages on this alignment (one 128-byte cache line, so
 * a lane's 2 KiB chunk pair is whole lines) and zero-pads them up to it.  The kernels need
 * only 16-byte aligned offsets (sd_extent.msg_offset) and zero padding to a 64-byte boundary. */
#define SD_STAGE_ALIGN 128u

typedef enum sd_rc {
    SD_OK = 0,
    SD_ERR_INVALID = -1,  /* bad argument (null pointer, misaligned extent, ...) */
    SD_ERR_DEVICE = -2,   /* HIP / device error, or no gfx950 device */
    SD_ERR_NOMEM = -3,    /* device or pinned-host allocation failed */
    SD_ERR_INTERNAL = -4, /* unexpected exception caught at the boundary, or a HIP call
                             attempted on a private-fd-table worker thread */
    SD_ERR_COMM = -5,     /* collective (RCCL) failure */
    SD_ERR_CAPACITY = -6  /* sd_cas_dedup_mgpu: some rank's output capacity is too small (every
                             rank returns it, before the exchange; *m_out = own requirement) */
} sd_rc;

/* per-file status, mapped back to io::ErrorKind by the Rust shim */
typedef enum sd_file_status {
    SD_FILE_OK = 0,
    SD_FILE_SKIPPED_EMPTY = 1, /* FileMetadata::new skips len 0 (file_identifier/mod.rs:80-88) */
    SD_FILE_IO_ERROR = 2,      /* open/read failed: errno in the high 16 bits */
    SD_FILE_SHORT_READ = 3,    /* read_exact hit EOF: io::ErrorKind::UnexpectedEof (cas.rs:36,43,56) */
    SD_FILE_CHANGED = 4        /* staging only (sd_cas_stage_file/_files): the whole-kind file holds
                                  more bytes than its extent's room (it grew since the caller's
                                  stat); the reference hashes them all -- re-stage it with a larger
                                  extent, or use sd_cas_ids_files / sd_cas_id_path, which do */
} sd_file_status;

typedef enum sd_kind {
    SD_KIND_WHOLE = 1,  /* size <= 102400: le64(size) || whole file          (cas.rs:27-29) */
    SD_KIND_SAMPLED = 2 /* size  > 102400: le64(size) || head || 4 samples || tail (cas.rs:30-58) */
} sd_kind;

/* One file of a cas batch: where its hashed message sits in the staged buffer. 24 bytes. */
typedef struct sd_extent {
    uint64_t size;       /* file size as passed to generate_cas_id (hashed as le64)  */
    uint64_t msg_offset; /* byte offset of the message in the staged buffer (16-B aligned) */
    uint32_t msg_len;    /* SAMPLED: 57352; WHOLE: 8 + the bytes staged (planned 8 + size) */
    uint32_t kind;       /* sd_kind                                                  */
} sd_extent;

typedef struct sd_cas_ctx sd_cas_ctx;
typedef struct sd_cas_batch sd_cas_batch;
typedef struct sd_checksum_batch sd_checksum_batch;

/* ---------------------------------------------------------------- context */
int sd_cas_abi_version(void);
/* The host thread budget: the most host threads one call of this
 * process starts -- readers, CPU-path workers and co-hashing threads alike.  Resolved once
 * as min(affinity share, quota share), at least 1: the CPUs in the affinity mask, divided by
 * LOCAL_WORLD_SIZE (the ranks sharing the node's host; 1 when unset) only when the mask holds
 * every CPU of its scope -- the online CPUs, or the cgroup cpuset when that is smaller (a
 * narrower mask is a per-rank binding); and the tightest cgroup CPU quota
 * from the process's cgroup up, rounded up, divided by LOCAL_WORLD_SIZE.  The tuning key
 * "host_cpu_budget" > 0 replaces it.  out[5]: [0] the budget, [1] affinity CPUs, [2] cgroup
 * quota in milli-CPUs (0 = none), [3] LOCAL_WORLD_SIZE, [4] 1 if the tuning key set it. */
int sd_host_cpu_budget(int out[5]);
/* Where the library's own threads run: out[0] = 1 when they are placed on the CPUs of the
 * NUMA node of the first context's device (within each thread's own affinity mask; tuning
 * "numa_pin", default 0 = not placed), out[1] = those CPUs, out[2] = the device's node (-1
 * unknown).  Callers' threads are never moved; with "numa_pin" 0 no thread is. */
int sd_host_numa(int out[3]);
/* last error message of the calling thread ("" if none) */
const char* sd_cas_last_error(void);
int sd_cas_ctx_create(int device, sd_cas_ctx** out);
void sd_cas_ctx_destroy(sd_cas_ctx* ctx);
/* pinned host staging memory (fastest H2D); free with sd_cas_host_free */
int sd_cas_host_alloc(sd_cas_ctx* ctx, uint64_t bytes, void** out);
void sd_cas_host_free(sd_cas_ctx* ctx, void* p);

/* ---------------------------------------------------------------- staging (host) */
/* Layout of the cas messages of n files (cas.rs:25-58): fills extents_out[n] and the
 * staged-buffer size.  Pure host arithmetic; no device needed. */
int sd_cas_stage_plan(const uint64_t* sizes, size_t n, sd_extent* extents_out,
                      uint64_t* total_bytes_out);
/* Shards a library of n files (by global index, as the multi-GPU scan does) over nranks
 * ranks in contiguous index ranges of balanced hashing cost: the cost
 * of a file is the BLAKE3 compressions of its cas message (953 for every sampled file,
 * 1..146 for a small one).  bounds_out[nranks + 1]: rank r hashes [bounds[r], bounds[r+1]),
 * bounds ascending (sd_cas_dedup_mgpu's index-ordered fast path).  Pure host arithmetic. */
int sd_shard_plan(const uint64_t* sizes, size_t n, int nranks, uint64_t* bounds_out);
/* Reads one file into its extent exactly as generate_cas_id does (le64 header, then the
 * whole file until EOF, or head/samples by read_exact and the tail at the file's real end),
 * zero-padding to the next 64-byte boundary.  The extent is in/out: for a whole-kind file
 * msg_len becomes 8 + the bytes read, which may be fewer than planned (the file is shorter
 * than `size`; room = the planned msg_len - 8).  Sets *status to an sd_file_status
 * (SD_FILE_CHANGED when the file holds more than the room); returns SD_OK unless
 * arguments are invalid. */
int sd_cas_stage_file(const char* path, sd_extent* ext, uint8_t* staged, int32_t* status);
/* The same for n files on nthreads threads (the reference does these reads one tokio
 * blocking-pool hop at a time: cas.rs:29-58).  status[n] receives each file's outcome. */
int sd_cas_stage_files(const char* const* paths, sd_extent* extents, size_t n, uint8_t* staged,
                       int32_t* status, int nthreads);

/* ---------------------------------------------------------------- cas ids */
/* Drop-in batch: staged messages in host memory (pinned or pageable) -> n cas_ids as
 * 16 lowercase hex chars + NUL (cas.rs:61), 17 bytes per file.  status may be NULL;
 * entries whose status[i] != SD_FILE_OK on input are skipped and left untouched.  Whole-
 * kind messages of any length are accepted (longer than 8 + 102400 B: hashed by the
 * chunk-parallel checksum kernels).  A call of >= 8192 files is PCIe-bound, and feeding
 * the GPU costs the host only DMA, so "host_cohash_threads" (default 15; 0 = GPU only)
 * host threads hash files from the end of the list on the library's CPU path meanwhile,
 * the GPU taking windows from the front until the two meet; sd_cas_ids_stats counts the
 * files each side hashed. */
int sd_cas_ids_stats(sd_cas_ctx* ctx, uint64_t out[2]); /* files hashed: [0] GPU, [1] host threads */
int sd_cas_ids(sd_cas_ctx* ctx, const uint8_t* staged, uint64_t staged_bytes,
               const sd_extent* extents, size_t n, char* out_hex17, int32_t* status);

/* Path-based drop-in batch (SURVEY.md §8(b)'s "library does pread" entry): n (path,
 * size) pairs -> cas_ids, sizes as the caller's metadata reported them (the size is
 * hashed as given, cas.rs:25).  The library plans the messages, preads them on a
 * persistent pool of nthreads stager threads into pinned windows ("files_window_mb",
 * default 32), and overlaps staging window k+1 with window k's H2D copy and kernels.
 * status[n] (required) receives each file's sd_file_status.  Batch-size policy: a call of
 * at most "batch_cpu_max" files (default 4096; 0 = never) is hashed by
 * sd_cpu_cas_ids_files on nthreads host threads instead, which returns the same ids sooner
 * for an identifier step (100 files: ~0.1 ms vs ~0.3 ms from the page cache). */
int sd_cas_ids_files(sd_cas_ctx* ctx, const char* const* paths, const uint64_t* sizes, size_t n,
                     char* out_hex17, int32_t* status, int nthreads);
/* Calls of sd_cas_ids_files on this context so far: out[0] on the CPU path (batch-size
 * policy), out[1] through the GPU. */
int sd_cas_ids_files_stats(sd_cas_ctx* ctx, uint64_t out[2]);
/* The same, with the full 32-byte hashes left in device memory for a multi-GPU library
 * scan (sd_cas_dedup_mgpu takes them as they are): d_hash32 (device, n x 32 bytes) row i =
 * file i's hash when status[i] == SD_FILE_OK (other rows untouched); d_valid (device, n
 * bytes, may be NULL) = 1 for the files the identifier dedups -- hashed and not empty
 * (file_identifier/mod.rs:80-88).  Returns when the rows are written. */
int sd_cas_hashes_files(sd_cas_ctx* ctx, const char* const* paths, const uint64_t* sizes, size_t n,
                        uint8_t* d_hash32, uint8_t* d_valid, int32_t* status, int nthreads);

/* Prepared batch for device-resident data: builds the work lists for these extents once
 * (host arithmetic + one upload).  extents are host pointers. */
int sd_cas_batch_create(sd_cas_ctx* ctx, const sd_extent* extents, size_t n, sd_cas_batch** out);
void sd_cas_batch_destroy(sd_cas_batch* batch);
/* Enqueue the hashing of a prepared batch: d_staged (device, >= staged size) ->
 * d_hash32 (device, n x 32 bytes: the full BLAKE3 hash; the cas_id is its first 8).
 * The batch holds the device scratch its kernels pass between them (subtree chaining
 * values), so runs of ONE batch must be ordered: the same stream, or an event between
 * streams.  Its sampled and whole parts use separate scratch and may overlap each other
 * (run_part on two streams).  Separate batches are independent. */
int sd_cas_batch_run(sd_cas_ctx* ctx, const sd_cas_batch* batch, const uint8_t* d_staged,
                     uint8_t* d_hash32, void* stream);
/* Same, restricted to one part of the batch (bitmask): SD_PART_SAMPLED runs only the
 * sampled-file kernels, SD_PART_WHOLE only the whole-file kernels (lets a caller time
 * each part with events on `stream`). */
#define SD_PART_SAMPLED 1
#define SD_PART_WHOLE 2
int sd_cas_batch_run_part(sd_cas_ctx* ctx, const sd_cas_batch* batch, int parts, const uint8_t* d_staged,
                          uint8_t* d_hash32, void* stream);
/* Statistics of a prepared batch: [0] files, [1] sampled files, [2] whole files,
 * [3] chunks of whole files, [4] BLAKE3 compressions, [5] message bytes, [6] full-pair
 * and [7] tail work items of the whole-file kernel (its launch shape). */
int sd_cas_batch_stats(const sd_cas_batch* batch, uint64_t out[8]);

/* ---------------------------------------------------------------- checksums */
/* Full-file BLAKE3 (hash.rs:10-24) of n files that are byte ranges of one device
 * buffer.  offsets/lens are HOST arrays; each range must start 16-byte aligned and the
 * buffer must be readable up to the next 64-byte boundary after each range.  Start ranges
 * on SD_STAGE_ALIGN (128 B, a whole cache line) for full speed: a range that starts mid-line
 * hashes about 5% slower (every line-pair load straddles two lines; scripts/ck_align_probe.py). */
int sd_checksum_batch_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens,
                             size_t n, sd_checksum_batch** out);
void sd_checksum_batch_destroy(sd_checksum_batch* batch);
int sd_checksum_batch_run(sd_cas_ctx* ctx, const sd_checksum_batch* batch, const uint8_t* d_data,
                          uint8_t* d_hash32, void* stream);
/* [0] files, [1] total bytes, [2] BLAKE3 compressions, [3] 1 MiB leaf blocks */
int sd_checksum_batch_stats(const sd_checksum_batch* batch, uint64_t out[4]);
/* Drop-in over host memory (pinned or pageable; hash.rs:10-24 on data already read):
 * full BLAKE3 of n byte ranges of `data` -> 65-byte hex each.  Ranges start 16-byte
 * aligned (ranges of 1 MiB or more are placed on 128-B device lines whatever their host
 * start); no page that holds no range byte is read (a range may end where `data` ends, and
 * `data` may have unmapped holes between ranges; bytes between two ranges on a page they
 * share may be copied).  Consecutive ranges are copied 256 MiB window at a time, larger
 * ranges stream; two windows alternate so the H2D copies overlap the kernels.  In calls of
 * >= 1 GiB, "host_cohash_threads" host threads (default 15; 0 = GPU only) hash ranges from
 * the end on the CPU path meanwhile (ranges of >= 8 MiB block-parallel), the GPU taking
 * them from the front until the two meet; one range of >= 256 MiB, the one nearest the
 * predicted meeting point, is shared 1 MiB block by block.  Such a call
 * ("checksum_split_adapt" k > 0, default 8) runs co-hashed or on the CPU path alone
 * (sd_cpu_checksums on the host budget's threads), whichever this context has measured
 * faster: each once (a warm-up call, then a counted one), then the faster by an EWMA of
 * its GB/s, the other every k-th call; results are identical either way (round 6). */
int sd_checksums(sd_cas_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                 char* out_hex65);
/* bytes sd_checksums hashed so far on this context: [0] by the GPU, [1] by host threads --
 * the co-hashing threads, and every byte of a call the learned route sent to the CPU path
 * (their share of a call: the host_share of the bench's with-H2D rows) */
int sd_checksums_stats(sd_cas_ctx* ctx, uint64_t out[2]);
/* what the context learned for sd_checksums' co-hash-eligible calls: [0] the co-hashed
 * call's GB/s, [1] the CPU path's, [2] / [3] how many calls each was counted for */
int sd_checksums_learned(sd_cas_ctx* ctx, double out[4]);
/* Drop-in: checksums of n files on disk -> 65-byte lowercase hex each (hash.rs:21-23);
 * status[n] required.  Each file is read as hash.rs reads it: 1 MiB read calls until a
 * short one -- for a regular file its bytes up to EOF, read with parallel preads
 * ("read_threads"); a pipe or device sequentially.  Small files are packed many per
 * pinned window, large ones (or ones that grow while read) streamed window by window,
 * whatever their final length; two windows alternate so host reads overlap the H2D
 * copies and the kernels (the readers stream each piece through a cache-resident buffer into
 * the pinned window, "checksum_stage_hot" 1).  Batch policy: with "checksum_hybrid_threads"
 * g > 0 (default 6), a call whose regular files of >= 8 MiB add up to >= 512 MiB is split
 * between the GPU and the CPU path on the 16 "read_threads" at once, claimed by 1 MiB blocks
 * ("checksum_split_blocks" 1): a thread that finds one of g GPU slots free reads a run of up
 * to 32 blocks of a file into it (fewer slots under a smaller host budget); otherwise it
 * hashes the small files, then single blocks, on the CPU path; each file's root is merged
 * from both sides' block CVs -- from the page cache 1.13-1.43x the CPU path alone
 * (round 4's whole-file claims, "checksum_split_blocks" 0: 0.9-1.24x).  On a
 * host whose threads hash fast the split can lose to them (0.93x on one box), so by default
 * ("checksum_split_adapt" 8) such a call takes the split or the CPU path alone by the context's
 * recent GB/s of each: each route once, then the faster, the other every 8th call (the
 * routes give identical results).  Any other call of at most "checksum_cpu_max" files is
 * hashed by sd_cpu_file_checksums on "read_threads" threads -- by default every such call,
 * because from the page cache the host's threads hash faster than PCIe can carry the bytes
 * to the GPU; "checksum_cpu_max" 0 = the GPU route alone for every call. */
int sd_file_checksums_stats(sd_cas_ctx* ctx, uint64_t out[2]);  /* calls: [0] CPU path, [1] GPU */
int sd_file_checksums_routes(sd_cas_ctx* ctx, uint64_t out[3]); /* [0] CPU path, [1] GPU, [2] split */
/* bytes (stat lengths) of the files [0] the GPU route hashed (GPU-only and split calls) and
 * [1] the CPU path hashed inside split calls: the split's share on this host */
int sd_file_checksums_bytes(sd_cas_ctx* ctx, uint64_t out[2]);
/* what the context learned for the calls the split applies to ("checksum_split_adapt"):
 * [0] the split's GB/s, [1] the CPU path's (EWMAs of counted calls), [2] / [3] how many
 * calls each was counted for (each route's first call is a warm-up and not counted) */
int sd_file_checksums_learned(sd_cas_ctx* ctx, double out[4]);
int sd_file_checksums(sd_cas_ctx* ctx, const char* const* paths, size_t n, char* out_hex65,
                      int32_t* status);

/* ---------------------------------------------------------------- fingerprints */
/* cas_id AND checksum of files whose bytes are already resident, from one copy of them: what
 * the watcher's inner_update_file computes per file (core/src/location/manager/watcher/
 * utils.rs:393 FileMetadata::new -> generate_cas_id, :438-446 file_checksum on the same path)
 * and what a location that is identified and then validated computes per job.  A gather
 * kernel builds each file's cas message -- le64(size) || file, or le64(size) || head || 4
 * samples || tail (cas.rs:25-58) -- from the file's bytes in device memory into a staged
 * extent; the cas and checksum kernels then run as they are.
 * Semantics: results equal generate_cas_id(path, size) and file_checksum(path) for a file that
 * holds exactly size = lens[i] bytes.  A caller whose metadata size may disagree with the
 * file keeps using the path entries.  Empty ranges are hashed; the caller
 * applies FileMetadata::new's skip of empty files, as with sd_cas_ids. */
typedef struct sd_fingerprint_batch sd_fingerprint_batch;
/* utils.rs:393,438-446 for device-resident files: files = byte ranges of one device buffer
 * (host arrays; starts 16-B aligned, the buffer itself too, readable up to the next 64-byte
 * boundary after each range, as for sd_checksum_batch_create); size hashed = lens[i].  The
 * batch's device scratch (the staged messages) is allocated here, once. */
int sd_fingerprint_batch_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                                sd_fingerprint_batch** out);
void sd_fingerprint_batch_destroy(sd_fingerprint_batch* batch);
/* [0] files [1] sampled [2] whole [3] file bytes [4] staged bytes (the scratch size, what
 * the gather writes into) [5] cas compressions [6] checksum compressions [7] bytes the
 * gather reads */
int sd_fingerprint_batch_stats(const sd_fingerprint_batch* batch, uint64_t out[8]);
/* the extents of the gathered messages: sd_cas_stage_plan's layout for sizes = lens */
int sd_fingerprint_batch_extents(const sd_fingerprint_batch* batch, sd_extent* extents_out /* n */);
/* utils.rs:393's message alone: the gather into the caller's buffer of >= stats[4] bytes
 * (every message and its zero padding up to SD_STAGE_ALIGN; nothing else is written);
 * afterwards sd_cas_batch_run over these extents gives the cas hashes.  Asynchronous. */
int sd_fingerprint_batch_gather(sd_cas_ctx* ctx, const sd_fingerprint_batch* batch, const uint8_t* d_data,
                                uint8_t* d_staged, void* stream);
/* utils.rs:393,438-446: gather into the batch's own scratch + cas kernels + checksum kernels;
 * d_cas_hash32 and d_checksum32 (device) n x 32 B each; asynchronous on stream.  Runs of one
 * batch are ordered (one stream, or an event between streams), as for sd_cas_batch. */
int sd_fingerprint_batch_run(sd_cas_ctx* ctx, const sd_fingerprint_batch* batch, const uint8_t* d_data,
                             uint8_t* d_cas_hash32, uint8_t* d_checksum32, void* stream);
/* Drop-in over host memory (pinned or pageable; utils.rs:393,438-446 on data already read):
 * n ranges of `data` (starts 16-B aligned) -> a 17-byte cas_id hex and a 65-byte checksum hex
 * each, every file byte sent to the device once.  Consecutive ranges that fit a window
 * ("fingerprint_window_mb", default 256) go up together, and one fingerprint batch runs per
 * window; two windows alternate so the copies
 * overlap the kernels.  A range longer than the window streams through the checksum kernels
 * window by window, and the host copies its 57 352-byte cas message (six pieces, ~0.02 % of
 * such a range) into a pinned side list hashed as one ordinary cas batch at the end.  The GPU
 * route only: no host thread co-hashes and no route is learned here -- from files both routes
 * are bound by the reads, and the right policy needs measurements nobody
 * has; sd_cpu_fingerprints is the explicit host sibling.
 * Copies: ranges that ascend in `data` with no whole page between them that holds no range
 * byte keep their relative offsets and go up as ONE H2D per window, starting on a 128-B device
 * line (the bytes between two such neighbours ride along; as in sd_checksums, no page that
 * holds no range byte is read); a range after a hole, or one of 1 MiB or more that would start
 * mid-line, starts a copy of its own on the next 128-B line. */
int sd_fingerprints(sd_cas_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                    char* out_hex17, char* out_hex65);
/* sd_fingerprints on this context so far: [0] bytes sent H2D -- payload: each range's bytes,
 * counted when the range is put into its copy, and each side-list message's 57 352 (not the
 * alignment bytes that ride along between neighbours, nor the plans' tables), so a call adds
 * exactly sum(lens) + 57352 x its large ranges when every byte went up once; [1] files gathered
 * on the device; [2] large ranges (message staged by the host) */
int sd_fingerprints_stats(sd_cas_ctx* ctx, uint64_t out[3]);
/* utils.rs:393,438-446 on host cores, no device: each message built from its range, both
 * hashed by the library's CPU BLAKE3 on nthreads threads */
int sd_cpu_fingerprints(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                        char* out_hex17, char* out_hex65, int nthreads);

/* ---------------------------------------------------------------- latency path */
/* Single-file generate_cas_id (cas.rs:23) / file_checksum (hash.rs:10) for the
 * reference's per-file callers -- the location watcher (core/src/location/manager/
 * watcher/utils.rs:235,393,438-446) and non_indexed::walk (core/src/location/
 * non_indexed.rs:164-187).  Blocking and thread-safe.  Policy: while fewer than
 * "latency_cpu_max" (default 16; 0 = never) single-file calls are in flight on the
 * context, a call is hashed on the calling thread by the CPU path -- one GPU round trip
 * per file costs more than hashing it; beyond that, concurrent calls are coalesced by a
 * dispatcher thread into one batch per window (tuning "coalesce_window_us", default 200,
 * or "coalesce_max" requests, default 4096), handed to sd_cas_ids_files /
 * sd_file_checksums -- whose batch policies route it ("batch_cpu_max",
 * "checksum_cpu_max": with the defaults a coalesced batch is hashed on the CPU path by
 * the dispatcher's 16 threads; with them at 0, on the GPU).  Return SD_OK with *status =
 * sd_file_status (the hex is written only for SD_FILE_OK). */
int sd_cas_id_path(sd_cas_ctx* ctx, const char* path, uint64_t size, char* out_hex17, int32_t* status);
int sd_file_checksum_path(sd_cas_ctx* ctx, const char* path, char* out_hex65, int32_t* status);
/* [0] single-file requests, [1] batches they were coalesced into (each routed by the batch
 * policies), [2] largest batch, [3] requests hashed on their caller's thread (CPU path) */
int sd_coalescer_stats(sd_cas_ctx* ctx, uint64_t out[4]);

/* ---------------------------------------------------------------- CPU path (no device) */
/* The library's own host BLAKE3 (AVX-512 16-lane / AVX2 8-lane / SSE2 4-lane chunk
 * hashing, picked at run time) with the same file-read semantics as the GPU path.  No
 * context needed; nthreads host threads (the caller's included). */
int sd_cpu_simd_lanes(void);
/* sd_cas_ids on the host: staged messages -> 17-byte hex cas_ids (status as sd_cas_ids) */
int sd_cpu_cas_ids(const uint8_t* staged, uint64_t staged_bytes, const sd_extent* extents, size_t n,
                   char* out_hex17, int32_t* status, int nthreads);
/* sd_cas_ids_files on the host: (path, size) pairs -> cas_ids; status[n] required */
int sd_cpu_cas_ids_files(const char* const* paths, const uint64_t* sizes, size_t n, char* out_hex17,
                         int32_t* status, int nthreads);
/* full BLAKE3 of n byte ranges of one host buffer -> 32 raw bytes each (the 1 MiB blocks
 * of a range of >= 8 MiB are tasks of their own when nthreads > 1) */
int sd_cpu_checksums(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                     uint8_t* out_hash32, int nthreads);
/* sd_file_checksums on the host: paths -> 65-byte hex; status[n] required */
int sd_cpu_file_checksums(const char* const* paths, size_t n, char* out_hex65, int32_t* status, int nthreads);
/* one file on the calling thread (the latency path's CPU route) */
int sd_cpu_cas_id_path(const char* path, uint64_t size, char* out_hex17, int32_t* status);
int sd_cpu_file_checksum_path(const char* path, char* out_hex65, int32_t* status);

/* ---------------------------------------------------------------- dedup (post-hash) */
/* Bucket records (cas_id as big-endian u64 of the first 8 hash bytes, global file
 * index) by the top bits of the cas_id for an all-to-all over nparts ranks.
 * d_hash32: n x 32 bytes on device; d_valid: n bytes (0 = skip, e.g. empty files;
 * may be NULL).  Writes d_counts[nparts] (u64) and d_records[n] (2 x u64 each,
 * grouped by destination, stable within a destination).  Returns the number of valid
 * records in *n_valid (host). */
int sd_dedup_partition(sd_cas_ctx* ctx, const uint8_t* d_hash32, const uint8_t* d_valid,
                       uint64_t n, uint64_t global_index_base, int nparts, uint64_t* d_counts,
                       uint64_t* d_records, uint64_t* n_valid, void* stream);
/* Group received records by cas_id: sorts d_records[m] (in place) by (cas_id, index) and
 * writes d_rep[m] (u64): for each record, the smallest global index with an equal
 * cas_id -- the Object-link candidate (file_identifier/mod.rs:168-225 semantics up to
 * the chunk-of-100 rule).  Returns the number of groups.
 * flags: SD_DEDUP_INDEX_SORTED promises the records are already in ascending index
 * order -- true for sd_dedup_partition's output after an all-to-all in rank order over
 * contiguous index shards -- and saves one radix sort. */
#define SD_DEDUP_INDEX_SORTED 1
int sd_dedup_group(sd_cas_ctx* ctx, uint64_t* d_records, uint64_t m, int flags, uint64_t* d_rep,
                   uint64_t* n_groups, void* stream);
/* Object owner per grouped record (d_records / d_rep as sd_dedup_group leaves them), the
 * reference's link-or-create rule for identifier steps of `chunk_size` files
 * (file_identifier/mod.rs:36,136-333): d_owner[i] = index if index / chunk_size ==
 * rep / chunk_size (the group's first step creates an Object per file), else rep (a later
 * step links to it).  Asynchronous on `stream`; no host sync. */
int sd_dedup_owners(sd_cas_ctx* ctx, const uint64_t* d_records, uint64_t m, const uint64_t* d_rep,
                    uint64_t chunk_size, uint64_t* d_owner, void* stream);
/* Confirm candidate groups by full checksum.  A cas_id samples files over 100 KiB
 * (core/src/object/cas.rs:30-58): equal cas_ids mean equal size, head, four samples and tail,
 * not equal bytes; file_checksum (core/src/object/validation/hash.rs:10-24) hashes every byte.
 * d_keys[m]: the cas key of file i (the big-endian u64 of the first 8 cas hash bytes, as in
 * d_records and the index); d_hash32: m x 32 bytes of full checksum per file, 8-byte aligned
 * (what sd_fingerprint_batch_run leaves in d_checksum32); d_valid: m bytes, may be NULL (every
 * file valid), 0 = a file whose checksum could not be computed.  Per valid file i:
 *   group(i) = the valid j with keys[j] == keys[i]
 *   class(i) = the valid j with keys[j] == keys[i] and hash32[j] == hash32[i] over all 32 bytes
 * (equal checksums under different keys are different classes).
 *   d_rep[i]        = the smallest member of class(i)          UINT64_MAX for an invalid file
 *   d_class_size[i] = the size of class(i)                     0
 *   d_verdict[i]    = SD_CONFIRM_SINGLE / _CONFIRMED / _REFUTED   SD_CONFIRM_INVALID
 * An invalid file is never a representative and never counted, even with the smallest index of
 * its key.  Any of the three may be NULL.
 * d_sets_out (3 x u64 per row): one row (key, rep, size) per class of at least 2 members,
 * ascending by key, within a key ascending by the 32 checksum bytes as memcmp compares them;
 * *n_sets (host, may be NULL) = the rows.  If d_sets_out is given and capacity < *n_sets: the
 * call returns SD_ERR_CAPACITY with *n_sets = the requirement and nothing written to
 * d_sets_out; the per-file outputs and stats do not depend on capacity and are written in full
 * then too.  Nothing past the first *n_sets rows is ever written; with d_sets_out NULL the call
 * only counts.
 * stats[8] (host, may be NULL): [0] valid files, [1] groups, [2] candidate groups (at least 2
 * files), [3] classes, [4] confirmed classes (size at least 2; == *n_sets), [5] files in
 * confirmed classes, [6] refuted files, [7] candidate groups that hold at least 2 classes: the
 * cas_ids that lied.  Confirmed redundant files = [5] - [4]; [0] == ([1] - [2]) + [5] + [6] and
 * [3] == ([1] - [2]) + [4] + [6].
 * m == 0 is valid: counts are 0, nothing is written.  A NULL d_keys or d_hash32 with m > 0 is
 * SD_ERR_INVALID.  Runs on `stream` and syncs it; scratch comes from the context's pooled slot
 * (grow-only: 49 bytes per file plus the radix sort's; no allocation in a call whose m fits what
 * the slot holds), so concurrent calls on one context are as safe as sd_dedup_group's.  Not
 * collective: a key lives in one shard of sd_dedup_partition, so per-shard answers concatenate.
 * rep is a position in the call's arrays; the caller maps it to its own file ids.
 * Two paths, equal answers ("confirm_full_sort", sd_cas_set_tuning): a sort by (key, first 8
 * checksum bytes) whose head pass compares the other 24 through the permutation, and, only when
 * some run of equal (key, first 8 bytes) holds unequal tails, a sort over all 40 bytes. */
#define SD_CONFIRM_INVALID   0  /* d_valid[i] == 0: not looked at */
#define SD_CONFIRM_SINGLE    1  /* the only valid file of its key: nothing to confirm */
#define SD_CONFIRM_CONFIRMED 2  /* another valid file has the same key AND the same 32 bytes */
#define SD_CONFIRM_REFUTED   3  /* shares its key with other valid files, its checksum with none */
int sd_dedup_confirm(sd_cas_ctx* ctx, const uint64_t* d_keys, const uint8_t* d_hash32, const uint8_t* d_valid,
                     uint64_t m, uint64_t* d_rep, uint64_t* d_class_size, uint8_t* d_verdict,
                     uint64_t* d_sets_out, uint64_t capacity, uint64_t* n_sets, uint64_t stats[8], void* stream);
/* out[0] = the sd_dedup_confirm calls of this context that finished on the prefix path, out[1] =
 * those that took the full-width path (m == 0 takes neither). */
int sd_dedup_confirm_stats(sd_cas_ctx* ctx, uint64_t out[2]);
/* The same over host arrays, without a context or a device (hash.rs:10-24; cas.rs:30-58). */
int sd_cpu_dedup_confirm(const uint64_t* keys, const uint8_t* hash32, const uint8_t* valid, uint64_t m,
                         uint64_t* rep, uint64_t* class_size, uint8_t* verdict, uint64_t* sets_out,
                         uint64_t capacity, uint64_t* n_sets, uint64_t stats[8]);

/* ---------------------------------------------------------------- Object index */
/* Which Object of the library already owns a cas_id: the join identifier_job_step does per
 * 100-row step through the DB (file_identifier/mod.rs:168-175, `find_many ... cas_id in_vec`)
 * before it links each file to the FIRST such Object (mod.rs:189-225).  The index keeps, on
 * the device, one entry per cas_id key (the big-endian u64 of its first 8 hash bytes = the
 * 16 hex digits read as a number, as in d_records) -> Object id, so a re-scan, a second
 * location, the watcher's single file or a resumed job link to Objects of earlier scans
 * without a DB round trip per step.  Object ids are the host's (the DB's); any u64 is legal.
 * The cycle: scan (sd_dedup_owners_indexed gives owners and the new group heads) -> the host
 * creates those Objects and gives them ids -> insert (key, id) of the new heads.
 * Semantics of insert are KEEP FIRST: an entry the index has wins over any new pair, and
 * among new pairs with equal keys the earliest in the caller's order (DB order) wins -- the
 * first Object, in the order the caller lists them, that owns the cas_id (mod.rs:189-225).
 * An index created for (nparts, part) keeps only the keys sd_dedup_partition sends to rank
 * `part` of `nparts` and skips the others, so every rank can be handed the same DB dump;
 * nparts 1, part 0 = unsharded.  Entries leave through sd_object_index_remove* as the DB's
 * Objects and file_paths do (below), so a live library never rebuilds the index.
 * Thread safety: concurrent sd_object_index_lookup / _count / _export calls on one index are
 * safe; sd_object_index_insert* and sd_object_index_remove* are exclusive (no other call on
 * the index, and no kernel of an earlier call still reading it, while one runs), and
 * sd_dedup_owners_indexed uses scratch owned by the index: one such call in flight per
 * index. */
typedef struct sd_object_index sd_object_index;
int sd_object_index_create(sd_cas_ctx* ctx, int nparts, int part, sd_object_index** out);
void sd_object_index_destroy(sd_object_index* index);
/* m pairs (key, Object id) on the device, in the caller's (DB) order; *taken (host, may be
 * NULL) = the entries added: first of their key, of this shard, and not already present
 * (mod.rs:168-225: the first Object wins).  Runs on `stream` and syncs it; buffers grow
 * (hipMalloc) when the count exceeds their capacity.  m == 0 is a no-op. */
int sd_object_index_insert(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_keys,
                           const uint64_t* d_object_ids, uint64_t m, uint64_t* taken, void* stream);
/* The same from host memory: hex17 = m x 17 bytes, each a 16-digit lower-case hex cas_id
 * and a NUL (what sd_cas_ids writes; mod.rs:168-175 reads the same strings from the DB). */
int sd_object_index_insert_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* hex17,
                               const uint64_t* object_ids, uint64_t m, uint64_t* taken);
/* Removal.  The reference takes Objects and their cas_ids away all the time: the orphan
 * remover deletes every Object without a file_path, 512 per query
 * (core/src/object/orphan_remover.rs:57-95); deleting a file takes a file_path from its
 * Object; a content change moves a file_path from cas_id A to B on the same Object
 * (core/src/location/manager/watcher/utils.rs:410-494).  After a removal the index is
 * bit-identical to a fresh one built from the surviving entries with the same (nparts,
 * part): the same keys and ids in ascending key order, the same count, the directory bits
 * re-chosen for the new count and the directory rebuilt.  Buffers never shrink.
 * Both calls: *removed (host, may be NULL) = the entries dropped; d_removed_out (device, may
 * be NULL; `capacity` entries of 2 x u64) receives (key, Object id) of each dropped entry in
 * ascending key order, so the host can ask the DB who else owns those cas_ids; nothing past
 * the first *removed entries is written.  If d_removed_out is given and `capacity` is
 * smaller than the count, the call returns SD_ERR_CAPACITY with *removed = the requirement
 * and the index (and d_removed_out) unchanged.  They run on `stream` and sync it, are
 * exclusive on the index as insert is, and are not collective: a sharded index drops what
 * it holds, so every rank can be handed the same list.  m == 0 is a no-op; after a removal
 * that empties the index, lookups miss everything and insert works.
 * By key (watcher/utils.rs:410-494; a deleted file_path): entry (k, v) goes iff some pair i
 * has d_keys[i] == k and either d_object_ids == NULL or d_object_ids[i] == v -- "drop A -> O
 * only if the index still says O", without a lookup round trip.  Repeated keys, absent keys,
 * keys of other shards and pairs whose id does not match are no-ops. */
int sd_object_index_remove(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_keys,
                           const uint64_t* d_object_ids, uint64_t m, uint64_t* d_removed_out, uint64_t capacity,
                           uint64_t* removed, void* stream);
/* By Object (orphan_remover.rs:57-95; its batch is 512 ids, :62): every entry whose Object
 * id is among the m ids goes.  One Object may own several keys after watcher updates; any
 * u64 is a legal id; repeated and absent ids are no-ops. */
int sd_object_index_remove_objects(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_object_ids,
                                   uint64_t m, uint64_t* d_removed_out, uint64_t capacity, uint64_t* removed,
                                   void* stream);
/* sd_object_index_remove from the DB's strings (hex17 as sd_object_index_insert_hex takes
 * it; watcher/utils.rs:410-494 holds the old cas_id as such a string); object_ids on the
 * host, may be NULL. */
int sd_object_index_remove_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* hex17,
                               const uint64_t* object_ids, uint64_t m, uint64_t* removed);
int sd_object_index_count(const sd_object_index* index, uint64_t* n);
/* d_found[i] (u8) = 1 and d_object_ids[i] = the Object id if d_keys[i] is in the index, else
 * 0 and 0 (mod.rs:168-175 for m keys in any order).  Asynchronous on `stream`. */
int sd_object_index_lookup(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys, uint64_t m,
                           uint64_t* d_object_ids, uint8_t* d_found, void* stream);
/* The index's entries in ascending key order into device arrays of `capacity` entries
 * (SD_ERR_CAPACITY if smaller than the count).  Asynchronous on `stream`. */
int sd_object_index_export(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t* d_keys_out,
                           uint64_t* d_object_ids_out, uint64_t capacity, void* stream);
/* The OWNERS MODE: every owner of a cas_id and its link count.  The one entry per cas_id
 * above cannot tell whether another Object, or another file_path of the same Object, still
 * owns a cas_id after a file_path goes, so its host asks the DB for "the remaining owners"
 * after every deletion, content change and orphan pass.  Duplicates inside one 100-row step
 * each get an Object of their own (mod.rs:229-333) and every later duplicate links to an
 * existing Object (mod.rs:189-225), so both cases are the normal ones.  An owners-mode index
 * holds one entry per (cas_id, Object) pair with the number of file_paths that link them;
 * deleting a file_path takes one link, the entry leaves at zero, and the next owner becomes
 * the answer by itself.  The cycle: scan (sd_dedup_owners_indexed / sd_cas_dedup_mgpu_indexed
 * as above; the host creates the new heads' Objects) -> ONE insert of (key, Object id) for
 * EVERY record of the scan, linked and created alike; a file_path (c, O) deleted -> remove of
 * the pair (c, O) with the id given; a file_path changed A -> B on O -> remove (A, O), insert
 * (B, O), or both in one sd_object_index_apply (below); the orphan remover -> sd_object_index_remove_objects(ids),
 * or, without its DB scan, sd_object_index_orphans over the Objects of the pairs that left (below).  No DB query for owners.
 * Opting in: sd_object_index_create_ex(ctx, nparts, part, flags, &index) with
 *   SD_OBJECT_INDEX_OWNERS (1); flags 0 is sd_object_index_create.  sd_object_index_flags
 *   (index, &flags) reads the mode back.  An index made without the flag behaves bit for bit
 *   as described above.
 * Layout: three arrays plus the directory.  keys[n] ascending, no longer strictly; vals[n]
 *   Object ids, strictly ascending (unsigned) within equal keys; links[n] u64 >= 1; the same
 *   prefix directory over keys.  THE FIRST OWNER OF A KEY IS ITS SMALLEST OBJECT ID: the
 *   reference's existing_objects.iter().find(..) over a find_many in id order (mod.rs:168-210).
 *   sd_object_index_lookup, sd_dedup_owners_indexed and sd_cas_dedup_mgpu_indexed answer with
 *   that entry, by the same rule as in the first mode.
 * insert (m pairs): each pair of this shard adds one link to (k, v); the entry is created at
 *   1 if absent.  Repeated pairs in one call add up.  *taken = entries created.  The order of
 *   the pairs does not matter.
 * remove with ids: each pair takes one link from (k, v).  Pairs naming one entry add up.  An
 *   entry asked for at least as many links as it has is dropped; asking for more is not an
 *   error.  Absent pairs, keys of other shards, and a present key with another id are no-ops.
 * remove with d_object_ids == NULL: every entry of each listed key goes.
 * remove_objects: every entry whose id is listed goes, whatever its links.
 * Outputs of all three removals: d_removed_out receives (key, id) of each dropped entry in
 *   ascending (key, id) order; *removed = dropped entries.  On SD_ERR_CAPACITY nothing
 *   changes, the link counts of entries that would have survived included; *removed = the
 *   requirement.  After any removal the index is bit-identical to a fresh owners-mode index
 *   built from the surviving links.
 * sd_object_index_export and _count report entries (pairs); _insert_hex / _remove_hex follow
 * the mode.  Memory: 24 bytes per entry, one entry per pair. */
#define SD_OBJECT_INDEX_OWNERS 1
int sd_object_index_create_ex(sd_cas_ctx* ctx, int nparts, int part, int flags, sd_object_index** out);
int sd_object_index_flags(const sd_object_index* index, int* flags);
/* New reads of an owners-mode index, asynchronous on `stream`; both return SD_ERR_INVALID on
 * an index without the flag, and both may run concurrently with the other reads, as
 * sd_object_index_lookup may.  d_links_out[i] = the link count of the pair (d_keys[i],
 * d_object_ids[i]), 0 if absent. */
int sd_object_index_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys,
                          const uint64_t* d_object_ids, uint64_t m, uint64_t* d_links_out, void* stream);
/* The entries in ascending (key, id) order with their link counts, into device arrays of
 * `capacity` entries (SD_ERR_CAPACITY if smaller than the count). */
int sd_object_index_export_links(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t* d_keys_out,
                                 uint64_t* d_ids_out, uint64_t* d_links_out, uint64_t capacity, void* stream);
/* APPLY: "these links went, these links came" in one call, for an owners-mode index only.  A
 * content change moves a file_path from cas_id A to B on its Object (watcher/utils.rs:410-494),
 * a re-identified location and a burst of watcher events produce pairs that leave and pairs
 * that enter together; remove then insert rewrites the index twice and shows concurrent
 * lookups a state between the two.  For every pair p = (key, id) of this shard, with held(p)
 * its links before the call (0 if absent), asked(p) its multiplicity in the removal list and
 * added(p) its multiplicity in the insertion list:
 *   kept(p)  = 0 if held(p) == 0 or asked(p) >= held(p) > 0 with asked(p) > 0, else held(p) - asked(p)
 *   after(p) = kept(p) + added(p)
 * which is what sd_object_index_remove with ids followed by sd_object_index_insert leaves:
 * asking for more than held is not an error, the removals apply before the insertions, the
 * order inside each list does not matter.  After the call the index is bit-identical to a
 * fresh owners-mode index holding the `after` relation (ascending (key, id), the same count,
 * directory bits re-chosen, directory rebuilt), and to a twin given the two calls.
 * Reports, of the NET effect (not the two calls' counters): *removed (host, may be NULL) = the
 *   entries present before and absent after; d_removed_out (device, may be NULL; `capacity`
 *   rows of 2 x u64) receives their (key, id) in ascending (key, id) order, nothing past the
 *   first *removed rows; *taken (host, may be NULL) = the entries absent before and present
 *   after.  A pair whose last link is taken and that gains a link in the same call stays with
 *   links = added and counts in neither.
 * Pairs of other shards, absent pairs in the removal list and a present key with another id
 *   are no-ops.  m_rm == 0 is an insert, m_in == 0 a removal with ids, both 0 a no-op.
 *   d_rm_ids == NULL with m_rm > 0 is SD_ERR_INVALID (every owner of a key: sd_object_index_remove),
 *   and so is an index without SD_OBJECT_INDEX_OWNERS.
 * If d_removed_out is given and capacity < *removed: SD_ERR_CAPACITY, *removed = the
 *   requirement, *taken = 0, and nothing changes: no entry, no link count, no new pair.
 * Exclusive on the index, runs on `stream` and syncs it, grows the buffers as insert does; not
 * collective.  When nothing leaves or enters only the link counts change, in place.
 * sd_object_index_apply_hex: both lists from the DB's strings (hex17 as
 * sd_object_index_insert_hex takes it) and host ids; a malformed cas_id in either list is
 * SD_ERR_INVALID with nothing changed. */
int sd_object_index_apply(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_rm_keys,
                          const uint64_t* d_rm_ids, uint64_t m_rm, const uint64_t* d_in_keys,
                          const uint64_t* d_in_ids, uint64_t m_in, uint64_t* d_removed_out, uint64_t capacity,
                          uint64_t* removed, uint64_t* taken, void* stream);
int sd_object_index_apply_hex(sd_cas_ctx* ctx, sd_object_index* index, const char* rm_hex17, const uint64_t* rm_ids,
                              uint64_t m_rm, const char* in_hex17, const uint64_t* in_ids, uint64_t m_in,
                              uint64_t* removed, uint64_t* taken);
/* THE VIEW BY OBJECT of an owners-mode index: per-Object link totals and orphan detection.  The
 * orphan remover asks the DB, every minute and after every delete job, which Objects have no
 * file_path any more: `object().find_many(vec![object::file_paths::none(vec![])]).take(512)` in
 * a loop (core/src/object/orphan_remover.rs:57-95), a scan of the Object table against
 * file_path.  In the owners mode the answer is a property of the index: an Object whose pairs
 * have all left has no entry.  For an Object id o and one index (one shard), ids compared
 * unsigned:
 *   entries(o) = the number of entries whose Object id is o
 *   links(o)   = the sum of their link counts, in u64
 *   o is unowned in this shard iff entries(o) == 0
 * Both calls take m ids on the device, in any order, repeats allowed; the id of element j is
 * d_object_ids[j * id_stride].  id_stride is in u64 units and is 1 or 2 (anything else is
 * SD_ERR_INVALID): stride 2 reads the id column of (key, id) rows, so a caller passes
 * d_removed_out + 1 of sd_object_index_apply / _remove / _remove_objects and the candidates never
 * leave the device.  Any u64 is a legal id.  m == 0 and an empty index are valid: with m == 0
 * nothing is written and *count = 0; on an empty index every total is 0 and every distinct id an
 * orphan.  An index without SD_OBJECT_INDEX_OWNERS is SD_ERR_INVALID.
 * Both only read the index and may run beside sd_object_index_lookup / _links / _export*,
 * sd_dedup_owners_indexed and sd_cas_dedup_mgpu_indexed (they share no buffer with those); they
 * are exclusive with insert, remove and apply, as every read is.  Unlike lookups they are NOT
 * free to run beside each other: they sort the ids and keep their totals in scratch owned by the
 * index, so ONE call by Object (or of the view by key below, which shares that scratch) is in
 * flight per index.  sd_object_index_object_links is
 * asynchronous: the next call by Object on that index goes to the same stream or waits for it;
 * nothing checks this.
 * Neither is collective: on a sharded index each rank answers for its shard; the host adds the
 * links and entries rows across ranks, and an id is an orphan iff every shard lists it.
 * The limit: the index knows only links that have a cas_id.  An empty file has no cas_id
 * (file_identifier/mod.rs:80-88) and still gets an Object (mod.rs:233-333), so the host keeps,
 * per Object, the count of its file_paths without a cas_id and deletes an Object iff the index
 * lists it as an orphan AND that count is zero.
 * sd_object_index_object_links (orphan_remover.rs:57-95): d_links_out[j] = links(id j),
 *   d_entries_out[j] = entries(id j); either output may be NULL.  Asynchronous on `stream`. */
int sd_object_index_object_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_object_ids,
                                 uint64_t id_stride, uint64_t m, uint64_t* d_links_out, uint64_t* d_entries_out,
                                 void* stream);
/* sd_object_index_orphans (orphan_remover.rs:57-95): the DISTINCT listed ids that have no entry
 *   in this index, ascending (unsigned), into d_orphans_out (device, may be NULL; `capacity`
 *   u64); *count (host, may be NULL) = how many.  If d_orphans_out is given and `capacity` is
 *   smaller than the count: SD_ERR_CAPACITY with *count = the requirement and nothing written to
 *   d_orphans_out (the convention of d_removed_out).  Nothing past the first *count elements is
 *   written.  Runs on `stream` and syncs it. */
int sd_object_index_orphans(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_object_ids,
                            uint64_t id_stride, uint64_t m, uint64_t* d_orphans_out, uint64_t capacity,
                            uint64_t* count, void* stream);
/* THE VIEW BY KEY of an owners-mode index: the duplicate groups per cas_id.  The reference plans
 * a duplicate finder and has not built it (a disabled "Duplicates" sidebar entry,
 * interface/app/$libraryId/Layout/Sidebar/Contents.tsx:58-62; an empty guide,
 * docs/product/guides/discover-duplicates.mdx; docs/changelog/alpha/0.1.0.mdx:45); against its DB
 * the question is a GROUP BY cas_id HAVING COUNT(*) > 1 over file_path, whose cas_id has no
 * index (core/prisma/schema.prisma:162, :196-199).  In the owners mode the answer is a property
 * of the index: entries with equal keys are adjacent.  Both kinds of duplicate are there:
 * same-step duplicates each get an Object (file_identifier/mod.rs:229-333), so one cas_id has
 * several owners; later duplicates link to an existing Object (mod.rs:189-225), so one pair
 * carries several links.  For one index (one shard) and a key k that has at least one entry:
 *   owners(k) = the number of entries with key k
 *   links(k)  = the sum of their link counts, in u64
 *   first(k)  = the smallest Object id among them (what sd_object_index_lookup answers with)
 *   k QUALIFIES under (min_links, min_owners) iff links(k) >= min_links and owners(k) >=
 *   min_owners; 0 means 1 for both, so every key qualifies.
 * min_links = 2 selects content that more than one file_path has; min_owners = 2 selects content
 * split over several Objects, the merge candidates of mod.rs:229-333.
 * An index without SD_OBJECT_INDEX_OWNERS, an index of another context and a NULL d_keys with
 * m > 0 are SD_ERR_INVALID.  m == 0 and an empty index are valid: counts are 0, stats all 0,
 * nothing is written.  All four only read the index: they are exclusive with insert, remove and
 * apply, as every read is.  sd_object_index_key_links needs no scratch and may run beside every
 * other read.  The three group calls keep their group totals in scratch owned by the index,
 * shared with the calls by Object above: ONE call by Object or of this view is in flight per
 * index (the next goes to the same stream or waits; nothing checks this); beside lookups,
 * _links, _export*, _key_links and sd_dedup_owners_indexed they are free to run.  That scratch
 * is grow-only: 18 bytes per entry and 17 KiB (never more than 32 bytes per entry above 1300
 * entries).
 * None is collective.  sd_dedup_partition's destination is monotone in the key, so the shards'
 * groups are disjoint and the shards' rows concatenated in rank order are the library's answer,
 * still ascending; stats rows add up over shards ([7] takes the maximum); key_links rows add up
 * (a key lives in one shard).
 * The limits: a cas_id samples files over 100 KiB (core/src/object/cas.rs:30-58), so a group is
 * a candidate set until sd_dedup_confirm (or sd_cpu_dedup_confirm, over sd_file_checksums'
 * output) has split it by full checksum; the index knows no paths and no sizes (the
 * host joins them from the DB by cas_id: the key's 16 hex digits); files without a cas_id are
 * invisible.
 * sd_object_index_key_links (mod.rs:189-225, :229-333): per listed key (any order, repeats
 *   allowed) d_links_out[j] = links(k), d_owners_out[j] = owners(k); 0 and 0 for a key the index
 *   does not hold (absent, or of another shard).  Either output may be NULL.  Asynchronous. */
int sd_object_index_key_links(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_keys, uint64_t m,
                              uint64_t* d_links_out, uint64_t* d_owners_out, void* stream);
/* sd_object_index_duplicates (mod.rs:189-225, :229-333): one row per qualifying key, ascending:
 *   key, first(k), links(k), owners(k) (device, `capacity` u64 each; each may be NULL); *count
 *   (host, may be NULL) = the qualifying keys.  If any output is given and `capacity` is smaller
 *   than the count: SD_ERR_CAPACITY with *count = the requirement and nothing written.  Nothing
 *   past the first *count rows is ever written; with every output NULL the call only counts.
 *   Runs on `stream` and syncs it. */
int sd_object_index_duplicates(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t min_links, uint64_t min_owners,
                               uint64_t* d_keys_out, uint64_t* d_first_out, uint64_t* d_links_out,
                               uint64_t* d_owners_out, uint64_t capacity, uint64_t* count, void* stream);
/* sd_object_index_duplicate_entries (mod.rs:189-225, :229-333): the ENTRIES of the qualifying
 *   keys, ascending (key, id), with their link counts: the members of each duplicate group.
 *   sd_object_index_export_links filtered; with (0, 0) equal to it, row for row.  *count = the
 *   entries; outputs, capacity and sync as sd_object_index_duplicates. */
int sd_object_index_duplicate_entries(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t min_links,
                                      uint64_t min_owners, uint64_t* d_keys_out, uint64_t* d_ids_out,
                                      uint64_t* d_links_out, uint64_t capacity, uint64_t* count, void* stream);
/* sd_object_index_duplicate_stats (mod.rs:189-225, :229-333): out[8] (host): [0] keys, [1]
 *   entries, [2] links, [3] keys with links(k) >= 2, [4] the links of those keys, [5] keys with
 *   owners(k) >= 2, [6] the entries of those keys, [7] the largest links(k) (0 on an empty
 *   index).  Redundant file_paths = [4] - [3]; surplus Objects = [6] - [5].  Runs on `stream` and
 *   syncs it. */
int sd_object_index_duplicate_stats(sd_cas_ctx* ctx, const sd_object_index* index, uint64_t out[8], void* stream);
/* MERGE OBJECTS: "Object `from` IS Object `to`", the step that acts on the view by key.  Same-step
 * duplicates each get an Object (file_identifier/mod.rs:229-333), so one cas_id ends up split over
 * several; sd_object_index_duplicate_entries(0, 2) lists those entries and sd_dedup_confirm says
 * which are safe to act on.  Without this call the host exports B's entries, calls
 * sd_object_index_remove_objects(B) and re-inserts every (key, A) pair once per link: two rewrites
 * with a host round trip between them, and lookups see a state in which B's content belongs to
 * nobody.  The m pairs (d_from[j], d_to[j]) -- device, ids compared unsigned, any u64 legal --
 * define phi(v) = d_to[j] if some d_from[j] == v, else v.  phi is applied ONCE and SIMULTANEOUSLY
 * to the ids as they stand before the call: a -> b with b -> c sends a's entries to b and b's to
 * c, a -> b with b -> a is a swap; resolving chains is the host's job (spacedrive_amd.dedup.merge_map
 * does it).  Repeated identical pairs, pairs with from == to and `from` ids the index (this shard)
 * does not hold are no-ops.  One `from` with two different `to` is a contradiction ((a -> a) with
 * (a -> b) counts as one): SD_ERR_INVALID, the index bit-unchanged.
 *   Owners mode: after(k, w) = the sum, in u64, of links(k, v) over every v with phi(v) = w; an
 *   entry exists iff that sum is >= 1.  After the call the index is bit-identical to a fresh
 *   owners-mode index of the same (nparts, part) built from `after`: ascending (key, id), the same
 *   count, directory bits re-chosen, directory rebuilt.  Keys never change; entries move only
 *   inside their key's run, and entries of one key that now share an id coalesce into one.
 *   First mode: one entry per key, so vals[i] = phi(vals[i]) in place; count, keys and directory
 *   stand.
 * Reports (host, each may be NULL): *moved = the entries, counted before the call, whose id phi
 *   changes; *coalesced = the count before less the count after (0 in the first mode).  When
 *   *moved == 0 nothing is written and no buffer is swapped.
 * Exclusive on the index, as apply is; runs on `stream` and syncs it; grows the index's scratch,
 * never its buffers (the count cannot grow).  Not collective: every shard may be handed the same
 * map, and moved and coalesced add up over the shards.  m == 0 and an empty index are valid
 * no-ops (a contradiction is refused on an empty index too).  A NULL d_from or d_to with m > 0 and
 * an index of another context are SD_ERR_INVALID before anything is launched.  There is no row
 * output and so no capacity: the merged-away Objects are the caller's d_from, and
 * sd_object_index_orphans(d_from, ...) after the call lists exactly those that no longer own
 * anything (the limit stated there applies: file_paths without a cas_id). */
int sd_object_index_merge_objects(sd_cas_ctx* ctx, sd_object_index* index, const uint64_t* d_from,
                                  const uint64_t* d_to, uint64_t m, uint64_t* moved, uint64_t* coalesced,
                                  void* stream);
/* sd_dedup_owners against the Objects the library already has (mod.rs:168-225, then
 * :229-333 for the rest), per grouped record i:
 *   d_owner[i] = index[cas_id], d_existing[i] = 1     if the index has the record's cas_id;
 *   d_owner[i] = what sd_dedup_owners writes (a file index), d_existing[i] = 0   otherwise.
 * d_new_out (2 x u64 per entry, capacity m) receives (key, smallest file index) of every
 * group the index does not have, in ascending key order, and *d_n_new (device u64) their
 * count: the Objects the host creates, names and inserts.  Only the first *d_n_new entries
 * of d_new_out are defined.  index == NULL is sd_dedup_owners itself (d_existing,
 * d_new_out and d_n_new are not touched and may be NULL).  Asynchronous on `stream`; no
 * host sync. */
int sd_dedup_owners_indexed(sd_cas_ctx* ctx, const sd_object_index* index, const uint64_t* d_records, uint64_t m,
                            const uint64_t* d_rep, uint64_t chunk_size, uint64_t* d_owner, uint8_t* d_existing,
                            uint64_t* d_new_out, uint64_t* d_n_new, void* stream);
/* The host-only siblings, over host arrays, for a host without a gfx950 device: the same
 * semantics, layout and directory (mod.rs:168-225).  sd_cpu_dedup_owners_indexed takes
 * *n_new on the host; the removals (orphan_remover.rs:57-95, watcher/utils.rs:410-494) take
 * removed_out / capacity / removed on the host. */
typedef struct sd_cpu_object_index sd_cpu_object_index;
int sd_cpu_object_index_create(int nparts, int part, sd_cpu_object_index** out);
void sd_cpu_object_index_destroy(sd_cpu_object_index* index);
int sd_cpu_object_index_insert(sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids,
                               uint64_t m, uint64_t* taken);
int sd_cpu_object_index_remove(sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids,
                               uint64_t m, uint64_t* removed_out, uint64_t capacity, uint64_t* removed);
int sd_cpu_object_index_remove_objects(sd_cpu_object_index* index, const uint64_t* object_ids, uint64_t m,
                                       uint64_t* removed_out, uint64_t capacity, uint64_t* removed);
int sd_cpu_object_index_lookup(const sd_cpu_object_index* index, const uint64_t* keys, uint64_t m,
                               uint64_t* object_ids, uint8_t* found);
int sd_cpu_object_index_count(const sd_cpu_object_index* index, uint64_t* n);
int sd_cpu_object_index_export(const sd_cpu_object_index* index, uint64_t* keys_out, uint64_t* object_ids_out,
                               uint64_t capacity);
/* The owners mode of the host twin: the same flag, semantics and layout as
 * sd_object_index_create_ex / _flags / _links / _export_links, over host arrays; the other
 * sd_cpu_object_index_* calls follow the mode. */
int sd_cpu_object_index_create_ex(int nparts, int part, int flags, sd_cpu_object_index** out);
int sd_cpu_object_index_flags(const sd_cpu_object_index* index, int* flags);
int sd_cpu_object_index_links(const sd_cpu_object_index* index, const uint64_t* keys, const uint64_t* object_ids,
                              uint64_t m, uint64_t* links_out);
int sd_cpu_object_index_export_links(const sd_cpu_object_index* index, uint64_t* keys_out, uint64_t* ids_out,
                                     uint64_t* links_out, uint64_t capacity);
/* sd_object_index_apply over host arrays: the same rule, reports and refusals. */
int sd_cpu_object_index_apply(sd_cpu_object_index* index, const uint64_t* rm_keys, const uint64_t* rm_ids,
                              uint64_t m_rm, const uint64_t* in_keys, const uint64_t* in_ids, uint64_t m_in,
                              uint64_t* removed_out, uint64_t capacity, uint64_t* removed, uint64_t* taken);
/* sd_object_index_object_links / _orphans over host arrays (orphan_remover.rs:57-95): the same
 * rule, strides, reports and refusals. */
int sd_cpu_object_index_object_links(const sd_cpu_object_index* index, const uint64_t* object_ids,
                                     uint64_t id_stride, uint64_t m, uint64_t* links_out, uint64_t* entries_out);
int sd_cpu_object_index_orphans(const sd_cpu_object_index* index, const uint64_t* object_ids, uint64_t id_stride,
                                uint64_t m, uint64_t* orphans_out, uint64_t capacity, uint64_t* count);
/* sd_object_index_key_links / _duplicates / _duplicate_entries / _duplicate_stats over host arrays
 * (mod.rs:189-225, :229-333): the same rule, reports and refusals. */
int sd_cpu_object_index_key_links(const sd_cpu_object_index* index, const uint64_t* keys, uint64_t m,
                                  uint64_t* links_out, uint64_t* owners_out);
int sd_cpu_object_index_duplicates(const sd_cpu_object_index* index, uint64_t min_links, uint64_t min_owners,
                                   uint64_t* keys_out, uint64_t* first_out, uint64_t* links_out, uint64_t* owners_out,
                                   uint64_t capacity, uint64_t* count);
int sd_cpu_object_index_duplicate_entries(const sd_cpu_object_index* index, uint64_t min_links, uint64_t min_owners,
                                          uint64_t* keys_out, uint64_t* ids_out, uint64_t* links_out,
                                          uint64_t capacity, uint64_t* count);
int sd_cpu_object_index_duplicate_stats(const sd_cpu_object_index* index, uint64_t out[8]);
/* sd_object_index_merge_objects over host arrays (mod.rs:229-333): the same rule, reports and
 * refusals. */
int sd_cpu_object_index_merge_objects(sd_cpu_object_index* index, const uint64_t* from, const uint64_t* to,
                                      uint64_t m, uint64_t* moved, uint64_t* coalesced);
int sd_cpu_dedup_owners_indexed(const sd_cpu_object_index* index, const uint64_t* records, uint64_t m,
                                const uint64_t* rep, uint64_t chunk_size, uint64_t* owner, uint8_t* existing,
                                uint64_t* new_out, uint64_t* n_new);

/* ---------------------------------------------------------------- multi-GPU dedup (RCCL) */
/* One process (or thread) per GPU, files sharded by global index.  The
 * communicator is RCCL's: rank 0 calls sd_comm_id (ncclGetUniqueId) and hands the 128
 * bytes to every rank out of band; each rank calls sd_comm_create (ncclCommInitRank,
 * collective) on its context's device. */
#define SD_COMM_ID_BYTES 128
typedef struct sd_comm sd_comm;
int sd_comm_id(uint8_t* out_id /* SD_COMM_ID_BYTES */);
int sd_comm_create(sd_cas_ctx* ctx, const uint8_t* id, int nranks, int rank, sd_comm** out);
void sd_comm_destroy(sd_comm* comm);
/* In-process communicator: the ranks are threads of ONE process (each with its own context,
 * on one device or several) that share an sd_comm_group.  Every collective below has the
 * same semantics over it; the exchange is device-to-device copies between the ranks'
 * buffers, ordered by a host barrier (a rank whose thread never arrives makes its peers
 * return SD_ERR_COMM after 120 s).  For a host that drives several GPUs from one process,
 * and for rehearsing N ranks on one GPU, which RCCL refuses.  Destroy every member comm
 * before the group. */
typedef struct sd_comm_group sd_comm_group;
int sd_comm_group_create(int nranks, sd_comm_group** out);
void sd_comm_group_destroy(sd_comm_group* group);
int sd_comm_create_local(sd_cas_ctx* ctx, sd_comm_group* group, int rank, sd_comm** out);
/* The whole post-hash step of one rank, collective over the communicator: partition its n
 * records by cas_id prefix (sd_dedup_partition), all-gather the count matrix and the
 * shards' index ranges (ncclAllGather), exchange the 16-byte records with grouped
 * ncclSend / ncclRecv -- the all-to-all over xGMI --, then group the records this rank
 * receives (sd_dedup_group; index order is exploited when the shards' ranges ascend with
 * the rank) and assign their Objects (sd_dedup_owners, identifier steps of chunk_size).
 * Outputs hold `capacity` entries: d_records_out 2 x u64 each (sorted by (cas_id,
 * index)), d_rep_out and d_owner_out u64 each; *m_out = the records this rank owns,
 * *n_groups_out = its groups.  If any rank's capacity is too small, every rank returns
 * SD_ERR_CAPACITY before the record exchange, with *m_out = its own requirement (and
 * SD_ERR_INTERNAL together if any rank's partition counts disagree with its valid records:
 * the gathered rows carry both, so no rank is left waiting in the exchange).  Runs on
 * `stream`; returns after the group counts are known (host sync).  Over RCCL, each wait for
 * the peers is bounded by the tuning key "comm_timeout_ms" (300 000; 0 = unbounded): a peer
 * that died or hung, or an RCCL asynchronous error, makes the call return SD_ERR_COMM naming
 * the step, and the communicator is broken from then on -- later calls on it return
 * SD_ERR_COMM, and sd_comm_destroy releases nothing of it (work may still be queued against
 * it; the host is expected to exit).  Overlapping it with the
 * next batch's hashing (a second stream) pays only with the hashing stream at the higher
 * priority (107.5 vs 103.9-104.3 M files/s with equal priorities). */
int sd_cas_dedup_mgpu(sd_cas_ctx* ctx, sd_comm* comm, const uint8_t* d_hash32, const uint8_t* d_valid, uint64_t n,
                      uint64_t global_index_base, uint64_t chunk_size, uint64_t* d_records_out, uint64_t* d_rep_out,
                      uint64_t* d_owner_out, uint64_t capacity, uint64_t* m_out, uint64_t* n_groups_out,
                      void* stream);
/* sd_cas_dedup_mgpu with its last step's owners taken through this rank's Object index
 * (sd_dedup_owners_indexed; file_identifier/mod.rs:168-225): d_existing_out (u8) and d_new_out
 * (2 x u64) hold `capacity` entries, *n_new_out (host) = the new heads.  The index must have
 * been created on `ctx` for (nparts, part) = the communicator's (nranks, rank); if any rank's
 * is not, EVERY rank returns SD_ERR_INVALID before any record moves (the gathered rows carry
 * it, as they carry the capacities).  index == NULL: sd_cas_dedup_mgpu itself (the three
 * extra outputs are not touched and may be NULL). */
int sd_cas_dedup_mgpu_indexed(sd_cas_ctx* ctx, sd_comm* comm, const uint8_t* d_hash32, const uint8_t* d_valid,
                              uint64_t n, uint64_t global_index_base, uint64_t chunk_size, uint64_t* d_records_out,
                              uint64_t* d_rep_out, uint64_t* d_owner_out, uint64_t capacity, uint64_t* m_out,
                              uint64_t* n_groups_out, void* stream, const sd_object_index* index,
                              uint8_t* d_existing_out, uint64_t* d_new_out, uint64_t* n_new_out);
/* Phase timing of sd_cas_dedup_mgpu (diagnostics): with timing on, each call records HIP
 * events on its stream at the phase boundaries; sd_comm_last_phases waits for the last
 * call's events and returns the SD_DEDUP_PHASES durations in ms, in order:
 *   [0] partition (kernels), [1] all-gather of the rows + their copy to the host,
 *   [2] host turnaround: the stream idles from the rows' arrival until the host, having read
 *       them, has queued the exchange (the call's one mid-call sync),
 *   [3] grouped ncclSend / ncclRecv of the records, [4] group + Object owners. */
#define SD_DEDUP_PHASES 5
/* The RCCL that serves sd_comm in this process: *version = ncclGetVersion's code (e.g.
 * 22606 = 2.26.6) and path_out = the shared object its symbols were bound to (librccl.so.1
 * is one soname: a host that loaded another RCCL first -- torch's ProcessGroupNCCL -- has
 * libsdcas's communicators served by that one).  path_out may be NULL. */
int sd_comm_rccl_info(int* version, char* path_out, size_t path_cap);
int sd_comm_set_timing(sd_comm* comm, int on);
int sd_comm_last_phases(sd_comm* comm, float* ms_out /* SD_DEDUP_PHASES */);

/* ---------------------------------------------------------------- one file over many GPUs */
/* file_checksum (hash.rs:10-24) of ONE file whose bytes are spread over the ranks of a
 * communicator (a file's 1 MiB blocks shard naturally).  The file's
 * total_len bytes are cut into nb = max(1, ceil(total_len / 1 MiB)) blocks; rank r of R
 * holds blocks [r*q, min((r+1)*q, nb)) with q = ceil(nb / R) -- sd_split_range gives its
 * byte range [offset, offset + len) and the CV buffer size, R * q * 32 bytes.  Each rank
 * hashes its blocks to their 32-byte chaining values at block index b of the CV buffer
 * (a block's CV depends only on its bytes and its position, not on the total); the
 * buffers of all ranks laid end to end in rank order are the file's block CVs in order,
 * and one reduce gives the BLAKE3 of the whole file, bit-identical to file_checksum's.
 * A file of one block (total_len <= 1 MiB) is held by rank 0, whose "CV" slot 0 then
 * holds the root hash itself.  GPU-free. */
int sd_split_range(uint64_t total_len, int nranks, int rank, uint64_t* offset, uint64_t* len,
                   uint64_t* cv_bytes);
typedef struct sd_split_checksum sd_split_checksum;
int sd_split_checksum_create(sd_cas_ctx* ctx, uint64_t total_len, int nranks, int rank,
                             sd_split_checksum** out);
void sd_split_checksum_destroy(sd_split_checksum* split);
/* This rank's blocks -> d_cvs (device, cv_bytes; only this rank's slots are written).
 * d_slice = the rank's `len` bytes (device, 16-byte aligned, zero-padded to the next
 * 64-byte boundary).  Asynchronous on `stream`. */
int sd_split_checksum_leaves(sd_cas_ctx* ctx, const sd_split_checksum* split, const uint8_t* d_slice,
                             uint8_t* d_cvs, void* stream);
/* All ranks' CVs (device, every slot filled) -> the 32-byte file hash (device).
 * Asynchronous on `stream`; one call at a time per split object. */
int sd_split_checksum_root(sd_cas_ctx* ctx, sd_split_checksum* split, const uint8_t* d_cvs,
                           uint8_t* d_hash32, void* stream);
/* Collective over the communicator (nranks / rank must match the split's): leaves, an
 * in-place ncclAllGather of the CV slots (32 B per MiB of file: 1 MB per 32 GiB), root.
 * Every rank gets the hash.  Asynchronous on `stream`. */
int sd_split_checksum_mgpu(sd_cas_ctx* ctx, sd_comm* comm, sd_split_checksum* split, const uint8_t* d_slice,
                           uint8_t* d_cvs, uint8_t* d_hash32, void* stream);
/* The same two steps on host cores (host pointers). */
int sd_cpu_split_leaves(const uint8_t* slice, uint64_t total_len, int nranks, int rank, uint8_t* cvs,
                        int nthreads);
int sd_cpu_split_root(const uint8_t* cvs, uint64_t total_len, uint8_t* out_hash32);

/* ---------------------------------------------------------------- checksum trees */
/* WHERE a file stopped matching its checksum (validator_job.rs:138-141 "we can also compare old
 * and new checksums here"; spaceblock's 128 KiB blocks, p2p/src/spaceblock/block_size.rs:20-23):
 * the file's BLAKE3 tree cut at block granularity, stored beside the checksum.
 *   block size  B = 2^block_log2 bytes, SD_TREE_BLOCK_LOG2_MIN <= block_log2 <= _MAX (128 KiB ..
 *               1 MiB); any other value is SD_ERR_INVALID
 *   blocks      nb = max(1, ceil(len / B)); block j = bytes [jB, min((j+1)B, len))
 *   node N_j    32 bytes (8 little-endian words): the BLAKE3 chaining value of the subtree over
 *               block j's chunks, chunk counters from j*B/1024, ROOT not set; inside the block
 *               pairs merge level by level with the odd node carried up (BLAKE3's own tree); the
 *               trailing partial block the same over the chunks it has
 *   nb == 1     N_0 is the file's root hash itself (ROOT set), as slot 0 of sd_split_*; an empty
 *               file has one node, the hash of the empty message
 *   level       N_0 .. N_{nb-1}; its root is N_0 if nb == 1, else the level-wise pairwise merge
 *               of the nodes, the odd node carried up, ROOT on the last parent -- file_checksum's
 *               32 bytes, bit for bit
 *   position    a full block's node, unless nb == 1, does not depend on the file's length
 *   batch       file i's level starts at node node_base[i]; node_base is the exclusive prefix sum
 *               of nb, node_base[n] the total
 * The ranges are those of sd_checksum_batch_create (host arrays, 16-byte aligned starts, the
 * buffer readable to the next 64-byte boundary).  d_nodes / d_expected are 16-byte aligned.
 * Only the device-resident batch has levels; the streamed and from-files routes do not. */
#define SD_TREE_BLOCK_LOG2_MIN 17
#define SD_TREE_BLOCK_LOG2_MAX 20
typedef struct sd_checksum_tree sd_checksum_tree;
/* nb of a file of len bytes.  GPU-free. */
int sd_checksum_tree_nodes(uint64_t len, uint32_t block_log2, uint64_t* n_nodes);
int sd_checksum_tree_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                            uint32_t block_log2, sd_checksum_tree** out);
void sd_checksum_tree_destroy(sd_checksum_tree* tree);
/* node_base[0 .. n] (host) */
int sd_checksum_tree_layout(const sd_checksum_tree* tree, uint64_t* node_base);
/* [0] files, [1] total bytes, [2] BLAKE3 compressions (those of sd_checksum_batch: the nodes cost
 * none), [3] nodes */
int sd_checksum_tree_stats(const sd_checksum_tree* tree, uint64_t out[4]);
/* One pass over the data: every file's level -> d_nodes (node_base[n] * 32 B) and its root ->
 * d_hash32 (n * 32 B), the bytes sd_checksum_batch_run writes for the same ranges.  Asynchronous
 * on `stream`; one run of a tree at a time (it owns its scratch). */
int sd_checksum_tree_run(sd_cas_ctx* ctx, const sd_checksum_tree* tree, const uint8_t* d_data, uint8_t* d_nodes,
                         uint8_t* d_hash32, void* stream);
/* Roots from levels alone, no file bytes: does a level I was sent belong to the checksum I trust?
 * Asynchronous on `stream`. */
int sd_checksum_tree_roots(sd_cas_ctx* ctx, const sd_checksum_tree* tree, const uint8_t* d_nodes, uint8_t* d_hash32,
                           void* stream);
/* Hashes d_data's blocks and compares each node with d_expected (same layout, 32 bytes per node).
 *   d_bad (node_base[n] bytes, may be NULL): 1 where block's node differs, else 0
 *   d_rows_out (2 x u64 per row, may be NULL): one row (file, block) per differing block,
 *     ascending; *count (host, may be NULL) = the rows.  If d_rows_out is given and capacity <
 *     *count: SD_ERR_CAPACITY with *count = the requirement and no row written; d_bad and stats are
 *     complete then too.  With d_rows_out NULL the call only counts.
 *   stats[4] (host, may be NULL): [0] files, [1] blocks compared, [2] blocks that differ, [3] files
 *     with at least one differing block
 * Runs on `stream` and syncs it; the level it computes lives in the context's pooled slot
 * (grow-only, 33 bytes per node and 33 per file: no allocation in a call that fits). */
int sd_checksum_tree_verify(sd_cas_ctx* ctx, const sd_checksum_tree* tree, const uint8_t* d_data,
                            const uint8_t* d_expected, uint8_t* d_bad, uint64_t* d_rows_out, uint64_t capacity,
                            uint64_t* count, uint64_t stats[4], void* stream);
/* The same over host memory on host cores, without a context or a device, with the device calls'
 * rules (a start that is not 16-byte aligned is SD_ERR_INVALID here too: one batch description
 * serves both).  nodes is laid out as node_base says (sd_checksum_tree_nodes per file). */
int sd_cpu_checksum_tree(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                         uint32_t block_log2, uint8_t* nodes, uint8_t* hash32, int nthreads);
int sd_cpu_checksum_tree_roots(const uint8_t* nodes, const uint64_t* lens, size_t n, uint32_t block_log2,
                               uint8_t* hash32);
int sd_cpu_checksum_tree_verify(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                                uint32_t block_log2, const uint8_t* expected, uint8_t* bad, uint64_t* rows_out,
                                uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads);

/* Listed blocks: the nodes of SOME blocks of SOME files, from bytes that sit anywhere in a buffer
 * -- a spaceblock Block {offset, size, data} as it arrives (p2p/src/spaceblock/block.rs:5-11), the
 * blocks a sender resent after a scrub, the blocks a write in place touched.  Only the listed bytes
 * are hashed.
 *   lens          the files' current lengths (host, n_files); nb and node_base as above
 *   rows          m x (file f, block j), 2 x u64 each (host): f < n_files, j < nb(f); any order,
 *                 not every file, repeats allowed (but see _update)
 *   data_offsets  m (host): row r's bytes -- block j of file f, lens[f] == 0 ? 0 : min(B, lens[f] -
 *                 jB) of them -- start at d_data + data_offsets[r]; sd_checksum_batch_create's rule
 *                 (16-byte aligned starts, the buffer readable to the next 64-byte boundary; what
 *                 lies after a block's last byte is not assumed zero)
 *   node          row r's node is N_j of file f exactly: the root hash when nb(f) == 1 (the empty
 *                 file too), else the plain chaining value with chunk counters from j*B/1024 (64
 *                 bits) -- a 1-byte trailing block or a one-chunk block at a counter > 0 has no ROOT
 * Anything else is SD_ERR_INVALID at create, before any allocation.  m == 0 is valid, and every call
 * on such a list does nothing and returns SD_OK.  d_nodes_out / d_expected / d_nodes are 16-byte
 * aligned. */
typedef struct sd_checksum_tree_blocks sd_checksum_tree_blocks;
int sd_checksum_tree_blocks_create(sd_cas_ctx* ctx, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                   const uint64_t* rows, const uint64_t* data_offsets, size_t m,
                                   sd_checksum_tree_blocks** out);
void sd_checksum_tree_blocks_destroy(sd_checksum_tree_blocks* blocks);
/* [0] files, [1] rows, [2] bytes hashed, [3] BLAKE3 compressions */
int sd_checksum_tree_blocks_stats(const sd_checksum_tree_blocks* blocks, uint64_t out[4]);
/* Row r's node -> d_nodes_out[32 r] (m x 32 B, list order).  Asynchronous on `stream`. */
int sd_checksum_tree_blocks_run(sd_cas_ctx* ctx, const sd_checksum_tree_blocks* blocks, const uint8_t* d_data,
                                uint8_t* d_nodes_out, void* stream);
/* Row r's node against d_expected[32 (node_base[f] + j)] (d_expected: the batch's whole level
 * layout, node_base[n_files] x 32 B; only the listed nodes are read).
 *   d_bad (m bytes, may be NULL): 1 where row r's node differs, else 0
 *   d_rows_out (2 x u64 per row, may be NULL): (file, block) of the differing rows in LIST order, a
 *     repeated row once per repeat; *count, capacity and SD_ERR_CAPACITY as sd_checksum_tree_verify
 *   stats[4] (host, may be NULL): [0] files, [1] rows compared, [2] rows that differ, [3] files with
 *     at least one differing row
 * Runs on `stream` and syncs it; the nodes it computes live in the context's pooled slot (grow-only,
 * 33 bytes per row and 1 per file). */
int sd_checksum_tree_blocks_verify(sd_cas_ctx* ctx, const sd_checksum_tree_blocks* blocks, const uint8_t* d_data,
                                   const uint8_t* d_expected, uint8_t* d_bad, uint64_t* d_rows_out,
                                   uint64_t capacity, uint64_t* count, uint64_t stats[4], void* stream);
/* Row r's node -> d_nodes[32 (node_base[f] + j)] (d_nodes: the whole level layout, patched in place;
 * every node not listed stays bit for bit), then on the same stream every file's root from the
 * patched level -> d_hash32 (n_files x 32 B), the bytes sd_checksum_tree_roots would write.  A list
 * with a repeated (file, block) is SD_ERR_INVALID here (two writers of one node), nothing written.
 * Asynchronous on `stream`; one update of a list at a time (the first plans the roots' reduce and
 * the list owns its scratch). */
int sd_checksum_tree_blocks_update(sd_cas_ctx* ctx, sd_checksum_tree_blocks* blocks, const uint8_t* d_data,
                                   uint8_t* d_nodes, uint8_t* d_hash32, void* stream);
/* The same over host memory on host cores (host pointers; the list's arrays passed again in place
 * of a handle), with the device calls' rules. */
int sd_cpu_checksum_tree_blocks(const uint8_t* data, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                const uint64_t* rows, const uint64_t* data_offsets, size_t m, uint8_t* nodes_out,
                                int nthreads);
int sd_cpu_checksum_tree_blocks_verify(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                       uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                       size_t m, const uint8_t* expected, uint8_t* bad, uint64_t* rows_out,
                                       uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads);
int sd_cpu_checksum_tree_blocks_update(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                       uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                       size_t m, uint8_t* nodes, uint8_t* hash32, int nthreads);

/* Block proofs: a listed block checked against the file's checksum and length ALONE -- what the
 * library's database keeps per file_path (integrity_checksum, size_in_bytes) -- instead of against
 * a stored level.  The project's own level-wise definitions; not Bao's byte format.
 *   levels    of a file of nb nodes: level 0 is N_0 .. N_{nb-1}, n_0 = nb; level L+1 has n_{L+1} =
 *             ceil(n_L / 2) nodes, node i = parent(level L's node 2i, node 2i+1) if 2i+1 < n_L, else
 *             a copy of the carried node 2i; ROOT goes on the one parent formed when n_L == 2; the
 *             height is h = ceil(log2 nb), 0 for nb == 1
 *   proof     of block j: for L = 0 .. h-1, i = j >> L, s = i ^ 1: if s < n_L one 32-byte entry, level
 *             L's node s, else nothing (the node was carried).  Entries bottom-up, packed.  Their
 *             count p(len, k, j) depends only on the length, block_log2 and j: nothing about a
 *             proof's shape is taken from the sender
 *   climb     from the block's node cv, at each level that has an entry: cv = parent(entry, cv) if i
 *             is odd, else parent(cv, entry), ROOT iff n_L == 2.  The result must equal the file's
 *             checksum; for nb == 1 the proof is empty and the node is the checksum
 *   trusted   the checksum AND the length: a proof is checked for a block of a file of that length
 *   layout    proof_base[0 .. m] is the exclusive prefix sum of the rows' entry counts: row r's
 *             proof is proof_base[r+1] - proof_base[r] entries at byte 32 proof_base[r]
 * d_proofs / d_proofs_out / d_roots / d_nodes_out are 16-byte aligned. */
/* p(len, block_log2, block).  GPU-free.  A block the file does not have, or a block_log2 outside
 * 17..20, is SD_ERR_INVALID. */
int sd_checksum_tree_proof_entries(uint64_t len, uint32_t block_log2, uint64_t block, uint32_t* entries);
/* proof_base[0 .. m] (host) of the list's rows.  GPU-free. */
int sd_checksum_tree_blocks_proof_layout(sd_checksum_tree_blocks* blocks, uint64_t* proof_base);
/* Every row's proof, in list order (repeats allowed), from d_nodes (the whole level layout,
 * node_base[n_files] x 32 B, as _update takes it) -> d_proofs_out (proof_base[m] x 32 B).  Reads no
 * file bytes, data_offsets play no part, and only the levels of files with at least one row are
 * read: the others may hold anything.  Asynchronous on `stream`; one prove of a list at a time (the
 * first plans the passes, and the list owns the scratch of the listed files' interior levels:
 * fewer than nb + h nodes per listed file). */
int sd_checksum_tree_blocks_prove(sd_cas_ctx* ctx, sd_checksum_tree_blocks* blocks, const uint8_t* d_nodes,
                                  uint8_t* d_proofs_out, void* stream);
/* Hashes the listed bytes, climbs each row's node through its proof (d_proofs, laid out by
 * proof_base) and compares the result with d_roots[32 f] (n_files x 32 B, the layout
 * sd_checksum_tree_roots writes; only the listed files' entries are read).
 *   d_nodes_out (m x 32 B, may be NULL): the rows' nodes, list order -- a receiver assembles its own
 *     level from the blocks that passed
 *   d_bad, d_rows_out, capacity, *count, SD_ERR_CAPACITY, stats[4]: exactly as
 *     sd_checksum_tree_blocks_verify (rows in LIST order, a repeated row once per repeat)
 * Runs on `stream` and syncs it; uses the context's pooled slot as _verify does. */
int sd_checksum_tree_blocks_verify_proofs(sd_cas_ctx* ctx, sd_checksum_tree_blocks* blocks, const uint8_t* d_data,
                                          const uint8_t* d_proofs, const uint8_t* d_roots, uint8_t* d_nodes_out,
                                          uint8_t* d_bad, uint64_t* d_rows_out, uint64_t capacity, uint64_t* count,
                                          uint64_t stats[4], void* stream);
/* The same over host memory on host cores, with the device calls' rules.  _prove takes no
 * data_offsets: it reads no file bytes. */
int sd_cpu_checksum_tree_blocks_prove(const uint8_t* nodes, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                      const uint64_t* rows, size_t m, uint8_t* proofs_out);
int sd_cpu_checksum_tree_blocks_verify_proofs(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                              uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                              size_t m, const uint8_t* proofs, const uint8_t* roots,
                                              uint8_t* nodes_out, uint8_t* bad, uint64_t* rows_out, uint64_t capacity,
                                              uint64_t* count, uint64_t stats[4], int nthreads);

/* Range proofs: a RUN of blocks [a, b) of one file checked against the checksum and the length alone
 * -- a resumed or partial transfer, spaceblock's Range::Partial(start..end)
 * (p2p/src/spaceblock/sb_request.rs:10-15).  Every interior sibling of a contiguous run is computable
 * from the run itself, so only its two flanks travel: at most 2h entries for the whole run, where
 * per-block proofs carry up to h entries per block.  Levels, parent, ROOT (on the one parent formed
 * when n_L == 2), h and the carried odd node are exactly those of the block proofs above.
 *   range     blocks [a, b) of a file of nb nodes, 0 <= a < b <= nb.  At level L = 0 .. h-1 its nodes
 *             are lo = a >> L .. hi = (b-1) >> L
 *   proof     for L = 0 .. h-1, bottom-up and packed: if lo is odd one entry, level L's node lo-1 (the
 *             left flank); then, if hi is even and hi+1 < n_L, one entry, level L's node hi+1 (the
 *             right flank).  If hi is even and hi+1 == n_L the node is carried and contributes
 *             nothing.  The entry count p(len, k, a, b-a) <= 2h follows from the length, block_log2,
 *             a and b alone: nothing about the shape is the sender's to choose
 *   climb     start from the range's nodes N_a .. N_{b-1}.  At each level prepend the left entry and
 *             append the right entry where the rule above says they exist, pair from the (now even)
 *             lo -- a last unpaired node is the file's own carry -- with ROOT iff n_L == 2.  After h
 *             levels one node remains, and it must equal the checksum
 *   special   nb == 1 or [0, nb): the proof is empty, and the climb is sd_checksum_tree_roots'
 *             computation.  b == a+1: the proof is byte for byte the block proof of block a
 *   trusted   the checksum AND the length
 *   ranges    are declared over an existing block list: range_base[0 .. q] (host) ascends strictly
 *             from range_base[0] == 0 to range_base[q] == m, and range i is rows [range_base[i],
 *             range_base[i+1]) of the list, which must be (f, a), (f, a+1), ... consecutive blocks of
 *             one file.  Bytes still sit anywhere per row (data_offsets).  Two ranges may overlap or
 *             repeat.  q == 0 is valid only for m == 0
 *   layout    proof_base[0 .. q] is the exclusive prefix sum of the ranges' entry counts
 * A failing range says "a byte of these blocks or an entry of this proof is wrong", NOT which block:
 * per-block proofs or a level remain the tools for naming the block.  Every range call on a list
 * with m > 0 before sd_checksum_tree_blocks_set_ranges is SD_ERR_INVALID.  d_proofs / d_proofs_out /
 * d_roots / d_nodes_out are 16-byte aligned. */
/* p(len, block_log2, first, count).  GPU-free.  A range the file does not have, count == 0, or a
 * block_log2 outside 17..20 is SD_ERR_INVALID. */
int sd_checksum_tree_range_proof_entries(uint64_t len, uint32_t block_log2, uint64_t first, uint64_t count,
                                         uint32_t* entries);
/* Declares the list's ranges.  GPU-free.  Anything but the rules above is SD_ERR_INVALID and the
 * list is unchanged; calling again replaces the ranges (not while a range call of the list runs). */
int sd_checksum_tree_blocks_set_ranges(sd_checksum_tree_blocks* blocks, const uint64_t* range_base, size_t q);
/* proof_base[0 .. q] (host) of the list's ranges.  GPU-free. */
int sd_checksum_tree_blocks_range_proof_layout(sd_checksum_tree_blocks* blocks, uint64_t* proof_base);
/* Every range's proof, in range order, from d_nodes (the whole level layout, as _prove takes it) ->
 * d_proofs_out (proof_base[q] x 32 B).  Reads no file bytes, and only the levels of files with a
 * range.  Asynchronous on `stream`; one prove_ranges of a list at a time (the list owns the scratch
 * of those files' interior levels). */
int sd_checksum_tree_blocks_prove_ranges(sd_cas_ctx* ctx, sd_checksum_tree_blocks* blocks, const uint8_t* d_nodes,
                                         uint8_t* d_proofs_out, void* stream);
/* Hashes the listed bytes, climbs each range through its proof (d_proofs, laid out by proof_base)
 * as a tree reduce -- about m + 2h compressions per range, not m h -- and compares the result with
 * d_roots[32 f] (n_files x 32 B; only the entries of files with a range are read).
 *   d_nodes_out (m x 32 B, may be NULL): the rows' nodes in list order, as _verify_proofs gives them
 *   d_bad (q bytes, may be NULL): 1 where range i fails, else 0
 *   d_ranges_out (3 x u64 per range, may be NULL): (file, first block, blocks) of the failing ranges
 *     in RANGE order; *count, capacity and SD_ERR_CAPACITY as sd_checksum_tree_blocks_verify
 *   stats[4] (host, may be NULL): [0] files, [1] ranges compared, [2] ranges that differ, [3] files
 *     with at least one
 * Runs on `stream` and syncs it; uses the context's pooled slot, and the list owns the scratch of the
 * groups' tops between the passes: one verify_range_proofs of a list at a time. */
int sd_checksum_tree_blocks_verify_range_proofs(sd_cas_ctx* ctx, sd_checksum_tree_blocks* blocks,
                                                const uint8_t* d_data, const uint8_t* d_proofs,
                                                const uint8_t* d_roots, uint8_t* d_nodes_out, uint8_t* d_bad,
                                                uint64_t* d_ranges_out, uint64_t capacity, uint64_t* count,
                                                uint64_t stats[4], void* stream);
/* The same over host memory on host cores: the list's arrays plus range_base are passed again, with
 * the device calls' rules (the ranges are planned, and climbed group by group, as on the device). */
int sd_cpu_checksum_tree_blocks_prove_ranges(const uint8_t* nodes, const uint64_t* lens, size_t n_files,
                                             uint32_t block_log2, const uint64_t* rows, size_t m,
                                             const uint64_t* range_base, size_t q, uint8_t* proofs_out);
int sd_cpu_checksum_tree_blocks_verify_range_proofs(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                                    uint32_t block_log2, const uint64_t* rows,
                                                    const uint64_t* data_offsets, size_t m, const uint64_t* range_base,
                                                    size_t q, const uint8_t* proofs, const uint8_t* roots,
                                                    uint8_t* nodes_out, uint8_t* bad, uint64_t* ranges_out,
                                                    uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads);

/* Shared blocks: WHICH blocks of a batch of levels are there more than once -- what sd_dedup_confirm
 * leaves open about a file it marks SD_CONFIRM_REFUTED (one block rewritten, or all of them?), and
 * about content that partly repeats: an interrupted copy, a log and its shorter version, an image
 * written in place.  By the position rule above a full block's node depends on its bytes and its
 * index only, so two files hold the same bytes in block j exactly when their level nodes at j are
 * equal.  No file byte is read and nothing is hashed: the nodes are opaque 32-byte values.
 *   input     the level layout of sd_checksum_tree_run, _roots and _blocks_update: lens[n] (host),
 *             nb_f = sd_checksum_tree_nodes(lens[f], block_log2), node_base = the exclusive prefix
 *             sum of nb, m = node_base[n]; d_nodes holds m x 32 B, 16-byte aligned; slot s =
 *             node_base[f] + j is block j of file f
 *   class(s)  the slots t = (g, j') with j' == j and all 32 bytes equal.  Equal nodes at different
 *             block indices are different classes (a node carries its chunk counter, so equal bytes
 *             at different positions do not give equal nodes anyway).  A one-node file's N_0 is a
 *             root hash and a trailing partial block's node covers fewer chunks: the byte comparison
 *             keeps those apart, they need no rule of their own.  Content that is SHIFTED, by an
 *             insertion or at another offset, is therefore not found: that takes content-defined
 *             chunking, which this is not.  Aligned blocks only (shifted content: sd_cdc_cut,
 *             sd_cdc_hash and sd_cdc_shared below, "content-defined chunks")
 *   d_rep[s]         the smallest slot of class(s); it lies in the lowest-numbered file that holds
 *                    the block (a file has one slot per j)
 *   d_class_size[s]  |class(s)|
 *   shared    d_class_size[s] >= 2;  redundant  d_rep[s] != s: an earlier file has the block
 *   bytes(s)  min(B, lens[f] - j B); an empty file's one slot has 0 bytes
 *   d_files_out  4 x u64 per file: [0] nb_f, [1] shared blocks, [2] redundant blocks, [3] redundant bytes
 *   d_pairs_out  4 x u64 per row (f, g, blocks, bytes): one row per pair g < f such that at least
 *             max(1, min_blocks) redundant slots of f have their representative in g, blocks and
 *             bytes summed over those slots; rows ascend by (f, g).  This is the star towards the
 *             FIRST holder of each block, not all pairs: at most m - 1 rows, however many files
 *             share the all-zero block.  *n_pairs (host, may be NULL) = the rows.  If d_pairs_out is
 *             given and capacity < *n_pairs: SD_ERR_CAPACITY with *n_pairs = the requirement and no
 *             row written; every other output is complete then too.  With d_pairs_out NULL the call
 *             only counts.  Nothing past the first *n_pairs rows is ever written
 *   stats[8]  (host, may be NULL) [0] files, [1] blocks (m), [2] classes, [3] classes of size >= 2,
 *             [4] redundant blocks, [5] redundant bytes, [6] files with a redundant block, [7] files
 *             EVERY block of which is redundant.  They do not depend on min_blocks or capacity.
 *             [4] == [1] - [2] == the sum of files[.][2]; [5] == the sum of files[.][3]; with
 *             min_blocks <= 1 the rows' blocks add up to [4] and their bytes to [5]; file 0 is
 *             never in [6]
 * Any output pointer may be NULL.  n == 0 is valid: counts are 0, nothing is written.  A block_log2
 * outside 17..20, a NULL lens or d_nodes with m > 0, or n >= 2^32 is SD_ERR_INVALID.  Runs on
 * `stream` and syncs it; scratch comes from the context's pooled slot (grow-only: 77 bytes per slot,
 * 32 per file and 16 per file of tables, plus the radix sort's; no allocation in a call that fits
 * what the slot holds).  The grouping is sd_dedup_confirm's with key = j and hash = node, both of
 * its paths included ("confirm_full_sort" applies; sd_dedup_confirm_stats does not count these
 * calls).  One device, not collective: sharding a library's levels over ranks is not provided. */
int sd_checksum_tree_shared(sd_cas_ctx* ctx, const uint64_t* lens, size_t n, uint32_t block_log2,
                            const uint8_t* d_nodes, uint64_t min_blocks, uint64_t* d_rep, uint64_t* d_class_size,
                            uint64_t* d_files_out, uint64_t* d_pairs_out, uint64_t capacity, uint64_t* n_pairs,
                            uint64_t stats[8], void* stream);
/* The same over host arrays, without a context or a device. */
int sd_cpu_checksum_tree_shared(const uint64_t* lens, size_t n, uint32_t block_log2, const uint8_t* nodes,
                                uint64_t min_blocks, uint64_t* rep, uint64_t* class_size, uint64_t* files_out,
                                uint64_t* pairs_out, uint64_t capacity, uint64_t* n_pairs, uint64_t stats[8]);

/* ---------------------------------------------------------------- content-defined chunks */
/* Content-defined chunks: content that is there more than once at ANY offset -- what the shared
 * blocks above cannot see (a header rewritten, a log and its rotated copy, an edited document, a
 * container with one member changed).  A file is cut where its content says so, every chunk gets
 * the plain BLAKE3 of its bytes as its id, and sd_cdc_shared groups the chunks of a batch of files
 * by (length, id).  One byte inserted at the front moves the cuts with the content: all chunks but
 * the first few are found again.
 *   gear      G[b] = splitmix64(0x5DCDC0DE ^ b), b = 0..255 (add 0x9E3779B97F4A7C15, two
 *             multiply-xorshift rounds, xorshift 31); G[0] = 0x2df3228afbc5cb53, G[255] =
 *             0xdd9fba0f5362ab8e
 *   rolling   per file h(-1) = 0, h(i) = (h(i-1) << 1) + G[byte i] mod 2^64: the last 64 bytes of
 *             the file only, never a byte before the file's start
 *   candidate position i is a candidate end e = i + 1 when h(i) & MASK == 0, MASK = the top
 *             mask_bits bits
 *   select    per file from s = 0: e = the smallest candidate end with s + min_size <= e <= s +
 *             max_size, else s + max_size; e = min(e, len); repeat from s = e until e == len.  An
 *             empty file has the one chunk (0, 0)
 *   id        BLAKE3 of the chunk's bytes (32 bytes, ROOT, chunk counters from 0): file_checksum
 *             of the chunk as a file, wherever it lies
 *   params    valid iff 1 <= mask_bits <= 32, 64 <= min_size <= max_size <= 2^20, reserved == 0;
 *             anything else is SD_ERR_INVALID before any allocation.  min_size >= 64 makes the
 *             rolling value equal the one that restarts at each chunk; max_size <= 1 MiB keeps a
 *             chunk inside one BLAKE3 subtree of 1024 chunk CVs.  The mean chunk is about
 *             min_size + 2^mask_bits bytes */
typedef struct sd_cdc_params {
    uint32_t mask_bits, min_size, max_size, reserved;
} sd_cdc_params;
#define SD_CDC_DEFAULT_MASK_BITS 16
#define SD_CDC_DEFAULT_MIN_SIZE 16384
#define SD_CDC_DEFAULT_MAX_SIZE 262144
typedef struct sd_cdc sd_cdc;
/* The gear table.  Needs no GPU. */
int sd_cdc_gear(uint64_t out[256]);
/* A batch of files that are byte ranges of one device buffer: sd_checksum_batch_create's rule
 * (host arrays, 16-byte aligned starts, the buffer readable to the next 64-byte boundary after
 * each range; the buffer itself 16-byte aligned).  The sum of ceil(lens[f] / min_size) plus n must
 * stay below 2^32, else SD_ERR_INVALID.  The batch owns its tables, its candidate bitmap (one bit
 * per byte) and its chunk table; one cut or hash of it runs at a time. */
int sd_cdc_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                  const sd_cdc_params* params, sd_cdc** out);
void sd_cdc_destroy(sd_cdc* cdc);
/* Scans the files for candidates and selects the cuts.  Runs on `stream` and syncs it: *n_chunks
 * (host) sizes the caller's buffers.  One wave walks each file's bitmap, so a single huge file is a
 * serial walk (DESIGN.md §3.6 has the measured time). */
int sd_cdc_cut(sd_cas_ctx* ctx, sd_cdc* cdc, const uint8_t* d_data, void* stream, uint64_t* n_chunks);
/* chunk_base[0 .. n] (host): the exclusive prefix sum of the chunks per file.  After a cut. */
int sd_cdc_layout(const sd_cdc* cdc, uint64_t* chunk_base);
/* After a cut: [0] files, [1] bytes, [2] candidates (set bits), [3] chunks, [4] chunks ended at a
 * candidate, [5] chunks ended at s + max_size with no candidate (forced), [6] chunks that end at
 * the file's end, counted here whatever else holds (an empty file's one chunk included), [7] BLAKE3
 * compressions of the hash.  [3] == [4] + [5] + [6]. */
int sd_cdc_stats(const sd_cdc* cdc, uint64_t out[8]);
/* The chunks in layout order: d_chunks_out takes 2 x u64 per chunk (offset in its file, length),
 * d_ids_out 32 bytes per chunk (16-byte aligned).  Either may be NULL.  The data is read once, in
 * place: a chunk starts at any byte and is realigned in registers.  Asynchronous on `stream` and
 * without an allocation: the piece CVs of chunks longer than 4 KiB pass through scratch the cut
 * sized (grow-only, 32 bytes per 4 KiB piece), which is why one cut or hash of a batch runs at a
 * time.  Before any cut: SD_ERR_INVALID (so are _layout and _stats). */
int sd_cdc_hash(sd_cas_ctx* ctx, sd_cdc* cdc, const uint8_t* d_data, uint64_t* d_chunks_out,
                uint8_t* d_ids_out, void* stream);
/* Which chunks of a batch are there more than once: sd_checksum_tree_shared's contract with the
 * chunk table in the place of the level -- chunk_base[0 .. n] (host, sd_cdc_layout), d_chunks and
 * d_ids as sd_cdc_hash leaves them, slot s = chunk_base[f] + k.  Representatives, d_rep,
 * d_class_size, d_files_out (4 x u64 per file: chunks, shared, redundant, redundant bytes),
 * d_pairs_out rows (f, g, chunks, bytes) for g < f ascending by (f, g) with at least
 * max(1, min_chunks) slots, the star towards the first holder, capacity / *n_pairs /
 * SD_ERR_CAPACITY, count-only calls, any NULL output and n == 0 are as there.  What differs:
 *   class(s)  the slots of equal length and equal 32 id bytes, at ANY position in any file
 *   bytes(s)  the chunk's length
 *   a file may repeat a chunk inside itself: such a slot is redundant, counts in d_files_out and in
 *             stats[4] and [5], and gets no pair row (rows are for g < f only)
 *   stats[8]  [0] files, [1] chunks, [2] classes, [3] classes of size >= 2, [4] redundant chunks,
 *             [5] redundant bytes, [6] files with a redundant chunk, [7] redundant chunks whose
 *             representative lies in the same file.  With min_chunks <= 1 the rows' chunks add up
 *             to [4] - [7]
 * The grouping is sd_dedup_confirm's with key = length and hash = id, both of its paths.  Runs on
 * `stream` and syncs it; scratch comes from the context's pooled slot. */
int sd_cdc_shared(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, const uint64_t* d_chunks,
                  const uint8_t* d_ids, uint64_t min_chunks, uint64_t* d_rep, uint64_t* d_class_size,
                  uint64_t* d_files_out, uint64_t* d_pairs_out, uint64_t capacity, uint64_t* n_pairs,
                  uint64_t stats[8], void* stream);
/* The same over host memory on host cores, without a context or a device.  _cut: chunk_base
 * [0 .. n] and the stats are always complete; chunks_out (2 x u64 per chunk, may be NULL) takes at
 * most `capacity` chunks, and a smaller capacity is SD_ERR_CAPACITY with *n_chunks = the
 * requirement and no chunk written.  _hash takes _cut's arrays back. */
int sd_cpu_cdc_cut(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                   const sd_cdc_params* params, uint64_t* chunk_base, uint64_t* chunks_out, uint64_t capacity,
                   uint64_t* n_chunks, uint64_t stats[8], int nthreads);
int sd_cpu_cdc_hash(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                    const uint64_t* chunk_base, const uint64_t* chunks, uint8_t* ids_out, int nthreads);
int sd_cpu_cdc_shared(const uint64_t* chunk_base, size_t n, const uint64_t* chunks, const uint8_t* ids,
                      uint64_t min_chunks, uint64_t* rep, uint64_t* class_size, uint64_t* files_out,
                      uint64_t* pairs_out, uint64_t capacity, uint64_t* n_pairs, uint64_t stats[8]);

/* Deltas: acting on shared chunks.  Files 0 .. n_base-1 of a chunk table are the BASE (what a
 * receiver holds), files n_base .. n-1 the TARGETS, 0 <= n_base <= n.  The plan turns the table and
 * sd_cdc_shared's d_rep over it into a recipe: runs that copy from a base file or from a literal
 * buffer, and the few literal bytes.  It reads tables only, never data and never ids, so a sender
 * that has the receiver's chunk table (lengths and ids) in front of its own can plan.
 *   kind(s)   of target slot s with r = d_rep[s]:
 *             zero     its length is 0 (an empty file's one chunk): a literal chunk of 0 bytes
 *                      whatever its class; emits no run
 *             copy     r lies in a base file g: source 1 + g, source offset chunks[r].offset
 *             literal  r == s: its bytes are appended to the literal buffer; lit_off[s] = the sum of
 *                      the lengths of the literal slots before s in slot order
 *             repeat   r is an earlier target slot (a literal, by the representatives' rule): source
 *                      0, source offset lit_off[r] -- sent once, referred to again
 *   runs      per target file, consecutive non-zero chunks k, k + 1 merge iff they have the same
 *             source and src_off(k) + len(k) == src_off(k + 1); never across a file boundary.  A row
 *             is 4 x u64 (t, source, src_off, bytes), t = the target's file index - n_base; rows
 *             ascend by t, then by position in the file.  A run's destination offset in its file is
 *             the sum of the bytes of that file's earlier runs.  A target identical to base file g
 *             is the one row (t, 1 + g, 0, len)
 *   d_lit_off one u64 per target slot (slot s at s - chunk_base[n_base]): the offset in the literal
 *             buffer for a literal or a repeat, ~0 for a copy or a zero
 *   d_files_out  6 x u64 per target: chunks, copied chunks, copied bytes, new literal bytes,
 *             repeated bytes, runs
 *   stats[8]  [0] target files, [1] target chunks, [2] copied chunks, [3] copied bytes, [4] literal
 *             chunks (zeros included), [5] literal bytes = the literal buffer's size, [6] repeated
 *             chunks, [7] runs.  [1] == [2] + [4] + [6]; the targets' bytes == [3] + [5] + the
 *             repeated bytes (the sum of the files' fifth column)
 * d_runs_out / capacity / *n_runs / SD_ERR_CAPACITY are sd_cdc_shared's pair rows' rule: NULL only
 * counts, a short capacity writes no row and leaves the requirement in *n_runs with everything else
 * complete, nothing is written past *n_runs.  Any output may be NULL; n_base == n or n == 0 gives
 * zeros.  n_base > n, a NULL table with slots, or a d_rep that is not a representative table
 * (r > s, lengths that differ, a representative that has one itself) is SD_ERR_INVALID, the first
 * two before any allocation.  Runs on `stream` and syncs it; scratch comes from the context's pooled
 * slot.  The plan also sizes the context's delta scratch for sd_cdc_delta_pack over this table. */
int sd_cdc_delta_plan(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* d_chunks,
                      const uint64_t* d_rep, uint64_t* d_lit_off, uint64_t* d_runs_out, uint64_t capacity,
                      uint64_t* n_runs, uint64_t* d_files_out, uint64_t stats[8], void* stream);
/* Gathers the literal slots' bytes into d_lit_out at their lit_off (stats[5] bytes): the tables as
 * the plan took and left them, offsets[0 .. n) (host) the files' ranges in d_data as sd_cdc_create
 * took them.  Only target ranges of d_data are read, under sd_cdc_create's promise (16-byte aligned
 * buffer and starts, readable to the next 64-byte boundary after a range); d_lit_out has no
 * alignment rule.  Asynchronous on `stream` and without an allocation after a plan over the same
 * table: its segment list lives in the context's delta scratch, so one pack or apply of a context
 * runs at a time.  The tables are trusted: they are the plan's own. */
int sd_cdc_delta_pack(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* offsets,
                      const uint64_t* d_chunks, const uint64_t* d_lit_off, const uint64_t* d_rep, const uint8_t* d_data,
                      uint8_t* d_lit_out, void* stream);
/* Rebuilds the targets: run (t, source, src_off, bytes) copies `bytes` bytes from source 0 = d_lit
 * [0, lit_bytes) or source 1 + g = d_base + base_offsets[g] [0, base_lens[g]) to d_out +
 * out_offsets[t] at the run's destination offset.  The recipe is UNTRUSTED (it arrives off a wire)
 * and is validated first, on the device, with one host wait for the verdict:
 *   t < n_targets and the rows ascend by t; source <= n_base; src_off + bytes is at most the
 *   source's length, computed without 64-bit wrap; every file's runs sum to out_lens[t] (a file
 *   without a run is empty)
 * Anything else is SD_ERR_INVALID with NO byte of d_out written.  Only then are the bytes copied,
 * asynchronously on `stream`.  Output ranges have no alignment rule (and must not overlap); d_base,
 * base_offsets and d_lit follow sd_cdc_create's (d_lit as one range from 0).  base_offsets,
 * base_lens, out_offsets, out_lens are host arrays; n_runs, n_base and n_targets stay below 2^32. */
int sd_cdc_delta_apply(sd_cas_ctx* ctx, const uint64_t* d_runs, uint64_t n_runs, const uint64_t* base_offsets,
                       const uint64_t* base_lens, size_t n_base, const uint8_t* d_base, const uint8_t* d_lit,
                       uint64_t lit_bytes, const uint64_t* out_offsets, const uint64_t* out_lens, size_t n_targets,
                       uint8_t* d_out, void* stream);
/* The same over host arrays on host cores, with the same rules and refusals (no alignment rule). */
int sd_cpu_cdc_delta_plan(const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* chunks,
                          const uint64_t* rep, uint64_t* lit_off, uint64_t* runs_out, uint64_t capacity,
                          uint64_t* n_runs, uint64_t* files_out, uint64_t stats[8]);
int sd_cpu_cdc_delta_pack(const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* offsets,
                          const uint64_t* chunks, const uint64_t* lit_off, const uint64_t* rep, const uint8_t* data,
                          uint8_t* lit_out);
int sd_cpu_cdc_delta_apply(const uint64_t* runs, uint64_t n_runs, const uint64_t* base_offsets,
                           const uint64_t* base_lens, size_t n_base, const uint8_t* base, const uint8_t* lit,
                           uint64_t lit_bytes, const uint64_t* out_offsets, const uint64_t* out_lens, size_t n_targets,
                           uint8_t* out, int nthreads);

/* ---------------------------------------------------------------- synthetic data */
/* Device generator of SURVEY.md §8(d) (seed 0x5D5DCA51D, splitmix64 counter stream),
 * for benchmarks and parity tests: writes the exact cas message of each synthetic file
 * (content id cids[i], twin tag twins[i]) into its extent.  All arrays device. */
int sd_synth_stage_cas(sd_cas_ctx* ctx, const uint64_t* d_sizes, const uint64_t* d_cids,
                       const uint32_t* d_twins, const sd_extent* d_extents, size_t n,
                       uint8_t* d_staged, void* stream);
/* bytes [0, len) of synthetic content (cid, twin) -> d_out (device) */
int sd_synth_fill(sd_cas_ctx* ctx, uint64_t cid, uint32_t twin, uint64_t len, uint8_t* d_out,
                  void* stream);
/* bytes [offset, offset + len) of the same content -> d_out (offset and d_out 8-aligned) */
int sd_synth_fill_at(sd_cas_ctx* ctx, uint64_t cid, uint32_t twin, uint64_t offset, uint64_t len,
                     uint8_t* d_out, void* stream);

/* ---------------------------------------------------------------- device utilities */
int sd_device_malloc(sd_cas_ctx* ctx, uint64_t bytes, void** out);
void sd_device_free(sd_cas_ctx* ctx, void* p);
int sd_memcpy(sd_cas_ctx* ctx, void* dst, const void* src, uint64_t bytes, void* stream);
int sd_stream_sync(sd_cas_ctx* ctx, void* stream);
/* Time `iters` back-to-back runs of a prepared batch with HIP events on `stream`:
 * *ms_total = elapsed milliseconds (kernel time on that stream, no host sync inside). */
int sd_cas_batch_time(sd_cas_ctx* ctx, const sd_cas_batch* batch, const uint8_t* d_staged,
                      uint8_t* d_hash32, int iters, void* stream, float* ms_total);
int sd_checksum_batch_time(sd_cas_ctx* ctx, const sd_checksum_batch* batch, const uint8_t* d_data,
                           uint8_t* d_hash32, int iters, void* stream, float* ms_total);
/* Process-wide knobs (results are identical for every value): "coalesce_window_us"
 * (200), "coalesce_max" (4096) and "latency_cpu_max" (16) of the latency path;
 * "files_window_mb" (32) of sd_cas_ids_files; "read_threads" (16) of sd_file_checksums;
 * "dedup_variant" (sd_dedup_group) 0 =
 * rocPRIM radix sort, 1 = LDS buckets with the radix sort as overflow fallback (default);
 * "sampled_wave_max" (6144) / "whole_wave_max" (512): a cas batch with at most that many
 * sampled / whole-kind files takes the latency kernels (one wave or workgroup per file),
 * a larger one the throughput kernels -- read when the batch is planned; "batch_cpu_max"
 * (4096): sd_cas_ids_files calls of at most that many files take the CPU path;
 * "files_ring" (4): pinned window buffers sd_cas_ids_files' readers may fill ahead of the
 * copies; "files_stage_hot" (1): its readers read each file into a per-thread buffer and
 * stream-copy it into the window (0 = read straight into the window); "checksum_cpu_max" (2147483647): sd_file_checksums calls of at most that many
 * files take the CPU path (sd_cpu_file_checksums on "read_threads" threads; 0 = the GPU
 * route always); "checksum_hybrid_threads" (6): GPU slots -- threads feeding the GPU at once
 * -- when sd_file_checksums splits a large call with the CPU path (0 = never split);
 * "checksum_stage_hot" (1): sd_file_checksums' GPU-route readers deliver through a
 * cache-resident buffer and streaming stores (0 = pread straight into the pinned window);
 * "cpu_read_piece_kib" (256): the CPU path reads and hashes each 1 MiB block of a large file
 * in pieces of this many KiB, each hashed while still in the core's L2 (0 = one 1 MiB read,
 * then the hash; 256 measured 1.04-1.07x, profiles/r5/r5d_hybrid.json);
 * "checksum_split_blocks" (1): sd_file_checksums' split claims work by 1 MiB blocks (the
 * GPU's "checksum_hybrid_threads" slots take runs of blocks while free, the host threads
 * single blocks); 0 = by whole files (round 4);
 * "checksum_split_adapt" (8): a call the split applies to takes the split or the CPU path
 * alone, learned per context from the GB/s of its past calls -- each once, then the faster,
 * the other every k-th call to keep its rate current; 0 = always the split;
 * "host_cohash_threads" (15): host threads hashing beside the GPU in sd_cas_ids calls of
 * >= 8192 files and sd_checksums calls of >= 1 GiB (0 = the GPU alone; never more than the
 * host budget less one in sd_cas_ids, less 3/16 of it (at least one) in sd_checksums -- 13
 * of 16 measured best there); "host_cpu_budget" (0 = resolved, see sd_host_cpu_budget): the cap
 * on every call's host threads -- thread counts callers pass (nthreads) and the knobs above
 * are clamped to it; "comm_timeout_ms" (300000): the longest sd_cas_dedup_mgpu waits for its
 * RCCL peers (0 = no bound); "fingerprint_window_mb" (256): the device window of ranges
 * sd_fingerprints uploads at once (a longer range streams); "index_dir_max_bits" (24): the
 * most prefix-directory bits an Object-index insert chooses (0 = no directory: every lookup is
 * a binary search over the whole key array); "confirm_full_sort" (0): sd_dedup_confirm sorts by
 * (key, first 8 checksum bytes) and takes the full-width sort only on a tie with unequal tails
 * (1 = always the full-width sort).  Unknown keys fail with SD_ERR_INVALID. */
int sd_cas_set_tuning(const char* key, int value);
int sd_cas_get_tuning(const char* key, int* value);
/* Read-only probe over d_buf[0, bytes) (bytes a multiple of 4096) for calibrating the
 * PMC byte counters on this kernel family's access patterns: pattern 0 = coalesced
 * 16 B/lane streaming, pattern 1 = one lane per 1 KiB chunk reading 4 x 16 B per 64-byte
 * block (the hashing kernels' pattern), pattern 2 = pattern 1 with 2 chunks per lane,
 * pattern 3 = pattern 0 with its loads marked non-temporal. */
int sd_read_probe(sd_cas_ctx* ctx, const uint8_t* d_buf, uint64_t bytes, int pattern, void* stream);
/* VALU ceiling of the kernels' BLAKE3 G instruction mix (asm, registers only, 8 waves per SIMD):
 * measured lane-ops/s on this device. */
int sd_valu_peak(sd_cas_ctx* ctx, double* lane_ops_per_s);

#ifdef __cplusplus
}
#endif
#endif /* SD_CAS_H */
