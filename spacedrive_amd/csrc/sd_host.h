// sd_host.h -- the GPU-free half of libsdcas: batch planners, the file stager with the
// reference's read semantics, the sequential message reader, error plumbing.
//
// Nothing here includes HIP, so this code (sd_host.cpp, cpu_blake3.cpp, stage_pool.h) is
// also built with g++ under ASan/UBSan and TSan by `make sanitize` (csrc/host_selftest.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sd_cas.h"
#include "stage_pool.h"

// ------------------------------------------------------------------ errors
struct sd_failure : std::runtime_error {
    int rc;
    sd_failure(int r, const std::string& m) : std::runtime_error(m), rc(r) {}
};
void sd_set_err(const char* fmt, ...);

// The HIP-thread rule: a thread that ran private_fd_table() has closed its
// copies of the HIP runtime's device descriptors, so a HIP call from it faults the process
// (round 5's first block split did exactly that).  Every HIP_CHECK (sd_api_impl.h) asks
// this first and throws SD_ERR_INTERNAL with `what` named instead of calling HIP there.
bool on_private_fd_table();
void hip_thread_check(const char* what);

// every extern "C" entry point: no C++ exception crosses the ABI (the reference FFI fences
// panics with catch_unwind, apps/mobile/modules/sd-core/ios/crate/src/lib.rs:41,60)
#define SD_GUARD_BEGIN try {
#define SD_GUARD_END                                   \
    }                                                  \
    catch (const sd_failure& f) {                      \
        sd_set_err("%s", f.what());                    \
        return f.rc;                                   \
    }                                                  \
    catch (const std::bad_alloc&) {                    \
        sd_set_err("host allocation failed");          \
        return SD_ERR_NOMEM;                           \
    }                                                  \
    catch (const std::exception& ex) {                 \
        sd_set_err("internal error: %s", ex.what());   \
        return SD_ERR_INTERNAL;                        \
    }                                                  \
    catch (...) {                                      \
        sd_set_err("internal error");                  \
        return SD_ERR_INTERNAL;                        \
    }

// process-wide tuning knobs (sd_cas_set_tuning, defined in sd_host.cpp); read at call time
enum sd_tune_key {
    SD_TUNE_COALESCE_US = 0,      // latency path: GPU batch collection window (us)
    SD_TUNE_COALESCE_MAX = 1,     // latency path: largest coalesced GPU batch
    SD_TUNE_FILES_WINDOW_MB = 2,  // sd_cas_ids_files: pinned staging window (MiB)
    SD_TUNE_DEDUP_VARIANT = 3,    // sd_dedup_group: 0 = radix sort, 1 = LDS buckets (radix on overflow)
    SD_TUNE_LATENCY_CPU_MAX = 4,  // latency path: hash on the CPU while fewer calls are in flight
    SD_TUNE_READ_THREADS = 5,     // sd_file_checksums: parallel preads of regular files
    SD_TUNE_SAMPLED_WAVE_MAX = 6, // batches of at most this many sampled files: one wave per file (latency)
    SD_TUNE_WHOLE_WAVE_MAX = 7,   // batches of at most this many whole-kind files: one workgroup per file
    SD_TUNE_BATCH_CPU_MAX = 8,    // sd_cas_ids_files: calls of at most this many files take the CPU path
    SD_TUNE_FILES_RING = 9,       // sd_cas_ids_files: pinned window buffers the readers may fill ahead
    SD_TUNE_CHECKSUM_CPU_MAX = 10,  // sd_file_checksums: calls of at most this many files take the CPU path
    SD_TUNE_FILES_STAGE_HOT = 11,   // sd_cas_ids_files: read into a per-thread buffer, stream-copy to the window
    SD_TUNE_CHECKSUM_HYBRID_THREADS = 12,  // sd_file_checksums: reader threads of the GPU route in a hybrid call
    SD_TUNE_HOST_COHASH_THREADS = 13,      // sd_cas_ids: host threads hashing beside the GPU (large calls)
    SD_TUNE_HOST_CPU_BUDGET = 14,          // cap on the host threads one call starts (0 = resolve it)
    SD_TUNE_CHECKSUM_STAGE_HOT = 15,       // sd_file_checksums' GPU route: pread_stream into the windows
    SD_TUNE_NUMA_PIN = 16,                 // library threads on the GPU's NUMA node (0 = float)
    SD_TUNE_CPU_READ_PIECE_KIB = 17,       // CPU path: a 1 MiB block read and hashed in pieces of this size
    SD_TUNE_CHECKSUM_SPLIT_BLOCKS = 18,    // sd_file_checksums' split: 1 = claims by blocks, 0 = by files
    SD_TUNE_CHECKSUM_SPLIT_ADAPT = 19,     // split-eligible calls: 0 = always split, k = learn the faster route
    SD_TUNE_COMM_TIMEOUT_MS = 20,          // sd_cas_dedup_mgpu over RCCL: longest wait for the peers (0 = none)
    SD_TUNE_FINGERPRINT_WINDOW_MB = 21,    // sd_fingerprints: device window of ranges per upload (MiB)
    SD_TUNE_INDEX_DIR_MAX_BITS = 22,       // Object index: most directory bits an insert chooses (0 = no directory)
    SD_TUNE_CONFIRM_FULL_SORT = 23,        // sd_dedup_confirm: 0 = the prefix path first, 1 = always the full-width path
    SD_TUNE_NKEYS = 24
};
int tuning_get(int key);

// ------------------------------------------------------------------ host thread budget
// The host threads one call of this process may run at once, at least
// 1: min(the affinity share, the quota share), where
//   * the affinity share is the CPUs in the process's affinity mask -- divided by the GPU
//     ranks sharing the node (LOCAL_WORLD_SIZE, which torch.distributed.run sets; 1 when
//     absent) only when the mask holds every online CPU; a narrower mask is a per-rank
//     binding and already this rank's own;
//   * the quota share is the cgroup CPU bandwidth quota, rounded up, divided by those
//     ranks: every rank of the container draws on the one quota.  The quota is the
//     tightest limit on the path from the process's own cgroup (/proc/self/cgroup) up to
//     the mount root.
// "host_cpu_budget" > 0 replaces the resolved value (a Rust host that knows its own share
// sets it).  Every pool size, reader count and co-hash thread count is capped by it.
struct CpuBudget {
    int budget = 1;       // the cap
    int affinity = 1;     // CPUs in sched_getaffinity
    int online = 1;       // CPUs the process's container may use: online, or its cpuset when smaller
    int quota_milli = 0;  // cgroup CPU quota in milli-CPUs (0 = no limit)
    int local_world = 1;  // ranks per node sharing the host
    int overridden = 0;   // 1 when "host_cpu_budget" set the cap
};
// pure arithmetic of the rule (host_selftest checks it with fake masks, quotas and world sizes)
CpuBudget cpu_budget_resolve(int affinity, int online, double quota_cpus, int local_world);
// the CPU bandwidth limit of the cgroup directory `root` (v2 cpu.max, else v1
// cpu/cpu.cfs_quota_us / cpu.cfs_period_us), in CPUs; 0 when unlimited or unreadable
double cgroup_cpu_quota(const char* root);
// the tightest limit over the mount root and every directory from the process's own cgroup
// (read from `proc_cgroup`, default /proc/self/cgroup) up to it; `root` defaults to
// /sys/fs/cgroup.  0 when none is set
double cgroup_cpu_quota_self(const char* root, const char* proc_cgroup);
// CPUs in the process's cgroup cpuset (v2 cpuset.cpus.effective of its own cgroup, else the
// mount root's; v1 cpuset/<path>/cpuset.effective_cpus or cpuset.cpus), 0 when unreadable:
// a container pinned with --cpuset-cpus and no quota shows the host's CPUs online, and an
// affinity mask of the whole cpuset is then shared by the node's ranks, not one rank's binding
int cgroup_cpuset_count(const char* root, const char* proc_cgroup);
// CPUs in a cpuset list ("0-15,32,40-47"); 0 when malformed
int cpulist_count(const char* list);
CpuBudget host_cpu_budget_detail();  // resolved once per process, then the override applied
int host_cpu_budget();
inline int cap_host_threads(int n) {
    const int b = host_cpu_budget();
    return n < 1 ? 1 : (n > b ? b : n);
}

// ------------------------------------------------------------------ NUMA placement
// With "numa_pin" 1 (opt-in) the library's own threads (pool workers, co-hashing threads)
// run on the CPUs of the GPU's NUMA node, within each thread's own affinity mask; with 0 a
// thread is never touched, and one placed earlier gets its own mask back.  When the
// files' page cache was written on that node too, it pays (scripts/numa_probe.sh: the CPU
// path 90 vs 77 GB/s, the split checksum 106 vs 100 GB/s); with the page cache where an
// unplaced writer left it -- the usual case -- it measured neutral (0.93-1.04x,
// scripts/numa_lib_probe.py), so it is off by default.  `node_cpulist` is the node's sysfs
// cpulist ("0-63,128-191"); the first context sets the preference.  Returns the CPUs kept.
int numa_prefer_cpus(const char* node_cpulist);
// the node of a PCI device ("0000:23:00.0") from sysfs, or -1
int pci_numa_node(const char* bdf);
// the sysfs cpulist of a NUMA node ("" when absent)
std::string numa_node_cpulist(int node);
// 1 when library threads are placed on a preferred CPU set; the set's CPU count in *ncpus,
// the first context's device node in *node (-1 unknown)
int numa_placement(int* ncpus, int* node);
void numa_note_node(int node);

// latency path (coalesce.cpp): single-file calls, CPU route or coalesced GPU batches
struct sd_coalescer;
sd_coalescer* coalescer_create(sd_cas_ctx* ctx);
void coalescer_destroy(sd_coalescer* c);
int coalescer_submit(sd_coalescer* c, int kind, const char* path, uint64_t size, char* out, int32_t* status,
                     std::string* err);
void coalescer_stats(sd_coalescer* c, uint64_t out[4]);

inline uint64_t sd_align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
// sd_file_status IO_ERROR with the errno in the high 16 bits
inline int32_t io_status(int err) { return (int32_t)(SD_FILE_IO_ERROR | ((uint32_t)(err & 0xFFFF) << 16)); }

// What the kernels need of a staged message: a 16-byte aligned start (validate_extent) and
// zero padding up to the next 64-byte boundary.  The planner places messages on
// SD_STAGE_ALIGN (128, whole cache lines) but callers' own layouts only need this.
constexpr uint64_t SD_STAGE_PAD = 64;
// Whole-file cas messages up to this length (8 + 102400: every file the reference hashes
// whole when its length equals `size`) go through the work-list kernels; longer ones (a
// file that grew past the size it was planned with) through the chunk-parallel checksum
// kernels -- a message is just bytes.
constexpr uint32_t SD_WHOLE_ITEMS_MAX = 8 + SD_MINIMUM_FILE_SIZE;
// hash.rs:8 BLOCK_LEN: file_checksum reads 1 MiB per read call; also the checksum
// kernels' leaf block (1024 chunks per workgroup)
constexpr uint64_t SD_CK_BLOCK = 1ull << 20;

// ------------------------------------------------------------------ device tables
struct sd_u32x2 { uint32_t x, y; };        // layout of HIP's uint2
struct sd_u32x4 { uint32_t x, y, z, w; };  // layout of HIP's uint4

// one message of a checksum batch
struct ck_file {
    uint64_t offset;   // byte offset in the data buffer
    uint64_t len;      // message length
    uint64_t cv_base;  // first slot of this message's 1 MiB block CVs in the level-0 CV buffer
};

// one workgroup of a checksum reduce pass
struct ck_reduce_wg {
    uint64_t src_base;   // first CV (index into the source level) of this group
    uint64_t dst_index;  // CV slot in the destination level
    uint32_t count;      // CVs in this group (1..256)
    uint32_t file;       // file index (for the root output)
    uint32_t is_root;    // the group is the file's whole level: ROOT on the final parent
    uint32_t pad;
};

// ------------------------------------------------------------------ planners
// cas.rs:25-58 message layout of a file of `size` bytes at `off`: le64(size) || the whole
// file (size <= 102400, cas.rs:27 -- inclusive) or head / 4 samples / tail (57 352 B)
sd_extent plan_extent(uint64_t size, uint64_t off);
// the kind follows the size argument (cas.rs:27); a sampled message is 57 352 B; a whole
// message is le64(size) + the bytes the file held when read (any count, cas.rs:29)
void validate_extent(const sd_extent& e, size_t i);
uint32_t msg_chunks(uint32_t msg_len);
// BLAKE3 compressions of a message: block compressions of every chunk + parents
uint64_t msg_compressions(uint64_t len);

// whole-file work lists (item formats: cas_kernels.hip, k_whole_items / k_whole_merge8)
struct WholePlan {
    std::vector<sd_u32x4> full, tail, merge_a, merge_b;
    uint32_t n_cv = 0, n_cv2 = 0;  // pair-node CV slots, pass-A output slots
};
void plan_whole_items(WholePlan& p, const sd_extent* ext, size_t n);

// checksum batch plan: per-message tables, leaf workgroups, reduce passes
struct CkPlan {
    std::vector<ck_file> files;
    std::vector<sd_u32x2> wg_map;                 // leaf workgroup -> (message, 1 MiB block)
    std::vector<std::vector<ck_reduce_wg>> passes;  // reduce passes, level 0 -> 1 -> 0 ...
    uint64_t lvl_cap[2] = {0, 0};                 // CVs each level buffer must hold
    uint64_t total_bytes = 0, compressions = 0, blocks = 0;
};
void plan_checksum(CkPlan& p, const uint64_t* offsets, const uint64_t* lens, size_t n);
// The reduce passes alone -> p.passes and p.lvl_cap (raised, never lowered): message i has
// level_n[i] CVs from slot base[i] of the level-0 buffer, whatever bytes a CV covers (1 MiB
// leaf blocks for plan_checksum, the blocks of a checksum tree's level for its roots).
void plan_reduce_passes(CkPlan& p, std::vector<uint64_t> level_n, std::vector<uint64_t> base);

// ------------------------------------------------------------------ content-defined chunks (cdc_host.cpp)
// the gear table of include/sd_cas.h's content-defined chunks (256 entries)
const uint64_t* cdc_gear();
// throws SD_ERR_INVALID unless the parameters are valid
void cdc_check_params(const sd_cdc_params* p);
// the ranges' rule (16-byte aligned starts, the sum of ceil(len / min_size) plus n below 2^32);
// params already checked.  Returns the bytes of all files
uint64_t cdc_check_ranges(const uint64_t* offsets, const uint64_t* lens, size_t n, const sd_cdc_params& p);
// BLAKE3 compressions of a message of len bytes: its 64-byte blocks and its parents
inline uint64_t cdc_compressions(uint64_t len) {
    if (len == 0) return 1;
    const uint64_t chunks = (len + 1023) / 1024;
    return (len / 1024) * 16 + (len % 1024 + 63) / 64 + chunks - 1;
}
// the host half of sd_cdc_shared and the whole of sd_cpu_cdc_shared's checks: chunk_base ascends
// from 0, every file has a chunk, n < 2^32.  Returns m = chunk_base[n] (0 for n == 0)
uint64_t cdc_check_layout(const uint64_t* chunk_base, size_t n);
// the deltas' argument rules, both halves (cdc_delta_host.cpp).  _plan: cdc_check_layout, n_base <= n,
// no NULL table with slots; returns the target slots and leaves the first one at *t0
uint64_t cdc_delta_check_plan(const uint64_t* chunk_base, size_t n, size_t n_base, const void* chunks, const void* rep,
                              uint64_t* t0);
// _apply: counts below 2^32, no NULL array with entries, no NULL buffer that a length says is read
void cdc_delta_check_apply(const void* runs, uint64_t n_runs, const uint64_t* base_offsets, const uint64_t* base_lens,
                           size_t n_base, const void* base, const void* lit, uint64_t lit_bytes,
                           const uint64_t* out_offsets, const uint64_t* out_lens, size_t n_targets, const void* out);

// ------------------------------------------------------------------ checksum trees
// nb of include/sd_cas.h's checksum trees; block_log2 already checked
inline uint64_t tree_nodes(uint64_t len, uint32_t block_log2) {
    return len == 0 ? 1 : ((len - 1) >> block_log2) + 1;
}
// node_base[0 .. n] of a batch; throws SD_ERR_INVALID on a block_log2 outside
// [SD_TREE_BLOCK_LOG2_MIN, SD_TREE_BLOCK_LOG2_MAX]
void plan_tree_layout(const uint64_t* lens, size_t n, uint32_t block_log2, std::vector<uint64_t>& node_base);
// one listed block (include/sd_cas.h, listed blocks; k_ck_blocks, cas_kernels.hip): 32 bytes
struct ck_block_item {
    uint64_t src;     // byte offset of the block's bytes in the data buffer
    uint64_t chunk0;  // counter of its first chunk: j * B / 1024
    uint32_t len;     // its bytes, 0 .. B (0: the empty file)
    uint32_t root;    // its file has one node: ROOT on its last compression
    uint64_t dst;     // its slot in the batch's level layout: node_base[f] + j
};
static_assert(sizeof(ck_block_item) == 32, "two 16-byte loads per item");
// A block list checked and planned: node_base[0 .. n_files], one item per row, whether a (file,
// block) repeats, the bytes and compressions of its items.  Throws SD_ERR_INVALID on a block_log2
// out of range, a file or block past the end, a start that is not 16-byte aligned.
struct TreeBlocksPlan {
    std::vector<uint64_t> node_base;
    std::vector<ck_block_item> items;
    bool repeats = false;
    uint64_t bytes = 0, compressions = 0;
};
void plan_tree_blocks(TreeBlocksPlan& p, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                      const uint64_t* rows, const uint64_t* data_offsets, size_t m);

// Block proofs (include/sd_cas.h, block proofs).  Level L of a file of nb nodes has n_L nodes, n_0 =
// nb, n_{L+1} = ceil(n_L / 2); the height h = ceil(log2 nb) is the first L with n_L == 1.
inline uint32_t tree_height(uint64_t nb) {
    uint32_t h = 0;
    for (uint64_t n = nb; n > 1; n = (n + 1) >> 1) h++;
    return h;
}
// p(len, k, j): the levels at which block j's node has a sibling (nb from tree_nodes, j < nb)
inline uint32_t tree_proof_entries(uint64_t nb, uint64_t j) {
    uint32_t p = 0;
    for (uint64_t n = nb; n > 1; n = (n + 1) >> 1, j >>= 1) p += (j ^ 1) < n;
    return p;
}
// one row of a list for the proof kernels (k_tree_proof_gather, proof_climb; checksum_tree.hip): 32 bytes
struct ck_proof_row {
    uint64_t node0;    // node_base[f]: the file's first slot of the level layout
    uint64_t nb;       // the file's nodes
    uint64_t pbase;    // proof_base[r]: the row's first entry among the packed proofs
    uint32_t lvl_tab;  // index into lvl_off of the file's level 1 (prove; 0 when the file has none)
    uint32_t file;
};
static_assert(sizeof(ck_proof_row) == 32, "two 16-byte loads per row");
// one workgroup of an interior-levels pass (k_tree_levels): up to 256 consecutive nodes of one
// file's level 8p, reduced through `levels` levels, each of them stored
struct ck_levels_wg {
    uint64_t src_base;  // the group's first node in the source buffer (the caller's level, or the scratch)
    uint64_t first;     // its index within the file's source level: a multiple of 256
    uint32_t count;     // nodes in this group (1..256)
    uint32_t levels;    // levels to store (1..8)
    uint32_t lvl_tab;   // index into lvl_off of the first level stored
    uint32_t pad;
};
static_assert(sizeof(ck_levels_wg) == 32, "two 16-byte loads per workgroup");
// A list's proofs planned from node_base[0 .. n_files] and the rows.  Throws SD_ERR_INVALID on a
// file or block past the end.  With `levels`: the scratch layout of the interior levels 1 .. h - 1
// of every listed file (lvl_off, in nodes) and the passes that fill it, 8 levels a pass.
struct TreeProofPlan {
    std::vector<ck_proof_row> prow;
    std::vector<uint64_t> proof_base;  // m + 1
    bool levels = false;
    std::vector<uint64_t> lvl_off;
    std::vector<std::vector<ck_levels_wg>> passes;
    uint64_t scratch_nodes = 0;
};
void plan_tree_proofs(TreeProofPlan& p, const std::vector<uint64_t>& node_base, const uint64_t* rows, size_t m,
                      bool levels);

// Range proofs (include/sd_cas.h, range proofs): blocks [a, a + cnt) of a file of nb nodes, cnt >= 1,
// a + cnt <= nb.  At level L the range's nodes are lo = a >> L .. hi = (a + cnt - 1) >> L; the left
// flank exists iff lo is odd, the right one iff hi is even and hi + 1 < n_L.
inline uint32_t tree_range_proof_entries(uint64_t nb, uint64_t a, uint64_t cnt) {
    uint32_t p = 0;
    uint64_t lo = a, hi = a + cnt - 1;
    for (uint64_t n = nb; n > 1; n = (n + 1) >> 1, lo >>= 1, hi >>= 1) p += (uint32_t)(lo & 1) + (!(hi & 1) && hi + 1 < n);
    return p;
}
// one range of a list for k_tree_range_gather and range_differs (checksum_tree.hip): 48 bytes
struct ck_range_row {
    uint64_t node0;    // node_base[f]: the file's first slot of the level layout
    uint64_t nb;       // the file's nodes
    uint64_t first;    // a: the range's first block
    uint64_t count;    // its blocks
    uint64_t pbase;    // proof_base[i]: the range's first entry among the packed proofs
    uint32_t lvl_tab;  // index into lvl_off of the file's level 1 (prove; 0 when the file has none)
    uint32_t file;
};
static_assert(sizeof(ck_range_row) == 48, "three 16-byte loads per range");
// one workgroup of a climb pass (k_tree_range_climb): the nodes of one range that fall into one
// 256-aligned group of the file's level 8p, climbed through `levels` levels with the range's flanks
constexpr uint8_t CK_RANGE_FIRST = 1, CK_RANGE_LAST = 2, CK_RANGE_FINAL = 4;
struct ck_range_wg {
    uint64_t src_base;  // the group's first present node in the source (pass 0: the rows' nodes; else the scratch)
    uint64_t dst;       // where its top goes: a scratch slot, or the range (FINAL: top[dst])
    uint64_t pbase;     // the range's first entry of this pass among the packed proofs
    uint16_t count;     // present nodes (1..256), at slots start .. start + count - 1
    uint8_t start;      // (index of the first present node at level 8p) & 255
    uint8_t levels;     // levels to climb (0..8; 0: a file of one node, the node is the top)
    uint8_t lmask;      // bit l: the range has a left entry at level 8p + l
    uint8_t rmask;      // bit l: the range has a right entry at level 8p + l
    uint8_t flags;      // CK_RANGE_FIRST / _LAST: the range's first / last group; _FINAL: the pass reaches level h
    uint8_t pad;
};
static_assert(sizeof(ck_range_wg) == 32, "two 16-byte loads per workgroup");
// A list's ranges checked and planned from node_base, the rows and range_base[0 .. q].  Throws
// SD_ERR_INVALID (p untouched) unless range_base ascends strictly from 0 to m and every range's
// rows are consecutive blocks of one file.  `levels` is plan_tree_proofs over the ranges' first
// rows: the scratch layout (and, once asked for, the passes) of the interior levels of the files
// with a range, which k_tree_levels fills for the gather.
struct TreeRangePlan {
    bool set = false;
    std::vector<uint64_t> range_base;  // q + 1
    std::vector<uint64_t> proof_base;  // q + 1
    std::vector<ck_range_row> rrow;
    std::vector<uint64_t> firsts;                  // q x (file, first block): the rows `levels` is planned over
    std::vector<std::vector<ck_range_wg>> passes;  // ceil(h_max / 8), at least one when q > 0
    uint64_t scratch_nodes = 0;                    // the groups' tops between the passes
    TreeProofPlan levels;
    size_t q() const { return rrow.size(); }
};
void plan_tree_ranges(TreeRangePlan& p, const std::vector<uint64_t>& node_base, const uint64_t* rows, size_t m,
                      const uint64_t* range_base, size_t q);

// ------------------------------------------------------------------ fingerprints
// k_cas_gather (gather.hip) builds each file's cas message from its resident bytes.  Its
// output is cut into 16-byte units; the units of all files, in file order, form one flat
// space cut into tiles of SD_GATHER_TILE_UNITS units, one workgroup each, so a million
// small files cost as many workgroups as their bytes need and a sampled file 3.5.
struct gather_row {
    uint64_t data_off;  // first file byte in the data buffer (16-B aligned)
    uint64_t msg_off;   // the message's offset in the staged buffer
    uint64_t len;       // file length = the size hashed; the kind follows from it (cas.rs:27)
    uint64_t unit0;     // first 16-byte output unit of this file in the flat space
};
constexpr uint32_t SD_GATHER_TILE_UNITS = 1024;
struct GatherPlan {
    std::vector<sd_extent> extents;    // as sd_cas_stage_plan lays them out for sizes = lens
    std::vector<gather_row> rows;      // n files + one sentinel row (unit0 = units)
    std::vector<uint32_t> tile_first;  // tile t's units belong to files [tile_first[t], tile_first[t + 1]]
    uint64_t units = 0, staged_bytes = 0, file_bytes = 0, read_bytes = 0;
    uint32_t n_sampled = 0, n_whole = 0;
};
// throws SD_ERR_INVALID on a start that is not 16-byte aligned
void plan_gather(GatherPlan& p, const uint64_t* offsets, const uint64_t* lens, size_t n);
// The cas message of a file that holds exactly `len` bytes (cas.rs:25-58 on memory): le64(len)
// || file, or le64(len) || head || 4 samples || tail.  out holds 8 + min(len, 102400) or
// SD_SAMPLED_MSG_LEN bytes; returns the message length.
uint32_t cas_message_from_bytes(const uint8_t* file, uint64_t len, uint8_t* out);

// One file over R ranks (sd_split_range, include/sd_cas.h): nb = max(1, ceil(total / 1 MiB))
// blocks, rank r holds blocks [b0, b1) = [r*q, min((r+1)*q, nb)), q = ceil(nb / R), i.e.
// file bytes [off, off + len).  Throws SD_ERR_INVALID on a bad rank / rank count.
struct SplitPlan {
    uint64_t total = 0, nb = 1, q = 1, b0 = 0, b1 = 0, off = 0, len = 0;
    int nranks = 1, rank = 0;
    uint64_t cv_bytes() const { return (uint64_t)nranks * q * 32; }
};
SplitPlan split_plan(uint64_t total, int nranks, int rank);

// The multi-GPU dedup exchange (sd_cas_dedup_mgpu) as seen by rank `me` from the gathered
// rows of all R ranks, row r = [count to rank 0 .. count to rank R-1, index base, file
// count, output capacity, valid records].  Every rank derives `fits`, `consistent` and
// `ascending` from the same matrix, so all ranks take the same branch.  Records go out in destination order (the partition's
// order) and come in in source-rank order.
struct ExchangePlan {
    std::vector<uint64_t> send_cnt, send_off, recv_cnt, recv_off;  // per peer, in records
    uint64_t send_total = 0, recv_total = 0;
    bool fits = true;        // every rank's capacity holds what it receives
    bool consistent = true;  // every rank's counts add up to its valid records
    bool ascending = true;   // the ranks' index ranges ascend with the rank
};
constexpr int SD_EXCHANGE_ROW_EXTRA = 4;
ExchangePlan exchange_plan(const uint64_t* rows, int R, int me);

// The in-process communicator's rendezvous (sd_comm_group_create, dedup_mgpu.cpp): its
// ranks are threads of one process.  A generation barrier plus one published pointer pair
// per rank: a rank writes its slots before a barrier and reads its peers' after it, the
// barrier's mutex ordering the two.  A rank that never arrives (its thread failed) makes
// the others throw SD_ERR_COMM after `timeout_s` rather than hang.
struct sd_comm_group {
    int nranks = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t generation = 0;
    std::vector<const void*> slot_a, slot_b;
    std::vector<int> joined;
    double timeout_s = 120.0;
    explicit sd_comm_group(int n) : nranks(n), slot_a(n, nullptr), slot_b(n, nullptr), joined(n, 0) {}
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t gen = generation;
        if (++arrived == nranks) {
            arrived = 0;
            generation++;
            cv.notify_all();
            return;
        }
        // a system_clock deadline: libstdc++ waits on it with pthread_cond_timedwait, which
        // TSan intercepts (a steady_clock wait_for goes to pthread_cond_clockwait, which GCC
        // 11's TSan does not, and reads as a double lock); a clock step only moves a timeout
        const auto deadline = std::chrono::system_clock::now() +
                              std::chrono::duration_cast<std::chrono::system_clock::duration>(
                                  std::chrono::duration<double>(timeout_s));
        if (!cv.wait_until(lk, deadline, [&] { return generation != gen; })) {
            arrived--;
            throw sd_failure(SD_ERR_COMM, "in-process group: a rank did not reach the barrier in time");
        }
    }
};

// ------------------------------------------------------------------ file reading
// Reads one file's cas message into staged + e.msg_offset exactly as generate_cas_id reads
// it (cas.rs:25-58) and zero-pads it to the next 64-byte boundary.  Returns an
// sd_file_status:
//   whole kind: every byte read() returns until EOF (fs::read, cas.rs:29); e.msg_len is
//     set to 8 + that count.  SD_FILE_CHANGED if the file holds more bytes than the
//     extent's planned room (e.msg_len - 8 on entry): the reference would hash them all.
//     With `capture`, a file that is not a regular file (a pipe, a character device: its
//     bytes cannot be read a second time) is read to its end instead, all its bytes
//     (the room's, then the rest) going to *capture; the status is still SD_FILE_CHANGED
//     and the caller hashes le64(size) || *capture.  A regular file that grew is left
//     for the caller to re-read (it may be large).
//   sampled kind: read_exact of the head and the samples at their traced offsets
//     (SHORT_READ past EOF), then the footer at seek(End(-8192)) -- the file's real end,
//     EINVAL when it is shorter than 8192 bytes.
int32_t stage_one(const char* path, sd_extent& e, uint8_t* staged, std::vector<uint8_t>* capture = nullptr);
// pread until n bytes or EOF; returns the count, or -errno
int64_t pread_full(int fd, uint8_t* dst, uint64_t n, uint64_t off);
// pread_full's result, delivered through this thread's cache-resident 256 KiB buffer and
// streamed (non-temporal stores) into dst: the page-cache copy lands in L2 and the
// destination -- a pinned window the GPU will DMA -- is written without being read first.
// On the MI355X box's host this costs 0.068 ns/B against 0.087 for pread straight into the
// pinned window and 0.172 for pread + BLAKE3 (scripts/ck_host_cost.cpp,
// profiles/r4/r4b_ck_host_cost.jsonl).  Same return convention as pread_full.
int64_t pread_stream(int fd, uint8_t* dst, uint64_t n, uint64_t off);

// A message read front to back from a file: optional le64 prefix (a cas message's size
// header), optional bytes already read from the file, then the file itself.
class MsgSource {
public:
    enum Mode {
        READ_TO_EOF,     // fs::read (cas.rs:29): read() until it returns 0
        CHECKSUM_READS,  // hash.rs:14-20: one read() of 1 MiB per call until one returns fewer
    };
    static constexpr uint64_t CHECKSUM_READ = SD_CK_BLOCK;
    MsgSource(int fd, Mode m) : fd_(fd), mode_(m) {}
    void set_prefix_le64(uint64_t v);
    // a message held in memory: after the prefix, exactly these bytes, then the end
    void set_memory(const uint8_t* p, uint64_t n) {
        pend_ = p;
        pend_len_ = n;
        mem_only_ = true;
    }
    // the file's first n bytes, already taken from it (whole 1 MiB reads in CHECKSUM_READS mode)
    void set_pending(const uint8_t* p, uint64_t n) {
        pend_ = p;
        pend_len_ = n;
        file_pos_ = n;
    }
    // A regular file (S_ISREG) read in CHECKSUM_READS mode: hash.rs's 1 MiB reads until a
    // short one return exactly the bytes up to EOF, so each window is filled with 1 MiB
    // preads at their offsets in parallel on `pool`, and ends at the first short piece.
    // At most `threads` of the pool's threads read one window; `stream` delivers the pieces
    // through pread_stream (a pinned destination) instead of pread straight into dst.
    void set_parallel(StagePool* pool, int threads = 1 << 30, bool stream = false) {
        pool_ = pool;
        par_threads_ = threads;
        par_stream_ = stream;
    }
    // A regular file's stat length: when the reads reach exactly that many file bytes, one
    // 1-byte pread past it decides whether the message has ended (a read there returns 0,
    // as the reference's next read would), so a reader of W-byte windows learns the end
    // with the last full window instead of from an extra, empty one.  A file that grew
    // keeps going: nothing is consumed by the probe.
    void set_eof_hint(uint64_t file_len) {
        eof_hint_ = file_len;
        has_eof_hint_ = true;
    }
    // Writes up to n message bytes to dst and returns the count; fewer than n only at the
    // end of the message (done) or on an error (err = errno).  CHECKSUM_READS: n is a
    // multiple of 1 MiB.
    uint64_t read(uint8_t* dst, uint64_t n);
    bool done = false;
    int err = 0;

private:
    uint64_t read_parallel(uint8_t* dst, uint64_t n);
    uint64_t read_impl(uint8_t* dst, uint64_t n);
    int fd_;
    Mode mode_;
    StagePool* pool_ = nullptr;
    int par_threads_ = 1 << 30;
    bool par_stream_ = false;
    uint64_t file_pos_ = 0;  // bytes taken from the file so far
    uint8_t prefix_[8] = {};
    uint32_t prefix_len_ = 0, prefix_pos_ = 0;
    const uint8_t* pend_ = nullptr;
    uint64_t pend_len_ = 0;
    uint64_t eof_hint_ = 0;
    bool has_eof_hint_ = false;
    bool mem_only_ = false;
};

// ------------------------------------------------------------------ CPU BLAKE3 (cpu_blake3.cpp)
// The library's own CPU hasher: the BLAKE3 spec's incremental chunk / CV-stack structure,
// with whole chunks hashed many at a time across SIMD lanes (AVX-512 16-way, AVX2 8-way,
// portable 1-way, picked at run time).  Used by the sd_cpu_* entry points and the
// latency path's CPU route.
class CpuHasher {
public:
    CpuHasher();
    // a subtree whose first chunk has index chunk0 (a 1 MiB block of a longer message)
    explicit CpuHasher(uint64_t chunk0);
    void update(const uint8_t* p, size_t n);
    void finalize(uint8_t out[32]) const;
    // the subtree's chaining value: no ROOT flag (a block of a message of several blocks)
    void finalize_cv(uint8_t out[32]) const;

private:
    static constexpr uint32_t BLOCK_CHUNKS = 1024;  // 1 MiB: the unit merged level-wise
    void push_chunk_cv(const uint32_t cv[8]);
    void finish(uint8_t out[32], bool root) const;
    // chunk CVs of the current 1 MiB block, merged level-wise (SIMD parents) when it is
    // complete; complete blocks' CVs on a stack that merges every completed subtree
    // (the first SMALL_CHUNKS CVs inline: a cas message never needs the heap -- a 32 KiB
    // allocation per message cost the 16-thread CPU path a third of its rate)
    static constexpr uint32_t SMALL_CHUNKS = 128;
    uint32_t (*blk())[8] { return big_ ? big_.get() : small_; }
    const uint32_t (*blk() const)[8] { return big_ ? big_.get() : small_; }
    uint32_t small_[SMALL_CHUNKS][8];
    std::unique_ptr<uint32_t[][8]> big_;  // BLOCK_CHUNKS entries, once a message outgrows small_
    uint32_t nblk_ = 0;
    uint32_t stack_[48][8];
    int sp_ = 0;
    uint64_t blocks_ = 0;  // complete blocks pushed so far
    uint64_t ctr0_ = 0;    // chunk index of the first chunk
    uint64_t chunks_ = 0;  // complete chunks pushed so far
    uint8_t buf_[1024];
    uint32_t buf_len_ = 0;
};
void cpu_blake3(const uint8_t* p, size_t n, uint8_t out[32]);
// BLAKE3 of n messages, the chunks of all of them packed across the SIMD lanes together
// (cas messages of a few chunks each); out[i] = the hash of msg[i][0, len[i])
void cpu_blake3_batch(const uint8_t* const* msg, const uint64_t* len, size_t n, uint8_t (*out)[32]);
// BLAKE3 root of a message from its nb >= 2 consecutive 1 MiB block CVs (32 B each)
void cpu_root_from_cvs(const uint8_t* cvs, uint64_t nb, uint8_t out[32]);
// one parent node from its two children's 32 bytes each (ROOT on it when `root`); out may be l or r
void cpu_parent(const uint8_t l[32], const uint8_t r[32], bool root, uint8_t out[32]);
// the (non-root) chaining values of 1 MiB blocks [b0, b1) of a message of total_len >= 2
// blocks, on nthreads threads: block b's 32 bytes at cvs + 32 * b
void cpu_block_cvs(const uint8_t* msg, uint64_t total_len, uint64_t b0, uint64_t b1, uint8_t* cvs, int nthreads);
// fn(i) for i in [0, n) on up to nthreads threads of the CPU path's persistent pools (the
// caller's included; capped by the host budget)
void cpu_parallel_for(size_t n, int nthreads, const std::function<void(size_t)>& fn);
// sd_checksums' co-hashing: the index of the range of >= min_len bytes
// nearest the byte where the GPU (gpu_gbps, from the front) and host_threads host threads
// (thread_gbps each, from the back) are predicted to meet; the first of equally near ones;
// SIZE_MAX if no range is that long
size_t shared_range_pick(const uint64_t* lens, size_t n, uint64_t min_len, int host_threads, double gpu_gbps,
                         double thread_gbps);
// lanes of the SIMD chunk hasher this CPU runs (16, 8 or 1)
int cpu_lanes();
// generate_cas_id / file_checksum of one file on the calling thread -> sd_file_status
int32_t cpu_cas_id_file(const char* path, uint64_t size, char out_hex17[17]);
int32_t cpu_checksum_file(const char* path, char out_hex65[65]);
// the (non-root) chaining value of 1 MiB block `block` of a regular file of file_len >= 2
// blocks, read from fd at its offset ("cpu_read_piece_kib" pieces); false on a short read
bool cpu_block_cv_fd(int fd, uint64_t file_len, uint64_t block, uint8_t cv[32]);

// sd_file_checksums' route for a call the split applies to, learned per context (round 5:
// the split lost 7 % to the CPU path alone on a host whose CPU path read and hashed 103 GB/s
// from files, and won 34 % on one at 78).  rate[r] is the EWMA of GB/s of
// route r's past calls (0 = the split, 1 = the CPU path alone), n[r] how many were counted
// -- a route's first call in the context is not (it pays for its pinned windows and pools:
// a split's first call ran at 82 GB/s against 100+ after) -- and each route runs until one
// call is counted, then the faster one, and every explore_every-th call the other (0 = never).
struct SplitRoutes {
    double rate[2] = {0.0, 0.0};
    uint32_t n[2] = {0, 0};
    uint32_t seen[2] = {0, 0};  // calls recorded per route, the uncounted first included
    uint64_t calls = 0;         // counted calls
};
int split_route_choose(const SplitRoutes& s, uint32_t explore_every);
void split_route_record(SplitRoutes& s, int route, double gbps);
// bumped by sd_cas_set_tuning when a key either route's rate depends on changes value
// (read_threads, checksum_hybrid_threads, host_cpu_budget, checksum_split_blocks,
// cpu_read_piece_kib, checksum_stage_hot, numa_pin, host_cohash_threads): a context's
// learned rates from before are dropped at its next eligible call
uint64_t split_route_tuning_gen();
// co-hashing threads of a sd_checksums call under a host budget of b: b less 3/16 of it, at
// least one less (16 -> 13, 8 -> 6, 4 -> 3, 2 -> 1, 1 -> 0)
inline int checksum_cohash_cap(int b) { return b <= 1 ? 0 : b - std::max(1, (3 * b + 8) / 16); }

// ------------------------------------------------------------------ claim protocols
// Who hashes what in a call that the GPU and host threads share.  Host-only state machines:
// host_selftest.cpp drives each with threads under ASan + UBSan and TSan.

// A context's SplitRoutes with the tuning generation they were learned under.
class LearnedRoute {
public:
    // this call's route; a change of split_route_tuning_gen() starts the learning again
    int begin(uint32_t explore_every);
    // the call took `route` for `bytes` bytes and started at t0
    void record(int route, uint64_t bytes, std::chrono::steady_clock::time_point t0);
    SplitRoutes snapshot();

private:
    std::mutex mu_;
    SplitRoutes r_;
    uint64_t gen_ = 0;
};

// n items claimed from both ends: [0, front) by the front side (the GPU loop), [back, n) by
// the back side (host threads), until the two meet.  One item may be `shared`: neither side
// claims it whole; the front side takes its blocks [0, sf) on reaching it, the back side
// [sb, nb) once every item after it is claimed, and a back block claim stays in flight until
// its done-marker runs.
class EndClaims {
public:
    static constexpr size_t NONE = SIZE_MAX;
    explicit EndClaims(size_t n, size_t shared = NONE, uint64_t shared_blocks = 0)
        : back_(n), shared_(shared), sb_(shared == NONE ? 0 : shared_blocks) {}

    // The back side takes items [b0, b1): the last unclaimed one, then further ones, at most
    // max_items in all, while more(j, b1) holds for the next one, j ([j + 1, b1) being taken
    // so far).  False when nothing is left for it.
    template <class More>
    bool back_claim(size_t max_items, size_t& b0, size_t& b1, More more) {
        std::lock_guard<std::mutex> g(mu_);
        if (!back_open_) return false;
        if (back_ > front_ && back_ - 1 == shared_) back_ = shared_;  // its blocks only: back_blocks
        if (back_ <= front_) return false;
        b1 = back_;
        b0 = b1 - 1;
        while (b0 > front_ && b1 - b0 < max_items && b0 - 1 != shared_ && more(b0 - 1, b1)) b0--;
        back_ = b0;
        return true;
    }
    // The front side takes items from `from` on while the back side has not claimed them (the
    // shared item it never has) and take(i) accepts them; the first index not taken.
    template <class Take>
    size_t front_claim(size_t from, Take take) {
        std::lock_guard<std::mutex> g(mu_);
        size_t i = from;
        while (front_open_ && (i < back_ || i == shared_) && take(i)) i++;
        front_ = std::max(front_, i);
        return i;
    }
    bool front_claim(size_t i) {
        return front_claim(i, [i](size_t q) { return q == i; }) > i;
    }
    // after a failed front_claim(i): the shared item if it lies ahead (the back side may have
    // claimed whole items on both sides of it), else NONE
    size_t front_skip(size_t i) {
        std::lock_guard<std::mutex> g(mu_);
        return front_open_ && shared_ != NONE && shared_ > i ? shared_ : NONE;
    }
    // The shared item's blocks [w0, w1) for the front side: at most `max`, shrinking to a
    // third of what is left (>= 32 blocks), so the GPU's last windows in flight are short
    // when the two sides meet.
    bool front_blocks(uint64_t max, uint64_t& w0, uint64_t& w1) {
        std::lock_guard<std::mutex> g(mu_);
        if (!front_open_ || sf_ >= sb_) return false;
        w0 = sf_;
        w1 = std::min(sb_, w0 + std::min<uint64_t>(max, std::max<uint64_t>(32, (sb_ - w0) / 3)));
        sf_ = w1;
        return true;
    }
    // Its blocks [u0, u1) for the back side, `unit` at a time, once every item after the
    // shared one is claimed.  Each claim is in flight until its BlocksDone goes.
    bool back_blocks(uint64_t unit, uint64_t& u0, uint64_t& u1) {
        std::lock_guard<std::mutex> g(mu_);
        if (!back_open_ || sb_ <= sf_ || back_ > shared_ + 1) return false;
        u1 = sb_;
        u0 = std::max(sf_, u1 > unit ? u1 - unit : 0);
        sb_ = u0;
        inflight_++;
        return true;
    }
    struct BlocksDone {  // a back block claim's done-marker: on every exit, so wait_back_blocks ends
        EndClaims& c;
        ~BlocksDone() {
            {
                std::lock_guard<std::mutex> g(c.mu_);
                c.inflight_--;
            }
            c.cv_.notify_all();
        }
    };
    // waits until no back block claim is in flight; the back side's first block
    uint64_t wait_back_blocks() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return inflight_ == 0; });
        return sb_;
    }
    // the back side takes nothing further (what it holds stays its own)
    void stop_back() {
        std::lock_guard<std::mutex> g(mu_);
        back_open_ = false;
    }
    // the front side takes nothing further
    void stop_front() {
        std::lock_guard<std::mutex> g(mu_);
        front_open_ = false;
    }
    struct StopBack {  // a caller's guard: declared after everything the back side's threads touch
        EndClaims& c;
        std::vector<std::thread>& t;
        ~StopBack() {
            c.stop_back();
            for (auto& x : t)
                if (x.joinable()) x.join();
        }
    };

private:
    std::mutex mu_;
    std::condition_variable cv_;
    size_t front_ = 0, back_;
    const size_t shared_;
    uint64_t sf_ = 0, sb_;
    int inflight_ = 0;
    bool front_open_ = true, back_open_ = true;
};

// sd_file_checksums' block split: the 1 MiB blocks of every large file as one queue in file
// order, file q's being [fb[q], fb[q + 1]) of all.  A claim never spans two files.  It has no
// lock of its own: split_checksums_blocks asks and claims under its slot lock, as one step.
class BlockQueue {
public:
    static constexpr uint64_t GPU_RUN = 32;  // blocks per GPU claim while plenty is left
    BlockQueue(const std::vector<uint64_t>& fb, int threads) : fb_(fb), threads_(threads), left_(fb.back()) {}
    uint64_t left() const { return left_; }
    // blocks [b0, b1) of file q, at most `want`
    bool claim(uint64_t want, size_t& q, uint64_t& b0, uint64_t& b1);
    // what a GPU slot asks for: its runs shrink towards the end, so its last ones finish with the host's
    uint64_t gpu_run() const { return std::max<uint64_t>(4, std::min<uint64_t>(GPU_RUN, left_ / (2 * (uint64_t)threads_))); }

private:
    const std::vector<uint64_t>& fb_;
    const int threads_;
    size_t cf_ = 0;  // the cursor: file cf_, its block cb_
    uint64_t cb_ = 0, left_;
};

// One packed window of sd_checksums: ranges i.. whose device layout fits W bytes.
struct RangeWindow {
    struct Run {  // a piece of the window copied with one H2D
        uint64_t host_lo, host_end, dev_lo;
    };
    std::vector<Run> runs;
    std::vector<uint64_t> offs, lens;  // the taken ranges' device offsets and lengths
};
// Fills `w` from range i on and returns the first index not taken.  Range i is the caller's
// already; each further one is taken only if claim(j) grants it.
size_t plan_range_window(const uint64_t* offsets, const uint64_t* lens, size_t i, size_t n, uint64_t W,
                         const std::function<bool(size_t)>& claim, RangeWindow& w);
void hex_lower(const uint8_t* h, int nbytes, char* out);
