// sd_api_impl.h -- the host-side types shared by the C ABI's translation units
// (sd_cas_api.cpp: context, batches, dedup; sd_files.cpp: the file readers' pipelines and
// streaming): device / pinned buffers, stream slots, the opaque ABI structs.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "sd_host.h"
#include "sd_internal.h"
#include "stage_pool.h"

#define HIP_CHECK(expr)                                                                              \
    do {                                                                                             \
        hip_thread_check(#expr); /* never on a private-fd-table thread (sd_host.h) */                \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            throw sd_failure(e_ == hipErrorOutOfMemory ? SD_ERR_NOMEM : SD_ERR_DEVICE,              \
                             std::string(#expr) + ": " + hipGetErrorString(e_));                    \
    } while (0)

namespace sdi {

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
inline void to_hex(const uint8_t* h, int nbytes, char* out) { hex_lower(h, nbytes, out); }

// RAII device buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void alloc(size_t n) {
        reset();
        if (n == 0) n = 16;
        HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
    }
    // grow-only (never frees a buffer that is large enough: hipFree synchronises the device)
    void ensure(size_t n) {
        if (n > bytes) alloc(n);
    }
    // grow keeping the contents (the caller has synchronised every stream writing it)
    void grow_preserve(size_t n) {
        if (n <= bytes) return;
        void* q = nullptr;
        HIP_CHECK(hipMalloc(&q, n));
        if (p) {
            const hipError_t e = hipMemcpy(q, p, bytes, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) {
                (void)hipFree(q);
                HIP_CHECK(e);
            }
            (void)hipFree(p);
        }
        p = q;
        bytes = n;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
    template <class T>
    void upload(const std::vector<T>& v, hipStream_t s = nullptr) {
        ensure(v.size() * sizeof(T));
        if (v.empty()) return;
        if (s) HIP_CHECK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
        else HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    }
};

struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() { reset(); }
    void reset() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    void ensure(size_t n) {
        if (n <= bytes) return;
        reset();
        HIP_CHECK(hipHostMalloc(&p, n, hipHostMallocDefault));
        bytes = n;
    }
    uint8_t* u8() const { return reinterpret_cast<uint8_t*>(p); }
};

// A plan's host tables packed into one pinned buffer and copied to one device buffer with
// a single H2D: one DMA the host does not wait on, instead of an allocation and a staged
// pageable copy per table (those cost ~12 us each, most of a small batch's host time).
// add() queues a table at a 16-byte aligned offset; upload() packs and copies.  The pinned
// buffer is read by the async copy: the caller syncs the stream before the next upload
// (every plan is rebuilt only after its previous run has drained).
struct Tables {
    PinnedBuf host;
    DevBuf dev;
    std::vector<std::pair<const void*, size_t>> parts;
    std::vector<size_t> offs;
    size_t bytes = 0;
    void begin() {
        parts.clear();
        offs.clear();
        bytes = 0;
    }
    template <class T>
    size_t add(const std::vector<T>& v) {
        const size_t o = bytes;
        parts.emplace_back(v.data(), v.size() * sizeof(T));
        offs.push_back(o);
        bytes = align_up(o + v.size() * sizeof(T), 16);
        return o;
    }
    void upload(hipStream_t s) {
        if (bytes == 0) return;
        host.ensure(bytes);
        dev.ensure(bytes);
        for (size_t k = 0; k < parts.size(); k++)
            if (parts[k].second) memcpy(host.u8() + offs[k], parts[k].first, parts[k].second);
        if (s) HIP_CHECK(hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, s));
        else HIP_CHECK(hipMemcpy(dev.p, host.p, bytes, hipMemcpyHostToDevice));
    }
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>(reinterpret_cast<uint8_t*>(dev.p) + off); }
};

}  // namespace sdi

struct sd_checksum_batch {
    size_t n = 0;
    CkPlan plan;
    sdi::Tables tab;  // files, wg_map, then one table per reduce pass
    size_t o_files = 0, o_map = 0;
    std::vector<size_t> o_pass;
    sdi::DevBuf lvl[2];
    const ck_file* d_files() const { return tab.at<ck_file>(o_files); }
    const uint2* d_map() const { return tab.at<uint2>(o_map); }
    const ck_reduce_wg* d_pass(size_t k) const { return tab.at<ck_reduce_wg>(o_pass[k]); }
};

// a checksum batch that also leaves every file's level at 2^block_log2-byte granularity
// (include/sd_cas.h, checksum trees; checksum_tree.hip)
struct sd_checksum_tree {
    uint32_t block_log2 = 0;
    sd_checksum_batch ck;             // the leaf tables and the reduce over 1 MiB CVs: _run's roots
    std::vector<uint64_t> node_base;  // n + 1
    CkPlan roots;                     // reduce passes whose level 0 is the level itself: _roots
    sdi::Tables tab;                  // node_base, then one table per pass of `roots`
    size_t o_base = 0;
    std::vector<size_t> o_pass;
    sdi::DevBuf lvl[2];               // _roots' levels above the caller's (pass k writes lvl[1 - (k & 1)])
    uint64_t total() const { return node_base.empty() ? 0 : node_base.back(); }
    const uint64_t* d_base() const { return tab.at<uint64_t>(o_base); }
    const ck_reduce_wg* d_pass(size_t k) const { return tab.at<ck_reduce_wg>(o_pass[k]); }
};

// listed blocks of a batch of files (include/sd_cas.h, listed blocks; checksum_tree.hip)
struct sd_checksum_tree_blocks {
    uint32_t block_log2 = 0;
    size_t n_files = 0;
    TreeBlocksPlan plan;         // node_base, the items, whether a (file, block) repeats
    std::vector<uint64_t> rows;  // m x (file, block): what _verify reports
    sdi::Tables tab;             // the items, then the rows: one upload
    size_t o_items = 0, o_rows = 0;
    // _update's roots, planned by the first _update: node_base and the reduce passes over the level
    bool roots_planned = false;
    CkPlan roots;
    sdi::Tables rtab;
    size_t o_base = 0;
    std::vector<size_t> o_pass;
    sdi::DevBuf lvl[2];
    // the proofs, planned by the first proof call: the rows' table and the listed files' level
    // offsets (ptab); _prove's passes (ltab) and the interior levels they fill (levels)
    TreeProofPlan proofs;
    sdi::Tables ptab, ltab;
    size_t o_prow = 0, o_lvl = 0;
    std::vector<size_t> o_lpass;
    sdi::DevBuf levels;
    const ck_proof_row* d_prow() const { return ptab.at<ck_proof_row>(o_prow); }
    const uint64_t* d_lvl_off() const { return ptab.at<uint64_t>(o_lvl); }
    const ck_levels_wg* d_lpass(size_t k) const { return ltab.at<ck_levels_wg>(o_lpass[k]); }
    // the ranges (_set_ranges, GPU-free): their rows and climb passes go up with the first range
    // call after it (gtab), with the scratch of the groups' tops between the passes (tops);
    // _prove_ranges' level offsets and passes (gltab) and the interior levels they fill (rlevels)
    TreeRangePlan ranges;
    bool ranges_up = false;
    sdi::Tables gtab, gltab;
    size_t o_rrow = 0, o_rlvl = 0;
    std::vector<size_t> o_gpass, o_rlpass;
    sdi::DevBuf tops, rlevels;
    const ck_range_row* d_rrow() const { return gtab.at<ck_range_row>(o_rrow); }
    const ck_range_wg* d_gpass(size_t k) const { return gtab.at<ck_range_wg>(o_gpass[k]); }
    const uint64_t* d_rlvl_off() const { return gltab.at<uint64_t>(o_rlvl); }
    const ck_levels_wg* d_rlpass(size_t k) const { return gltab.at<ck_levels_wg>(o_rlpass[k]); }
    size_t m() const { return plan.items.size(); }
    uint64_t total() const { return plan.node_base.back(); }
    const ck_block_item* d_items() const { return tab.at<ck_block_item>(o_items); }
    const uint64_t* d_rows() const { return tab.at<uint64_t>(o_rows); }
    const uint64_t* d_base() const { return rtab.at<uint64_t>(o_base); }
    const ck_reduce_wg* d_pass(size_t k) const { return rtab.at<ck_reduce_wg>(o_pass[k]); }
};

// one file over the ranks of a communicator (include/sd_cas.h, sd_split_range)
struct sd_split_checksum {
    SplitPlan sp;
    sd_checksum_batch plan;  // the whole file as one message: leaf table + reduce passes
};

struct sd_cas_batch {
    size_t n = 0;
    uint32_t n_sampled = 0, n_whole = 0, n_long = 0;
    uint64_t compressions = 0, msg_bytes = 0, staged_bytes = 0, whole_chunks = 0;
    WholePlan whole;  // work lists (kernel formats in cas_kernels.hip, k_whole_items / _merge8)
    sdi::Tables tab;  // the sampled files' rows and offsets, the work lists, the long-message rows
    size_t o_sidx = 0, o_soff = 0, o_full = 0, o_tail = 0, o_ma = 0, o_mb = 0, o_lidx = 0, o_wrows = 0;
    bool whole_wave = false;  // n_whole <= "whole_wave_max" at plan time: one workgroup per file
    sdi::DevBuf cvbuf, cv2;
    bool sampled_wave = false;  // n_sampled <= "sampled_wave_max" at plan time: one wave per file
    sdi::DevBuf srows;          // otherwise the sampled files' node CVs between the two kernels
    // whole-file messages longer than SD_WHOLE_ITEMS_MAX: a checksum sub-batch over their
    // byte ranges, its hashes scattered to out[long_idx[i]]
    sd_checksum_batch lng;
    sdi::DevBuf long_out;
    // host tables (packed into tab by the plan)
    std::vector<uint32_t> h_sidx, h_long_idx;
    std::vector<sd_u32x4> h_wrows;  // whole_wave: (u64 message offset, length, output row)
    std::vector<uint64_t> h_soff;
    const uint32_t* d_sidx() const { return tab.at<uint32_t>(o_sidx); }
    const uint64_t* d_soff() const { return tab.at<uint64_t>(o_soff); }
    const uint4* d_full() const { return tab.at<uint4>(o_full); }
    const uint4* d_tail() const { return tab.at<uint4>(o_tail); }
    const uint4* d_ma() const { return tab.at<uint4>(o_ma); }
    const uint4* d_mb() const { return tab.at<uint4>(o_mb); }
    const uint32_t* d_lidx() const { return tab.at<uint32_t>(o_lidx); }
    const uint4* d_wrows() const { return tab.at<uint4>(o_wrows); }
};

// cas_id and checksum of files that are byte ranges of one device buffer (sd_fingerprint.cpp):
// the gather's tables, the two batches it feeds, and the staged messages between them
struct sd_fingerprint_batch {
    size_t n = 0;
    GatherPlan gp;
    sdi::Tables tab;  // rows, tile_first
    size_t o_rows = 0, o_tiles = 0;
    sd_cas_batch cas;
    sd_checksum_batch ck;
    sdi::DevBuf scratch;  // gp.staged_bytes: what the gather writes and the cas kernels read
    const gather_row* d_rows() const { return tab.at<gather_row>(o_rows); }
    const uint32_t* d_tiles() const { return tab.at<uint32_t>(o_tiles); }
};

// The device-resident Object index (object_index.cpp; layout in object_index.h): two
// buffers of `cap` keys and values swapped by an insert or a removal, the prefix directory,
// and scratch of its own (an insert's sort and compaction; a removal's flags and sorted ids;
// the per-workgroup counts of an ordered compaction), so no call borrows a context slot it
// could not hold until its kernels ran.
struct sd_object_index {
    sd_cas_ctx* ctx = nullptr;
    int nparts = 1, part = 0;
    uint64_t n = 0, cap = 0;
    uint32_t bits = 0;
    int cur = 0;                        // which buffer pair holds the index
    int flags = 0;                      // SD_OBJECT_INDEX_OWNERS: one entry per (key, Object id) + links
    sdi::DevBuf keys[2], vals[2], dir;  // dir: 2^bits + 1 offsets
    sdi::DevBuf links[2];               // owners mode: the third array beside keys / vals, grown with them
    sdi::DevBuf counts;                 // OI_COUNT_SLOTS u64, then one device count
    sdi::DevBuf scratch;                // sdk::index_insert_scratch / index_remove_scratch
    sdi::PinnedBuf host;                // an insert's survivor count; a removal's per-slice counts
    sdi::PinnedBuf objects_host;        // sd_object_index_orphans' per-slice counts, and those and the stats of
                                        // the view by key: reads of their own, which may run beside
                                        // sd_cas_dedup_mgpu_indexed's use of `host`
    bool owners() const { return (flags & SD_OBJECT_INDEX_OWNERS) != 0; }
    sdk::oi_view view() const {
        return {keys[cur].as<uint64_t>(), vals[cur].as<uint64_t>(), dir.as<uint64_t>(), n, bits,
                owners() ? links[cur].as<uint64_t>() : nullptr};
    }
};

namespace sdi {

// per-call working set of the host drop-in entry points; its batches persist with the slot
// in the context's pool, so a call reuses their device and pinned tables
struct Slot {
    hipStream_t stream = nullptr;
    DevBuf staged, hashes;
    PinnedBuf host_hashes, window;
    Tables aux;  // a call's own tables (the split checksum's block map), grown with the slot
    sd_cas_batch cas;
    sd_checksum_batch ck;
    sd_fingerprint_batch fp;  // sd_fingerprints' window
    hipEvent_t drained = nullptr;  // sync()'s blocking-sync event
    Slot() = default;
    Slot(const Slot&) = delete;
    Slot& operator=(const Slot&) = delete;
    ~Slot() {
        if (drained) (void)hipEventDestroy(drained);
    }
    // Waits for the stream's queued work with the thread asleep (a blocking-sync event), as
    // the file stager's waits do: the reader and co-hash threads beside it share the host
    // budget.  (A/B against hipStreamSynchronize, profiles/r4/r4l_sync_ab/: no difference
    // beyond the box's noise -- the runtime's own wait already sleeps after a short poll.)
    void sync() {
        if (!drained) HIP_CHECK(hipEventCreateWithFlags(&drained, hipEventDisableTiming | hipEventBlockingSync));
        HIP_CHECK(hipEventRecord(drained, stream));
        HIP_CHECK(hipEventSynchronize(drained));
    }
};

// The CDC deltas' working set (cdc_delta.hip), one per context: the segment lists and prefix sums
// of a pack or an apply (grown by sd_cdc_delta_plan and sd_cdc_delta_apply, so a pack allocates
// nothing), and the host tables, which go up through pinned memory: `up` marks the end of the last
// upload, after which the next call may overwrite them.
struct DeltaWork {
    DevBuf scratch;
    Tables tab;
    hipEvent_t up = nullptr;
    DeltaWork() = default;
    DeltaWork(const DeltaWork&) = delete;
    DeltaWork& operator=(const DeltaWork&) = delete;
    ~DeltaWork() {
        if (up) (void)hipEventDestroy(up);
    }
};

}  // namespace sdi

struct sd_cas_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::mutex coal_mu;
    sd_coalescer* coal = nullptr;  // latency path, created on the first single-file call
    std::atomic<uint64_t> files_calls_cpu{0}, files_calls_gpu{0};  // sd_cas_ids_files routes
    std::atomic<uint64_t> checksum_calls_cpu{0}, checksum_calls_gpu{0},  // sd_file_checksums routes
        checksum_calls_hybrid{0};
    // bytes (stat lengths) of the files sd_file_checksums gave the GPU route, and the CPU path
    // in split calls
    std::atomic<uint64_t> checksum_bytes_gpu{0}, checksum_bytes_cpu_split{0};
    std::atomic<uint64_t> cas_ids_gpu_files{0}, cas_ids_host_files{0};  // sd_cas_ids: who hashed
    std::atomic<uint64_t> checksums_gpu_bytes{0}, checksums_host_bytes{0};  // sd_checksums: who hashed
    // sd_fingerprints: bytes sent H2D, files gathered on the device, large ranges
    std::atomic<uint64_t> fp_h2d_bytes{0}, fp_gathered{0}, fp_large{0};
    // sd_dedup_confirm: calls that finished on the prefix path, calls that took the full-width path
    std::atomic<uint64_t> confirm_calls_prefix{0}, confirm_calls_full{0};
    LearnedRoute split_route;  // sd_file_checksums: the split or the CPU path, learned (sd_host.h)
    // sd_checksums' co-hashed calls: the GPU + host threads, or the CPU path alone, learned
    // the same way (route 0 = co-hash, 1 = CPU path)
    LearnedRoute cohash_route;
    std::mutex pool_mu;
    // Reader threads.  stage_pool: tasks that open and close their own files (the cas
    // stager, checksum packs), on private fd tables (stage_pool.h); io_pool: parallel preads
    // of a descriptor the caller opened (a streamed checksum), on the shared table.  One of
    // each per context, grown to the largest thread count any call asked for; a caller holds
    // its shared_ptr while it runs, so a concurrent call that grows a pool never destroys
    // one in use.
    std::shared_ptr<StagePool> pool, iopool;
    std::shared_ptr<StagePool> stage_pool(int nthreads) {
        std::lock_guard<std::mutex> g(pool_mu);
        if (!pool || pool->threads() < nthreads) pool = std::make_shared<StagePool>(nthreads, true);
        return pool;
    }
    std::shared_ptr<StagePool> io_pool(int nthreads) {
        std::lock_guard<std::mutex> g(pool_mu);
        if (!iopool || iopool->threads() < nthreads) iopool = std::make_shared<StagePool>(nthreads, false);
        return iopool;
    }
    sd_coalescer* coalescer() {
        std::lock_guard<std::mutex> g(coal_mu);
        if (!coal) coal = coalescer_create(this);
        return coal;
    }
    std::vector<std::unique_ptr<sdi::Slot>> free_slots;
    sdi::DeltaWork delta;  // sd_cdc_delta_pack / _apply: one of them runs at a time

    std::unique_ptr<sdi::Slot> acquire() {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!free_slots.empty()) {
                auto s = std::move(free_slots.back());
                free_slots.pop_back();
                return s;
            }
        }
        auto s = std::make_unique<sdi::Slot>();
        HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        return s;
    }
    void release(std::unique_ptr<sdi::Slot> s) {
        std::lock_guard<std::mutex> g(mu);
        free_slots.push_back(std::move(s));
    }
    void bind() { HIP_CHECK(hipSetDevice(device)); }
    static hipStream_t pick(void* s) { return reinterpret_cast<hipStream_t>(s); }  // NULL = null stream
};

namespace sdi {

// Two slots held for one call; released (after their streams drain) on scope exit.
struct SlotPair {
    sd_cas_ctx* c;
    std::unique_ptr<Slot> s[2];
    std::unique_ptr<Slot> cp;  // a third queue, for H2D copies issued back to back (copy_stream)
    explicit SlotPair(sd_cas_ctx* ctx) : c(ctx) {
        s[0] = c->acquire();
        s[1] = c->acquire();
    }
    ~SlotPair() {
        for (auto* x : {&s[0], &s[1], &cp})
            if (*x) {
                (void)hipStreamSynchronize((*x)->stream);
                c->release(std::move(*x));
            }
    }
    // One stream for all of a call's host-to-device copies: they run one after the other on
    // one DMA queue (two copies in flight on two streams measured 46 instead of 56 GB/s on
    // some boxes), while the kernels of the two slots overlap them.
    hipStream_t copy_stream() {
        if (!cp) cp = c->acquire();
        return cp->stream;
    }
    Slot& operator[](int k) { return *s[k]; }
    void sync_all() {
        s[0]->sync();
        s[1]->sync();
    }
};

}  // namespace sdi

namespace sdi {
// checksum batches (device): (re)plan reusing the batch's buffers; the reduce passes; leaf + reduce
void plan_checksum_batch(sd_checksum_batch* b, const uint64_t* offsets, const uint64_t* lens, size_t n,
                         hipStream_t stream);
void run_checksum_reduce(const sd_checksum_batch* b, uint32_t* out, hipStream_t s);
void run_checksum_batch(const sd_checksum_batch* b, const uint8_t* d_data, uint8_t* d_hash32, hipStream_t s);
// cas batches (device)
void plan_cas_batch(sd_cas_batch* b, const sd_extent* ext, size_t n, hipStream_t stream);
void run_cas_batch(const sd_cas_batch* b, const uint8_t* d_staged, uint8_t* d_hash32, hipStream_t s,
                   int parts = SD_PART_SAMPLED | SD_PART_WHOLE);
// fingerprint batches (device, sd_fingerprint.cpp): gather -> d_staged; gather + cas + checksum
void plan_fingerprint_batch(sd_fingerprint_batch* b, const uint64_t* offsets, const uint64_t* lens, size_t n,
                            hipStream_t stream);
void run_fingerprint_gather(const sd_fingerprint_batch* b, const uint8_t* d_data, uint8_t* d_staged, hipStream_t s);
void run_fingerprint_batch(const sd_fingerprint_batch* b, const uint8_t* d_data, uint8_t* d_cas_hash32,
                           uint8_t* d_checksum32, hipStream_t s);
}  // namespace sdi
