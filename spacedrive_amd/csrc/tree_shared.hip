// tree_shared.hip -- which blocks of a batch of levels are there more than once
// (sd_checksum_tree_shared, include/sd_cas.h "shared blocks").
//
// A full block's node depends on its bytes and its index only (the position rule of the checksum
// trees), so two files hold the same bytes in block j exactly when their level nodes at j are equal.
// No file byte is read and nothing is hashed: the nodes are opaque 32-byte values.
//
//   map      one lane per slot: its file by binary search in the uploaded node_base, its block index
//            j -> keys[s], file[s]
//   classes  sdk::dedup_confirm (dedup_confirm.hip) with key = j, hash = node, every record valid:
//            rep[s] and class_size[s] in slot order, the class totals in its state; the prefix path
//            first and, when it reports a tie, the full-width path
//   files    one lane per slot: shared / redundant / redundant bytes, combined inside the wave over
//            the lanes of one file (slots are in file order), one u64 add per file and wave into the
//            zeroed per-file rows; then one lane per file: nb, and the totals over the files
//   pairs    the redundant slots compacted (sliced.h) into one u64 (f << 32 | file of rep) each,
//            sorted (rocprim), the run heads compacted into hpos, the runs of at least
//            max(1, min_blocks) slots flagged and written in order.  A run's blocks = the distance
//            to the next head; its bytes = blocks * B less the deficit of f's last block when that
//            block is partial, redundant and held by g -- every other slot of a run is a full block
// Integer adds only: the results do not depend on the order of the atomics.
//
// sd_cdc_shared (include/sd_cas.h, "content-defined chunks") is the same report over a chunk table:
// key = the chunk's length, hash = its id, a slot's bytes = its length (the k_cs_* kernels: the bodies instantiated with
// CDC).  A file can repeat a chunk inside itself, so the records of such slots (f << 32 | f) are
// counted (stats[7]) and their runs never become rows; and a run's bytes are no multiple of a block,
// so the sort carries the slots along and a prefix sum over the sorted slots' lengths gives them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "sd_api_impl.h"
#include "sliced.h"

using namespace sliced;
using namespace sdi;

namespace {

// state (device u64) behind dedup_confirm's DEDUP_CONFIRM_STATE words
constexpr uint32_t TS_RED = 0, TS_HEADS = 1, TS_ROWS = 2, TS_STAT4 = 4;  // [4..7] = stats[4..7]
constexpr uint32_t TS_STATE = 8;

// tab: node_base[0 .. n], then lens[0 .. n); CDC: chunk_base[0 .. n] alone, and the key is the
// chunk's length chunks[2 s + 1]
template <bool CDC>
__device__ __forceinline__ void ts_map_body(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                            const uint64_t* __restrict__ chunks, uint64_t* __restrict__ keys,
                                            uint32_t* __restrict__ file) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < m; s += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;  // node_base[lo] <= s < node_base[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (tab[mid] <= s) lo = mid;
            else hi = mid;
        }
        keys[s] = CDC ? chunks[2 * s + 1] : s - tab[lo];
        file[s] = lo;
    }
}

// files[4 f + {1, 2, 3}] += the shared slots, redundant slots and redundant bytes of file f.  A wave
// holds 64 consecutive slots; the lanes of one file are a run, summed by an inclusive scan and
// added once by the run's first lane.  Every lane of a wave makes the same trips.  CDC: a slot's
// bytes are its key, and st[TS_STAT4 + 3] += the redundant slots whose representative lies in
// their own file (one add per wave).
template <bool CDC>
__device__ __forceinline__ void ts_slots_body(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                              uint32_t block_log2, const uint64_t* __restrict__ keys,
                                              const uint32_t* __restrict__ file, const uint64_t* __restrict__ rep,
                                              const uint64_t* __restrict__ class_size, uint64_t* __restrict__ files,
                                              uint64_t* __restrict__ st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t B = 1ull << block_log2;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b < m; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = b + threadIdx.x;
        uint32_t f = ~0u, cnt = 0;  // cnt: shared in the low half, redundant in the high half (each <= 64)
        uint64_t bytes = 0;
        bool self = false;
        if (s < m) {
            f = file[s];
            const bool red = rep[s] != s;
            cnt = (class_size[s] >= 2 ? 1u : 0u) | (red ? 1u << 16 : 0u);
            if (red && CDC) {
                bytes = keys[s];
                self = file[rep[s]] == f;
            } else if (red) {
                const uint64_t at = keys[s] << block_log2, len = tab[n + 1 + f];
                bytes = len > at ? (len - at < B ? len - at : B) : 0;
            }
        }
        if constexpr (CDC) {
            const uint64_t selfs = __ballot(self);
            if (lane == 0 && selfs)
                atomicAdd(reinterpret_cast<unsigned long long*>(st + TS_STAT4 + 3), (unsigned long long)__popcll(selfs));
        }
        const uint32_t prev = __shfl_up(f, 1);
        const bool head = lane == 0 || prev != f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t c = __shfl_up(cnt, o);
            const uint64_t y = __shfl_up(bytes, o);
            if (lane >= (uint32_t)o) cnt += c, bytes += y;
        }
        const uint64_t heads = __ballot(head);
        const uint64_t later = lane == 63 ? 0 : heads & ~((2ull << lane) - 1);
        const int end = later ? __ffsll((unsigned long long)later) - 2 : 63;  // the run's last lane
        uint32_t c_end = __shfl(cnt, end), c_before = __shfl_up(cnt, 1);
        uint64_t y_end = __shfl(bytes, end), y_before = __shfl_up(bytes, 1);
        if (!head || f == ~0u) continue;
        if (lane != 0) c_end -= c_before, y_end -= y_before;
        unsigned long long* row = reinterpret_cast<unsigned long long*>(files + 4 * (uint64_t)f);
        if (c_end & 0xffff) atomicAdd(row + 1, (unsigned long long)(c_end & 0xffff));
        if (c_end >> 16) atomicAdd(row + 2, (unsigned long long)(c_end >> 16));
        if (y_end) atomicAdd(row + 3, (unsigned long long)y_end);
    }
}

// files[4 f] = nb; st[TS_STAT4 ..] += redundant blocks, redundant bytes, files with a redundant
// block, files every block of which is redundant (CDC: not the last one, k_ts_slots counts that word)
template <bool CDC>
__device__ __forceinline__ void ts_files_body(const uint64_t* __restrict__ tab, uint32_t n,
                                              uint64_t* __restrict__ files, uint64_t* __restrict__ st) {
    uint64_t v[4] = {0, 0, 0, 0};
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t nb = tab[f + 1] - tab[f], red = files[4 * f + 2];
        files[4 * f] = nb;
        v[0] += red;
        v[1] += files[4 * f + 3];
        v[2] += red != 0;
        if (!CDC) v[3] += red == nb;
    }
    block_sum(v);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 4; k++)
        if (v[k]) atomicAdd(reinterpret_cast<unsigned long long*>(st + TS_STAT4 + k), (unsigned long long)v[k]);
}

// the kernels of the two reports: the levels' (k_ts_*) and the chunk table's (k_cs_*)
__global__ __launch_bounds__(256) void k_ts_map(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ file) {
    ts_map_body<false>(tab, n, m, nullptr, keys, file);
}
__global__ __launch_bounds__(256) void k_cs_map(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                                const uint64_t* __restrict__ chunks, uint64_t* __restrict__ keys,
                                                uint32_t* __restrict__ file) {
    ts_map_body<true>(tab, n, m, chunks, keys, file);
}
__global__ __launch_bounds__(256) void k_ts_slots(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                                  uint32_t block_log2, const uint64_t* __restrict__ keys,
                                                  const uint32_t* __restrict__ file, const uint64_t* __restrict__ rep,
                                                  const uint64_t* __restrict__ class_size,
                                                  uint64_t* __restrict__ files) {
    ts_slots_body<false>(tab, n, m, block_log2, keys, file, rep, class_size, files, nullptr);
}
__global__ __launch_bounds__(256) void k_cs_slots(const uint64_t* __restrict__ tab, uint32_t n, uint64_t m,
                                                  const uint64_t* __restrict__ keys, const uint32_t* __restrict__ file,
                                                  const uint64_t* __restrict__ rep, const uint64_t* __restrict__ class_size,
                                                  uint64_t* __restrict__ files, uint64_t* __restrict__ st) {
    ts_slots_body<true>(tab, n, m, 0, keys, file, rep, class_size, files, st);
}
__global__ __launch_bounds__(256) void k_ts_files(const uint64_t* __restrict__ tab, uint32_t n,
                                                  uint64_t* __restrict__ files, uint64_t* __restrict__ st) {
    ts_files_body<false>(tab, n, files, st);
}
__global__ __launch_bounds__(256) void k_cs_files(const uint64_t* __restrict__ tab, uint32_t n,
                                                  uint64_t* __restrict__ files, uint64_t* __restrict__ st) {
    ts_files_body<true>(tab, n, files, st);
}

// the redundant slots ...
struct ts_redundant {
    const uint64_t* __restrict__ rep;
    __device__ bool operator()(uint64_t i, uint64_t) const { return rep[i] != i; }
};
// ... each as (its file << 32 | the file of its representative), in slot order
struct ts_records : from_flags {
    const uint64_t* __restrict__ rep;
    const uint32_t* __restrict__ file;
    uint64_t* __restrict__ rec;
    uint64_t* __restrict__ val;  // CDC: the slot beside its record; else null
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (!flag) return;
        rec[slot] = (uint64_t)file[i] << 32 | file[rep[i]];
        if (val) val[slot] = i;
    }
};
// the first record of every run of the sorted records ...
struct ts_head {
    const uint64_t* __restrict__ rec;
    __device__ bool operator()(uint64_t i, uint64_t) const { return i == 0 || rec[i] != rec[i - 1]; }
};
// ... and its position
struct ts_head_pos : from_flags {
    uint64_t* __restrict__ hpos;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (flag) hpos[slot] = i;
    }
};
// the runs (by head h of n) of at least `need` of the r records; skip_self (CDC): but no run of a
// file with itself
struct ts_long_run {
    const uint64_t* __restrict__ hpos;
    const uint64_t* __restrict__ rec;
    uint64_t r, need;
    bool skip_self;
    __device__ bool operator()(uint64_t h, uint64_t n) const {
        if (skip_self) {
            const uint64_t x = rec[hpos[h]];
            if ((x >> 32) == (x & 0xffffffffull)) return false;
        }
        return (h + 1 < n ? hpos[h + 1] : r) - hpos[h] >= need;
    }
};

// CDC: lens[i] = the length of the slot at position i of the sorted records, lens[r] = 0
__global__ __launch_bounds__(256) void k_cs_lens(const uint64_t* __restrict__ chunks, const uint64_t* __restrict__ val,
                                                 uint64_t r, uint64_t* __restrict__ lens) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= r; i += (uint64_t)gridDim.x * blockDim.x)
        lens[i] = i < r ? chunks[2 * val[i] + 1] : 0;
}

// One row (f, g, blocks, bytes) per flagged run, in order; the row count -> st[TS_ROWS].  Nothing
// is written when rows is null or the rows exceed `capacity`.  The same grid as the flagging pass.
// ps: null, or (CDC) what the rows' bytes come from.
__global__ __launch_bounds__(256) void k_ts_rows(const uint64_t* __restrict__ rec, const uint64_t* __restrict__ hpos,
                                                 const uint8_t* __restrict__ flags, const uint64_t* __restrict__ counts,
                                                 uint64_t r, const uint64_t* __restrict__ tab, uint32_t n,
                                                 uint32_t block_log2, const uint64_t* __restrict__ rep,
                                                 const uint32_t* __restrict__ file, const uint64_t* __restrict__ ps,
                                                 uint64_t* __restrict__ rows, uint64_t capacity,
                                                 uint64_t* __restrict__ st) {
    uint64_t base[1], all[1];
    slice_bases<1, true>(counts, 0, base, all);
    if (blockIdx.x == 0 && threadIdx.x == 0) st[TS_ROWS] = all[0];
    if (!rows || all[0] > capacity) return;
    const uint64_t heads = st[TS_HEADS], B = 1ull << block_log2;
    uint64_t run = base[0];
    const slice sl = slice_of(heads);
    for (uint64_t b = sl.lo; b < sl.hi; b += blockDim.x) {
        const uint64_t h = b + threadIdx.x;
        const bool flag = h < sl.hi && flags[h];
        const uint64_t slot = tile_slot(flag, run);
        if (!flag) continue;
        const uint64_t at = hpos[h], x = rec[at], f = x >> 32, g = x & 0xffffffffull;
        const uint64_t blocks = (h + 1 < heads ? hpos[h + 1] : r) - at;
        uint64_t bytes = blocks << block_log2;
        if (ps) {  // CDC: ps = the exclusive prefix sum of the sorted slots' lengths
            bytes = ps[at + blocks] - ps[at];
        } else {
            // f's last block: partial (an empty file's is 0 bytes), redundant and held by g?
            const uint64_t last = tab[f + 1] - 1, tail = tab[n + 1 + f] - ((last - tab[f]) << block_log2);
            if (tail < B && rep[last] != last && file[rep[last]] == g) bytes -= B - tail;
        }
        rows[4 * slot] = f;
        rows[4 * slot + 1] = g;
        rows[4 * slot + 2] = blocks;
        rows[4 * slot + 3] = bytes;
    }
}

size_t sort_keys_bytes(uint64_t m, hipStream_t s) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (rocprim::radix_sort_keys(nullptr, b, nul, nul, (size_t)m, 0, 64, s) != hipSuccess) return 0;
    return round256(b);
}

// scratch: keys, rep, class_size [m] u64, file [m] u32, files [4 n] u64, then one region that first
// is dedup_confirm's scratch and then the pair passes': rec, rec2, hpos [m] u64, two flags [m] u8,
// counts [3 * BLOCKS] u64, the sort's temporary storage
struct ts_scratch {
    uint64_t *keys, *rep, *class_size, *files, *rec, *rec2, *hpos, *counts;
    uint32_t* file;
    uint8_t *flags, *flags2;
    void *phase, *tmp;
    size_t phase_bytes, tmp_bytes;
    ts_scratch(void* base, uint64_t m, uint64_t n) {
        uintptr_t p = ((uintptr_t)base + 255) & ~uintptr_t(255);
        auto take = [&](size_t b) {
            const uintptr_t q = p;
            p += round256(b);
            return q;
        };
        keys = reinterpret_cast<uint64_t*>(take(8 * m));
        rep = reinterpret_cast<uint64_t*>(take(8 * m));
        class_size = reinterpret_cast<uint64_t*>(take(8 * m));
        file = reinterpret_cast<uint32_t*>(take(4 * m));
        files = reinterpret_cast<uint64_t*>(take(32 * n));
        const uintptr_t ph = p;
        phase = reinterpret_cast<void*>(ph);
        rec = reinterpret_cast<uint64_t*>(take(8 * m));
        rec2 = reinterpret_cast<uint64_t*>(take(8 * m));
        hpos = reinterpret_cast<uint64_t*>(take(8 * m));
        flags = reinterpret_cast<uint8_t*>(take(m));
        flags2 = reinterpret_cast<uint8_t*>(take(m));
        counts = reinterpret_cast<uint64_t*>(take(3 * BLOCKS * sizeof(uint64_t)));
        tmp = reinterpret_cast<void*>(p);
        phase_bytes = std::max((size_t)(p - ph) + sort_keys_bytes(m, nullptr), sdk::dedup_confirm_scratch(m));
        tmp_bytes = phase_bytes - (size_t)(p - ph);
    }
    // from an aligned base; the caller adds 256 for the alignment
    size_t bytes() const { return (size_t)((uintptr_t)phase - (uintptr_t)keys) + phase_bytes; }
};

uint32_t bits_of(uint64_t v) {  // the bits that hold every value below v
    uint32_t b = 1;
    while (b < 64 && (v - 1) >> b) b++;
    return b;
}

// cdc scratch behind ts_scratch: the slots beside the records through the sort, the sorted slots'
// lengths and their prefix sum [m + 1], the pair sort's and the scan's temporary storage
struct cs_scratch {
    uint64_t *val = nullptr, *val2 = nullptr, *lens = nullptr, *ps = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0, total = 0;
    cs_scratch() = default;
    cs_scratch(void* base, uint64_t m) {
        uintptr_t p = (uintptr_t)base;
        auto take = [&](size_t b) {
            const uintptr_t q = p;
            p += round256(b);
            return reinterpret_cast<uint64_t*>(q);
        };
        val = take(8 * m), val2 = take(8 * m), lens = take(8 * (m + 1)), ps = take(8 * (m + 1));
        tmp = reinterpret_cast<void*>(p);
        size_t sb = 0;
        uint64_t* nul = nullptr;
        if (rocprim::exclusive_scan(nullptr, sb, nul, nul, uint64_t(0), (size_t)(m + 1), rocprim::plus<uint64_t>(), nullptr) !=
            hipSuccess)
            sb = 0;
        tmp_bytes = std::max(sort_pairs_bytes(m, nullptr), round256(sb));
        total = (size_t)(p - (uintptr_t)base) + tmp_bytes;
    }
};

// Both reports.  tab: the slots' prefix sum [0 .. n] (then, for the levels, lens); d_chunks: null for
// the levels, else the chunk table (key = length, bytes = length, self-repeats: the header)
int shared_run(sd_cas_ctx* ctx, std::vector<uint64_t>& tab, size_t n, uint32_t block_log2, const uint64_t* d_chunks,
               const uint8_t* d_nodes, uint64_t min_blocks, uint64_t* d_rep, uint64_t* d_class_size,
               uint64_t* d_files_out, uint64_t* d_pairs_out, uint64_t capacity, uint64_t* n_pairs, uint64_t stats[8],
               void* stream) {
    const bool cdc = d_chunks != nullptr;
    const uint64_t m = tab[n];
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    auto slot = ctx->acquire();
    struct Rel {
        sd_cas_ctx* c;
        std::unique_ptr<Slot>* s;
        ~Rel() { c->release(std::move(*s)); }
    } rel{ctx, &slot};
    const size_t ts_bytes = round256(ts_scratch(nullptr, m, n).bytes());
    slot->staged.ensure(256 + ts_bytes + (cdc ? cs_scratch(nullptr, m).total : 0));
    const ts_scratch x(slot->staged.p, m, n);
    const cs_scratch y = cdc ? cs_scratch(reinterpret_cast<uint8_t*>(x.keys) + ts_bytes, m) : cs_scratch();
    constexpr uint32_t NST = sdk::DEDUP_CONFIRM_STATE + TS_STATE;
    slot->hashes.ensure(NST * sizeof(uint64_t));
    slot->host_hashes.ensure(NST * sizeof(uint64_t));
    uint64_t* d_st = slot->hashes.as<uint64_t>();
    uint64_t* d_ts = d_st + sdk::DEDUP_CONFIRM_STATE;
    const uint64_t* st = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    const uint64_t* ts = st + sdk::DEDUP_CONFIRM_STATE;
    slot->aux.begin();
    slot->aux.add(tab);
    slot->aux.upload(s);
    const uint64_t* d_tab = slot->aux.at<uint64_t>(0);
    uint64_t* rep = d_rep ? d_rep : x.rep;
    uint64_t* class_size = d_class_size ? d_class_size : x.class_size;
    uint64_t* files = d_files_out ? d_files_out : x.files;
    const uint32_t n32 = (uint32_t)n;

    if (cdc) hipLaunchKernelGGL(k_cs_map, dim3(flat_grid(m)), dim3(256), 0, s, d_tab, n32, m, d_chunks, x.keys, x.file);
    else hipLaunchKernelGGL(k_ts_map, dim3(flat_grid(m)), dim3(256), 0, s, d_tab, n32, m, x.keys, x.file);
    bool full = tuning_get(SD_TUNE_CONFIRM_FULL_SORT) != 0;
    for (;;) {  // as sd_dedup_confirm: the prefix path, its state read once, the full-width path on a tie
        HIP_CHECK(sdk::dedup_confirm(x.keys, d_nodes, nullptr, m, full, rep, class_size, nullptr, nullptr, 0, d_st,
                                     x.phase, x.phase_bytes, s));
        HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, d_st, sdk::DEDUP_CONFIRM_STATE * sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (full || st[8] == 0) break;
        full = true;
    }
    const uint64_t classes = st[3], classes2 = st[4];
    if (st[0] != m || classes == 0 || classes > m || classes2 > classes)
        throw sd_failure(SD_ERR_INTERNAL, "shared: inconsistent class totals");
    const uint64_t r = m - classes;  // the redundant slots: every class has one slot that is not

    HIP_CHECK(hipMemsetAsync(d_ts, 0, TS_STATE * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(files, 0, 32 * (uint64_t)n, s));
    if (cdc) {
        hipLaunchKernelGGL(k_cs_slots, dim3(flat_grid(m)), dim3(256), 0, s, d_tab, n32, m, x.keys, x.file, rep, class_size,
                           files, d_ts);
        hipLaunchKernelGGL(k_cs_files, dim3(flat_grid(n)), dim3(256), 0, s, d_tab, n32, files, d_ts);
    } else {
        hipLaunchKernelGGL(k_ts_slots, dim3(flat_grid(m)), dim3(256), 0, s, d_tab, n32, m, block_log2, x.keys, x.file, rep,
                           class_size, files);
        hipLaunchKernelGGL(k_ts_files, dim3(flat_grid(n)), dim3(256), 0, s, d_tab, n32, files, d_ts);
    }
    if (r) {
        const uint32_t g_m = sliced_grid(m), g_r = sliced_grid(r);
        launch_flag(g_m, s, ts_redundant{rep}, nullptr, m, x.flags, x.counts);
        launch_compact(g_m, s, ts_records{{x.flags}, rep, x.file, x.rec, cdc ? y.val : nullptr}, nullptr, m, x.counts,
                       d_ts + TS_RED);
        if (cdc) {  // the slots travel with their records; then the prefix sum of their lengths in that order
            size_t tb = y.tmp_bytes;
            HIP_CHECK(rocprim::radix_sort_pairs(y.tmp, tb, x.rec, x.rec2, y.val, y.val2, (size_t)r, 0, 32 + bits_of(n), s));
            hipLaunchKernelGGL(k_cs_lens, dim3(flat_grid(r + 1)), dim3(256), 0, s, d_chunks, y.val2, r, y.lens);
            tb = y.tmp_bytes;
            HIP_CHECK(rocprim::exclusive_scan(y.tmp, tb, y.lens, y.ps, uint64_t(0), (size_t)(r + 1),
                                              rocprim::plus<uint64_t>(), s));
        } else {
            size_t tb = x.tmp_bytes;
            if (sort_keys_bytes(r, s) > tb) throw sd_failure(SD_ERR_INTERNAL, "shared: the sort's storage does not fit");
            HIP_CHECK(rocprim::radix_sort_keys(x.tmp, tb, x.rec, x.rec2, (size_t)r, 0, 32 + bits_of(n), s));
        }
        launch_flag(g_r, s, ts_head{x.rec2}, nullptr, r, x.flags, x.counts + BLOCKS);
        launch_compact(g_r, s, ts_head_pos{{x.flags}, x.hpos}, nullptr, r, x.counts + BLOCKS, d_ts + TS_HEADS);
        launch_flag(g_r, s, ts_long_run{x.hpos, x.rec2, r, std::max<uint64_t>(1, min_blocks), cdc}, d_ts + TS_HEADS, 0,
                    x.flags2, x.counts + 2 * BLOCKS);
        hipLaunchKernelGGL(k_ts_rows, dim3(g_r), dim3(256), 0, s, x.rec2, x.hpos, x.flags2, x.counts + 2 * BLOCKS, r,
                           d_tab, n32, block_log2, rep, x.file, cdc ? y.ps : nullptr, d_pairs_out, capacity, d_ts);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, d_st, NST * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (ts[TS_STAT4] != r || (r && ts[TS_RED] != r) || ts[TS_HEADS] > r || ts[TS_ROWS] > ts[TS_HEADS] ||
        ts[TS_STAT4 + 2] > n || ts[TS_STAT4 + 3] > ts[TS_STAT4 + (cdc ? 0 : 2)])
        throw sd_failure(SD_ERR_INTERNAL, "shared: inconsistent totals");
    if (n_pairs) *n_pairs = ts[TS_ROWS];
    if (stats) {
        stats[0] = n, stats[1] = m, stats[2] = classes, stats[3] = classes2;
        memcpy(stats + 4, ts + TS_STAT4, 4 * sizeof(uint64_t));
    }
    if (d_pairs_out && capacity < ts[TS_ROWS])
        throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of pairs");
    return SD_OK;
}

}  // namespace

int sd_checksum_tree_shared(sd_cas_ctx* ctx, const uint64_t* lens, size_t n, uint32_t block_log2,
                            const uint8_t* d_nodes, uint64_t min_blocks, uint64_t* d_rep, uint64_t* d_class_size,
                            uint64_t* d_files_out, uint64_t* d_pairs_out, uint64_t capacity, uint64_t* n_pairs,
                            uint64_t stats[8], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || (n && !lens)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if ((uint64_t)n >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "too many files");
    std::vector<uint64_t> tab;  // node_base[0 .. n], then lens
    plan_tree_layout(lens, n, block_log2, tab);
    const uint64_t m = tab[n];
    if (m && !d_nodes) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_nodes) % 16) throw sd_failure(SD_ERR_INVALID, "d_nodes not 16-byte aligned");
    if (n_pairs) *n_pairs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0) return SD_OK;
    tab.insert(tab.end(), lens, lens + n);
    return shared_run(ctx, tab, n, block_log2, nullptr, d_nodes, min_blocks, d_rep, d_class_size, d_files_out, d_pairs_out,
                      capacity, n_pairs, stats, stream);
    SD_GUARD_END
}

int sd_cdc_shared(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, const uint64_t* d_chunks, const uint8_t* d_ids,
                  uint64_t min_chunks, uint64_t* d_rep, uint64_t* d_class_size, uint64_t* d_files_out,
                  uint64_t* d_pairs_out, uint64_t capacity, uint64_t* n_pairs, uint64_t stats[8], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx) throw sd_failure(SD_ERR_INVALID, "null argument");
    const uint64_t m = cdc_check_layout(chunk_base, n);
    if (m && (!d_chunks || !d_ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_ids) % 16) throw sd_failure(SD_ERR_INVALID, "d_ids not 16-byte aligned");
    if (n_pairs) *n_pairs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0) return SD_OK;
    std::vector<uint64_t> tab(chunk_base, chunk_base + n + 1);
    return shared_run(ctx, tab, n, 0, d_chunks, d_ids, min_chunks, d_rep, d_class_size, d_files_out, d_pairs_out, capacity,
                      n_pairs, stats, stream);
    SD_GUARD_END
}
