// dedup.hip -- post-hash duplicate grouping (the cas_id -> Object link step).
//
// Reference semantics: identifier_job_step links each file_path to an Object owning an
// equal cas_id and otherwise creates one (core/src/object/file_identifier/mod.rs:136-333);
// size-0 files never take part (:80-88).  Here, per SURVEY.md §8(e): records
// (cas_id as a big-endian u64 of the first 8 hash bytes = the 16-hex string's order,
// global file index) are bucketed by the top bits of the cas_id for an all-to-all
// exchange across ranks, then each rank sorts its bucket and maps every record to the
// smallest file index of its equal-cas_id group (the Object-link candidate).
#include <hip/hip_runtime.h>

#include <algorithm>

#include <cstring>
#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "sd_internal.h"

namespace {

__device__ __forceinline__ uint64_t cas_key(const uint8_t* h) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(h);
    // bytes h[0..7] as a big-endian number == lexicographic order of the hex cas_id
    return ((uint64_t)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
}

__device__ __forceinline__ uint32_t dest_of(uint64_t key, int nparts) {
    return (uint32_t)(((key >> 48) * (uint64_t)nparts) >> 16);  // top 16 bits scaled: contiguous ranges
}

// Deterministic, contention-free partition in two passes over a fixed grid of PART_BLOCKS
// workgroups, each owning one contiguous slice of the input:
//   count:   per (destination, block) histogram, wave-aggregated into LDS;
//   scan:    one workgroup turns the histogram into destination-major offsets;
//   scatter: each block walks its slice again in order; a record's position is its
//            block's offset for its destination + its rank among earlier records of the
//            same destination (ballot/popcount inside a wave, LDS counts across waves).
// Output is stable: grouped by destination, in input order within a destination.
constexpr uint32_t PART_BLOCKS = 1024;
constexpr uint32_t PART_MAXD = 64;

struct slice_t { uint64_t lo, hi; };
__device__ __forceinline__ slice_t slice_of(uint64_t n, uint32_t b) {
    const uint64_t per = (n + PART_BLOCKS - 1) / PART_BLOCKS;
    uint64_t lo = (uint64_t)b * per, hi = lo + per;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
    return {lo, hi};
}

// rank of this lane among active lanes with the same destination, and that group's size
__device__ __forceinline__ void wave_match(bool active, uint32_t d, uint32_t& rank, uint32_t& size, bool& leader) {
    const uint32_t lane = threadIdx.x & 63;
    uint64_t remaining = __ballot(active);
    rank = 0; size = 0; leader = false;
    while (remaining) {
        const uint32_t first = __builtin_ctzll(remaining);
        const uint32_t dl = __shfl(d, first);
        const uint64_t m = __ballot(active && d == dl);
        if (active && d == dl) {
            rank = __popcll(m & ((1ull << lane) - 1));
            size = __popcll(m);
            leader = lane == first;
        }
        remaining &= ~m;
    }
}

__global__ __launch_bounds__(256) void k_part_count(const uint8_t* __restrict__ hash32,
                                                    const uint8_t* __restrict__ valid, uint64_t n, int nparts,
                                                    uint32_t* __restrict__ hist) {
    __shared__ uint32_t local[PART_MAXD];
    if (threadIdx.x < PART_MAXD) local[threadIdx.x] = 0;
    __syncthreads();
    const slice_t sl = slice_of(n, blockIdx.x);
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi && (!valid || valid[i]);
        const uint32_t d = act ? dest_of(cas_key(hash32 + i * 32), nparts) : 0;
        uint32_t rank, size;
        bool leader;
        wave_match(act, d, rank, size, leader);
        if (leader) atomicAdd(&local[d], size);
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nparts) hist[threadIdx.x * PART_BLOCKS + blockIdx.x] = local[threadIdx.x];
}

// exclusive scan of hist[nparts * PART_BLOCKS] (destination-major) -> offs; counts[d].
// One workgroup of PART_SCAN_LANES, each lane owning PART_BLOCKS / PART_SCAN_LANES adjacent
// blocks of a destination: one wave per SIMD, so the workgroup starts wherever a CU has one
// free wave slot per SIMD (a 1024-lane workgroup needs four, which beside the hash kernels
// only a kernel's drain tail offers).  With `row` it also completes the exchange row behind
// the counts -- index base, file count, capacity, valid records (~0: row.bad_index) -- so no
// copy has to follow it on the stream.
constexpr uint32_t PART_SCAN_LANES = 256;
constexpr uint32_t PART_SCAN_PER = PART_BLOCKS / PART_SCAN_LANES;
static_assert(PART_SCAN_PER == 4, "k_part_scan loads a lane's blocks as one uint4");

__global__ __launch_bounds__(PART_SCAN_LANES) void k_part_scan(const uint32_t* __restrict__ hist, int nparts,
                                                               uint64_t* __restrict__ offs,
                                                               unsigned long long* __restrict__ counts,
                                                               unsigned long long* __restrict__ total,
                                                               bool with_row, sdk::part_row row) {
    constexpr uint32_t NW = PART_SCAN_LANES / 64;
    __shared__ uint64_t wsum[2][NW];  // alternating per destination: one barrier each
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint64_t carry = 0;  // records of the destinations before d (the same in every lane)
    for (int d = 0; d < nparts; d++) {
        const uint4 v = reinterpret_cast<const uint4*>(hist + (size_t)d * PART_BLOCKS)[t];
        const uint64_t mine = (uint64_t)v.x + v.y + v.z + v.w;
        uint64_t x = mine;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_up(x, o);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63) wsum[d & 1][w] = x;
        __syncthreads();
        uint64_t before = carry, all = 0;
        for (uint32_t k = 0; k < NW; k++) {
            if (k < w) before += wsum[d & 1][k];
            all += wsum[d & 1][k];
        }
        uint64_t* o4 = offs + (size_t)d * PART_BLOCKS + PART_SCAN_PER * t;
        uint64_t at = before + x - mine;
        o4[0] = at;
        o4[1] = at += v.x;
        o4[2] = at += v.y;
        o4[3] = at += v.z;
        if (t == 0) counts[d] = all;
        carry += all;
    }
    if (t == 0) {
        *total = carry;
        if (with_row) {
            counts[nparts] = row.base;
            counts[nparts + 1] = row.n;
            counts[nparts + 2] = row.capacity;
            counts[nparts + 3] = row.bad_index ? ~0ull : carry;
        }
    }
}

__global__ __launch_bounds__(256) void k_part_scatter(const uint8_t* __restrict__ hash32,
                                                      const uint8_t* __restrict__ valid, uint64_t n, uint64_t base_idx,
                                                      int nparts, const uint64_t* __restrict__ offs,
                                                      uint64_t* __restrict__ records) {
    __shared__ uint64_t run[PART_MAXD];
    __shared__ uint32_t wcnt[4][PART_MAXD];
    const uint32_t w = threadIdx.x >> 6;
    if (threadIdx.x < (unsigned)nparts) run[threadIdx.x] = offs[threadIdx.x * PART_BLOCKS + blockIdx.x];
    for (uint32_t k = threadIdx.x; k < 4 * PART_MAXD; k += blockDim.x) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    const slice_t sl = slice_of(n, blockIdx.x);
    for (uint64_t base = sl.lo; base < sl.hi; base += blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        const bool act = i < sl.hi && (!valid || valid[i]);
        const uint64_t key = act ? cas_key(hash32 + i * 32) : 0;
        const uint32_t d = act ? dest_of(key, nparts) : 0;
        uint32_t rank, size;
        bool leader;
        wave_match(act, d, rank, size, leader);
        if (leader) wcnt[w][d] = size;
        __syncthreads();
        if (act) {
            uint64_t pos = run[d] + rank;
            for (uint32_t k = 0; k < w; k++) pos += wcnt[k][d];
            records[2 * pos] = key;
            records[2 * pos + 1] = base_idx + i;
        }
        __syncthreads();
        if (threadIdx.x < (unsigned)nparts)
            run[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 4 * PART_MAXD; k += blockDim.x) (&wcnt[0][0])[k] = 0;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_split(const uint64_t* __restrict__ rec, uint64_t m, uint64_t* __restrict__ keys,
                                               uint64_t* __restrict__ idx) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        keys[i] = rec[2 * i];
        idx[i] = rec[2 * i + 1];
    }
}

// after the (idx, then stable key) sorts: head positions, then max-scan -> group head
__global__ __launch_bounds__(256) void k_heads(const uint64_t* __restrict__ keys, uint64_t m,
                                               uint64_t* __restrict__ headpos, uint64_t* __restrict__ nheads) {
    __shared__ unsigned long long cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const bool head = i == 0 || keys[i] != keys[i - 1];
        headpos[i] = head ? i : 0;
        mine += head;
    }
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(nheads), cnt);
}

__global__ __launch_bounds__(256) void k_join(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ idx,
                                              const uint64_t* __restrict__ headscan, uint64_t m,
                                              uint64_t* __restrict__ rec, uint64_t* __restrict__ rep) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        rec[2 * i] = keys[i];
        rec[2 * i + 1] = idx[i];
        rep[i] = idx[headscan[i]];
    }
}

uint32_t grid_for(uint64_t n) {
    uint64_t g = (n + 255) / 256;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (uint32_t)g;
}

// ------------------------------------------------- bucket grouping (dedup_variant 1)
// cas_ids are uniform hash bits, so an order-preserving split of the key range into
// nb = 2^lg buckets -- (key - kmin) >> shift -- leaves ~m/nb (24-48) records per bucket,
// and equal keys share a bucket, so every group lies inside one.  The records are bucketed
// by a radix sort of the lg-bit bucket numbers alone (2-3 passes of u32 pairs instead of
// 8 passes of u64 pairs).  Each bucket is then sorted by (key, index) with a bitonic
// network and a max-scan of head positions gives every record its group head, whose
// index is the group minimum (the representative):
//   s <= 64        one wave, one record per lane, in registers (lane shuffles);
//   s <= GB_CAP    one wave, in LDS;
//   s <= GB_BIG_CAP  one 1024-lane workgroup (k_gb_sort_big; a large duplicate group);
//   larger         copied through unsorted, flagging `overflow`: the caller then runs the
//                  radix path over the permuted records.
// No global atomics on the data path (only the rare big-bucket listing): partial results
// go to per-workgroup slots reduced by one small workgroup.
constexpr uint32_t GB_CAP = 128;   // wave LDS path for 64 < s <= 128; larger buckets go to k_gb_sort_big
constexpr uint32_t GB_WAVES = 4;  // buckets per workgroup, one per wave
constexpr uint32_t GB_MM_BLOCKS = 512;
constexpr uint32_t GB_BIG_CAP = 4096;   // 64 KiB of LDS
constexpr uint32_t GB_BIG_GRID = 128;   // workgroups of k_gb_sort_big (each loops over the list)

struct gb_state {
    unsigned long long ngroups, overflow, kmin, kmax, shift, nbig;
};

// per-workgroup key minimum / maximum -> part[2 * blockIdx.x + {0, 1}]
__global__ __launch_bounds__(256) void k_gb_minmax(const uint64_t* __restrict__ rec, uint64_t m,
                                                   uint64_t* __restrict__ part) {
    __shared__ uint64_t slo[4], shi[4];
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = rec[2 * i];
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { slo[w] = lo; shi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < blockDim.x / 64; k++) {
            lo = slo[k] < lo ? slo[k] : lo;
            hi = shi[k] > hi ? shi[k] : hi;
        }
        part[2 * blockIdx.x] = lo;
        part[2 * blockIdx.x + 1] = hi;
    }
}

// one workgroup of 64: reduce the partials, fix the bucket shift, clear the counters
__global__ __launch_bounds__(64) void k_gb_final(const uint64_t* __restrict__ part, uint32_t np, uint32_t lg,
                                                 gb_state* st) {
    uint64_t lo = ~0ull, hi = 0;
    for (uint32_t i = threadIdx.x; i < np; i += 64) {
        lo = part[2 * i] < lo ? part[2 * i] : lo;
        hi = part[2 * i + 1] > hi ? part[2 * i + 1] : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if (threadIdx.x == 0) {
        const uint64_t span = hi - lo;
        const uint32_t bits = span ? 64u - (uint32_t)__builtin_clzll(span) : 0u;
        st->kmin = lo;
        st->kmax = hi;
        st->shift = bits > lg ? bits - lg : 0u;  // lg >= 1, so shift <= 63
        st->ngroups = 0;
        st->overflow = 0;
        st->nbig = 0;
    }
}

// a copy of the records (the output overwrites them) + the bucket number of each and its position
__global__ __launch_bounds__(256) void k_gb_split(const uint4* __restrict__ rec, uint64_t m, const gb_state* st,
                                                  uint4* __restrict__ copy, uint32_t* __restrict__ bk,
                                                  uint32_t* __restrict__ pos) {
    const uint64_t kmin = st->kmin;
    const uint32_t sh = (uint32_t)st->shift;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 r = rec[i];
        copy[i] = r;
        bk[i] = (uint32_t)(((((uint64_t)r.y << 32) | r.x) - kmin) >> sh);
        pos[i] = (uint32_t)i;
    }
}

// bucket b occupies sorted slots [offs[b], offs[b + 1]) (offs[nb] = m)
__global__ __launch_bounds__(256) void k_gb_bounds(const uint32_t* __restrict__ bk, uint64_t m, uint32_t nb,
                                                   uint32_t* __restrict__ offs) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t cur = bk[i];
        const uint32_t first = i == 0 ? 0u : bk[i - 1] + 1u;
        for (uint32_t b = first; b <= cur; b++) offs[b] = (uint32_t)i;
        if (i + 1 == m)
            for (uint32_t b = cur + 1; b <= nb; b++) offs[b] = (uint32_t)m;
    }
}

__device__ __forceinline__ uint64_t lo64(const uint4& v) { return ((uint64_t)v.y << 32) | v.x; }
__device__ __forceinline__ uint64_t hi64(const uint4& v) { return ((uint64_t)v.w << 32) | v.z; }

__device__ __forceinline__ bool rec_gt(const uint4& a, const uint4& b) {  // (key, index) order
    const uint64_t ka = lo64(a), kb = lo64(b);
    return ka > kb || (ka == kb && hi64(a) > hi64(b));
}

__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave per bucket: its s records are padded to P = 2^k >= s with (~0, ~0) and
// bitonic-sorted by (key, index) in LDS -- O(P log^2 P), so a bucket holding a large
// duplicate group costs ~45 stages rather than the s^2 of a rank sort.  Then, in chunks
// of 64 sorted records, a wave max-scan of head positions (a head is the first record
// of its key) gives each record its group head, whose index is the group minimum (the
// representative).  Head counts -> heads[blockIdx.x].
__global__ __launch_bounds__(64 * GB_WAVES) void k_gb_sort(const uint4* __restrict__ copy,
                                                           const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ offs, uint32_t nb,
                                                           uint4* __restrict__ rec, uint64_t* __restrict__ rep,
                                                           uint32_t* __restrict__ heads, uint32_t* __restrict__ big,
                                                           gb_state* st) {
    __shared__ uint4 sr[GB_WAVES][GB_CAP];  // (key, index) per record
    __shared__ uint32_t wh[GB_WAVES];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t b = blockIdx.x * GB_WAVES + w;
    uint32_t h = 0;
    if (b < nb) {
        const uint32_t lo = offs[b], s = offs[b + 1] - lo;
        if (s > GB_CAP) {  // k_gb_sort_big takes it
            if (lane == 0) big[atomicAdd(&st->nbig, 1ull)] = b;
        } else if (s > 0 && s <= 64) {
            // the common case (mean ~38): one record per lane, a bitonic network over
            // lane shuffles, then head / representative by shuffles -- no LDS at all
            uint32_t P = 1;
            while (P < s) P <<= 1;
            const bool act = lane < s;
            uint64_t k = ~0ull, id = ~0ull;
            if (act) {
                const uint4 r = copy[pos[lo + lane]];
                k = lo64(r);
                id = hi64(r);
            }
            for (uint32_t kk = 2; kk <= P; kk <<= 1) {
                for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                    const uint64_t ok = __shfl_xor(k, (int)j), oid = __shfl_xor(id, (int)j);
                    const bool other_less = ok < k || (ok == k && oid < id);
                    const bool me_less = k < ok || (k == ok && id < oid);
                    const bool want_min = ((lane & j) == 0) == ((lane & kk) == 0);
                    if (want_min ? other_less : me_less) {
                        k = ok;
                        id = oid;
                    }
                }
            }
            const uint64_t pk = __shfl_up(k, 1);
            const bool head = act && (lane == 0 || pk != k);
            uint32_t hp = head ? lane : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(hp, o);
                if (lane >= (uint32_t)o) hp = y > hp ? y : hp;
            }
            const uint64_t r = __shfl(id, (int)hp);
            if (act) {
                rec[lo + lane] = make_uint4((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)id, (uint32_t)(id >> 32));
                rep[lo + lane] = r;
            }
            h += head;
        } else if (s > 0) {
            uint4* r_ = sr[w];
            uint32_t P = 1;
            while (P < s) P <<= 1;
            for (uint32_t e = lane; e < P; e += 64)
                r_[e] = e < s ? copy[pos[lo + e]] : make_uint4(~0u, ~0u, ~0u, ~0u);
            wave_lds_fence();
            for (uint32_t k = 2; k <= P; k <<= 1) {
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    // a lane's (up to 4) pairs of a stage are disjoint: load them all, then
                    // compare and store, so one LDS latency covers the stage
                    constexpr uint32_t Q = GB_CAP / 128;
                    uint4 x[Q], y[Q];
#pragma unroll
                    for (uint32_t q = 0; q < Q; q++) {
                        const uint32_t t = lane + 64 * q;
                        if (t < (P >> 1)) {
                            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                            x[q] = r_[i];
                            y[q] = r_[i + j];
                        }
                    }
#pragma unroll
                    for (uint32_t q = 0; q < Q; q++) {
                        const uint32_t t = lane + 64 * q;
                        if (t < (P >> 1)) {
                            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                            if (rec_gt(x[q], y[q]) == ((i & k) == 0)) {
                                r_[i] = y[q];
                                r_[i + j] = x[q];
                            }
                        }
                    }
                    wave_lds_fence();
                }
            }
            uint32_t carry = 0;  // head position of the record before this chunk
            for (uint32_t c = 0; c < s; c += 64) {
                const uint32_t p = c + lane;
                const bool act = p < s;
                const uint4 me = r_[act ? p : 0];
                const bool head = act && (p == 0 || lo64(r_[p - 1]) != lo64(me));
                uint32_t hp = head ? p : carry;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(hp, o);
                    if (lane >= (uint32_t)o) hp = y > hp ? y : hp;
                }
                if (act) {
                    rec[lo + p] = me;
                    rep[lo + p] = hi64(r_[hp]);
                }
                h += head;
                carry = __shfl(hp, 63);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if (lane == 0) wh[w] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t k = 0; k < GB_WAVES; k++) t += wh[k];
        heads[blockIdx.x] = t;
    }
}

// Buckets of GB_CAP < s <= GB_BIG_CAP records (a duplicate group of hundreds to thousands
// of files): one 1024-lane workgroup per listed bucket, the same bitonic sort and head
// max-scan with workgroup barriers.  Larger buckets are copied through unsorted and flag
// `overflow`.  Head counts -> heads[blockIdx.x] (every workgroup writes its slot).
__global__ __launch_bounds__(1024) void k_gb_sort_big(const uint4* __restrict__ copy, const uint32_t* __restrict__ pos,
                                                      const uint32_t* __restrict__ offs,
                                                      const uint32_t* __restrict__ big, uint4* __restrict__ rec,
                                                      uint64_t* __restrict__ rep, uint32_t* __restrict__ heads,
                                                      gb_state* st) {
    __shared__ uint4 sr[GB_BIG_CAP];
    __shared__ uint32_t wmax[16], carry_s;
    __shared__ uint32_t wh[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t nbig = (uint32_t)st->nbig;
    uint32_t h = 0;
    for (uint32_t q = blockIdx.x; q < nbig; q += gridDim.x) {
        const uint32_t b = big[q];
        const uint32_t lo = offs[b], s = offs[b + 1] - lo;
        if (s > GB_BIG_CAP) {  // copied through unsorted; the caller re-sorts everything
            for (uint32_t e = t; e < s; e += 1024) rec[lo + e] = copy[pos[lo + e]];
            if (t == 0) st->overflow = 1;
            continue;
        }
        uint32_t P = 1;
        while (P < s) P <<= 1;
        for (uint32_t e = t; e < P; e += 1024) sr[e] = e < s ? copy[pos[lo + e]] : make_uint4(~0u, ~0u, ~0u, ~0u);
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                constexpr uint32_t Q = GB_BIG_CAP / 2048;
                uint4 x[Q], y[Q];
#pragma unroll
                for (uint32_t r = 0; r < Q; r++) {
                    const uint32_t u = t + 1024 * r;
                    if (u < (P >> 1)) {
                        const uint32_t i = ((u & ~(j - 1)) << 1) | (u & (j - 1));
                        x[r] = sr[i];
                        y[r] = sr[i + j];
                    }
                }
#pragma unroll
                for (uint32_t r = 0; r < Q; r++) {
                    const uint32_t u = t + 1024 * r;
                    if (u < (P >> 1)) {
                        const uint32_t i = ((u & ~(j - 1)) << 1) | (u & (j - 1));
                        if (rec_gt(x[r], y[r]) == ((i & k) == 0)) {
                            sr[i] = y[r];
                            sr[i + j] = x[r];
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (t == 0) carry_s = 0;
        __syncthreads();
        for (uint32_t c = 0; c < s; c += 1024) {
            const uint32_t p = c + t;
            const bool act = p < s;
            const uint4 me = sr[act ? p : 0];
            const bool head = act && (p == 0 || lo64(sr[p - 1]) != lo64(me));
            uint32_t hp = head ? p : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(hp, o);
                if (lane >= (uint32_t)o) hp = y > hp ? y : hp;
            }
            if (lane == 63) wmax[w] = hp;
            __syncthreads();
            uint32_t before = carry_s;
            for (uint32_t k = 0; k < w; k++) before = wmax[k] > before ? wmax[k] : before;
            hp = before > hp ? before : hp;
            if (act) {
                rec[lo + p] = me;
                rep[lo + p] = hi64(sr[hp]);
            }
            h += head;
            __syncthreads();
            if (t == 1023) carry_s = hp;
            __syncthreads();
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
    if (lane == 0) wh[w] = h;
    __syncthreads();
    if (t == 0) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 16; k++) v += wh[k];
        heads[blockIdx.x] = v;
    }
}

// one workgroup of 1024: group count = sum of the per-workgroup head counts
__global__ __launch_bounds__(1024) void k_gb_sum(const uint32_t* __restrict__ heads, uint32_t n, gb_state* st) {
    __shared__ unsigned long long ws[16];
    unsigned long long v = 0;
    for (uint32_t i = threadIdx.x; i < n; i += 1024) v += heads[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < 16; k++) t += ws[k];
        st->ngroups = t;
    }
}

// Object owner per record under the reference's chunk-of-100 rule (file_identifier/
// mod.rs:136-333; spacedrive_amd/identifier.py): a file links to its group's first Object
// when that was created in an earlier identifier step, else it creates its own.
__global__ __launch_bounds__(256) void k_owners(const uint64_t* __restrict__ rec, uint64_t m,
                                                const uint64_t* __restrict__ rep, uint64_t chunk,
                                                uint64_t* __restrict__ owner) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t idx = rec[2 * i + 1], r = rep[i];
        owner[i] = idx / chunk == r / chunk ? idx : r;
    }
}

}  // namespace

namespace sdk {

hipError_t dedup_partition(const uint8_t* hash32, const uint8_t* valid, uint64_t n, uint64_t base, int nparts,
                           uint64_t* counts, uint64_t* records, uint64_t* scratch, hipStream_t s,
                           const part_row* row) {
    // scratch: hist (u32 nparts x PART_BLOCKS), offs (u64 nparts x PART_BLOCKS), total (u64)
    uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
    uint64_t* offs = scratch + (size_t)nparts * PART_BLOCKS / 2 + 1;
    auto* total = reinterpret_cast<unsigned long long*>(offs + (size_t)nparts * PART_BLOCKS);
    hipLaunchKernelGGL(k_part_count, dim3(PART_BLOCKS), dim3(256), 0, s, hash32, valid, n, nparts, hist);
    hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(PART_SCAN_LANES), 0, s, hist, nparts, offs,
                       reinterpret_cast<unsigned long long*>(counts), total, row != nullptr,
                       row ? *row : part_row{});
    hipLaunchKernelGGL(k_part_scatter, dim3(PART_BLOCKS), dim3(256), 0, s, hash32, valid, n, base, nparts, offs,
                       records);
    return hipGetLastError();
}

size_t dedup_partition_scratch(int nparts) {
    return ((size_t)nparts * PART_BLOCKS / 2 + 1 + (size_t)nparts * PART_BLOCKS + 1) * sizeof(uint64_t);
}

// scratch layout: keys[m], idx[m], keys2[m], idx2[m], heads[m], then rocprim temp storage
hipError_t dedup_group(uint64_t* records, uint64_t m, int flags, uint64_t* rep, uint64_t* n_groups_dev,
                       void* scratch, size_t* scratch_bytes, hipStream_t s) {
    size_t sort_bytes = 0, scan_bytes = 0;
    uint64_t* nul = nullptr;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, nul, nul, nul, nul, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    e = rocprim::inclusive_scan(nullptr, scan_bytes, nul, nul, (size_t)m, rocprim::maximum<uint64_t>(), s);
    if (e != hipSuccess) return e;
    const size_t arrays = 5 * m * sizeof(uint64_t);
    size_t temp = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    temp = (temp + 255) & ~size_t(255);
    const size_t need = arrays + temp + 256;
    if (scratch == nullptr) { *scratch_bytes = need; return hipSuccess; }
    if (*scratch_bytes < need) return hipErrorInvalidValue;
    uint64_t* keys = reinterpret_cast<uint64_t*>(scratch);
    uint64_t* idx = keys + m;
    uint64_t* keys2 = idx + m;
    uint64_t* idx2 = keys2 + m;
    uint64_t* heads = idx2 + m;
    void* tmp = reinterpret_cast<void*>(((uintptr_t)(heads + m) + 255) & ~uintptr_t(255));
    e = hipMemsetAsync(n_groups_dev, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || m == 0) return e;
    hipLaunchKernelGGL(k_split, dim3(grid_for(m)), dim3(256), 0, s, records, m, keys, idx);
    size_t tb = temp;
    if (!(flags & SD_DEDUP_INDEX_SORTED)) {
        // sort by index first, so the stable cas_id sort below leaves equal cas_ids in
        // ascending index order
        e = rocprim::radix_sort_pairs(tmp, tb, idx, idx2, keys, keys2, (size_t)m, 0, 64, s);
        if (e != hipSuccess) return e;
        std::swap(keys, keys2);
        std::swap(idx, idx2);
        tb = temp;
    }
    e = rocprim::radix_sort_pairs(tmp, tb, keys, keys2, idx, idx2, (size_t)m, 0, 64, s);
    if (e != hipSuccess) return e;
    // grid-stride over at most 1024 workgroups: one global atomic per workgroup, so the
    // count does not serialise ~m/256 atomics on one L2 line
    hipLaunchKernelGGL(k_heads, dim3(std::min<unsigned>(grid_for(m), 1024u)), dim3(256), 0, s, keys2, m, heads,
                       n_groups_dev);
    tb = temp;
    e = rocprim::inclusive_scan(tmp, tb, heads, keys, (size_t)m, rocprim::maximum<uint64_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_join, dim3(grid_for(m)), dim3(256), 0, s, keys2, idx2, keys, m, records, rep);
    return hipGetLastError();
}

static uint32_t gb_lg(uint64_t m) {  // nb = 2^lg >= m / 48: ~24-48 records per bucket; lg >= 1
    uint32_t lg = 1;                  // keeps the bucket shift (bit length of the span - lg) < 64
    while (lg < 24 && ((uint64_t)48 << lg) < m) lg++;
    return lg;
}

static size_t gb_sort_bytes(uint64_t m, uint32_t lg, hipStream_t s) {
    size_t b = 0;
    uint32_t* nul = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, b, nul, nul, nul, nul, (size_t)m, 0, lg, s) != hipSuccess) return 0;
    return (b + 255) & ~size_t(255);
}

// scratch: copy[m] (16-B records), bk, bk2, pos, pos2 [m] (u32), offs[nb + 1],
// heads[n_wg + GB_BIG_GRID], big[m / (GB_CAP + 1) + 1], minmax partials, then the radix
// sort's temporary storage
static uint64_t gb_big_slots(uint64_t m) { return m / (GB_CAP + 1) + 1; }
static size_t gb_layout_bytes(uint64_t m, uint32_t nb) {
    size_t b = 2 * m * sizeof(uint64_t) + 4 * m * sizeof(uint32_t) +
               (nb + 1 + nb / GB_WAVES + 1 + GB_BIG_GRID + gb_big_slots(m)) * sizeof(uint32_t);
    b = (b + 15) & ~size_t(15);
    b += 2 * GB_MM_BLOCKS * sizeof(uint64_t);
    return (b + 255) & ~size_t(255);
}

size_t dedup_group_buckets_scratch(uint64_t m) {
    const uint32_t lg = gb_lg(m);
    return gb_layout_bytes(m, 1u << lg) + gb_sort_bytes(m, lg, nullptr) + 256;
}

// state: 6 u64 (ngroups, overflow, kmin, kmax, shift, nbig); 0 < m < 2^31
hipError_t dedup_group_buckets(uint64_t* records, uint64_t m, uint64_t* rep, uint64_t* state, void* scratch,
                               size_t scratch_bytes, hipStream_t s) {
    if (m == 0 || m >= (1ull << 31) || scratch_bytes < dedup_group_buckets_scratch(m)) return hipErrorInvalidValue;
    const uint32_t lg = gb_lg(m), nb = 1u << lg, n_wg = (nb + GB_WAVES - 1) / GB_WAVES;
    auto* st = reinterpret_cast<gb_state*>(state);
    uint8_t* base = reinterpret_cast<uint8_t*>(((uintptr_t)scratch + 255) & ~uintptr_t(255));
    uint4* copy = reinterpret_cast<uint4*>(base);
    uint32_t* bk = reinterpret_cast<uint32_t*>(copy + m);
    uint32_t* bk2 = bk + m;
    uint32_t* pos = bk2 + m;
    uint32_t* pos2 = pos + m;
    uint32_t* offs = pos2 + m;  // nb + 1
    uint32_t* heads = offs + nb + 1;  // n_wg + GB_BIG_GRID
    uint32_t* big = heads + n_wg + GB_BIG_GRID;
    uint64_t* part = reinterpret_cast<uint64_t*>(((uintptr_t)(big + gb_big_slots(m)) + 15) & ~uintptr_t(15));
    void* tmp = base + gb_layout_bytes(m, nb);
    size_t tb = gb_sort_bytes(m, lg, s);
    const uint32_t g = std::min<unsigned>(grid_for(m), GB_MM_BLOCKS);
    hipLaunchKernelGGL(k_gb_minmax, dim3(g), dim3(256), 0, s, records, m, part);
    hipLaunchKernelGGL(k_gb_final, dim3(1), dim3(64), 0, s, part, g, lg, st);
    hipLaunchKernelGGL(k_gb_split, dim3(grid_for(m)), dim3(256), 0, s, reinterpret_cast<const uint4*>(records), m, st,
                       copy, bk, pos);
    hipError_t e = rocprim::radix_sort_pairs(tmp, tb, bk, bk2, pos, pos2, (size_t)m, 0, lg, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gb_bounds, dim3(grid_for(m)), dim3(256), 0, s, bk2, m, nb, offs);
    hipLaunchKernelGGL(k_gb_sort, dim3(n_wg), dim3(64 * GB_WAVES), 0, s, copy, pos2, offs, nb,
                       reinterpret_cast<uint4*>(records), rep, heads, big, st);
    hipLaunchKernelGGL(k_gb_sort_big, dim3(GB_BIG_GRID), dim3(1024), 0, s, copy, pos2, offs, big,
                       reinterpret_cast<uint4*>(records), rep, heads + n_wg, st);
    hipLaunchKernelGGL(k_gb_sum, dim3(1), dim3(1024), 0, s, heads, n_wg + GB_BIG_GRID, st);
    return hipGetLastError();
}

hipError_t dedup_owners(const uint64_t* records, uint64_t m, const uint64_t* rep, uint64_t chunk, uint64_t* owner,
                        hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_owners, dim3(grid_for(m)), dim3(256), 0, s, records, m, rep, chunk, owner);
    return hipGetLastError();
}

}  // namespace sdk
