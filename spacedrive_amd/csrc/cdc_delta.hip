// cdc_delta.hip -- the CDC deltas on the device (include/sd_cas.h, "Deltas"): sd_cdc_delta_plan,
// sd_cdc_delta_pack, sd_cdc_delta_apply.
//
//   plan     k_dp_classify: one lane per target slot -- its kind from its representative, the literal
//            lengths for the scan, the statistics and the files' rows (a wave whose 64 slots lie in
//            one file adds once).  rocprim's exclusive scan of the literal lengths gives lit_off.
//            dp_head (sliced.h's flag skeleton) marks the slots that begin a run and writes lit_off;
//            the compact skeleton leaves the heads' positions in order; k_dp_rows writes one row per
//            head, its bytes from the chunk offsets up to the next head or the file's end.  No row
//            is written when the count exceeds the capacity
//   copy     k_seg_copy, the hot path of pack and apply: segments (source address, destination
//            address, bytes) and the flat space of their destination pieces -- the 4 KiB ALIGNED
//            blocks of the address space a segment's destination touches, so that one workgroup's
//            256 lanes are the 256 aligned 16-byte units of a block.  A workgroup takes
//            SEG_WG_PIECES consecutive pieces: the owner of the first by binary search in the
//            pieces' prefix sum, the next by walking on.  A lane whose unit lies inside the
//            segment stores 16 bytes; at the segment's two ends it stores the dwords that lie
//            inside and then single bytes, so every destination byte is written once and no byte
//            outside a segment is written, also where two segments meet inside a unit.  The source
//            is read as aligned 16-byte units (at most the two that hold a byte the lane stores)
//            and realigned in registers by (src - dst) mod 16: two conditional dword moves, then
//            v_alignbyte, as cdc.hip's load_block_shift
//   pack     k_dk_segs: one segment per literal slot, data -> the literal buffer at lit_off
//   apply    k_da_check / k_da_segs validate the recipe without touching the output -- order,
//            sources, ranges without wrap, every file's sum (a scan of the valid runs' bytes gives
//            the destination offsets; that no sum wraps follows run by run from offset + bytes <=
//            the file's length) -- and build the segments beside; the host waits once for the
//            verdict and the piece count, then launches the copy
// Integer adds only in the statistics: they do not depend on the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "sd_api_impl.h"
#include "sliced.h"

using namespace sdi;
using namespace sliced;

namespace {

constexpr uint32_t SEG_PIECE_LOG2 = 12;   // a destination piece: one aligned 4 KiB block, 256 units of 16 bytes
constexpr uint32_t SEG_WG_PIECES = 8;     // consecutive pieces of one workgroup trip
constexpr uint64_t NONE = ~0ull;
static_assert((1u << SEG_PIECE_LOG2) == TILE * 16, "one 16-byte unit per lane");

// plan state (u64)
enum { DP_COPY_CHUNKS, DP_COPY_BYTES, DP_LIT_CHUNKS, DP_LIT_BYTES, DP_REP_CHUNKS, DP_RUNS, DP_BAD, DP_STATE };
// apply state (u64) at the head of the delta scratch
enum { DA_BAD, DA_STATE };

using ull = unsigned long long;

// the last index i in [0, n] with base[i] <= x (base ascends, base[0] <= x); cdc.hip's
__device__ __forceinline__ uint64_t owner_of(const uint64_t* __restrict__ base, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t pieces_of(uint64_t dst, uint64_t bytes) {
    return bytes ? ((dst + bytes - 1) >> SEG_PIECE_LOG2) - (dst >> SEG_PIECE_LOG2) + 1 : 0;
}

// ---------------------------------------------------------------- the plan
struct dp_view {
    const uint64_t* __restrict__ tab;  // chunk_base[0 .. n]
    uint32_t n, n_base;
    uint64_t t0, mt;                   // the first target slot, the target slots
    const uint64_t* __restrict__ chunks;
    const uint64_t* __restrict__ rep;
    const uint64_t* __restrict__ ps;   // [mt + 1]: the exclusive scan of the literal lengths
    // a representative that lies behind its slot is refused by the classify; here it only must not
    // lead outside the tables
    __device__ uint64_t rep_of(uint64_t s) const {
        const uint64_t r = rep[s];
        return r < s ? r : s;
    }
    __device__ void source(uint64_t s, uint64_t& src, uint64_t& off) const {
        const uint64_t r = rep_of(s);
        if (r < t0) src = 1 + owner_of(tab, n_base, r), off = chunks[2 * r];
        else src = 0, off = ps[r - t0];
    }
};

// lens[i] = the length of target slot i if it is a literal, else 0; lens[mt] = 0.  files: 6 x u64
// per target, columns 0 .. 4.  Whole tiles: every lane makes the same trips (the wave adds together)
__global__ __launch_bounds__(256) void k_dp_classify(dp_view v, uint64_t* __restrict__ lens,
                                                     uint64_t* __restrict__ files, uint64_t* __restrict__ st) {
    uint64_t tot[6] = {0, 0, 0, 0, 0, 0};  // DP_COPY_CHUNKS .. DP_REP_CHUNKS, then bad
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x; b <= v.mt; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = b + threadIdx.x;
        const bool act = i < v.mt;
        if (i == v.mt) lens[i] = 0;
        uint64_t row[5] = {0, 0, 0, 0, 0};  // chunks, copied chunks, copied bytes, new literal bytes, repeated bytes
        uint64_t f = 0;
        if (act) {
            const uint64_t s = v.t0 + i, len = v.chunks[2 * s + 1], r = v.rep[s];
            f = owner_of(v.tab, v.n, s);
            row[0] = 1;
            uint64_t lit = 0;
            if (len == 0) {
                tot[DP_LIT_CHUNKS]++;
            } else if (r > s || v.chunks[2 * r + 1] != len || v.rep[r] != r) {
                tot[5]++;
            } else if (r < v.t0) {
                tot[DP_COPY_CHUNKS]++, tot[DP_COPY_BYTES] += len, row[1] = 1, row[2] = len;
            } else if (r == s) {
                tot[DP_LIT_CHUNKS]++, tot[DP_LIT_BYTES] += len, row[3] = len, lit = len;
            } else {
                tot[DP_REP_CHUNKS]++, row[4] = len;
            }
            lens[i] = lit;
        }
        // a wave's first lane is active whenever one of its lanes is
        const uint64_t f0 = __shfl(f, 0);
        if (!act) f = f0;
        if (__ballot(f != f0) == 0) {  // one file: the wave's sums leave through its first lane
#pragma unroll
            for (int k = 0; k < 5; k++) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) row[k] += __shfl_xor(row[k], o);
                if ((threadIdx.x & 63) != 0) row[k] = 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (row[k]) atomicAdd(reinterpret_cast<ull*>(files + 6 * (f - v.n_base) + k), (ull)row[k]);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot[k] += __shfl_xor(tot[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; k++)
            if (tot[k]) atomicAdd(reinterpret_cast<ull*>(st + k), (ull)tot[k]);
        if (tot[5]) atomicAdd(reinterpret_cast<ull*>(st + DP_BAD), (ull)tot[5]);
    }
}

// Does target slot i begin a run?  Side outputs: lit_off[i], and the runs of the slot's file
struct dp_head {
    dp_view v;
    uint64_t* __restrict__ lit_off;
    uint64_t* __restrict__ files;
    __device__ bool operator()(uint64_t i, uint64_t) const {
        const uint64_t s = v.t0 + i, len = v.chunks[2 * s + 1], r = v.rep_of(s);
        if (lit_off) lit_off[i] = (len == 0 || r < v.t0) ? NONE : v.ps[r - v.t0];
        if (len == 0) return false;
        const uint64_t f = owner_of(v.tab, v.n, s);
        bool head = s == v.tab[f];
        if (!head) {
            const uint64_t plen = v.chunks[2 * (s - 1) + 1];
            uint64_t src, off, psrc, poff;
            v.source(s, src, off);
            v.source(s - 1, psrc, poff);
            head = plen == 0 || psrc != src || poff + plen != off;
        }
        if (head) atomicAdd(reinterpret_cast<ull*>(files + 6 * (f - v.n_base) + 5), 1ull);
        return head;
    }
};

struct dp_head_pos : from_flags {
    uint64_t* __restrict__ hpos;
    __device__ void emit(uint64_t i, bool flag, uint64_t slot, uint64_t) const {
        if (flag) hpos[slot] = i;
    }
};

// row j = the run that begins at target slot hpos[j]; nothing unless the st[DP_RUNS] rows fit
__global__ __launch_bounds__(256) void k_dp_rows(dp_view v, const uint64_t* __restrict__ hpos,
                                                 const uint64_t* __restrict__ st, uint64_t* __restrict__ rows,
                                                 uint64_t capacity) {
    const uint64_t R = st[DP_RUNS];
    if (R > capacity) return;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = v.t0 + hpos[j], f = owner_of(v.tab, v.n, s);
        const uint64_t next = j + 1 < R ? v.t0 + hpos[j + 1] : v.t0 + v.mt, last = v.tab[f + 1] - 1;
        const uint64_t end = next <= last ? v.chunks[2 * next] : v.chunks[2 * last] + v.chunks[2 * last + 1];
        uint64_t src, off;
        v.source(s, src, off);
        rows[4 * j] = f - v.n_base;
        rows[4 * j + 1] = src;
        rows[4 * j + 2] = off;
        rows[4 * j + 3] = end - v.chunks[2 * s];
    }
}

// ---------------------------------------------------------------- the segment copy
// segs: 3 x u64 per segment (source address, destination address, bytes); piece_base[0 .. nseg]:
// the exclusive prefix sum of pieces_of.  A segment without a piece is never an owner.
__global__ __launch_bounds__(256) void k_seg_copy(const uint64_t* __restrict__ segs,
                                                  const uint64_t* __restrict__ piece_base, uint64_t nseg) {
    const uint64_t total = piece_base[nseg];
    for (uint64_t p0 = (uint64_t)blockIdx.x * SEG_WG_PIECES; p0 < total; p0 += (uint64_t)gridDim.x * SEG_WG_PIECES) {
        uint64_t c = owner_of(piece_base, nseg, p0);
        const uint64_t p1 = total - p0 < SEG_WG_PIECES ? total : p0 + SEG_WG_PIECES;
        for (uint64_t p = p0; p < p1; p++) {
            while (piece_base[c + 1] <= p) c++;
            const uint64_t src = segs[3 * c], dst = segs[3 * c + 1], bytes = segs[3 * c + 2];
            // this lane's unit [u, u + 16) and what of it the segment holds: [u + fo, u + lo)
            const uint64_t u = (((dst >> SEG_PIECE_LOG2) + (p - piece_base[c])) << SEG_PIECE_LOG2) + 16 * threadIdx.x;
            const uint64_t a = u > dst ? u : dst, e = u + 16 < dst + bytes ? u + 16 : dst + bytes;
            if (a >= e) continue;
            const uint32_t fo = (uint32_t)(a - u), lo = (uint32_t)(e - u);
            const uint64_t sa = u + (src - dst);  // the source address of the unit's first byte
            const uint32_t r = (uint32_t)sa & 15u;
            const uint4* q = reinterpret_cast<const uint4*>(sa & ~15ull);
            // unit 0 holds the unit's bytes [0, 16 - r), unit 1 the rest: only one that holds a stored byte is read
            uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
            if (fo + r < 16) v0 = q[0];
            if (lo - 1 + r >= 16) v1 = q[1];
            uint32_t w[9] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, 0};
            if (r & 4u) {
#pragma unroll
                for (int i = 0; i < 8; i++) w[i] = w[i + 1];
            }
            if (r & 8u) {
#pragma unroll
                for (int i = 0; i < 7; i++) w[i] = w[i + 2];
            }
            uint32_t o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], r & 3u);
            if (fo == 0 && lo == 16) {
                *reinterpret_cast<uint4*>(u) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {  // a segment's head or tail: the dwords inside, then bytes
#pragma unroll
                for (uint32_t d = 0; d < 4; d++) {
                    if (4 * d >= fo && 4 * d + 4 <= lo) {
                        *reinterpret_cast<uint32_t*>(u + 4 * d) = o[d];
                    } else {
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++)
                            if (4 * d + k >= fo && 4 * d + k < lo)
                                *reinterpret_cast<uint8_t*>(u + 4 * d + k) = (uint8_t)(o[d] >> (8 * k));
                    }
                }
            }
        }
    }
}

// the delta scratch for k segments: the apply's state, the segment list, the pieces and their
// prefix sum, the apply's valid bytes and their prefix sum, the scan's temporary storage
struct seg_scratch {
    uint64_t *state, *segs, *pieces, *piece_base, *blen, *ps;
    void* tmp;
    size_t tmp_bytes, total;
    seg_scratch(void* base, uint64_t k) {
        uintptr_t p = (uintptr_t)base;
        auto take = [&](size_t b) {
            const uintptr_t q = p;
            p += round256(b);
            return reinterpret_cast<uint64_t*>(q);
        };
        state = take(8 * DA_STATE), segs = take(24 * k), pieces = take(8 * (k + 1)), piece_base = take(8 * (k + 1));
        blen = take(8 * (k + 1)), ps = take(8 * (k + 1));
        tmp = reinterpret_cast<void*>(p);
        size_t sb = 0;
        uint64_t* nul = nullptr;
        if (rocprim::exclusive_scan(nullptr, sb, nul, nul, uint64_t(0), (size_t)(k + 1), rocprim::plus<uint64_t>(), nullptr) !=
            hipSuccess)
            throw sd_failure(SD_ERR_INTERNAL, "delta: the scan's storage size");
        tmp_bytes = round256(sb);
        total = (size_t)(p - (uintptr_t)base) + tmp_bytes;
    }
};

void scan(const seg_scratch& x, const uint64_t* in, uint64_t* out, uint64_t count, hipStream_t s) {
    size_t tb = x.tmp_bytes;
    HIP_CHECK(rocprim::exclusive_scan(x.tmp, tb, in, out, uint64_t(0), (size_t)count, rocprim::plus<uint64_t>(), s));
}

// as many workgroups as keep every CU's lanes busy; the copy strides over the pieces
uint32_t copy_grid(uint64_t pieces) {
    static const uint32_t most = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return (uint32_t)cus * 8;
    }();
    const uint64_t g = (pieces + SEG_WG_PIECES - 1) / SEG_WG_PIECES;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g, 1), most);
}

// the context's tables through pinned memory: wait for the last upload's end, pack, copy, mark
const uint64_t* upload_tab(sd_cas_ctx* ctx, const std::vector<uint64_t>& tab, hipStream_t s) {
    DeltaWork& w = ctx->delta;
    if (!w.up) HIP_CHECK(hipEventCreateWithFlags(&w.up, hipEventDisableTiming));
    else HIP_CHECK(hipEventSynchronize(w.up));
    w.tab.begin();
    w.tab.add(tab);
    w.tab.upload(s);
    HIP_CHECK(hipEventRecord(w.up, s));
    return w.tab.at<uint64_t>(0);
}

// ---------------------------------------------------------------- pack
// tab: chunk_base[0 .. n], then offsets [n].  One segment per target slot: a literal's bytes from
// the data to the literal buffer, nothing for any other slot; pieces[mt] = 0
__global__ __launch_bounds__(256) void k_dk_segs(const uint64_t* __restrict__ tab, uint32_t n, uint64_t t0, uint64_t mt,
                                                 const uint64_t* __restrict__ chunks, const uint64_t* __restrict__ rep,
                                                 const uint64_t* __restrict__ lit_off, uint64_t data, uint64_t lit,
                                                 uint64_t* __restrict__ segs, uint64_t* __restrict__ pieces) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= mt; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == mt) {
            pieces[i] = 0;
            continue;
        }
        const uint64_t s = t0 + i, len = chunks[2 * s + 1];
        uint64_t src = 0, dst = 0, bytes = 0;
        if (len != 0 && rep[s] == s) {
            const uint64_t f = owner_of(tab, n, s);
            src = data + tab[n + 1 + f] + chunks[2 * s], dst = lit + lit_off[i], bytes = len;
        }
        segs[3 * i] = src, segs[3 * i + 1] = dst, segs[3 * i + 2] = bytes;
        pieces[i] = pieces_of(dst, bytes);
    }
}

// ---------------------------------------------------------------- apply
struct da_view {
    const uint64_t* __restrict__ runs;
    uint64_t R;
    const uint64_t* __restrict__ tab;  // base_offsets, base_lens [nb], out_offsets, out_lens [nt]
    uint32_t nb, nt;
    uint64_t lit_bytes;
    __device__ uint64_t out_off(uint64_t t) const { return tab[2 * (uint64_t)nb + t]; }
    __device__ uint64_t out_len(uint64_t t) const { return tab[2 * (uint64_t)nb + nt + t]; }
    // what a run says of itself and of the run before it: the file, the order, the source, the range
    __device__ bool ok(uint64_t j) const {
        const uint64_t t = runs[4 * j], src = runs[4 * j + 1], off = runs[4 * j + 2], bytes = runs[4 * j + 3];
        if (t >= nt || src > nb) return false;
        if (j && runs[4 * (j - 1)] > t) return false;
        const uint64_t len = src ? tab[nb + src - 1] : lit_bytes;
        return off <= len && bytes <= len - off;  // no sum that could wrap
    }
    // the first run whose file is at least t (the files ascend wherever ok() held)
    __device__ uint64_t first_of(uint64_t t) const {
        uint64_t lo = 0, hi = R;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (runs[4 * mid] < t) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
};

// blen[j] = the run's bytes if ok(j), else 0 with the verdict; blen[R] = 0
__global__ __launch_bounds__(256) void k_da_check(da_view v, uint64_t* __restrict__ blen, uint64_t* __restrict__ st) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= v.R; j += (uint64_t)gridDim.x * blockDim.x) {
        const bool ok = j < v.R && v.ok(j);
        blen[j] = ok ? v.runs[4 * j + 3] : 0;
        if (j < v.R && !ok) atomicAdd(reinterpret_cast<ull*>(st + DA_BAD), 1ull);
    }
}

// ps: the exclusive scan of blen.  A run's destination offset is ps[j] - ps[the file's first run];
// offset + bytes <= the file's length for every run of a file, in order, keeps every such sum
// below 2^64, and the file's last run must end at its length.  A file without a run must be
// empty.  The segments are built beside (nothing for a refused run): they are scratch, the output
// is not touched.
__global__ __launch_bounds__(256) void k_da_segs(da_view v, const uint64_t* __restrict__ ps, uint64_t base, uint64_t lit,
                                                 uint64_t out, uint64_t* __restrict__ segs, uint64_t* __restrict__ pieces,
                                                 uint64_t* __restrict__ st) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    for (uint64_t j = first; j <= v.R; j += stride) {
        if (j == v.R) {
            pieces[j] = 0;
            continue;
        }
        uint64_t src = 0, dst = 0, bytes = 0;
        if (v.ok(j)) {
            const uint64_t t = v.runs[4 * j], s = v.runs[4 * j + 1], off = v.runs[4 * j + 2], b = v.runs[4 * j + 3];
            const uint64_t at = ps[j] - ps[v.first_of(t)], len = v.out_len(t);
            const bool is_last = j + 1 == v.R || v.runs[4 * (j + 1)] != t;
            if (at > len || b > len - at || (is_last && at + b != len)) {
                bad++;
            } else {
                src = (s ? base + v.tab[s - 1] : lit) + off, dst = out + v.out_off(t) + at, bytes = b;
            }
        }
        segs[3 * j] = src, segs[3 * j + 1] = dst, segs[3 * j + 2] = bytes;
        pieces[j] = pieces_of(dst, bytes);
    }
    for (uint64_t t = first; t < v.nt; t += stride) {
        const uint64_t j = v.first_of(t);
        if ((j == v.R || v.runs[4 * j] != t) && v.out_len(t) != 0) bad++;
    }
    if (bad) atomicAdd(reinterpret_cast<ull*>(st + DA_BAD), (ull)bad);
}

struct SlotHold {
    sd_cas_ctx* c;
    std::unique_ptr<Slot> s;
    explicit SlotHold(sd_cas_ctx* ctx) : c(ctx), s(ctx->acquire()) {}
    ~SlotHold() { c->release(std::move(s)); }
    Slot* operator->() const { return s.get(); }
};

}  // namespace

extern "C" int sd_cdc_delta_plan(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, size_t n_base,
                                 const uint64_t* d_chunks, const uint64_t* d_rep, uint64_t* d_lit_off,
                                 uint64_t* d_runs_out, uint64_t capacity, uint64_t* n_runs, uint64_t* d_files_out,
                                 uint64_t stats[8], void* stream) {
    SD_GUARD_BEGIN
    if (!ctx) throw sd_failure(SD_ERR_INVALID, "null argument");
    uint64_t t0 = 0;
    const uint64_t mt = cdc_delta_check_plan(chunk_base, n, n_base, d_chunks, d_rep, &t0);
    if (n_runs) *n_runs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0 || n_base == n) return SD_OK;
    const uint64_t nt = n - n_base;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    SlotHold slot(ctx);
    // the pack's working set over this table: grown here, so the pack allocates nothing
    ctx->delta.scratch.ensure(seg_scratch(nullptr, mt).total);
    ctx->delta.tab.host.ensure((2 * n + 1) * sizeof(uint64_t));
    ctx->delta.tab.dev.ensure((2 * n + 1) * sizeof(uint64_t));
    // scratch: lens, ps [mt + 1], hpos [mt], files [6 nt], counts [BLOCKS] u64, flags [mt] u8, the scan's storage
    size_t sb = 0;
    {
        uint64_t* nul = nullptr;
        if (rocprim::exclusive_scan(nullptr, sb, nul, nul, uint64_t(0), (size_t)(mt + 1), rocprim::plus<uint64_t>(), s) !=
            hipSuccess)
            throw sd_failure(SD_ERR_INTERNAL, "delta: the scan's storage size");
    }
    const size_t b_ps = round256(8 * (mt + 1)), b_m = round256(8 * mt), b_files = round256(48 * nt);
    const size_t b_counts = round256(8 * BLOCKS), b_flags = round256(mt);
    slot->staged.ensure(256 + 2 * b_ps + b_m + b_files + b_counts + b_flags + round256(sb));
    uint8_t* p = reinterpret_cast<uint8_t*>(((uintptr_t)slot->staged.p + 255) & ~uintptr_t(255));
    uint64_t* lens = reinterpret_cast<uint64_t*>(p);
    uint64_t* ps = reinterpret_cast<uint64_t*>(p += b_ps);
    uint64_t* hpos = reinterpret_cast<uint64_t*>(p += b_ps);
    uint64_t* x_files = reinterpret_cast<uint64_t*>(p += b_m);
    uint64_t* counts = reinterpret_cast<uint64_t*>(p += b_files);
    uint8_t* flags = p += b_counts;
    void* tmp = p += b_flags;
    slot->hashes.ensure(DP_STATE * sizeof(uint64_t));
    slot->host_hashes.ensure(DP_STATE * sizeof(uint64_t));
    uint64_t* d_st = slot->hashes.as<uint64_t>();
    const uint64_t* st = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);
    std::vector<uint64_t> tab(chunk_base, chunk_base + n + 1);
    slot->aux.begin();
    slot->aux.add(tab);
    slot->aux.upload(s);
    uint64_t* files = d_files_out ? d_files_out : x_files;
    const dp_view v{slot->aux.at<uint64_t>(0), (uint32_t)n, (uint32_t)n_base, t0, mt, d_chunks, d_rep, ps};

    HIP_CHECK(hipMemsetAsync(d_st, 0, DP_STATE * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(files, 0, 48 * nt, s));
    hipLaunchKernelGGL(k_dp_classify, dim3(flat_grid(mt + 1)), dim3(256), 0, s, v, lens, files, d_st);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(rocprim::exclusive_scan(tmp, sb, lens, ps, uint64_t(0), (size_t)(mt + 1), rocprim::plus<uint64_t>(), s));
    const uint32_t g = sliced_grid(mt);
    launch_flag(g, s, dp_head{v, d_lit_off, files}, nullptr, mt, flags, counts);
    launch_compact(g, s, dp_head_pos{{flags}, hpos}, nullptr, mt, counts, d_st + DP_RUNS);
    if (d_runs_out) hipLaunchKernelGGL(k_dp_rows, dim3(flat_grid(mt)), dim3(256), 0, s, v, hpos, d_st, d_runs_out, capacity);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, d_st, DP_STATE * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (st[DP_BAD]) throw sd_failure(SD_ERR_INVALID, "rep is not a representative table of these chunks");
    if (st[DP_COPY_CHUNKS] + st[DP_LIT_CHUNKS] + st[DP_REP_CHUNKS] != mt || st[DP_RUNS] > mt)
        throw sd_failure(SD_ERR_INTERNAL, "delta: inconsistent totals");
    if (n_runs) *n_runs = st[DP_RUNS];
    if (stats) {
        const uint64_t out[8] = {nt, mt, st[DP_COPY_CHUNKS], st[DP_COPY_BYTES], st[DP_LIT_CHUNKS], st[DP_LIT_BYTES],
                                 st[DP_REP_CHUNKS], st[DP_RUNS]};
        memcpy(stats, out, sizeof out);
    }
    if (d_runs_out && capacity < st[DP_RUNS]) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of runs");
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cdc_delta_pack(sd_cas_ctx* ctx, const uint64_t* chunk_base, size_t n, size_t n_base,
                                 const uint64_t* offsets, const uint64_t* d_chunks, const uint64_t* d_lit_off,
                                 const uint64_t* d_rep, const uint8_t* d_data, uint8_t* d_lit_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx) throw sd_failure(SD_ERR_INVALID, "null argument");
    uint64_t t0 = 0;
    const uint64_t mt = cdc_delta_check_plan(chunk_base, n, n_base, d_chunks, d_rep, &t0);
    if (mt == 0) return SD_OK;
    if (!offsets || !d_lit_off) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_data) % 16) throw sd_failure(SD_ERR_INVALID, "d_data not 16-byte aligned");
    for (size_t f = n_base; f < n; f++)
        if (offsets[f] % 16) throw sd_failure(SD_ERR_INVALID, "a range does not start 16-byte aligned");
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    ctx->delta.scratch.ensure(seg_scratch(nullptr, mt).total);  // grown by the plan already
    const seg_scratch x(ctx->delta.scratch.p, mt);
    std::vector<uint64_t> tab(chunk_base, chunk_base + n + 1);
    tab.insert(tab.end(), offsets, offsets + n);
    const uint64_t* d_tab = upload_tab(ctx, tab, s);
    hipLaunchKernelGGL(k_dk_segs, dim3(flat_grid(mt + 1)), dim3(256), 0, s, d_tab, (uint32_t)n, t0, mt, d_chunks, d_rep,
                       d_lit_off, (uint64_t)(uintptr_t)d_data, (uint64_t)(uintptr_t)d_lit_out, x.segs, x.pieces);
    HIP_CHECK(hipGetLastError());
    scan(x, x.pieces, x.piece_base, mt + 1, s);
    // the piece count stays on the device: a full grid strides over whatever it is
    hipLaunchKernelGGL(k_seg_copy, dim3(copy_grid(1ull << 40)), dim3(256), 0, s, x.segs, x.piece_base, mt);
    HIP_CHECK(hipGetLastError());
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cdc_delta_apply(sd_cas_ctx* ctx, const uint64_t* d_runs, uint64_t n_runs, const uint64_t* base_offsets,
                                  const uint64_t* base_lens, size_t n_base, const uint8_t* d_base, const uint8_t* d_lit,
                                  uint64_t lit_bytes, const uint64_t* out_offsets, const uint64_t* out_lens,
                                  size_t n_targets, uint8_t* d_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx) throw sd_failure(SD_ERR_INVALID, "null argument");
    cdc_delta_check_apply(d_runs, n_runs, base_offsets, base_lens, n_base, d_base, d_lit, lit_bytes, out_offsets, out_lens,
                          n_targets, d_out);
    if (reinterpret_cast<uintptr_t>(d_base) % 16 || reinterpret_cast<uintptr_t>(d_lit) % 16)
        throw sd_failure(SD_ERR_INVALID, "d_base or d_lit not 16-byte aligned");
    for (size_t g = 0; g < n_base; g++)
        if (base_offsets[g] % 16) throw sd_failure(SD_ERR_INVALID, "a range does not start 16-byte aligned");
    if (n_targets == 0 && n_runs == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    SlotHold slot(ctx);
    const uint64_t R = n_runs;
    ctx->delta.scratch.ensure(seg_scratch(nullptr, R).total);
    const seg_scratch x(ctx->delta.scratch.p, R);
    std::vector<uint64_t> tab;
    tab.reserve(2 * n_base + 2 * n_targets + 1);
    tab.insert(tab.end(), base_offsets, base_offsets + n_base);
    tab.insert(tab.end(), base_lens, base_lens + n_base);
    tab.insert(tab.end(), out_offsets, out_offsets + n_targets);
    tab.insert(tab.end(), out_lens, out_lens + n_targets);
    tab.push_back(0);  // never empty
    const da_view v{d_runs, R, upload_tab(ctx, tab, s), (uint32_t)n_base, (uint32_t)n_targets, lit_bytes};
    slot->host_hashes.ensure(2 * sizeof(uint64_t));
    const uint64_t* host = reinterpret_cast<const uint64_t*>(slot->host_hashes.p);

    HIP_CHECK(hipMemsetAsync(x.state, 0, DA_STATE * sizeof(uint64_t), s));
    hipLaunchKernelGGL(k_da_check, dim3(flat_grid(R + 1)), dim3(256), 0, s, v, x.blen, x.state);
    HIP_CHECK(hipGetLastError());
    scan(x, x.blen, x.ps, R + 1, s);
    hipLaunchKernelGGL(k_da_segs, dim3(flat_grid(std::max<uint64_t>(R + 1, n_targets))), dim3(256), 0, s, v, x.ps,
                       (uint64_t)(uintptr_t)d_base, (uint64_t)(uintptr_t)d_lit, (uint64_t)(uintptr_t)d_out, x.segs, x.pieces,
                       x.state);
    HIP_CHECK(hipGetLastError());
    scan(x, x.pieces, x.piece_base, R + 1, s);
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.p, x.state + DA_BAD, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(slot->host_hashes.u8() + 8, x.piece_base + R, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the one wait: the verdict, and the pieces for the grid
    if (host[0]) throw sd_failure(SD_ERR_INVALID, "the recipe is not valid for these files: nothing was written");
    if (host[1] == 0) return SD_OK;
    hipLaunchKernelGGL(k_seg_copy, dim3(copy_grid(host[1])), dim3(256), 0, s, x.segs, x.piece_base, R);
    HIP_CHECK(hipGetLastError());
    return SD_OK;
    SD_GUARD_END
}
