// cdc.hip -- content-defined chunks on the device (include/sd_cas.h, "content-defined chunks"):
// sd_cdc_create / _cut / _layout / _stats / _hash.
//
//   scan     k_cdc_scan: one workgroup per tile of CDC_TILE consecutive bytes of one file.  The tile
//            and the 64 bytes in front of it (none for a file's first tile: bytes of the range
//            before never enter) are staged into LDS with coalesced 16-byte loads, in 64-byte rows
//            padded to 17 dwords so that the lanes' row walks hit 64 different banks.  Lane t warms
//            its rolling value over row t and walks row t + 1, its own 64 bytes; the 64 answers
//            leave as one 64-bit word of the file's bitmap (one bit per byte position, the bits past
//            the file's end cleared).  The gear table sits in LDS (2 KiB).  A bitmap and no list: a
//            constant-byte file can make every position a candidate
//   select   k_cdc_select: one wave per file walks its bitmap.  Per step the 64 lanes load
//            CDC_SELECT_WORDS consecutive words (four independent loads per lane, 64 words each) from
//            bit s + min_size - 1 on, as far as s + max_size - 1 and the file's end; a ballot per 64
//            words and the first set bit give the chunk's end.  Every loop is bounded
//            by the file's length; min_size >= 64 guarantees progress.  The first pass leaves the
//            chunks per file, a prefix sum (rocprim) their bases, the second pass writes (offset,
//            length) and the chunk's byte address.  A single huge file is a serial walk
//   hash     k_cdc_pieces: one lane per 4 KiB piece (CDC_LANE_CHUNKS BLAKE3 chunks) over the flat
//            space of all pieces of all CDC chunks, its owner by binary search in the pieces' prefix
//            sum.  The data is read in place: load_block_shift takes the aligned 16-byte units that
//            hold the block's bytes and realigns them by the start's residue (two conditional dword
//            moves, then v_alignbyte).  A CDC chunk of at most 4 KiB finishes in its lane with ROOT;
//            k_cdc_tree then merges the up to 256 piece CVs of every longer one in LDS, ROOT on the
//            last parent
// Integer adds only in the statistics: they do not depend on the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "blake3_cv.h"
#include "sd_api_impl.h"

using namespace sdb3;
using namespace sdi;

namespace {

constexpr uint32_t CDC_TILE = 16384;     // bytes of a scan tile: 256 lanes x one 64-bit bitmap word
constexpr uint32_t CDC_ROW_DWORDS = 17;  // a 64-byte LDS row and its pad
constexpr uint32_t CDC_SELECT_WORDS = 256;  // bitmap words a wave of the select looks at per step: 4 per lane
constexpr uint32_t CDC_LANE_CHUNKS = 4;  // BLAKE3 chunks of a hash lane's piece
constexpr uint32_t CDC_PIECE = CDC_LANE_CHUNKS * CHUNK_LEN;
static_assert(CDC_TILE == 256 * 64, "one bitmap word per lane");
static_assert(CDC_SELECT_WORDS % 64 == 0 && CDC_SELECT_WORDS >= 64, "whole words per lane");

// device state (u64): [2] candidates, [4..6] the chunk kinds, [7] compressions
constexpr uint32_t CDC_STATE = 8;

__device__ __forceinline__ uint64_t gear_of(uint32_t b) {
    uint64_t z = (0x5DCDC0DEull ^ b) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the last index i in [0, n] with base[i] <= x (base ascends, base[0] <= x)
__device__ __forceinline__ uint64_t owner_of(const uint64_t* __restrict__ base, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// tab: tile_base[0 .. n], then offsets, lens and word_base, n each
__global__ __launch_bounds__(256) void k_cdc_scan(const uint4* __restrict__ units, const uint64_t* __restrict__ tab,
                                                  uint32_t n, uint64_t ntiles, uint64_t mask,
                                                  uint64_t* __restrict__ bitmap, uint64_t* __restrict__ st) {
    __shared__ uint64_t gear[256];
    __shared__ uint32_t rows[(CDC_TILE / 64 + 1) * CDC_ROW_DWORDS];
    const uint32_t t = threadIdx.x;
    gear[t] = gear_of(t);
    uint32_t found = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t f = owner_of(tab, n, tile);
        const uint64_t off = tab[n + 1 + f], len = tab[2 * (uint64_t)n + 1 + f], wbase = tab[3 * (uint64_t)n + 1 + f];
        const uint64_t t0 = (tile - tab[f]) * CDC_TILE;  // the tile's first byte in its file
        const uint32_t tlen = (uint32_t)(len - t0 < CDC_TILE ? len - t0 : CDC_TILE);
        // staged unit u holds the file's bytes t0 - 64 + 16 u ..; row 0 is the warm-up
        const uint32_t u_begin = t0 ? 0 : 4, u_end = 4 + (tlen + 15) / 16;
        const uint4* src = units + ((off + t0) >> 4);
        for (uint32_t u = u_begin + t; u < u_end; u += 256) {
            const uint4 v = src[(int64_t)u - 4];
            uint32_t* d = rows + (u >> 2) * CDC_ROW_DWORDS + (u & 3) * 4;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        __syncthreads();
        if (64 * t < tlen) {
            uint64_t h = 0;
            if (t0 != 0 || t != 0) {
                const uint32_t* w = rows + t * CDC_ROW_DWORDS;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const uint32_t x = w[k];
#pragma unroll
                    for (int b = 0; b < 4; b++) h = (h << 1) + gear[(x >> (8 * b)) & 255];
                }
            }
            const uint32_t* w = rows + (t + 1) * CDC_ROW_DWORDS;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t x = w[k];
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    h = (h << 1) + gear[(x >> (8 * b)) & 255];
                    const uint32_t c = (h & mask) == 0 ? 1u : 0u;
                    if (k < 8) lo |= c << (4 * k + b);
                    else hi |= c << (4 * (k - 8) + b);
                }
            }
            uint64_t bits = (uint64_t)lo | ((uint64_t)hi << 32);
            const uint32_t valid = tlen - 64 * t;  // bytes of the file in this word
            if (valid < 64) bits &= (1ull << valid) - 1;
            bitmap[wbase + t0 / 64 + t] = bits;
            found += (uint32_t)__popcll(bits);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) found += __shfl_xor(found, o);
    if ((t & 63) == 0 && found) atomicAdd(reinterpret_cast<unsigned long long*>(st + 2), (unsigned long long)found);
}

// One wave per file.  WRITE false: counts[f] = the file's chunks, the kinds -> st[4..6].  WRITE true:
// chunk c = chunk_base[f] + k gets chunks[2 c] = its offset in the file, chunks[2 c + 1] = its
// length, addr[c] = its first byte in the buffer.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_cdc_select(const uint64_t* __restrict__ tab, uint32_t n,
                                                    const uint64_t* __restrict__ bitmap, uint32_t min_size,
                                                    uint32_t max_size, uint64_t* __restrict__ counts,
                                                    const uint64_t* __restrict__ chunk_base,
                                                    uint64_t* __restrict__ chunks, uint64_t* __restrict__ addr,
                                                    uint64_t* __restrict__ st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64);
    for (uint64_t f = (uint64_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; f < n; f += waves) {
        const uint64_t off = tab[n + 1 + f], len = tab[2 * (uint64_t)n + 1 + f];
        const uint64_t* bm = bitmap + tab[3 * (uint64_t)n + 1 + f];
        uint64_t s = 0, k = 0, at_cand = 0, forced = 0, at_end = 0;
        const uint64_t c0 = WRITE ? chunk_base[f] : 0;
        do {
            uint64_t e = 0;
            bool hit = false;
            if (len - s >= min_size) {
                // candidate positions i with s + min_size <= i + 1 <= min(s + max_size, len)
                const uint64_t lo = s + min_size - 1;
                const uint64_t hi = (len - s < max_size ? len : s + max_size) - 1;
                const uint64_t first = lo >> 6, last = hi >> 6;
                for (uint64_t w0 = first; w0 <= last && !hit; w0 += CDC_SELECT_WORDS) {
                    uint64_t v[CDC_SELECT_WORDS / 64];  // the loads of a step are independent: one latency per step
#pragma unroll
                    for (uint32_t j = 0; j < CDC_SELECT_WORDS / 64; j++) {
                        const uint64_t w = w0 + 64 * j + lane;
                        v[j] = 0;
                        if (w <= last) {
                            v[j] = bm[w];
                            if (w == first) v[j] &= ~0ull << (lo & 63);
                            if (w == last) v[j] &= ~0ull >> (63 - (hi & 63));
                        }
                    }
#pragma unroll
                    for (uint32_t j = 0; j < CDC_SELECT_WORDS / 64; j++) {
                        const uint64_t any = __ballot(v[j] != 0);
                        if (any && !hit) {
                            const int lane1 = __ffsll((unsigned long long)any) - 1;
                            const uint64_t vv = __shfl(v[j], lane1);
                            e = (w0 + 64 * j + lane1) * 64 + (uint64_t)__ffsll((unsigned long long)vv);  // position + 1
                            hit = true;
                        }
                    }
                }
            }
            if (!hit) e = len - s < max_size ? len : s + max_size;
            at_end += e == len;
            at_cand += e != len && hit;
            forced += e != len && !hit;
            if (WRITE && lane == 0) {
                chunks[2 * (c0 + k)] = s;
                chunks[2 * (c0 + k) + 1] = e - s;
                addr[c0 + k] = off + s;
            }
            k++;
            s = e;
        } while (s < len);
        if (!WRITE && lane == 0) {
            counts[f] = k;
            unsigned long long* t = reinterpret_cast<unsigned long long*>(st);
            if (at_cand) atomicAdd(t + 4, (unsigned long long)at_cand);
            if (forced) atomicAdd(t + 5, (unsigned long long)forced);
            atomicAdd(t + 6, (unsigned long long)at_end);
        }
    }
}

// pieces[c] = the 4 KiB pieces of chunk c (an empty chunk has one), pieces[m] = 0; st[7] += the
// compressions of the chunks' hashes
__global__ __launch_bounds__(256) void k_cdc_count_pieces(const uint64_t* __restrict__ chunks, uint64_t m,
                                                          uint64_t* __restrict__ pieces, uint64_t* __restrict__ st) {
    uint64_t comp = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= m; c += (uint64_t)gridDim.x * blockDim.x) {
        if (c == m) {
            pieces[c] = 0;
            continue;
        }
        const uint64_t len = chunks[2 * c + 1];
        pieces[c] = len == 0 ? 1 : (len + CDC_PIECE - 1) / CDC_PIECE;
        comp += len == 0 ? 1 : (len / 1024) * 16 + (len % 1024 + 63) / 64 + (len + 1023) / 1024 - 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) comp += __shfl_xor(comp, o);
    if ((threadIdx.x & 63) == 0 && comp) atomicAdd(reinterpret_cast<unsigned long long*>(st + 7), (unsigned long long)comp);
}

// nbytes (0..64) message bytes from byte address a of the buffer, any alignment -> 16 little-endian
// words, the bytes past nbytes zero (BLAKE3 padding).  Loads only the aligned 16-byte units that
// hold one of those bytes: the buffer is promised readable to the next 64-byte boundary after a
// range, no further.
__device__ __forceinline__ void load_block_shift(uint32_t (&m)[16], const uint4* __restrict__ units, uint64_t a,
                                                 uint32_t nbytes) {
    const uint4* q = units + (a >> 4);
    const uint32_t r = (uint32_t)a & 15u;
    const uint32_t held = nbytes ? ((r + nbytes - 1) >> 4) + 1 : 0;  // units that hold a byte: 0..5
    uint32_t w[20];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if ((uint32_t)k < held) v = q[k];
        w[4 * k + 0] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    if (r & 4u) {
#pragma unroll
        for (int i = 0; i < 19; i++) w[i] = w[i + 1];
    }
    if (r & 8u) {
#pragma unroll
        for (int i = 0; i < 18; i++) w[i] = w[i + 2];
    }
#pragma unroll
    for (int i = 0; i < 16; i++) m[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], r & 3u);
    if (nbytes < 64) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t lo = 4u * i;
            m[i] &= nbytes <= lo ? 0u : (nbytes >= lo + 4 ? 0xFFFFFFFFu : (0xFFFFFFFFu >> (8 * (lo + 4 - nbytes))));
        }
    }
}

// chunk_cv (blake3_device.h) for a chunk that starts at any byte address
template <bool W>
__device__ __forceinline__ void chunk_cv_shift(uint32_t (&cv)[8], const uint4* __restrict__ units, uint64_t a,
                                               uint32_t len, uint32_t counter, bool is_root) {
    set_iv(cv);
    const uint32_t nblocks = len == 0 ? 1u : (len + 63u) >> 6;
    uint32_t m[16];
#pragma unroll 1
    for (uint32_t b = 0; b + 1 < nblocks; b++) {
        load_block_shift(m, units, a + 64u * b, 64u);
        compress<W>(cv, m, counter, 0u, BLOCK_LEN, b == 0 ? CHUNK_START : 0u);
    }
    const uint32_t last = nblocks - 1, tail = len - 64u * last;
    load_block_shift(m, units, a + 64u * last, tail);
    compress<W>(cv, m, counter, 0u, tail, (last == 0 ? CHUNK_START : 0u) | CHUNK_END | (is_root ? ROOT : 0u));
}

// One lane per piece p of the flat piece space: chunk c = the owner of p in piece_base, piece j of
// it = its bytes [4096 j, 4096 (j + 1)) -- BLAKE3 chunks 4 j .. of the chunk as a message, merged
// in the lane.  A chunk of one piece leaves its id (ROOT inside the lane), any other piece its CV
// at cvs[p].
template <bool W>
__global__ __launch_bounds__(256) void k_cdc_pieces(const uint4* __restrict__ units, const uint64_t* __restrict__ chunks,
                                                    const uint64_t* __restrict__ addr,
                                                    const uint64_t* __restrict__ piece_base, uint64_t m,
                                                    uint64_t total, uint32_t* __restrict__ cvs,
                                                    uint32_t* __restrict__ ids) {
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t c = owner_of(piece_base, m, p);
        const uint32_t j = (uint32_t)(p - piece_base[c]);
        const uint32_t len = (uint32_t)chunks[2 * c + 1];  // <= 1 MiB
        const uint64_t a = addr[c] + (uint64_t)j * CDC_PIECE;
        const uint32_t plen = len - j * CDC_PIECE < CDC_PIECE ? len - j * CDC_PIECE : CDC_PIECE;
        const bool single = len <= CDC_PIECE;  // the whole chunk inside this lane
        const uint32_t nch = plen == 0 ? 1u : (plen + CHUNK_LEN - 1) / CHUNK_LEN;
        CvStack<ilog2(CDC_LANE_CHUNKS)> st;  // after BLAKE3 chunk i it holds popcount(i + 1) subtrees
        uint32_t cv[8];
#pragma unroll 1
        for (uint32_t i = 0; i < nch; i++) {
            const uint32_t rem = plen - i * CHUNK_LEN;
            chunk_cv_shift<W>(cv, units, a + (uint64_t)i * CHUNK_LEN, rem < CHUNK_LEN ? rem : CHUNK_LEN,
                              j * CDC_LANE_CHUNKS + i, single && nch == 1);
            if (i + 1 < nch) {  // an aligned group that ends here merges, then waits on the stack
#pragma unroll 1
                for (uint32_t g = i + 1; (g & 1u) == 0; g >>= 1) st.template merge_top<W>(cv, 0u);
                st.push(cv);
            } else {  // the lane's last chunk: its aligned merges and the fold
                const uint32_t ops = (uint32_t)__builtin_popcount(nch - 1);
#pragma unroll 1
                for (uint32_t k = ops; k > 0; k--) st.template merge_top<W>(cv, (single && k == 1) ? ROOT : 0u);
            }
        }
        store_cv(single ? ids + 8 * c : cvs + 8 * p, cv);
    }
}

// One workgroup per chunk of more than one piece: its 2..256 piece CVs merged level-wise in LDS,
// ROOT on the last parent -> ids[c]
__global__ __launch_bounds__(256) void k_cdc_tree(const uint64_t* __restrict__ piece_base, uint64_t m,
                                                  const uint32_t* __restrict__ cvs, uint32_t* __restrict__ ids) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[256][8];
    const uint32_t t = threadIdx.x;
    for (uint64_t c = blockIdx.x; c < m; c += gridDim.x) {
        const uint64_t p0 = piece_base[c];
        const uint32_t np = (uint32_t)(piece_base[c + 1] - p0);
        if (np < 2) continue;  // the same in every lane
        if (t < np) {
            uint32_t cv[8];
            load_cv(cv, cvs + 8 * (p0 + t));
            store_cv(lds[t], cv);
        }
        __syncthreads();
        lds_reduce<false>(lds, np, true);
        if (t < 8) ids[8 * c + t] = lds[0][t];
        __syncthreads();
    }
}

// cas_kernels.hip's rule for the priority windows of blake3_device.h: they pay once a launch has
// more waves than the device has SIMDs
bool windows_for(uint64_t waves) {
    static const uint64_t simds = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        return (uint64_t)cus * 4;
    }();
    return SD_G_PRIO != 0 && waves > simds;
}

uint32_t grid_for(uint64_t items, uint64_t per_wg, uint32_t most) {
    const uint64_t g = (items + per_wg - 1) / per_wg;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(g, 1), most);
}

size_t scan_bytes(uint64_t count, hipStream_t s) {
    size_t b = 0;
    uint64_t* nul = nullptr;
    if (rocprim::exclusive_scan(nullptr, b, nul, nul, uint64_t(0), (size_t)count, rocprim::plus<uint64_t>(), s) != hipSuccess)
        throw sd_failure(SD_ERR_INTERNAL, "cdc: the scan's storage size");
    return b;
}

}  // namespace

struct sd_cdc {
    sd_cas_ctx* ctx = nullptr;
    size_t n = 0;
    sd_cdc_params p{};
    uint64_t bytes = 0, ntiles = 0, nwords = 0;
    DevBuf tab, bitmap, state;
    DevBuf counts, base;          // n + 1 each: the chunks per file and their prefix sum
    DevBuf chunks, addr;          // per chunk: (offset, length), first byte in the buffer
    DevBuf pieces, piece_base;    // m + 1 each
    DevBuf cvs;                   // 32 bytes per piece
    DevBuf tmp;                   // the prefix sums' temporary storage
    PinnedBuf host;               // CDC_STATE + 1 u64
    std::vector<uint64_t> chunk_base;  // host, n + 1, after a cut
    bool cut = false;
    uint64_t m = 0, total_pieces = 0, stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t* d_tab() const { return tab.as<uint64_t>(); }
};

extern "C" int sd_cdc_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                             const sd_cdc_params* params, sd_cdc** out) {
    SD_GUARD_BEGIN
    if (!ctx || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    cdc_check_params(params);
    const uint64_t bytes = cdc_check_ranges(offsets, lens, n, *params);
    auto c = std::make_unique<sd_cdc>();
    c->ctx = ctx, c->n = n, c->p = *params, c->bytes = bytes;
    std::vector<uint64_t> tab(4 * n + 1);  // tile_base[0 .. n], offsets, lens, word_base
    for (size_t f = 0; f < n; f++) {
        tab[f] = c->ntiles;
        tab[n + 1 + f] = offsets[f];
        tab[2 * n + 1 + f] = lens[f];
        tab[3 * n + 1 + f] = c->nwords;
        c->ntiles += (lens[f] + CDC_TILE - 1) / CDC_TILE;
        c->nwords += (lens[f] + 63) / 64;
    }
    tab[n] = c->ntiles;
    ctx->bind();
    c->tab.upload(tab);
    c->bitmap.ensure(c->nwords * sizeof(uint64_t));
    c->state.ensure(CDC_STATE * sizeof(uint64_t));
    c->counts.ensure((n + 1) * sizeof(uint64_t));
    c->base.ensure((n + 1) * sizeof(uint64_t));
    c->host.ensure((CDC_STATE + 1) * sizeof(uint64_t));
    c->chunk_base.assign(n + 1, 0);
    *out = c.release();
    return SD_OK;
    SD_GUARD_END
}

extern "C" void sd_cdc_destroy(sd_cdc* cdc) { delete cdc; }

extern "C" int sd_cdc_cut(sd_cas_ctx* ctx, sd_cdc* cdc, const uint8_t* d_data, void* stream, uint64_t* n_chunks) {
    SD_GUARD_BEGIN
    if (!ctx || !cdc || cdc->ctx != ctx) throw sd_failure(SD_ERR_INVALID, "null argument or another context's batch");
    if (cdc->bytes && !d_data) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_data) % 16) throw sd_failure(SD_ERR_INVALID, "d_data not 16-byte aligned");
    if (n_chunks) *n_chunks = 0;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    const size_t n = cdc->n;
    const uint32_t n32 = (uint32_t)n;
    cdc->cut = false;
    uint64_t* d_st = cdc->state.as<uint64_t>();
    uint64_t* host = reinterpret_cast<uint64_t*>(cdc->host.p);
    const uint4* units = reinterpret_cast<const uint4*>(d_data);
    const uint64_t mask = ((1ull << cdc->p.mask_bits) - 1) << (64 - cdc->p.mask_bits);
    uint64_t m = 0, total_pieces = 0;
    memset(host, 0, (CDC_STATE + 1) * sizeof(uint64_t));
    if (n) {
        HIP_CHECK(hipMemsetAsync(d_st, 0, CDC_STATE * sizeof(uint64_t), s));
        if (cdc->ntiles)
            hipLaunchKernelGGL(k_cdc_scan, dim3(grid_for(cdc->ntiles, 1, 1u << 16)), dim3(256), 0, s, units, cdc->d_tab(),
                               n32, cdc->ntiles, mask, cdc->bitmap.as<uint64_t>(), d_st);
        uint64_t* counts = cdc->counts.as<uint64_t>();
        uint64_t* base = cdc->base.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(counts + n, 0, sizeof(uint64_t), s));
        const uint32_t g_sel = grid_for(n, 4, 1u << 16);
        hipLaunchKernelGGL(k_cdc_select<false>, dim3(g_sel), dim3(256), 0, s, cdc->d_tab(), n32,
                           cdc->bitmap.as<uint64_t>(), cdc->p.min_size, cdc->p.max_size, counts, nullptr, nullptr,
                           nullptr, d_st);
        HIP_CHECK(hipGetLastError());
        size_t tb = scan_bytes(n + 1, s);
        cdc->tmp.ensure(tb);
        HIP_CHECK(rocprim::exclusive_scan(cdc->tmp.p, tb, counts, base, uint64_t(0), n + 1, rocprim::plus<uint64_t>(), s));
        HIP_CHECK(hipMemcpyAsync(cdc->chunk_base.data(), base, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        m = cdc->chunk_base[n];
        if (m < n || m >= (1ull << 32)) throw sd_failure(SD_ERR_INTERNAL, "cdc: inconsistent chunk count");
        // the buffers the count sizes: grown only after the stream has drained
        cdc->chunks.ensure(2 * m * sizeof(uint64_t));
        cdc->addr.ensure(m * sizeof(uint64_t));
        cdc->pieces.ensure((m + 1) * sizeof(uint64_t));
        cdc->piece_base.ensure((m + 1) * sizeof(uint64_t));
        tb = scan_bytes(m + 1, s);
        cdc->tmp.ensure(tb);
        uint64_t* chunks = cdc->chunks.as<uint64_t>();
        hipLaunchKernelGGL(k_cdc_select<true>, dim3(g_sel), dim3(256), 0, s, cdc->d_tab(), n32,
                           cdc->bitmap.as<uint64_t>(), cdc->p.min_size, cdc->p.max_size, nullptr, base, chunks,
                           cdc->addr.as<uint64_t>(), d_st);
        hipLaunchKernelGGL(k_cdc_count_pieces, dim3(grid_for(m + 1, 256, 4096)), dim3(256), 0, s, chunks, m,
                           cdc->pieces.as<uint64_t>(), d_st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(rocprim::exclusive_scan(cdc->tmp.p, tb, cdc->pieces.as<uint64_t>(), cdc->piece_base.as<uint64_t>(),
                                          uint64_t(0), m + 1, rocprim::plus<uint64_t>(), s));
        HIP_CHECK(hipMemcpyAsync(host, d_st, CDC_STATE * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(host + CDC_STATE, cdc->piece_base.as<uint64_t>() + m, sizeof(uint64_t),
                                 hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        total_pieces = host[CDC_STATE];
        if (host[4] + host[5] + host[6] != m || total_pieces < m)
            throw sd_failure(SD_ERR_INTERNAL, "cdc: inconsistent chunk totals");
        cdc->cvs.ensure(32 * total_pieces);
    }
    cdc->m = m, cdc->total_pieces = total_pieces;
    const uint64_t st[8] = {n, cdc->bytes, host[2], m, host[4], host[5], host[6], host[7]};
    memcpy(cdc->stats, st, sizeof st);
    cdc->cut = true;
    if (n_chunks) *n_chunks = m;
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cdc_layout(const sd_cdc* cdc, uint64_t* chunk_base) {
    SD_GUARD_BEGIN
    if (!cdc || !chunk_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!cdc->cut) throw sd_failure(SD_ERR_INVALID, "no cut yet");
    memcpy(chunk_base, cdc->chunk_base.data(), (cdc->n + 1) * sizeof(uint64_t));
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cdc_stats(const sd_cdc* cdc, uint64_t out[8]) {
    SD_GUARD_BEGIN
    if (!cdc || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (!cdc->cut) throw sd_failure(SD_ERR_INVALID, "no cut yet");
    memcpy(out, cdc->stats, 8 * sizeof(uint64_t));
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cdc_hash(sd_cas_ctx* ctx, sd_cdc* cdc, const uint8_t* d_data, uint64_t* d_chunks_out,
                           uint8_t* d_ids_out, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !cdc || cdc->ctx != ctx) throw sd_failure(SD_ERR_INVALID, "null argument or another context's batch");
    if (!cdc->cut) throw sd_failure(SD_ERR_INVALID, "no cut yet");
    if (cdc->bytes && !d_data) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_data) % 16) throw sd_failure(SD_ERR_INVALID, "d_data not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_ids_out) % 16) throw sd_failure(SD_ERR_INVALID, "d_ids_out not 16-byte aligned");
    const uint64_t m = cdc->m, total = cdc->total_pieces;
    if (m == 0) return SD_OK;
    ctx->bind();
    hipStream_t s = ctx->pick(stream);
    if (d_chunks_out)
        HIP_CHECK(hipMemcpyAsync(d_chunks_out, cdc->chunks.p, 2 * m * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    if (!d_ids_out) return SD_OK;
    const uint4* units = reinterpret_cast<const uint4*>(d_data);
    uint32_t* ids = reinterpret_cast<uint32_t*>(d_ids_out);
    const uint32_t g = grid_for(total, 256, 1u << 20);
    if (windows_for((uint64_t)g * 4))
        hipLaunchKernelGGL(k_cdc_pieces<true>, dim3(g), dim3(256), 0, s, units, cdc->chunks.as<uint64_t>(),
                           cdc->addr.as<uint64_t>(), cdc->piece_base.as<uint64_t>(), m, total, cdc->cvs.as<uint32_t>(), ids);
    else
        hipLaunchKernelGGL(k_cdc_pieces<false>, dim3(g), dim3(256), 0, s, units, cdc->chunks.as<uint64_t>(),
                           cdc->addr.as<uint64_t>(), cdc->piece_base.as<uint64_t>(), m, total, cdc->cvs.as<uint32_t>(), ids);
    if (total > m)  // some chunk has more than one piece
        hipLaunchKernelGGL(k_cdc_tree, dim3(grid_for(m, 1, 1u << 16)), dim3(256), 0, s, cdc->piece_base.as<uint64_t>(), m,
                           cdc->cvs.as<uint32_t>(), ids);
    HIP_CHECK(hipGetLastError());
    return SD_OK;
    SD_GUARD_END
}
