// gather.hip -- k_cas_gather: the cas message of each file of a fingerprint batch, built on the
// device from the file's bytes where they already sit (a byte range of one device buffer), into
// the staged layout every cas kernel of cas_kernels.hip reads: le64(len) || file for a
// whole-kind file, le64(len) || head || 4 samples || tail for a sampled one (cas.rs:25-58; the
// same source map as synth.hip's sampled_src and oracle/cas_spec.py's sample_windows), then
// zeros up to the next SD_STAGE_ALIGN.  Nothing else is written.
//
// Mapping: one lane per 16-byte output unit.  The units of all files, in file order, form one
// flat space; a workgroup takes a tile of SD_GATHER_TILE_UNITS of them (4 units per lane, a
// wave's 64 lanes on 1 KiB of consecutive output) and finds each unit's file by a binary search
// between the first files of its tile and of the next (sd_host.h, GatherPlan).
//
// Every segment boundary of a message sits at a position = 8 (mod 16), so each 8-byte half of
// a unit comes from one segment: 8 consecutive file bytes at any byte alignment.  They are read
// with aligned 16-byte loads -- one, or two when the 8 bytes straddle units -- and 64-bit
// shifts; a unit that holds no needed byte is never loaded (the buffer is only promised
// readable to the 64-byte boundary after each range).  Stores are whole aligned 16-byte units,
// the zero padding inside the last partial one included.
#include <hip/hip_runtime.h>

#include "sd_internal.h"

namespace {

__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// `valid` (1..8) bytes of the buffer from byte address a, little-endian packed, the rest zero
__device__ __forceinline__ uint64_t load8(const uint4* __restrict__ units, uint64_t a, uint32_t valid) {
    const uint64_t A = a >> 4;
    const uint32_t s = (uint32_t)a & 15u;
    const uint4 v0 = units[A];
    uint64_t r;
    if (s < 8) {  // bytes s .. s + 7 of this unit
        r = u64_of(v0.x, v0.y) >> (8 * s);
        if (s) r |= u64_of(v0.z, v0.w) << (64 - 8 * s);
    } else {
        const uint32_t t = s - 8;
        r = u64_of(v0.z, v0.w) >> (8 * t);
        if (s + valid > 16) {  // the needed bytes run into the next unit (t > 0 here)
            const uint4 v1 = units[A + 1];
            r |= u64_of(v1.x, v1.y) << (64 - 8 * t);
        }
    }
    if (valid < 8) r &= (1ull << (8 * valid)) - 1;
    return r;
}

// message position q (multiple of 8, 8 <= q < 57352) -> file offset (cas.rs:31-58)
__device__ __forceinline__ uint64_t sampled_src(uint64_t len, uint32_t q) {
    const uint32_t H = SD_HEADER_OR_FOOTER_SIZE, S = SD_SAMPLE_SIZE;
    const uint32_t m = q - 8;  // position inside head || samples || tail
    if (m < H) return m;
    if (m < H + SD_SAMPLE_COUNT * S) {
        const uint32_t k = (m - H) / S;
        const uint64_t jump = (len - 2 * H) / SD_SAMPLE_COUNT;
        return H + k * jump + (m - H - k * S);
    }
    return len - H + (m - H - SD_SAMPLE_COUNT * S);
}

// the 8 message bytes at position q (multiple of 8) of a file of `len` bytes at data_off
__device__ __forceinline__ uint64_t msg8(const uint4* __restrict__ units, uint64_t data_off, uint64_t len,
                                         bool sampled, uint32_t msg_len, uint32_t q) {
    if (q == 0) return len;         // cas.rs:25 le64(size)
    if (q >= msg_len) return 0;     // zero padding
    const uint64_t src = sampled ? sampled_src(len, q) : (uint64_t)(q - 8);
    const uint32_t left = msg_len - q;
    return load8(units, data_off + src, left < 8 ? left : 8);
}

__global__ __launch_bounds__(256) void k_cas_gather(const uint8_t* __restrict__ data,
                                                    const gather_row* __restrict__ rows,
                                                    const uint32_t* __restrict__ tile_first, uint64_t total_units,
                                                    uint8_t* __restrict__ staged) {
    const uint4* units = reinterpret_cast<const uint4*>(data);
    const uint32_t f_lo = tile_first[blockIdx.x], f_hi = tile_first[blockIdx.x + 1];
    for (uint32_t k = 0; k < SD_GATHER_TILE_UNITS / 256; k++) {
        const uint64_t g = (uint64_t)blockIdx.x * SD_GATHER_TILE_UNITS + k * 256 + threadIdx.x;
        if (g >= total_units) return;
        uint32_t lo = f_lo, hi = f_hi;  // the last file whose first unit is <= g
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (rows[mid].unit0 <= g) lo = mid;
            else hi = mid - 1;
        }
        const gather_row r = rows[lo];
        const bool sampled = r.len > SD_MINIMUM_FILE_SIZE;  // cas.rs:27
        const uint32_t msg_len = sampled ? SD_SAMPLED_MSG_LEN : (uint32_t)(8 + r.len);
        const uint32_t q = (uint32_t)(g - r.unit0) * 16;    // < the padded message length
        const uint64_t a = msg8(units, r.data_off, r.len, sampled, msg_len, q);
        const uint64_t b = msg8(units, r.data_off, r.len, sampled, msg_len, q + 8);
        uint4 v;
        v.x = (uint32_t)a;
        v.y = (uint32_t)(a >> 32);
        v.z = (uint32_t)b;
        v.w = (uint32_t)(b >> 32);
        *reinterpret_cast<uint4*>(staged + r.msg_off + q) = v;
    }
}

}  // namespace

namespace sdk {

hipError_t launch_cas_gather(const uint8_t* data, const gather_row* rows, const uint32_t* tile_first,
                             uint64_t total_units, uint8_t* staged, hipStream_t s) {
    if (total_units == 0) return hipSuccess;
    const uint64_t tiles = (total_units + SD_GATHER_TILE_UNITS - 1) / SD_GATHER_TILE_UNITS;
    if (tiles >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cas_gather, dim3((uint32_t)tiles), dim3(256), 0, s, data, rows, tile_first, total_units,
                       staged);
    return hipGetLastError();
}

}  // namespace sdk
