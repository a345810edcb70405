// fingerprint_host.cpp -- the GPU-free half of the fingerprint entry points (include/sd_cas.h):
// the gather planner, the cas message of a file already in memory, and sd_cpu_fingerprints.
//
// A fingerprint is what the watcher's inner_update_file computes for one file
// (core/src/location/manager/watcher/utils.rs:393 generate_cas_id, :438-446 file_checksum):
// here both come from one copy of the file's bytes.  No HIP: built with g++ under the
// sanitizers too (fingerprint_selftest.cpp, `make sanitize-fingerprint`).
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "sd_host.h"

void plan_gather(GatherPlan& p, const uint64_t* offsets, const uint64_t* lens, size_t n) {
    if (n >= (1ull << 31)) throw sd_failure(SD_ERR_INVALID, "batch too large");
    p.extents.resize(n);
    p.rows.resize(n + 1);
    p.tile_first.clear();
    p.units = p.staged_bytes = p.file_bytes = p.read_bytes = 0;
    p.n_sampled = p.n_whole = 0;
    uint64_t off = 0, units = 0;
    for (size_t i = 0; i < n; i++) {
        if (offsets[i] % 16) throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + " not 16-byte aligned");
        const sd_extent e = plan_extent(lens[i], off);
        p.extents[i] = e;
        const uint64_t padded = sd_align_up(e.msg_len, SD_STAGE_ALIGN);
        p.rows[i] = gather_row{offsets[i], e.msg_offset, lens[i], units};
        // tiles that begin inside this file's units: it is the first file they touch
        while ((uint64_t)p.tile_first.size() * SD_GATHER_TILE_UNITS < units + padded / 16)
            p.tile_first.push_back((uint32_t)i);
        units += padded / 16;
        off += padded;
        p.file_bytes += lens[i];
        p.read_bytes += e.msg_len - 8;
        if (e.kind == SD_KIND_SAMPLED) p.n_sampled++;
        else p.n_whole++;
    }
    p.rows[n] = gather_row{0, off, 0, units};
    p.tile_first.push_back(n ? (uint32_t)(n - 1) : 0);  // the last tile's upper bound
    p.units = units;
    p.staged_bytes = off;
}

uint32_t cas_message_from_bytes(const uint8_t* file, uint64_t len, uint8_t* out) {
    for (int k = 0; k < 8; k++) out[k] = (uint8_t)(len >> (8 * k));  // cas.rs:25 size.to_le_bytes()
    if (len <= SD_MINIMUM_FILE_SIZE) {                                // cas.rs:27-29
        if (len) memcpy(out + 8, file, len);
        return (uint32_t)(8 + len);
    }
    const uint64_t H = SD_HEADER_OR_FOOTER_SIZE, S = SD_SAMPLE_SIZE;
    const uint64_t jump = (len - 2 * H) / SD_SAMPLE_COUNT;  // cas.rs:33
    uint8_t* q = out + 8;
    memcpy(q, file, H);  // cas.rs:35-37 header
    q += H;
    for (uint64_t k = 0; k < SD_SAMPLE_COUNT; k++, q += S) memcpy(q, file + H + k * jump, S);  // cas.rs:41-49
    memcpy(q, file + len - H, H);  // cas.rs:52-57 footer at End(-8192)
    return SD_SAMPLED_MSG_LEN;
}

extern "C" {

int sd_cpu_fingerprints(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n, char* out_hex17,
                        char* out_hex65, int nthreads) {
    SD_GUARD_BEGIN
    if (n && (!data || !offsets || !lens || !out_hex17 || !out_hex65)) throw sd_failure(SD_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n; i++)
        if (offsets[i] % 16) throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + " not 16-byte aligned");
    if (n == 0) return SD_OK;
    // checksums: the family's own entry (a range of 8 MiB or more block-parallel)
    std::vector<uint8_t> h32(32 * n);
    const int rc = sd_cpu_checksums(data, offsets, lens, n, h32.data(), cap_host_threads(nthreads));
    if (rc != SD_OK) return rc;
    for (size_t i = 0; i < n; i++) hex_lower(h32.data() + 32 * i, 32, out_hex65 + 65 * i);
    // cas ids: each thread builds a file's message in its own buffer and hashes it
    int threads = cap_host_threads(nthreads);
    if ((size_t)threads > n) threads = (int)n;
    std::atomic<size_t> cursor{0};
    std::atomic<bool> failed{false};
    auto work = [&] {
        try {
            std::vector<uint8_t> msg(8 + SD_MINIMUM_FILE_SIZE);
            uint8_t h[32];
            for (;;) {
                const size_t i = cursor.fetch_add(1, std::memory_order_relaxed);
                if (i >= n) break;
                const uint32_t ml = cas_message_from_bytes(data + offsets[i], lens[i], msg.data());
                cpu_blake3(msg.data(), ml, h);
                hex_lower(h, 8, out_hex17 + 17 * i);  // cas.rs:61 to_hex()[..16]
            }
        } catch (...) {
            failed.store(true);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; t++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    if (failed.load()) throw sd_failure(SD_ERR_NOMEM, "host allocation failed");
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
