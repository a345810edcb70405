// cdc_host.cpp -- the GPU-free half of the content-defined chunks (include/sd_cas.h, "content-defined
// chunks"): the gear table, the parameter and range rules both halves share, and the host twins
// sd_cpu_cdc_cut, sd_cpu_cdc_hash and sd_cpu_cdc_shared with the device calls' semantics.
//
// The cut is one pass per file: the rolling value is carried from byte to byte (h <- (h << 1) +
// G[byte]; what a byte added has left the 64 bits after 64 steps, so no reset and no window are
// needed), and a chunk ends at the first candidate at or after s + min_size or at s + max_size.
// Files run in parallel, a file is serial.  The ids are the library's CPU BLAKE3 of each chunk as a
// message of its own.  The shared report sorts the slots by (length, the 32 id bytes as memcmp
// compares them, slot): classes are runs of that order, a class's representative the slot at its
// head.  No HIP: built with g++ under the sanitizers too (cdc_selftest.cpp, `make sanitize-cdc`).
#include <string.h>

#include <algorithm>
#include <vector>

#include "sd_host.h"

namespace {

uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct GearTable {
    uint64_t g[256];
    GearTable() {
        for (uint64_t b = 0; b < 256; b++) g[b] = splitmix64(0x5DCDC0DEull ^ b);
    }
};

struct FileCut {
    std::vector<uint64_t> ends;  // the chunk ends of one file, ascending; the last one is len
    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void cut_file(const uint8_t* p, uint64_t len, const sd_cdc_params& pr, FileCut& out) {
    const uint64_t* G = cdc_gear();
    const uint64_t mask = ((1ull << pr.mask_bits) - 1) << (64 - pr.mask_bits);
    uint64_t h = 0, s = 0;
    for (uint64_t i = 0; i < len; i++) {
        h = (h << 1) + G[p[i]];
        const bool cand = (h & mask) == 0;
        out.st[2] += cand;
        const uint64_t e = i + 1;
        if (!((cand && e - s >= pr.min_size) || e - s == pr.max_size)) continue;
        out.ends.push_back(e);
        out.st[e == len ? 6 : cand ? 4 : 5]++;
        s = e;
    }
    if (s < len || len == 0) {
        out.ends.push_back(len);
        out.st[6]++;
    }
    out.st[3] = out.ends.size();
}

}  // namespace

const uint64_t* cdc_gear() {
    static const GearTable t;
    return t.g;
}

void cdc_check_params(const sd_cdc_params* p) {
    if (!p) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (p->mask_bits < 1 || p->mask_bits > 32) throw sd_failure(SD_ERR_INVALID, "mask_bits outside 1..32");
    if (p->min_size < 64 || p->min_size > p->max_size || p->max_size > (1u << 20))
        throw sd_failure(SD_ERR_INVALID, "64 <= min_size <= max_size <= 1 MiB does not hold");
    if (p->reserved != 0) throw sd_failure(SD_ERR_INVALID, "reserved is not 0");
}

uint64_t cdc_check_ranges(const uint64_t* offsets, const uint64_t* lens, size_t n, const sd_cdc_params& p) {
    if (n && (!offsets || !lens)) throw sd_failure(SD_ERR_INVALID, "null argument");
    uint64_t bytes = 0, bound = n;
    for (size_t f = 0; f < n; f++) {
        if (offsets[f] % 16) throw sd_failure(SD_ERR_INVALID, "a range does not start 16-byte aligned");
        if (lens[f] > (1ull << 62) || bytes + lens[f] < bytes) throw sd_failure(SD_ERR_INVALID, "a range is too long");
        bytes += lens[f];
        bound += (lens[f] + p.min_size - 1) / p.min_size;
        if (bound >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "too many chunks: ceil(len / min_size) + n >= 2^32");
    }
    return bytes;
}

uint64_t cdc_check_layout(const uint64_t* chunk_base, size_t n) {
    if ((uint64_t)n >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "too many files");
    if (n == 0) return 0;
    if (!chunk_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (chunk_base[0] != 0) throw sd_failure(SD_ERR_INVALID, "chunk_base does not start at 0");
    for (size_t f = 0; f < n; f++)
        if (chunk_base[f + 1] <= chunk_base[f]) throw sd_failure(SD_ERR_INVALID, "a file without a chunk");
    return chunk_base[n];
}

extern "C" int sd_cdc_gear(uint64_t out[256]) {
    SD_GUARD_BEGIN
    if (!out) throw sd_failure(SD_ERR_INVALID, "null argument");
    memcpy(out, cdc_gear(), 256 * sizeof(uint64_t));
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cpu_cdc_cut(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                              const sd_cdc_params* params, uint64_t* chunk_base, uint64_t* chunks_out,
                              uint64_t capacity, uint64_t* n_chunks, uint64_t stats[8], int nthreads) {
    SD_GUARD_BEGIN
    cdc_check_params(params);
    const uint64_t bytes = cdc_check_ranges(offsets, lens, n, *params);
    if (bytes && !data) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (n_chunks) *n_chunks = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (chunk_base) chunk_base[0] = 0;
    if (n == 0) return SD_OK;
    std::vector<FileCut> cuts(n);
    cpu_parallel_for(n, nthreads, [&](size_t f) { cut_file(data + offsets[f], lens[f], *params, cuts[f]); });
    uint64_t st[8] = {n, bytes, 0, 0, 0, 0, 0, 0}, total = 0;
    for (size_t f = 0; f < n; f++) {
        for (int k = 2; k < 7; k++) st[k] += cuts[f].st[k];
        uint64_t s = 0;
        for (uint64_t e : cuts[f].ends) st[7] += cdc_compressions(e - s), s = e;
        total += cuts[f].ends.size();
        if (chunk_base) chunk_base[f + 1] = total;
    }
    if (n_chunks) *n_chunks = total;
    if (stats) memcpy(stats, st, sizeof st);
    if (!chunks_out) return SD_OK;
    if (capacity < total) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of chunks");
    uint64_t c = 0;
    for (size_t f = 0; f < n; f++) {
        uint64_t s = 0;
        for (uint64_t e : cuts[f].ends) {
            chunks_out[2 * c] = s;
            chunks_out[2 * c + 1] = e - s;
            c++, s = e;
        }
    }
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cpu_cdc_hash(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                               const uint64_t* chunk_base, const uint64_t* chunks, uint8_t* ids_out, int nthreads) {
    SD_GUARD_BEGIN
    if (n && (!offsets || !lens)) throw sd_failure(SD_ERR_INVALID, "null argument");
    const uint64_t m = cdc_check_layout(chunk_base, n);
    if (m && (!chunks || !ids_out)) throw sd_failure(SD_ERR_INVALID, "null argument");
    uint64_t bytes = 0;
    for (size_t f = 0; f < n; f++) {
        for (uint64_t c = chunk_base[f]; c < chunk_base[f + 1]; c++)
            if (chunks[2 * c] > lens[f] || chunks[2 * c + 1] > lens[f] - chunks[2 * c])
                throw sd_failure(SD_ERR_INVALID, "a chunk lies outside its file");
        bytes += lens[f];
    }
    if (bytes && !data) throw sd_failure(SD_ERR_INVALID, "null argument");
    // a file's chunks are hashed by one task when there are many files, else one chunk per task
    if (n >= 64) {
        cpu_parallel_for(n, nthreads, [&](size_t f) {
            for (uint64_t c = chunk_base[f]; c < chunk_base[f + 1]; c++)
                cpu_blake3(data + offsets[f] + chunks[2 * c], chunks[2 * c + 1], ids_out + 32 * c);
        });
        return SD_OK;
    }
    std::vector<uint32_t> file_of(m);
    for (size_t f = 0; f < n; f++)
        for (uint64_t c = chunk_base[f]; c < chunk_base[f + 1]; c++) file_of[c] = (uint32_t)f;
    cpu_parallel_for(m, nthreads, [&](size_t c) {
        cpu_blake3(data + offsets[file_of[c]] + chunks[2 * c], chunks[2 * c + 1], ids_out + 32 * c);
    });
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cpu_cdc_shared(const uint64_t* chunk_base, size_t n, const uint64_t* chunks, const uint8_t* ids,
                                 uint64_t min_chunks, uint64_t* rep, uint64_t* class_size, uint64_t* files_out,
                                 uint64_t* pairs_out, uint64_t capacity, uint64_t* n_pairs, uint64_t stats[8]) {
    SD_GUARD_BEGIN
    const uint64_t m = cdc_check_layout(chunk_base, n);
    if (m && (!chunks || !ids)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (n_pairs) *n_pairs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0) return SD_OK;

    std::vector<uint32_t> file_of(m);
    for (size_t f = 0; f < n; f++)
        for (uint64_t s = chunk_base[f]; s < chunk_base[f + 1]; s++) file_of[s] = (uint32_t)f;
    auto len_of = [&](uint64_t s) { return chunks[2 * s + 1]; };
    std::vector<uint64_t> order(m);
    for (uint64_t s = 0; s < m; s++) order[s] = s;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (len_of(a) != len_of(b)) return len_of(a) < len_of(b);
        const int c = memcmp(ids + 32 * a, ids + 32 * b, 32);
        return c != 0 ? c < 0 : a < b;
    });
    std::vector<uint64_t> rp(m), cs(m);
    uint64_t st[8] = {n, m, 0, 0, 0, 0, 0, 0};
    for (uint64_t c0 = 0; c0 < m;) {  // one class: [c0, c1), slots ascending inside it
        uint64_t c1 = c0 + 1;
        while (c1 < m && len_of(order[c1]) == len_of(order[c0]) && memcmp(ids + 32 * order[c1], ids + 32 * order[c0], 32) == 0)
            c1++;
        for (uint64_t k = c0; k < c1; k++) rp[order[k]] = order[c0], cs[order[k]] = c1 - c0;
        st[2]++;
        st[3] += c1 - c0 >= 2;
        c0 = c1;
    }
    if (rep) memcpy(rep, rp.data(), m * sizeof(uint64_t));
    if (class_size) memcpy(class_size, cs.data(), m * sizeof(uint64_t));

    struct row { uint64_t f, g, chunks, bytes; };
    std::vector<row> rows;
    const uint64_t need = std::max<uint64_t>(1, min_chunks);
    std::vector<std::pair<uint64_t, uint64_t>> red;  // (g, bytes) of one file's redundant slots held by an earlier file
    for (size_t f = 0; f < n; f++) {
        uint64_t shared = 0, nred = 0, rbytes = 0;
        red.clear();
        for (uint64_t s = chunk_base[f]; s < chunk_base[f + 1]; s++) {
            shared += cs[s] >= 2;
            if (rp[s] == s) continue;
            nred++;
            rbytes += len_of(s);
            if (file_of[rp[s]] == f) st[7]++;  // repeated inside the file: no row
            else red.emplace_back(file_of[rp[s]], len_of(s));
        }
        if (files_out) {
            files_out[4 * f] = chunk_base[f + 1] - chunk_base[f];
            files_out[4 * f + 1] = shared;
            files_out[4 * f + 2] = nred;
            files_out[4 * f + 3] = rbytes;
        }
        st[4] += nred;
        st[5] += rbytes;
        st[6] += nred != 0;
        std::sort(red.begin(), red.end());
        for (size_t a = 0; a < red.size();) {
            size_t b = a;
            uint64_t bytes = 0;
            for (; b < red.size() && red[b].first == red[a].first; b++) bytes += red[b].second;
            if (b - a >= need) rows.push_back({f, red[a].first, b - a, bytes});
            a = b;
        }
    }
    if (n_pairs) *n_pairs = rows.size();
    if (stats) memcpy(stats, st, sizeof st);
    if (pairs_out) {
        if (capacity < rows.size()) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of pairs");
        for (size_t r = 0; r < rows.size(); r++) {
            pairs_out[4 * r] = rows[r].f;
            pairs_out[4 * r + 1] = rows[r].g;
            pairs_out[4 * r + 2] = rows[r].chunks;
            pairs_out[4 * r + 3] = rows[r].bytes;
        }
    }
    return SD_OK;
    SD_GUARD_END
}
