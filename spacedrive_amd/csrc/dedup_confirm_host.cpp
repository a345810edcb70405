// dedup_confirm_host.cpp -- the GPU-free sibling of sd_dedup_confirm (include/sd_cas.h):
// sd_cpu_dedup_confirm over host arrays, with the device call's semantics.
//
// Reference: a cas_id samples files over 100 KiB (core/src/object/cas.rs:30-58), so the files
// of one cas_id are candidates; file_checksum (core/src/object/validation/hash.rs:10-24) hashes
// every byte, and equal checksums confirm.  The valid positions are sorted by (key, the 32 bytes
// as memcmp compares them, position); classes and groups are runs of that order.  No HIP: built
// with g++ under the sanitizers too (dedup_confirm_selftest.cpp, `make sanitize-dedup-confirm`).
#include <string.h>

#include <algorithm>
#include <vector>

#include "sd_host.h"

extern "C" int sd_cpu_dedup_confirm(const uint64_t* keys, const uint8_t* hash32, const uint8_t* valid, uint64_t m,
                                    uint64_t* rep, uint64_t* class_size, uint8_t* verdict, uint64_t* sets_out,
                                    uint64_t capacity, uint64_t* n_sets, uint64_t stats[8]) {
    SD_GUARD_BEGIN
    if (m && (!keys || !hash32)) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (n_sets) *n_sets = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    std::vector<uint64_t> order;
    order.reserve(m);
    for (uint64_t i = 0; i < m; i++) {
        if (!valid || valid[i]) {
            order.push_back(i);
            continue;
        }
        if (rep) rep[i] = ~0ull;
        if (class_size) class_size[i] = 0;
        if (verdict) verdict[i] = SD_CONFIRM_INVALID;
    }
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (keys[a] != keys[b]) return keys[a] < keys[b];
        const int c = memcmp(hash32 + 32 * a, hash32 + 32 * b, 32);
        return c != 0 ? c < 0 : a < b;
    });
    const size_t v = order.size();
    uint64_t st[8] = {v, 0, 0, 0, 0, 0, 0, 0};
    struct set_row { uint64_t key, rep, size; };
    std::vector<set_row> rows;
    for (size_t g0 = 0; g0 < v;) {  // one group: [g0, g1)
        size_t g1 = g0 + 1;
        while (g1 < v && keys[order[g1]] == keys[order[g0]]) g1++;
        const uint64_t gsize = g1 - g0;
        uint64_t nclasses = 0;
        for (size_t c0 = g0; c0 < g1;) {  // one class: [c0, c1)
            size_t c1 = c0 + 1;
            while (c1 < g1 && memcmp(hash32 + 32 * order[c1], hash32 + 32 * order[c0], 32) == 0) c1++;
            const uint64_t csize = c1 - c0;
            const uint8_t vd = gsize == 1 ? SD_CONFIRM_SINGLE : csize >= 2 ? SD_CONFIRM_CONFIRMED : SD_CONFIRM_REFUTED;
            for (size_t k = c0; k < c1; k++) {
                const uint64_t i = order[k];
                if (rep) rep[i] = order[c0];  // positions ascend inside a class
                if (class_size) class_size[i] = csize;
                if (verdict) verdict[i] = vd;
            }
            nclasses++;
            if (csize >= 2) {
                st[4]++;
                st[5] += csize;
                rows.push_back({keys[order[c0]], order[c0], csize});
            } else if (gsize >= 2) {
                st[6]++;
            }
            c0 = c1;
        }
        st[1]++;
        st[3] += nclasses;
        if (gsize >= 2) {
            st[2]++;
            if (nclasses >= 2) st[7]++;
        }
        g0 = g1;
    }
    if (n_sets) *n_sets = rows.size();
    if (stats) memcpy(stats, st, sizeof st);
    if (sets_out) {
        if (capacity < rows.size()) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of sets");
        for (size_t r = 0; r < rows.size(); r++) {
            sets_out[3 * r] = rows[r].key;
            sets_out[3 * r + 1] = rows[r].rep;
            sets_out[3 * r + 2] = rows[r].size;
        }
    }
    return SD_OK;
    SD_GUARD_END
}
