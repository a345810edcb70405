// tree_shared_host.cpp -- the GPU-free sibling of sd_checksum_tree_shared (include/sd_cas.h,
// "shared blocks"): sd_cpu_checksum_tree_shared over host arrays, with the device call's semantics.
//
// A full block's node depends on its bytes and its index only (the position rule of the checksum
// trees), so two files hold the same bytes in block j exactly when their level nodes at j are equal.
// The slots are sorted by (block index, the 32 node bytes as memcmp compares them, slot); classes
// are runs of that order, a class's representative the slot at its head.  One pass over the slots in
// file order then gives the per-file rows and, per file, the redundant slots by the file of their
// representative.  No HIP: built with g++ under the sanitizers too (tree_shared_selftest.cpp,
// `make sanitize-tree-shared`).
#include <string.h>

#include <algorithm>
#include <vector>

#include "sd_host.h"

extern "C" int sd_cpu_checksum_tree_shared(const uint64_t* lens, size_t n, uint32_t block_log2, const uint8_t* nodes,
                                           uint64_t min_blocks, uint64_t* rep, uint64_t* class_size,
                                           uint64_t* files_out, uint64_t* pairs_out, uint64_t capacity,
                                           uint64_t* n_pairs, uint64_t stats[8]) {
    SD_GUARD_BEGIN
    if (n && !lens) throw sd_failure(SD_ERR_INVALID, "null argument");
    if ((uint64_t)n >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "too many files");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n, block_log2, node_base);
    const uint64_t m = node_base[n], B = 1ull << block_log2;
    if (m && !nodes) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (n_pairs) *n_pairs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0) return SD_OK;

    std::vector<uint32_t> file_of(m);
    for (size_t f = 0; f < n; f++)
        for (uint64_t s = node_base[f]; s < node_base[f + 1]; s++) file_of[s] = (uint32_t)f;
    auto block_of = [&](uint64_t s) { return s - node_base[file_of[s]]; };
    std::vector<uint64_t> order(m);
    for (uint64_t s = 0; s < m; s++) order[s] = s;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        const uint64_t ja = block_of(a), jb = block_of(b);
        if (ja != jb) return ja < jb;
        const int c = memcmp(nodes + 32 * a, nodes + 32 * b, 32);
        return c != 0 ? c < 0 : a < b;
    });
    std::vector<uint64_t> rp(m), cs(m);
    uint64_t st[8] = {n, m, 0, 0, 0, 0, 0, 0};
    for (uint64_t c0 = 0; c0 < m;) {  // one class: [c0, c1), slots ascending inside it
        uint64_t c1 = c0 + 1;
        while (c1 < m && block_of(order[c1]) == block_of(order[c0]) &&
               memcmp(nodes + 32 * order[c1], nodes + 32 * order[c0], 32) == 0)
            c1++;
        for (uint64_t k = c0; k < c1; k++) rp[order[k]] = order[c0], cs[order[k]] = c1 - c0;
        st[2]++;
        st[3] += c1 - c0 >= 2;
        c0 = c1;
    }
    if (rep) memcpy(rep, rp.data(), m * sizeof(uint64_t));
    if (class_size) memcpy(class_size, cs.data(), m * sizeof(uint64_t));

    struct row { uint64_t f, g, blocks, bytes; };
    std::vector<row> rows;
    const uint64_t need = std::max<uint64_t>(1, min_blocks);
    std::vector<std::pair<uint64_t, uint64_t>> red;  // (g, bytes) of one file's redundant slots
    for (size_t f = 0; f < n; f++) {
        uint64_t shared = 0, rbytes = 0;
        red.clear();
        for (uint64_t s = node_base[f]; s < node_base[f + 1]; s++) {
            shared += cs[s] >= 2;
            if (rp[s] == s) continue;
            const uint64_t at = (s - node_base[f]) * B;  // an empty file's one slot: 0 bytes
            const uint64_t bytes = lens[f] > at ? std::min<uint64_t>(B, lens[f] - at) : 0;
            red.emplace_back(file_of[rp[s]], bytes);
            rbytes += bytes;
        }
        if (files_out) {
            files_out[4 * f] = node_base[f + 1] - node_base[f];
            files_out[4 * f + 1] = shared;
            files_out[4 * f + 2] = red.size();
            files_out[4 * f + 3] = rbytes;
        }
        st[4] += red.size();
        st[5] += rbytes;
        st[6] += !red.empty();
        st[7] += red.size() == node_base[f + 1] - node_base[f];
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
            pairs_out[4 * r + 2] = rows[r].blocks;
            pairs_out[4 * r + 3] = rows[r].bytes;
        }
    }
    return SD_OK;
    SD_GUARD_END
}
