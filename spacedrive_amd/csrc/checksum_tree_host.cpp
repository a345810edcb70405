// checksum_tree_host.cpp -- the GPU-free half of the checksum trees (include/sd_cas.h): the node
// count and batch layout, and sd_cpu_checksum_tree / _roots / _verify over host memory with the
// device calls' semantics.
//
// A node is what the CPU hasher already computes for the split checksum: CpuHasher(chunk0) over
// the block's bytes, finalize_cv -- a block's CV depends only on its bytes and its position.  A
// file of one node is hashed whole (ROOT), and a level's root is cpu_root_from_cvs over it.  No
// HIP: built with g++ under the sanitizers too (checksum_tree_selftest.cpp).
#include <string.h>

#include <algorithm>
#include <vector>

#include "sd_host.h"

void plan_tree_layout(const uint64_t* lens, size_t n, uint32_t block_log2, std::vector<uint64_t>& node_base) {
    if (block_log2 < SD_TREE_BLOCK_LOG2_MIN || block_log2 > SD_TREE_BLOCK_LOG2_MAX)
        throw sd_failure(SD_ERR_INVALID, "block_log2 " + std::to_string(block_log2) + " outside [17, 20]");
    node_base.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) node_base[i + 1] = node_base[i] + tree_nodes(lens[i], block_log2);
}

namespace {

void check_ranges(const uint64_t* offsets, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (offsets[i] % 16) throw sd_failure(SD_ERR_INVALID, "checksum range " + std::to_string(i) + " not 16-byte aligned");
}

// every file's level -> nodes (laid out by node_base), one task per node
void cpu_tree_nodes(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n, uint32_t k,
                    const std::vector<uint64_t>& node_base, uint8_t* nodes, int nthreads) {
    struct Task { size_t file; uint64_t block; };
    std::vector<Task> tasks;
    tasks.reserve(node_base[n]);
    for (size_t i = 0; i < n; i++)
        for (uint64_t j = 0; j < node_base[i + 1] - node_base[i]; j++) tasks.push_back({i, j});
    const uint64_t B = 1ull << k;
    cpu_parallel_for(tasks.size(), nthreads, [&](size_t t) {
        const size_t i = tasks[t].file;
        const uint64_t j = tasks[t].block;
        uint8_t* out = nodes + 32 * (node_base[i] + j);
        if (node_base[i + 1] - node_base[i] == 1) {  // the file is this block: its root hash
            cpu_blake3(data + offsets[i], lens[i], out);
            return;
        }
        CpuHasher h(j * (B / 1024));
        h.update(data + offsets[i] + j * B, std::min<uint64_t>(B, lens[i] - j * B));
        h.finalize_cv(out);
    });
}

void cpu_tree_roots(const uint8_t* nodes, size_t n, const std::vector<uint64_t>& node_base, uint8_t* hash32) {
    for (size_t i = 0; i < n; i++) {
        const uint64_t nb = node_base[i + 1] - node_base[i];
        if (nb == 1) memcpy(hash32 + 32 * i, nodes + 32 * node_base[i], 32);
        else cpu_root_from_cvs(nodes + 32 * node_base[i], nb, hash32 + 32 * i);
    }
}

}  // namespace

extern "C" {

int sd_checksum_tree_nodes(uint64_t len, uint32_t block_log2, uint64_t* n_nodes) {
    SD_GUARD_BEGIN
    if (!n_nodes) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> nb;
    plan_tree_layout(&len, 1, block_log2, nb);
    *n_nodes = nb[1];
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                         uint32_t block_log2, uint8_t* nodes, uint8_t* hash32, int nthreads) {
    SD_GUARD_BEGIN
    if (n && (!data || !offsets || !lens || !nodes || !hash32)) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n, block_log2, node_base);
    check_ranges(offsets, n);
    cpu_tree_nodes(data, offsets, lens, n, block_log2, node_base, nodes, nthreads);
    cpu_tree_roots(nodes, n, node_base, hash32);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_roots(const uint8_t* nodes, const uint64_t* lens, size_t n, uint32_t block_log2,
                               uint8_t* hash32) {
    SD_GUARD_BEGIN
    if (n && (!nodes || !lens || !hash32)) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n, block_log2, node_base);
    cpu_tree_roots(nodes, n, node_base, hash32);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_verify(const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                                uint32_t block_log2, const uint8_t* expected, uint8_t* bad, uint64_t* rows_out,
                                uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads) {
    SD_GUARD_BEGIN
    if (n && (!data || !offsets || !lens || !expected)) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n, block_log2, node_base);
    check_ranges(offsets, n);
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    std::vector<uint8_t> nodes(32 * node_base[n]);
    cpu_tree_nodes(data, offsets, lens, n, block_log2, node_base, nodes.data(), nthreads);
    uint64_t st[4] = {n, node_base[n], 0, 0};
    for (size_t i = 0; i < n; i++) {
        bool any = false;
        for (uint64_t q = node_base[i]; q < node_base[i + 1]; q++) {
            const bool differs = memcmp(nodes.data() + 32 * q, expected + 32 * q, 32) != 0;
            if (bad) bad[q] = differs ? 1 : 0;
            st[2] += differs;
            any |= differs;
        }
        st[3] += any;
    }
    if (count) *count = st[2];
    if (stats) memcpy(stats, st, sizeof st);
    if (rows_out) {
        if (capacity < st[2]) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing blocks");
        uint64_t r = 0;
        for (size_t i = 0; i < n; i++)
            for (uint64_t q = node_base[i]; q < node_base[i + 1]; q++)
                if (memcmp(nodes.data() + 32 * q, expected + 32 * q, 32) != 0) {
                    rows_out[2 * r] = i;
                    rows_out[2 * r + 1] = q - node_base[i];
                    r++;
                }
    }
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
