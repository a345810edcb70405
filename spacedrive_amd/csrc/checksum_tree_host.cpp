// checksum_tree_host.cpp -- the GPU-free half of the checksum trees (include/sd_cas.h): the node
// count and batch layout, and sd_cpu_checksum_tree / _roots / _verify over host memory with the
// device calls' semantics.
//
// A node is what the CPU hasher already computes for the split checksum: CpuHasher(chunk0) over
// the block's bytes, finalize_cv -- a block's CV depends only on its bytes and its position.  A
// file of one node is hashed whole (ROOT), and a level's root is cpu_root_from_cvs over it.  The
// listed blocks (sd_cpu_checksum_tree_blocks / _verify / _update) are the same two hashers over
// the items plan_tree_blocks makes, which the device list uses too.  No HIP: built with g++ under
// the sanitizers too (checksum_tree_selftest.cpp).
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

void plan_tree_blocks(TreeBlocksPlan& p, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                      const uint64_t* rows, const uint64_t* data_offsets, size_t m) {
    if (block_log2 < SD_TREE_BLOCK_LOG2_MIN || block_log2 > SD_TREE_BLOCK_LOG2_MAX)
        throw sd_failure(SD_ERR_INVALID, "block_log2 " + std::to_string(block_log2) + " outside [17, 20]");
    const uint64_t B = 1ull << block_log2;
    for (size_t r = 0; r < m; r++) {  // everything refused before anything is allocated
        const uint64_t f = rows[2 * r], j = rows[2 * r + 1];
        if (f >= n_files) throw sd_failure(SD_ERR_INVALID, "block row " + std::to_string(r) + ": no such file");
        if (j >= tree_nodes(lens[f], block_log2))
            throw sd_failure(SD_ERR_INVALID, "block row " + std::to_string(r) + ": no such block");
        if (data_offsets[r] % 16)
            throw sd_failure(SD_ERR_INVALID, "block row " + std::to_string(r) + " not 16-byte aligned");
    }
    plan_tree_layout(lens, n_files, block_log2, p.node_base);
    p.items.resize(m);
    p.bytes = p.compressions = 0;
    for (size_t r = 0; r < m; r++) {
        const uint64_t f = rows[2 * r], j = rows[2 * r + 1];
        ck_block_item& it = p.items[r];
        it.src = data_offsets[r];
        it.chunk0 = j * (B / 1024);
        it.len = (uint32_t)(lens[f] == 0 ? 0 : std::min<uint64_t>(B, lens[f] - j * B));
        it.root = p.node_base[f + 1] - p.node_base[f] == 1;
        it.dst = p.node_base[f] + j;
        p.bytes += it.len;
        p.compressions += msg_compressions(it.len);
    }
    std::vector<uint64_t> slots(m);
    for (size_t r = 0; r < m; r++) slots[r] = p.items[r].dst;
    std::sort(slots.begin(), slots.end());
    p.repeats = std::adjacent_find(slots.begin(), slots.end()) != slots.end();
}

namespace {

// the items' nodes -> out + 32 * (scatter ? the item's level slot : its row), one task per item
void cpu_block_nodes(const uint8_t* data, const TreeBlocksPlan& p, bool scatter, uint8_t* out, int nthreads) {
    cpu_parallel_for(p.items.size(), nthreads, [&](size_t r) {
        const ck_block_item& it = p.items[r];
        uint8_t* o = out + 32 * (scatter ? it.dst : (uint64_t)r);
        if (it.root) {  // the file is this block: its root hash
            cpu_blake3(data + it.src, it.len, o);
            return;
        }
        CpuHasher h(it.chunk0);
        h.update(data + it.src, it.len);
        h.finalize_cv(o);
    });
}

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

int sd_cpu_checksum_tree_blocks(const uint8_t* data, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                const uint64_t* rows, const uint64_t* data_offsets, size_t m, uint8_t* nodes_out,
                                int nthreads) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!data || !rows || !data_offsets || !nodes_out)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    TreeBlocksPlan p;
    plan_tree_blocks(p, lens, n_files, block_log2, rows, data_offsets, m);
    cpu_block_nodes(data, p, false, nodes_out, nthreads);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_verify(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                       uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                       size_t m, const uint8_t* expected, uint8_t* bad, uint64_t* rows_out,
                                       uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!data || !rows || !data_offsets || !expected)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    TreeBlocksPlan p;
    plan_tree_blocks(p, lens, n_files, block_log2, rows, data_offsets, m);
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (m == 0) return SD_OK;
    std::vector<uint8_t> nodes(32 * m);
    cpu_block_nodes(data, p, false, nodes.data(), nthreads);
    std::vector<uint8_t> differs(m), file_bad(n_files, 0);
    uint64_t st[4] = {n_files, m, 0, 0};
    for (size_t r = 0; r < m; r++) {
        differs[r] = memcmp(nodes.data() + 32 * r, expected + 32 * p.items[r].dst, 32) != 0;
        if (bad) bad[r] = differs[r];
        st[2] += differs[r];
        if (differs[r] && !file_bad[rows[2 * r]]) file_bad[rows[2 * r]] = 1, st[3]++;
    }
    if (count) *count = st[2];
    if (stats) memcpy(stats, st, sizeof st);
    if (rows_out) {
        if (capacity < st[2]) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing rows");
        uint64_t q = 0;
        for (size_t r = 0; r < m; r++)
            if (differs[r]) rows_out[2 * q] = rows[2 * r], rows_out[2 * q + 1] = rows[2 * r + 1], q++;
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_update(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                       uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                       size_t m, uint8_t* nodes, uint8_t* hash32, int nthreads) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!data || !rows || !data_offsets || !nodes || !hash32)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    TreeBlocksPlan p;
    plan_tree_blocks(p, lens, n_files, block_log2, rows, data_offsets, m);
    if (p.repeats) throw sd_failure(SD_ERR_INVALID, "a (file, block) is listed twice: two writers of one node");
    if (m == 0) return SD_OK;
    cpu_block_nodes(data, p, true, nodes, nthreads);
    cpu_tree_roots(nodes, n_files, p.node_base, hash32);
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
