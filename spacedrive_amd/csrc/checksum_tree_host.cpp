// checksum_tree_host.cpp -- the GPU-free half of the checksum trees (include/sd_cas.h): the node
// count and batch layout, and sd_cpu_checksum_tree / _roots / _verify over host memory with the
// device calls' semantics.
//
// A node is what the CPU hasher already computes for the split checksum: CpuHasher(chunk0) over
// the block's bytes, finalize_cv -- a block's CV depends only on its bytes and its position.  A
// file of one node is hashed whole (ROOT), and a level's root is cpu_root_from_cvs over it.  The
// listed blocks (sd_cpu_checksum_tree_blocks / _verify / _update) are the same two hashers over
// the items plan_tree_blocks makes, which the device list uses too.  The range proofs' twins run
// the workgroups plan_tree_ranges plans for the device, one by one.  No HIP: built with g++ under
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

void plan_tree_proofs(TreeProofPlan& p, const std::vector<uint64_t>& node_base, const uint64_t* rows, size_t m,
                      bool levels) {
    const size_t n = node_base.size() - 1;
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    if (p.proof_base.empty()) {
        for (size_t r = 0; r < m; r++) {  // everything refused before anything is allocated
            const uint64_t f = rows[2 * r], j = rows[2 * r + 1];
            if (f >= n) throw sd_failure(SD_ERR_INVALID, "block row " + std::to_string(r) + ": no such file");
            if (j >= node_base[f + 1] - node_base[f])
                throw sd_failure(SD_ERR_INVALID, "block row " + std::to_string(r) + ": no such block");
        }
        // the listed files' interior levels 1 .. h - 1 in the scratch, file by file in list order
        std::vector<uint32_t> tab(n, NONE);
        p.lvl_off.clear();
        p.scratch_nodes = 0;
        p.prow.resize(m);
        p.proof_base.assign(m + 1, 0);
        for (size_t r = 0; r < m; r++) {
            const uint64_t f = rows[2 * r], j = rows[2 * r + 1], nb = node_base[f + 1] - node_base[f];
            if (tab[f] == NONE) {
                if (p.lvl_off.size() >= (1ull << 31)) {
                    p.proof_base.clear();
                    throw sd_failure(SD_ERR_INVALID, "list too large");
                }
                tab[f] = (uint32_t)p.lvl_off.size();
                for (uint64_t c = (nb + 1) >> 1; c > 1; c = (c + 1) >> 1) {
                    p.lvl_off.push_back(p.scratch_nodes);
                    p.scratch_nodes += c;
                }
            }
            p.prow[r] = ck_proof_row{node_base[f], nb, p.proof_base[r], tab[f], (uint32_t)f};
            p.proof_base[r + 1] = p.proof_base[r] + tree_proof_entries(nb, j);
        }
    }
    if (!levels || p.levels) return;
    // the passes: a listed file's level 8p in groups of 256, each stored through min(8, h - 1 - 8p) levels
    std::vector<uint8_t> seen(n, 0);
    p.passes.clear();
    for (size_t r = 0; r < m; r++) {
        const uint64_t f = rows[2 * r];
        if (seen[f]) continue;
        seen[f] = 1;
        const uint64_t nb = node_base[f + 1] - node_base[f];
        const uint32_t h = tree_height(nb), tab = p.prow[r].lvl_tab;
        uint64_t cnt = nb;
        for (uint32_t q = 0; 8 * q + 1 < h; q++) {
            if (p.passes.size() <= q) p.passes.emplace_back();
            const uint64_t src = q == 0 ? node_base[f] : p.lvl_off[tab + 8 * q - 1];
            const uint32_t lv = std::min<uint32_t>(8, h - 1 - 8 * q);
            for (uint64_t g = 0; g * 256 < cnt; g++)
                p.passes[q].push_back(ck_levels_wg{src + 256 * g, 256 * g, (uint32_t)std::min<uint64_t>(256, cnt - 256 * g),
                                                   lv, tab + 8 * q, 0});
            cnt = (cnt + 255) >> 8;
        }
    }
    for (const auto& ps : p.passes)
        if (ps.size() >= (1ull << 31)) throw sd_failure(SD_ERR_INVALID, "list too large");
    p.levels = true;
}

void plan_tree_ranges(TreeRangePlan& out, const std::vector<uint64_t>& node_base, const uint64_t* rows, size_t m,
                      const uint64_t* range_base, size_t q) {
    const size_t n = node_base.size() - 1;
    TreeRangePlan p;
    p.set = true;
    p.range_base.assign(1, 0);
    p.proof_base.assign(1, 0);
    if (q == 0) {
        if (m) throw sd_failure(SD_ERR_INVALID, "no ranges over a list with rows");
        out = std::move(p);
        return;
    }
    if (!range_base) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (q >= (1ull << 32)) throw sd_failure(SD_ERR_INVALID, "list too large");
    if (range_base[0] != 0 || range_base[q] != m) throw sd_failure(SD_ERR_INVALID, "range_base does not run from 0 to m");
    std::vector<uint64_t>& firsts = p.firsts;
    firsts.resize(2 * q);
    for (size_t i = 0; i < q; i++) {  // everything refused before anything is planned (p is a local)
        const uint64_t r0 = range_base[i], r1 = range_base[i + 1];
        if (r1 <= r0 || r1 > m) throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + ": empty or out of order");
        const uint64_t f = rows[2 * r0], a = rows[2 * r0 + 1];
        if (f >= n || a >= node_base[f + 1] - node_base[f] || r1 - r0 > node_base[f + 1] - node_base[f] - a)
            throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + ": no such blocks");
        for (uint64_t r = r0 + 1; r < r1; r++)
            if (rows[2 * r] != f || rows[2 * r + 1] != a + (r - r0))
                throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + ": its rows are not consecutive blocks of one file");
        firsts[2 * i] = f, firsts[2 * i + 1] = a;
    }
    plan_tree_proofs(p.levels, node_base, firsts.data(), q, false);
    p.range_base.assign(range_base, range_base + q + 1);
    p.proof_base.assign(q + 1, 0);
    p.rrow.resize(q);
    for (size_t i = 0; i < q; i++) {
        const uint64_t f = firsts[2 * i], a = firsts[2 * i + 1], cnt = range_base[i + 1] - range_base[i];
        const uint64_t nb = node_base[f + 1] - node_base[f], last = a + cnt - 1;
        p.rrow[i] = ck_range_row{node_base[f], nb, a, cnt, p.proof_base[i], p.levels.prow[i].lvl_tab, (uint32_t)f};
        p.proof_base[i + 1] = p.proof_base[i] + tree_range_proof_entries(nb, a, cnt);
        // the passes: the range's nodes at level 8s in the 256-aligned groups they fall into
        const uint32_t h = tree_height(nb), n_pass = std::max<uint32_t>(1, (h + 7) / 8);
        uint64_t src0 = range_base[i], pb = p.proof_base[i], n_lvl = nb;
        for (uint32_t s = 0; s < n_pass; s++) {
            const uint32_t Lb = 8 * s, levels = std::min<uint32_t>(8, h - Lb);
            const bool fin = s + 1 == n_pass;
            uint8_t lmask = 0, rmask = 0;
            for (uint32_t l = 0; l < levels; l++, n_lvl = (n_lvl + 1) >> 1) {
                const uint64_t lo = a >> (Lb + l), hi = last >> (Lb + l);
                if (lo & 1) lmask |= (uint8_t)(1u << l);
                if (!(hi & 1) && hi + 1 < n_lvl) rmask |= (uint8_t)(1u << l);
            }
            const uint64_t lo = a >> Lb, hi = last >> Lb, g0 = lo >> 8, g1 = hi >> 8;
            const uint64_t dst0 = fin ? i : p.scratch_nodes;
            if (!fin) p.scratch_nodes += g1 - g0 + 1;
            if (p.passes.size() <= s) p.passes.emplace_back();
            for (uint64_t g = g0; g <= g1; g++) {
                const uint64_t i0 = std::max(lo, 256 * g), i1 = std::min(hi, 256 * g + 255);
                const uint8_t flags = (g == g0 ? CK_RANGE_FIRST : 0) | (g == g1 ? CK_RANGE_LAST : 0) | (fin ? CK_RANGE_FINAL : 0);
                p.passes[s].push_back(ck_range_wg{src0 + (i0 - lo), fin ? dst0 : dst0 + (g - g0), pb, (uint16_t)(i1 - i0 + 1),
                                                  (uint8_t)(i0 & 255), (uint8_t)levels, lmask, rmask, flags, 0});
            }
            pb += (uint64_t)__builtin_popcount(lmask) + (uint64_t)__builtin_popcount(rmask);
            src0 = dst0;
        }
    }
    for (const auto& ps : p.passes)
        if (ps.size() >= (1ull << 31)) throw sd_failure(SD_ERR_INVALID, "list too large");
    out = std::move(p);
}

namespace {

// one workgroup of a climb pass, as k_tree_range_climb runs it: the group's nodes at their slots,
// each level's flanks beside them, pairs from the even slot, the file's own carry last
void cpu_range_wg(const ck_range_wg& w, const uint8_t* src, uint8_t* scratch, const uint8_t* proofs, uint8_t* top) {
    uint8_t lds[256][32];
    uint32_t s = w.start, e = w.start + w.count - 1u;
    memcpy(lds[s], src + 32 * w.src_base, 32 * (size_t)w.count);
    const bool first = w.flags & CK_RANGE_FIRST, last = w.flags & CK_RANGE_LAST, fin = w.flags & CK_RANGE_FINAL;
    uint64_t at = w.pbase;
    for (uint32_t l = 0; l < w.levels; l++) {
        const uint32_t lb = (w.lmask >> l) & 1u, rb = (w.rmask >> l) & 1u;
        if (first && lb) memcpy(lds[s - 1], proofs + 32 * at, 32);
        if (last && rb) memcpy(lds[e + 1], proofs + 32 * (at + lb), 32);
        at += lb + rb;
        const uint32_t e2 = e + (last && rb ? 1u : 0u);
        s >>= 1, e >>= 1;
        for (uint32_t t = s; t <= e; t++) {
            if (2 * t + 1 <= e2) cpu_parent(lds[2 * t], lds[2 * t + 1], fin && l + 1 == w.levels, lds[t]);
            else memcpy(lds[t], lds[2 * t], 32);
        }
    }
    memcpy((fin ? top : scratch) + 32 * w.dst, lds[0], 32);
}

// every listed file's interior levels 1 .. h - 1 -> scratch (by p.lvl_off), level by level, the odd node carried
void cpu_fill_levels(const TreeProofPlan& p, const uint8_t* nodes, size_t n_files, uint8_t* scratch) {
    std::vector<uint8_t> seen(n_files, 0);
    for (const ck_proof_row& w : p.prow) {
        if (seen[w.file]) continue;
        seen[w.file] = 1;
        const uint8_t* src = nodes + 32 * w.node0;
        uint32_t L = 1;
        for (uint64_t n = w.nb; ((n + 1) >> 1) > 1; n = (n + 1) >> 1, L++) {
            uint8_t* dst = scratch + 32 * p.lvl_off[w.lvl_tab + L - 1];
            for (uint64_t i = 0; 2 * i + 1 < n; i++) cpu_parent(src + 64 * i, src + 64 * i + 32, false, dst + 32 * i);
            if (n & 1) memcpy(dst + 32 * (n >> 1), src + 32 * (n - 1), 32);
            src = dst;
        }
    }
}

// block j's proof from the file's level 0 (`level`) and its interior levels (`scratch` by lvl_off[tab ..])
// -> out, bottom-up
void cpu_gather_proof(const uint8_t* level, const uint8_t* scratch, const uint64_t* lvl_off, uint64_t nb, uint64_t j,
                      uint8_t* out) {
    uint32_t L = 0;
    for (uint64_t n = nb; n > 1; n = (n + 1) >> 1, j >>= 1, L++) {
        const uint64_t s = j ^ 1;
        if (s >= n) continue;
        memcpy(out, L == 0 ? level + 32 * s : scratch + 32 * (lvl_off[L - 1] + s), 32);
        out += 32;
    }
}

// block j's node climbed through its proof -> out (the root it claims)
void cpu_climb(const uint8_t* node, const uint8_t* proof, uint64_t nb, uint64_t j, uint8_t out[32]) {
    memcpy(out, node, 32);
    for (uint64_t n = nb; n > 1; n = (n + 1) >> 1, j >>= 1) {
        if ((j ^ 1) >= n) continue;
        if (j & 1) cpu_parent(proof, out, n == 2, out);
        else cpu_parent(out, proof, n == 2, out);
        proof += 32;
    }
}

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

int sd_checksum_tree_proof_entries(uint64_t len, uint32_t block_log2, uint64_t block, uint32_t* entries) {
    SD_GUARD_BEGIN
    if (!entries) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> nb;
    plan_tree_layout(&len, 1, block_log2, nb);
    if (block >= nb[1]) throw sd_failure(SD_ERR_INVALID, "no such block");
    *entries = tree_proof_entries(nb[1], block);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_prove(const uint8_t* nodes, const uint64_t* lens, size_t n_files, uint32_t block_log2,
                                      const uint64_t* rows, size_t m, uint8_t* proofs_out) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!nodes || !rows))) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n_files, block_log2, node_base);
    TreeProofPlan p;
    plan_tree_proofs(p, node_base, rows, m, false);
    if (m == 0 || p.proof_base[m] == 0) return SD_OK;
    if (!proofs_out) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint8_t> scratch(32 * p.scratch_nodes);
    cpu_fill_levels(p, nodes, n_files, scratch.data());
    for (size_t r = 0; r < m; r++) {
        const ck_proof_row& w = p.prow[r];
        cpu_gather_proof(nodes + 32 * w.node0, scratch.data(), p.lvl_off.data() + w.lvl_tab, w.nb, rows[2 * r + 1],
                         proofs_out + 32 * w.pbase);
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_verify_proofs(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                              uint32_t block_log2, const uint64_t* rows, const uint64_t* data_offsets,
                                              size_t m, const uint8_t* proofs, const uint8_t* roots,
                                              uint8_t* nodes_out, uint8_t* bad, uint64_t* rows_out, uint64_t capacity,
                                              uint64_t* count, uint64_t stats[4], int nthreads) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!data || !rows || !data_offsets || !roots)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    TreeBlocksPlan p;
    plan_tree_blocks(p, lens, n_files, block_log2, rows, data_offsets, m);
    TreeProofPlan pp;
    plan_tree_proofs(pp, p.node_base, rows, m, false);
    if (m && pp.proof_base[m] && !proofs) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (m == 0) return SD_OK;
    std::vector<uint8_t> own;
    if (!nodes_out) own.resize(32 * m), nodes_out = own.data();
    cpu_block_nodes(data, p, false, nodes_out, nthreads);
    std::vector<uint8_t> differs(m), file_bad(n_files, 0);
    cpu_parallel_for(m, nthreads, [&](size_t r) {
        const ck_proof_row& w = pp.prow[r];
        uint8_t top[32];
        cpu_climb(nodes_out + 32 * r, proofs + 32 * w.pbase, w.nb, rows[2 * r + 1], top);
        differs[r] = memcmp(top, roots + 32 * (uint64_t)w.file, 32) != 0;
    });
    uint64_t st[4] = {n_files, m, 0, 0};
    for (size_t r = 0; r < m; r++) {
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

int sd_checksum_tree_range_proof_entries(uint64_t len, uint32_t block_log2, uint64_t first, uint64_t count,
                                         uint32_t* entries) {
    SD_GUARD_BEGIN
    if (!entries) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> nb;
    plan_tree_layout(&len, 1, block_log2, nb);
    if (count == 0 || first >= nb[1] || count > nb[1] - first) throw sd_failure(SD_ERR_INVALID, "no such range");
    *entries = tree_range_proof_entries(nb[1], first, count);
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_prove_ranges(const uint8_t* nodes, const uint64_t* lens, size_t n_files,
                                             uint32_t block_log2, const uint64_t* rows, size_t m,
                                             const uint64_t* range_base, size_t q, uint8_t* proofs_out) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!nodes || !rows))) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint64_t> node_base;
    plan_tree_layout(lens, n_files, block_log2, node_base);
    TreeRangePlan p;
    plan_tree_ranges(p, node_base, rows, m, range_base, q);
    if (p.proof_base[q] == 0) return SD_OK;
    if (!proofs_out) throw sd_failure(SD_ERR_INVALID, "null argument");
    std::vector<uint8_t> scratch(32 * p.levels.scratch_nodes);
    cpu_fill_levels(p.levels, nodes, n_files, scratch.data());
    for (const ck_range_row& w : p.rrow) {  // the flanks that exist, bottom-up, left before right
        uint8_t* o = proofs_out + 32 * w.pbase;
        uint64_t lo = w.first, hi = w.first + w.count - 1;
        uint32_t L = 0;
        for (uint64_t n = w.nb; n > 1; n = (n + 1) >> 1, lo >>= 1, hi >>= 1, L++) {
            const uint8_t* lvl = L == 0 ? nodes + 32 * w.node0 : scratch.data() + 32 * p.levels.lvl_off[w.lvl_tab + L - 1];
            if (lo & 1) memcpy(o, lvl + 32 * (lo - 1), 32), o += 32;
            if (!(hi & 1) && hi + 1 < n) memcpy(o, lvl + 32 * (hi + 1), 32), o += 32;
        }
    }
    return SD_OK;
    SD_GUARD_END
}

int sd_cpu_checksum_tree_blocks_verify_range_proofs(const uint8_t* data, const uint64_t* lens, size_t n_files,
                                                    uint32_t block_log2, const uint64_t* rows,
                                                    const uint64_t* data_offsets, size_t m, const uint64_t* range_base,
                                                    size_t q, const uint8_t* proofs, const uint8_t* roots,
                                                    uint8_t* nodes_out, uint8_t* bad, uint64_t* ranges_out,
                                                    uint64_t capacity, uint64_t* count, uint64_t stats[4], int nthreads) {
    SD_GUARD_BEGIN
    if ((n_files && !lens) || (m && (!data || !rows || !data_offsets || !roots)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    TreeBlocksPlan p;
    plan_tree_blocks(p, lens, n_files, block_log2, rows, data_offsets, m);
    TreeRangePlan rp;
    plan_tree_ranges(rp, p.node_base, rows, m, range_base, q);
    if (rp.proof_base[q] && !proofs) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (count) *count = 0;
    if (stats) memset(stats, 0, 4 * sizeof(uint64_t));
    if (m == 0) return SD_OK;
    std::vector<uint8_t> own;
    if (!nodes_out) own.resize(32 * m), nodes_out = own.data();
    cpu_block_nodes(data, p, false, nodes_out, nthreads);
    // the device's passes, one task per workgroup: pass s reads what pass s - 1 left in the scratch
    std::vector<uint8_t> scratch(32 * rp.scratch_nodes), top(32 * q);
    for (size_t s = 0; s < rp.passes.size(); s++) {
        const uint8_t* src = s == 0 ? nodes_out : scratch.data();
        cpu_parallel_for(rp.passes[s].size(), nthreads,
                         [&](size_t g) { cpu_range_wg(rp.passes[s][g], src, scratch.data(), proofs, top.data()); });
    }
    std::vector<uint8_t> differs(q), file_bad(n_files, 0);
    uint64_t st[4] = {n_files, q, 0, 0};
    for (size_t i = 0; i < q; i++) {
        const uint32_t f = rp.rrow[i].file;
        differs[i] = memcmp(top.data() + 32 * i, roots + 32 * (uint64_t)f, 32) != 0;
        if (bad) bad[i] = differs[i];
        st[2] += differs[i];
        if (differs[i] && !file_bad[f]) file_bad[f] = 1, st[3]++;
    }
    if (count) *count = st[2];
    if (stats) memcpy(stats, st, sizeof st);
    if (ranges_out) {
        if (capacity < st[2]) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of differing ranges");
        uint64_t o = 0;
        for (size_t i = 0; i < q; i++)
            if (differs[i])
                ranges_out[3 * o] = rp.rrow[i].file, ranges_out[3 * o + 1] = rp.rrow[i].first, ranges_out[3 * o + 2] = rp.rrow[i].count, o++;
    }
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
