// checksum_tree_selftest.cpp -- sd_cpu_checksum_tree, _roots and _verify (checksum_tree_host.cpp)
// against a byte-at-a-time model of the node definitions (include/sd_cas.h, checksum trees): a
// scalar BLAKE3 of its own that absorbs one byte per step, compresses a block when the next byte
// arrives, and builds every node and every root by the level-wise rule, sharing nothing with
// cpu_blake3.cpp.  Small sizes around the chunk, the lane (4 KiB) and the block boundaries at each
// block size, in one batch with an odd start; the position rule; the flips of a verify with the
// capacity rule over pre-filled buffers and every NULL output; the refusals; an empty batch; and
// concurrent calls.  The listed blocks (sd_cpu_checksum_tree_blocks, _verify, _update) against the
// same model: every block of those batches in a scrambled order from scattered places over 0xA5, a
// block at chunk counter 2^32, a repeated and an omitted row, the patched level.  The range proofs
// (sd_checksum_tree_range_proof_entries, sd_cpu_checksum_tree_blocks_prove_ranges, _verify_range_proofs)
// against the model's own range climb: every range of small files, one block equal to the block proof,
// a flipped entry and a flipped byte, ranges across the groups of 256, the refusals.
// A program of its own: built plain for the CPU suite (`make
// checksum-tree-selftest`, tests/test_checksum_tree.py) and under ASan + UBSan and TSan (`make
// sanitize-checksum-tree`, logs in profiles/checksum_tree/).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <thread>
#include <vector>

#include "sd_host.h"
#include "selftest_blake3.h"

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

typedef std::vector<uint8_t> bytes;

// ---------------------------------------------------------------- batches
static uint64_t mix(uint64_t seed, uint64_t i) {  // splitmix64
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct batch_t {
    uint32_t k = 17;
    std::vector<uint64_t> offs, lens, base;
    bytes data;
    size_t n() const { return lens.size(); }
    uint64_t total() const { return base.back(); }
    void build(uint32_t k_, const std::vector<uint64_t>& ls, uint64_t seed) {
        k = k_;
        lens = ls;
        offs.clear();
        base.assign(1, 0);
        uint64_t cur = 0;
        for (size_t i = 0; i < ls.size(); i++) {
            if (i == 3) cur += 16;  // a 16-byte aligned start that is on no 128-byte line
            offs.push_back(cur);
            cur = (cur + ls[i] + 127) / 128 * 128;
            base.push_back(base.back() + std::max<uint64_t>(1, (ls[i] + (1ull << k) - 1) >> k));
        }
        data.resize(cur + 64);
        for (size_t i = 0; i < data.size(); i += 8) {
            const uint64_t v = mix(seed, i);
            memcpy(data.data() + i, &v, std::min<size_t>(8, data.size() - i));
        }
    }
};

struct answer_t {
    bytes nodes, roots;
};

static answer_t model(const batch_t& b) {
    answer_t a;
    a.nodes.resize(32 * b.total());
    a.roots.resize(32 * b.n());
    const uint64_t B = 1ull << b.k;
    for (size_t i = 0; i < b.n(); i++) {
        const uint8_t* p = b.data.data() + b.offs[i];
        const uint64_t nb = b.base[i + 1] - b.base[i];
        if (nb == 1) {
            m_put(m_subtree(p, b.lens[i], 0, true), a.nodes.data() + 32 * b.base[i]);
            memcpy(a.roots.data() + 32 * i, a.nodes.data() + 32 * b.base[i], 32);
            continue;
        }
        std::vector<cv_t> lvl;
        for (uint64_t j = 0; j < nb; j++) {
            lvl.push_back(m_subtree(p + j * B, std::min<uint64_t>(B, b.lens[i] - j * B), j * B / 1024, false));
            m_put(lvl.back(), a.nodes.data() + 32 * (b.base[i] + j));
        }
        m_put(m_merge(lvl, true), a.roots.data() + 32 * i);
    }
    return a;
}

static answer_t run(const batch_t& b, int nthreads) {
    answer_t a;
    a.nodes.assign(32 * b.total() + 32, 0xA5);  // one guard row each
    a.roots.assign(32 * b.n() + 32, 0xA5);
    CHECK(sd_cpu_checksum_tree(b.data.data(), b.offs.data(), b.lens.data(), b.n(), b.k, a.nodes.data(), a.roots.data(),
                               nthreads) == SD_OK);
    CHECK(std::all_of(a.nodes.end() - 32, a.nodes.end(), [](uint8_t x) { return x == 0xA5; }));
    CHECK(std::all_of(a.roots.end() - 32, a.roots.end(), [](uint8_t x) { return x == 0xA5; }));
    a.nodes.resize(32 * b.total());
    a.roots.resize(32 * b.n());
    return a;
}

static std::vector<uint64_t> small_sizes(uint32_t k) {
    const uint64_t B = 1ull << k;
    std::vector<uint64_t> ls = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, B - 1, B, B + 1};
    if (k == 17) {
        const uint64_t more[] = {2 * B - 1, 2 * B + 1, 3 * B + 5000, 8 * B + 1, 9 * B + 1024};  // past one 1 MiB block too
        ls.insert(ls.end(), more, more + 5);
    }
    return ls;
}

static void test_levels_and_roots() {
    for (uint32_t k = SD_TREE_BLOCK_LOG2_MIN; k <= SD_TREE_BLOCK_LOG2_MAX; k++) {
        batch_t b;
        b.build(k, small_sizes(k), 100 + k);
        const answer_t want = model(b);
        for (int nthreads : {1, 4}) {
            const answer_t got = run(b, nthreads);
            CHECK(got.nodes == want.nodes);
            CHECK(got.roots == want.roots);
        }
        // the roots are file_checksum's, and come from the level alone
        for (size_t i = 0; i < b.n(); i++) {
            uint8_t h[32];
            cpu_blake3(b.data.data() + b.offs[i], b.lens[i], h);
            CHECK(memcmp(h, want.roots.data() + 32 * i, 32) == 0);
        }
        bytes roots(32 * b.n(), 0);
        CHECK(sd_cpu_checksum_tree_roots(want.nodes.data(), b.lens.data(), b.n(), k, roots.data()) == SD_OK);
        CHECK(roots == want.roots);
        for (size_t i = 0; i < b.n(); i++) {
            uint64_t nb = 0;
            CHECK(sd_checksum_tree_nodes(b.lens[i], k, &nb) == SD_OK && nb == b.base[i + 1] - b.base[i]);
        }
    }
}

static void test_position_rule() {  // a full block's node does not depend on the file's length
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t a, c;
    a.build(k, {3 * B + 5000}, 7);
    c.build(k, {3 * B + 5000 - B - 7}, 7);  // the same bytes, shorter
    const answer_t x = run(a, 2), y = run(c, 2);
    CHECK(memcmp(x.nodes.data(), y.nodes.data(), 2 * 32) == 0);       // blocks 0 and 1: full in both
    CHECK(memcmp(x.nodes.data() + 64, y.nodes.data() + 64, 32) != 0);  // block 2: partial in the shorter
    CHECK(m_get(x.nodes.data()) == m_subtree(a.data.data(), B, 0, false));
}

static void test_verify() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t b;
    b.build(k, {4097, 3 * B + 5000, 0, 2 * B + 1, B, 700}, 9);
    const answer_t want = model(b);
    const uint64_t total = b.total();
    uint64_t count = 99, stats[4];
    bytes bad(total + 1, 0xA5);
    std::vector<uint64_t> rows(2 * total + 2, 0xA5A5);
    // a clean batch
    CHECK(sd_cpu_checksum_tree_verify(b.data.data(), b.offs.data(), b.lens.data(), b.n(), k, want.nodes.data(), bad.data(),
                                      rows.data(), total, &count, stats, 3) == SD_OK);
    CHECK(count == 0 && stats[0] == b.n() && stats[1] == total && stats[2] == 0 && stats[3] == 0);
    CHECK(std::all_of(bad.begin(), bad.end() - 1, [](uint8_t x) { return x == 0; }) && bad[total] == 0xA5);
    CHECK(std::all_of(rows.begin(), rows.end(), [](uint64_t x) { return x == 0xA5A5; }));
    // the first byte of a middle block, the last byte of a file, a byte of a partial last block, a
    // byte of a one-block file
    batch_t f = b;
    f.data[f.offs[1] + B] ^= 1, f.data[f.offs[3] + 2 * B] ^= 1, f.data[f.offs[1] + 3 * B + 4000] ^= 1, f.data[f.offs[0] + 100] ^= 1;
    const std::vector<uint64_t> want_rows = {0, 0, 1, 1, 1, 3, 3, 2};
    bytes want_bad(total, 0);
    for (size_t r = 0; r < want_rows.size(); r += 2) want_bad[b.base[want_rows[r]] + want_rows[r + 1]] = 1;
    for (int mask = 0; mask < 4; mask++) {  // bad and rows each NULL in turn
        std::fill(bad.begin(), bad.end(), 0xA5);
        std::fill(rows.begin(), rows.end(), 0xA5A5);
        count = 99;
        CHECK(sd_cpu_checksum_tree_verify(f.data.data(), f.offs.data(), f.lens.data(), f.n(), k, want.nodes.data(),
                                          mask & 1 ? bad.data() : nullptr, mask & 2 ? rows.data() : nullptr, 4, &count,
                                          mask == 3 ? stats : nullptr, 1 + mask) == SD_OK);
        CHECK(count == 4);
        if (mask & 1) CHECK(memcmp(bad.data(), want_bad.data(), total) == 0 && bad[total] == 0xA5);
        if (mask & 2) CHECK(std::equal(want_rows.begin(), want_rows.end(), rows.begin()) && rows[8] == 0xA5A5);
    }
    CHECK(stats[0] == b.n() && stats[1] == total && stats[2] == 4 && stats[3] == 3);
    // a capacity one short: the requirement, the flags and stats complete, no row written
    std::fill(bad.begin(), bad.end(), 0xA5);
    std::fill(rows.begin(), rows.end(), 0xA5A5);
    count = 0;
    memset(stats, 0, sizeof stats);
    CHECK(sd_cpu_checksum_tree_verify(f.data.data(), f.offs.data(), f.lens.data(), f.n(), k, want.nodes.data(), bad.data(),
                                      rows.data(), 3, &count, stats, 2) == SD_ERR_CAPACITY);
    CHECK(count == 4 && stats[2] == 4 && stats[3] == 3 && memcmp(bad.data(), want_bad.data(), total) == 0);
    CHECK(std::all_of(rows.begin(), rows.end(), [](uint64_t x) { return x == 0xA5A5; }));
    // count and stats may be NULL
    CHECK(sd_cpu_checksum_tree_verify(f.data.data(), f.offs.data(), f.lens.data(), f.n(), k, want.nodes.data(), nullptr,
                                      nullptr, 0, nullptr, nullptr, 1) == SD_OK);
}

static void test_refusals_and_empty() {
    batch_t b;
    b.build(17, {100, 5000}, 3);
    bytes nodes(64, 0xA5), roots(64, 0xA5);
    uint64_t nb = 7, count = 0;
    for (uint32_t k : {0u, 16u, 21u, 64u, ~0u}) {
        CHECK(sd_checksum_tree_nodes(1, k, &nb) == SD_ERR_INVALID && nb == 7);
        CHECK(sd_cpu_checksum_tree(b.data.data(), b.offs.data(), b.lens.data(), 2, k, nodes.data(), roots.data(), 1) == SD_ERR_INVALID);
        CHECK(sd_cpu_checksum_tree_roots(nodes.data(), b.lens.data(), 2, k, roots.data()) == SD_ERR_INVALID);
        CHECK(sd_cpu_checksum_tree_verify(b.data.data(), b.offs.data(), b.lens.data(), 2, k, nodes.data(), nullptr, nullptr, 0,
                                          &count, nullptr, 1) == SD_ERR_INVALID);
    }
    CHECK(sd_checksum_tree_nodes(1, 17, nullptr) == SD_ERR_INVALID);
    const uint64_t odd[2] = {0, 136};
    CHECK(sd_cpu_checksum_tree(b.data.data(), odd, b.lens.data(), 2, 17, nodes.data(), roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_verify(b.data.data(), odd, b.lens.data(), 2, 17, nodes.data(), nullptr, nullptr, 0, &count,
                                      nullptr, 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree(nullptr, b.offs.data(), b.lens.data(), 2, 17, nodes.data(), roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree(b.data.data(), nullptr, b.lens.data(), 2, 17, nodes.data(), roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree(b.data.data(), b.offs.data(), nullptr, 2, 17, nodes.data(), roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree(b.data.data(), b.offs.data(), b.lens.data(), 2, 17, nullptr, roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree(b.data.data(), b.offs.data(), b.lens.data(), 2, 17, nodes.data(), nullptr, 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_verify(b.data.data(), b.offs.data(), b.lens.data(), 2, 17, nullptr, nullptr, nullptr, 0, &count,
                                      nullptr, 1) == SD_ERR_INVALID);
    CHECK(std::all_of(nodes.begin(), nodes.end(), [](uint8_t x) { return x == 0xA5; }));
    CHECK(std::all_of(roots.begin(), roots.end(), [](uint8_t x) { return x == 0xA5; }));
    // an empty batch
    uint64_t stats[4] = {9, 9, 9, 9};
    count = 9;
    CHECK(sd_cpu_checksum_tree(nullptr, nullptr, nullptr, 0, 17, nullptr, nullptr, 1) == SD_OK);
    CHECK(sd_cpu_checksum_tree_roots(nullptr, nullptr, 0, 17, nullptr) == SD_OK);
    CHECK(sd_cpu_checksum_tree_verify(nullptr, nullptr, nullptr, 0, 17, nullptr, nullptr, nullptr, 0, &count, stats, 1) == SD_OK);
    CHECK(count == 0 && stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0);
}

static void test_concurrent_calls() {  // the calls hold no shared state beyond the thread pools
    batch_t b;
    b.build(17, small_sizes(17), 21);
    const answer_t want = model(b);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            const answer_t got = run(b, 1 + t);
            ok[t] = got.nodes == want.nodes && got.roots == want.roots;
        });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

// ---------------------------------------------------------------- listed blocks
// rows (file, block) of a batch's files, their bytes copied to scattered, 16-byte aligned places of
// a buffer of their own whose every other byte is 0xA5
struct list_t {
    std::vector<uint64_t> rows, offs;
    bytes data;
    size_t m() const { return offs.size(); }
    void add(const batch_t& b, uint64_t f, uint64_t j) {
        const uint64_t B = 1ull << b.k, len = b.lens[f] == 0 ? 0 : std::min<uint64_t>(B, b.lens[f] - j * B);
        const uint64_t at = (data.size() + 127) / 128 * 128 + (m() % 3 == 1 ? 16 : 0);
        data.resize(at + len + 64, 0xA5);
        memcpy(data.data() + at, b.data.data() + b.offs[f] + j * B, len);
        rows.push_back(f), rows.push_back(j), offs.push_back(at);
    }
    // every block of every file, in an order scrambled by `seed`
    void every(const batch_t& b, uint64_t seed) {
        std::vector<std::pair<uint64_t, std::pair<uint64_t, uint64_t>>> order;
        for (size_t i = 0; i < b.n(); i++)
            for (uint64_t j = 0; j < b.base[i + 1] - b.base[i]; j++) order.push_back({mix(seed, order.size()), {i, j}});
        std::sort(order.begin(), order.end());
        for (const auto& o : order) add(b, o.second.first, o.second.second);
    }
};

static bytes run_blocks(const batch_t& b, const list_t& l, int nthreads) {
    bytes out(32 * l.m() + 32, 0xA5);  // one guard row
    CHECK(sd_cpu_checksum_tree_blocks(l.data.data(), b.lens.data(), b.n(), b.k, l.rows.data(), l.offs.data(), l.m(),
                                      out.data(), nthreads) == SD_OK);
    CHECK(std::all_of(out.end() - 32, out.end(), [](uint8_t x) { return x == 0xA5; }));
    out.resize(32 * l.m());
    return out;
}

static void test_blocks() {
    for (uint32_t k = SD_TREE_BLOCK_LOG2_MIN; k <= SD_TREE_BLOCK_LOG2_MAX; k++) {
        batch_t b;
        b.build(k, small_sizes(k), 300 + k);
        const answer_t want = model(b);
        list_t l;
        l.every(b, 17 + k);
        CHECK(l.m() == b.total());
        for (int nthreads : {1, 4}) {
            const bytes got = run_blocks(b, l, nthreads);
            for (size_t r = 0; r < l.m(); r++)
                CHECK(memcmp(got.data() + 32 * r, want.nodes.data() + 32 * (b.base[l.rows[2 * r]] + l.rows[2 * r + 1]), 32) == 0);
        }
        // a block at chunk counter exactly 2^32 of a file of 4 TiB: only its bytes are resident
        batch_t h;
        h.build(k, {4097}, 5);
        const uint64_t hl[1] = {(1ull << 42) + 4097}, hr[2] = {0, 1ull << (42 - k)}, ho[1] = {0};
        uint8_t node[32];
        CHECK(sd_cpu_checksum_tree_blocks(h.data.data(), hl, 1, k, hr, ho, 1, node, 1) == SD_OK);
        CHECK(m_get(node) == m_subtree(h.data.data(), 4097, 1ull << 32, false));
        CHECK(!(m_get(node) == m_subtree(h.data.data(), 4097, 0, false)));
    }
}

static void test_blocks_verify_and_update() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t b;
    b.build(k, {4097, 3 * B + 5000, 0, 2 * B + 1, B, 700}, 9);
    const answer_t want = model(b);
    // flips: the first byte of a middle block, the last byte of a partial last block, a byte of a
    // one-block file, and a byte of a block the list omits
    batch_t f = b;
    f.data[f.offs[1] + B] ^= 1, f.data[f.offs[3] + 2 * B] ^= 1, f.data[f.offs[0] + 100] ^= 1, f.data[f.offs[1] + 2 * B + 9] ^= 1;
    list_t l;  // (1, 2) is not listed; (1, 1) is listed twice
    for (const auto& r : std::vector<std::pair<uint64_t, uint64_t>>{{3, 2}, {1, 0}, {1, 1}, {2, 0}, {5, 0}, {0, 0}, {1, 3}, {3, 0}, {1, 1}, {4, 0}})
        l.add(f, r.first, r.second);
    const std::vector<uint64_t> want_rows = {3, 2, 1, 1, 0, 0, 1, 1};
    const bytes want_bad = {1, 0, 1, 0, 0, 1, 0, 0, 1, 0};
    const size_t m = l.m();
    uint64_t count = 99, stats[4];
    bytes bad(m + 1, 0xA5);
    std::vector<uint64_t> rows(2 * m + 2, 0xA5A5);
    for (int mask = 0; mask < 4; mask++) {  // bad and rows each NULL in turn
        std::fill(bad.begin(), bad.end(), 0xA5);
        std::fill(rows.begin(), rows.end(), 0xA5A5);
        count = 99;
        CHECK(sd_cpu_checksum_tree_blocks_verify(l.data.data(), f.lens.data(), f.n(), k, l.rows.data(), l.offs.data(), m,
                                                 want.nodes.data(), mask & 1 ? bad.data() : nullptr,
                                                 mask & 2 ? rows.data() : nullptr, 4, &count, mask == 3 ? stats : nullptr,
                                                 1 + mask) == SD_OK);
        CHECK(count == 4);
        if (mask & 1) CHECK(memcmp(bad.data(), want_bad.data(), m) == 0 && bad[m] == 0xA5);
        if (mask & 2) CHECK(std::equal(want_rows.begin(), want_rows.end(), rows.begin()) && rows[8] == 0xA5A5);
    }
    CHECK(stats[0] == b.n() && stats[1] == m && stats[2] == 4 && stats[3] == 3);
    // a capacity one short: the requirement, the flags and stats complete, no row written
    std::fill(bad.begin(), bad.end(), 0xA5);
    std::fill(rows.begin(), rows.end(), 0xA5A5);
    count = 0;
    memset(stats, 0, sizeof stats);
    CHECK(sd_cpu_checksum_tree_blocks_verify(l.data.data(), f.lens.data(), f.n(), k, l.rows.data(), l.offs.data(), m,
                                             want.nodes.data(), bad.data(), rows.data(), 3, &count, stats, 2) == SD_ERR_CAPACITY);
    CHECK(count == 4 && stats[2] == 4 && stats[3] == 3 && memcmp(bad.data(), want_bad.data(), m) == 0);
    CHECK(std::all_of(rows.begin(), rows.end(), [](uint64_t x) { return x == 0xA5A5; }));
    // update: the repeated row is refused and nothing is written; without it the listed nodes are
    // the flipped data's, the unlisted ones stay, the roots follow the patched level
    bytes nodes = want.nodes, roots(32 * b.n() + 32, 0xA5);
    CHECK(sd_cpu_checksum_tree_blocks_update(l.data.data(), f.lens.data(), f.n(), k, l.rows.data(), l.offs.data(), m,
                                             nodes.data(), roots.data(), 2) == SD_ERR_INVALID);
    CHECK(nodes == want.nodes && std::all_of(roots.begin(), roots.end(), [](uint8_t x) { return x == 0xA5; }));
    list_t u;
    for (const auto& r : std::vector<std::pair<uint64_t, uint64_t>>{{3, 2}, {1, 1}, {0, 0}, {4, 0}}) u.add(f, r.first, r.second);
    CHECK(sd_cpu_checksum_tree_blocks_update(u.data.data(), f.lens.data(), f.n(), k, u.rows.data(), u.offs.data(), u.m(),
                                             nodes.data(), roots.data(), 2) == SD_OK);
    batch_t g = b;  // the bytes the patched level stands for: the listed flips only
    g.data[g.offs[1] + B] ^= 1, g.data[g.offs[3] + 2 * B] ^= 1, g.data[g.offs[0] + 100] ^= 1;
    const answer_t after = model(g);
    CHECK(nodes == after.nodes);
    CHECK(memcmp(roots.data(), after.roots.data(), 32 * b.n()) == 0);
    CHECK(std::all_of(roots.end() - 32, roots.end(), [](uint8_t x) { return x == 0xA5; }));
}

static void test_blocks_refusals_and_empty() {
    const uint64_t B = 1ull << 17;
    batch_t b;
    b.build(17, {100, B + 1}, 3);
    list_t l;
    l.add(b, 0, 0), l.add(b, 1, 1);
    bytes out(64, 0xA5), nodes(96, 0xA5), roots(64, 0xA5);
    uint64_t count = 0;
    auto blocks = [&](const uint8_t* d, const uint64_t* ls, uint32_t k, const uint64_t* rw, const uint64_t* of, uint8_t* o) {
        return sd_cpu_checksum_tree_blocks(d, ls, 2, k, rw, of, 2, o, 1);
    };
    for (uint32_t k : {0u, 16u, 21u, 64u, ~0u}) {
        CHECK(blocks(l.data.data(), b.lens.data(), k, l.rows.data(), l.offs.data(), out.data()) == SD_ERR_INVALID);
        CHECK(sd_cpu_checksum_tree_blocks_verify(l.data.data(), b.lens.data(), 2, k, l.rows.data(), l.offs.data(), 2, nodes.data(),
                                                 nullptr, nullptr, 0, &count, nullptr, 1) == SD_ERR_INVALID);
        CHECK(sd_cpu_checksum_tree_blocks_update(l.data.data(), b.lens.data(), 2, k, l.rows.data(), l.offs.data(), 2, nodes.data(),
                                                 roots.data(), 1) == SD_ERR_INVALID);
    }
    const uint64_t no_file[4] = {2, 0, 1, 1}, no_block[4] = {0, 1, 1, 1}, past[4] = {0, 0, 1, 2}, odd[2] = {0, l.offs[1] + 8};
    CHECK(blocks(l.data.data(), b.lens.data(), 17, no_file, l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, no_block, l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, past, l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, l.rows.data(), odd, out.data()) == SD_ERR_INVALID);
    CHECK(blocks(nullptr, b.lens.data(), 17, l.rows.data(), l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), nullptr, 17, l.rows.data(), l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, nullptr, l.offs.data(), out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, l.rows.data(), nullptr, out.data()) == SD_ERR_INVALID);
    CHECK(blocks(l.data.data(), b.lens.data(), 17, l.rows.data(), l.offs.data(), nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_verify(l.data.data(), b.lens.data(), 2, 17, l.rows.data(), l.offs.data(), 2, nullptr, nullptr,
                                             nullptr, 0, &count, nullptr, 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_update(l.data.data(), b.lens.data(), 2, 17, l.rows.data(), l.offs.data(), 2, nullptr,
                                             roots.data(), 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_update(l.data.data(), b.lens.data(), 2, 17, l.rows.data(), l.offs.data(), 2, nodes.data(),
                                             nullptr, 1) == SD_ERR_INVALID);
    for (const bytes* x : {&out, &nodes, &roots}) CHECK(std::all_of(x->begin(), x->end(), [](uint8_t v) { return v == 0xA5; }));
    // an empty list: every call does nothing
    uint64_t stats[4] = {9, 9, 9, 9};
    count = 9;
    CHECK(sd_cpu_checksum_tree_blocks(nullptr, b.lens.data(), 2, 17, nullptr, nullptr, 0, nullptr, 1) == SD_OK);
    CHECK(sd_cpu_checksum_tree_blocks_verify(nullptr, b.lens.data(), 2, 17, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, &count,
                                             stats, 1) == SD_OK);
    CHECK(count == 0 && stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0);
    CHECK(sd_cpu_checksum_tree_blocks_update(nullptr, b.lens.data(), 2, 17, nullptr, nullptr, 0, nullptr, nullptr, 1) == SD_OK);
    CHECK(sd_cpu_checksum_tree_blocks(nullptr, nullptr, 0, 17, nullptr, nullptr, 0, nullptr, 1) == SD_OK);
}

static void test_blocks_concurrent_calls() {
    batch_t b;
    b.build(17, small_sizes(17), 23);
    const answer_t want = model(b);
    list_t l;
    l.every(b, 4);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            const bytes got = run_blocks(b, l, 1 + t);
            int good = 1;
            for (size_t r = 0; r < l.m(); r++)
                good &= memcmp(got.data() + 32 * r, want.nodes.data() + 32 * (b.base[l.rows[2 * r]] + l.rows[2 * r + 1]), 32) == 0;
            ok[t] = good;
        });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

// ---------------------------------------------------------------- block proofs
// the model's climb: block j's node through `proof` to the root it claims (include/sd_cas.h, block proofs)
static cv_t m_climb(cv_t cv, const uint8_t* proof, uint64_t nb, uint64_t j, size_t* used) {
    size_t at = 0;
    for (uint64_t n = nb; n > 1; n = (n + 1) / 2, j >>= 1) {
        if ((j ^ 1) >= n) continue;
        const cv_t e = m_get(proof + 32 * at++);
        cv = (j & 1) ? m_parent(e, cv, n == 2) : m_parent(cv, e, n == 2);
    }
    *used = at;
    return cv;
}

static void test_proofs() {
    for (uint32_t k : {17u, 20u}) {
        const uint64_t B = 1ull << k;
        batch_t b;  // nb = 1 (empty, 1 byte), 2, 3, 5, 8, 9
        b.build(k, {0, 1, B + 1, 2 * B + 4097, 4 * B + 77, 8 * B, 8 * B + 1}, 40 + k);
        const answer_t want = model(b);
        list_t l;
        l.every(b, 5 + k);
        l.add(b, 5, 3), l.add(b, 4, 4);  // repeats
        const size_t m = l.m();
        std::vector<uint64_t> base(m + 1, 0);
        for (size_t r = 0; r < m; r++) {
            uint32_t e = 99;
            CHECK(sd_checksum_tree_proof_entries(b.lens[l.rows[2 * r]], k, l.rows[2 * r + 1], &e) == SD_OK);
            base[r + 1] = base[r] + e;
        }
        bytes proofs(32 * base[m] + 32, 0xA5);  // one guard row
        CHECK(sd_cpu_checksum_tree_blocks_prove(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, proofs.data()) == SD_OK);
        CHECK(std::all_of(proofs.end() - 32, proofs.end(), [](uint8_t x) { return x == 0xA5; }));
        for (size_t r = 0; r < m; r++) {  // every proof climbs to the model's root, using exactly its entries
            const uint64_t f = l.rows[2 * r], j = l.rows[2 * r + 1];
            size_t used = 0;
            const cv_t top = m_climb(m_get(want.nodes.data() + 32 * (b.base[f] + j)), proofs.data() + 32 * base[r],
                                     b.base[f + 1] - b.base[f], j, &used);
            CHECK(used == base[r + 1] - base[r]);
            CHECK(top == m_get(want.roots.data() + 32 * f));
        }
        // verify_proofs: clean, then one flipped byte, one flipped entry and one flipped root
        uint64_t count = 99, stats[4];
        bytes bad(m + 1, 0xA5), nodes(32 * m + 32, 0xA5);
        std::vector<uint64_t> rows(2 * m + 2, 0xA5A5);
        CHECK(sd_cpu_checksum_tree_blocks_verify_proofs(l.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(), m,
                                                        proofs.data(), want.roots.data(), nodes.data(), bad.data(), rows.data(),
                                                        m, &count, stats, 3) == SD_OK);
        CHECK(count == 0 && stats[0] == b.n() && stats[1] == m && stats[2] == 0 && stats[3] == 0);
        CHECK(std::all_of(bad.begin(), bad.end() - 1, [](uint8_t x) { return x == 0; }) && bad[m] == 0xA5);
        CHECK(nodes.size() == 32 * m + 32 && memcmp(nodes.data(), run_blocks(b, l, 2).data(), 32 * m) == 0);
        CHECK(std::all_of(nodes.end() - 32, nodes.end(), [](uint8_t x) { return x == 0xA5; }));
        CHECK(std::all_of(rows.begin(), rows.end(), [](uint64_t x) { return x == 0xA5A5; }));
        list_t fl = l;
        bytes fp = proofs, fr = want.roots;
        size_t r_byte = 0, r_entry = 0;
        for (size_t r = 0; r < m; r++) {
            if (l.rows[2 * r] == 6 && l.rows[2 * r + 1] == 8) r_byte = r;   // the 1-byte trailing block
            if (l.rows[2 * r] == 3 && l.rows[2 * r + 1] == 2) r_entry = r;  // nb = 3, carried once: one entry
        }
        CHECK(base[r_entry + 1] - base[r_entry] == 1);
        fl.data[fl.offs[r_byte]] ^= 0x80;
        fp[32 * base[r_entry] + 31] ^= 0x01;
        fr[32 * 2 + 5] ^= 0x10;  // file 2 (nb = 2): both of its rows
        bytes want_bad(m, 0);
        std::vector<uint64_t> want_rows;
        for (size_t r = 0; r < m; r++) {
            want_bad[r] = r == r_byte || r == r_entry || l.rows[2 * r] == 2;
            if (want_bad[r]) want_rows.push_back(l.rows[2 * r]), want_rows.push_back(l.rows[2 * r + 1]);
        }
        CHECK(want_rows.size() == 8);
        for (int mask = 0; mask < 4; mask++) {  // bad and rows each NULL in turn, nodes_out NULL
            std::fill(bad.begin(), bad.end(), 0xA5);
            std::fill(rows.begin(), rows.end(), 0xA5A5);
            count = 99;
            CHECK(sd_cpu_checksum_tree_blocks_verify_proofs(fl.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(), m,
                                                            fp.data(), fr.data(), nullptr, mask & 1 ? bad.data() : nullptr,
                                                            mask & 2 ? rows.data() : nullptr, 4, &count,
                                                            mask == 3 ? stats : nullptr, 1 + mask) == SD_OK);
            CHECK(count == 4);
            if (mask & 1) CHECK(memcmp(bad.data(), want_bad.data(), m) == 0 && bad[m] == 0xA5);
            if (mask & 2) CHECK(std::equal(want_rows.begin(), want_rows.end(), rows.begin()) && rows[8] == 0xA5A5);
        }
        CHECK(stats[0] == b.n() && stats[1] == m && stats[2] == 4 && stats[3] == 3);
        std::fill(rows.begin(), rows.end(), 0xA5A5);
        count = 0;
        CHECK(sd_cpu_checksum_tree_blocks_verify_proofs(fl.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(), m,
                                                        fp.data(), fr.data(), nullptr, nullptr, rows.data(), 3, &count, stats,
                                                        2) == SD_ERR_CAPACITY);
        CHECK(count == 4 && stats[2] == 4 && std::all_of(rows.begin(), rows.end(), [](uint64_t x) { return x == 0xA5A5; }));
    }
}

static void test_proofs_levels_and_refusals() {
    // levels alone: random nodes, nb = 255, 256, 257, 513; an unlisted file's level is never read
    const uint32_t k = 17;
    const std::vector<uint64_t> nbs = {255, 256, 300, 257, 513};
    std::vector<uint64_t> lens, base(1, 0);
    for (uint64_t nb : nbs) lens.push_back(nb << k), base.push_back(base.back() + nb);
    bytes level(32 * base.back());
    for (size_t i = 0; i < level.size(); i += 8) {
        const uint64_t v = mix(77, i);
        memcpy(level.data() + i, &v, 8);
    }
    std::vector<uint64_t> rows;
    for (size_t f = 0; f < nbs.size(); f++)
        if (f != 2)
            for (uint64_t j : {uint64_t(0), uint64_t(1), nbs[f] / 2, uint64_t(254), nbs[f] - 2, nbs[f] - 1}) rows.push_back(f), rows.push_back(j);
    const size_t m = rows.size() / 2;
    std::vector<uint64_t> pb(m + 1, 0);
    for (size_t r = 0; r < m; r++) {
        uint32_t e = 0;
        CHECK(sd_checksum_tree_proof_entries(lens[rows[2 * r]], k, rows[2 * r + 1], &e) == SD_OK);
        pb[r + 1] = pb[r] + e;
    }
    uint32_t e = 0;
    CHECK(sd_checksum_tree_proof_entries(513ull << k, k, 512, &e) == SD_OK && e == 1);
    CHECK(sd_checksum_tree_proof_entries(513ull << k, k, 0, &e) == SD_OK && e == 10);
    CHECK(sd_checksum_tree_proof_entries(5ull << k, k, 4, &e) == SD_OK && e == 1);
    CHECK(sd_checksum_tree_proof_entries(3ull << k, k, 2, &e) == SD_OK && e == 1);
    bytes proofs(32 * pb[m]), again(32 * pb[m]);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), k, rows.data(), m, proofs.data()) == SD_OK);
    for (size_t r = 0; r < m; r++) {
        const uint64_t f = rows[2 * r], j = rows[2 * r + 1];
        std::vector<cv_t> lvl;
        for (uint64_t i = base[f]; i < base[f + 1]; i++) lvl.push_back(m_get(level.data() + 32 * i));
        size_t used = 0;
        CHECK(m_climb(lvl[j], proofs.data() + 32 * pb[r], nbs[f], j, &used) == m_merge(lvl, true));
        CHECK(used == pb[r + 1] - pb[r]);
    }
    bytes garbage = level;
    std::fill(garbage.begin() + 32 * base[2], garbage.begin() + 32 * base[3], 0x5A);
    CHECK(sd_cpu_checksum_tree_blocks_prove(garbage.data(), lens.data(), lens.size(), k, rows.data(), m, again.data()) == SD_OK);
    CHECK(again == proofs);
    // refusals: nothing written
    std::fill(again.begin(), again.end(), 0xA5);
    e = 7;
    CHECK(sd_checksum_tree_proof_entries(1ull << k, k, 1, &e) == SD_ERR_INVALID);
    CHECK(sd_checksum_tree_proof_entries(0, k, 1, &e) == SD_ERR_INVALID);
    for (uint32_t bad_k : {0u, 16u, 21u, ~0u}) CHECK(sd_checksum_tree_proof_entries(1ull << 30, bad_k, 0, &e) == SD_ERR_INVALID);
    CHECK(sd_checksum_tree_proof_entries(1ull << 30, k, 0, nullptr) == SD_ERR_INVALID && e == 7);
    const uint64_t no_file[2] = {5, 0}, no_block[2] = {0, 255};
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), k, no_file, 1, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), k, no_block, 1, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), 16, rows.data(), m, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(nullptr, lens.data(), lens.size(), k, rows.data(), m, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), nullptr, lens.size(), k, rows.data(), m, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), k, nullptr, m, again.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_blocks_prove(level.data(), lens.data(), lens.size(), k, rows.data(), m, nullptr) == SD_ERR_INVALID);
    CHECK(std::all_of(again.begin(), again.end(), [](uint8_t x) { return x == 0xA5; }));
    const uint64_t B = 1ull << k;
    batch_t b;
    b.build(k, {100, B + 1}, 3);
    list_t l;
    l.add(b, 0, 0), l.add(b, 1, 1);
    const answer_t want = model(b);
    uint8_t pf[32];
    uint64_t count = 0;
    CHECK(sd_cpu_checksum_tree_blocks_prove(want.nodes.data(), b.lens.data(), 2, k, l.rows.data(), 2, pf) == SD_OK);
    auto ver = [&](const uint8_t* d, const uint64_t* of, const uint8_t* p, const uint8_t* rt) {
        return sd_cpu_checksum_tree_blocks_verify_proofs(d, b.lens.data(), 2, k, l.rows.data(), of, 2, p, rt, nullptr, nullptr,
                                                         nullptr, 0, &count, nullptr, 1);
    };
    const uint64_t odd[2] = {0, l.offs[1] + 8};
    CHECK(ver(l.data.data(), l.offs.data(), pf, want.roots.data()) == SD_OK && count == 0);
    CHECK(ver(nullptr, l.offs.data(), pf, want.roots.data()) == SD_ERR_INVALID);
    CHECK(ver(l.data.data(), nullptr, pf, want.roots.data()) == SD_ERR_INVALID);
    CHECK(ver(l.data.data(), odd, pf, want.roots.data()) == SD_ERR_INVALID);
    CHECK(ver(l.data.data(), l.offs.data(), nullptr, want.roots.data()) == SD_ERR_INVALID);
    CHECK(ver(l.data.data(), l.offs.data(), pf, nullptr) == SD_ERR_INVALID);
    // an empty list: every call does nothing
    uint64_t stats[4] = {9, 9, 9, 9};
    count = 9;
    CHECK(sd_cpu_checksum_tree_blocks_prove(nullptr, b.lens.data(), 2, k, nullptr, 0, nullptr) == SD_OK);
    CHECK(sd_cpu_checksum_tree_blocks_verify_proofs(nullptr, b.lens.data(), 2, k, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr, 0, &count, stats, 1) == SD_OK);
    CHECK(count == 0 && stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0);
}

static void test_proofs_concurrent_calls() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t b;
    b.build(k, {B + 1, 4 * B + 77, 8 * B + 1, 5}, 61);
    const answer_t want = model(b);
    list_t l;
    l.every(b, 6);
    const size_t m = l.m();
    size_t total = 0;
    for (size_t r = 0; r < m; r++) {
        uint32_t e = 0;
        CHECK(sd_checksum_tree_proof_entries(b.lens[l.rows[2 * r]], k, l.rows[2 * r + 1], &e) == SD_OK);
        total += e;
    }
    bytes proofs(32 * total);
    CHECK(sd_cpu_checksum_tree_blocks_prove(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, proofs.data()) == SD_OK);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            bytes mine(32 * total);
            uint64_t count = 9;
            int good = sd_cpu_checksum_tree_blocks_prove(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, mine.data()) == SD_OK;
            good &= mine == proofs;
            good &= sd_cpu_checksum_tree_blocks_verify_proofs(l.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(), m,
                                                              mine.data(), want.roots.data(), nullptr, nullptr, nullptr, 0, &count,
                                                              nullptr, 1 + t) == SD_OK;
            ok[t] = good && count == 0;
        });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

// ---------------------------------------------------------------- range proofs
// the model's climb: blocks [a, b) through `proof` to the root they claim (include/sd_cas.h, range proofs)
static cv_t m_range_climb(std::vector<cv_t> cur, const uint8_t* proof, uint64_t nb, uint64_t a, uint64_t b, size_t* used) {
    size_t at = 0;
    uint64_t lo = a, hi = b - 1;
    for (uint64_t n = nb; n > 1; n = (n + 1) / 2, lo >>= 1, hi >>= 1) {
        if (lo & 1) cur.insert(cur.begin(), m_get(proof + 32 * at++));
        if (!(hi & 1) && hi + 1 < n) cur.push_back(m_get(proof + 32 * at++));
        std::vector<cv_t> nxt;
        for (size_t i = 0; i + 1 < cur.size(); i += 2) nxt.push_back(m_parent(cur[i], cur[i + 1], n == 2));
        if (cur.size() & 1) nxt.push_back(cur.back());
        cur.swap(nxt);
    }
    *used = at;
    return cur[0];
}

static void test_ranges() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t b;  // nb = 1 (empty), 2, 3, 5, 9 with a 1-byte trailing block
    b.build(k, {0, B + 1, 2 * B + 4097, 4 * B + 77, 8 * B + 1}, 71);
    const answer_t want = model(b);
    // every range of every file, each row with bytes of its own
    list_t l;
    std::vector<uint64_t> rb(1, 0);
    std::vector<std::array<uint64_t, 3>> rg;
    for (size_t f = 0; f < b.n(); f++) {
        const uint64_t nb = b.base[f + 1] - b.base[f];
        for (uint64_t a = 0; a < nb; a++)
            for (uint64_t e = a + 1; e <= nb; e++) {
                for (uint64_t j = a; j < e; j++) l.add(b, f, j);
                rb.push_back(l.m());
                rg.push_back({f, a, e});
            }
    }
    const size_t m = l.m(), q = rg.size();
    std::vector<uint64_t> pb(q + 1, 0);
    for (size_t i = 0; i < q; i++) {
        uint32_t e = 99;
        CHECK(sd_checksum_tree_range_proof_entries(b.lens[rg[i][0]], k, rg[i][1], rg[i][2] - rg[i][1], &e) == SD_OK);
        uint32_t h = 0;
        for (uint64_t n = b.base[rg[i][0] + 1] - b.base[rg[i][0]]; n > 1; n = (n + 1) / 2) h++;
        CHECK(e <= 2 * h);
        pb[i + 1] = pb[i] + e;
    }
    bytes proofs(32 * pb[q] + 32, 0xA5);  // one guard row
    CHECK(sd_cpu_checksum_tree_blocks_prove_ranges(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, rb.data(), q,
                                                   proofs.data()) == SD_OK);
    CHECK(std::all_of(proofs.end() - 32, proofs.end(), [](uint8_t x) { return x == 0xA5; }));
    for (size_t i = 0; i < q; i++) {  // every proof climbs to the model's root, using exactly its entries
        const uint64_t f = rg[i][0], a = rg[i][1], e = rg[i][2];
        std::vector<cv_t> cur;
        for (uint64_t j = a; j < e; j++) cur.push_back(m_get(want.nodes.data() + 32 * (b.base[f] + j)));
        size_t used = 0;
        CHECK(m_range_climb(cur, proofs.data() + 32 * pb[i], b.base[f + 1] - b.base[f], a, e, &used) == m_get(want.roots.data() + 32 * f));
        CHECK(used == pb[i + 1] - pb[i]);
        if (e == a + 1) {  // one block: byte for byte the block proof
            const uint64_t row[2] = {f, a};
            bytes one(32 * used + 32, 0xA5);
            CHECK(sd_cpu_checksum_tree_blocks_prove(want.nodes.data(), b.lens.data(), b.n(), k, row, 1, one.data()) == SD_OK);
            CHECK(memcmp(one.data(), proofs.data() + 32 * pb[i], 32 * used) == 0);
        }
        if (a == 0 && e == b.base[f + 1] - b.base[f]) CHECK(used == 0);  // the whole file: empty
    }
    // verify: clean, then a flipped entry, a flipped byte of the trailing block, the capacity rule
    bytes nodes(32 * m + 32, 0xA5), bad(q + 1, 0xA5);
    std::vector<uint64_t> out(3 * q + 3, 0xA5A5);
    uint64_t count = 9, stats[4];
    auto ver = [&](const bytes& d, const bytes& p, uint64_t cap, int nt) {
        return sd_cpu_checksum_tree_blocks_verify_range_proofs(d.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(), m,
                                                               rb.data(), q, p.data(), want.roots.data(), nodes.data(), bad.data(),
                                                               out.data(), cap, &count, stats, nt);
    };
    CHECK(ver(l.data, proofs, q, 3) == SD_OK && count == 0);
    CHECK(stats[0] == b.n() && stats[1] == q && stats[2] == 0 && stats[3] == 0);
    CHECK(std::all_of(bad.begin(), bad.begin() + q, [](uint8_t x) { return x == 0; }) && bad[q] == 0xA5);
    CHECK(std::all_of(out.begin(), out.end(), [](uint64_t x) { return x == 0xA5A5; }));
    for (size_t r = 0; r < m; r++)
        CHECK(memcmp(nodes.data() + 32 * r, want.nodes.data() + 32 * (b.base[l.rows[2 * r]] + l.rows[2 * r + 1]), 32) == 0);
    CHECK(std::all_of(nodes.end() - 32, nodes.end(), [](uint8_t x) { return x == 0xA5; }));
    size_t ie = 0, ib = 0;  // [2, 5) of the nb = 9 file (entries at two levels); a range that ends with its last block
    for (size_t i = 0; i < q; i++) {
        if (rg[i][0] == 4 && rg[i][1] == 2 && rg[i][2] == 5) ie = i;
        if (rg[i][0] == 4 && rg[i][1] == 6 && rg[i][2] == 9) ib = i;
    }
    CHECK(pb[ie + 1] - pb[ie] >= 2);
    bytes fp = proofs;
    fp[32 * (pb[ie] + 1) + 9] ^= 1;
    list_t fl = l;
    fl.data[fl.offs[rb[ib + 1] - 1]] ^= 0x80;  // the 1-byte trailing block
    CHECK(ver(fl.data, fp, q, 2) == SD_OK && count == 2 && stats[2] == 2 && stats[3] == 1);
    const size_t i0 = std::min(ie, ib), i1 = std::max(ie, ib);
    for (size_t i = 0; i < q; i++) CHECK(bad[i] == (i == ie || i == ib));
    CHECK(out[0] == 4 && out[1] == rg[i0][1] && out[2] == rg[i0][2] - rg[i0][1]);
    CHECK(out[3] == 4 && out[4] == rg[i1][1] && out[5] == rg[i1][2] - rg[i1][1] && out[6] == 0xA5A5);
    std::fill(out.begin(), out.end(), 0xA5A5);
    CHECK(ver(fl.data, fp, 1, 1) == SD_ERR_CAPACITY && count == 2 && stats[2] == 2);
    CHECK(std::all_of(out.begin(), out.end(), [](uint64_t x) { return x == 0xA5A5; }));
    // refusals: a gap, an empty range, base[q] != m, two ranges merged (non-consecutive blocks, then two files)
    auto refused = [&](std::vector<uint64_t> base) {
        return sd_cpu_checksum_tree_blocks_verify_range_proofs(l.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(),
                                                               m, base.data(), base.size() - 1, proofs.data(), want.roots.data(),
                                                               nullptr, nullptr, nullptr, 0, &count, nullptr, 1) == SD_ERR_INVALID &&
               sd_cpu_checksum_tree_blocks_prove_ranges(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, base.data(),
                                                        base.size() - 1, fp.data()) == SD_ERR_INVALID;
    };
    std::vector<uint64_t> w = rb;
    w[0] = 1;
    CHECK(refused(w));
    w = rb, w.insert(w.begin() + 3, w[3]);
    CHECK(refused(w));
    w = rb, w.back() -= 1;
    CHECK(refused(w));
    w = rb, w.erase(w.begin() + ie + 1);
    CHECK(refused(w));
    w = rb, w.erase(w.begin() + 1);  // the empty file's block and block 0 of the next file
    CHECK(refused(w));
    CHECK(refused({0}));
    uint32_t e = 7;
    CHECK(sd_checksum_tree_range_proof_entries(8 * B, k, 0, 0, &e) == SD_ERR_INVALID);
    CHECK(sd_checksum_tree_range_proof_entries(8 * B, k, 7, 2, &e) == SD_ERR_INVALID);
    CHECK(sd_checksum_tree_range_proof_entries(8 * B, 16, 0, 1, &e) == SD_ERR_INVALID);
    CHECK(sd_checksum_tree_range_proof_entries(8 * B, k, 0, 1, nullptr) == SD_ERR_INVALID && e == 7);
    // an empty list
    count = 9;
    const uint64_t zero = 0;
    CHECK(sd_cpu_checksum_tree_blocks_prove_ranges(nullptr, b.lens.data(), b.n(), k, nullptr, 0, &zero, 0, nullptr) == SD_OK);
    CHECK(sd_cpu_checksum_tree_blocks_verify_range_proofs(nullptr, b.lens.data(), b.n(), k, nullptr, nullptr, 0, nullptr, 0, nullptr,
                                                          nullptr, nullptr, nullptr, nullptr, 0, &count, stats, 1) == SD_OK);
    CHECK(count == 0 && stats[1] == 0);
}

// ranges across the groups of 256 (the device's plan, run group by group on the host): a level of
// random nodes of nb = 513 and 65 537, proofs against the model's climb; and [254, 258) of the first
// verified from real bytes, its nodes spliced into the level
static void test_ranges_across_groups() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    const std::vector<uint64_t> nbs = {513, 65537};
    std::vector<uint64_t> lens, base(1, 0);
    for (uint64_t nb : nbs) lens.push_back(nb << k), base.push_back(base.back() + nb);
    bytes level(32 * base.back());
    for (size_t i = 0; i < level.size(); i += 8) {
        const uint64_t v = mix(79, i);
        memcpy(level.data() + i, &v, 8);
    }
    // the bytes of [254, 258) of file 0, and their nodes into the level
    bytes data(4 * B + 64);
    for (size_t i = 0; i < data.size(); i += 8) {
        const uint64_t v = mix(80, i);
        memcpy(data.data() + i, &v, std::min<size_t>(8, data.size() - i));
    }
    const uint64_t brow[8] = {0, 254, 0, 255, 0, 256, 0, 257}, boff[4] = {0, B, 2 * B, 3 * B};
    CHECK(sd_cpu_checksum_tree_blocks(data.data(), lens.data(), 2, k, brow, boff, 4, level.data() + 32 * 254, 2) == SD_OK);
    std::vector<std::array<uint64_t, 3>> rg = {{0, 254, 258}, {0, 255, 257}, {0, 0, 513}, {0, 1, 512}, {0, 256, 512}, {0, 512, 513},
                                               {1, 65535, 65537}, {1, 1, 65536}, {1, 65536, 65537}, {1, 300, 301}};
    std::vector<uint64_t> rows, rb(1, 0);
    for (const auto& r : rg) {
        for (uint64_t j = r[1]; j < r[2]; j++) rows.push_back(r[0]), rows.push_back(j);
        rb.push_back(rows.size() / 2);
    }
    const size_t m = rows.size() / 2, q = rg.size();
    std::vector<uint64_t> pb(q + 1, 0);
    for (size_t i = 0; i < q; i++) {
        uint32_t e = 0;
        CHECK(sd_checksum_tree_range_proof_entries(lens[rg[i][0]], k, rg[i][1], rg[i][2] - rg[i][1], &e) == SD_OK);
        pb[i + 1] = pb[i] + e;
    }
    bytes proofs(32 * pb[q] + 32, 0xA5);
    CHECK(sd_cpu_checksum_tree_blocks_prove_ranges(level.data(), lens.data(), 2, k, rows.data(), m, rb.data(), q, proofs.data()) == SD_OK);
    CHECK(std::all_of(proofs.end() - 32, proofs.end(), [](uint8_t x) { return x == 0xA5; }));
    cv_t root[2];
    for (size_t f = 0; f < 2; f++) {
        std::vector<cv_t> lvl;
        for (uint64_t i = base[f]; i < base[f + 1]; i++) lvl.push_back(m_get(level.data() + 32 * i));
        root[f] = m_merge(lvl, true);
    }
    for (size_t i = 0; i < q; i++) {
        const uint64_t f = rg[i][0];
        std::vector<cv_t> cur;
        for (uint64_t j = rg[i][1]; j < rg[i][2]; j++) cur.push_back(m_get(level.data() + 32 * (base[f] + j)));
        size_t used = 0;
        CHECK(m_range_climb(cur, proofs.data() + 32 * pb[i], nbs[f], rg[i][1], rg[i][2], &used) == root[f]);
        CHECK(used == pb[i + 1] - pb[i]);
    }
    // the first two ranges as a list of their own over the real bytes: two groups of one pass, two passes
    bytes roots(64);
    m_put(root[0], roots.data()), m_put(root[1], roots.data() + 32);
    const uint64_t vrow[12] = {0, 254, 0, 255, 0, 256, 0, 257, 0, 255, 0, 256}, voff[6] = {0, B, 2 * B, 3 * B, B, 2 * B};
    const uint64_t vrb[3] = {0, 4, 6};
    uint64_t count = 9, stats[4];
    uint8_t bad[2];
    CHECK(sd_cpu_checksum_tree_blocks_verify_range_proofs(data.data(), lens.data(), 2, k, vrow, voff, 6, vrb, 2, proofs.data(),
                                                          roots.data(), nullptr, bad, nullptr, 0, &count, stats, 2) == SD_OK);
    CHECK(count == 0 && stats[1] == 2 && !bad[0] && !bad[1]);
    data[3 * B + 5] ^= 4;  // block 257: only [254, 258)
    CHECK(sd_cpu_checksum_tree_blocks_verify_range_proofs(data.data(), lens.data(), 2, k, vrow, voff, 6, vrb, 2, proofs.data(),
                                                          roots.data(), nullptr, bad, nullptr, 0, &count, stats, 2) == SD_OK);
    CHECK(count == 1 && bad[0] == 1 && bad[1] == 0);
}

static void test_ranges_concurrent_calls() {
    const uint32_t k = 17;
    const uint64_t B = 1ull << k;
    batch_t b;
    b.build(k, {4 * B + 77, 8 * B + 1}, 73);
    const answer_t want = model(b);
    list_t l;
    std::vector<uint64_t> rb(1, 0);
    const std::vector<std::array<uint64_t, 3>> rg = {{0, 1, 4}, {1, 0, 9}, {1, 3, 8}, {0, 4, 5}};
    for (const auto& r : rg) {
        for (uint64_t j = r[1]; j < r[2]; j++) l.add(b, r[0], j);
        rb.push_back(l.m());
    }
    const size_t m = l.m(), q = rb.size() - 1;
    bytes proofs(32 * 2 * 4 * q);
    CHECK(sd_cpu_checksum_tree_blocks_prove_ranges(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, rb.data(), q,
                                                   proofs.data()) == SD_OK);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            bytes mine(proofs.size());
            uint64_t count = 9;
            int good = sd_cpu_checksum_tree_blocks_prove_ranges(want.nodes.data(), b.lens.data(), b.n(), k, l.rows.data(), m, rb.data(),
                                                                q, mine.data()) == SD_OK;
            good &= mine == proofs;
            good &= sd_cpu_checksum_tree_blocks_verify_range_proofs(l.data.data(), b.lens.data(), b.n(), k, l.rows.data(), l.offs.data(),
                                                                    m, rb.data(), q, mine.data(), want.roots.data(), nullptr, nullptr,
                                                                    nullptr, 0, &count, nullptr, 1 + t) == SD_OK;
            ok[t] = good && count == 0;
        });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

int main() {
    test_ranges();
    test_ranges_across_groups();
    test_ranges_concurrent_calls();
    test_proofs();
    test_proofs_levels_and_refusals();
    test_proofs_concurrent_calls();
    test_blocks();
    test_blocks_verify_and_update();
    test_blocks_refusals_and_empty();
    test_blocks_concurrent_calls();
    test_levels_and_roots();
    test_position_rule();
    test_verify();
    test_refusals_and_empty();
    test_concurrent_calls();
    if (g_fail) {
        printf("checksum_tree_selftest: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("checksum_tree_selftest: ok\n");
    return 0;
}
