// tree_shared_selftest.cpp -- sd_cpu_checksum_tree_shared (tree_shared_host.cpp) against a
// std::map model (block index, 32 bytes) -> slots on the rules of tests/tree_shared_cases.py: seeded
// batches of crafted levels at the slot counts around a wave, a tile and two tiles, at 128 KiB and
// 1 MiB blocks; only one-node files; empty files; a class of 300; a pair run of 700 blocks; three
// holders of one block; equal nodes at different block indices; tails A, B, A behind equal first 8
// bytes; a shared partial last block, an exact multiple, a last block held by another file than the
// rest of the run; min_blocks below, at and above a pair's count; the capacity rule with pre-filled
// buffers and every combination of NULL outputs; the refusals; n == 0; and concurrent calls.  A
// program of its own: built plain for the CPU suite (`make tree-shared-selftest`,
// tests/test_tree_shared.py) and under ASan + UBSan and TSan (`make sanitize-tree-shared`, logs in
// profiles/tree_shared/).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "sd_host.h"

static int g_fail = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            g_fail++;                                                     \
        }                                                                 \
    } while (0)

typedef std::vector<uint64_t> vec;
typedef std::vector<uint8_t> bytes;
typedef std::array<uint8_t, 32> node_t;
static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ull;

static uint64_t mix(uint64_t seed, uint64_t i) {  // splitmix64
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static node_t node_of(uint64_t seed) {
    node_t s;
    for (int w = 0; w < 4; w++) {
        const uint64_t x = mix(seed, (uint64_t)w);
        memcpy(s.data() + 8 * w, &x, 8);
    }
    return s;
}

struct case_t {
    uint32_t k = 17;
    vec lens, base{0};
    bytes nodes;  // m x 32
    uint64_t B() const { return 1ull << k; }
    size_t n() const { return lens.size(); }
    uint64_t m() const { return base.back(); }
    void add(uint64_t len, uint64_t seed) {  // a file of fresh nodes
        const uint64_t nb = std::max<uint64_t>(1, (len + B() - 1) / B());
        for (uint64_t j = 0; j < nb; j++) {
            const node_t x = node_of(seed * 1000003 + j);
            nodes.insert(nodes.end(), x.begin(), x.end());
        }
        lens.push_back(len);
        base.push_back(base.back() + nb);
    }
    uint8_t* at(size_t f, uint64_t j) { return nodes.data() + 32 * (base[f] + j); }
    void plant(size_t f, size_t g, uint64_t j) { memcpy(at(f, j), at(g, j), 32); }
    node_t node(uint64_t s) const {
        node_t x;
        memcpy(x.data(), nodes.data() + 32 * s, 32);
        return x;
    }
};

struct answer_t {
    vec rep, size, files, pairs, stats;
    bool operator==(const answer_t& o) const {
        return rep == o.rep && size == o.size && files == o.files && pairs == o.pairs && stats == o.stats;
    }
};

// the rule, by maps
static answer_t model(const case_t& c, uint64_t min_blocks = 0) {
    const uint64_t m = c.m();
    std::map<std::pair<uint64_t, node_t>, vec> classes;
    std::vector<size_t> file_of(m);
    for (size_t f = 0; f < c.n(); f++)
        for (uint64_t s = c.base[f]; s < c.base[f + 1]; s++) {
            file_of[s] = f;
            classes[{s - c.base[f], c.node(s)}].push_back(s);  // slots ascend
        }
    answer_t a;
    a.rep.assign(m, 0), a.size.assign(m, 0), a.files.assign(4 * c.n(), 0), a.stats.assign(8, 0);
    a.stats[0] = c.n(), a.stats[1] = m, a.stats[2] = classes.size();
    for (const auto& e : classes) {
        a.stats[3] += e.second.size() >= 2;
        for (uint64_t s : e.second) a.rep[s] = e.second[0], a.size[s] = e.second.size();
    }
    std::map<std::pair<uint64_t, uint64_t>, std::pair<uint64_t, uint64_t>> rows;  // (f, g) -> (blocks, bytes)
    for (uint64_t s = 0; s < m; s++) {
        const size_t f = file_of[s];
        const uint64_t at = (s - c.base[f]) * c.B();
        a.files[4 * f] = c.base[f + 1] - c.base[f];
        a.files[4 * f + 1] += a.size[s] >= 2;
        if (a.rep[s] == s) continue;
        const uint64_t by = c.lens[f] > at ? std::min(c.B(), c.lens[f] - at) : 0;
        a.files[4 * f + 2]++, a.files[4 * f + 3] += by;
        auto& r = rows[{f, file_of[a.rep[s]]}];
        r.first++, r.second += by;
    }
    for (size_t f = 0; f < c.n(); f++) {
        a.stats[4] += a.files[4 * f + 2], a.stats[5] += a.files[4 * f + 3];
        a.stats[6] += a.files[4 * f + 2] != 0, a.stats[7] += a.files[4 * f + 2] == a.files[4 * f];
    }
    for (const auto& r : rows)
        if (r.second.first >= std::max<uint64_t>(1, min_blocks))
            a.pairs.insert(a.pairs.end(), {r.first.first, r.first.second, r.second.first, r.second.second});
    return a;
}

static answer_t run(const case_t& c, uint64_t min_blocks = 0) {
    const uint64_t m = c.m();
    answer_t a;
    a.rep.assign(m + 2, FILL), a.size.assign(m + 2, FILL), a.files.assign(4 * (c.n() + 1), FILL);
    a.pairs.assign(4 * (m + 1), FILL), a.stats.assign(8, FILL);
    uint64_t p = FILL;
    CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), c.n(), c.k, c.nodes.data(), min_blocks, a.rep.data(), a.size.data(),
                                      a.files.data(), a.pairs.data(), m, &p, a.stats.data()) == SD_OK);
    CHECK(p < std::max<uint64_t>(m, 1));
    p = std::min(p, m);
    CHECK(a.rep[m] == FILL && a.rep[m + 1] == FILL && a.size[m] == FILL && a.files[4 * c.n()] == FILL);
    for (size_t i = 4 * (size_t)p; i < a.pairs.size(); i++) CHECK(a.pairs[i] == FILL);
    a.rep.resize(m), a.size.resize(m), a.files.resize(4 * c.n()), a.pairs.resize(4 * (size_t)p);
    return a;
}

static void check_case(const case_t& c, const char* what, uint64_t min_blocks = 0) {
    const answer_t want = model(c, min_blocks), got = run(c, min_blocks);
    if (!(got == want)) printf("case %s (m = %llu) differs from the model\n", what, (unsigned long long)c.m());
    CHECK(got == want);
    const vec& s = want.stats;
    CHECK(s[4] == s[1] - s[2] && s[7] <= s[6] && (c.n() == 0 || want.files[2] == 0));
    if (min_blocks <= 1) {
        uint64_t blocks = 0, by = 0;
        for (size_t r = 0; r < want.pairs.size(); r += 4) blocks += want.pairs[r + 2], by += want.pairs[r + 3];
        CHECK(blocks == s[4] && by == s[5]);
    }
}

// m slots in files of 1 .. 12 blocks (exact multiples, empty files and partial tails), a third of
// the files copying half the blocks they have in common with another file
static case_t pooled(uint64_t m, uint64_t seed, uint32_t k = 17) {
    case_t c;
    c.k = k;
    for (uint64_t left = m, i = 0; left; i++) {
        const uint64_t nb = std::min<uint64_t>(left, 1 + mix(seed, i) % 12), kind = mix(seed + 1, i) % 4;
        c.add(kind == 0 ? nb * c.B() : kind == 1 && nb == 1 ? 0 : (nb - 1) * c.B() + 1 + mix(seed + 2, i) % (c.B() - 1),
              seed * 31 + i);
        left -= nb;
    }
    for (size_t f = 0; f < c.n() && c.n() >= 2; f++) {
        if (mix(seed + 3, f) % 3) continue;
        size_t g = mix(seed + 4, f) % (c.n() - 1);
        g += g >= f;
        const uint64_t common = std::min(c.base[f + 1] - c.base[f], c.base[g + 1] - c.base[g]);
        for (uint64_t j = 0; j < common; j++)
            if (mix(seed + 5 + f, j) & 1) c.plant(f, g, j);
    }
    return c;
}

static void test_sizes() {
    check_case(case_t(), "no files");
    for (uint64_t m : {1, 2, 63, 64, 65, 255, 256, 257, 513, 4099}) {
        check_case(pooled(m, 100 + m), "pooled");
        check_case(pooled(m, 200 + m, 20), "pooled, 1 MiB blocks");
    }
    CHECK(model(pooled(4099, 4199)).stats[4] > 200);
    case_t one;  // only one-node files
    for (int i = 0; i < 60; i++) one.add(1 + 1000 * (uint64_t)i, 300 + (uint64_t)(i % 20));
    check_case(one, "one-node files");
    CHECK(model(one).stats[2] == 20 && model(one).stats[7] == 40);
    case_t empty;  // empty files share their node at 0 bytes
    empty.add(0, 1), empty.add(300000, 2), empty.add(0, 1), empty.add(5, 3), empty.add(0, 1);
    check_case(empty, "empty files");
    CHECK((run(empty).pairs == vec{2, 0, 1, 0, 4, 0, 1, 0}) && run(empty).stats[5] == 0);
}

static void test_classes_and_runs() {
    case_t big;  // a class of 300
    for (int f = 0; f < 300; f++) big.add(big.B() + 1 + (uint64_t)f, 400 + (uint64_t)f);
    for (int f = 1; f < 300; f++) big.plant((size_t)f, 0, 0);
    check_case(big, "class of 300");
    CHECK(run(big).size[0] == 300 && run(big).pairs.size() == 4 * 299);
    case_t longrun;  // a pair run of 700 blocks
    const uint64_t B = longrun.B();
    longrun.add(90 * B + 7, 1), longrun.add(700 * B, 2), longrun.add(40 * B, 3), longrun.add(700 * B, 4);
    longrun.add(100 * B + 9, 5), longrun.add(90 * B + 7, 6);
    for (uint64_t j = 0; j < 700; j++) longrun.plant(3, 1, j);
    for (uint64_t j = 0; j < 91; j++) longrun.plant(5, 0, j);
    for (uint64_t j = 0; j < 40; j += 2) longrun.plant(4, 2, j);
    check_case(longrun, "run of 700");
    CHECK((run(longrun).pairs == vec{3, 1, 700, 700 * B, 4, 2, 20, 20 * B, 5, 0, 91, 90 * B + 7}));
    case_t three;  // three holders: both later ones point at the first
    three.add(3 * B, 1), three.add(4 * B + 1, 2), three.add(2 * B, 3), three.add(5 * B, 4);
    three.plant(1, 0, 1), three.plant(3, 0, 1);
    check_case(three, "three holders");
    CHECK((run(three).pairs == vec{1, 0, 1, B, 3, 0, 1, B}) && run(three).size[1] == 3);
    case_t other;  // equal nodes at different block indices do not match
    other.add(4 * B, 1), other.add(4 * B, 2), other.add(6 * B, 3);
    memcpy(other.at(1, 2), other.at(0, 1), 32), memcpy(other.at(2, 5), other.at(0, 0), 32);
    memcpy(other.at(2, 0), other.at(2, 3), 32);
    check_case(other, "different index");
    CHECK(run(other).stats[4] == 0 && run(other).pairs.empty());
}

static void test_ties() {
    node_t A, Bt;
    A.fill(0x11), Bt.fill(0x22);
    for (int i = 0; i < 8; i++) A[i] = Bt[i] = (uint8_t)i;  // equal first 8 bytes
    case_t c;
    const uint64_t B = c.B();
    c.add(3 * B, 1), c.add(3 * B, 2), c.add(3 * B, 3);
    memcpy(c.at(0, 1), A.data(), 32), memcpy(c.at(1, 1), Bt.data(), 32), memcpy(c.at(2, 1), A.data(), 32);
    check_case(c, "A B A");
    CHECK(run(c).rep[1] == 1 && run(c).rep[4] == 4 && run(c).rep[7] == 1 && (run(c).pairs == vec{2, 0, 1, B}));
    node_t A31 = A;
    A31[31] ^= 1;
    memcpy(c.at(1, 1), A31.data(), 32);
    check_case(c, "byte 31");
    memcpy(c.at(1, 1), A.data(), 32);
    check_case(c, "uniform");
    CHECK(run(c).size[1] == 3);
}

static void test_trailing_and_min_blocks() {
    case_t t;  // two files of equal non-multiple length share the partial last block
    const uint64_t B = t.B();
    t.add(4 * B + 1000, 1), t.add(4 * B + 1000, 2);
    t.plant(1, 0, 0), t.plant(1, 0, 2), t.plant(1, 0, 4);
    check_case(t, "tail shared");
    CHECK((run(t).pairs == vec{1, 0, 3, 2 * B + 1000}));
    case_t x;  // an exact multiple
    x.add(4 * B, 1), x.add(4 * B, 2), x.add(5 * B, 3);
    x.plant(1, 0, 3), x.plant(2, 0, 2), x.plant(2, 0, 3);
    check_case(x, "exact multiple");
    CHECK((run(x).pairs == vec{1, 0, 1, B, 2, 0, 2, 2 * B}));
    case_t o;  // the last partial block's holder is another file than the rest of the run's
    o.add(5 * B, 1), o.add(4 * B + 77, 2), o.add(4 * B + 77, 3), o.add(4 * B + 77, 4);
    for (uint64_t j = 0; j < 4; j++) o.plant(2, 0, j);
    o.plant(2, 1, 4), o.plant(3, 1, 0), o.plant(3, 1, 4), o.plant(3, 0, 2);
    check_case(o, "tail, other holder");
    CHECK((run(o).pairs == vec{2, 0, 4, 4 * B, 2, 1, 1, 77, 3, 0, 1, B, 3, 1, 2, B + 77}) && run(o).stats[7] == 1);
    case_t mb;  // pairs of 1, 3 and 5 blocks
    for (int f = 0; f < 4; f++) mb.add(8 * B, 10 + (uint64_t)f);
    mb.plant(1, 0, 7);
    for (uint64_t j = 0; j < 3; j++) mb.plant(2, 0, j);
    for (uint64_t j = 1; j < 6; j++) mb.plant(3, 1, j);
    const size_t rows[] = {3, 3, 2, 2, 1, 1, 0};
    for (uint64_t need = 0; need < 7; need++) {
        check_case(mb, "min_blocks", need);
        CHECK(run(mb, need).pairs.size() == 4 * rows[need] && run(mb, need).stats == run(mb).stats);
    }
    check_case(pooled(513, 613), "pooled, min_blocks 2", 2);
}

static void test_capacity_and_nulls() {
    const case_t c = pooled(513, 713);
    const answer_t want = model(c);
    const uint64_t m = c.m(), rows = want.pairs.size() / 4;
    CHECK(rows >= 3);
    for (uint64_t cap : {rows - 1, (uint64_t)0}) {  // short: refused, every other output complete
        vec rep(m, FILL), size(m, FILL), files(4 * c.n(), FILL), pairs(4 * (rows + 2), FILL), stats(8, FILL);
        uint64_t p = 0;
        CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), c.n(), c.k, c.nodes.data(), 0, rep.data(), size.data(),
                                          files.data(), pairs.data(), cap, &p, stats.data()) == SD_ERR_CAPACITY);
        CHECK(p == rows && pairs == vec(4 * (rows + 2), FILL));
        CHECK(rep == want.rep && size == want.size && files == want.files && stats == want.stats);
    }
    for (int mask = 0; mask < 32; mask++) {  // every combination of NULL outputs
        vec rep(m, FILL), size(m, FILL), files(4 * c.n(), FILL), pairs(4 * rows, FILL), stats(8, FILL);
        uint64_t p = FILL;
        CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), c.n(), c.k, c.nodes.data(), 0, mask & 1 ? rep.data() : nullptr,
                                          mask & 2 ? size.data() : nullptr, mask & 4 ? files.data() : nullptr,
                                          mask & 8 ? pairs.data() : nullptr, mask & 8 ? rows : 0,
                                          mask & 16 ? &p : nullptr, mask & 16 ? stats.data() : nullptr) == SD_OK);
        CHECK(rep == (mask & 1 ? want.rep : vec(m, FILL)) && size == (mask & 2 ? want.size : vec(m, FILL)));
        CHECK(files == (mask & 4 ? want.files : vec(4 * c.n(), FILL)) && pairs == (mask & 8 ? want.pairs : vec(4 * rows, FILL)));
        CHECK(p == (mask & 16 ? rows : FILL) && stats == (mask & 16 ? want.stats : vec(8, FILL)));
    }
    uint64_t p = FILL;
    vec stats(8, FILL);
    CHECK(sd_cpu_checksum_tree_shared(nullptr, 0, 17, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &p, stats.data()) == SD_OK);
    CHECK(p == 0 && stats == vec(8, 0));
    for (uint32_t k : {0u, 16u, 21u}) {
        CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), c.n(), k, c.nodes.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) == SD_ERR_INVALID);
        CHECK(sd_cpu_checksum_tree_shared(nullptr, 0, k, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) == SD_ERR_INVALID);
    }
    CHECK(sd_cpu_checksum_tree_shared(nullptr, c.n(), 17, c.nodes.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), c.n(), 17, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_checksum_tree_shared(c.lens.data(), (size_t)1 << 32, 17, c.nodes.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, &p, nullptr) == SD_ERR_INVALID);
}

static void test_concurrent_calls() {  // the call holds no shared state
    const case_t c = pooled(4099, 900);
    const answer_t want = model(c);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] { ok[t] = run(c) == want; });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

int main() {
    test_sizes();
    test_classes_and_runs();
    test_ties();
    test_trailing_and_min_blocks();
    test_capacity_and_nulls();
    test_concurrent_calls();
    if (g_fail) {
        printf("tree_shared_selftest: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("tree_shared_selftest: ok\n");
    return 0;
}
