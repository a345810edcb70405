// dedup_confirm_selftest.cpp -- sd_cpu_dedup_confirm (dedup_confirm_host.cpp) against a std::map
// model (key, 32 bytes) -> members on the rules of tests/dedup_confirm_cases.py: seeded pools at
// the sizes around a wave, a tile and two tiles, with and without a validity array; a class of
// 700 among singles; tails A, B, A behind equal first 8 bytes, and tails that differ in byte 8 or
// byte 31 only; the byte order of the sets (00 01 against 01 00, 7f against 80, before and after
// byte 8); the keys 0 and 2^64 - 1 under checksums all 00 and all ff beside invalid files of the
// largest key and checksum; an invalid file first of its key and one equal to a confirmed class;
// the capacity rule with pre-filled buffers and every combination of NULL outputs; the refusals;
// m == 0; "confirm_full_sort" beside the learned-route generation; and concurrent calls.  A
// program of its own: built plain for the CPU suite (`make dedup-confirm-selftest`,
// tests/test_dedup_confirm.py) and under ASan + UBSan and TSan (`make sanitize-dedup-confirm`,
// logs in profiles/dedup_confirm/).
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
typedef std::array<uint8_t, 32> sum_t;  // operator< is lexicographic over unsigned bytes = memcmp
static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ull;
static const uint64_t M64 = ~0ull;

static uint64_t mix(uint64_t seed, uint64_t i) {  // splitmix64
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct case_t {
    vec keys;
    bytes hashes;  // m x 32
    bytes valid;   // m, or empty = NULL
    size_t m() const { return keys.size(); }
    const uint8_t* v() const { return valid.empty() ? nullptr : valid.data(); }
    void add(uint64_t k, const sum_t& h, int ok = 1) {
        keys.push_back(k);
        hashes.insert(hashes.end(), h.begin(), h.end());
        valid.push_back((uint8_t)ok);
    }
    sum_t sum(size_t i) const {
        sum_t s;
        memcpy(s.data(), hashes.data() + 32 * i, 32);
        return s;
    }
};

static sum_t sum_of(uint64_t seed) {
    sum_t s;
    for (int w = 0; w < 4; w++) {
        const uint64_t x = mix(seed, (uint64_t)w);
        memcpy(s.data() + 8 * w, &x, 8);
    }
    return s;
}
static sum_t filled(uint8_t b) {
    sum_t s;
    s.fill(b);
    return s;
}

struct answer_t {
    vec rep, size, sets, stats;
    bytes verdict;
};

// the rule, by maps
static answer_t model(const case_t& c) {
    const size_t m = c.m();
    std::map<uint64_t, vec> groups;
    std::map<std::pair<uint64_t, sum_t>, vec> classes;
    for (size_t i = 0; i < m; i++)
        if (c.valid.empty() || c.valid[i]) {
            groups[c.keys[i]].push_back(i);
            classes[{c.keys[i], c.sum(i)}].push_back(i);
        }
    answer_t a;
    a.rep.assign(m, M64), a.size.assign(m, 0), a.verdict.assign(m, SD_CONFIRM_INVALID), a.stats.assign(8, 0);
    std::map<uint64_t, uint64_t> per_group;
    for (const auto& e : classes) {  // ascending (key, bytes): the order of the sets
        const vec& mem = e.second;
        const uint64_t gsize = groups[e.first.first].size();
        for (uint64_t i : mem) {
            a.rep[i] = mem[0], a.size[i] = mem.size();
            a.verdict[i] = gsize == 1 ? SD_CONFIRM_SINGLE : mem.size() >= 2 ? SD_CONFIRM_CONFIRMED : SD_CONFIRM_REFUTED;
        }
        per_group[e.first.first]++;
        a.stats[3]++;
        if (mem.size() >= 2) {
            a.sets.insert(a.sets.end(), {e.first.first, mem[0], (uint64_t)mem.size()});
            a.stats[4]++, a.stats[5] += mem.size();
        } else if (gsize >= 2) {
            a.stats[6]++;
        }
    }
    for (const auto& g : groups) {
        a.stats[0] += g.second.size(), a.stats[1]++;
        if (g.second.size() >= 2) a.stats[2]++, a.stats[7] += per_group[g.first] >= 2;
    }
    return a;
}

static answer_t run(const case_t& c) {
    const size_t m = c.m();
    answer_t a;
    a.rep.assign(m + 2, FILL), a.size.assign(m + 2, FILL), a.verdict.assign(m + 2, 0xA5), a.stats.assign(8, FILL);
    a.sets.assign(3 * (m / 2 + 2), FILL);
    uint64_t n = FILL;
    CHECK(sd_cpu_dedup_confirm(c.keys.data(), c.hashes.data(), c.v(), m, a.rep.data(), a.size.data(), a.verdict.data(),
                               a.sets.data(), m / 2, &n, a.stats.data()) == SD_OK);
    CHECK(n <= m / 2);
    // nothing past m per-file rows, nothing past n set rows
    CHECK(a.rep[m] == FILL && a.rep[m + 1] == FILL && a.size[m] == FILL && a.verdict[m] == 0xA5);
    for (size_t i = 3 * (size_t)std::min<uint64_t>(n, m / 2); i < a.sets.size(); i++) CHECK(a.sets[i] == FILL);
    a.rep.resize(m), a.size.resize(m), a.verdict.resize(m), a.sets.resize(3 * (size_t)std::min<uint64_t>(n, m / 2));
    return a;
}

static void check_case(const case_t& c, const char* what) {
    const answer_t want = model(c), got = run(c);
    const bool same = got.rep == want.rep && got.size == want.size && got.verdict == want.verdict &&
                      got.sets == want.sets && got.stats == want.stats;
    if (!same) printf("case %s (m = %zu) differs from the model\n", what, c.m());
    CHECK(same);
    const vec& s = want.stats;
    CHECK(s[0] == (s[1] - s[2]) + s[5] + s[6] && s[3] == (s[1] - s[2]) + s[4] + s[6]);
}

// m files over about m / 3 keys with two checksums each
static case_t pooled(size_t m, uint64_t seed, bool with_valid) {
    case_t c;
    const uint64_t nk = m / 3 + 1;
    for (size_t i = 0; i < m; i++) {
        const uint64_t w = mix(seed, i) % nk;
        c.add(mix(seed + 1, w), sum_of(seed + 2 + 2 * w + (mix(seed + 3, i) & 1)), !with_valid || mix(seed + 4, i) % 10 != 0);
    }
    if (!with_valid) c.valid.clear();
    return c;
}

static case_t tied(const std::vector<sum_t>& sums, uint64_t key = 0x123456789ABCDEF0ull) {
    case_t c;
    for (const sum_t& s : sums) c.add(key, s);
    c.valid.clear();
    return c;
}

static void test_sizes() {
    for (size_t m : {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 4099}) {
        check_case(pooled(m, 100 + m, false), "pooled");
        check_case(pooled(m, 200 + m, true), "pooled, valid");
    }
    case_t c = pooled(1000, 300, false);  // a class of 700 among singles
    for (size_t i = 0; i < 1000; i++) {
        c.keys[i] = mix(301, i);
        const sum_t s = i % 10 < 7 ? sum_of(77) : sum_of(1000 + i);
        if (i % 10 < 7) c.keys[i] = 42;
        memcpy(c.hashes.data() + 32 * i, s.data(), 32);
    }
    check_case(c, "long class");
    CHECK(model(c).stats[5] == 700);
    case_t none = pooled(300, 320, true);
    std::fill(none.valid.begin(), none.valid.end(), 0);
    check_case(none, "all invalid");
    CHECK(model(none).stats == vec(8, 0));
}

static void test_ties_and_order() {
    sum_t A = filled(0x11), B = filled(0x22);
    for (int i = 0; i < 8; i++) A[i] = B[i] = (uint8_t)i;  // equal first 8 bytes
    const case_t aba = tied({A, B, A});
    check_case(aba, "A B A");
    const answer_t a = run(aba);
    CHECK((a.rep == vec{0, 1, 0}) && (a.size == vec{2, 1, 2}) && (a.sets == vec{aba.keys[0], 0, 2}));
    CHECK((a.verdict == bytes{SD_CONFIRM_CONFIRMED, SD_CONFIRM_REFUTED, SD_CONFIRM_CONFIRMED}));
    sum_t A8 = A, A31 = A;
    A8[8] ^= 1, A31[31] ^= 1;
    check_case(tied({A, A8, A, A8, A}), "byte 8");
    check_case(tied({A, A31, A31, A}), "byte 31");
    CHECK(run(tied({A, A31, A31, A})).stats[4] == 2);
    check_case(tied({A, A, A, A, A}), "uniform");
    // the sets of one key ascend as memcmp orders the checksums; files listed descending
    struct { int at; uint8_t hi0, hi1, lo0, lo1; } orders[] = {
        {0, 0x01, 0x00, 0x00, 0x01}, {0, 0x80, 0x00, 0x7f, 0x00}, {8, 0x01, 0x00, 0x00, 0x01}, {30, 0x00, 0x80, 0x00, 0x7f}};
    for (const auto& o : orders) {
        sum_t hi = filled(0x09), lo = filled(0x09);
        hi[o.at] = o.hi0, hi[o.at + 1] = o.hi1, lo[o.at] = o.lo0, lo[o.at + 1] = o.lo1;
        const case_t c = tied({hi, hi, lo, lo}, 5);
        check_case(c, "byte order");
        CHECK((run(c).sets == vec{5, 2, 2, 5, 0, 2}));
    }
    sum_t lowbyte_hi = filled(0), lowbyte_lo = filled(0);  // a little-endian word compare gets this wrong
    lowbyte_hi[0] = 1, lowbyte_lo[7] = 2;
    CHECK((run(tied({lowbyte_hi, lowbyte_hi, lowbyte_lo, lowbyte_lo}, 5)).sets == vec{5, 2, 2, 5, 0, 2}));
}

static void test_extremes_and_invalid() {
    case_t c;
    for (int rnd = 0; rnd < 2; rnd++)
        for (uint64_t k : {(uint64_t)0, M64})
            for (uint8_t b : {(uint8_t)0x00, (uint8_t)0xFF}) {
                c.add(M64, filled(0xFF), 0);
                c.add(k, filled(b));
            }
    c.add(M64, filled(0xFF), 0);
    check_case(c, "extremes");
    CHECK((model(c).stats == vec{8, 2, 2, 4, 4, 8, 0, 2}));
    const sum_t h0 = sum_of(1), h1 = sum_of(2), h2 = sum_of(3);
    case_t first;  // an invalid file with the smallest index of its key
    first.add(9, h0, 0), first.add(9, h0), first.add(9, h0), first.add(4, h1);
    check_case(first, "invalid first");
    CHECK((run(first).rep == vec{M64, 1, 1, 3}));
    case_t same;  // an invalid file whose checksum equals a confirmed class's
    same.add(9, h0), same.add(9, h0, 0), same.add(9, h0), same.add(9, h2);
    check_case(same, "invalid equals a class");
    CHECK((run(same).size == vec{2, 0, 2, 1}));
    case_t lone;
    lone.add(9, h0), lone.add(9, h0, 0);
    check_case(lone, "invalid leaves a single");
    CHECK((run(lone).verdict == bytes{SD_CONFIRM_SINGLE, SD_CONFIRM_INVALID}));
}

static void test_capacity_and_nulls() {
    const case_t c = pooled(513, 713, true);
    const answer_t want = model(c);
    const uint64_t n_sets = want.sets.size() / 3;
    CHECK(n_sets >= 3);
    for (uint64_t cap : {n_sets - 1, (uint64_t)0}) {  // short: refused, the per-file outputs complete
        vec rep(c.m(), FILL), size(c.m(), FILL), sets(3 * (n_sets + 2), FILL), stats(8, FILL);
        bytes verdict(c.m(), 0xA5);
        uint64_t n = 0;
        CHECK(sd_cpu_dedup_confirm(c.keys.data(), c.hashes.data(), c.v(), c.m(), rep.data(), size.data(), verdict.data(),
                                   sets.data(), cap, &n, stats.data()) == SD_ERR_CAPACITY);
        CHECK(n == n_sets && sets == vec(3 * (n_sets + 2), FILL));
        CHECK(rep == want.rep && size == want.size && verdict == want.verdict && stats == want.stats);
    }
    for (int mask = 0; mask < 32; mask++) {  // every combination of NULL outputs
        vec rep(c.m(), FILL), size(c.m(), FILL), sets(3 * n_sets, FILL), stats(8, FILL);
        bytes verdict(c.m(), 0xA5);
        uint64_t n = FILL;
        CHECK(sd_cpu_dedup_confirm(c.keys.data(), c.hashes.data(), c.v(), c.m(), mask & 1 ? rep.data() : nullptr,
                                   mask & 2 ? size.data() : nullptr, mask & 4 ? verdict.data() : nullptr,
                                   mask & 8 ? sets.data() : nullptr, mask & 8 ? n_sets : 0, mask & 16 ? &n : nullptr,
                                   mask & 16 ? stats.data() : nullptr) == SD_OK);
        CHECK(rep == (mask & 1 ? want.rep : vec(c.m(), FILL)) && size == (mask & 2 ? want.size : vec(c.m(), FILL)));
        CHECK(verdict == (mask & 4 ? want.verdict : bytes(c.m(), 0xA5)) && sets == (mask & 8 ? want.sets : vec(3 * n_sets, FILL)));
        CHECK(n == (mask & 16 ? n_sets : FILL) && stats == (mask & 16 ? want.stats : vec(8, FILL)));
    }
    uint64_t n = FILL;
    vec stats(8, FILL);
    CHECK(sd_cpu_dedup_confirm(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &n, stats.data()) == SD_OK);
    CHECK(n == 0 && stats == vec(8, 0));
    CHECK(sd_cpu_dedup_confirm(nullptr, c.hashes.data(), nullptr, 4, nullptr, nullptr, nullptr, nullptr, 0, &n, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_dedup_confirm(c.keys.data(), nullptr, nullptr, 4, nullptr, nullptr, nullptr, nullptr, 0, &n, nullptr) == SD_ERR_INVALID);
}

static void test_tuning_key() {
    int v = -1;
    CHECK(sd_cas_get_tuning("confirm_full_sort", &v) == SD_OK && v == 0);
    const uint64_t g0 = split_route_tuning_gen();
    CHECK(sd_cas_set_tuning("confirm_full_sort", 1) == SD_OK && split_route_tuning_gen() == g0);  // no learned route depends on it
    CHECK(sd_cas_get_tuning("confirm_full_sort", &v) == SD_OK && v == 1);
    CHECK(sd_cas_set_tuning("confirm_full_sort", 0) == SD_OK && split_route_tuning_gen() == g0);
}

static void test_concurrent_calls() {  // the call holds no shared state
    const case_t c = pooled(4099, 900, true);
    const answer_t want = model(c);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            const answer_t got = run(c);
            ok[t] = got.rep == want.rep && got.sets == want.sets && got.stats == want.stats;
        });
    for (auto& t : ts) t.join();
    CHECK(ok == std::vector<int>(4, 1));
}

int main() {
    test_sizes();
    test_ties_and_order();
    test_extremes_and_invalid();
    test_capacity_and_nulls();
    test_tuning_key();
    test_concurrent_calls();
    if (g_fail) {
        printf("dedup_confirm_selftest: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("dedup_confirm_selftest: ok\n");
    return 0;
}
