// object_index_duplicates_selftest.cpp -- sd_cpu_object_index_key_links, _duplicates,
// _duplicate_entries and _duplicate_stats (object_index_host.cpp; the rule oi_key_run /
// oi_qualifies of object_index.h, which the kernels share) against a std::map model key ->
// (links, owners, first) kept beside a seeded sequence of inserts and removals: the entry counts
// at which the directory bits change, with runs at both ends of the index and the keys 0 and
// 2^64 - 1; 3000 owners of one key; 70 000 links on one pair; the full cross of thresholds; key
// lists with present, absent, repeated and edge keys; the capacity rule with pre-filled buffers
// and every combination of NULL outputs; the refusals; the shards' rows concatenated; and
// concurrent reads.  A program of its own: built plain for the CPU suite (`make
// object-index-duplicates-selftest`, tests/test_object_index_duplicates.py) and under ASan +
// UBSan and TSan (`make sanitize-object-index-duplicates`, logs in profiles/object_index/).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "object_index.h"
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
typedef std::pair<uint64_t, uint64_t> pair_t;
typedef std::map<pair_t, uint64_t> model_t;  // (key, id) -> links
static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ull;
static const uint64_t RUN = 3000;

// tests/object_index_cases.py splitmix(seed, n)
static vec splitmix(uint64_t seed, size_t n) {
    vec v(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t z = seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        v[i] = z ^ (z >> 31);
    }
    return v;
}

struct index_t {
    sd_cpu_object_index* x = nullptr;
    int nparts, part;
    explicit index_t(int np = 1, int p = 0, int flags = SD_OBJECT_INDEX_OWNERS) : nparts(np), part(p) {
        CHECK(sd_cpu_object_index_create_ex(np, p, flags, &x) == SD_OK);
    }
    ~index_t() { sd_cpu_object_index_destroy(x); }
    index_t(const index_t&) = delete;
    void insert(model_t& m, const vec& k, const vec& v) {
        CHECK(sd_cpu_object_index_insert(x, k.data(), v.data(), k.size(), nullptr) == SD_OK);
        for (size_t i = 0; i < k.size(); i++)
            if (oi_dest_of(k[i], nparts) == (uint32_t)part) m[pair_t(k[i], v[i])]++;
    }
};

// ---- the model: object_index.h, by key
struct group_t {
    uint64_t links = 0, owners = 0, first = 0;
};
static std::map<uint64_t, group_t> groups_of(const model_t& m) {
    std::map<uint64_t, group_t> g;
    for (const auto& e : m) {  // ascending (key, id): a key's first pair carries its smallest id
        group_t& t = g[e.first.first];
        if (t.owners == 0) t.first = e.first.second;
        t.links += e.second, t.owners++;
    }
    return g;
}
static bool qualifies(const group_t& t, uint64_t ml, uint64_t mo) {
    return t.links >= (ml ? ml : 1) && t.owners >= (mo ? mo : 1);
}

// duplicates and duplicate_entries under (ml, mo) against the model: outputs between guards, the
// capacity rule, every combination of NULL outputs
static void check_select(const index_t& ix, const model_t& m, uint64_t ml, uint64_t mo) {
    const std::map<uint64_t, group_t> g = groups_of(m);
    vec wk, wf, wl, wo, ek, ei, el;
    for (const auto& e : g)
        if (qualifies(e.second, ml, mo))
            wk.push_back(e.first), wf.push_back(e.second.first), wl.push_back(e.second.links), wo.push_back(e.second.owners);
    for (const auto& e : m)
        if (qualifies(g.at(e.first.first), ml, mo)) ek.push_back(e.first.first), ei.push_back(e.first.second), el.push_back(e.second);
    const uint64_t n = wk.size(), ne = ek.size();
    const vec* want[4] = {&wk, &wf, &wl, &wo};
    const vec* wante[3] = {&ek, &ei, &el};
    for (unsigned mask = 0; mask < 16; mask++) {  // bit j: output j is given
        vec out[4];
        uint64_t* p[4];
        for (int j = 0; j < 4; j++) out[j].assign(n + 2, FILL), p[j] = (mask >> j) & 1 ? out[j].data() + 1 : nullptr;
        uint64_t count = ~0ull;
        CHECK(sd_cpu_object_index_duplicates(ix.x, ml, mo, p[0], p[1], p[2], p[3], n, &count) == SD_OK && count == n);
        for (int j = 0; j < 4; j++) {
            CHECK(out[j][0] == FILL && out[j][n + 1] == FILL);
            for (uint64_t i = 0; i < n; i++) CHECK(out[j][i + 1] == (p[j] ? (*want[j])[i] : FILL));
        }
        if (mask && n) {  // one short: nothing written, the requirement reported
            uint64_t need = 0;
            CHECK(sd_cpu_object_index_duplicates(ix.x, ml, mo, p[0], p[1], p[2], p[3], n - 1, &need) == SD_ERR_CAPACITY);
            CHECK(need == n);
            for (int j = 0; j < 4; j++)
                for (uint64_t i = 0; i < n; i++) CHECK(out[j][i + 1] == (p[j] ? (*want[j])[i] : FILL));
        }
    }
    for (unsigned mask = 0; mask < 8; mask++) {
        vec out[3];
        uint64_t* p[3];
        for (int j = 0; j < 3; j++) out[j].assign(ne + 2, FILL), p[j] = (mask >> j) & 1 ? out[j].data() + 1 : nullptr;
        uint64_t count = ~0ull;
        CHECK(sd_cpu_object_index_duplicate_entries(ix.x, ml, mo, p[0], p[1], p[2], ne, &count) == SD_OK && count == ne);
        for (int j = 0; j < 3; j++) {
            CHECK(out[j][0] == FILL && out[j][ne + 1] == FILL);
            for (uint64_t i = 0; i < ne; i++) CHECK(out[j][i + 1] == (p[j] ? (*wante[j])[i] : FILL));
        }
        if (mask && ne) {
            vec small(ne + 1, FILL);
            uint64_t need = 0;
            CHECK(sd_cpu_object_index_duplicate_entries(ix.x, ml, mo, p[0] ? small.data() : nullptr, p[1] ? small.data() : nullptr,
                                                        p[2] ? small.data() : nullptr, ne - 1, &need) == SD_ERR_CAPACITY);
            CHECK(need == ne);
            for (uint64_t s : small) CHECK(s == FILL);
        }
    }
    CHECK(sd_cpu_object_index_duplicates(ix.x, ml, mo, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SD_OK);
}

static void check_stats_and_keys(const index_t& ix, const model_t& m, uint64_t seed) {
    const std::map<uint64_t, group_t> g = groups_of(m);
    uint64_t want[8] = {g.size(), m.size(), 0, 0, 0, 0, 0, 0}, got[8];
    for (const auto& e : g) {
        const group_t& t = e.second;
        want[2] += t.links;
        if (t.links >= 2) want[3]++, want[4] += t.links;
        if (t.owners >= 2) want[5]++, want[6] += t.owners;
        want[7] = std::max(want[7], t.links);
    }
    CHECK(sd_cpu_object_index_duplicate_stats(ix.x, got) == SD_OK);
    for (int k = 0; k < 8; k++) CHECK(got[k] == want[k]);
    CHECK(got[1] - got[0] == got[6] - got[5] && got[2] - got[0] == got[4] - got[3]);
    // key lists: present keys (some twice), key + 1, the edges, uniform misses
    vec q = {0, ~0ull, 1ull << 63, (1ull << 63) - 1, 1};
    size_t i = 0;
    for (const auto& e : g) {
        if (i++ % 3 == 0) q.push_back(e.first), q.push_back(e.first + 1);
        if (i % 7 == 0) q.push_back(e.first);
    }
    const vec miss = splitmix(seed + 77, 40);
    q.insert(q.end(), miss.begin(), miss.end());
    const vec r = splitmix(seed + 5, q.size());
    for (size_t j = q.size(); j > 1; j--) std::swap(q[j - 1], q[r[j - 1] % j]);
    for (size_t mq : {(size_t)0, (size_t)1, std::min<size_t>(63, q.size()), q.size()}) {
        vec l(mq + 2, FILL), o(mq + 2, FILL);
        CHECK(sd_cpu_object_index_key_links(ix.x, mq ? q.data() : nullptr, mq, l.data() + 1, o.data() + 1) == SD_OK);
        CHECK(l[0] == FILL && l[mq + 1] == FILL && o[0] == FILL && o[mq + 1] == FILL);
        for (size_t j = 0; j < mq; j++) {
            const auto it = g.find(q[j]);
            CHECK(l[j + 1] == (it == g.end() ? 0 : it->second.links));
            CHECK(o[j + 1] == (it == g.end() ? 0 : it->second.owners));
        }
        vec only(mq + 1, FILL);
        CHECK(sd_cpu_object_index_key_links(ix.x, mq ? q.data() : nullptr, mq, nullptr, only.data()) == SD_OK);
        for (size_t j = 0; j < mq; j++) CHECK(only[j] == o[j + 1]);
        CHECK(only[mq] == FILL);
        CHECK(sd_cpu_object_index_key_links(ix.x, mq ? q.data() : nullptr, mq, only.data(), nullptr) == SD_OK);
        for (size_t j = 0; j < mq; j++) CHECK(only[j] == l[j + 1]);
    }
}

static void check_all(const index_t& ix, const model_t& m, uint64_t seed) {
    uint64_t largest = 0;
    for (const auto& e : groups_of(m)) largest = std::max(largest, e.second.links);
    for (uint64_t ml : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)3, largest, largest + 1, ~(uint64_t)0})
        for (uint64_t mo : {(uint64_t)0, (uint64_t)1, (uint64_t)2, RUN, RUN + 1}) check_select(ix, m, ml, mo);
    check_stats_and_keys(ix, m, seed);
    // (0, 0): the entries are export_links row for row
    vec k(m.size() + 1), v(m.size() + 1), l(m.size() + 1), ek(m.size() + 1), ev(m.size() + 1), el(m.size() + 1);
    uint64_t count = 0;
    CHECK(sd_cpu_object_index_duplicate_entries(ix.x, 0, 0, k.data(), v.data(), l.data(), m.size(), &count) == SD_OK);
    CHECK(sd_cpu_object_index_export_links(ix.x, ek.data(), ev.data(), el.data(), m.size()) == SD_OK);
    CHECK(count == m.size() && k == ek && v == ev && l == el);
}

// n entries: runs of 3 and 2 owners at both ends (keys 0, 1, 2^64 - 2, 2^64 - 1), every fourth
// other key with a second owner, 1 to 3 links
static void build(index_t& ix, model_t& m, size_t n, uint64_t seed) {
    vec ik, iv;
    const uint64_t ends[10][2] = {{0, 0}, {0, 5}, {0, ~0ull}, {1, 0}, {1, 5}, {~0ull, 0}, {~0ull, ~0ull},
                                  {~0ull - 1, 0}, {~0ull - 1, ~0ull}, {1ull << 63, 7}};
    const vec k = splitmix(seed, n), r = splitmix(seed + 1, n);
    for (size_t i = 0; i < n; i++) {
        uint64_t key = k[i], id = r[i] % 50;
        if (n >= 15 && i < 10) key = ends[i][0], id = ends[i][1];
        else if (i % 4 == 3) key = k[i - 1], id = 60 + r[i] % 5;  // a second owner of the key before
        const size_t copies = 1 + (i % 3 == 0) + (i % 5 == 0);
        for (size_t c = 0; c < copies; c++) ik.push_back(key), iv.push_back(id);
    }
    if (n) ix.insert(m, ik, iv);
}

static void test_entry_counts() {
    for (size_t n : {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097}) {
        index_t ix;
        model_t m;
        build(ix, m, n, 100 + n);
        CHECK(m.size() == n);
        check_all(ix, m, n);
    }
}

static void test_long_run_one_key_and_copies() {
    {
        index_t ix;  // RUN owners of one key among 2000 others
        model_t m;
        const vec other = splitmix(654, 2000);
        ix.insert(m, other, splitmix(656, 2000));
        ix.insert(m, vec(RUN, other[7] ^ (1ull << 20)), splitmix(655, RUN));
        check_all(ix, m, 1);
        uint64_t count = 0, key = 0, owners = 0;
        CHECK(sd_cpu_object_index_duplicates(ix.x, 0, RUN, &key, nullptr, nullptr, &owners, 1, &count) == SD_OK);
        CHECK(count == 1 && key == (other[7] ^ (1ull << 20)) && owners == RUN);
        CHECK(sd_cpu_object_index_duplicates(ix.x, 0, RUN + 1, nullptr, nullptr, nullptr, nullptr, 0, &count) == SD_OK && count == 0);
    }
    {
        index_t ix;  // 1025 entries of one key; then 1025 distinct keys beside it
        model_t m;
        vec ids(1025);
        for (size_t i = 0; i < 1025; i++) ids[i] = 3 * i;
        ix.insert(m, vec(1025, 1ull << 40), ids);
        check_all(ix, m, 2);
        ix.insert(m, splitmix(4545, 1025), ids);
        check_all(ix, m, 3);
    }
    {
        index_t ix;  // 70 000 links on one pair beside a key with three owners
        model_t m;
        ix.insert(m, vec(70000, 42), vec(70000, 9));
        ix.insert(m, {43, 44, 43, 43}, {9, 10, 11, 12});
        check_all(ix, m, 4);
        uint64_t st[8];
        CHECK(sd_cpu_object_index_duplicate_stats(ix.x, st) == SD_OK && st[7] == 70000 && st[3] == 2 && st[5] == 1);
    }
}

// a history of inserts and removals: the view follows the relation
static void test_after_removals() {
    index_t ix;
    model_t m;
    build(ix, m, 1025, 31);
    vec rk, rv;
    size_t i = 0;
    for (const auto& e : m)
        if (i++ % 2 == 0) rk.push_back(e.first.first), rv.push_back(e.first.second);  // one link of every second pair
    CHECK(sd_cpu_object_index_remove(ix.x, rk.data(), rv.data(), rk.size(), nullptr, 0, nullptr) == SD_OK);
    i = 0;
    for (auto it = m.begin(); it != m.end();) {
        if (i++ % 2 != 0) ++it;
        else if (it->second == 1) it = m.erase(it);
        else it->second--, ++it;
    }
    CHECK(!m.empty());
    check_all(ix, m, 5);
}

static void test_refusals() {
    index_t first(1, 0, 0), ix, empty;
    model_t m;
    const vec k = {1, 2, 3};
    CHECK(sd_cpu_object_index_insert(first.x, k.data(), k.data(), 3, nullptr) == SD_OK);
    ix.insert(m, k, k);
    vec out(8, FILL);
    uint64_t* o = out.data();
    uint64_t count = 9;
    CHECK(sd_cpu_object_index_key_links(first.x, k.data(), 3, o, o) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicates(first.x, 0, 0, o, o, o, o, 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicate_entries(first.x, 0, 0, o, o, o, 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicate_stats(first.x, o) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_key_links(ix.x, nullptr, 3, o, o) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_key_links(nullptr, k.data(), 3, o, o) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicates(nullptr, 0, 0, o, o, o, o, 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicate_entries(nullptr, 0, 0, o, o, o, 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicate_stats(nullptr, o) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_duplicate_stats(ix.x, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_key_links(ix.x, nullptr, 0, o, o) == SD_OK);
    // an empty index: counts 0, stats all 0, nothing written
    CHECK(sd_cpu_object_index_duplicates(empty.x, 0, 0, o, o, o, o, 0, &count) == SD_OK && count == 0);
    count = 9;
    CHECK(sd_cpu_object_index_duplicate_entries(empty.x, 0, 0, o, o, o, 0, &count) == SD_OK && count == 0);
    for (uint64_t v : out) CHECK(v == FILL);
    uint64_t st[8];
    CHECK(sd_cpu_object_index_duplicate_stats(empty.x, st) == SD_OK);
    for (uint64_t v : st) CHECK(v == 0);
    uint64_t l = 9, w = 9;
    const uint64_t key = 7;
    CHECK(sd_cpu_object_index_key_links(empty.x, &key, 1, &l, &w) == SD_OK && l == 0 && w == 0);
}

// the shards' rows concatenated in rank order are the unsharded answer; the stats add up
static void test_shards() {
    const vec k0 = splitmix(51, 3000), r = splitmix(52, 3000);
    vec k = k0, v(3000);
    for (size_t i = 0; i < 3000; i++) {
        v[i] = r[i] % 400;
        if (i % 5 == 4) k[i] = k[i - 1];  // second owners
    }
    k.insert(k.end(), k0.begin(), k0.begin() + 700), v.insert(v.end(), v.begin(), v.begin() + 700);  // second links
    index_t whole;
    model_t wm;
    whole.insert(wm, k, v);
    for (uint64_t ml : {0ull, 2ull})
        for (uint64_t mo : {0ull, 2ull}) {
            const uint64_t n = wm.size();
            vec wk(n), wf(n), wl(n), wo(n);
            uint64_t wc = 0, wst[8];
            CHECK(sd_cpu_object_index_duplicates(whole.x, ml, mo, wk.data(), wf.data(), wl.data(), wo.data(), n, &wc) == SD_OK);
            CHECK(sd_cpu_object_index_duplicate_stats(whole.x, wst) == SD_OK);
            CHECK(wc > 100);
            for (int nparts : {2, 3, 8}) {
                vec gk, gf, gl, go;
                uint64_t sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int part = 0; part < nparts; part++) {
                    index_t ix(nparts, part);
                    model_t m;
                    ix.insert(m, k, v);
                    check_select(ix, m, ml, mo);
                    vec a(n), b(n), c(n), d(n);
                    uint64_t cnt = 0, st[8];
                    CHECK(sd_cpu_object_index_duplicates(ix.x, ml, mo, a.data(), b.data(), c.data(), d.data(), n, &cnt) == SD_OK);
                    gk.insert(gk.end(), a.begin(), a.begin() + cnt), gf.insert(gf.end(), b.begin(), b.begin() + cnt);
                    gl.insert(gl.end(), c.begin(), c.begin() + cnt), go.insert(go.end(), d.begin(), d.begin() + cnt);
                    CHECK(sd_cpu_object_index_duplicate_stats(ix.x, st) == SD_OK);
                    for (int j = 0; j < 7; j++) sum[j] += st[j];
                    sum[7] = std::max(sum[7], st[7]);
                }
                wk.resize(wc), wf.resize(wc), wl.resize(wc), wo.resize(wc);
                CHECK(gk == wk && gf == wf && gl == wl && go == wo);
                for (int j = 0; j < 8; j++) CHECK(sum[j] == wst[j]);
            }
        }
}

// the reads by key are const on the index: four threads ask at once between writes
static void test_concurrent_reads() {
    index_t ix;
    model_t m;
    build(ix, m, 4097, 61);
    for (int round = 0; round < 3; round++) {
        std::vector<std::thread> ts;
        for (int t = 0; t < 4; t++)
            ts.emplace_back([&, t] {
                check_select(ix, m, (uint64_t)(t % 3), (uint64_t)(t / 2 + 1));
                check_stats_and_keys(ix, m, 70 + t);
            });
        for (auto& t : ts) t.join();
        const vec k = splitmix(80 + round, 200);
        ix.insert(m, k, vec(200, 1000 + round));
    }
}

int main() {
    test_entry_counts();
    test_long_run_one_key_and_copies();
    test_after_removals();
    test_refusals();
    test_shards();
    test_concurrent_reads();
    if (g_fail) {
        printf("object_index_duplicates_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_duplicates_selftest: ok\n");
    return 0;
}
