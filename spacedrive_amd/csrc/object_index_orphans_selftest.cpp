// object_index_orphans_selftest.cpp -- sd_cpu_object_index_object_links and
// sd_cpu_object_index_orphans (object_index_host.cpp; the rule oi_object_slot / oi_unowned of
// object_index.h, which the kernels share) against a std::map model Object id -> (links,
// entries) kept beside a seeded sequence of inserts, removals and applies: id lists that are
// empty, one id, repeats, all absent, all present, above 2^63 and equal to key values; the entry
// counts at which the directory bits change; stride 2 over the rows a removal reports; one
// Object owning every entry; 70 000 copies of one pair; the capacity rule with a pre-filled
// buffer; the refusals; the shard sums and intersection; and concurrent reads.  A program of its
// own: built plain for the CPU suite (`make object-index-orphans-selftest`,
// tests/test_object_index_orphans.py) and under ASan + UBSan and TSan (`make
// sanitize-object-index-orphans`, logs in profiles/object_index/).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <set>
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

// ---- the model: object_index.h, by Object
struct totals_t {
    uint64_t links = 0, entries = 0;
};
static std::map<uint64_t, totals_t> totals_of(const model_t& m) {
    std::map<uint64_t, totals_t> t;
    for (const auto& e : m) t[e.first.second].links += e.second, t[e.first.second].entries++;
    return t;
}

// both calls on the m ids read at `stride` from `ids`, against the model; outputs between guards
static void check_ids(const index_t& ix, const model_t& m, const vec& ids, uint64_t stride, uint64_t n_ids) {
    const std::map<uint64_t, totals_t> t = totals_of(m);
    vec links(n_ids + 2, FILL), entries(n_ids + 2, FILL);
    CHECK(sd_cpu_object_index_object_links(ix.x, n_ids ? ids.data() : nullptr, stride, n_ids, links.data() + 1,
                                           entries.data() + 1) == SD_OK);
    CHECK(links[0] == FILL && links[n_ids + 1] == FILL && entries[0] == FILL && entries[n_ids + 1] == FILL);
    std::set<uint64_t> want;
    for (uint64_t j = 0; j < n_ids; j++) {
        const uint64_t id = ids[j * stride];
        const auto it = t.find(id);
        CHECK(links[j + 1] == (it == t.end() ? 0 : it->second.links));
        CHECK(entries[j + 1] == (it == t.end() ? 0 : it->second.entries));
        if (it == t.end()) want.insert(id);
    }
    vec out(n_ids + 2, FILL);
    uint64_t count = ~0ull;
    CHECK(sd_cpu_object_index_orphans(ix.x, n_ids ? ids.data() : nullptr, stride, n_ids, out.data() + 1, n_ids, &count) ==
          SD_OK);
    CHECK(count == want.size() && out[0] == FILL);
    size_t j = 1;
    for (uint64_t id : want) CHECK(out[j++] == id);  // ascending, unsigned
    for (; j < out.size(); j++) CHECK(out[j] == FILL);
    // the capacity rule: one short writes nothing and reports the requirement; NULL only counts
    if (count > 0) {
        vec small(count + 1, FILL);
        uint64_t need = 0;
        CHECK(sd_cpu_object_index_orphans(ix.x, ids.data(), stride, n_ids, small.data(), count - 1, &need) ==
              SD_ERR_CAPACITY);
        CHECK(need == count);
        for (uint64_t s : small) CHECK(s == FILL);
    }
    uint64_t only = ~0ull;
    CHECK(sd_cpu_object_index_orphans(ix.x, n_ids ? ids.data() : nullptr, stride, n_ids, nullptr, 0, &only) == SD_OK);
    CHECK(only == count);
}

static vec id_list(const model_t& m, int kind, uint64_t seed) {
    vec have, keys;
    for (const auto& e : m) have.push_back(e.first.second), keys.push_back(e.first.first);
    std::sort(have.begin(), have.end());
    have.erase(std::unique(have.begin(), have.end()), have.end());
    const vec absent = splitmix(seed + 900, 20);
    vec ids;
    switch (kind) {
        case 0: break;                                                   // empty
        case 1: ids.push_back(have.empty() ? 7 : have[0]); break;        // one id
        case 2: ids.assign(9, have.empty() ? 7 : have.back()); break;    // repeats of one id
        case 3: ids = absent; break;                                     // all absent (with the model's say)
        case 4: ids = have; std::reverse(ids.begin(), ids.end()); break; // all present
        case 5:                                                          // above 2^63: the unsigned order
            ids = {~0ull, ~0ull - 1, 1ull << 63, (1ull << 63) + 5, (1ull << 63) - 1, 0, 5, 1};
            break;
        case 6:                                                          // ids equal to key values
            for (size_t i = 0; i < keys.size() && i < 6; i++) ids.push_back(keys[i]);
            break;
        default:                                                         // a shuffled mix with repeats
            for (size_t i = 0; i < have.size(); i += 2) ids.push_back(have[i]);
            for (size_t i = 0; i < 7; i++) ids.push_back(absent[i]);
            for (size_t i = 0; i < have.size(); i += 5) ids.push_back(have[i]);
            const vec r = splitmix(seed + 5, ids.size());
            for (size_t i = ids.size(); i > 1; i--) std::swap(ids[i - 1], ids[r[i - 1] % i]);
    }
    return ids;
}

static void check_all_lists(const index_t& ix, const model_t& m, uint64_t seed) {
    for (int kind = 0; kind < 8; kind++) {
        const vec ids = id_list(m, kind, seed);
        check_ids(ix, m, ids, 1, ids.size());
    }
}

// n entries: few Objects (several keys each), ids 0 and 2^64 - 1 among them, 1 to 3 links
static void build(index_t& ix, model_t& m, size_t n, uint64_t seed) {
    if (n == 0) return;
    const vec k = splitmix(seed, n), r = splitmix(seed + 1, n);
    vec ik, iv;
    for (size_t i = 0; i < n; i++) {
        const uint64_t id = i % 7 == 0 ? 0 : i % 11 == 0 ? ~0ull : r[i] % (n / 3 + 2);
        const size_t copies = 1 + (i % 3 == 0) + (i % 5 == 0);
        for (size_t c = 0; c < copies; c++) ik.push_back(k[i]), iv.push_back(id);
    }
    ix.insert(m, ik, iv);
}

static void test_entry_counts() {
    for (size_t n : {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097}) {
        index_t ix;
        model_t m;
        build(ix, m, n, 100 + n);
        check_all_lists(ix, m, n);
    }
}

static void test_stride_2_over_removed_rows() {
    index_t ix;
    model_t m;
    build(ix, m, 600, 31);
    // every pair of Objects 0..9, by Object: the rows the removal reports are (key, id)
    vec objs;
    for (uint64_t o = 0; o < 10; o++) objs.push_back(o);
    vec rows(2 * 600, FILL);
    uint64_t removed = 0;
    CHECK(sd_cpu_object_index_remove_objects(ix.x, objs.data(), objs.size(), rows.data(), 600, &removed) == SD_OK);
    for (auto it = m.begin(); it != m.end();) it = it->first.second < 10 ? m.erase(it) : std::next(it);
    CHECK(removed > 10);
    check_ids(ix, m, vec(rows.begin() + 1, rows.begin() + 2 * removed), 2, removed);  // the id column
    check_ids(ix, m, vec(rows.begin(), rows.begin() + 2 * removed), 2, removed);      // the key column
    // an apply that takes one link of every remaining pair: the Objects with single links leave
    vec rk, rv;
    for (const auto& e : m) rk.push_back(e.first.first), rv.push_back(e.first.second);
    CHECK(sd_cpu_object_index_apply(ix.x, rk.data(), rv.data(), rk.size(), nullptr, nullptr, 0, rows.data(), 600,
                                    &removed, nullptr) == SD_OK);
    for (auto it = m.begin(); it != m.end();) {
        if (it->second == 1) it = m.erase(it);
        else it->second--, ++it;
    }
    CHECK(removed > 0 && !m.empty());
    check_ids(ix, m, vec(rows.begin() + 1, rows.begin() + 2 * removed), 2, removed);
}

static void test_one_owner_and_copies() {
    {
        index_t ix;
        model_t m;
        const vec k = splitmix(41, 1025);
        ix.insert(m, k, vec(1025, 77));
        ix.insert(m, vec(k.begin(), k.begin() + 300), vec(300, 77));
        check_ids(ix, m, {77, 78, 77, 0}, 1, 4);
        uint64_t l = 0, e = 0;
        const uint64_t id = 77;
        CHECK(sd_cpu_object_index_object_links(ix.x, &id, 1, 1, &l, &e) == SD_OK && l == 1325 && e == 1025);
        CHECK(sd_cpu_object_index_object_links(ix.x, &id, 1, 1, nullptr, &e) == SD_OK && e == 1025);  // either may be NULL
        CHECK(sd_cpu_object_index_object_links(ix.x, &id, 1, 1, &l, nullptr) == SD_OK && l == 1325);
    }
    {
        index_t ix;
        model_t m;
        ix.insert(m, vec(70000, 42), vec(70000, 9));
        ix.insert(m, {43, 44}, {9, 10});
        const vec ids = {9, 10, 11};
        vec l(3), e(3);
        CHECK(sd_cpu_object_index_object_links(ix.x, ids.data(), 1, 3, l.data(), e.data()) == SD_OK);
        CHECK(l[0] == 70001 && l[1] == 1 && l[2] == 0 && e[0] == 2 && e[1] == 1 && e[2] == 0);
        check_ids(ix, m, ids, 1, 3);
    }
}

static void test_refusals() {
    index_t first(1, 0, 0), ix;
    model_t m;
    const vec k = {1, 2, 3};
    CHECK(sd_cpu_object_index_insert(first.x, k.data(), k.data(), 3, nullptr) == SD_OK);
    ix.insert(m, k, k);
    vec out(8, FILL);
    uint64_t count = 9;
    CHECK(sd_cpu_object_index_object_links(first.x, k.data(), 1, 3, out.data(), out.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_orphans(first.x, k.data(), 1, 3, out.data(), 8, &count) == SD_ERR_INVALID);
    for (uint64_t stride : {0ull, 3ull, 4ull, 1ull << 40}) {
        CHECK(sd_cpu_object_index_object_links(ix.x, k.data(), stride, 1, out.data(), out.data()) == SD_ERR_INVALID);
        CHECK(sd_cpu_object_index_orphans(ix.x, k.data(), stride, 1, out.data(), 8, &count) == SD_ERR_INVALID);
    }
    CHECK(sd_cpu_object_index_orphans(ix.x, nullptr, 1, 3, out.data(), 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_orphans(nullptr, k.data(), 1, 3, out.data(), 8, &count) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_orphans(ix.x, nullptr, 1, 0, out.data(), 8, &count) == SD_OK && count == 0);
    CHECK(sd_cpu_object_index_object_links(ix.x, nullptr, 2, 0, out.data(), out.data()) == SD_OK);
    for (uint64_t o : out) CHECK(o == FILL);
}

// the sums over the shards are the unsharded totals; an id is an orphan iff every shard lists it
static void test_shards() {
    const vec k = splitmix(51, 3000), r = splitmix(52, 3000);
    vec v(3000);
    for (size_t i = 0; i < 3000; i++) v[i] = r[i] % 400;
    index_t whole;
    model_t wm;
    whole.insert(wm, k, v);
    vec ids = splitmix(53, 30);
    for (uint64_t o = 0; o < 400; o += 3) ids.push_back(o);
    const size_t q = ids.size();
    vec wl(q), we(q), wo(q);
    uint64_t wcount = 0;
    CHECK(sd_cpu_object_index_object_links(whole.x, ids.data(), 1, q, wl.data(), we.data()) == SD_OK);
    CHECK(sd_cpu_object_index_orphans(whole.x, ids.data(), 1, q, wo.data(), q, &wcount) == SD_OK && wcount >= 30);
    for (int nparts : {2, 3, 8}) {
        vec sl(q, 0), se(q, 0);
        std::map<uint64_t, int> listed;
        for (int part = 0; part < nparts; part++) {
            index_t ix(nparts, part);
            model_t m;
            ix.insert(m, k, v);
            check_ids(ix, m, ids, 1, q);
            vec l(q), e(q), o(q);
            uint64_t c = 0;
            CHECK(sd_cpu_object_index_object_links(ix.x, ids.data(), 1, q, l.data(), e.data()) == SD_OK);
            CHECK(sd_cpu_object_index_orphans(ix.x, ids.data(), 1, q, o.data(), q, &c) == SD_OK && c >= wcount);
            for (size_t j = 0; j < q; j++) sl[j] += l[j], se[j] += e[j];
            for (uint64_t j = 0; j < c; j++) listed[o[j]]++;
        }
        CHECK(sl == wl && se == we);
        vec both;
        for (const auto& e : listed)
            if (e.second == nparts) both.push_back(e.first);
        CHECK(both == vec(wo.begin(), wo.begin() + wcount));
    }
}

// the reads by Object are const on the index: four threads ask at once between writes
static void test_concurrent_reads() {
    index_t ix;
    model_t m;
    build(ix, m, 4097, 61);
    for (int round = 0; round < 3; round++) {
        std::vector<std::thread> ts;
        for (int t = 0; t < 4; t++)
            ts.emplace_back([&, t] {
                const vec ids = id_list(m, 7, 70 + t);
                check_ids(ix, m, ids, 1, ids.size());
                uint64_t found_id = 0;
                uint8_t found = 0;
                const uint64_t key = m.begin()->first.first;
                CHECK(sd_cpu_object_index_lookup(ix.x, &key, 1, &found_id, &found) == SD_OK && found == 1);
            });
        for (auto& t : ts) t.join();
        const vec k = splitmix(80 + round, 200);
        ix.insert(m, k, vec(200, 1000 + round));
    }
}

int main() {
    test_entry_counts();
    test_stride_2_over_removed_rows();
    test_one_owner_and_copies();
    test_refusals();
    test_shards();
    test_concurrent_reads();
    if (g_fail) {
        printf("object_index_orphans_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_orphans_selftest: ok\n");
    return 0;
}
