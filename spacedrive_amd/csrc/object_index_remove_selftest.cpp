// object_index_remove_selftest.cpp -- the Object index's removals in the host code
// (object_index_host.cpp: sd_cpu_object_index_remove, sd_cpu_object_index_remove_objects; and
// object_index.h, the rules the kernels share) against a std::map model, on the lists of
// tests/object_index_remove_cases.py restated in C++: the by-key sweep over index sizes,
// removal counts and key sets, unconditional and conditional; the by-Object lists; the fixed
// cases; the 300 007-entry shape; the capacity rule; the argument checks; and concurrent
// lookups between removals.  A program of its own: built plain for the CPU suite (`make
// object-index-remove-selftest`, tests/test_object_index_remove.py) and under ASan + UBSan
// and TSan (`make sanitize-object-index-remove`, logs in profiles/object_index/).
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
typedef std::map<uint64_t, uint64_t> model_t;
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

static vec edge_keys() {
    const uint64_t top = 1ull << 63;
    return {0, 1, top - 1, top, top + 1, ~0ull - 1, ~0ull};
}

static vec distinct(vec v, size_t n) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    CHECK(v.size() >= n);
    v.resize(n);
    return v;
}

// the three key sets of an index of n entries: uniform, edges, one bucket holding everything
static vec key_set(int kind, size_t n) {
    if (kind == 0) return distinct(splitmix(1000 + n, n + 8), n);
    if (kind == 1) {
        vec k = edge_keys();
        if (n <= k.size()) {
            k.resize(n);
            return k;
        }
        const vec rest = splitmix(2000 + n, n);
        k.insert(k.end(), rest.begin(), rest.end());
        return distinct(k, n);
    }
    vec low = splitmix(77, n + n / 8 + 8);
    for (auto& x : low) x = (x & 0xFFFFFFFFull) | (0xC0FFEE42ull << 32);
    return distinct(low, n);
}

static vec vals_for(const vec& keys, uint64_t salt) {
    vec v = splitmix(salt, keys.size());
    for (size_t i = 0; i < v.size(); i++) v[i] ^= keys[i] * 3;
    if (v.size() > 2) { v[0] = 0; v[1] = ~0ull; }
    return v;
}

// m removal keys against sorted keys: present ones with repeats, absent ones between two
// keys, below the minimum, above the maximum, uniform misses
static vec removal_keys(const vec& s, size_t m, uint64_t seed) {
    vec q;
    const vec r = splitmix(seed, m), miss = splitmix(seed + 9, m);
    for (size_t i = 0; i < m; i++) {
        if (s.empty() || i % 4 == 3) q.push_back(miss[i]);
        else if (i % 4 == 2) q.push_back(s[r[i] % s.size()] + 1);
        else q.push_back(s[r[i] % s.size()]);
    }
    if (m > 4 && !s.empty()) {
        q[2] = s.front() - 1;
        q[3] = s.back() + 1;
    }
    return q;
}

static bool wrong_key(uint64_t k) { return ((k * 0x9E3779B97F4A7C15ull) >> 60) % 3 == 0; }

struct dropped_t { vec pairs; uint64_t r; };

static dropped_t model_remove(model_t& m, const vec& k, const vec* ids) {
    std::set<uint64_t> gone;
    for (size_t i = 0; i < k.size(); i++) {
        const auto it = m.find(k[i]);
        if (it != m.end() && (!ids || (*ids)[i] == it->second)) gone.insert(k[i]);
    }
    dropped_t d{{}, gone.size()};
    for (uint64_t g : gone) {
        d.pairs.push_back(g);
        d.pairs.push_back(m[g]);
        m.erase(g);
    }
    return d;
}

static dropped_t model_remove_objects(model_t& m, const vec& ids) {
    const std::set<uint64_t> want(ids.begin(), ids.end());
    dropped_t d{{}, 0};
    for (auto it = m.begin(); it != m.end();) {
        if (want.count(it->second)) {
            d.pairs.push_back(it->first);
            d.pairs.push_back(it->second);
            d.r++;
            it = m.erase(it);
        } else {
            ++it;
        }
    }
    return d;
}

static void check_equals_model(const sd_cpu_object_index* x, const model_t& m) {
    uint64_t n = ~0ull;
    CHECK(sd_cpu_object_index_count(x, &n) == SD_OK && n == m.size());
    vec k(n + 1, FILL), v(n + 1, FILL);
    CHECK(sd_cpu_object_index_export(x, k.data(), v.data(), n) == SD_OK);
    CHECK(k[n] == FILL && v[n] == FILL);
    size_t i = 0;
    for (const auto& kv : m) {
        CHECK(k[i] == kv.first && v[i] == kv.second);
        i++;
    }
    // the rebuilt directory finds every key that stayed
    vec ids(n + 1, 7);
    std::vector<uint8_t> found(n + 1, 9);
    CHECK(sd_cpu_object_index_lookup(x, k.data(), n, ids.data(), found.data()) == SD_OK);
    for (size_t j = 0; j < n; j++) CHECK(found[j] == 1 && ids[j] == v[j]);
}

// one removal on the index and the model: the count, the dropped pairs in ascending key
// order, nothing past them, the export, and every dropped key missed afterwards
static uint64_t remove_both(sd_cpu_object_index* x, model_t& m, const vec& a, const vec* ids, bool by_object) {
    const dropped_t want = by_object ? model_remove_objects(m, a) : model_remove(m, a, ids);
    vec out(2 * (want.r + 2), FILL);
    uint64_t r = ~0ull;
    const int rc = by_object
        ? sd_cpu_object_index_remove_objects(x, a.data(), a.size(), out.data(), want.r + 2, &r)
        : sd_cpu_object_index_remove(x, a.data(), ids ? ids->data() : nullptr, a.size(), out.data(), want.r + 2, &r);
    CHECK(rc == SD_OK && r == want.r);
    for (size_t j = 0; j < want.pairs.size(); j++) CHECK(out[j] == want.pairs[j]);
    for (size_t j = want.pairs.size(); j < out.size(); j++) CHECK(out[j] == FILL);
    check_equals_model(x, m);
    vec gone;
    for (size_t j = 0; j < want.pairs.size(); j += 2) gone.push_back(want.pairs[j]);
    vec got(gone.size() + 1, 7);
    std::vector<uint8_t> found(gone.size() + 1, 9);
    CHECK(sd_cpu_object_index_lookup(x, gone.data(), gone.size(), got.data(), found.data()) == SD_OK);
    for (size_t j = 0; j < gone.size(); j++) CHECK(found[j] == 0 && got[j] == 0);
    return want.r;
}

static void insert_both(sd_cpu_object_index* x, model_t& m, const vec& k, const vec& v) {
    uint64_t want = 0, taken = ~0ull;
    for (size_t i = 0; i < k.size(); i++)
        if (!m.count(k[i])) {
            m[k[i]] = v[i];
            want++;
        }
    CHECK(sd_cpu_object_index_insert(x, k.data(), v.data(), k.size(), &taken) == SD_OK && taken == want);
}

static sd_cpu_object_index* fresh() {
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(1, 0, &x) == SD_OK && x);
    return x;
}

static const size_t SIZES[] = {0, 1, 2, 15, 16, 17, 255, 256, 257, 4097, 100003};
static const size_t COUNTS[] = {0, 1, 63, 64, 65, 257, 5000};

static void test_by_key() {
    uint64_t right = 0, wrong = 0, absent = 0;
    for (int kind = 0; kind < 3; kind++)
        for (size_t n : SIZES) {
            const vec keys = key_set(kind, n), vals = vals_for(keys, 31);
            for (int cond = 0; cond < 2; cond++) {
                sd_cpu_object_index* x = fresh();
                model_t m;
                insert_both(x, m, keys, vals);
                for (size_t c : COUNTS) {
                    vec rk = removal_keys(keys, c, 5 + c);
                    if (!cond) {
                        for (uint64_t k : rk) absent += !m.count(k);
                        remove_both(x, m, rk, nullptr, false);
                    } else {
                        // the right id, a wrong one for a third of the keys, anything for absent
                        // keys; pairs 0 and 1 name one key, wrongly then rightly
                        if (c >= 2 && n) rk[0] = rk[1] = keys[n / 2];
                        vec ids = splitmix(4242, c);
                        for (size_t i = 0; i < c; i++) {
                            const auto it = m.find(rk[i]);
                            if (it == m.end()) continue;
                            ids[i] = wrong_key(rk[i]) ? it->second ^ 1 : it->second;
                            (wrong_key(rk[i]) ? wrong : right)++;
                        }
                        if (c >= 2 && n) {
                            ids[0] = m[rk[0]] ^ 1;
                            ids[1] = m[rk[1]];
                        }
                        const bool had = c >= 2 && n;
                        remove_both(x, m, rk, &ids, false);
                        if (had) CHECK(!m.count(keys[n / 2]));  // one right pair is enough
                    }
                    insert_both(x, m, keys, vals);  // filled up again, the same values
                    CHECK(m.size() == n);
                }
                sd_cpu_object_index_destroy(x);
            }
        }
    CHECK(right > 0 && wrong > 0 && absent > 0);
}

static void test_by_object() {
    vec idset = splitmix(808, 14), none = splitmix(909, 16);
    idset.insert(idset.begin(), {0, ~0ull});
    for (size_t n : SIZES) {
        const vec keys = key_set(0, n), pick = splitmix(3100 + n, n);
        vec vals(n);
        for (size_t i = 0; i < n; i++) vals[i] = idset[pick[i] % idset.size()];
        sd_cpu_object_index* x = fresh();
        model_t m;
        insert_both(x, m, keys, vals);
        CHECK(remove_both(x, m, none, nullptr, true) == 0);  // ids owning nothing
        for (size_t c : COUNTS) {
            // repeated ids over half of the set (0 among them) and the absent ones
            const vec r = splitmix(3200 + c, c);
            vec ids(c);
            for (size_t i = 0; i < c; i++) ids[i] = r[i] % 2 ? none[r[i] % none.size()] : idset[(r[i] % 8) * 2];
            const uint64_t dropped = remove_both(x, m, ids, nullptr, true);
            if (n >= 255 && c >= 63) CHECK(dropped > 0 && dropped < n);
            insert_both(x, m, keys, vals);
        }
        vec all = idset;
        all.insert(all.end(), idset.begin(), idset.begin() + 3);
        CHECK(remove_both(x, m, all, nullptr, true) == n && m.empty());  // every id: the index is empty
        insert_both(x, m, keys, vals);  // and insert works
        check_equals_model(x, m);
        sd_cpu_object_index_destroy(x);
    }
}

static void test_fixed() {
    const vec keys = key_set(0, 4097), vals = vals_for(keys, 62);
    CHECK(oi_dir_bits(4097) == 9);
    {   // the first entry, the last entry, then both conditionally on a fresh index
        sd_cpu_object_index* x = fresh();
        model_t m;
        insert_both(x, m, keys, vals);
        CHECK(remove_both(x, m, {keys.front()}, nullptr, false) == 1);
        CHECK(remove_both(x, m, {keys.back()}, nullptr, false) == 1);
        insert_both(x, m, keys, vals);
        const vec ends = {keys.front(), keys.back()}, ids = {vals.front(), vals.back()};
        CHECK(remove_both(x, m, ends, &ids, false) == 2);
        // one whole directory bucket, in descending order; a second time it finds nothing
        insert_both(x, m, keys, vals);
        const uint64_t p = oi_prefix(keys[keys.size() / 2], 9);
        vec bucket;
        for (uint64_t k : keys)
            if (oi_prefix(k, 9) == p) bucket.push_back(k);
        std::reverse(bucket.begin(), bucket.end());
        CHECK(!bucket.empty() && remove_both(x, m, bucket, nullptr, false) == bucket.size());
        CHECK(remove_both(x, m, bucket, nullptr, false) == 0);
        sd_cpu_object_index_destroy(x);
    }
    {   // three_growth backwards: 240 -> 40 -> 10 -> 0 entries, directory bits 4 -> 2 -> 0 -> 0
        const vec g1 = splitmix(15, 10), g2 = splitmix(16, 30), g3 = splitmix(17, 200);
        const vec v1 = vals_for(g1, 9), v2 = vals_for(g2, 10), v3 = vals_for(g3, 11);
        CHECK(oi_dir_bits(240) == 4 && oi_dir_bits(40) == 2 && oi_dir_bits(10) == 0 && oi_dir_bits(0) == 0);
        sd_cpu_object_index* x = fresh();
        model_t m;
        insert_both(x, m, g1, v1);
        insert_both(x, m, g2, v2);
        insert_both(x, m, g3, v3);
        CHECK(m.size() == 240);
        CHECK(remove_both(x, m, g3, nullptr, false) == 200 && m.size() == 40);
        CHECK(remove_both(x, m, g2, &v2, false) == 30 && m.size() == 10);
        CHECK(remove_both(x, m, v1, nullptr, true) == 10 && m.empty());
        insert_both(x, m, g3, v3);  // into the emptied index
        check_equals_model(x, m);
        sd_cpu_object_index_destroy(x);
    }
    {   // nothing from an empty index
        sd_cpu_object_index* x = fresh();
        model_t m;
        const vec few = splitmix(63, 5);
        CHECK(remove_both(x, m, few, nullptr, false) == 0 && remove_both(x, m, few, &few, false) == 0);
        CHECK(remove_both(x, m, few, nullptr, true) == 0 && remove_both(x, m, {}, nullptr, true) == 0);
        sd_cpu_object_index_destroy(x);
    }
}

static void test_large() {
    const size_t n = 300007;
    const vec keys = key_set(0, n);
    vec vals(n);
    for (size_t i = 0; i < n; i++) vals[i] = i / 1000;  // keys are sorted: runs of 1000 per Object
    sd_cpu_object_index* x = fresh();
    model_t m;
    insert_both(x, m, keys, vals);
    vec every_other, odd_runs, all_but_one;
    for (size_t i = 0; i < n; i += 2) every_other.push_back(keys[i]);
    for (uint64_t o = 1; o <= n / 1000; o += 2) odd_runs.push_back(o);
    for (size_t i = n; i-- > 0;)
        if (i != 123456) all_but_one.push_back(keys[i]);
    CHECK(remove_both(x, m, every_other, nullptr, false) == (n + 1) / 2);
    insert_both(x, m, keys, vals);
    CHECK(remove_both(x, m, odd_runs, nullptr, true) == 150000);
    insert_both(x, m, keys, vals);
    CHECK(remove_both(x, m, all_but_one, nullptr, false) == n - 1 && m.size() == 1);
    const vec lone = {keys[123456]}, id = {vals[123456]};
    CHECK(remove_both(x, m, lone, &id, false) == 1 && m.empty());
    sd_cpu_object_index_destroy(x);
}

// a capacity short by one: the error, the requirement, nothing written, the index unchanged
static void test_capacity() {
    const vec keys = key_set(0, 1000), vals = vals_for(keys, 5);
    for (int by_object = 0; by_object < 2; by_object++) {
        sd_cpu_object_index* x = fresh();
        model_t m;
        insert_both(x, m, keys, vals);
        const vec a = by_object ? vec(vals.begin(), vals.begin() + 100) : vec(keys.begin() + 50, keys.begin() + 150);
        vec out(2 * 101, FILL);
        uint64_t r = 0;
        const int rc = by_object ? sd_cpu_object_index_remove_objects(x, a.data(), a.size(), out.data(), 99, &r)
                                 : sd_cpu_object_index_remove(x, a.data(), nullptr, a.size(), out.data(), 99, &r);
        CHECK(rc == SD_ERR_CAPACITY && r == 100);
        for (uint64_t o : out) CHECK(o == FILL);
        check_equals_model(x, m);
        // without an output buffer the capacity is not looked at
        const int rc2 = by_object ? sd_cpu_object_index_remove_objects(x, a.data(), a.size(), nullptr, 0, &r)
                                  : sd_cpu_object_index_remove(x, a.data(), nullptr, a.size(), nullptr, 0, &r);
        CHECK(rc2 == SD_OK && r == 100);
        if (by_object) model_remove_objects(m, a);
        else model_remove(m, a, nullptr);
        check_equals_model(x, m);
        sd_cpu_object_index_destroy(x);
    }
}

// concurrent lookups on one index are safe between removals (removals are exclusive)
static void test_concurrent_lookups_between_removals() {
    sd_cpu_object_index* x = fresh();
    const vec k = key_set(0, 6000), v = vals_for(k, 72);
    model_t m;
    insert_both(x, m, k, v);
    for (int round = 0; round < 4; round++) {
        std::vector<int> bad(4, 0);
        std::vector<std::thread> th;
        for (int t = 0; t < 4; t++)
            th.emplace_back([&, t] {
                vec ids(k.size());
                std::vector<uint8_t> found(k.size());
                for (int rep = 0; rep < 2; rep++) {
                    if (sd_cpu_object_index_lookup(x, k.data(), k.size(), ids.data(), found.data()) != SD_OK) bad[t]++;
                    for (size_t i = 0; i < k.size(); i++) {
                        const auto it = m.find(k[i]);
                        bad[t] += !(found[i] == (it != m.end()) && ids[i] == (it != m.end() ? it->second : 0));
                    }
                }
            });
        for (auto& t : th) t.join();
        for (int b : bad) CHECK(b == 0);
        const vec part(k.begin() + 1500 * round, k.begin() + 1500 * (round + 1));
        if (round % 2) {
            const vec ids(v.begin() + 1500 * round, v.begin() + 1500 * (round + 1));
            remove_both(x, m, ids, nullptr, true);
        } else {
            remove_both(x, m, part, nullptr, false);
        }
    }
    CHECK(m.empty());
    sd_cpu_object_index_destroy(x);
}

static void test_arguments() {
    sd_cpu_object_index* x = fresh();
    const vec k = {1, 2, 3};
    uint64_t r = 5;
    CHECK(sd_cpu_object_index_remove(nullptr, k.data(), nullptr, 3, nullptr, 0, &r) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_remove_objects(nullptr, k.data(), 3, nullptr, 0, &r) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_remove(x, nullptr, nullptr, 3, nullptr, 0, &r) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_remove_objects(x, nullptr, 3, nullptr, 0, &r) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_remove(x, nullptr, nullptr, 0, nullptr, 0, &r) == SD_OK && r == 0);  // m == 0: a no-op
    r = 5;
    CHECK(sd_cpu_object_index_remove_objects(x, nullptr, 0, nullptr, 0, &r) == SD_OK && r == 0);
    CHECK(sd_cpu_object_index_remove(x, k.data(), nullptr, 3, nullptr, 0, nullptr) == SD_OK);
    sd_cpu_object_index_destroy(x);
}

int main() {
    test_arguments();
    test_by_key();
    test_by_object();
    test_fixed();
    test_large();
    test_capacity();
    test_concurrent_lookups_between_removals();
    if (g_fail) {
        printf("object_index_remove_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_remove_selftest: ok\n");
    return 0;
}
