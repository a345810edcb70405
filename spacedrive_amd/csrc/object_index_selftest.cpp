// object_index_selftest.cpp -- the Object index's host code under test (object_index_host.cpp:
// the directory / growth policies, sd_cpu_object_index_*, sd_cpu_dedup_owners_indexed; and
// object_index.h, the lookup the kernels share), on the generator and case table of
// tests/object_index_cases.py, against a std::map model.  A program of its own: built plain
// for the CPU suite (`make object-index-selftest`, tests/test_object_index.py) and under
// ASan + UBSan and TSan (`make sanitize-object-index`, logs in profiles/object_index/).
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
typedef std::map<uint64_t, uint64_t> model_t;

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

static vec shared_prefix_keys(size_t n) {
    vec low = splitmix(77, n + n / 8 + 8);
    for (auto& x : low) x &= 0xFFFFFFFFull;
    std::sort(low.begin(), low.end());
    low.erase(std::unique(low.begin(), low.end()), low.end());
    low.resize(n);
    for (auto& x : low) x |= 0xC0FFEE42ull << 32;
    return low;
}

static vec vals_for(const vec& keys, uint64_t salt) {
    vec v = splitmix(salt, keys.size());
    for (size_t i = 0; i < v.size(); i++) v[i] ^= keys[i] * 3;
    if (v.size() > 2) { v[0] = 0; v[1] = ~0ull; }
    return v;
}

static uint64_t model_insert(model_t& m, const vec& k, const vec& v, int nparts, int part) {
    uint64_t taken = 0;
    for (size_t i = 0; i < k.size(); i++)
        if (oi_dest_of(k[i], nparts) == (uint32_t)part && !m.count(k[i])) {
            m[k[i]] = v[i];
            taken++;
        }
    return taken;
}

static void check_equals_model(const sd_cpu_object_index* x, const model_t& m) {
    uint64_t n = ~0ull;
    CHECK(sd_cpu_object_index_count(x, &n) == SD_OK && n == m.size());
    vec k(n + 1, 0xABABABABABABABABull), v(n + 1, 0xCDCDCDCDCDCDCDCDull);
    CHECK(sd_cpu_object_index_export(x, k.data(), v.data(), n) == SD_OK);
    CHECK(k[n] == 0xABABABABABABABABull && v[n] == 0xCDCDCDCDCDCDCDCDull);  // only n rows written
    size_t i = 0;
    for (const auto& kv : m) {
        CHECK(k[i] == kv.first && v[i] == kv.second);
        i++;
    }
    if (n && sd_cpu_object_index_export(x, k.data(), v.data(), n - 1) != SD_ERR_CAPACITY) CHECK(!"capacity");
    // every key is found; its neighbours are found exactly when the model has them
    vec q;
    for (const auto& kv : m) {
        q.push_back(kv.first);
        q.push_back(kv.first + 1);
        q.push_back(kv.first - 1);
    }
    const vec extra = splitmix(991, 64);
    q.insert(q.end(), extra.begin(), extra.end());
    vec ids(q.size() + 1, 7);
    std::vector<uint8_t> found(q.size() + 1, 9);
    CHECK(sd_cpu_object_index_lookup(x, q.data(), q.size(), ids.data(), found.data()) == SD_OK);
    for (size_t j = 0; j < q.size(); j++) {
        const auto it = m.find(q[j]);
        CHECK(found[j] == (it != m.end() ? 1 : 0));
        CHECK(ids[j] == (it != m.end() ? it->second : 0));
    }
    CHECK(ids[q.size()] == 7 && found[q.size()] == 9);
}

static void run_steps(const char* name, const std::vector<std::pair<vec, vec>>& steps, int nparts = 1, int part = 0) {
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(nparts, part, &x) == SD_OK && x);
    model_t m;
    for (const auto& st : steps) {
        const model_t before = m;
        uint64_t taken = ~0ull;
        CHECK(sd_cpu_object_index_insert(x, st.first.data(), st.second.data(), st.first.size(), &taken) == SD_OK);
        CHECK(taken == model_insert(m, st.first, st.second, nparts, part));
        for (const auto& kv : before) CHECK(m[kv.first] == kv.second);
        check_equals_model(x, m);
    }
    sd_cpu_object_index_destroy(x);
    if (g_fail) printf("  (case %s)\n", name);
}

static void test_policies() {
    CHECK(oi_dir_bits(0) == 0 && oi_dir_bits(15) == 0 && oi_dir_bits(16) == 1 && oi_dir_bits(31) == 1);
    CHECK(oi_dir_bits(32) == 2 && oi_dir_bits(40) == 2 && oi_dir_bits(240) == 4 && oi_dir_bits(10000000) == 20);
    CHECK(oi_dir_bits(~0ull) == 24);
    CHECK(oi_grow_capacity(10, 0) == 16 && oi_grow_capacity(40, 16) == 40 && oi_grow_capacity(17, 16) == 24);
    CHECK(oi_grow_capacity(16, 16) == 16 && oi_grow_capacity(0, 0) == 0);
    uint64_t k = 0;
    CHECK(oi_key_from_hex("00000000000000ff", &k) && k == 255);
    CHECK(oi_key_from_hex("ffffffffffffffff", &k) && k == ~0ull);
    CHECK(oi_key_from_hex("8000000000000000", &k) && k == 1ull << 63);
    CHECK(!oi_key_from_hex("00000000000000FF", &k) && !oi_key_from_hex("0000000000000g00", &k));
    CHECK(oi_dest_of(0, 3) == 0 && oi_dest_of(~0ull, 3) == 2 && oi_dest_of(~0ull, 1) == 0);
}

static void test_insert_cases() {
    const vec a = splitmix(11, 50);
    vec mid = splitmix(12, 40), below = splitmix(13, 30), above = splitmix(14, 30);
    for (auto& x : mid) x = (x >> 2) | (1ull << 62);
    for (auto& x : below) x >>= 3;
    for (auto& x : above) x |= 1ull << 63;
    const vec a20(a.begin(), a.begin() + 20);
    vec arev(a.rbegin(), a.rend());
    vec dup(a.begin(), a.begin() + 10);
    dup.insert(dup.end(), a.rend() - 10, a.rend());
    dup.insert(dup.end(), a.begin() + 5, a.begin() + 15);
    dup.insert(dup.end(), a.begin(), a.begin() + 3);
    const vec g1 = splitmix(15, 10), g2 = splitmix(16, 30);
    vec g3 = splitmix(17, 200);
    g3.insert(g3.end(), g1.begin(), g1.end());
    const vec e = edge_keys();
    vec e2;
    for (size_t i = 0; i < e.size(); i += 2) e2.push_back(e[i]);
    const vec sp = shared_prefix_keys(300);
    const vec sp100(sp.begin(), sp.begin() + 100);
    run_steps("empty", {{a20, vals_for(a20, 1)}});
    run_steps("all_present", {{a, vals_for(a, 2)}, {arev, vals_for(a, 3)}});
    run_steps("dups_in_input", {{dup, vals_for(dup, 4)}});
    run_steps("below_min", {{mid, vals_for(mid, 5)}, {below, vals_for(below, 6)}});
    run_steps("above_max", {{mid, vals_for(mid, 7)}, {above, vals_for(above, 8)}});
    run_steps("three_growth", {{g1, vals_for(g1, 9)}, {g2, vals_for(g2, 10)}, {g3, vals_for(g3, 11)}});
    run_steps("edges", {{e2, vals_for(e2, 12)}, {e, vals_for(e, 13)}});
    run_steps("shared_prefix", {{sp100, vals_for(sp100, 14)}, {sp, vals_for(sp, 15)}});
    // the shard filter: every part of nparts 1, 2, 3, 8
    vec keys = splitmix(21, 500);
    keys.insert(keys.end(), e.begin(), e.end());
    const int parts[4] = {1, 2, 3, 8};
    for (int np : parts)
        for (int p = 0; p < np; p++) run_steps("shard", {{keys, vals_for(keys, 22)}}, np, p);
    // sizes around the directory's thresholds, one insert each and one key at a time
    for (size_t n : {0u, 1u, 2u, 15u, 16u, 17u, 255u, 256u, 257u, 4097u}) {
        const vec k = splitmix(1000 + n, n);
        run_steps("sizes", {{k, vals_for(k, 31)}});
    }
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(1, 0, &x) == SD_OK);
    model_t m;
    const vec one = splitmix(5, 70);
    for (size_t i = 0; i < one.size(); i++) {
        uint64_t taken = 0;
        const uint64_t v = i;
        CHECK(sd_cpu_object_index_insert(x, &one[i], &v, 1, &taken) == SD_OK && taken == 1);
        m[one[i]] = v;
    }
    check_equals_model(x, m);
    sd_cpu_object_index_destroy(x);
}

// sd_cpu_dedup_owners_indexed against the rule written out, and index == NULL = the plain rule
static void test_owners() {
    const uint64_t chunk = 7;
    const vec pool = splitmix(61, 120);
    const vec pick = splitmix(62, 600);
    std::vector<std::pair<uint64_t, uint64_t>> recs;  // (key, index)
    for (uint64_t i = 0; i < 600; i++) recs.push_back({pool[pick[i] % pool.size()], 1000 + i});
    std::sort(recs.begin(), recs.end());
    vec flat, rep;
    for (size_t i = 0; i < recs.size(); i++) {
        flat.push_back(recs[i].first);
        flat.push_back(recs[i].second);
        rep.push_back(i && recs[i - 1].first == recs[i].first ? rep[i - 1] : recs[i].second);
    }
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(1, 0, &x) == SD_OK);
    model_t m;
    vec known(pool.begin(), pool.begin() + 60);
    const vec kv = vals_for(known, 63);
    CHECK(sd_cpu_object_index_insert(x, known.data(), kv.data(), known.size(), nullptr) == SD_OK);
    model_insert(m, known, kv, 1, 0);
    const size_t n = recs.size();
    vec owner(n + 1, 5), plain(n + 1, 5), fresh(2 * n + 2, 6);
    std::vector<uint8_t> ex(n + 1, 3);
    uint64_t n_new = ~0ull;
    CHECK(sd_cpu_dedup_owners_indexed(x, flat.data(), n, rep.data(), chunk, owner.data(), ex.data(), fresh.data(),
                                      &n_new) == SD_OK);
    CHECK(sd_cpu_dedup_owners_indexed(nullptr, flat.data(), n, rep.data(), chunk, plain.data(), nullptr, nullptr,
                                      nullptr) == SD_OK);
    uint64_t heads = 0, hits = 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t idx = recs[i].second, want_plain = idx / chunk == rep[i] / chunk ? idx : rep[i];
        CHECK(plain[i] == want_plain);
        const auto it = m.find(recs[i].first);
        CHECK(ex[i] == (it != m.end() ? 1 : 0));
        CHECK(owner[i] == (it != m.end() ? it->second : want_plain));
        hits += it != m.end();
        if (it == m.end() && (i == 0 || recs[i - 1].first != recs[i].first)) {
            CHECK(heads < n_new && fresh[2 * heads] == recs[i].first && fresh[2 * heads + 1] == rep[i]);
            heads++;
        }
    }
    CHECK(heads == n_new && hits > 0 && hits < n);
    CHECK(owner[n] == 5 && plain[n] == 5 && ex[n] == 3 && fresh[2 * n_new] == 6);  // nothing past the rows
    uint64_t zero = 9;
    CHECK(sd_cpu_dedup_owners_indexed(x, nullptr, 0, nullptr, chunk, nullptr, nullptr, nullptr, &zero) == SD_OK && zero == 0);
    CHECK(sd_cpu_dedup_owners_indexed(x, flat.data(), n, rep.data(), 0, owner.data(), ex.data(), fresh.data(), &n_new) ==
          SD_ERR_INVALID);
    sd_cpu_object_index_destroy(x);
}

// concurrent lookups on one index are safe (the header's promise); inserts are exclusive
static void test_concurrent_lookups() {
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(1, 0, &x) == SD_OK);
    const vec k = splitmix(71, 5000), v = vals_for(k, 72);
    CHECK(sd_cpu_object_index_insert(x, k.data(), v.data(), k.size(), nullptr) == SD_OK);
    std::vector<int> bad(4, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
        th.emplace_back([&, t] {
            vec ids(k.size());
            std::vector<uint8_t> found(k.size());
            for (int rep = 0; rep < 3; rep++) {
                if (sd_cpu_object_index_lookup(x, k.data(), k.size(), ids.data(), found.data()) != SD_OK) bad[t]++;
                for (size_t i = 0; i < k.size(); i++) bad[t] += !(found[i] == 1 && ids[i] == v[i]);
            }
        });
    for (auto& t : th) t.join();
    for (int b : bad) CHECK(b == 0);
    sd_cpu_object_index_destroy(x);
}

static void test_arguments() {
    sd_cpu_object_index* x = nullptr;
    CHECK(sd_cpu_object_index_create(0, 0, &x) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_create(65, 0, &x) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_create(2, 2, &x) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_create(1, 0, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_create(1, 0, &x) == SD_OK);
    uint64_t n = 5, taken = 5;
    CHECK(sd_cpu_object_index_count(nullptr, &n) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_insert(x, nullptr, nullptr, 3, &taken) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_insert(x, nullptr, nullptr, 0, &taken) == SD_OK && taken == 0);  // m == 0: a no-op
    CHECK(sd_cpu_object_index_lookup(x, nullptr, 0, nullptr, nullptr) == SD_OK);
    CHECK(sd_cpu_object_index_lookup(x, nullptr, 2, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_count(x, &n) == SD_OK && n == 0);
    sd_cpu_object_index_destroy(x);
    sd_cpu_object_index_destroy(nullptr);
}

int main() {
    test_policies();
    test_arguments();
    test_insert_cases();
    test_owners();
    test_concurrent_lookups();
    if (g_fail) {
        printf("object_index_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_selftest: ok\n");
    return 0;
}
