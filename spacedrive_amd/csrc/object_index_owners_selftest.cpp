// object_index_owners_selftest.cpp -- the Object index's owners mode in the host code
// (object_index_host.cpp: sd_cpu_object_index_create_ex and the sd_cpu_* calls in that mode;
// object_index.h: the (key, id) bound and the "links asked >= links held" rule the kernels
// share) against a std::map model (key, id) -> links that follows include/sd_cas.h word for
// word: seeded scripts of insert / remove with ids / remove without / remove_objects / links /
// lookup; the entry counts at which the directory bits and the tiles change; a run of two
// across positions 255 | 256 and one of 3000 owners; 70 000 copies of one pair; the capacity
// rule with the link counts; the shard union; the fence between the modes; and concurrent
// reads between writes.  A program of its own: built plain for the CPU suite (`make
// object-index-owners-selftest`, tests/test_object_index_owners.py) and under ASan + UBSan and
// TSan (`make sanitize-object-index-owners`, logs in profiles/object_index/).
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
typedef std::map<pair_t, uint64_t> model_t;
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
    uint64_t count() const {
        uint64_t n = ~0ull;
        CHECK(sd_cpu_object_index_count(x, &n) == SD_OK);
        return n;
    }
};

// ---- the model: include/sd_cas.h, the owners mode
static uint64_t model_insert(model_t& m, const vec& k, const vec& v, int nparts, int part) {
    uint64_t taken = 0;
    for (size_t i = 0; i < k.size(); i++) {
        if (oi_dest_of(k[i], nparts) != (uint32_t)part) continue;
        uint64_t& l = m[pair_t(k[i], v[i])];
        taken += l == 0;
        l++;
    }
    return taken;
}

static vec model_drop(model_t& m, const std::set<pair_t>& gone) {
    vec out;
    for (const pair_t& p : gone) {
        out.push_back(p.first), out.push_back(p.second);
        m.erase(p);
    }
    return out;
}

static vec model_remove(model_t& m, const vec& k, const vec* ids) {
    std::set<pair_t> gone;
    if (!ids) {
        const std::set<uint64_t> want(k.begin(), k.end());
        for (const auto& e : m)
            if (want.count(e.first.first)) gone.insert(e.first);
        return model_drop(m, gone);
    }
    std::map<pair_t, uint64_t> asked;
    for (size_t i = 0; i < k.size(); i++) asked[pair_t(k[i], (*ids)[i])]++;
    for (const auto& a : asked) {
        const auto it = m.find(a.first);
        if (it == m.end()) continue;
        if (a.second >= it->second) gone.insert(a.first);
        else it->second -= a.second;
    }
    return model_drop(m, gone);
}

static vec model_remove_objects(model_t& m, const vec& ids) {
    const std::set<uint64_t> want(ids.begin(), ids.end());
    std::set<pair_t> gone;
    for (const auto& e : m)
        if (want.count(e.first.second)) gone.insert(e.first);
    return model_drop(m, gone);
}

// the index equals the model: entries in (key, id) order with their links; links() of every
// entry and of a neighbour; lookup gives each key's smallest id
static void check_equal(const index_t& ix, const model_t& m) {
    const uint64_t n = ix.count();
    CHECK(n == m.size());
    vec k(n + 1, FILL), v(n + 1, FILL), l(n + 1, FILL);
    CHECK(sd_cpu_object_index_export_links(ix.x, k.data(), v.data(), l.data(), n) == SD_OK);
    CHECK(k[n] == FILL && v[n] == FILL && l[n] == FILL);
    size_t i = 0;
    vec qk, qv, want, first_k, first_v;
    for (const auto& e : m) {
        if (i < n) CHECK(k[i] == e.first.first && v[i] == e.first.second && l[i] == e.second);
        i++;
        qk.push_back(e.first.first), qv.push_back(e.first.second), want.push_back(e.second);
        qk.push_back(e.first.first), qv.push_back(e.first.second + 1);
        want.push_back(m.count(pair_t(e.first.first, e.first.second + 1)) ? m.at(pair_t(e.first.first, e.first.second + 1)) : 0);
        if (first_k.empty() || first_k.back() != e.first.first) first_k.push_back(e.first.first), first_v.push_back(e.first.second);
    }
    vec got(qk.size() + 1, FILL);
    CHECK(sd_cpu_object_index_links(ix.x, qk.data(), qv.data(), qk.size(), got.data()) == SD_OK);
    got.pop_back();
    CHECK(got == want);
    first_k.push_back(first_k.empty() ? 5 : first_k.back() + 1);  // mostly absent
    vec ids(first_k.size());
    std::vector<uint8_t> found(first_k.size());
    CHECK(sd_cpu_object_index_lookup(ix.x, first_k.data(), first_k.size(), ids.data(), found.data()) == SD_OK);
    for (size_t j = 0; j + 1 < first_k.size(); j++) CHECK(found[j] == 1 && ids[j] == first_v[j]);
}

static void do_insert(index_t& ix, model_t& m, const vec& k, const vec& v) {
    uint64_t taken = ~0ull;
    CHECK(sd_cpu_object_index_insert(ix.x, k.data(), v.data(), k.size(), &taken) == SD_OK);
    CHECK(taken == model_insert(m, k, v, ix.nparts, ix.part));
}

static void check_removed(const vec& want, const vec& out, uint64_t removed) {
    CHECK(removed * 2 == want.size());
    CHECK(std::equal(want.begin(), want.end(), out.begin()));
    for (size_t i = want.size(); i < out.size(); i++) CHECK(out[i] == FILL);  // nothing past the count
}

static void do_remove(index_t& ix, model_t& m, const vec& k, const vec* ids) {
    const uint64_t cap = ix.count() + 2;
    vec out(2 * cap, FILL);
    uint64_t removed = ~0ull;
    CHECK(sd_cpu_object_index_remove(ix.x, k.data(), ids ? ids->data() : nullptr, k.size(), out.data(), cap, &removed) == SD_OK);
    check_removed(model_remove(m, k, ids), out, removed);
}

static void do_remove_objects(index_t& ix, model_t& m, const vec& ids) {
    const uint64_t cap = ix.count() + 2;
    vec out(2 * cap, FILL);
    uint64_t removed = ~0ull;
    CHECK(sd_cpu_object_index_remove_objects(ix.x, ids.data(), ids.size(), out.data(), cap, &removed) == SD_OK);
    check_removed(model_remove_objects(m, ids), out, removed);
}

// ---- seeded scripts over small pools: pairs repeat, keys have several owners
static void seeded_scripts() {
    for (uint64_t seed = 1; seed <= 6; seed++) {
        vec keys = splitmix(500 + seed, 24);
        const vec edges = {0, 1, (1ull << 63) - 1, 1ull << 63, ~0ull - 1, ~0ull};
        keys.insert(keys.end(), edges.begin(), edges.end());
        vec ids = splitmix(600 + seed, 8);
        ids.push_back(0), ids.push_back(~0ull);
        const vec r = splitmix(seed, 40 * 700);
        size_t at = 0;
        index_t ix;
        model_t m;
        for (int step = 0; step < 40; step++) {
            const uint64_t kind = step < 3 ? 0 : r[at++] % 8;
            static const size_t counts[4] = {1, 5, 60, 300};
            const size_t cnt = counts[r[at++] % 4];
            vec k, v;
            if (kind <= 3) {  // insert, or remove with ids: drawn pairs repeat and miss
                for (size_t i = 0; i < cnt; i++) k.push_back(keys[r[at++] % keys.size()]), v.push_back(ids[r[at++] % ids.size()]);
                if (kind <= 1) do_insert(ix, m, k, v);
                else {
                    // and, for a few held pairs, one link less than held, as many, and more
                    size_t j = 0;
                    for (const auto& e : m) {
                        if (j++ % 7 != (size_t)step % 7) continue;
                        const uint64_t ask = e.second - 1 + j % 3;
                        for (uint64_t c = 0; c < ask; c++) k.push_back(e.first.first), v.push_back(e.first.second);
                    }
                    do_remove(ix, m, k, &v);
                }
            } else if (kind <= 5) {
                for (int i = 0; i < 3; i++) k.push_back(keys[r[at++] % keys.size()]);
                do_remove(ix, m, k, nullptr);
            } else {
                for (int i = 0; i < 2; i++) v.push_back(ids[r[at++] % ids.size()]);
                v.push_back(r[at++]);
                do_remove_objects(ix, m, v);
            }
            check_equal(ix, m);
        }
    }
}

// ---- shapes
static void shaped_pairs(size_t n, vec* k, vec* v) {
    const vec a = splitmix(4000 + n, n);
    k->clear(), v->clear();
    for (size_t i = 0; i < n; i++) {
        // runs of equal keys at both ends, every fourth key owned twice, ids 0 and 2^64 - 1
        const uint64_t key = i < 3 ? 0 : i + 3 >= n ? ~0ull : (i % 4 == 1 ? a[i - 1] : a[i]);
        k->push_back(key);
        v->push_back(i % 11 == 0 ? 0 : i % 11 == 1 ? ~0ull : 7 + i);
    }
}

static void entry_counts() {
    const size_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097, 262144 + 300};
    for (size_t n : sizes) {
        vec k, v;
        shaped_pairs(n, &k, &v);
        index_t ix;
        model_t m;
        vec ik, iv;
        for (size_t i = 0; i < n; i++)
            for (size_t c = 0; c < 1u + (i % 3 == 0) + (i % 5 == 0); c++) ik.push_back(k[i]), iv.push_back(v[i]);
        const vec sh = splitmix(n + 2, ik.size());
        for (size_t i = 0; i < ik.size(); i++) {  // a shuffle: the order of the pairs does not matter
            const size_t j = sh[i] % ik.size();
            std::swap(ik[i], ik[j]), std::swap(iv[i], iv[j]);
        }
        do_insert(ix, m, ik, iv);
        CHECK(ix.count() == n);
        const bool walk = n <= 4097;  // the model comparison walks every entry
        if (walk) check_equal(ix, m);
        do_remove(ix, m, k, &v);  // one link of every pair: asked < held, asked = held
        vec qk, qv;
        for (size_t i = 0; i < n; i += 4)
            for (int c = 0; c < 3; c++) qk.push_back(k[i]), qv.push_back(v[i]);
        do_remove(ix, m, qk, &qv);  // asked > held, and absent pairs
        if (walk) check_equal(ix, m);
        qk.clear();
        for (size_t i = 1; i < n; i += 7) qk.push_back(k[i]);
        do_remove(ix, m, qk, nullptr);
        do_remove_objects(ix, m, {0, ~0ull, 12345});
        if (walk) check_equal(ix, m);
        do_insert(ix, m, ik, iv);
        CHECK(ix.count() == n);
        vec all_k = ik, all_v = iv;
        all_k.insert(all_k.end(), ik.begin(), ik.end()), all_v.insert(all_v.end(), iv.begin(), iv.end());
        do_remove(ix, m, all_k, &all_v);  // everything
        CHECK(ix.count() == 0 && m.empty());
        do_insert(ix, m, k, v);  // and an insert into the emptied index
        CHECK(ix.count() == n);
        check_equal(ix, m);
    }
}

static void runs_and_copies() {
    // two owners of one key across positions 255 | 256
    vec ks = splitmix(321, 599);
    std::sort(ks.begin(), ks.end());
    vec k = ks, v(599, 10);
    k.push_back(ks[255]), v.push_back(4);
    {
        index_t ix;
        model_t m;
        do_insert(ix, m, k, v);
        vec ek(600), ev(600), el(600);
        CHECK(sd_cpu_object_index_export_links(ix.x, ek.data(), ev.data(), el.data(), 600) == SD_OK);
        CHECK(ek[255] == ks[255] && ek[256] == ks[255] && ev[255] == 4 && ev[256] == 10);
        const vec one = {ks[255]}, ten = {10}, four = {4};
        do_remove(ix, m, one, &ten);
        check_equal(ix, m);
        do_insert(ix, m, k, v);
        do_remove(ix, m, one, &four);
        check_equal(ix, m);
        do_remove(ix, m, one, nullptr);
        check_equal(ix, m);
    }
    // 3000 owners of one key among 2000 entries
    {
        index_t ix;
        model_t m;
        vec rk = splitmix(654, 2000), rv = splitmix(656, 2000);
        const uint64_t key = rk[7] ^ (1ull << 20);
        const vec owners = splitmix(655, 3000);
        for (uint64_t o : owners) rk.push_back(key), rv.push_back(o);
        do_insert(ix, m, rk, rv);
        CHECK(ix.count() == 5000);
        do_remove(ix, m, vec(5, key), &owners);  // vec(5, key) pairs with the first five owners
        do_remove_objects(ix, m, vec(owners.begin() + 100, owners.begin() + 110));
        check_equal(ix, m);
        do_insert(ix, m, rk, rv);
        do_remove(ix, m, {key}, nullptr);
        CHECK(ix.count() == 2000);
        check_equal(ix, m);
    }
    // 70 000 copies of one pair: one entry, 70 000 links
    {
        index_t ix;
        model_t m;
        do_insert(ix, m, vec(70000, 42), vec(70000, 9));
        CHECK(ix.count() == 1 && m.begin()->second == 70000);
        const vec fewer_k(69999, 42), fewer_v(69999, 9);
        do_remove(ix, m, fewer_k, &fewer_v);
        CHECK(ix.count() == 1 && m.begin()->second == 1);
        check_equal(ix, m);
    }
}

// short by one: nothing changes, the links of the entries that would have survived included;
// no output buffer still reports the count
static void capacity_rule() {
    vec k, v;
    shaped_pairs(1025, &k, &v);
    vec ik = k, iv = v;
    ik.insert(ik.end(), k.begin(), k.begin() + 500), iv.insert(iv.end(), v.begin(), v.begin() + 500);
    for (int by = 0; by < 3; by++) {
        index_t ix;
        model_t m;
        do_insert(ix, m, ik, iv);
        model_t after = m;
        const vec ids = {0, 7 + 5, 7 + 6};
        const vec want = by == 0 ? model_remove(after, k, &v) : by == 1 ? model_remove(after, vec(k.begin(), k.begin() + 40), nullptr)
                                                                        : model_remove_objects(after, ids);
        const uint64_t r = want.size() / 2;
        CHECK(r > 1 && r < m.size());
        vec out(2 * r + 4, FILL);
        uint64_t removed = 0;
        auto call = [&](uint64_t* o, uint64_t cap) {
            return by == 0   ? sd_cpu_object_index_remove(ix.x, k.data(), v.data(), k.size(), o, cap, &removed)
                   : by == 1 ? sd_cpu_object_index_remove(ix.x, k.data(), nullptr, 40, o, cap, &removed)
                             : sd_cpu_object_index_remove_objects(ix.x, ids.data(), ids.size(), o, cap, &removed);
        };
        CHECK(call(out.data(), r - 1) == SD_ERR_CAPACITY && removed == r);
        for (uint64_t x : out) CHECK(x == FILL);
        check_equal(ix, m);  // entries and links as they were
        removed = 0;
        CHECK(call(nullptr, 0) == SD_OK && removed == r);
        check_equal(ix, after);
    }
}

static void shard_union() {
    vec k = splitmix(21, 3000), v = splitmix(23, 3000);
    for (auto& x : v) x %= 16;
    k.insert(k.end(), k.begin(), k.begin() + 1000), v.insert(v.end(), v.begin(), v.begin() + 1000);
    const vec rk(k.begin() + 500, k.begin() + 2000), rv(v.begin() + 500, v.begin() + 2000);
    index_t whole;
    model_t wm;
    do_insert(whole, wm, k, v);
    do_remove(whole, wm, rk, &rv);
    for (int nparts : {2, 3, 8}) {
        model_t all;
        for (int part = 0; part < nparts; part++) {
            index_t ix(nparts, part);
            model_t m;
            do_insert(ix, m, k, v);
            do_remove(ix, m, rk, &rv);
            check_equal(ix, m);
            for (const auto& e : m) {
                CHECK(oi_dest_of(e.first.first, nparts) == (uint32_t)part);
                all.insert(e);
            }
        }
        CHECK(all == wm);
    }
}

static void mode_fence() {
    index_t first(1, 0, 0), owners;
    int f = 7;
    CHECK(sd_cpu_object_index_flags(first.x, &f) == SD_OK && f == 0);
    CHECK(sd_cpu_object_index_flags(owners.x, &f) == SD_OK && f == SD_OBJECT_INDEX_OWNERS);
    const vec k = {1, 2, 3};
    vec out(3, FILL);
    uint64_t taken = 0;
    CHECK(sd_cpu_object_index_insert(first.x, k.data(), k.data(), 3, &taken) == SD_OK && taken == 3);
    CHECK(sd_cpu_object_index_links(first.x, k.data(), k.data(), 3, out.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_export_links(first.x, out.data(), out.data(), out.data(), 3) == SD_ERR_INVALID);
    CHECK(out == vec(3, FILL));
    sd_cpu_object_index* bad = nullptr;
    CHECK(sd_cpu_object_index_create_ex(1, 0, 2, &bad) == SD_ERR_INVALID && !bad);
    CHECK(sd_cpu_object_index_create_ex(1, 0, 1, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_links(owners.x, k.data(), nullptr, 3, out.data()) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_links(owners.x, nullptr, nullptr, 0, nullptr) == SD_OK);
}

// the header's thread-safety rule: reads run concurrently; writes are exclusive
static void concurrent_reads() {
    index_t ix;
    model_t m;
    vec k = splitmix(91, 20000), v = splitmix(92, 20000);
    for (auto& x : k) x %= 5000;
    for (auto& x : v) x %= 8;
    do_insert(ix, m, k, v);
    for (int round = 0; round < 3; round++) {
        std::vector<std::thread> ts;
        for (int t = 0; t < 4; t++)
            ts.emplace_back([&, t] {
                vec out(k.size());
                std::vector<uint8_t> found(k.size());
                CHECK(sd_cpu_object_index_links(ix.x, k.data(), v.data(), k.size(), out.data()) == SD_OK);
                for (size_t i = t; i < k.size(); i += 97) CHECK(out[i] == (m.count(pair_t(k[i], v[i])) ? m.at(pair_t(k[i], v[i])) : 0));
                CHECK(sd_cpu_object_index_lookup(ix.x, k.data(), k.size(), out.data(), found.data()) == SD_OK);
            });
        for (auto& t : ts) t.join();
        const vec rk(k.begin() + 1000 * round, k.begin() + 1000 * round + 3000);
        const vec rv(v.begin() + 1000 * round, v.begin() + 1000 * round + 3000);
        do_remove(ix, m, rk, &rv);
    }
    check_equal(ix, m);
}

int main() {
    seeded_scripts();
    entry_counts();
    runs_and_copies();
    capacity_rule();
    shard_union();
    mode_fence();
    concurrent_reads();
    if (g_fail) {
        printf("object_index_owners_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_owners_selftest: ok\n");
    return 0;
}
