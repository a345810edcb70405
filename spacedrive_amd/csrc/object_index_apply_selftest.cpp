// object_index_apply_selftest.cpp -- sd_cpu_object_index_apply (object_index_host.cpp; the rule
// oi_links_after of object_index.h, which the kernels share) against a std::map model (key, id)
// -> links that follows include/sd_cas.h word for word, and against a twin index given remove
// then insert: seeded scripts mixing apply with the other calls; the entry counts at which the
// directory bits and the tiles change (a quarter leaves while as many enter, all leave, all
// leave and as many enter, pairs at rank 0 and rank n, the empty index); pairs entering around
// positions 255 | 256; 3000 owners of one key; 70 000 copies of one pair in both lists; the
// in-place case; the capacity rule; the refusals; the shard union; and concurrent reads between
// applies.  A program of its own: built plain for the CPU suite (`make
// object-index-apply-selftest`, tests/test_object_index_apply.py) and under ASan + UBSan and TSan
// (`make sanitize-object-index-apply`, logs in profiles/object_index/).
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

// ---- the model: include/sd_cas.h, apply.  Returns the dropped pairs; *taken = the entered ones.
static vec model_apply(model_t& m, const vec& rk, const vec& rv, const vec& ik, const vec& iv, int nparts, int part,
                       uint64_t* taken) {
    std::map<pair_t, uint64_t> asked, added;
    std::set<pair_t> named;
    for (size_t i = 0; i < rk.size(); i++) asked[pair_t(rk[i], rv[i])]++, named.insert(pair_t(rk[i], rv[i]));
    for (size_t i = 0; i < ik.size(); i++)
        if (oi_dest_of(ik[i], nparts) == (uint32_t)part) added[pair_t(ik[i], iv[i])]++, named.insert(pair_t(ik[i], iv[i]));
    vec gone;
    *taken = 0;
    for (const pair_t& p : named) {  // ascending (key, id)
        const auto it = m.find(p);
        const uint64_t held = it == m.end() ? 0 : it->second;
        const uint64_t a = asked.count(p) ? asked[p] : 0, b = added.count(p) ? added[p] : 0;
        const uint64_t kept = (held == 0 || (a != 0 && a >= held)) ? 0 : held - a;
        const uint64_t after = kept + b;
        if (held > 0 && after == 0) {
            gone.push_back(p.first), gone.push_back(p.second);
            m.erase(it);
        } else if (after > 0) {
            *taken += held == 0;
            m[p] = after;
        }
    }
    return gone;
}

static void export_of(const index_t& ix, vec* k, vec* v, vec* l) {
    const uint64_t n = ix.count();
    k->assign(n + 1, FILL), v->assign(n + 1, FILL), l->assign(n + 1, FILL);
    CHECK(sd_cpu_object_index_export_links(ix.x, k->data(), v->data(), l->data(), n) == SD_OK);
    CHECK((*k)[n] == FILL && (*v)[n] == FILL && (*l)[n] == FILL);
    k->pop_back(), v->pop_back(), l->pop_back();
}

// the index equals the model (entries in (key, id) order with their links; lookup gives each
// key's smallest id) and the twin, entry for entry
static void check_equal(const index_t& ix, const model_t& m, const index_t* twin = nullptr) {
    vec k, v, l;
    export_of(ix, &k, &v, &l);
    CHECK(k.size() == m.size());
    size_t i = 0;
    vec first_k, first_v;
    for (const auto& e : m) {
        if (i < k.size()) CHECK(k[i] == e.first.first && v[i] == e.first.second && l[i] == e.second);
        i++;
        if (first_k.empty() || first_k.back() != e.first.first) first_k.push_back(e.first.first), first_v.push_back(e.first.second);
    }
    first_k.push_back(first_k.empty() ? 5 : first_k.back() + 1);
    vec ids(first_k.size());
    std::vector<uint8_t> found(first_k.size());
    CHECK(sd_cpu_object_index_lookup(ix.x, first_k.data(), first_k.size(), ids.data(), found.data()) == SD_OK);
    for (size_t j = 0; j + 1 < first_k.size(); j++) CHECK(found[j] == 1 && ids[j] == first_v[j]);
    if (twin) {
        vec tk, tv, tl;
        export_of(*twin, &tk, &tv, &tl);
        CHECK(tk == k && tv == v && tl == l);
    }
}

static void do_insert(index_t& ix, model_t* m, const vec& k, const vec& v) {
    uint64_t taken = ~0ull, want = 0;
    CHECK(sd_cpu_object_index_insert(ix.x, k.data(), v.data(), k.size(), &taken) == SD_OK);
    if (m) {
        model_apply(*m, vec(), vec(), k, v, ix.nparts, ix.part, &want);
        CHECK(taken == want);
    }
}

// apply on the index and the model, remove then insert on the twin (may be null)
static void do_apply(index_t& ix, model_t& m, index_t* twin, const vec& rk, const vec& rv, const vec& ik, const vec& iv) {
    const uint64_t cap = ix.count() + 2;
    vec out(2 * cap, FILL);
    uint64_t removed = ~0ull, taken = ~0ull, want_taken = 0;
    CHECK(sd_cpu_object_index_apply(ix.x, rk.data(), rv.data(), rk.size(), ik.data(), iv.data(), ik.size(), out.data(),
                                    cap, &removed, &taken) == SD_OK);
    const vec want = model_apply(m, rk, rv, ik, iv, ix.nparts, ix.part, &want_taken);
    CHECK(removed * 2 == want.size() && taken == want_taken);
    CHECK(std::equal(want.begin(), want.end(), out.begin()));
    for (size_t i = want.size(); i < out.size(); i++) CHECK(out[i] == FILL);  // nothing past the count
    if (twin) {
        CHECK(sd_cpu_object_index_remove(twin->x, rk.data(), rv.data(), rk.size(), nullptr, 0, nullptr) == SD_OK);
        CHECK(sd_cpu_object_index_insert(twin->x, ik.data(), iv.data(), ik.size(), nullptr) == SD_OK);
    }
}

// ---- seeded scripts over small pools: pairs repeat, keys have several owners
static void seeded_scripts() {
    uint64_t seen[8] = {0};  // asked <, =, > held x added 0 / > 0; absent in the removal list; another id
    for (uint64_t seed = 1; seed <= 6; seed++) {
        vec keys = splitmix(500 + seed, 24);
        const vec edges = {0, 1, (1ull << 63) - 1, 1ull << 63, ~0ull - 1, ~0ull};
        keys.insert(keys.end(), edges.begin(), edges.end());
        vec ids = splitmix(600 + seed, 8);
        ids.push_back(0), ids.push_back(~0ull);
        const vec r = splitmix(seed, 40 * 1500);
        size_t at = 0;
        index_t ix, twin;
        model_t m;
        for (int step = 0; step < 40; step++) {
            static const size_t counts[4] = {1, 5, 60, 300};
            const size_t cnt = counts[r[at++] % 4];
            vec rk, rv, ik, iv;
            for (size_t i = 0; i < cnt; i++) ik.push_back(keys[r[at++] % keys.size()]), iv.push_back(ids[r[at++] % ids.size()]);
            if (step < 2 || r[at++] % 5 == 0) {
                do_insert(ix, &m, ik, iv), do_insert(twin, nullptr, ik, iv);
            } else {
                size_t j = 0;
                for (const auto& e : m) {  // for a few held pairs: one link less than held, as many, more
                    if (j++ % 5 != (size_t)step % 5) continue;
                    const uint64_t ask = e.second - 1 + j % 3, add = (j / 3) % 3;
                    for (uint64_t c = 0; c < ask; c++) rk.push_back(e.first.first), rv.push_back(e.first.second);
                    for (uint64_t c = 0; c < add; c++) ik.push_back(e.first.first), iv.push_back(e.first.second);
                    if (ask) seen[(ask < e.second ? 0 : ask == e.second ? 2 : 4) + (add ? 1 : 0)]++;
                    if (!m.count(pair_t(e.first.first, e.first.second ^ 1))) rk.push_back(e.first.first), rv.push_back(e.first.second ^ 1), seen[7]++;
                }
                for (int i = 0; i < 4; i++) {
                    const uint64_t pk = keys[r[at++] % keys.size()];
                    const pair_t p(pk, ids[r[at++] % ids.size()]);
                    rk.push_back(p.first), rv.push_back(p.second);
                    seen[6] += !m.count(p);
                }
                do_apply(ix, m, &twin, rk, rv, ik, iv);
            }
            check_equal(ix, m, &twin);
        }
    }
    for (uint64_t s : seen) CHECK(s > 0);
}

// ---- shapes
static void shaped_pairs(size_t n, vec* k, vec* v) {
    const vec a = splitmix(4000 + n, n);
    k->clear(), v->clear();
    for (size_t i = 0; i < n; i++) {
        // runs of equal keys at both ends, every fourth key owned twice, ids 0 and 2^64 - 1
        const uint64_t key = i < 3 ? 0 : i + 3 >= n ? ~0ull : (i % 4 == 1 ? a[i - 1] : a[i]);
        k->push_back(key);
        v->push_back(i % 11 == 0 ? 0 : i % 11 == 1 ? ~0ull - 1 : 7 + i);
    }
}

static void fresh_pairs(size_t n, uint64_t salt, vec* k, vec* v) {
    *k = splitmix(9000 + salt, n);
    v->assign(n, 0);
    for (size_t i = 0; i < n; i++) (*v)[i] = (1ull << 40) + i;  // no shaped pair has such an id
}

static void entry_counts() {
    const size_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4097, 262144 + 300};
    for (size_t n : sizes) {
        vec k, v, qk, qv, fk, fv, gk, gv;
        shaped_pairs(n, &k, &v);
        for (size_t i = 0; i < n; i += 4) qk.push_back(k[i]), qv.push_back(v[i]);
        fresh_pairs(qk.size(), n, &fk, &fv);
        fresh_pairs(n, n + 1, &gk, &gv);
        index_t ix, twin;
        model_t m;
        const bool walk = n <= 4097;  // the model comparison walks every entry
        do_apply(ix, m, &twin, {}, {}, k, v);  // on the empty index
        CHECK(ix.count() == n);
        do_apply(ix, m, &twin, qk, qv, fk, fv);  // every fourth leaves, as many enter: the count stands
        CHECK(ix.count() == n);
        if (walk) check_equal(ix, m, &twin);
        vec ak = k, av = v;
        ak.insert(ak.end(), fk.begin(), fk.end()), av.insert(av.end(), fv.begin(), fv.end());
        do_apply(ix, m, &twin, ak, av, {}, {});  // all leave, none enter
        CHECK(ix.count() == 0 && m.empty());
        do_apply(ix, m, &twin, k, v, {}, {});  // removals from the empty index
        do_insert(ix, &m, k, v), do_insert(twin, nullptr, k, v);
        do_apply(ix, m, &twin, k, v, gk, gv);  // all leave, n enter
        CHECK(ix.count() == n);
        do_apply(ix, m, &twin, {}, {}, {0, ~0ull}, {0, ~0ull});  // rank 0 and rank n
        CHECK(ix.count() == n + 2);
        check_equal(ix, m, &twin);
    }
}

static void runs_and_copies() {
    // pairs entering and entries leaving around positions 255 | 256, the two owners of one key
    vec ks = splitmix(321, 599);
    std::sort(ks.begin(), ks.end());
    vec k = ks, v(599, 10);
    k.push_back(ks[255]), v.push_back(4);
    const uint64_t key = ks[255];
    // between the two; leaving 255 / entering at 256; leaving 256 / entering at 255; around a leaving entry
    const vec rms[5][2] = {{vec(), vec()}, {vec{key}, vec{4}}, {vec{key}, vec{10}}, {vec{key}, vec{4}}, {vec{key}, vec{10}}};
    const vec ins[5][2] = {{vec{key}, vec{7}}, {vec{key}, vec{7}}, {vec{ks[254]}, vec{11}}, {vec{ks[254], key}, vec{11, 7}},
                           {vec{key, key}, vec{7, 11}}};
    for (int c = 0; c < 5; c++) {
        index_t ix, twin;
        model_t m;
        do_insert(ix, &m, k, v), do_insert(twin, nullptr, k, v);
        do_apply(ix, m, &twin, rms[c][0], rms[c][1], ins[c][0], ins[c][1]);
        CHECK(ix.count() == 600 + ins[c][0].size() - rms[c][0].size());
        check_equal(ix, m, &twin);
    }
    // 3000 owners of one key among 2000 entries: every second leaves, 1500 new ones enter
    {
        index_t ix, twin;
        model_t m;
        vec rk = splitmix(654, 2000), rv = splitmix(656, 2000);
        const uint64_t run_key = rk[7] ^ (1ull << 20);
        vec owners = splitmix(655, 3000);
        for (uint64_t o : owners) rk.push_back(run_key), rv.push_back(o);
        do_insert(ix, &m, rk, rv), do_insert(twin, nullptr, rk, rv);
        std::sort(owners.begin(), owners.end());
        vec gone;
        for (size_t i = 0; i < owners.size(); i += 2) gone.push_back(owners[i]);
        do_apply(ix, m, &twin, vec(1500, run_key), gone, vec(1500, run_key), splitmix(658, 1500));
        CHECK(ix.count() == 5000);
        check_equal(ix, m, &twin);
    }
    // 70 000 copies of one pair in each list: it stays, with 70 000 links
    {
        index_t ix, twin;
        model_t m;
        do_insert(ix, &m, {42, 43}, {9, 9}), do_insert(twin, nullptr, {42, 43}, {9, 9});
        const vec ck(70000, 42), cv(70000, 9);
        do_apply(ix, m, &twin, ck, cv, ck, cv);
        CHECK(ix.count() == 2 && m.begin()->second == 70000);
        check_equal(ix, m, &twin);
    }
}

// nothing leaves or enters: keys and ids stand, the links change
static void in_place() {
    vec k, v;
    shaped_pairs(1025, &k, &v);
    vec bk, bv, rk, rv, ik, iv;
    for (int c = 0; c < 3; c++) bk.insert(bk.end(), k.begin(), k.end()), bv.insert(bv.end(), v.begin(), v.end());
    for (size_t i = 0; i < k.size(); i++) {
        const int asks[4] = {1, 2, 0, 2}, adds[4] = {0, 1, 1, 2};
        for (int c = 0; c < asks[i % 4]; c++) rk.push_back(k[i]), rv.push_back(v[i]);
        for (int c = 0; c < adds[i % 4]; c++) ik.push_back(k[i]), iv.push_back(v[i]);
    }
    index_t ix, twin;
    model_t m;
    do_insert(ix, &m, bk, bv), do_insert(twin, nullptr, bk, bv);
    vec k0, v0, l0, k1, v1, l1;
    export_of(ix, &k0, &v0, &l0);
    do_apply(ix, m, &twin, rk, rv, ik, iv);
    export_of(ix, &k1, &v1, &l1);
    CHECK(k0 == k1 && v0 == v1 && l0 != l1);
    check_equal(ix, m, &twin);
}

// short by one: nothing changes -- no entry, no link count, no new pair; no output buffer still
// reports the counts
static void capacity_and_refusals() {
    vec k, v, fk, fv;
    shaped_pairs(1025, &k, &v);
    fresh_pairs(40, 9, &fk, &fv);
    vec bk = k, bv = v;
    bk.insert(bk.end(), k.begin(), k.begin() + 500), bv.insert(bv.end(), v.begin(), v.begin() + 500);
    vec ik = fk, iv = fv;
    ik.insert(ik.end(), k.begin() + 900, k.end()), iv.insert(iv.end(), v.begin() + 900, v.end());
    index_t ix;
    model_t m;
    do_insert(ix, &m, bk, bv);
    model_t after = m;
    uint64_t want_taken = 0;
    const vec want = model_apply(after, k, v, ik, iv, 1, 0, &want_taken);
    const uint64_t r = want.size() / 2;
    CHECK(r > 1 && r < m.size() && want_taken == 40);
    vec out(2 * r + 4, FILL);
    uint64_t removed = 0, taken = 7;
    CHECK(sd_cpu_object_index_apply(ix.x, k.data(), v.data(), k.size(), ik.data(), iv.data(), ik.size(), out.data(), r - 1,
                                    &removed, &taken) == SD_ERR_CAPACITY);
    CHECK(removed == r && taken == 0);
    for (uint64_t x : out) CHECK(x == FILL);
    check_equal(ix, m);
    // refusals: the removal list without ids; null lists; a first-mode index; and the no-op
    CHECK(sd_cpu_object_index_apply(ix.x, k.data(), nullptr, k.size(), nullptr, nullptr, 0, nullptr, 0, &removed, &taken) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_apply(ix.x, nullptr, v.data(), 3, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_apply(ix.x, nullptr, nullptr, 0, ik.data(), nullptr, 3, nullptr, 0, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_apply(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == SD_ERR_INVALID);
    index_t first(1, 0, 0);
    CHECK(sd_cpu_object_index_insert(first.x, k.data(), v.data(), 3, nullptr) == SD_OK);
    CHECK(sd_cpu_object_index_apply(first.x, k.data(), v.data(), 3, k.data(), v.data(), 3, nullptr, 0, &removed, &taken) == SD_ERR_INVALID);
    CHECK(first.count() == 1);  // keep first: the shaped pairs start with one key three times
    removed = taken = 7;
    CHECK(sd_cpu_object_index_apply(ix.x, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, &removed, &taken) == SD_OK);
    CHECK(removed == 0 && taken == 0);
    check_equal(ix, m);
    CHECK(sd_cpu_object_index_apply(ix.x, k.data(), v.data(), k.size(), ik.data(), iv.data(), ik.size(), nullptr, 0, &removed, &taken) == SD_OK);
    CHECK(removed == r && taken == want_taken);
    check_equal(ix, after);
}

static void shard_union() {
    vec k = splitmix(21, 3000), v = splitmix(23, 3000);
    for (auto& x : v) x %= 16;
    k.insert(k.end(), k.begin(), k.begin() + 1000), v.insert(v.end(), v.begin(), v.begin() + 1000);
    const vec rk(k.begin() + 500, k.begin() + 2000), rv(v.begin() + 500, v.begin() + 2000);
    vec ik = splitmix(25, 500), iv(500, 3);
    ik.insert(ik.end(), k.begin() + 1500, k.begin() + 2500), iv.insert(iv.end(), v.begin() + 1500, v.begin() + 2500);
    index_t whole;
    model_t wm;
    do_insert(whole, &wm, k, v);
    do_apply(whole, wm, nullptr, rk, rv, ik, iv);
    for (int nparts : {2, 3, 8}) {
        model_t all;
        for (int part = 0; part < nparts; part++) {
            index_t ix(nparts, part);
            model_t m;
            do_insert(ix, &m, k, v);
            do_apply(ix, m, nullptr, rk, rv, ik, iv);
            check_equal(ix, m);
            for (const auto& e : m) {
                CHECK(oi_dest_of(e.first.first, nparts) == (uint32_t)part);
                all.insert(e);
            }
        }
        CHECK(all == wm);
    }
}

// the header's thread-safety rule: reads run concurrently; apply is exclusive
static void concurrent_reads() {
    index_t ix;
    model_t m;
    vec k = splitmix(91, 20000), v = splitmix(92, 20000);
    for (auto& x : k) x %= 5000;
    for (auto& x : v) x %= 8;
    do_insert(ix, &m, k, v);
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
        vec ik(k.begin() + 2000 * round, k.begin() + 2000 * round + 2000), iv(2000, 9 + round);
        do_apply(ix, m, nullptr, rk, rv, ik, iv);
    }
    check_equal(ix, m);
}

int main() {
    seeded_scripts();
    entry_counts();
    runs_and_copies();
    in_place();
    capacity_and_refusals();
    shard_union();
    concurrent_reads();
    if (g_fail) {
        printf("object_index_apply_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_apply_selftest: ok\n");
    return 0;
}
