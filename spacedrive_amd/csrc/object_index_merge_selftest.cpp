// object_index_merge_selftest.cpp -- sd_cpu_object_index_merge_objects (object_index_host.cpp; the
// rule oi_relabel / oi_map_contradicts of object_index.h, which the kernels share) against a
// map-of-maps model key -> (id -> links) that follows include/sd_cas.h word for word, and against
// a twin index rebuilt from scratch from the model after every call: seeded histories mixing
// merges (several ids to one, swaps, cycles, chains, ids nobody holds, self maps, repeats) with
// insert, removal by Object and apply; the entry counts at which the directory bits and the
// tiles change; a run of six owners across positions 255 | 256; 600 owners of one key sent to one
// id; the extremes of keys and ids; a count that crosses a directory-bits threshold; the first
// mode; the contradiction and the refusals; the shards; and concurrent reads between merges.  A
// program of its own: built plain for the CPU suite (`make object-index-merge-selftest`,
// tests/test_object_index_merge.py) and under ASan + UBSan and TSan (`make
// sanitize-object-index-merge`, logs in profiles/object_index/).
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
typedef std::map<uint64_t, std::map<uint64_t, uint64_t>> model_t;  // key -> (id -> links)
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

static uint64_t model_count(const model_t& m) {
    uint64_t n = 0;
    for (const auto& e : m) n += e.second.size();
    return n;
}

// ---- the model: include/sd_cas.h, merge Objects.  false on a contradiction (nothing changes).
static bool model_merge(model_t& m, const vec& from, const vec& to, uint64_t* moved, uint64_t* coalesced) {
    std::map<uint64_t, uint64_t> phi;
    for (size_t j = 0; j < from.size(); j++) {
        const auto it = phi.insert(std::make_pair(from[j], to[j])).first;
        if (it->second != to[j]) return false;
    }
    *moved = *coalesced = 0;
    const uint64_t before = model_count(m);
    model_t after;
    for (const auto& e : m)
        for (const auto& o : e.second) {
            const auto it = phi.find(o.first);
            const uint64_t w = it == phi.end() ? o.first : it->second;
            *moved += w != o.first;
            after[e.first][w] += o.second;  // applied once, to the ids as they stood
        }
    if (*moved == 0) return true;
    m.swap(after);
    *coalesced = before - model_count(m);
    return true;
}

static void model_insert(model_t& m, const vec& k, const vec& v, int nparts, int part) {
    for (size_t i = 0; i < k.size(); i++)
        if (oi_dest_of(k[i], nparts) == (uint32_t)part) m[k[i]][v[i]]++;
}

static void model_remove_objects(model_t& m, const vec& ids) {
    for (auto e = m.begin(); e != m.end();) {
        for (uint64_t o : ids) e->second.erase(o);
        e = e->second.empty() ? m.erase(e) : std::next(e);
    }
}

static void export_of(const index_t& ix, vec* k, vec* v, vec* l) {
    const uint64_t n = ix.count();
    k->assign(n + 1, FILL), v->assign(n + 1, FILL), l->assign(n + 1, FILL);
    CHECK(sd_cpu_object_index_export_links(ix.x, k->data(), v->data(), l->data(), n) == SD_OK);
    CHECK((*k)[n] == FILL && (*v)[n] == FILL && (*l)[n] == FILL);
    k->pop_back(), v->pop_back(), l->pop_back();
}

// the index equals the model entry for entry, lookup gives every key's smallest id, and a twin
// built from scratch from the model's relation (each pair once per link) exports the same arrays
static void check_equal(const index_t& ix, const model_t& m, bool with_twin = true) {
    vec k, v, l, first_k, first_v, rk, rv;
    export_of(ix, &k, &v, &l);
    CHECK(k.size() == model_count(m));
    size_t i = 0;
    for (const auto& e : m) {
        first_k.push_back(e.first), first_v.push_back(e.second.begin()->first);
        for (const auto& o : e.second) {
            if (i < k.size()) CHECK(k[i] == e.first && v[i] == o.first && l[i] == o.second);
            i++;
            for (uint64_t c = 0; c < o.second; c++) rk.push_back(e.first), rv.push_back(o.first);
        }
    }
    first_k.push_back(first_k.empty() ? 5 : first_k.back() + 1);
    vec ids(first_k.size());
    std::vector<uint8_t> found(first_k.size());
    CHECK(sd_cpu_object_index_lookup(ix.x, first_k.data(), first_k.size(), ids.data(), found.data()) == SD_OK);
    for (size_t j = 0; j + 1 < first_k.size(); j++) CHECK(found[j] == 1 && ids[j] == first_v[j]);
    if (!with_twin) return;
    index_t twin(ix.nparts, ix.part);
    CHECK(sd_cpu_object_index_insert(twin.x, rk.data(), rv.data(), rk.size(), nullptr) == SD_OK);
    vec tk, tv, tl;
    export_of(twin, &tk, &tv, &tl);
    CHECK(tk == k && tv == v && tl == l);
}

static void do_insert(index_t& ix, model_t& m, const vec& k, const vec& v) {
    CHECK(sd_cpu_object_index_insert(ix.x, k.data(), v.data(), k.size(), nullptr) == SD_OK);
    model_insert(m, k, v, ix.nparts, ix.part);
}

// merge on the index and the model; the reports agree
static void do_merge(index_t& ix, model_t& m, const vec& from, const vec& to, uint64_t* moved_out = nullptr,
                     uint64_t* coalesced_out = nullptr) {
    uint64_t moved = ~0ull, coalesced = ~0ull, want_moved = 0, want_coalesced = 0;
    CHECK(model_merge(m, from, to, &want_moved, &want_coalesced));
    CHECK(sd_cpu_object_index_merge_objects(ix.x, from.data(), to.data(), from.size(), &moved, &coalesced) == SD_OK);
    CHECK(moved == want_moved && coalesced == want_coalesced);
    if (moved_out) *moved_out = moved;
    if (coalesced_out) *coalesced_out = coalesced;
}

// ---- seeded histories over small pools: pairs repeat, keys have several owners
static void seeded_histories() {
    uint64_t seen[6] = {0};  // coalesced; moved only; nothing moved; swap; cycle; chain
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
            static const size_t counts[4] = {1, 5, 60, 300};
            const uint64_t what = step < 2 ? 0 : r[at++] % 8;
            if (what == 0 || what == 1) {
                const size_t cnt = counts[r[at++] % 4];
                vec ik, iv;
                for (size_t i = 0; i < cnt; i++) ik.push_back(keys[r[at++] % keys.size()]), iv.push_back(ids[r[at++] % ids.size()]);
                do_insert(ix, m, ik, iv);
            } else if (what == 2) {
                const vec gone = {ids[r[at++] % ids.size()]};
                CHECK(sd_cpu_object_index_remove_objects(ix.x, gone.data(), 1, nullptr, 0, nullptr) == SD_OK);
                model_remove_objects(m, gone);
            } else {
                const uint64_t a = ids[r[at++] % ids.size()], b = ids[r[at++] % ids.size()], c = ids[r[at++] % ids.size()];
                vec from, to;
                const int shape = step % 5;
                if (shape == 0 && a != b) from = {a, b}, to = {b, a}, seen[3]++;
                else if (shape == 1 && a != b && b != c && a != c) from = {a, b, c}, to = {b, c, a}, seen[4]++;
                else if (shape == 2 && a != b) from = {a, b}, to = {b, c}, seen[5]++;
                else if (shape == 3) from = {a, b, c ^ 4, a, c}, to = {c, c, a, c, c};  // several to one; absent; repeat; self
                else from = {a ^ 8, b ^ 8}, to = {a, a};                                 // ids nobody holds
                uint64_t moved, coalesced;
                do_merge(ix, m, from, to, &moved, &coalesced);
                seen[coalesced ? 0 : moved ? 1 : 2]++;
            }
            check_equal(ix, m);
        }
    }
    for (uint64_t s : seen) CHECK(s > 0);
}

// ---- shapes
// n entries, two owners per key (the last key one when n is odd): tests/object_index_merge_cases.py
// counted_case
static void counted_pairs(size_t n, vec* k, vec* v) {
    const size_t nk = (n + 1) / 2;
    const vec ks = splitmix(7000 + n, nk);
    k->clear(), v->clear();
    for (size_t j = 0; j < nk; j++) k->push_back(ks[j]), v->push_back(j % 5 + 1);
    for (size_t j = 0; j < n - nk; j++) k->push_back(ks[j]), v->push_back(j % 5 + 101);
}

static void entry_counts() {
    const size_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 1000, 4097, 262144 + 257};
    const vec from = {101, 102, 103, 104, 105, 4, 77}, to = {1, 9999, 104, 103, 105, 1, 1};
    for (size_t n : sizes) {
        vec k, v;
        counted_pairs(n, &k, &v);
        index_t ix;
        model_t m;
        do_insert(ix, m, k, v);
        CHECK(ix.count() == n);
        uint64_t moved, coalesced;
        do_merge(ix, m, from, to, &moved, &coalesced);
        CHECK((moved > 0) == (n >= 2) && (coalesced > 0) == (n >= 2));
        check_equal(ix, m);
        do_merge(ix, m, {1, 9999, 103, 104}, {101, 102, 104, 103});  // the first owners go; a swap again
        check_equal(ix, m);
    }
}

static void runs() {
    // six owners (100 .. 105) of one key across positions 255 | 256, every other entry id 10
    vec ks = splitmix(321, 595);
    std::sort(ks.begin(), ks.end());
    vec k = ks, v(595, 10);
    const uint64_t key = ks[253];
    v[253] = 100;
    for (uint64_t o = 101; o <= 105; o++) k.push_back(key), v.push_back(o);
    const vec froms[4] = {{101, 102, 103, 104, 105}, {100, 101, 102, 103, 104}, {100, 101, 102, 103, 104, 105},
                          {100, 101, 102, 103, 104, 105}};
    const uint64_t tos[4] = {100, 105, 3, ~0ull};
    for (int c = 0; c < 4; c++) {
        index_t ix;
        model_t m;
        do_insert(ix, m, k, v);
        uint64_t moved, coalesced;
        do_merge(ix, m, froms[c], vec(froms[c].size(), tos[c]), &moved, &coalesced);
        CHECK(moved == froms[c].size() && coalesced == 5 && ix.count() == 595);
        check_equal(ix, m);
    }
    // 600 owners of one key among 900 entries, all sent to one id: in the run, absent, itself a from
    vec rk = splitmix(654, 900), rv(900, 1);
    const uint64_t run_key = rk[7] ^ (1ull << 20);
    vec owners = splitmix(655, 600);
    for (auto& o : owners) o |= 4;
    std::sort(owners.begin(), owners.end());
    for (uint64_t o : owners) rk.push_back(run_key), rv.push_back(o);
    const uint64_t mid = owners[300];
    for (int c = 0; c < 3; c++) {
        index_t ix;
        model_t m;
        do_insert(ix, m, rk, rv);
        vec from, to;
        for (uint64_t o : owners)
            if (c == 1 || o != mid) from.push_back(o), to.push_back(c == 1 ? 2 : mid);
        if (c == 2) from.push_back(mid), to.push_back(3);
        uint64_t moved, coalesced;
        do_merge(ix, m, from, to, &moved, &coalesced);
        CHECK(moved == from.size() && coalesced == (c == 2 ? 598u : 599u));
        check_equal(ix, m);
    }
}

static void extremes_and_directory_bits() {
    const vec k = {0, 0, 0, ~0ull, ~0ull, ~0ull, 7}, v = {0, 5, ~0ull, 0, 5, ~0ull, 5};
    const vec froms[4] = {{~0ull}, {0}, {0, ~0ull}, {5, 0}}, tos[4] = {{0}, {~0ull}, {~0ull, 0}, {~0ull, 5}};
    for (int c = 0; c < 4; c++) {
        index_t ix;
        model_t m;
        do_insert(ix, m, k, v);
        do_merge(ix, m, froms[c], tos[c]);
        check_equal(ix, m);
    }
    // 34 entries -> 17: the count crosses 32, where oi_dir_bits steps from 2 to 1
    CHECK(oi_dir_bits(34) == 2 && oi_dir_bits(32) == 2 && oi_dir_bits(31) == 1 && oi_dir_bits(17) == 1);
    vec dk = splitmix(91, 17), dv(17, 1);
    for (size_t i = 0; i < 17; i++) dk.push_back(dk[i]), dv.push_back(2);
    index_t ix;
    model_t m;
    do_insert(ix, m, dk, dv);
    uint64_t moved, coalesced;
    do_merge(ix, m, {2}, {1}, &moved, &coalesced);
    CHECK(moved == 17 && coalesced == 17 && ix.count() == 17);
    check_equal(ix, m);
}

// one entry per key: the ids change where they stand
static void first_mode() {
    index_t ix(1, 0, 0);
    const vec k = splitmix(5, 1000);
    vec v(1000);
    for (size_t i = 0; i < 1000; i++) v[i] = i % 7;
    CHECK(sd_cpu_object_index_insert(ix.x, k.data(), v.data(), 1000, nullptr) == SD_OK);
    const vec from = {1, 2, 77, 0, 0}, to = {2, 3, 1, ~0ull, ~0ull};
    uint64_t moved = 0, coalesced = 9;
    CHECK(sd_cpu_object_index_merge_objects(ix.x, from.data(), to.data(), from.size(), &moved, &coalesced) == SD_OK);
    uint64_t want = 0;
    for (uint64_t x : v) want += x <= 2;
    CHECK(moved == want && coalesced == 0 && ix.count() == 1000);
    vec ids(1000);
    std::vector<uint8_t> found(1000);
    CHECK(sd_cpu_object_index_lookup(ix.x, k.data(), 1000, ids.data(), found.data()) == SD_OK);
    for (size_t i = 0; i < 1000; i++) CHECK(found[i] && ids[i] == (v[i] == 0 ? ~0ull : v[i] == 1 ? 2 : v[i] == 2 ? 3 : v[i]));
    const vec cf = {5, 5}, ct = {1, 2};
    CHECK(sd_cpu_object_index_merge_objects(ix.x, cf.data(), ct.data(), 2, &moved, &coalesced) == SD_ERR_INVALID);
}

// a contradiction changes nothing; null lists; the no-ops
static void refusals() {
    vec k, v;
    counted_pairs(257, &k, &v);
    index_t ix;
    model_t m;
    do_insert(ix, m, k, v);
    const vec froms[3] = {{101, 102, 101}, {101, 101}, {77, 77}}, tos[3] = {{1, 2, 3}, {101, 1}, {1, 2}};
    uint64_t moved = 7, coalesced = 7;
    for (int c = 0; c < 3; c++) {
        model_t same = m;
        CHECK(!model_merge(same, froms[c], tos[c], &moved, &coalesced));
        CHECK(sd_cpu_object_index_merge_objects(ix.x, froms[c].data(), tos[c].data(), froms[c].size(), &moved, &coalesced) == SD_ERR_INVALID);
        check_equal(ix, m, false);
    }
    index_t empty;
    CHECK(sd_cpu_object_index_merge_objects(empty.x, froms[0].data(), tos[0].data(), 3, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_merge_objects(empty.x, froms[0].data(), tos[0].data(), 2, &moved, &coalesced) == SD_OK);
    CHECK(moved == 0 && coalesced == 0 && empty.count() == 0);
    CHECK(sd_cpu_object_index_merge_objects(nullptr, k.data(), k.data(), 1, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_merge_objects(ix.x, nullptr, k.data(), 1, nullptr, nullptr) == SD_ERR_INVALID);
    CHECK(sd_cpu_object_index_merge_objects(ix.x, k.data(), nullptr, 1, nullptr, nullptr) == SD_ERR_INVALID);
    moved = coalesced = 7;
    CHECK(sd_cpu_object_index_merge_objects(ix.x, nullptr, nullptr, 0, &moved, &coalesced) == SD_OK);
    CHECK(moved == 0 && coalesced == 0);
    const vec self = {1, 2, 101}, absent = {1ull << 40, 2ull << 40};
    do_merge(ix, m, self, self, &moved, &coalesced);  // from == to
    CHECK(moved == 0);
    do_merge(ix, m, absent, {1, 2}, &moved, &coalesced);
    CHECK(moved == 0);
    check_equal(ix, m);
}

// every part is handed the same map: the parts' entries are the whole index's, the reports add up
static void shards() {
    vec k, v;
    counted_pairs(3000, &k, &v);
    const vec from = {101, 102, 103, 104, 105, 4, 77}, to = {1, 9999, 104, 103, 105, 1, 1};
    index_t whole;
    model_t wm;
    do_insert(whole, wm, k, v);
    uint64_t w_moved, w_coalesced;
    do_merge(whole, wm, from, to, &w_moved, &w_coalesced);
    for (int nparts : {2, 4}) {
        model_t all;
        uint64_t moved = 0, coalesced = 0;
        for (int part = 0; part < nparts; part++) {
            index_t ix(nparts, part);
            model_t m;
            do_insert(ix, m, k, v);
            uint64_t mv, co;
            do_merge(ix, m, from, to, &mv, &co);
            check_equal(ix, m);
            moved += mv, coalesced += co;
            for (const auto& e : m) {
                CHECK(oi_dest_of(e.first, nparts) == (uint32_t)part);
                all.insert(e);
            }
        }
        CHECK(all == wm && moved == w_moved && coalesced == w_coalesced);
    }
}

// the header's thread-safety rule: reads run concurrently; the merge is exclusive
static void concurrent_reads() {
    index_t ix;
    model_t m;
    vec k = splitmix(91, 20000), v = splitmix(92, 20000);
    for (auto& x : k) x %= 5000;
    for (auto& x : v) x %= 8;
    do_insert(ix, m, k, v);
    for (uint64_t round = 0; round < 3; round++) {
        std::vector<std::thread> ts;
        for (int t = 0; t < 4; t++)
            ts.emplace_back([&, t] {
                vec out(k.size());
                std::vector<uint8_t> found(k.size());
                CHECK(sd_cpu_object_index_links(ix.x, k.data(), v.data(), k.size(), out.data()) == SD_OK);
                for (size_t i = t; i < k.size(); i += 97) {
                    const auto e = m.find(k[i]);
                    const bool has = e != m.end() && e->second.count(v[i]);
                    CHECK(out[i] == (has ? e->second.at(v[i]) : 0));
                }
                CHECK(sd_cpu_object_index_lookup(ix.x, k.data(), k.size(), out.data(), found.data()) == SD_OK);
            });
        for (auto& t : ts) t.join();
        do_merge(ix, m, {2 * round, 2 * round + 1}, {2 * round + 1, 2 * round + 2});
    }
    check_equal(ix, m, false);
}

int main() {
    seeded_histories();
    entry_counts();
    runs();
    extremes_and_directory_bits();
    first_mode();
    refusals();
    shards();
    concurrent_reads();
    if (g_fail) {
        printf("object_index_merge_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("object_index_merge_selftest: ok\n");
    return 0;
}
