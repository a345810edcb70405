// cdc_delta_selftest.cpp -- the host twins of the CDC deltas (include/sd_cas.h, "Deltas") against a
// byte-at-a-time model, stand-alone: plain for the CPU test suite (tests/test_cdc_delta.py) and under
// ASan + UBSan and TSan (`make sanitize-cdc-delta`).
//
// The model knows nothing of representatives: a map from (length, id) to the first slot that has
// them, a literal buffer that grows by one memcpy per new chunk, and a rebuilt target that grows by
// one memcpy per chunk from wherever the map says its bytes are.  The twins' plan must give the
// model's offsets, statistics and (merged) runs, the pack its literal buffer, the apply its targets;
// bad recipes must be refused with the output as it was.
#include <stdio.h>
#include <string.h>

#include <array>
#include <map>
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

typedef std::vector<uint8_t> bytes;
typedef std::vector<uint64_t> u64s;

static uint64_t mix(uint64_t seed, uint64_t i) {  // splitmix64
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bytes content(uint64_t seed, uint64_t len) {
    bytes b(len);
    for (uint64_t i = 0; i < len; i++) b[i] = (uint8_t)mix(seed, i);
    return b;
}

static bytes cat(std::initializer_list<bytes> parts) {
    bytes out;
    for (const bytes& p : parts) out.insert(out.end(), p.begin(), p.end());
    return out;
}

static bytes slice(const bytes& b, size_t from, size_t to) { return bytes(b.begin() + from, b.begin() + to); }

struct batch_t {
    bytes buf;
    u64s offs, lens, base, chunks, rep;
    bytes ids;
    size_t n = 0;
};

// the files at 16-byte aligned starts, cut, hashed and grouped by the twins of the CDC section
static batch_t make(const std::vector<bytes>& files, sd_cdc_params pr) {
    batch_t b;
    b.n = files.size();
    uint64_t cur = 0;
    for (const bytes& f : files) {
        b.offs.push_back(cur);
        b.lens.push_back(f.size());
        cur = (cur + f.size() + 15) / 16 * 16 + 16;
    }
    b.buf.assign(cur + 64, 0xEE);
    for (size_t f = 0; f < b.n; f++)
        if (!files[f].empty()) memcpy(b.buf.data() + b.offs[f], files[f].data(), files[f].size());
    b.base.assign(b.n + 1, 0);
    uint64_t m = 0;
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), b.n, &pr, b.base.data(), nullptr, 0, &m, nullptr, 2) == SD_OK);
    b.chunks.assign(2 * m + 2, 0);
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), b.n, &pr, b.base.data(), b.chunks.data(), m, &m, nullptr, 2) ==
          SD_OK);
    b.ids.assign(32 * m + 32, 0);
    CHECK(sd_cpu_cdc_hash(b.buf.data(), b.offs.data(), b.lens.data(), b.n, b.base.data(), b.chunks.data(), b.ids.data(), 2) == SD_OK);
    b.rep.assign(m + 1, 0);
    CHECK(sd_cpu_cdc_shared(b.base.data(), b.n, b.chunks.data(), b.ids.data(), 0, b.rep.data(), nullptr, nullptr, nullptr, 0,
                            nullptr, nullptr) == SD_OK);
    return b;
}

struct answer_t {
    u64s lit_off, runs, files, stats;
    bytes lit;
    std::vector<bytes> targets;
    bool operator==(const answer_t& o) const {
        return lit_off == o.lit_off && runs == o.runs && files == o.files && stats == o.stats && lit == o.lit &&
               targets == o.targets;
    }
};

static answer_t model(const batch_t& b, size_t nb) {
    typedef std::pair<uint64_t, std::array<uint8_t, 32>> key_t;
    struct where_t { uint64_t src, off; };  // 1 + g and the offset in base file g, or 0 and the offset in the literals
    std::map<key_t, where_t> seen;
    auto key_of = [&](uint64_t s) {
        key_t k;
        k.first = b.chunks[2 * s + 1];
        memcpy(k.second.data(), b.ids.data() + 32 * s, 32);
        return k;
    };
    for (size_t g = 0; g < nb; g++)
        for (uint64_t s = b.base[g]; s < b.base[g + 1]; s++) seen.insert({key_of(s), {1 + g, b.chunks[2 * s]}});  // the first stays
    answer_t a;
    a.stats = {b.n - nb, b.base[b.n] - b.base[nb], 0, 0, 0, 0, 0, 0};
    for (size_t f = nb; f < b.n; f++) {
        u64s row = {b.base[f + 1] - b.base[f], 0, 0, 0, 0, 0};
        bytes target;
        bool open = false;
        for (uint64_t s = b.base[f]; s < b.base[f + 1]; s++) {
            const uint64_t len = b.chunks[2 * s + 1];
            const uint8_t* p = b.buf.data() + b.offs[f] + b.chunks[2 * s];
            if (len == 0) {
                a.stats[4]++;
                a.lit_off.push_back(~0ull);
                open = false;
                continue;
            }
            auto it = seen.find(key_of(s));
            where_t w;
            if (it == seen.end()) {  // new: its bytes join the literals
                w = {0, a.lit.size()};
                a.lit.insert(a.lit.end(), p, p + len);
                seen.insert({key_of(s), w});
                a.stats[4]++, a.stats[5] += len, row[3] += len;
                a.lit_off.push_back(w.off);
            } else {
                w = it->second;
                if (w.src) a.stats[2]++, a.stats[3] += len, row[1]++, row[2] += len;
                else a.stats[6]++, row[4] += len;
                a.lit_off.push_back(w.src ? ~0ull : w.off);
            }
            const uint8_t* from = w.src ? b.buf.data() + b.offs[w.src - 1] + w.off : a.lit.data() + w.off;
            const size_t at = target.size();
            target.resize(at + len);
            memcpy(target.data() + at, from, len);  // a chunk never overlaps what it is copied from
            const size_t r = a.runs.size();
            if (open && a.runs[r - 3] == w.src && a.runs[r - 2] + a.runs[r - 1] == w.off) a.runs[r - 1] += len;
            else a.runs.insert(a.runs.end(), {f - nb, w.src, w.off, len}), row[5]++;
            open = true;
        }
        CHECK(target.size() == b.lens[f] && (target.empty() || memcmp(target.data(), b.buf.data() + b.offs[f], target.size()) == 0));
        a.targets.push_back(target);
        a.files.insert(a.files.end(), row.begin(), row.end());
    }
    a.stats[7] = a.runs.size() / 4;
    return a;
}

static answer_t run(const batch_t& b, size_t nb, int nthreads) {
    answer_t a;
    const uint64_t mt = b.base[b.n] - b.base[nb];
    const size_t nt = b.n - nb;
    a.stats.assign(8, 0);
    uint64_t r = 0;
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), b.n, nb, b.chunks.data(), b.rep.data(), nullptr, nullptr, 0, &r, nullptr,
                                a.stats.data()) == SD_OK);
    CHECK(r == a.stats[7]);
    a.lit_off.assign(mt, 5), a.runs.assign(4 * r, 5), a.files.assign(6 * nt, 5);
    uint64_t r2 = 0;
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), b.n, nb, b.chunks.data(), b.rep.data(), a.lit_off.data(), a.runs.data(), r, &r2,
                                a.files.data(), a.stats.data()) == SD_OK);
    CHECK(r2 == r);
    a.lit.assign(a.stats[5], 0);
    CHECK(sd_cpu_cdc_delta_pack(b.base.data(), b.n, nb, b.offs.data(), b.chunks.data(), a.lit_off.data(), b.rep.data(),
                                b.buf.data(), a.lit.data()) == SD_OK);
    // the targets back to back in one buffer with a guard byte between them
    u64s oo, ol(b.lens.begin() + nb, b.lens.end());
    uint64_t cur = 1;
    for (uint64_t L : ol) oo.push_back(cur), cur += L + 1;
    bytes out(cur, 0xC3);
    CHECK(sd_cpu_cdc_delta_apply(a.runs.data(), r, b.offs.data(), b.lens.data(), nb, b.buf.data(), a.lit.data(), a.lit.size(),
                                 oo.data(), ol.data(), nt, out.data(), nthreads) == SD_OK);
    CHECK(out[0] == 0xC3);
    for (size_t t = 0; t < nt; t++) {
        a.targets.push_back(slice(out, oo[t], oo[t] + ol[t]));
        CHECK(out[oo[t] + ol[t]] == 0xC3);
    }
    return a;
}

static void test_against_the_model() {
    const sd_cdc_params pr = {8, 64, 1024, 0};
    const bytes A = content(1, 40000), B = content(2, 9000), C = content(3, 5000), ins = {1, 2, 3, 4, 5};
    const bytes zeros(3 * 1024 + 100, 0);
    const std::vector<std::vector<bytes>> sets = {
        {A, cat({slice(A, 0, 1000), ins, slice(A, 1000, A.size())})},            // five bytes inserted
        {A, B, A, cat({B, A}), cat({C, slice(A, 5000, 9000), C})},               // identical, joined, a chunk new twice
        {cat({slice(A, 0, 8000), slice(A, 0, 8000)}), slice(A, 0, 8000), zeros},  // the base holds chunks twice; constant bytes
        {bytes(), B, bytes(), slice(B, 100, 3000), bytes()},                      // empty files on both sides
    };
    for (const auto& files : sets) {
        const batch_t b = make(files, pr);
        for (size_t nb = 0; nb <= files.size(); nb++) {
            const answer_t want = model(b, nb);
            CHECK(want.stats[1] == want.stats[2] + want.stats[4] + want.stats[6]);
            CHECK(run(b, nb, 1) == want);
            CHECK(run(b, nb, 4) == want);
        }
    }
    const batch_t b = make(sets[0], pr);
    const answer_t a = model(b, 1);
    CHECK(a.stats[1] - a.stats[2] <= 3 && a.stats[5] <= 3 * 1024 && a.stats[7] <= 3);
}

static void test_capacity_and_refusals() {
    const sd_cdc_params pr = {8, 64, 1024, 0};
    const bytes A = content(7, 20000), B = content(8, 6000);
    const batch_t b = make({A, B, cat({B, content(9, 3000), A})}, pr);
    const answer_t want = model(b, 2);
    const uint64_t r = want.stats[7];
    CHECK(r >= 3);
    u64s runs(4 * r, 7), stats(8, 7);
    uint64_t got = 0;
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), 3, 2, b.chunks.data(), b.rep.data(), nullptr, runs.data(), r - 1, &got, nullptr,
                                stats.data()) == SD_ERR_CAPACITY);
    CHECK(got == r && stats == want.stats && runs == u64s(4 * r, 7));
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), 3, 4, b.chunks.data(), b.rep.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr) ==
          SD_ERR_INVALID);
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), 3, 2, nullptr, b.rep.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr) ==
          SD_ERR_INVALID);
    CHECK(sd_cpu_cdc_delta_plan(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, &got, nullptr, stats.data()) == SD_OK);
    CHECK(got == 0 && stats == u64s(8, 0));
    u64s rep = b.rep;
    rep[b.base[2]] = b.base[2] + 1;  // a representative behind its slot
    CHECK(sd_cpu_cdc_delta_plan(b.base.data(), 3, 2, b.chunks.data(), rep.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr) ==
          SD_ERR_INVALID);

    // bad recipes: refused, and the output as it was
    const u64s oo = {3}, ol = {b.lens[2]};
    const bytes start(b.lens[2] + 8, 0x5A);
    auto apply = [&](const u64s& rn, bytes& out) {
        return sd_cpu_cdc_delta_apply(rn.data(), rn.size() / 4, b.offs.data(), b.lens.data(), 2, b.buf.data(), want.lit.data(),
                                      want.lit.size(), oo.data(), ol.data(), 1, out.data(), 3);
    };
    bytes out = start;
    CHECK(apply(want.runs, out) == SD_OK && slice(out, 3, 3 + ol[0]) == want.targets[0] && out[2] == 0x5A);
    struct edit { size_t j, col; uint64_t val; };
    const uint64_t L = b.lens[want.runs[1] - 1] - want.runs[2];  // what the first run's source has from its offset on
    CHECK(want.runs[1] != 0);
    const edit edits[] = {
        {0, 1, 3},                              // a source beyond n_base
        {0, 3, L + 1},                          // past its source by one byte
        {0, 2, ~0ull - 10},                     // offset + bytes wraps
        {r - 1, 3, want.runs[4 * r - 1] - 1},   // the file one byte short
        {r - 1, 0, 1},                          // t >= n_targets
    };
    for (const edit& e : edits) {
        u64s rn = want.runs;
        rn[4 * e.j + e.col] = e.val;
        out = start;
        CHECK(apply(rn, out) == SD_ERR_INVALID && out == start);
    }
    {
        const u64s oo2 = {3, 3}, ol2 = {0, b.lens[2]};  // the same runs for target 1 of two, then one that goes back to 0
        u64s rn = want.runs;
        for (uint64_t j = 0; j < r; j++) rn[4 * j] = 1;
        out = start;
        CHECK(sd_cpu_cdc_delta_apply(rn.data(), r, b.offs.data(), b.lens.data(), 2, b.buf.data(), want.lit.data(), want.lit.size(),
                                     oo2.data(), ol2.data(), 2, out.data(), 2) == SD_OK);
        CHECK(slice(out, 3, 3 + ol[0]) == want.targets[0]);
        rn[4 * (r - 1)] = 0;  // descending
        out = start;
        CHECK(sd_cpu_cdc_delta_apply(rn.data(), r, b.offs.data(), b.lens.data(), 2, b.buf.data(), want.lit.data(), want.lit.size(),
                                     oo2.data(), ol2.data(), 2, out.data(), 2) == SD_ERR_INVALID);
        CHECK(out == start);
    }
    CHECK(sd_cpu_cdc_delta_apply(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 1) == SD_OK);
    CHECK(sd_cpu_cdc_delta_apply(nullptr, 2, nullptr, nullptr, 0, nullptr, nullptr, 0, oo.data(), ol.data(), 1, out.data(), 1) ==
          SD_ERR_INVALID);
}

int main() {
    test_against_the_model();
    test_capacity_and_refusals();
    if (g_fail) {
        printf("cdc_delta_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("cdc_delta_selftest: ok\n");
    return 0;
}
