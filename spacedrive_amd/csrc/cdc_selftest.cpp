// cdc_selftest.cpp -- stand-alone check of the host half of the content-defined chunks
// (include/sd_cas.h, "content-defined chunks"; cdc_host.cpp): sd_cdc_gear, sd_cpu_cdc_cut, _hash and
// _shared against a byte-at-a-time model of the rule -- the rolling value as the explicit sum over
// the last 64 bytes of the file, every window searched from its first position, the ids from the
// selftests' own BLAKE3 (selftest_blake3.h), the shared report from a map of lists -- on the shapes
// of tests/cdc_cases.py: the lengths around 64, min_size and max_size, constant bytes (no candidate,
// or one at every position), ranges a few bytes apart, repeats inside a file and between files.
// Built plain for the CPU test suite (tests/test_cdc.py) and under ASan + UBSan and TSan
// (`make sanitize-cdc`).  No HIP.
#include <stdio.h>
#include <string.h>

#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "sd_host.h"
#include "selftest_blake3.h"

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

// ---------------------------------------------------------------- the model
static uint64_t m_gear(uint32_t b) {
    uint64_t z = (0x5DCDC0DEull ^ b) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// h(i) of a file: the sum over k = 0 .. min(i, 63) of G[byte(i - k)] << k
static bool m_candidate(const uint8_t* p, uint64_t i, uint32_t mask_bits) {
    uint64_t h = 0;
    for (uint64_t k = 0; k <= std::min<uint64_t>(i, 63); k++) h += m_gear(p[i - k]) << k;
    return (h >> (64 - mask_bits)) == 0;
}

struct batch_t {
    bytes buf;
    u64s offs, lens;
    sd_cdc_params pr;
};
struct answer_t {
    u64s base, chunks, stats;
    bytes ids;
    bool operator==(const answer_t& o) const {
        return base == o.base && chunks == o.chunks && stats == o.stats && ids == o.ids;
    }
};

static answer_t model(const batch_t& b) {
    answer_t a;
    a.base.push_back(0);
    a.stats.assign(8, 0);
    a.stats[0] = b.lens.size();
    for (size_t f = 0; f < b.lens.size(); f++) {
        const uint8_t* p = b.buf.data() + b.offs[f];
        const uint64_t len = b.lens[f];
        a.stats[1] += len;
        for (uint64_t i = 0; i < len; i++) a.stats[2] += m_candidate(p, i, b.pr.mask_bits);
        uint64_t s = 0;
        do {
            uint64_t e = 0;
            bool hit = false;
            for (uint64_t c = s + b.pr.min_size; c <= s + b.pr.max_size && c <= len && !hit; c++)
                if (m_candidate(p, c - 1, b.pr.mask_bits)) e = c, hit = true;
            if (!hit) e = std::min<uint64_t>(s + b.pr.max_size, len);
            a.stats[e == len ? 6 : hit ? 4 : 5]++;
            a.chunks.push_back(s), a.chunks.push_back(e - s);
            uint8_t id[32];
            m_put(m_subtree(p + s, e - s, 0, true), id);
            a.ids.insert(a.ids.end(), id, id + 32);
            for (uint64_t at = 0; at < std::max<uint64_t>(e - s, 1); at += 1024)  // blocks of every chunk, and the parents
                a.stats[7] += std::max<uint64_t>(1, (std::min<uint64_t>(1024, e - s - at) + 63) / 64);
            a.stats[7] += std::max<uint64_t>(1, (e - s + 1023) / 1024) - 1;
            s = e;
        } while (s < len);
        a.base.push_back(a.chunks.size() / 2);
    }
    a.stats[3] = a.chunks.size() / 2;
    return a;
}

static answer_t run(const batch_t& b, int nthreads) {
    answer_t a;
    const size_t n = b.lens.size();
    a.base.assign(n + 1, 99), a.stats.assign(8, 99);
    uint64_t m = 0;
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), n, &b.pr, a.base.data(), nullptr, 0, &m, a.stats.data(),
                         nthreads) == SD_OK);
    a.chunks.assign(2 * m, 99);
    uint64_t m2 = 0;
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), n, &b.pr, a.base.data(), a.chunks.data(), m, &m2,
                         a.stats.data(), nthreads) == SD_OK);
    CHECK(m2 == m);
    a.ids.assign(32 * m, 0x99);
    CHECK(sd_cpu_cdc_hash(b.buf.data(), b.offs.data(), b.lens.data(), n, a.base.data(), a.chunks.data(), a.ids.data(),
                          nthreads) == SD_OK);
    return a;
}

// files of these lengths at 16-byte aligned starts `gap16` units after the last one's end, random
// bytes everywhere; content: 0 = random bytes, else that constant byte + 1
static batch_t make(const u64s& lens, sd_cdc_params pr, uint64_t seed, uint32_t content = 0, uint64_t gap16 = 1) {
    batch_t b;
    b.pr = pr;
    uint64_t cur = 16;
    for (uint64_t L : lens) {
        b.offs.push_back(cur);
        b.lens.push_back(L);
        cur = (cur + L + 15) / 16 * 16 + 16 * gap16;
    }
    b.buf.resize(cur + 64);
    for (size_t i = 0; i < b.buf.size(); i++) b.buf[i] = (uint8_t)mix(seed, i);
    if (content)
        for (size_t f = 0; f < lens.size(); f++) memset(b.buf.data() + b.offs[f], (int)content - 1, lens[f]);
    return b;
}

static void test_gear() {
    uint64_t g[256];
    CHECK(sd_cdc_gear(g) == SD_OK);
    for (uint32_t b = 0; b < 256; b++) CHECK(g[b] == m_gear(b));
    CHECK(g[0] == 0x2df3228afbc5cb53ull && g[255] == 0xdd9fba0f5362ab8eull);
    CHECK(sd_cdc_gear(nullptr) == SD_ERR_INVALID);
}

static void test_against_the_model() {
    const sd_cdc_params sets[] = {{4, 64, 128, 0}, {6, 64, 256, 0}, {8, 64, 1024, 0}, {1, 64, 64, 0}, {1, 64, 128, 0},
                                  {7, 100, 300, 0}, {32, 64, 512, 0}};
    uint64_t seed = 1;
    for (const sd_cdc_params& pr : sets) {
        const u64s lens = {0, 1, 63, 64, 65, (uint64_t)pr.min_size - 1, pr.min_size, (uint64_t)pr.min_size + 1,
                           pr.max_size, (uint64_t)pr.max_size + 1, 3u * pr.max_size + 17, 5000};
        for (uint64_t gap : {0, 1, 5}) {
            const batch_t b = make(lens, pr, seed++, 0, gap);
            const answer_t want = model(b);
            CHECK(want.stats[3] == want.stats[4] + want.stats[5] + want.stats[6] && want.stats[6] == lens.size());
            CHECK(run(b, 1) == want);
            CHECK(run(b, 4) == want);
        }
    }
}

static void test_constant_bytes() {
    const sd_cdc_params pr = {4, 64, 1024, 0};
    int dense = -1;
    for (uint32_t b = 0; b < 256 && dense < 0; b++)
        if (((0 - m_gear(b)) >> 60) == 0) dense = (int)b;
    CHECK(dense >= 0);
    CHECK(((0 - m_gear(0)) >> 63) == 1);  // zeros: the steady rolling value has its top bit set
    const batch_t zeros = make({3 * 1024 + 17}, pr, 7, 1), all = make({64 * 5 + 3, 700}, pr, 8, (uint32_t)dense + 1);
    const answer_t wz = model(zeros), wa = model(all);
    CHECK(wz.chunks[1] == 1024 && wz.chunks[3] == 1024 && wz.stats[5] == 3);
    CHECK(wa.chunks[1] == 64 && wa.chunks[3] == 64 && wa.stats[5] == 0);
    CHECK(run(zeros, 2) == wz);
    CHECK(run(all, 2) == wa);
}

static void test_capacity_and_refusals() {
    const sd_cdc_params pr = {6, 64, 256, 0};
    const batch_t b = make({1000, 0, 300}, pr, 21);
    const answer_t want = model(b);
    const uint64_t m = want.stats[3];
    u64s base(4, 7), chunks(2 * m, 7), stats(8, 7);
    uint64_t got = 0;
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), 3, &pr, base.data(), chunks.data(), m - 1, &got,
                         stats.data(), 2) == SD_ERR_CAPACITY);
    CHECK(got == m && base == want.base && stats == want.stats && chunks == u64s(2 * m, 7));
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), 3, &pr, nullptr, nullptr, 0, nullptr, nullptr, 2) == SD_OK);
    const sd_cdc_params bad[] = {{0, 64, 256, 0}, {33, 64, 256, 0}, {6, 63, 256, 0}, {6, 512, 256, 0},
                                 {6, 64, (1u << 20) + 1, 0}, {6, 64, 256, 1}};
    for (const sd_cdc_params& p : bad)
        CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), 3, &p, nullptr, nullptr, 0, &got, nullptr, 1) ==
              SD_ERR_INVALID);
    CHECK(sd_cpu_cdc_cut(b.buf.data(), b.offs.data(), b.lens.data(), 3, nullptr, nullptr, nullptr, 0, &got, nullptr, 1) ==
          SD_ERR_INVALID);
    u64s off8 = b.offs;
    off8[1] += 8;
    CHECK(sd_cpu_cdc_cut(b.buf.data(), off8.data(), b.lens.data(), 3, &pr, nullptr, nullptr, 0, &got, nullptr, 1) == SD_ERR_INVALID);
    const uint64_t zero = 0, huge = 64ull * ((1ull << 32) - 1);  // ceil(len / 64) + 1 == 2^32
    CHECK(sd_cpu_cdc_cut(b.buf.data(), &zero, &huge, 1, &pr, nullptr, nullptr, 0, &got, nullptr, 1) == SD_ERR_INVALID);
    CHECK(sd_cpu_cdc_cut(nullptr, nullptr, nullptr, 0, &pr, base.data(), nullptr, 0, &got, stats.data(), 1) == SD_OK);
    CHECK(got == 0 && base[0] == 0 && stats == u64s(8, 0));
    bytes ids(32 * m);
    u64s out_of_file = want.chunks;
    out_of_file[1] += 1000;
    CHECK(sd_cpu_cdc_hash(b.buf.data(), b.offs.data(), b.lens.data(), 3, want.base.data(), out_of_file.data(), ids.data(), 1) ==
          SD_ERR_INVALID);
}

// ---------------------------------------------------------------- the shared report
struct shared_t {
    u64s rep, size, files, pairs, stats;
    bool operator==(const shared_t& o) const {
        return rep == o.rep && size == o.size && files == o.files && pairs == o.pairs && stats == o.stats;
    }
};

static shared_t shared_model(const answer_t& a, uint64_t min_chunks) {
    const size_t n = a.base.size() - 1, m = a.chunks.size() / 2;
    std::map<std::pair<uint64_t, bytes>, u64s> classes;  // (length, id) -> its slots, ascending
    for (size_t s = 0; s < m; s++) classes[{a.chunks[2 * s + 1], bytes(a.ids.begin() + 32 * s, a.ids.begin() + 32 * s + 32)}].push_back(s);
    shared_t r;
    r.rep.assign(m, 0), r.size.assign(m, 0), r.files.assign(4 * n, 0), r.stats.assign(8, 0);
    r.stats[0] = n, r.stats[1] = m, r.stats[2] = classes.size();
    for (const auto& c : classes) {
        r.stats[3] += c.second.size() >= 2;
        for (uint64_t s : c.second) r.rep[s] = c.second[0], r.size[s] = c.second.size();
    }
    auto file_of = [&](uint64_t s) {
        size_t f = 0;
        while (a.base[f + 1] <= s) f++;
        return (uint64_t)f;
    };
    std::map<std::pair<uint64_t, uint64_t>, std::pair<uint64_t, uint64_t>> rows;
    for (size_t f = 0; f < n; f++) {
        r.files[4 * f] = a.base[f + 1] - a.base[f];
        for (uint64_t s = a.base[f]; s < a.base[f + 1]; s++) {
            r.files[4 * f + 1] += r.size[s] >= 2;
            if (r.rep[s] == s) continue;
            r.files[4 * f + 2]++, r.files[4 * f + 3] += a.chunks[2 * s + 1];
            const uint64_t g = file_of(r.rep[s]);
            if (g == f) r.stats[7]++;
            else rows[{f, g}].first++, rows[{f, g}].second += a.chunks[2 * s + 1];
        }
        r.stats[4] += r.files[4 * f + 2], r.stats[5] += r.files[4 * f + 3], r.stats[6] += r.files[4 * f + 2] != 0;
    }
    for (const auto& row : rows)
        if (row.second.first >= std::max<uint64_t>(1, min_chunks))
            r.pairs.insert(r.pairs.end(), {row.first.first, row.first.second, row.second.first, row.second.second});
    return r;
}

static void test_shared() {
    // X = the first 6000 bytes of file 0: file 0 = X twice (it repeats itself and holds X first), file 1 =
    // 3 bytes + X, file 2 = X, file 3 unrelated, files 4 and 5 empty
    const sd_cdc_params pr = {5, 64, 256, 0};
    batch_t b = make({12000, 6003, 6000, 2000, 0, 0}, pr, 31);
    uint8_t* p = b.buf.data();
    memcpy(p + b.offs[0] + 6000, p + b.offs[0], 6000);
    memcpy(p + b.offs[1] + 3, p + b.offs[0], 6000);
    memcpy(p + b.offs[2], p + b.offs[0], 6000);
    const answer_t a = run(b, 2);
    CHECK(a == model(b));
    const size_t n = 6, m = a.chunks.size() / 2;
    for (uint64_t min_chunks : {0, 1, 2, 40, 1000}) {
        const shared_t want = shared_model(a, min_chunks);
        CHECK(want.stats[7] > 0 && want.stats[4] > want.stats[7]);
        shared_t got;
        got.rep.assign(m, 9), got.size.assign(m, 9), got.files.assign(4 * n, 9), got.pairs.assign(4 * m, 9), got.stats.assign(8, 9);
        uint64_t rows = 0;
        CHECK(sd_cpu_cdc_shared(a.base.data(), n, a.chunks.data(), a.ids.data(), min_chunks, got.rep.data(), got.size.data(),
                                got.files.data(), got.pairs.data(), m, &rows, got.stats.data()) == SD_OK);
        got.pairs.resize(4 * rows);
        CHECK(got == want);
        if (rows) {
            u64s few(4 * rows, 9);
            uint64_t need = 0;
            CHECK(sd_cpu_cdc_shared(a.base.data(), n, a.chunks.data(), a.ids.data(), min_chunks, nullptr, nullptr, nullptr,
                                    few.data(), rows - 1, &need, nullptr) == SD_ERR_CAPACITY);
            CHECK(need == rows && few == u64s(4 * rows, 9));
        }
    }
    const shared_t all = shared_model(a, 0);
    uint64_t in_rows = 0;
    for (size_t r = 0; r < all.pairs.size() / 4; r++) in_rows += all.pairs[4 * r + 2];
    CHECK(in_rows == all.stats[4] - all.stats[7]);
    uint64_t rows = 7;
    CHECK(sd_cpu_cdc_shared(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &rows, nullptr) == SD_OK && rows == 0);
    const uint64_t bad_base[3] = {0, 2, 2};
    CHECK(sd_cpu_cdc_shared(bad_base, 2, a.chunks.data(), a.ids.data(), 0, nullptr, nullptr, nullptr, nullptr, 0, &rows, nullptr) ==
          SD_ERR_INVALID);
}

static void test_concurrent_calls() {  // the calls hold no shared state beyond the thread pools and the gear table
    const sd_cdc_params pr = {6, 64, 256, 0};
    const batch_t b = make({3000, 100, 777, 0, 4096}, pr, 41);
    const answer_t want = model(b);
    std::vector<std::thread> ts;
    std::vector<int> ok(4, 0);
    for (int t = 0; t < 4; t++)
        ts.emplace_back([&, t] {
            int good = 1;
            for (int k = 0; k < 5; k++) good &= run(b, 1 + t % 3) == want;
            ok[t] = good;
        });
    for (auto& t : ts) t.join();
    for (int t = 0; t < 4; t++) CHECK(ok[t] == 1);
}

int main() {
    test_gear();
    test_against_the_model();
    test_constant_bytes();
    test_capacity_and_refusals();
    test_shared();
    test_concurrent_calls();
    if (g_fail) {
        printf("cdc_selftest: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("cdc_selftest: ok\n");
    return 0;
}
