// fingerprint_selftest.cpp -- the GPU-free half of the fingerprint entry points under test
// (fingerprint_host.cpp: plan_gather, cas_message_from_bytes, sd_cpu_fingerprints), on the
// case lists of tests/fingerprint_cases.py.  A program of its own: built plain for the CPU
// suite (`make fingerprint-selftest`, tests/test_fingerprint.py) and under ASan + UBSan and
// TSan (`make sanitize-fingerprint`, logs in profiles/fingerprint/).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
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

static std::vector<uint64_t> case_lens() {
    std::vector<uint64_t> v = {0, 1, 7, 8, 9, 15, 16, 17, 55, 56, 57, 63, 64, 65, 1015, 1016, 1017, 2040, 2041, 102399, 102400};
    for (uint64_t L = 102401; L <= 102464; L++) v.push_back(L);
    const uint64_t MiB = 1 << 20;
    for (uint64_t L : {(uint64_t)131072, MiB - 1, MiB, MiB + 1, 3 * MiB + 5}) v.push_back(L);
    return v;
}

// the placement of tests/fingerprint_cases.py: gaps of 0..47 bytes, every residue mod 128
static std::vector<uint64_t> place(const std::vector<uint64_t>& lens, uint64_t* total) {
    const int steps[7] = {0, 1, 2, 0, 2, 1, 0};
    std::vector<uint64_t> offs;
    uint64_t pos = 0;
    for (size_t i = 0; i < lens.size(); i++) {
        const uint64_t start = (pos + 15) / 16 * 16 + 16 * steps[i % 7];
        offs.push_back(start);
        pos = start + lens[i];
    }
    *total = (pos + 63) / 64 * 64 + 64;
    return offs;
}

// byte m of the message of a file of `len` bytes, by the source map alone (cas.rs:25-58)
static uint8_t msg_byte(const uint8_t* file, uint64_t len, uint64_t m) {
    if (m < 8) return (uint8_t)(len >> (8 * m));
    uint64_t p = m - 8;
    if (len <= 102400) return file[p];
    if (p < 8192) return file[p];
    p -= 8192;
    const uint64_t jump = (len - 16384) / 4;
    if (p < 4 * 10240) return file[8192 + (p / 10240) * jump + p % 10240];
    return file[len - 8192 + (p - 4 * 10240)];
}

static std::string hex_of(const uint8_t* h, int n) {
    std::string s(2 * n + 1, 0);
    hex_lower(h, n, &s[0]);
    s.resize(2 * n);
    return s;
}

int main() {
    const std::vector<uint64_t> lens = case_lens();
    const size_t n = lens.size();
    CHECK(n == 90);
    uint64_t total = 0;
    const std::vector<uint64_t> offs = place(lens, &total);
    std::vector<uint8_t> data(total, 0xA5);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < n; i++)
        for (uint64_t b = 0; b < lens[i]; b++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            data[offs[i] + b] = (uint8_t)(x >> 56);
        }

    // ---- the planner: sd_cas_stage_plan's layout, the flat unit space, the tile table
    GatherPlan gp;
    plan_gather(gp, offs.data(), lens.data(), n);
    std::vector<sd_extent> ext(n);
    uint64_t staged_total = 0;
    for (size_t i = 0; i < n; i++) {  // sd_cas_stage_plan's rule: one message after the other on 128-B lines
        ext[i] = plan_extent(lens[i], staged_total);
        CHECK(ext[i].msg_len == (lens[i] <= 102400 ? 8 + lens[i] : 57352));
        staged_total = sd_align_up(staged_total + ext[i].msg_len, SD_STAGE_ALIGN);
    }
    CHECK(gp.staged_bytes == staged_total && gp.units * 16 == staged_total);
    CHECK(gp.rows.size() == n + 1 && gp.rows[n].unit0 == gp.units);
    CHECK(gp.n_whole == 21 && gp.n_sampled == 69);
    uint64_t fb = 0, rb = 0;
    for (size_t i = 0; i < n; i++) {
        CHECK(memcmp(&gp.extents[i], &ext[i], sizeof(sd_extent)) == 0);
        CHECK(gp.rows[i].data_off == offs[i] && gp.rows[i].msg_off == ext[i].msg_offset && gp.rows[i].len == lens[i]);
        CHECK(gp.rows[i].unit0 * 16 == ext[i].msg_offset);
        fb += lens[i];
        rb += ext[i].msg_len - 8;
    }
    CHECK(gp.file_bytes == fb && gp.read_bytes == rb);
    const uint64_t tiles = (gp.units + SD_GATHER_TILE_UNITS - 1) / SD_GATHER_TILE_UNITS;
    CHECK(gp.tile_first.size() == tiles + 1 && gp.tile_first[tiles] == n - 1);
    for (uint64_t t = 0; t < tiles; t++) {  // tile t's first unit lies in file tile_first[t]
        const uint32_t f = gp.tile_first[t];
        CHECK(f < n && gp.rows[f].unit0 <= t * SD_GATHER_TILE_UNITS && t * SD_GATHER_TILE_UNITS < gp.rows[f + 1].unit0);
        CHECK(gp.tile_first[t] <= gp.tile_first[t + 1]);
    }
    {  // an empty batch, and a misaligned start
        GatherPlan e;
        plan_gather(e, nullptr, nullptr, 0);
        CHECK(e.units == 0 && e.staged_bytes == 0 && e.tile_first.size() == 1 && e.rows.size() == 1);
        const uint64_t bad_off = 8, one = 1;
        bool threw = false;
        try {
            plan_gather(e, &bad_off, &one, 1);
        } catch (const sd_failure& f) {
            threw = f.rc == SD_ERR_INVALID;
        }
        CHECK(threw);
    }

    // ---- the message builder against the source map, byte by byte
    std::vector<std::string> want17(n), want65(n);
    std::vector<uint8_t> msg(8 + 102400 + 64, 0xEE);
    for (size_t i = 0; i < n; i++) {
        const uint8_t* f = data.data() + offs[i];
        memset(msg.data(), 0xEE, msg.size());
        const uint32_t ml = cas_message_from_bytes(f, lens[i], msg.data());
        CHECK(ml == ext[i].msg_len);
        bool same = true;
        for (uint32_t m = 0; m < ml; m++) same = same && msg[m] == msg_byte(f, lens[i], m);
        CHECK(same);
        CHECK(msg[ml] == 0xEE);  // nothing past the message
        uint8_t h[32];
        cpu_blake3(msg.data(), ml, h);
        want17[i] = hex_of(h, 8);
        cpu_blake3(f, lens[i], h);
        want65[i] = hex_of(h, 32);
    }
    {  // content bytes(i % 251)
        const struct {
            uint64_t len;
            const char* id;
        } anchors[] = {{0, "71e0a99173564931"}, {1016, "c0de16cef5f85601"}, {1017, "62fe3d833d2df619"},
                       {102400, "c66a52267c7e5ee9"}, {102401, "17f74805066119da"}};
        std::vector<uint8_t> pat(102401 + 64);
        for (size_t i = 0; i < pat.size(); i++) pat[i] = (uint8_t)(i % 251);
        for (const auto& a : anchors) {
            const uint64_t o = 0;
            char h17[17], h65[65];
            CHECK(sd_cpu_fingerprints(pat.data(), &o, &a.len, 1, h17, h65, 1) == SD_OK);
            CHECK(strcmp(h17, a.id) == 0);
        }
    }

    // ---- sd_cpu_fingerprints: every thread count gives the expected strings; concurrent calls
    for (int threads : {1, 3, 16}) {
        std::vector<char> h17(17 * n), h65(65 * n);
        CHECK(sd_cpu_fingerprints(data.data(), offs.data(), lens.data(), n, h17.data(), h65.data(), threads) == SD_OK);
        for (size_t i = 0; i < n; i++) {
            CHECK(want17[i] == h17.data() + 17 * i);
            CHECK(want65[i] == h65.data() + 65 * i);
        }
    }
    {
        std::vector<std::thread> callers;
        std::vector<int> ok(4, 0);
        for (int c = 0; c < 4; c++)
            callers.emplace_back([&, c] {
                std::vector<char> h17(17 * n), h65(65 * n);
                bool good = sd_cpu_fingerprints(data.data(), offs.data(), lens.data(), n, h17.data(), h65.data(), 2) == SD_OK;
                for (size_t i = 0; good && i < n; i++) good = want17[i] == h17.data() + 17 * i && want65[i] == h65.data() + 65 * i;
                ok[c] = good;
            });
        for (auto& t : callers) t.join();
        for (int c = 0; c < 4; c++) CHECK(ok[c]);
    }
    CHECK(sd_cpu_fingerprints(nullptr, nullptr, nullptr, 0, nullptr, nullptr, 4) == SD_OK);
    {
        const uint64_t bad_off = 24, one = 1;
        char h17[17], h65[65];
        CHECK(sd_cpu_fingerprints(data.data(), &bad_off, &one, 1, h17, h65, 1) == SD_ERR_INVALID);
        CHECK(sd_cpu_fingerprints(nullptr, &bad_off, &one, 1, h17, h65, 1) == SD_ERR_INVALID);
    }
    if (g_fail) {
        printf("fingerprint_selftest: %d FAILED\n", g_fail);
        return 1;
    }
    printf("fingerprint_selftest: ok (%zu files, %llu staged bytes, %llu tiles)\n", n,
           (unsigned long long)gp.staged_bytes, (unsigned long long)tiles);
    return 0;
}
