// selftest_blake3.h -- the selftests' own BLAKE3: a byte-at-a-time model of the chunk, parent and
// tree definitions, written from the specification and sharing nothing with cpu_blake3.cpp.  For
// the stand-alone selftests only (checksum_tree_selftest.cpp, cdc_selftest.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <vector>

typedef std::array<uint32_t, 8> cv_t;

// ---------------------------------------------------------------- the model's BLAKE3
static const uint32_t M_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                                 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
static const int M_PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
enum { M_START = 1, M_END = 2, M_PARENT = 4, M_ROOT = 8 };

static inline uint32_t m_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static inline void m_g(uint32_t* s, int a, int b, int c, int d, uint32_t x, uint32_t y) {
    s[a] = s[a] + s[b] + x, s[d] = m_rotr(s[d] ^ s[a], 16);
    s[c] = s[c] + s[d], s[b] = m_rotr(s[b] ^ s[c], 12);
    s[a] = s[a] + s[b] + y, s[d] = m_rotr(s[d] ^ s[a], 8);
    s[c] = s[c] + s[d], s[b] = m_rotr(s[b] ^ s[c], 7);
}
static inline cv_t m_compress(const cv_t& cv, const uint8_t block[64], uint64_t counter, uint32_t len, uint32_t flags) {
    uint32_t m[16], s[16];
    for (int i = 0; i < 16; i++)
        m[i] = (uint32_t)block[4 * i] | (uint32_t)block[4 * i + 1] << 8 | (uint32_t)block[4 * i + 2] << 16 |
               (uint32_t)block[4 * i + 3] << 24;
    for (int i = 0; i < 8; i++) s[i] = cv[i];
    for (int i = 0; i < 4; i++) s[8 + i] = M_IV[i];
    s[12] = (uint32_t)counter, s[13] = (uint32_t)(counter >> 32), s[14] = len, s[15] = flags;
    for (int r = 0; r < 7; r++) {
        m_g(s, 0, 4, 8, 12, m[0], m[1]), m_g(s, 1, 5, 9, 13, m[2], m[3]);
        m_g(s, 2, 6, 10, 14, m[4], m[5]), m_g(s, 3, 7, 11, 15, m[6], m[7]);
        m_g(s, 0, 5, 10, 15, m[8], m[9]), m_g(s, 1, 6, 11, 12, m[10], m[11]);
        m_g(s, 2, 7, 8, 13, m[12], m[13]), m_g(s, 3, 4, 9, 14, m[14], m[15]);
        uint32_t p[16];
        for (int i = 0; i < 16; i++) p[i] = m[M_PERM[i]];
        memcpy(m, p, sizeof m);
    }
    cv_t out;
    for (int i = 0; i < 8; i++) out[i] = s[i] ^ s[i + 8];
    return out;
}

// one chunk, a byte at a time: a full block is compressed when the byte after it arrives
static inline cv_t m_chunk(const uint8_t* p, size_t n, uint64_t counter, bool root) {
    cv_t cv;
    memcpy(cv.data(), M_IV, 32);
    uint8_t block[64] = {0};
    uint32_t fill = 0, blocks = 0;
    for (size_t i = 0; i < n; i++) {
        if (fill == 64) {
            cv = m_compress(cv, block, counter, 64, blocks == 0 ? M_START : 0);
            blocks++, fill = 0;
            memset(block, 0, 64);
        }
        block[fill++] = p[i];
    }
    return m_compress(cv, block, counter, fill, (blocks == 0 ? M_START : 0) | M_END | (root ? M_ROOT : 0));
}
static inline cv_t m_parent(const cv_t& l, const cv_t& r, bool root) {
    uint8_t block[64];
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) block[4 * i + b] = (uint8_t)(l[i] >> (8 * b)), block[32 + 4 * i + b] = (uint8_t)(r[i] >> (8 * b));
    cv_t iv;
    memcpy(iv.data(), M_IV, 32);
    return m_compress(iv, block, 0, 64, M_PARENT | (root ? M_ROOT : 0));
}
// level-wise pairwise merge, the odd node carried up, ROOT (if asked) on the last parent
static inline cv_t m_merge(std::vector<cv_t> lvl, bool root) {
    while (lvl.size() > 1) {
        const bool last = lvl.size() == 2;
        std::vector<cv_t> nxt;
        for (size_t i = 0; i + 1 < lvl.size(); i += 2) nxt.push_back(m_parent(lvl[i], lvl[i + 1], root && last));
        if (lvl.size() & 1) nxt.push_back(lvl.back());
        lvl.swap(nxt);
    }
    return lvl[0];
}
// the subtree over chunks of [p, p + n), counters from chunk0; root: the whole message
static inline cv_t m_subtree(const uint8_t* p, size_t n, uint64_t chunk0, bool root) {
    if (n <= 1024) return m_chunk(p, n, chunk0, root);
    std::vector<cv_t> cvs;
    for (size_t at = 0; at < n; at += 1024) cvs.push_back(m_chunk(p + at, std::min<size_t>(1024, n - at), chunk0 + at / 1024, false));
    return m_merge(cvs, root);
}
static inline void m_put(const cv_t& cv, uint8_t* out) {
    for (int i = 0; i < 8; i++)
        for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(cv[i] >> (8 * b));
}
static inline cv_t m_get(const uint8_t* in) {
    cv_t cv;
    for (int i = 0; i < 8; i++)
        cv[i] = (uint32_t)in[4 * i] | (uint32_t)in[4 * i + 1] << 8 | (uint32_t)in[4 * i + 2] << 16 | (uint32_t)in[4 * i + 3] << 24;
    return cv;
}
