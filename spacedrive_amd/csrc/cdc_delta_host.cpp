// cdc_delta_host.cpp -- the GPU-free half of the CDC deltas (include/sd_cas.h, "Deltas"): the argument
// rules both halves share and the host twins sd_cpu_cdc_delta_plan, _pack and _apply with the device
// calls' semantics.
//
// The plan is one walk over the target slots in slot order: a slot's kind from its representative,
// the literal offsets as a running sum, a run kept open per file while source and offset continue.
// The apply validates the whole recipe before it touches the output (one pass: order, sources,
// ranges without wrap, the files' sums), then copies in tasks of at most 4 MiB on host threads.
// No HIP: built with g++ under the sanitizers too (cdc_delta_selftest.cpp, `make sanitize-cdc-delta`).
#include <string.h>

#include <algorithm>
#include <vector>

#include "sd_host.h"

namespace {
constexpr uint64_t TASK_BYTES = 4ull << 20;  // the most one copy task of the apply moves
constexpr uint64_t NONE = ~0ull;
}  // namespace

uint64_t cdc_delta_check_plan(const uint64_t* chunk_base, size_t n, size_t n_base, const void* chunks, const void* rep,
                              uint64_t* t0) {
    const uint64_t m = cdc_check_layout(chunk_base, n);
    if (n_base > n) throw sd_failure(SD_ERR_INVALID, "n_base is larger than n");
    if (m && (!chunks || !rep)) throw sd_failure(SD_ERR_INVALID, "null argument");
    *t0 = n ? chunk_base[n_base] : 0;
    return m - *t0;
}

void cdc_delta_check_apply(const void* runs, uint64_t n_runs, const uint64_t* base_offsets, const uint64_t* base_lens,
                           size_t n_base, const void* base, const void* lit, uint64_t lit_bytes,
                           const uint64_t* out_offsets, const uint64_t* out_lens, size_t n_targets, const void* out) {
    if (n_runs >= (1ull << 32) || (uint64_t)n_base >= (1ull << 32) || (uint64_t)n_targets >= (1ull << 32))
        throw sd_failure(SD_ERR_INVALID, "too many runs or files");
    if ((n_runs && !runs) || (n_base && (!base_offsets || !base_lens)) || (n_targets && (!out_offsets || !out_lens)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    if (lit_bytes && !lit) throw sd_failure(SD_ERR_INVALID, "null argument");
    bool base_bytes = false, out_bytes = false;
    for (size_t g = 0; g < n_base; g++) base_bytes |= base_lens[g] != 0;
    for (size_t t = 0; t < n_targets; t++) out_bytes |= out_lens[t] != 0;
    if ((base_bytes && !base) || (out_bytes && !out)) throw sd_failure(SD_ERR_INVALID, "null argument");
}

extern "C" int sd_cpu_cdc_delta_plan(const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* chunks,
                                     const uint64_t* rep, uint64_t* lit_off, uint64_t* runs_out, uint64_t capacity,
                                     uint64_t* n_runs, uint64_t* files_out, uint64_t stats[8]) {
    SD_GUARD_BEGIN
    uint64_t t0 = 0;
    const uint64_t mt = cdc_delta_check_plan(chunk_base, n, n_base, chunks, rep, &t0);
    if (n_runs) *n_runs = 0;
    if (stats) memset(stats, 0, 8 * sizeof(uint64_t));
    if (n == 0) return SD_OK;
    uint64_t st[8] = {n - n_base, mt, 0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> lo(mt, NONE), rows, files(6 * (n - n_base), 0);
    std::vector<uint32_t> base_file(t0);  // the file of every base slot
    for (size_t g = 0; g < n_base; g++)
        for (uint64_t s = chunk_base[g]; s < chunk_base[g + 1]; s++) base_file[s] = (uint32_t)g;
    for (size_t f = n_base; f < n; f++) {
        uint64_t* fo = files.data() + 6 * (f - n_base);
        fo[0] = chunk_base[f + 1] - chunk_base[f];
        bool open = false;
        uint64_t next_src = 0, next_off = 0;  // where the open run goes on
        for (uint64_t s = chunk_base[f]; s < chunk_base[f + 1]; s++) {
            const uint64_t len = chunks[2 * s + 1], r = rep[s];
            if (len == 0) {
                st[4]++;
                open = false;
                continue;
            }
            if (r > s || chunks[2 * r + 1] != len || rep[r] != r)
                throw sd_failure(SD_ERR_INVALID, "rep is not a representative table of these chunks");
            uint64_t src = 0, off = 0;
            if (r < t0) {
                src = 1 + base_file[r], off = chunks[2 * r];
                st[2]++, st[3] += len, fo[1]++, fo[2] += len;
            } else if (r == s) {
                off = lo[s - t0] = st[5];
                st[4]++, st[5] += len, fo[3] += len;
            } else {
                off = lo[s - t0] = lo[r - t0];
                st[6]++, fo[4] += len;
            }
            if (open && src == next_src && off == next_off) {
                rows.back() += len;
            } else {
                const uint64_t row[4] = {f - n_base, src, off, len};
                rows.insert(rows.end(), row, row + 4);
                fo[5]++;
            }
            open = true, next_src = src, next_off = off + len;
        }
    }
    st[7] = rows.size() / 4;
    if (lit_off && mt) memcpy(lit_off, lo.data(), mt * sizeof(uint64_t));
    if (files_out && !files.empty()) memcpy(files_out, files.data(), files.size() * sizeof(uint64_t));
    if (n_runs) *n_runs = st[7];
    if (stats) memcpy(stats, st, sizeof st);
    if (runs_out) {
        if (capacity < st[7]) throw sd_failure(SD_ERR_CAPACITY, "capacity is smaller than the number of runs");
        if (!rows.empty()) memcpy(runs_out, rows.data(), rows.size() * sizeof(uint64_t));
    }
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cpu_cdc_delta_pack(const uint64_t* chunk_base, size_t n, size_t n_base, const uint64_t* offsets,
                                     const uint64_t* chunks, const uint64_t* lit_off, const uint64_t* rep,
                                     const uint8_t* data, uint8_t* lit_out) {
    SD_GUARD_BEGIN
    uint64_t t0 = 0;
    const uint64_t mt = cdc_delta_check_plan(chunk_base, n, n_base, chunks, rep, &t0);
    if (mt && (!offsets || !lit_off)) throw sd_failure(SD_ERR_INVALID, "null argument");
    for (size_t f = n_base; f < n; f++)
        for (uint64_t s = chunk_base[f]; s < chunk_base[f + 1]; s++) {
            const uint64_t len = chunks[2 * s + 1];
            if (len == 0 || rep[s] != s) continue;
            if (!data || !lit_out) throw sd_failure(SD_ERR_INVALID, "null argument");
            memcpy(lit_out + lit_off[s - t0], data + offsets[f] + chunks[2 * s], len);
        }
    return SD_OK;
    SD_GUARD_END
}

extern "C" int sd_cpu_cdc_delta_apply(const uint64_t* runs, uint64_t n_runs, const uint64_t* base_offsets,
                                      const uint64_t* base_lens, size_t n_base, const uint8_t* base, const uint8_t* lit,
                                      uint64_t lit_bytes, const uint64_t* out_offsets, const uint64_t* out_lens,
                                      size_t n_targets, uint8_t* out, int nthreads) {
    SD_GUARD_BEGIN
    cdc_delta_check_apply(runs, n_runs, base_offsets, base_lens, n_base, base, lit, lit_bytes, out_offsets, out_lens,
                          n_targets, out);
    struct task { const uint8_t* src; uint8_t* dst; uint64_t bytes; };
    std::vector<task> tasks;
    uint64_t t_prev = 0, at = 0;  // the file of the last run and the bytes its runs hold so far
    auto close_files = [&](uint64_t upto) {  // t_prev is done; the files between it and `upto` have no run
        if (at != out_lens[t_prev]) throw sd_failure(SD_ERR_INVALID, "a file's runs do not sum to its length");
        for (uint64_t t = t_prev + 1; t < upto; t++)
            if (out_lens[t] != 0) throw sd_failure(SD_ERR_INVALID, "a file's runs do not sum to its length");
    };
    for (uint64_t j = 0; j < n_runs; j++) {
        const uint64_t t = runs[4 * j], src = runs[4 * j + 1], off = runs[4 * j + 2], bytes = runs[4 * j + 3];
        if (t >= n_targets || t < t_prev) throw sd_failure(SD_ERR_INVALID, "a run's file is out of range or descends");
        if (src > n_base) throw sd_failure(SD_ERR_INVALID, "a run's source is out of range");
        const uint64_t len = src ? base_lens[src - 1] : lit_bytes;
        if (off > len || bytes > len - off) throw sd_failure(SD_ERR_INVALID, "a run reads past its source");
        if (t != t_prev) close_files(t), t_prev = t, at = 0;
        if (at > out_lens[t] || bytes > out_lens[t] - at) throw sd_failure(SD_ERR_INVALID, "a file's runs do not sum to its length");
        if (bytes) {  // no arithmetic on a buffer that may be NULL
            const uint8_t* s = (src ? base + base_offsets[src - 1] : lit) + off;
            uint8_t* d = out + out_offsets[t] + at;
            for (uint64_t o = 0; o < bytes; o += TASK_BYTES) tasks.push_back({s + o, d + o, std::min(TASK_BYTES, bytes - o)});
        }
        at += bytes;
    }
    if (n_targets) close_files(n_targets);
    cpu_parallel_for(tasks.size(), nthreads, [&](size_t k) { memcpy(tasks[k].dst, tasks[k].src, tasks[k].bytes); });
    return SD_OK;
    SD_GUARD_END
}
