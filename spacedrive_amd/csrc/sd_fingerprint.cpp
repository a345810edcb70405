// sd_fingerprint.cpp -- the fingerprint entry points of the C ABI (include/sd_cas.h): cas_id
// and checksum of files whose bytes are resident, from one copy of them.
//
// Replaces the two reads of one file in the watcher's inner_update_file
//   FileMetadata::new -> generate_cas_id   core/src/location/manager/watcher/utils.rs:393
//   file_checksum on the same path         core/src/location/manager/watcher/utils.rs:438-446
// and the two uploads a caller of sd_cas_ids + sd_checksums pays today.  The gather kernel
// (gather.hip) writes each file's cas message from its bytes in device memory into a staged
// extent; the cas and checksum kernels of cas_kernels.hip then run unchanged.  The planner,
// the host message builder and sd_cpu_fingerprints are GPU-free (fingerprint_host.cpp).
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "sd_api_impl.h"

namespace sdi {

// (Re)plans `b` for these ranges reusing its device buffers (see plan_checksum_batch for the
// stream / host-copy lifetime rule).
void plan_fingerprint_batch(sd_fingerprint_batch* b, const uint64_t* offsets, const uint64_t* lens, size_t n,
                            hipStream_t stream) {
    plan_gather(b->gp, offsets, lens, n);
    b->n = n;
    b->tab.begin();
    b->o_rows = b->tab.add(b->gp.rows);
    b->o_tiles = b->tab.add(b->gp.tile_first);
    b->tab.upload(stream);
    plan_cas_batch(&b->cas, b->gp.extents.data(), n, stream);
    plan_checksum_batch(&b->ck, offsets, lens, n, stream);
    b->scratch.ensure(b->gp.staged_bytes);
}

void run_fingerprint_gather(const sd_fingerprint_batch* b, const uint8_t* d_data, uint8_t* d_staged, hipStream_t s) {
    HIP_CHECK(sdk::launch_cas_gather(d_data, b->d_rows(), b->d_tiles(), b->gp.units, d_staged, s));
}

void run_fingerprint_batch(const sd_fingerprint_batch* b, const uint8_t* d_data, uint8_t* d_cas_hash32,
                           uint8_t* d_checksum32, hipStream_t s) {
    run_fingerprint_gather(b, d_data, b->scratch.as<uint8_t>(), s);
    run_cas_batch(&b->cas, b->scratch.as<uint8_t>(), d_cas_hash32, s);
    run_checksum_batch(&b->ck, d_data, d_checksum32, s);
}

}  // namespace sdi

using namespace sdi;

extern "C" {

int sd_fingerprint_batch_create(sd_cas_ctx* ctx, const uint64_t* offsets, const uint64_t* lens, size_t n,
                                sd_fingerprint_batch** out) {
    SD_GUARD_BEGIN
    if (!ctx || !out || (n && (!offsets || !lens))) throw sd_failure(SD_ERR_INVALID, "null argument");
    *out = nullptr;
    ctx->bind();
    auto b = std::make_unique<sd_fingerprint_batch>();
    plan_fingerprint_batch(b.get(), offsets, lens, n, nullptr);
    *out = b.release();
    return SD_OK;
    SD_GUARD_END
}

void sd_fingerprint_batch_destroy(sd_fingerprint_batch* b) {
    try {
        delete b;
    } catch (...) {
    }
}

int sd_fingerprint_batch_stats(const sd_fingerprint_batch* b, uint64_t out[8]) {
    SD_GUARD_BEGIN
    if (!b || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    out[0] = b->n; out[1] = b->gp.n_sampled; out[2] = b->gp.n_whole; out[3] = b->gp.file_bytes;
    out[4] = b->gp.staged_bytes; out[5] = b->cas.compressions; out[6] = b->ck.plan.compressions;
    out[7] = b->gp.read_bytes;
    return SD_OK;
    SD_GUARD_END
}

int sd_fingerprint_batch_extents(const sd_fingerprint_batch* b, sd_extent* extents_out) {
    SD_GUARD_BEGIN
    if (!b || (b->n && !extents_out)) throw sd_failure(SD_ERR_INVALID, "null argument");
    for (size_t i = 0; i < b->n; i++) extents_out[i] = b->gp.extents[i];
    return SD_OK;
    SD_GUARD_END
}

int sd_fingerprint_batch_gather(sd_cas_ctx* ctx, const sd_fingerprint_batch* b, const uint8_t* d_data,
                                uint8_t* d_staged, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->n && (!d_data || !d_staged))) throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_data) % 16 || reinterpret_cast<uintptr_t>(d_staged) % 16)
        throw sd_failure(SD_ERR_INVALID, "d_data and d_staged must be 16-byte aligned");
    ctx->bind();
    run_fingerprint_gather(b, d_data, d_staged, ctx->pick(stream));
    return SD_OK;
    SD_GUARD_END
}

int sd_fingerprint_batch_run(sd_cas_ctx* ctx, const sd_fingerprint_batch* b, const uint8_t* d_data,
                             uint8_t* d_cas_hash32, uint8_t* d_checksum32, void* stream) {
    SD_GUARD_BEGIN
    if (!ctx || !b || (b->n && (!d_data || !d_cas_hash32 || !d_checksum32)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(d_data) % 16) throw sd_failure(SD_ERR_INVALID, "d_data must be 16-byte aligned");
    ctx->bind();
    run_fingerprint_batch(b, d_data, d_cas_hash32, d_checksum32, ctx->pick(stream));
    return SD_OK;
    SD_GUARD_END
}

// One window at a time: consecutive ranges of at most W bytes are laid out in a slot's device
// window, copied, and fingerprinted as one batch; two slots alternate, the copies on one queue
// of their own, so window k + 1's copies overlap window k's kernels.  Ranges keep their
// host-relative offsets while they ascend without a whole untouched page between them, so such
// a run -- usually the whole window -- is ONE H2D, the few alignment bytes between neighbours
// riding along (as in sd_checksums: no page that holds no range byte is read; the caller's
// buffer may have holes).  A run starts on a 128-B device line; a range after a hole, or one of
// a leaf block or more that would start mid-line, opens a new run.  sd_fingerprints_stats
// counts payload: each range's bytes once, when the range is put into its copy.
// A range longer than W streams through the checksum leaf kernel window by window (one plan of
// known length, as sd_checksums streams its large ranges), and its cas message goes to the
// pinned side list.
int sd_fingerprints(sd_cas_ctx* ctx, const uint8_t* data, const uint64_t* offsets, const uint64_t* lens, size_t n,
                    char* out_hex17, char* out_hex65) {
    SD_GUARD_BEGIN
    if (!ctx || (n && (!data || !offsets || !lens || !out_hex17 || !out_hex65)))
        throw sd_failure(SD_ERR_INVALID, "null argument");
    for (size_t i = 0; i < n; i++)
        if (offsets[i] % 16) throw sd_failure(SD_ERR_INVALID, "range " + std::to_string(i) + " not 16-byte aligned");
    if (n == 0) return SD_OK;
    ctx->bind();
    const uint64_t W = (uint64_t)std::min(16384, std::max(1, tuning_get(SD_TUNE_FINGERPRINT_WINDOW_MB))) << 20;
    constexpr uint64_t SIDE_STRIDE = (SD_SAMPLED_MSG_LEN + SD_STAGE_ALIGN - 1) / SD_STAGE_ALIGN * SD_STAGE_ALIGN;
    size_t n_large = 0;
    for (size_t i = 0; i < n; i++) n_large += lens[i] > W;
    sd_checksum_batch big;  // a large range's one-message plan (outlives the slots' streams)
    PinnedBuf side;         // the large ranges' cas messages, staged by the host
    std::vector<size_t> large;
    if (n_large) side.ensure(n_large * SIDE_STRIDE);
    SlotPair slots(ctx);
    for (int k = 0; k < 2; k++) {
        slots[k].staged.ensure(W + 128);
        slots[k].hashes.ensure(64);
        slots[k].host_hashes.ensure(64);
    }
    struct Pending {
        size_t i0 = 0, i1 = 0;
        bool busy = false;
    } pend[2];
    auto harvest = [&](int k) {
        if (!pend[k].busy) return;
        slots[k].sync();
        const size_t cnt = pend[k].i1 - pend[k].i0;
        const uint8_t* h = slots[k].host_hashes.u8();
        for (size_t i = pend[k].i0; i < pend[k].i1; i++) {
            to_hex(h + 32 * (i - pend[k].i0), 8, out_hex17 + 17 * i);  // cas.rs:61 to_hex()[..16]
            to_hex(h + 32 * cnt + 32 * (i - pend[k].i0), 32, out_hex65 + 65 * i);
        }
        pend[k].busy = false;
    };
    // copied[k] = slot k's window has landed; used[k] = slot k's kernels no longer read it
    hipStream_t cs = slots.copy_stream();
    hipEvent_t copied[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
    bool used_set[2] = {false, false};
    struct Events {
        hipEvent_t* e[2];
        ~Events() {
            for (auto* p : e)
                for (int k = 0; k < 2; k++)
                    if (p[k]) (void)hipEventDestroy(p[k]);
        }
    } ev_guard{{copied, used}};
    for (int k = 0; k < 2; k++) {
        HIP_CHECK(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&used[k], hipEventDisableTiming));
    }
    uint64_t sent = 0;
    auto copy_in = [&](int k, const uint8_t* src, uint64_t bytes, uint64_t dst, bool first, bool last) {
        if (first && used_set[k]) HIP_CHECK(hipStreamWaitEvent(cs, used[k], 0));
        HIP_CHECK(hipMemcpyAsync(slots[k].staged.as<uint8_t>() + dst, src, bytes, hipMemcpyHostToDevice, cs));
        if (!last) return;
        HIP_CHECK(hipEventRecord(copied[k], cs));
        HIP_CHECK(hipStreamWaitEvent(slots[k].stream, copied[k], 0));
    };
    auto done_with = [&](int k) {
        HIP_CHECK(hipEventRecord(used[k], slots[k].stream));
        used_set[k] = true;
    };
    struct Copy {
        uint64_t host_lo, host_end, dev_lo;
    };
    std::vector<Copy> copies;
    std::vector<uint64_t> offs, ls;
    int cur = 0;
    uint64_t gathered = 0;
    for (size_t i = 0; i < n;) {
        if (lens[i] > W) {  // a large range: streamed checksum, cas message staged by the host
            harvest(0);
            harvest(1);
            const uint64_t off0 = 0, L = lens[i];
            plan_checksum_batch(&big, &off0, &L, 1, nullptr);
            const uint64_t nb = big.plan.wg_map.size();
            for (uint64_t pos = 0; pos < L; pos += W) {
                const int k = cur;
                cur ^= 1;
                const uint64_t here = std::min<uint64_t>(W, L - pos);
                copy_in(k, data + offsets[i] + pos, here, 0, true, true);
                sent += here;
                const uint32_t wg0 = (uint32_t)(pos / SD_CK_BLOCK);
                const uint32_t wg1 = (uint32_t)std::min<uint64_t>(nb, wg0 + W / SD_CK_BLOCK);
                HIP_CHECK(sdk::launch_ck_leaf(slots[k].staged.as<uint8_t>(), pos, 0, big.d_files(), big.d_map() + wg0,
                                              wg1 - wg0, big.lvl[0].as<uint32_t>(), slots[k].hashes.as<uint32_t>(),
                                              slots[k].stream));
                done_with(k);
            }
            slots.sync_all();
            Slot& sl = slots[0];
            run_checksum_reduce(&big, sl.hashes.as<uint32_t>(), sl.stream);
            HIP_CHECK(hipMemcpyAsync(sl.host_hashes.p, sl.hashes.p, 32, hipMemcpyDeviceToHost, sl.stream));
            sl.sync();
            to_hex(sl.host_hashes.u8(), 32, out_hex65 + 65 * i);
            cas_message_from_bytes(data + offsets[i], L, side.u8() + large.size() * SIDE_STRIDE);
            large.push_back(i);
            i++;
            continue;
        }
        copies.clear();
        offs.clear();
        ls.clear();
        uint64_t dev_hi = 0;
        size_t j = i;
        while (j < n && lens[j] <= W) {
            const uint64_t o = offsets[j], L = lens[j];
            Copy* c = copies.empty() ? nullptr : &copies.back();
            // the same run: ascending, no whole page between that holds no range byte, and a
            // range of a leaf block or more stays on a 128-B line
            const bool cont = c && L && o >= c->host_end && align_up(c->host_end, 4096) + 4096 > o &&
                              !(L >= SD_CK_BLOCK && (c->dev_lo + (o - c->host_lo)) % SD_STAGE_ALIGN != 0);
            const uint64_t d = cont ? c->dev_lo + (o - c->host_lo) : align_up(dev_hi, SD_STAGE_ALIGN);
            if (j > i && d + L > W) break;
            if (cont) c->host_end = o + L;
            else if (L) copies.push_back(Copy{o, o + L, d});
            offs.push_back(d);
            ls.push_back(L);
            dev_hi = std::max(dev_hi, d + L);
            sent += L;
            j++;
        }
        const size_t cnt = j - i;
        const int k = cur;
        cur ^= 1;
        harvest(k);  // slot k's previous window is done: its plan and buffers are free
        Slot& sl = slots[k];
        plan_fingerprint_batch(&sl.fp, offs.data(), ls.data(), cnt, sl.stream);
        sl.hashes.ensure(64 * cnt);
        sl.host_hashes.ensure(64 * cnt);
        for (size_t q = 0; q < copies.size(); q++)
            copy_in(k, data + copies[q].host_lo, copies[q].host_end - copies[q].host_lo, copies[q].dev_lo, q == 0,
                    q + 1 == copies.size());
        run_fingerprint_batch(&sl.fp, sl.staged.as<uint8_t>(), sl.hashes.as<uint8_t>(),
                              sl.hashes.as<uint8_t>() + 32 * cnt, sl.stream);
        done_with(k);
        HIP_CHECK(hipMemcpyAsync(sl.host_hashes.p, sl.hashes.p, 64 * cnt, hipMemcpyDeviceToHost, sl.stream));
        pend[k] = Pending{i, j, true};
        gathered += cnt;
        i = j;
    }
    harvest(0);
    harvest(1);
    if (!large.empty()) {  // the side list: one ordinary cas batch of sampled messages
        const size_t nl = large.size();
        std::vector<sd_extent> ext(nl);
        for (size_t q = 0; q < nl; q++) ext[q] = plan_extent(lens[large[q]], q * SIDE_STRIDE);
        Slot& sl = slots[0];
        plan_cas_batch(&sl.cas, ext.data(), nl, sl.stream);
        sl.staged.ensure(nl * SIDE_STRIDE);
        sl.hashes.ensure(32 * nl);
        sl.host_hashes.ensure(32 * nl);
        // the messages' zero padding is written on the device; only message bytes cross
        HIP_CHECK(hipMemsetAsync(sl.staged.p, 0, nl * SIDE_STRIDE, sl.stream));
        for (size_t q = 0; q < nl; q++) {
            HIP_CHECK(hipMemcpyAsync(sl.staged.as<uint8_t>() + q * SIDE_STRIDE, side.u8() + q * SIDE_STRIDE,
                                     SD_SAMPLED_MSG_LEN, hipMemcpyHostToDevice, sl.stream));
            sent += SD_SAMPLED_MSG_LEN;
        }
        run_cas_batch(&sl.cas, sl.staged.as<uint8_t>(), sl.hashes.as<uint8_t>(), sl.stream);
        HIP_CHECK(hipMemcpyAsync(sl.host_hashes.p, sl.hashes.p, 32 * nl, hipMemcpyDeviceToHost, sl.stream));
        sl.sync();
        for (size_t q = 0; q < nl; q++) to_hex(sl.host_hashes.u8() + 32 * q, 8, out_hex17 + 17 * large[q]);
    }
    ctx->fp_h2d_bytes.fetch_add(sent, std::memory_order_relaxed);
    ctx->fp_gathered.fetch_add(gathered, std::memory_order_relaxed);
    ctx->fp_large.fetch_add(large.size(), std::memory_order_relaxed);
    return SD_OK;
    SD_GUARD_END
}

int sd_fingerprints_stats(sd_cas_ctx* ctx, uint64_t out[3]) {
    SD_GUARD_BEGIN
    if (!ctx || !out) throw sd_failure(SD_ERR_INVALID, "null argument");
    out[0] = ctx->fp_h2d_bytes.load(std::memory_order_relaxed);
    out[1] = ctx->fp_gathered.load(std::memory_order_relaxed);
    out[2] = ctx->fp_large.load(std::memory_order_relaxed);
    return SD_OK;
    SD_GUARD_END
}

}  // extern "C"
