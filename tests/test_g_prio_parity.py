"""Every kernel that inlines `compress` (spacedrive_amd/csrc/blake3_device.h), at the smallest
shapes that reach each of them: full 32-byte hashes against the C oracle -- run on an MI355X:
-m gpu.  The G function's issue order and its `SD_G_PRIO` priority windows must never change
a hash, whichever build option the library was made with.

  k_cas_sampled_wave                       1 and 37 sampled files (the default threshold)
  k_cas_sampled_lanes + _merge             the same with "sampled_wave_max" 0 (37 x 7 = 259
                                           lanes: a second, partial workgroup), and 6145
                                           files, just past the default threshold
  k_whole_wave                             3 whole-kind files
  k_whole_items + k_whole_merge8 (A, B)    513 whole-kind files, just past "whole_wave_max":
                                           messages of one chunk, the chunk and pair
                                           boundaries under the 8-byte prefix, three chunks
                                           (the full-pair path) and 8 + 102400 bytes (both
                                           merge passes)
  k_ck_leaf + k_ck_reduce                  one checksum of 2 MiB + 1 B: two full blocks and a
                                           partial one

A launch of more waves than the MI355X has SIMDs (1024) takes the kernel's instantiation with
the windows, a smaller one the instantiation without (cas_kernels.hip, g_windows), and the
shapes above are all of the second kind.  So each kernel that has both also runs at the
smallest shape that takes the first: 1100 sampled files (k_cas_sampled_wave, a wave per file),
9400 (k_cas_sampled_lanes: 1029 waves), 1400 whole-kind files of 102400 B (k_whole_items: 70 000
full pairs) and a checksum of 258 MiB + 1 B (k_ck_leaf: 130 workgroups of 8 waves).  The merge
kernels run one lane per file or per group of nodes and reach 1024 waves only past 65 536 lanes:
65 600 sampled files (k_cas_sampled_merge: 257 workgroups of 4 waves; 3.8 GB of messages) and
9400 whole-kind files of 102400 B (51 pair nodes each, 7 groups of <= 8: k_whole_merge8's first
pass on 65 800 lanes; its second pass, one lane per file, would need 65 537 such files and runs
with the windows only in tests/test_gpu_parity.py's 1 M-file batch).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NT = 16
WHOLE_SIZES = (1, 1016, 1017, 2040, 2041, 3064, 102400)


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return spacedrive_amd.default_context(0)


def full_hashes(ctx, oracle_native, sizes):
    """(device hashes, oracle hashes) of the staged messages of synthetic files of `sizes`"""
    from spacedrive_amd.device import stage_plan
    n = len(sizes)
    cids = np.arange(n, dtype=np.uint64) + 4242
    ext, total = stage_plan(sizes)
    d_staged = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    d_ext = torch.from_numpy(ext.view(np.uint8).copy()).cuda()
    ctx.synth_stage_cas(torch.from_numpy(sizes.view(np.int64)).cuda(), torch.from_numpy(cids.view(np.int64)).cuda(),
                        torch.zeros(n, dtype=torch.int32, device="cuda"), d_ext, n, d_staged)
    batch = ctx.cas_batch(ext)
    out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    batch.run(d_staged, out)
    torch.cuda.synchronize()
    want = oracle_native.checksums(d_staged.cpu().numpy(), ext["msg_offset"], ext["msg_len"].astype(np.uint64),
                                   nthreads=NT)
    return out.cpu().numpy().reshape(n, 32), want, batch


def mismatches(got, want, sizes):
    return [int(sizes[i]) for i in np.nonzero((got != want).any(axis=1))[0][:10]]


@pytest.mark.parametrize("n,wave_max", [(1, 6144), (37, 6144), (1, 0), (37, 0), (6145, 6144), (1100, 6144), (9400, 6144),
                                         (65600, 6144)])
def test_sampled(ctx, oracle_native, n, wave_max):
    from spacedrive_amd._native import lib
    assert lib().sd_cas_set_tuning(b"sampled_wave_max", wave_max) == 0
    try:
        sizes = np.full(n, 200001, np.uint64) + np.arange(n, dtype=np.uint64) * np.uint64(4099)
        got, want, batch = full_hashes(ctx, oracle_native, sizes)
        assert batch.n_sampled == n
        assert not mismatches(got, want, sizes)
    finally:
        lib().sd_cas_set_tuning(b"sampled_wave_max", 6144)  # the default


@pytest.mark.parametrize("n", [3, 513, 1400, 9400])
def test_whole(ctx, oracle_native, n):
    import spacedrive_amd as sd
    assert sd.get_tuning("whole_wave_max") == 512  # 3 files: k_whole_wave; more than 512: the work lists
    if n == 3:
        sizes = np.array(WHOLE_SIZES[-3:], np.uint64)
    elif n == 513:
        sizes = np.array([WHOLE_SIZES[i % len(WHOLE_SIZES)] for i in range(n)], np.uint64)
    else:
        sizes = np.full(n, 102400, np.uint64)
    got, want, batch = full_hashes(ctx, oracle_native, sizes)
    assert batch.n_sampled == 0
    assert not mismatches(got, want, sizes)


@pytest.mark.parametrize("mib", [2, 258])
def test_checksum(ctx, oracle_native, mib):
    L = (mib << 20) + 1
    data = torch.zeros(L + 128, dtype=torch.uint8, device="cuda")
    ctx.synth_fill(777, 0, L, data)
    out = torch.zeros(32, dtype=torch.uint8, device="cuda")
    ctx.checksum_batch([0], [L]).run(data, out)
    torch.cuda.synchronize()
    want = oracle_native.checksums_synth(np.array([L], np.uint64), np.array([777], np.uint64), nthreads=NT)
    assert out.cpu().numpy().tobytes() == want[0].tobytes()
