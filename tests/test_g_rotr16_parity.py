"""The two forms of rotr(d ^ a, 16) in G (spacedrive_amd/csrc/blake3_device.h) give the same
hashes -- run on an MI355X: -m gpu.

The instantiation with the priority windows writes it as v_xor_b32 + v_alignbit_b32, the one
without as two crosswise SDWA xors; a launch of more waves than the MI355X has SIMDs (1024)
takes the first (cas_kernels.hip, g_windows).  Full 32-byte hashes against the C oracle at the
two shapes where the windowed instantiation first runs and the two just below them:

  k_cas_sampled_lanes   9400 sampled files (258 workgroups, 1032 waves: windows) and 9300
                        (255 workgroups, 1018 waves of lanes: none), "sampled_wave_max" 0
  k_whole_items         1400 whole-kind files of 102400 B (70 000 full pairs: windows) and
                        513 files of the mixed sizes (none)

and the one place where the two forms meet on the same messages: 37 sampled files hashed
alone (no windows) and as the first 37 of the 9400 (windows) must agree bit for bit.
"""
import numpy as np
import pytest

from tests.test_g_prio_parity import WHOLE_SIZES, ctx, full_hashes, mismatches  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu


def sampled_sizes(n):
    return np.full(n, 200001, np.uint64) + np.arange(n, dtype=np.uint64) * np.uint64(4099)


@pytest.fixture(scope="module")
def lanes_only():
    """every sampled batch of this module through k_cas_sampled_lanes + _merge"""
    from spacedrive_amd._native import lib
    assert lib().sd_cas_set_tuning(b"sampled_wave_max", 0) == 0
    yield
    lib().sd_cas_set_tuning(b"sampled_wave_max", 6144)  # the default


@pytest.fixture(scope="module")
def sampled_9400(ctx, oracle_native, lanes_only):
    sizes = sampled_sizes(9400)
    got, want, batch = full_hashes(ctx, oracle_native, sizes)
    assert batch.n_sampled == 9400
    got.setflags(write=False)
    want.setflags(write=False)
    return got, want, sizes


def test_sampled_windows(sampled_9400):
    got, want, sizes = sampled_9400
    assert not mismatches(got, want, sizes)


def test_sampled_just_below(ctx, oracle_native, lanes_only):
    sizes = sampled_sizes(9300)
    got, want, batch = full_hashes(ctx, oracle_native, sizes)
    assert batch.n_sampled == 9300
    assert not mismatches(got, want, sizes)


def test_same_files_both_forms(ctx, oracle_native, lanes_only, sampled_9400):
    big, _, _ = sampled_9400
    sizes = sampled_sizes(37)  # the first 37 files of the 9400: same sizes, same content ids
    got, want, batch = full_hashes(ctx, oracle_native, sizes)
    assert batch.n_sampled == 37
    assert not mismatches(got, want, sizes)
    assert np.array_equal(got, big[:37])


@pytest.mark.parametrize("n", [1400, 513])
def test_whole(ctx, oracle_native, n):
    if n == 513:
        sizes = np.array([WHOLE_SIZES[i % len(WHOLE_SIZES)] for i in range(n)], np.uint64)
    else:
        sizes = np.full(n, 102400, np.uint64)
    got, want, batch = full_hashes(ctx, oracle_native, sizes)
    assert batch.n_sampled == 0
    assert not mismatches(got, want, sizes)
