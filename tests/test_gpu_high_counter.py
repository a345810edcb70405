"""Chunk counters past 2^32 and three-pass reduce trees on the device (tests/high_counter_cases.py).

High counters: sd_split_checksum_leaves hashes rank 2049's slice of a file of 2^22 - 1 + n blocks
at its true position, so k_ck_leaf (ck_leaf_body, full_chunk_cv_lp, chunk_cv) runs with chunk
counters from 0xFFFFFC00 through 2^32 and on -- a high counter word of 0 in the slice's first block
and 1 in every later one -- in the unwindowed instantiation (3 blocks) and the windowed one
(2 CUs + 3 blocks).  Every slot is compared with the oracle's CV of the same bytes at the 64-bit
counter, the first two with the pure-Python spec's (tests/golden/high_counter.json), and every
other byte of the 134 MB CV buffer must stay as it was.

Deep trees: sd_split_checksum_root (run_checksum_reduce) and sd_checksum_tree_roots (its own pass
loop, pass 0 reading the caller's nodes) on levels of more than 65 536 CVs -- a third pass, the
second buffer swap, a count-1 group on the second level, and files of different depth in one
batch -- against numpy's parent tree.  No file bytes are needed for either.

tests/test_high_counter.py pins the references against each other and holds the CPU twins to the
same cases."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import native  # noqa: E402
from spacedrive_amd.device import SplitChecksum  # noqa: E402
from tests import high_counter_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

G = 4  # guard rows either side of an output
POISON = 0xA5
LEAD = 128 + 16  # a slice starts 16 bytes past a 128-byte line, 0xA5 before it
ZERO_PAD = 64    # zero past its end, as the kernels require; 0xA5 again after that
TRAIL = 256


@pytest.fixture(scope="module")
def ctx():
    import spacedrive_amd
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = spacedrive_amd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


class Guarded:
    """`rows` rows of `row_bytes` device bytes between G guard rows, all 0xA5; the calls get `inner`"""

    def __init__(self, rows: int, row_bytes: int):
        self.rows, self.row_bytes = rows, row_bytes
        self.raw = torch.full(((rows + 2 * G) * row_bytes,), POISON, dtype=torch.uint8, device="cuda")
        self.inner = self.raw[G * row_bytes:(G + rows) * row_bytes]

    def host(self) -> np.ndarray:
        torch.cuda.synchronize()
        return self.raw.cpu().numpy().reshape(-1, self.row_bytes)[G:G + self.rows]

    def guards_intact(self) -> bool:
        torch.cuda.synchronize()
        edge = G * self.row_bytes
        return bool((self.raw[:edge] == POISON).all().item() and (self.raw[-edge:] == POISON).all().item())


def dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()  # the shared cases are read-only


def host_slice(case: hc.LeafCase) -> np.ndarray:
    """the slice's bytes from the oracle's generator, laid out as the device tensor will be"""
    buf = np.full(LEAD + case.len + ZERO_PAD + TRAIL, POISON, np.uint8)
    native.lib().sdo_synth_fill(hc.CID, 0, case.offset, case.len, ctypes.c_void_p(buf.ctypes.data + LEAD))
    buf[LEAD + case.len:LEAD + case.len + ZERO_PAD] = 0
    return buf


def oracle_cvs(case: hc.LeafCase, buf: np.ndarray) -> np.ndarray:
    s = buf[LEAD:LEAD + case.len]
    return np.frombuffer(b"".join(native.subtree_cv(s[k * hc.MIB:k * hc.MIB + case.block_len(k)], case.chunk0(k))
                                  for k in range(case.n)), np.uint8).reshape(case.n, 32)


def run_leaves(ctx, case: hc.LeafCase, golden) -> None:
    buf = host_slice(case)
    want = oracle_cvs(case, buf)
    assert [w.tobytes().hex() for w in want[:2]] == [b["cv"] for b in golden["high_counter"]["blocks"]]
    d_raw = dev(buf)
    del buf
    assert d_raw.data_ptr() % 128 == 0
    d_slice = d_raw[LEAD:]
    cvs = Guarded(case.slots, 32)
    sc = SplitChecksum(ctx, case.total, hc.R, hc.RANK)
    assert (sc.offset, sc.len, sc.cv_bytes) == (case.offset, case.len, case.cv_bytes) and cvs.inner.numel() == case.cv_bytes
    sc.leaves(d_slice, cvs.inner)
    torch.cuda.synchronize()
    lo, hi = (G + hc.B0) * 32, (G + hc.B0 + case.n) * 32
    got = cvs.raw[lo:hi].cpu().numpy().reshape(case.n, 32)
    bad = [k for k in range(case.n) if not np.array_equal(got[k], want[k])]
    assert not bad, (case.n, len(bad), bad[:8])
    # block 1 on: the control a counter kept in 32 bits would produce is another value
    assert got[1].tobytes().hex() != golden["high_counter"]["blocks"][1]["cv_counter_mod_2_32"]
    # every byte outside slots [B0, B0 + n), the guard rows included, compared on the device
    assert bool((cvs.raw[:lo] == POISON).all().item()) and bool((cvs.raw[hi:] == POISON).all().item())
    sc.close()
    # freed by reference only: torch.cuda.empty_cache() here also drops what earlier modules left cached,
    # and with that test_gpu_parity's test_file_checksums_hybrid_split[files-0] later found its GPU half
    # starting after the CPU half had taken every file (seen twice in the whole suite, not without the flush)
    del cvs, d_raw, d_slice


def test_synth_fill_at_a_4_tib_offset(ctx):
    """first, so that a generator bug cannot be read as a hash bug: the device's synthetic bytes at
    file offset (2^22 - 1) MiB are the oracle's"""
    case = hc.small_case()
    d = torch.full((case.len + 64,), POISON, dtype=torch.uint8, device="cuda")
    ctx.synth_fill(hc.CID, 0, case.len, d, offset=case.offset)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    want = np.frombuffer(native.synth_bytes(hc.CID, 0, case.offset, case.len), np.uint8)
    assert np.array_equal(got[:case.len], want)
    assert (got[(case.len + 7) // 8 * 8:] == POISON).all()  # whole 8-byte words, nothing after the last
    assert not np.array_equal(want[:4096], np.frombuffer(native.synth_bytes(hc.CID, 0, 0, 4096), np.uint8))


def test_split_leaves_past_2_32(ctx, golden):
    """the small slice (unwindowed), the wide one (windowed, its last workgroup half empty), the
    small one again on the same context, and a rank that holds nothing"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    small, wide = hc.small_case(), hc.wide_case(cus)
    assert 8 * ((small.n + 1) // 2) <= 4 * cus < 8 * ((wide.n + 1) // 2)  # k_ck_leaf<false>, k_ck_leaf<true>
    run_leaves(ctx, small, golden)
    run_leaves(ctx, wide, golden)
    run_leaves(ctx, small, golden)
    sc = SplitChecksum(ctx, hc.EMPTY_RANK_TOTAL, 4096, 4095)
    assert sc.len == 0 and sc.cv_bytes == 4096 * 32
    cvs = Guarded(4096, 32)
    sc.leaves(torch.zeros(16, dtype=torch.uint8, device="cuda"), cvs.inner)
    assert (cvs.host() == POISON).all() and cvs.guards_intact()
    sc.close()


def test_split_root_three_passes(ctx):
    """every reduce count, ascending then descending on one context (a large plan's scratch before
    a small one's), each run twice on its handle (the second reads the first's levels)"""
    for count in hc.REDUCE_COUNTS + hc.REDUCE_COUNTS[::-1]:
        cvs, total, want = hc.reduce_case(count)
        sc = SplitChecksum(ctx, total, 1, 0)
        assert sc.cv_bytes == 32 * count
        d_cvs = dev(cvs).reshape(-1)
        for _ in range(2):
            out = Guarded(1, 32)
            sc.root(d_cvs, out.inner)
            assert out.host()[0].tobytes() == want, (count, hc.passes(count))
            assert out.guards_intact()
        assert np.array_equal(d_cvs.cpu().numpy().reshape(-1, 32), cvs)  # the caller's CVs are only read
        sc.close()
        del d_cvs


@pytest.mark.parametrize("k", hc.KS)
def test_tree_roots_mixed_depths(ctx, k):
    """files that finish at passes 0, 1, 2 and 3 interleaved in one batch, then the same files in
    reverse order; a single-node file gets its node back.  Only the plan sees the lengths."""
    for counts in (hc.MIXED_COUNTS, hc.MIXED_COUNTS[::-1]):
        b = hc.MixedBatch(k, counts)
        t = ctx.checksum_tree(b.offsets, b.lens, k)
        assert np.array_equal(t.node_base, b.node_base) and t.total_nodes == b.total and t.n == b.n
        nodes, want = b.nodes(), b.roots()
        d_nodes = dev(nodes).reshape(-1)
        for _ in range(2):  # the second run reads the stale levels of the first
            roots = Guarded(b.n, 32)
            t.roots(d_nodes, roots.inner)
            got = roots.host()
            bad = [(i, counts[i]) for i in range(b.n) if not np.array_equal(got[i], want[i])]
            assert not bad, (k, bad)
            assert roots.guards_intact()
        i = counts.index(1)
        assert got[i].tobytes() == nodes[int(b.node_base[i])].tobytes()
        assert np.array_equal(d_nodes.cpu().numpy().reshape(-1, 32), nodes)
        t.close()
        del d_nodes
