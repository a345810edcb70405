"""Shared blocks without a device (include/sd_cas.h: sd_cpu_checksum_tree_shared): the host sibling
and the wrapper cpu.checksum_tree_shared against the restatement of tests/tree_shared_cases.py on
every case and at every min_blocks; the identities; the capacity rule and count-only calls with
every combination of NULL outputs; the refusals; the ABI, binding and Rust declarations; end to end
from real bytes through cpu.checksum_tree, and through tree.compare_files over real files; and the
stand-alone selftest's plain build.  tests/test_gpu_tree_shared.py runs the same cases through the
kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from spacedrive_amd import _native, cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import sliced_cases as sl
from tests import tree_shared_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)


def assert_equals_model(got, want, what):
    rep, size, files, pairs, stats = got
    assert np.array_equal(np.asarray(rep, U), want["rep"]), what
    assert np.array_equal(np.asarray(size, U), want["size"]), what
    assert np.array_equal(np.asarray(files, U).reshape(-1, 4), want["files"]), what
    assert np.array_equal(np.asarray(pairs, U).reshape(-1, 4), want["pairs"]), what
    assert np.array_equal(np.asarray(stats, U), want["stats"]), what


def test_host_sibling_equals_the_restatement():
    names = []
    for name, lens, k, nodes, want, _ in tc.all_cases():
        got = cpu.checksum_tree_shared(lens, nodes, k)
        assert_equals_model(got, want, name)
        tc.check_identities(want)
        tc.check_identities(dict(zip(("rep", "size", "files", "pairs", "stats"), got)))
        names.append(name)
    assert len(names) == len(set(names)) == 27
    assert {k for _, _, k, _, _, _ in tc.all_cases()} == {17, 20}


def test_the_cases_hold_what_they_are_for():
    by = {c[0]: c for c in tc.all_cases()}
    assert {n for n, *_, tie in tc.all_cases() if tie} == {"tie_aba", "tie_among_others"}
    assert (sl.TILE, sl.BLOCKS) == (256, 1024)
    for m in (255, 256, 257):
        assert len(by[f"slots_{m}"][4]["rep"]) == m
    assert len(by["past_grid"][4]["rep"]) == 1024 * 256 + 1 == tc.PAST_GRID
    st = by["past_grid"][4]["stats"]
    assert int(st[6]) >= 400 and int(st[4]) > 50_000  # a quarter of the files are near copies
    assert not by["no_files"][4]["stats"].any() and by["one_file"][4]["stats"].tolist()[2:] == [6, 0, 0, 0, 0, 0]
    # the last lane of a tile, its edge and the next workgroup hold redundant slots, not only singles
    for m in (255, 256, 257):
        assert int(by[f"slots_{m}"][4]["stats"][4]) > 10


@pytest.mark.parametrize("min_blocks", tc.MIN_BLOCKS)
def test_min_blocks(min_blocks):
    for name in ("min_blocks", "run_of_700", "tail_other_holder", "slots_257"):
        _, lens, k, nodes, want0, _ = next(c for c in tc.all_cases() if c[0] == name)
        want = tc.shared_model(lens, k, nodes, min_blocks)
        got = cpu.checksum_tree_shared(lens, nodes, k, min_blocks)
        assert_equals_model(got, want, (name, min_blocks))
        tc.check_identities(want, min_blocks)
        assert np.array_equal(want["stats"], want0["stats"]) and np.array_equal(want["files"], want0["files"])
        keep = want0["pairs"][:, 2] >= max(1, min_blocks)
        assert np.array_equal(want["pairs"], want0["pairs"][keep])


def raw_call(lens, k, nodes, rep, size, files, pairs, capacity, min_blocks=0, want_n=True, want_stats=True):
    n = ctypes.c_uint64(12345)
    stats = np.full(8, 777, U)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib().sd_cpu_checksum_tree_shared(p(lens), 0 if lens is None else len(lens), k, p(nodes), min_blocks, p(rep),
                                           p(size), p(files), p(pairs), capacity, ctypes.byref(n) if want_n else None,
                                           stats.ctypes.data if want_stats else None)
    return rc, int(n.value), stats


def test_capacity_rule_and_null_outputs():
    name, lens, k, nodes, want, _ = next(c for c in tc.all_cases() if c[0] == "slots_257")
    nodes = np.ascontiguousarray(nodes)
    n, m, rows = len(lens), len(want["rep"]), len(want["pairs"])
    assert rows >= 3
    for cap in (rows - 1, 0):  # one short, and none: refused, every other output complete
        rep, size, files = np.full(m, FILL, U), np.full(m, FILL, U), np.full((n, 4), FILL, U)
        pairs = np.full((rows + 4, 4), FILL, U)
        rc, got_n, stats = raw_call(lens, k, nodes, rep, size, files, pairs, cap)
        assert rc == SD_ERR_CAPACITY and got_n == rows and (pairs == FILL).all()
        assert_equals_model((rep, size, files, want["pairs"], stats), want, cap)
    pairs = np.full((rows + 4, 4), FILL, U)  # exactly enough: nothing past the rows
    rc, got_n, stats = raw_call(lens, k, nodes, None, None, None, pairs, rows)
    assert rc == 0 and got_n == rows and np.array_equal(pairs[:rows], want["pairs"]) and (pairs[rows:] == FILL).all()
    for mask in range(16):  # every combination of the four array outputs
        rep, size = (np.full(m, FILL, U) if mask & b else None for b in (1, 2))
        files = np.full((n, 4), FILL, U) if mask & 4 else None
        pairs = np.full((rows, 4), FILL, U) if mask & 8 else None
        rc, got_n, stats = raw_call(lens, k, nodes, rep, size, files, pairs, rows)
        assert rc == 0 and got_n == rows and np.array_equal(stats, want["stats"]), mask
        for got, key in ((rep, "rep"), (size, "size"), (files, "files"), (pairs, "pairs")):
            assert got is None or np.array_equal(got, want[key]), (mask, key)
    for want_n in (True, False):
        for want_stats in (True, False):
            rc, got_n, stats = raw_call(lens, k, nodes, None, None, None, None, 0, 0, want_n, want_stats)
            assert rc == 0 and got_n == (rows if want_n else 12345)
            assert np.array_equal(stats, want["stats"]) if want_stats else (stats == 777).all()
    with pytest.raises(SdCasError) as e:
        cpu.checksum_tree_shared(lens, nodes, k, capacity=rows - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == rows
    assert len(cpu.checksum_tree_shared(lens, nodes, k, want_pairs=False)[3]) == 0


def test_invalid_arguments_and_empty_call():
    lens, nodes = np.array([5, 300_000], U), np.zeros((4, 32), np.uint8)
    for k in (16, 21, 0):
        assert raw_call(lens, k, nodes, None, None, None, None, 0)[0] == -1
        assert raw_call(None, k, None, None, None, None, None, 0)[0] == -1  # even with no file
    assert raw_call(lens, 17, None, None, None, None, None, 0)[0] == -1 and b"null" in lib().sd_cas_last_error()
    n = ctypes.c_uint64(0)
    assert lib().sd_cpu_checksum_tree_shared(None, 2, 17, nodes.ctypes.data, 0, None, None, None, None, 0,
                                             ctypes.byref(n), None) == -1
    assert lib().sd_cpu_checksum_tree_shared(None, 1 << 32, 17, nodes.ctypes.data, 0, None, None, None, None, 0,
                                             ctypes.byref(n), None) == -1
    rc, got_n, stats = raw_call(None, 17, None, None, None, None, None, 0)  # n == 0: every pointer NULL
    assert rc == 0 and got_n == 0 and not stats.any()
    # the device entry refuses a missing context before any HIP call
    assert lib().sd_checksum_tree_shared(None, None, 0, 17, None, 0, None, None, None, None, 0, None, None, None) == -1
    with pytest.raises(ValueError):
        cpu.checksum_tree_shared(lens, nodes[:3], 17)
    with pytest.raises(ValueError):
        tree.shared_blocks([(300_000, nodes[:2])], 17)


def test_abi_binding_and_rust_declarations():
    hdr = open(_native.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    order = [code.index(s) for s in ("int sd_cpu_checksum_tree_blocks_verify_range_proofs(", "int sd_checksum_tree_shared(",
                                     "int sd_cpu_checksum_tree_shared(", "int sd_synth_stage_cas(")]
    assert order == sorted(order)  # a section of its own after the range proofs
    for word in ("Shared blocks", "content-defined", "star", "77 bytes per slot", "not collective"):
        assert word in hdr, word
    bound = {n: len(a) for n, _, a in _native.SIGNATURES}
    assert (bound["sd_checksum_tree_shared"], bound["sd_cpu_checksum_tree_shared"]) == (14, 12)
    rust = open(os.path.join(ROOT, "integration", "rust", "sd-cas-sys", "src", "lib.rs")).read()
    for fn, nargs in (("sd_checksum_tree_shared", 14), ("sd_cpu_checksum_tree_shared", 12)):
        decl = re.search(rf"pub fn {fn}\s*\(([^)]*)\)", rust, flags=re.S)
        assert decl, fn
        assert decl.group(1).strip().rstrip(",").count(",") + 1 == nargs, fn
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tree_shared.hip" in mk and "tree_shared_host.cpp" in mk and "resource-usage-shared:" in mk
    assert "sanitize-tree-shared" in mk.split("\nsanitize:")[-1]


# ---------------------------------------------------------------- end to end, no device
@pytest.fixture(scope="module")
def planted():
    return tc.scenario()


def test_end_to_end_from_real_bytes(planted):
    """An exact copy is wholly redundant, a copy with two blocks rewritten has nb - 2 redundant
    blocks, a copy truncated at a block boundary to three blocks is wholly redundant, one truncated
    to a single block shares nothing (its node is a root), an appended copy shares all the
    original's full blocks."""
    contents, want_files, want_pairs = planted
    buf, offs, lens = tc.scenario_buffer(contents)
    nodes, roots, base = cpu.checksum_tree(buf, offs, lens, 17)
    rep, size, files, pairs, stats = cpu.checksum_tree_shared(lens, nodes, 17)
    assert files.tolist() == want_files and pairs.tolist() == want_pairs
    assert stats.tolist() == [6, 34, 13, 7, 21, sum(r[3] for r in want_files), 4, 2]
    assert np.array_equal(rep[:7], np.arange(7, dtype=U))  # the original holds everything first
    assert rep[int(base[5]):int(base[5]) + 6].tolist() == list(range(6)) and size[0] == 5 and size[2] == 4
    assert len(set(bytes(r) for r in roots)) == 5  # the checksums say "refuted" and no more
    model = tc.shared_model(lens, 17, nodes)
    assert_equals_model((rep, size, files, pairs, stats), model, "scenario")
    # through the file-level interface
    f2, p2, s2 = tree.shared_blocks([(L, nodes[int(base[i]):int(base[i + 1])]) for i, L in enumerate(lens)], 17)
    assert np.array_equal(f2, files) and np.array_equal(p2, pairs) and np.array_equal(s2, stats)
    assert tree.shared_blocks([], 17)[2].tolist() == [0] * 8
    assert tree.shared_blocks([(L, nodes[int(base[i]):int(base[i + 1])]) for i, L in enumerate(lens)], 17, 6)[1].tolist() \
        == [r for r in want_pairs if r[2] >= 6]


def test_compare_files(planted, tmp_path):
    contents, want_files, want_pairs = planted
    paths = []
    for i, c in enumerate(contents):
        p = tmp_path / f"f{i}"
        p.write_bytes(c.tobytes())
        paths.append(p)
    sums, files, pairs, stats = tree.compare_files(paths, 17)
    assert files.tolist() == want_files and pairs.tolist() == want_pairs and int(stats[7]) == 2
    assert sums == [cpu.file_checksum(p) for p in paths] and sums[0] == sums[1] != sums[2]


def test_tree_shared_selftest():
    b = subprocess.run(["make", "-C", CSRC, "-j8", "tree-shared-selftest"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "tree_shared_selftest")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "tree_shared_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
