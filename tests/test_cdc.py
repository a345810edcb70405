"""The content-defined chunks without a device (include/sd_cas.h, content-defined chunks): the gear
table, sd_cpu_cdc_cut / _hash / _shared and their wrappers on every case of tests/cdc_cases.py
against the numpy restatement of the rule and the oracle's BLAKE3; the capacity rules, every
combination of NULL outputs, the refusals; the file-level interface; the selftest's plain build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from spacedrive_amd import _native, cdc, cpu, tree
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import cdc_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def cases():
    return cc.all_cases()


@pytest.fixture(scope="module")
def many():
    return cc.all_cases(True)


def assert_cpu_case(case):
    name, buf, offs, lens, params, want = case
    base, chunks, stats = cpu.cdc_cut(buf, offs, lens, params)
    assert np.array_equal(base, want["base"]) and np.array_equal(chunks, want["chunks"]), name
    assert np.array_equal(stats, want["stats"]), (name, stats, want["stats"])
    st = [int(x) for x in stats]
    assert st[3] == st[4] + st[5] + st[6] and st[6] == len(lens), name
    assert np.array_equal(cpu.cdc_hash(buf, offs, lens, base, chunks), want["ids"]), name


def test_gear_table():
    g = cpu.cdc_gear()
    assert np.array_equal(g, cc.GEAR) and int(g[0]) == 0x2df3228afbc5cb53 and int(g[255]) == 0xdd9fba0f5362ab8e
    assert cc.all_zero_has_no_candidate()
    assert lib().sd_cdc_gear(None) == -1


def test_rolling_restatement_is_the_recurrence():
    """the doubling form of cdc_cases.rolling against h(i) = (h(i-1) << 1) + G[byte i], byte by byte"""
    data = cc.synth(3, 700)
    h, want = 0, []
    for b in data:
        h = ((h << 1) + int(cc.GEAR[b])) & ((1 << 64) - 1)
        want.append(h)
    assert cc.rolling(cc.GEAR[data]).tolist() == want


def test_every_case_matches_the_restatement(cases):
    assert len({c[0] for c in cases}) == len(cases) >= 30
    assert {c[4] for c in cases} >= set(cc.PARAM_SETS)
    for case in cases:
        assert_cpu_case(case)


def test_many_chunks_and_many_files(many):
    by = {c[0]: c for c in many}
    assert len(by["many_chunks"][5]["chunks"]) >= 1024 * 256 + 1 and len(by["many_files"][3]) >= 70_000
    assert int(by["many_files"][3].max()) <= 200 and int(by["many_files"][3].min()) >= 1
    for case in many:
        assert_cpu_case(case)


def test_file_start_is_clipped(cases):
    """the bytes of a stand-alone file 16 bytes after another range's start: the same cuts and ids"""
    by = {c[0]: c for c in cases}
    (_, buf, offs, lens, pr, _), (_, buf1, offs1, lens1, _, _) = by["starts_pair"], by["starts_alone"]
    base, chunks, _ = cpu.cdc_cut(buf, offs, lens, pr)
    base1, chunks1, _ = cpu.cdc_cut(buf1, offs1, lens1, pr)
    k = int(base[1])
    assert np.array_equal(chunks[k:], chunks1)
    assert np.array_equal(cpu.cdc_hash(buf, offs, lens, base, chunks)[k:], cpu.cdc_hash(buf1, offs1, lens1, base1, chunks1))


def test_thread_counts_agree(cases):
    name, buf, offs, lens, params, want = next(c for c in cases if c[0] == "tile_lens")
    for nt in (1, 3, 64):
        base, chunks, stats = cpu.cdc_cut(buf, offs, lens, params, nthreads=nt)
        assert np.array_equal(chunks, want["chunks"]) and np.array_equal(stats, want["stats"])
        assert np.array_equal(cpu.cdc_hash(buf, offs, lens, base, chunks, nt), want["ids"])


# ---------------------------------------------------------------- the shared report
@pytest.fixture(scope="module")
def shift(cases):
    name, buf, offs, lens, params, want = next(c for c in cases if c[0] == "shift")
    return buf, offs, lens, params, want


def as_dict(out):
    return dict(zip(("rep", "size", "files", "pairs", "stats"), out))


def test_shift_is_found(shift):
    """5 bytes in front of, or in the middle of, 1 MiB: every chunk of the copy but at most 3 is found
    in the original; the aligned blocks of the same files share nothing; A twice repeats itself."""
    buf, offs, lens, params, want = shift
    base, chunks, ids = want["base"], want["chunks"], want["ids"]
    got = as_dict(cpu.cdc_shared(base, chunks, ids))
    model = cc.shared_model(base, chunks, ids)
    for k in got:
        assert np.array_equal(got[k], model[k]), k
    cc.check_identities(got)
    files, pairs = got["files"], {(int(f), int(g)): int(c) for f, g, c, _ in got["pairs"]}
    for f in (1, 2):
        assert int(files[f, 0]) - pairs[(f, 0)] <= 3 and pairs[(f, 0)] == int(files[f, 2])
    assert pairs[(3, 0)] >= int(files[3, 0]) - 3 and int(got["stats"][7]) == 0  # A twice after A: A holds it first
    nodes, _, _ = cpu.checksum_tree(buf, offs[:2], lens[:2], 17)
    assert int(cpu.checksum_tree_shared(lens[:2], nodes, 17)[4][4]) == 0  # aligned blocks: nothing


def test_a_file_that_repeats_itself(cases):
    """A twice, then A: the second half of file 0 is redundant with its representative in file 0 itself
    -- counted in the file's row and in stats[4], [5] and [7], with no pair row; file 1 is all file 0's."""
    want = next(c for c in cases if c[0] == "twice")[5]
    got = as_dict(cpu.cdc_shared(want["base"], want["chunks"], want["ids"]))
    model = cc.shared_model(want["base"], want["chunks"], want["ids"])
    for k in got:
        assert np.array_equal(got[k], model[k]), k
    cc.check_identities(got)
    st, files = got["stats"], got["files"]
    assert int(st[7]) > 0 and int(st[7]) == int(files[0, 2]) and int(files[0, 2]) >= int(files[0, 0]) // 2 - 3
    assert got["pairs"].tolist() == [[1, 0, int(files[1, 0]), 1 << 18]]
    assert int(got["pairs"][:, 2].sum()) == int(st[4]) - int(st[7])


@pytest.mark.parametrize("min_chunks", [0, 1, 2, 700])
def test_shared_min_chunks(shift, min_chunks):
    _, _, _, _, want = shift
    got = as_dict(cpu.cdc_shared(want["base"], want["chunks"], want["ids"], min_chunks))
    model = cc.shared_model(want["base"], want["chunks"], want["ids"], min_chunks)
    for k in got:
        assert np.array_equal(got[k], model[k]), k
    cc.check_identities(got, min_chunks)
    assert len(got["pairs"]) >= 2 and (got["pairs"][:, 2] >= max(1, min_chunks)).all()


def raw_shared(base, chunks, ids, rep, size, files, pairs, cap, want_n=True, want_stats=True):
    n = len(base) - 1
    n_pairs, stats = ctypes.c_uint64(12345), np.full(8, 777, U)
    rc = lib().sd_cpu_cdc_shared(base.ctypes.data, n, chunks.ctypes.data, ids.ctypes.data, 0,
                                 *(None if a is None else a.ctypes.data for a in (rep, size, files, pairs)), cap,
                                 ctypes.byref(n_pairs) if want_n else None, stats.ctypes.data if want_stats else None)
    return rc, int(n_pairs.value), stats


def test_shared_capacity_and_null_outputs(shift):
    _, _, _, _, want = shift
    base, chunks, ids = want["base"], np.ascontiguousarray(want["chunks"]), np.ascontiguousarray(want["ids"])
    model = cc.shared_model(base, chunks, ids)
    m, n, rows = len(chunks), len(base) - 1, len(model["pairs"])
    assert rows >= 3
    for mask in range(16):
        rep, size = (np.full(m, FILL, U) if mask & b else None for b in (1, 2))
        files = np.full((n, 4), FILL, U) if mask & 4 else None
        pairs = np.full((rows + 2, 4), FILL, U) if mask & 8 else None
        rc, got_n, stats = raw_shared(base, chunks, ids, rep, size, files, pairs, rows)  # exactly enough
        assert rc == 0 and got_n == rows and np.array_equal(stats, model["stats"]), mask
        for got, key in ((rep, "rep"), (size, "size"), (files, "files")):
            assert got is None or np.array_equal(got, model[key]), (mask, key)
        assert pairs is None or (np.array_equal(pairs[:rows], model["pairs"]) and (pairs[rows:] == FILL).all())
    pairs = np.full((rows, 4), FILL, U)
    rc, got_n, stats = raw_shared(base, chunks, ids, None, None, None, pairs, rows - 1)  # one short
    assert rc == SD_ERR_CAPACITY and got_n == rows and (pairs == FILL).all() and np.array_equal(stats, model["stats"])
    for want_n in (True, False):
        for want_stats in (True, False):
            rc, got_n, stats = raw_shared(base, chunks, ids, None, None, None, None, 0, want_n, want_stats)
            assert rc == 0 and got_n == (rows if want_n else 12345)
            assert np.array_equal(stats, model["stats"]) if want_stats else (stats == 777).all()
    with pytest.raises(SdCasError) as e:
        cpu.cdc_shared(base, chunks, ids, capacity=rows - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == rows


# ---------------------------------------------------------------- the cut's capacity rule and NULL outputs
def raw_cut(buf, offs, lens, params, base, chunks, cap, want_n=True, want_stats=True):
    pr = cpu.cdc_params(params)
    n_chunks, stats = ctypes.c_uint64(12345), np.full(8, 777, U)
    rc = lib().sd_cpu_cdc_cut(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, len(lens), ctypes.byref(pr),
                              None if base is None else base.ctypes.data, None if chunks is None else chunks.ctypes.data,
                              cap, ctypes.byref(n_chunks) if want_n else None, stats.ctypes.data if want_stats else None, 4)
    return rc, int(n_chunks.value), stats


def test_cut_capacity_and_null_outputs(cases):
    name, buf, offs, lens, params, want = next(c for c in cases if c[0] == "params_p8")
    m = len(want["chunks"])
    for mask in range(4):
        base = np.full(len(lens) + 1, FILL, U) if mask & 1 else None
        chunks = np.full((m + 2, 2), FILL, U) if mask & 2 else None
        for want_n in (True, False):
            for want_stats in (True, False):
                rc, got_n, stats = raw_cut(buf, offs, lens, params, base, chunks, m, want_n, want_stats)  # exactly enough
                assert rc == 0 and got_n == (m if want_n else 12345), mask
                assert np.array_equal(stats, want["stats"]) if want_stats else (stats == 777).all()
                assert base is None or np.array_equal(base, want["base"])
                assert chunks is None or (np.array_equal(chunks[:m], want["chunks"]) and (chunks[m:] == FILL).all())
    base, chunks = np.full(len(lens) + 1, FILL, U), np.full((m, 2), FILL, U)
    rc, got_n, stats = raw_cut(buf, offs, lens, params, base, chunks, m - 1)  # one short: the requirement, no chunk
    assert rc == SD_ERR_CAPACITY and got_n == m and (chunks == FILL).all()
    assert np.array_equal(base, want["base"]) and np.array_equal(stats, want["stats"])
    with pytest.raises(SdCasError) as e:
        cpu.cdc_cut(buf, offs, lens, params, capacity=m - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == m
    assert len(cpu.cdc_cut(buf, offs, lens, params, want_chunks=False)[1]) == 0


# ---------------------------------------------------------------- refusals
BAD_PARAMS = [(0, 64, 1024), (33, 64, 1024), (8, 63, 1024), (8, 2048, 1024), (8, 64, (1 << 20) + 1)]


def test_invalid_parameters_and_ranges():
    buf = np.zeros(4096, np.uint8)
    offs, lens = np.array([0, 1024], U), np.array([1000, 2000], U)
    good = (8, 64, 1024)
    assert raw_cut(buf, offs, lens, good, None, None, 0)[0] == 0
    for bad in BAD_PARAMS:
        assert raw_cut(buf, offs, lens, bad, None, None, 0)[0] == -1, bad
    for ok in [(1, 64, 64), (32, 64, 1 << 20), (8, 1 << 20, 1 << 20)]:
        assert raw_cut(buf, offs, lens, ok, None, None, 0)[0] == 0, ok
    pr = cpu.CdcParams(8, 64, 1024, 1)  # reserved != 0
    n = ctypes.c_uint64(0)
    args = (buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, 2)
    assert lib().sd_cpu_cdc_cut(*args, ctypes.byref(pr), None, None, 0, ctypes.byref(n), None, 1) == -1
    assert lib().sd_cpu_cdc_cut(*args, None, None, None, 0, ctypes.byref(n), None, 1) == -1 and b"null" in lib().sd_cas_last_error()
    assert raw_cut(buf, np.array([0, 1032], U), lens, good, None, None, 0)[0] == -1  # a start not 16-byte aligned
    pr = cpu.cdc_params(good)
    assert lib().sd_cpu_cdc_cut(None, offs.ctypes.data, lens.ctypes.data, 2, ctypes.byref(pr), None, None, 0, None, None, 1) == -1
    assert lib().sd_cpu_cdc_cut(buf.ctypes.data, None, lens.ctypes.data, 2, ctypes.byref(pr), None, None, 0, None, None, 1) == -1
    # the 2^32 bound: ceil(len / min_size) + n, refused before a byte is read
    huge = np.array([64 * ((1 << 32) - 1)], U)  # ceil(len / 64) + 1 == 2^32
    one = np.array([0], U)
    assert lib().sd_cpu_cdc_cut(buf.ctypes.data, one.ctypes.data, huge.ctypes.data, 1, ctypes.byref(pr), None, None, 0, None,
                                None, 1) == -1 and b"2^32" in lib().sd_cas_last_error()
    rc, got_n, stats = raw_cut(buf, offs[:0], lens[:0], good, None, None, 0)  # n == 0
    assert rc == 0 and got_n == 0 and not stats.any()
    # the device entries refuse a missing context or batch before any HIP call
    h = ctypes.c_void_p()
    assert lib().sd_cdc_create(None, offs.ctypes.data, lens.ctypes.data, 2, ctypes.byref(pr), ctypes.byref(h)) == -1
    assert lib().sd_cdc_cut(None, None, None, None, None) == -1 and lib().sd_cdc_hash(None, None, None, None, None, None) == -1
    assert lib().sd_cdc_layout(None, None) == -1 and lib().sd_cdc_stats(None, None) == -1
    assert lib().sd_cdc_shared(None, None, 0, None, None, 0, None, None, None, None, 0, None, None, None) == -1


def test_invalid_layouts():
    chunks, ids = np.zeros((3, 2), U), np.zeros((3, 32), np.uint8)
    n = ctypes.c_uint64(0)

    def call(base, count):
        b = np.array(base, U)
        return lib().sd_cpu_cdc_shared(b.ctypes.data, count, chunks.ctypes.data, ids.ctypes.data, 0, None, None, None, None, 0,
                                       ctypes.byref(n), None)
    assert call([0, 1, 3], 2) == 0
    assert call([1, 2, 3], 2) == -1 and call([0, 2, 2], 2) == -1 and call([0, 1, 3], 1 << 32) == -1
    assert lib().sd_cpu_cdc_shared(None, 0, None, None, 0, None, None, None, None, 0, ctypes.byref(n), None) == 0 and n.value == 0
    with pytest.raises(ValueError):
        cpu.cdc_shared([0, 1, 3], chunks[:2], ids)
    buf, offs, lens = np.zeros(256, np.uint8), np.array([0], U), np.array([100], U)
    with pytest.raises(SdCasError):  # a chunk outside its file
        cpu.cdc_hash(buf, offs, lens, [0, 1], [[50, 51]])


# ---------------------------------------------------------------- files, bindings, documents
def test_chunk_and_compare_files(tmp_path, shift):
    _, _, _, params, want = shift
    paths = []
    for i, f in enumerate(cc.shift_files()):
        p = tmp_path / f"f{i}"
        p.write_bytes(f.tobytes())
        paths.append(p)
    base, chunks, ids, stats = cdc.chunk_files(paths, params, device=False)
    assert np.array_equal(base, want["base"]) and np.array_equal(chunks, want["chunks"]) and np.array_equal(ids, want["ids"])
    assert ids[0].tobytes().hex() == cpu.blake3(cc.shift_files()[0][:int(chunks[0, 1])].tobytes()).hex()
    files, pairs, sstats = cdc.compare_files(paths, params, device=False)
    model = cc.shared_model(base, chunks, ids)
    assert np.array_equal(files, model["files"]) and np.array_equal(pairs, model["pairs"]) and np.array_equal(sstats, model["stats"])
    assert [int(f) for f, g, _, _ in pairs if g == 0] == [1, 2, 3]
    # what tree.compare_files says of the original and its shifted copy: nothing in common
    assert int(tree.compare_files(paths[:2], 17)[3][4]) == 0
    assert cdc.compare_files([], params, device=False)[2].tolist() == [0] * 8


def test_abi_binding_and_documents():
    hdr = open(_native.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    order = [code.index(s) for s in ("int sd_cpu_checksum_tree_shared(", "int sd_cdc_gear(", "int sd_cdc_create(", "int sd_cdc_shared(",
                                     "int sd_cpu_cdc_shared(", "int sd_synth_stage_cas(")]
    assert order == sorted(order)  # a section of its own after the shared blocks
    assert re.search(r"#define SD_CAS_ABI_VERSION 2\b", hdr)
    for c, v in (("SD_CDC_DEFAULT_MASK_BITS", 16), ("SD_CDC_DEFAULT_MIN_SIZE", 16384), ("SD_CDC_DEFAULT_MAX_SIZE", 262144)):
        assert re.search(rf"#define {c} {v}\b", hdr), c
    assert _native.SD_CDC_DEFAULT == (16, 16384, 262144) and ctypes.sizeof(cpu.CdcParams) == 16
    bound = {n: len(a) for n, _, a in _native.SIGNATURES}
    for fn, nargs in (("sd_cdc_gear", 1), ("sd_cdc_create", 6), ("sd_cdc_cut", 5), ("sd_cdc_hash", 6), ("sd_cdc_shared", 14),
                      ("sd_cpu_cdc_cut", 11), ("sd_cpu_cdc_hash", 8), ("sd_cpu_cdc_shared", 12)):
        assert bound[fn] == nargs, fn
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cdc.hip" in mk and "cdc_host.cpp" in mk and "resource-usage-cdc:" in mk
    assert "sanitize-cdc" in mk.split("\nsanitize:")[-1]
    for doc, words in (("README.md", ("Content-defined chunks",)), ("DESIGN.md", ("3.6", "content-defined", "serial walk")),
                       ("INTEGRATION.md", ("sd_cdc_shared", "content-defined"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_cdc_selftest():
    b = subprocess.run(["make", "-C", CSRC, "-j8", "cdc-selftest"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "cdc_selftest")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "cdc_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
