"""The CDC deltas without a device (include/sd_cas.h, "Deltas"): sd_cpu_cdc_delta_plan / _pack /
_apply and their wrappers on every case of tests/cdc_delta_cases.py against the numpy restatement
of the rule; the copy through hand-made recipes; the capacity rule, count-only calls and every NULL
output; the refusals, with the output compared whole; the file-level interface; the selftest's
plain build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import spacedrive_amd as sd
from spacedrive_amd import _native, cdc, cpu
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import cdc_cases as cc
from tests import cdc_delta_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)


def assert_plan(case):
    """the twin's plan against the restatement; -> (the restatement's answer, rep)"""
    name, base, nb, chunks, ids = case[:5]
    rep = dc.rep_of(chunks, ids)
    want = dc.plan_model(base, nb, chunks, rep)
    before = [a.copy() for a in (base, chunks, rep)]
    lit_off, runs, files, stats = cpu.cdc_delta_plan(base, nb, chunks, rep)
    for k, got in (("lit_off", lit_off), ("runs", runs), ("files", files), ("stats", stats)):
        assert np.array_equal(got, want[k]), (name, k)
    assert all(np.array_equal(a, b) for a, b in zip(before, (base, chunks, rep))), name
    return want, rep


def assert_round_trip(case):
    name, base, nb, chunks, ids, buf, offs, lens = case
    want, rep = assert_plan(case)
    lit = cpu.cdc_delta_pack(buf, offs, base, nb, chunks, rep, want["lit_off"], int(want["stats"][5]))
    assert np.array_equal(lit, dc.pack_model(buf, offs, base, nb, chunks, rep, want)), name
    out, oo = cpu.cdc_delta_apply(want["runs"], buf, offs[:nb], lens[:nb], lit, lens[nb:])
    for t, f in enumerate(range(nb, len(lens))):
        a, L = int(offs[f]), int(lens[f])
        assert np.array_equal(out[int(oo[t]):int(oo[t]) + L], buf[a:a + L]), (name, t)


# ---------------------------------------------------------------- the plan
def test_plan_on_tables():
    for case in dc.table_cases():
        assert_plan(case)


def test_plan_pack_apply_on_data_cases():
    cases = dc.data_cases()
    assert {c[0] for c in cases} >= {"identical", "insert5", "constant", "repeat_across_targets", "empty_files", "no_base", "all_base"}
    for case in cases:
        assert_round_trip(case)


def test_insert5_sends_at_most_three_chunks():
    """The reason for the feature: 5 bytes inserted at 1000 into 1 MiB at 10 / 256 / 4096.  All chunks
    of the copy but at most 3 are copied from the original; the literal bytes are at most 3 chunks' worth."""
    case = next(c for c in dc.data_cases() if c[0] == "insert5")
    want, _ = assert_plan(case)
    st = [int(x) for x in want["stats"]]
    assert st[0] == 1 and st[1] - st[2] <= 3 and st[5] <= 3 * cc.P10[2] and st[3] + st[5] == (1 << 20) + 5, st


def test_many_target_chunks():
    case = dc.many_table()
    want, _ = assert_plan(case)
    assert int(want["stats"][1]) > 262_144 and int(want["stats"][6]) > 0 and int(want["stats"][2]) > 0


def test_round_trip_on_every_cdc_case():
    """every case of cdc_cases split as base = the first half of its files, targets = the rest"""
    cases = cc.all_cases()
    assert len(cases) >= 30
    for case in cases:
        assert_round_trip(dc.split_of(case))


def raw_plan(base, nb, chunks, rep, lit_off, runs, cap, files, want_n=True, want_stats=True):
    n_runs, stats = ctypes.c_uint64(12345), np.full(8, 777, U)
    rc = lib().sd_cpu_cdc_delta_plan(base.ctypes.data, len(base) - 1, nb, chunks.ctypes.data, rep.ctypes.data,
                                     None if lit_off is None else lit_off.ctypes.data, None if runs is None else runs.ctypes.data,
                                     cap, ctypes.byref(n_runs) if want_n else None, None if files is None else files.ctypes.data,
                                     stats.ctypes.data if want_stats else None)
    return rc, int(n_runs.value), stats


def test_plan_capacity_and_null_outputs():
    name, base, nb, chunks, ids = next(c for c in dc.table_cases() if c[0] == "merge_and_not")
    chunks, rep = np.ascontiguousarray(chunks), dc.rep_of(chunks, ids)
    want = dc.plan_model(base, nb, chunks, rep)
    mt, nt, rows = len(want["lit_off"]), len(want["files"]), len(want["runs"])
    assert rows >= 3
    for mask in range(8):
        lit_off = np.full(mt + 2, FILL, U) if mask & 1 else None
        runs = np.full((rows + 2, 4), FILL, U) if mask & 2 else None
        files = np.full((nt + 1, 6), FILL, U) if mask & 4 else None
        rc, got_n, stats = raw_plan(base, nb, chunks, rep, lit_off, runs, rows, files)  # exactly enough
        assert rc == 0 and got_n == rows and np.array_equal(stats, want["stats"]), mask
        assert lit_off is None or (np.array_equal(lit_off[:mt], want["lit_off"]) and (lit_off[mt:] == FILL).all())
        assert runs is None or (np.array_equal(runs[:rows], want["runs"]) and (runs[rows:] == FILL).all())
        assert files is None or (np.array_equal(files[:nt], want["files"]) and (files[nt:] == FILL).all())
    runs, lit_off, files = np.full((rows, 4), FILL, U), np.full(mt, FILL, U), np.full((nt, 6), FILL, U)
    rc, got_n, stats = raw_plan(base, nb, chunks, rep, lit_off, runs, rows - 1, files)  # one short: no row, all else complete
    assert rc == SD_ERR_CAPACITY and got_n == rows and (runs == FILL).all()
    assert np.array_equal(stats, want["stats"]) and np.array_equal(lit_off, want["lit_off"]) and np.array_equal(files, want["files"])
    for want_n in (True, False):
        for want_stats in (True, False):
            rc, got_n, stats = raw_plan(base, nb, chunks, rep, None, None, 0, None, want_n, want_stats)  # count only
            assert rc == 0 and got_n == (rows if want_n else 12345)
            assert np.array_equal(stats, want["stats"]) if want_stats else (stats == 777).all()
    with pytest.raises(SdCasError) as e:
        cpu.cdc_delta_plan(base, nb, chunks, rep, capacity=rows - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == rows and np.array_equal(e.value.stats, want["stats"])


def test_plan_refusals():
    name, base, nb, chunks, ids = dc.table_cases()[0]
    chunks, rep = np.ascontiguousarray(chunks), dc.rep_of(chunks, ids)
    n = len(base) - 1
    assert raw_plan(base, n + 1, chunks, rep, None, None, 0, None)[0] == -1  # n_base > n
    assert lib().sd_cpu_cdc_delta_plan(base.ctypes.data, n, nb, None, rep.ctypes.data, None, None, 0, None, None, None) == -1
    assert lib().sd_cpu_cdc_delta_plan(base.ctypes.data, n, nb, chunks.ctypes.data, None, None, None, 0, None, None, None) == -1
    assert lib().sd_cpu_cdc_delta_plan(None, n, nb, chunks.ctypes.data, rep.ctypes.data, None, None, 0, None, None, None) == -1
    cnt = ctypes.c_uint64(7)
    assert lib().sd_cpu_cdc_delta_plan(None, 0, 0, None, None, None, None, 0, ctypes.byref(cnt), None, None) == 0 and cnt.value == 0
    t0 = int(base[nb])
    for bad in ([t0, t0 + 1], [t0 + 1, 0]):  # a representative behind its slot; one of another length
        r = rep.copy()
        r[bad[0]] = bad[1]
        assert raw_plan(base, nb, chunks, r, None, None, 0, None)[0] == -1, bad
    # the device entries refuse a missing context before any HIP call
    assert lib().sd_cdc_delta_plan(None, None, 0, 0, None, None, None, None, 0, None, None, None, None) == -1
    assert lib().sd_cdc_delta_pack(None, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert lib().sd_cdc_delta_apply(None, None, 0, None, None, 0, None, None, 0, None, None, 0, None, None) == -1


# ---------------------------------------------------------------- the copy through hand-made recipes
def run_recipe(case):
    name, lit, runs, out_offs, out_lens, size = case
    rng = np.random.default_rng(5)
    out = rng.integers(0, 256, size, dtype=np.uint8)  # random surroundings: they must come back unchanged
    want = dc.apply_model(runs, None, [], [], lit, len(lit), out.copy(), out_offs, out_lens)
    assert want is not dc.INVALID, name
    before = [a.copy() for a in (runs, lit)]
    got, _ = cpu.cdc_delta_apply(runs, np.zeros(0, np.uint8), [], [], lit, out_lens, out, out_offs, nthreads=4)
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
    assert np.array_equal(before[0], runs) and np.array_equal(before[1], lit), name


def test_recipes():
    cases = dc.recipe_cases()
    by = {c[0]: c for c in cases}
    assert len(by["residues"][4]) == 256 and len(by["many_runs"][2]) == 70_000
    assert {int(r[3]) for r in by["lengths"][2]} >= set(dc.COPY_LENS)
    for case in cases:
        run_recipe(case)


def test_one_run_of_64_mib_and_1():
    run_recipe(dc.recipe_cases(big=True)[0])


# ---------------------------------------------------------------- refusals
def test_bad_recipes_write_nothing():
    bad, good = dc.bad_recipes()
    rng = np.random.default_rng(6)
    base = rng.integers(0, 256, 4096 + dc.SLACK, dtype=np.uint8)
    bo, bl = np.array([0, 1024], U), np.array(dc.BAD_BASE_LENS, U)
    lit_all = rng.integers(0, 256, dc.BAD_LIT + 2 * dc.SLACK, dtype=np.uint8)
    lit = lit_all[dc.SLACK:dc.SLACK + dc.BAD_LIT]  # slack on both sides of the literal bytes
    oo, ol = np.array([7, 1001], U), np.array(dc.BAD_OUT_LENS, U)
    start = rng.integers(0, 256, 4096, dtype=np.uint8)

    def call(runs):
        out = start.copy()
        r = np.array(runs, U).reshape(-1, 4)
        rc = lib().sd_cpu_cdc_delta_apply(r.ctypes.data if len(r) else None, len(r), bo.ctypes.data, bl.ctypes.data, 2,
                                          base.ctypes.data, lit.ctypes.data, dc.BAD_LIT, oo.ctypes.data, ol.ctypes.data, 2,
                                          out.ctypes.data, 2)
        return rc, out
    rc, out = call(good)
    want = dc.apply_model(np.array(good, U), base, bo, bl, lit, dc.BAD_LIT, start.copy(), oo, ol)
    assert rc == 0 and np.array_equal(out, want) and not np.array_equal(out, start)
    for name, runs in bad:
        assert not dc.validate(runs, bl, dc.BAD_LIT, ol), name
        rc, out = call(runs)
        assert rc == -1 and np.array_equal(out, start), name
    with pytest.raises(SdCasError):
        cpu.cdc_delta_apply(bad[0][1], base, bo, bl, lit, ol)
    # bad arguments: counts past 2^32, NULL arrays with entries
    r = np.array(good, U)
    args = (bo.ctypes.data, bl.ctypes.data, 2, base.ctypes.data, lit.ctypes.data, dc.BAD_LIT, oo.ctypes.data, ol.ctypes.data, 2)
    out = start.copy()
    assert lib().sd_cpu_cdc_delta_apply(None, 3, *args, out.ctypes.data, 1) == -1
    assert lib().sd_cpu_cdc_delta_apply(r.ctypes.data, 1 << 32, *args, out.ctypes.data, 1) == -1
    assert lib().sd_cpu_cdc_delta_apply(r.ctypes.data, 3, *args, None, 1) == -1
    assert lib().sd_cpu_cdc_delta_apply(r.ctypes.data, 3, None, bl.ctypes.data, 2, *args[3:], out.ctypes.data, 1) == -1
    assert np.array_equal(out, start)
    assert lib().sd_cpu_cdc_delta_apply(None, 0, None, None, 0, None, None, 0, None, None, 0, None, 1) == 0  # nothing to do


# ---------------------------------------------------------------- files, bindings, documents
def write_files(tmp_path, files):
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / f"f{i}"
        p.write_bytes(f.tobytes())
        paths.append(p)
    return paths


def test_delta_and_patch_files(tmp_path):
    A, A5 = dc.insert5_files()
    other = cc.synth(31, 9000)
    paths = write_files(tmp_path, [A, other, A5, np.zeros(0, np.uint8), np.concatenate([other, A[:70000]])])
    d = sd.delta_files(paths[:2], paths[2:], cc.P10, device=False)
    assert d.params == cc.P10 and d.target_lens.tolist() == [(1 << 20) + 5, 0, 79000]
    st = [int(x) for x in d.stats]
    assert st[0] == 3 and st[1] - st[2] - st[6] <= 3 + 1 + 3 and len(d.literals) == st[5] <= 6 * cc.P10[2] and len(d.runs) == st[7]
    for t, p in enumerate(paths[2:]):
        assert d.checksums[t].tobytes().hex() == cpu.file_checksum(p)
    rebuilt = sd.patch_files(paths[:2], d, device=False)
    for got, p in zip(rebuilt, paths[2:]):
        assert got.tobytes() == p.read_bytes()
    # a flipped literal byte: the rebuilt file's checksum differs, and the error names the file
    flipped = cdc.Delta(d.runs, d.literals.copy(), d.target_lens, d.checksums, d.files, d.stats, d.params)
    flipped.literals[0] ^= 1
    with pytest.raises(ValueError, match="target 0"):
        sd.patch_files(paths[:2], flipped, device=False)
    # a recipe for other base files is refused, not applied
    with pytest.raises(SdCasError):
        sd.patch_files(paths[1:2], d, device=False)
    e = sd.delta_files([], [], cc.P10, device=False)
    assert not e.stats.any() and len(e.runs) == 0 and sd.patch_files([], e, device=False) == []


def test_abi_binding_and_documents():
    hdr = open(_native.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    order = [code.index(s) for s in ("int sd_cpu_cdc_shared(", "int sd_cdc_delta_plan(", "int sd_cdc_delta_pack(",
                                     "int sd_cdc_delta_apply(", "int sd_cpu_cdc_delta_plan(", "int sd_cpu_cdc_delta_apply(",
                                     "int sd_synth_stage_cas(")]
    assert order == sorted(order)  # after the CDC section
    assert re.search(r"#define SD_CAS_ABI_VERSION 2\b", hdr)
    bound = {n: len(a) for n, _, a in _native.SIGNATURES}
    for fn, nargs in (("sd_cdc_delta_plan", 13), ("sd_cdc_delta_pack", 11), ("sd_cdc_delta_apply", 14),
                      ("sd_cpu_cdc_delta_plan", 11), ("sd_cpu_cdc_delta_pack", 9), ("sd_cpu_cdc_delta_apply", 13)):
        assert bound[fn] == nargs, fn
        assert len(re.search(rf"int {fn}\((.*?)\);", code, re.S).group(1).split(",")) == nargs, fn
    assert "delta_files" in sd.__all__ and "patch_files" in sd.__all__
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "cdc_delta.hip" in mk and "cdc_delta_host.cpp" in mk and "resource-usage-cdc-delta:" in mk
    assert "sanitize-cdc-delta" in mk.split("\nsanitize:")[-1]
    for doc, words in (("README.md", ("delta_files",)), ("DESIGN.md", ("Deltas", "k_seg_copy", "wire format")),
                       ("INTEGRATION.md", ("Acting on shared chunks", "sd_cdc_delta_apply"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)


def test_cdc_delta_selftest():
    b = subprocess.run(["make", "-C", CSRC, "-j8", "cdc-delta-selftest"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "cdc_delta_selftest")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "cdc_delta_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
