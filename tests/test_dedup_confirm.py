"""The confirm step without a device (include/sd_cas.h: sd_cpu_dedup_confirm): the host sibling,
the numpy mirror dedup.confirm_host and the wrapper cpu.confirm against the dict model of
tests/dedup_confirm_cases.py on every case; the stats identities; the capacity rule and
count-only calls; the refusals; the ABI, binding and Rust declarations; the grid constants the
cases are derived from; end to end from planted file bytes through sd_cpu_fingerprints, and
through library.confirm_duplicates over real files; and the stand-alone selftest's plain build.
tests/test_gpu_dedup_confirm.py runs the same cases through the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import cas_spec as cs
from spacedrive_amd import _native, cpu, dedup, library
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib
from tests import dedup_confirm_cases as dc
from tests import sliced_cases as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacedrive_amd", "csrc")
U = np.uint64


def assert_equals_model(got, want, what):
    rep, size, verdict, sets, stats = got
    assert np.array_equal(np.asarray(rep, U), want["rep"]), what
    assert np.array_equal(np.asarray(size, U), want["size"]), what
    assert np.array_equal(verdict, want["verdict"]), what
    assert np.array_equal(np.asarray(sets, U).reshape(-1, 3), want["sets"]), what
    assert np.array_equal(np.asarray(stats, U), want["stats"]), what


def test_host_sibling_mirror_and_wrapper_equal_the_model():
    names = []
    for name, keys, hashes, valid, want, _ in dc.all_cases():
        assert_equals_model(cpu.confirm(keys, hashes, valid), want, name)
        assert_equals_model(dedup.confirm_host(keys, hashes, valid), want, name)
        dc.check_identities(want["stats"])
        assert int(want["stats"][4]) == len(want["sets"])
        names.append(name)
    assert len(names) == len(set(names)) == 2 * len(dc.SIZES) + 19


def test_random_mix_is_a_prefix_path_case():
    """Under the fixed seed no two valid files of the mix share key and first 8 checksum bytes with
    unequal tails, and its stats are the plant's; the tie cases tie, the uniform one does not."""
    keys, hashes, valid, n_dup, n_twin = dc.mix_plant()
    assert not dc.has_tie(keys, hashes, valid)
    by_name = {c[0]: c for c in dc.all_cases()}
    st = by_name["random_mix"][4]["stats"]
    assert abs(len(keys) - 100_000) <= 10_000 and 0 < int(st[0]) < len(keys)
    assert 0 < int(st[6]) <= 2 * n_twin and 0 < int(st[5]) - int(st[4]) <= n_dup and int(st[7]) > 0
    ties = {n for n, *_, tie in dc.all_cases() if tie}
    assert ties == {"tie_aba", "tie_byte8", "tie_byte31", "tie_among_others", "order_tail_0001_0100", "order_tail_7f_80"}


def parse_grid_constants(path: str, names) -> dict:
    src = open(path).read()
    out = {}
    for name in names:
        found = re.findall(r"^constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", src, re.M)
        assert len(found) == 1, name
        out[name] = int(found[0])
    return out


def test_grid_constants_match_the_kernels():
    """The cases' slice arithmetic (tests/sliced_cases.py, for the confirm step and the Object index
    alike) uses sliced.h's constants: a retune of the kernels fails here instead of moving a border
    out from under the sweeps.  Neither user of the header keeps constants of its own, and the
    index's count slots are the header's workgroups."""
    got = parse_grid_constants(os.path.join(CSRC, "sliced.h"), ("BLOCKS", "TILE"))
    assert got == {"BLOCKS": sl.BLOCKS, "TILE": sl.TILE} and (dc.BLOCKS, dc.TILE) == (sl.BLOCKS, sl.TILE)
    assert dc.slice_len is sl.slice_len
    assert dc.PAST_GRID == dc.BLOCKS * dc.TILE + 1 and dc.slice_len(dc.PAST_GRID) == 2 * dc.TILE
    assert dc.slice_len(1) == dc.slice_len(dc.BLOCKS * dc.TILE) == dc.TILE
    assert sl.SLICE_COUNTS == (1, 255, 256, 257, 262144, 262145)
    assert [sl.slice_len(n) for n in sl.SLICE_COUNTS] == [256] * 5 + [512]
    for name in ("dedup_confirm.hip", "object_index.hip"):
        assert not re.search(r"constexpr[^;=]*\b(\w+_)?(BLOCKS|TILE)\s*=", open(os.path.join(CSRC, name)).read()), name
    slots = parse_grid_constants(os.path.join(CSRC, "sd_internal.h"), ("OI_COUNT_SLOTS",))
    assert slots == {"OI_COUNT_SLOTS": got["BLOCKS"]}
    src = open(os.path.join(CSRC, "dedup_confirm.hip")).read()
    assert "__launch_bounds__(256)" in src and dc.TILE == 256  # a tile is a workgroup's lanes


def raw_call(keys, hashes, valid, rep, size, verdict, sets, capacity, want_n=True, want_stats=True):
    n = ctypes.c_uint64(12345)
    stats = np.full(8, 777, U)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib().sd_cpu_dedup_confirm(p(keys), p(hashes), p(valid), len(keys) if keys is not None else 0, p(rep), p(size),
                                    p(verdict), p(sets), capacity, ctypes.byref(n) if want_n else None,
                                    stats.ctypes.data if want_stats else None)
    return rc, int(n.value), stats


def test_capacity_rule_and_count_only():
    name, keys, hashes, valid, want, _ = next(c for c in dc.all_cases() if c[0] == "size_513_valid")
    m, n_sets = len(keys), len(want["sets"])
    assert n_sets >= 3
    hashes = np.ascontiguousarray(hashes)
    FILL = U(0xA5A5A5A5A5A5A5A5)
    for cap in (n_sets - 1, 0):  # one short, and none: refused, the per-file outputs complete
        rep, size, verdict = np.full(m, FILL, U), np.full(m, FILL, U), np.full(m, 0xA5, np.uint8)
        sets = np.full((n_sets + 4, 3), FILL, U)
        rc, n, stats = raw_call(keys, hashes, valid, rep, size, verdict, sets, cap)
        assert rc == SD_ERR_CAPACITY and n == n_sets and (sets == FILL).all()
        assert_equals_model((rep, size, verdict, want["sets"], stats), want, cap)
    # exactly enough: nothing past the rows
    sets = np.full((n_sets + 4, 3), FILL, U)
    rc, n, stats = raw_call(keys, hashes, valid, None, None, None, sets, n_sets)
    assert rc == 0 and n == n_sets and np.array_equal(sets[:n_sets], want["sets"]) and (sets[n_sets:] == FILL).all()
    # count only, with every combination of the optional host outputs
    for want_n in (True, False):
        for want_stats in (True, False):
            rc, n, stats = raw_call(keys, hashes, valid, None, None, None, None, 0, want_n, want_stats)
            assert rc == 0 and n == (n_sets if want_n else 12345)
            assert np.array_equal(stats, want["stats"]) if want_stats else (stats == 777).all()
    with pytest.raises(SdCasError) as e:
        cpu.confirm(keys, hashes, valid, capacity=n_sets - 1)
    assert e.value.rc == SD_ERR_CAPACITY and e.value.needed == n_sets
    assert len(cpu.confirm(keys, hashes, valid, want_sets=False)[3]) == 0


def test_invalid_arguments_and_empty_call():
    k, h = np.zeros(4, U), np.zeros((4, 32), np.uint8)
    for keys, hashes in ((None, h), (k, None)):
        n = ctypes.c_uint64(0)
        rc = lib().sd_cpu_dedup_confirm(None if keys is None else keys.ctypes.data,
                                        None if hashes is None else hashes.ctypes.data, None, 4, None, None, None,
                                        None, 0, ctypes.byref(n), None)
        assert rc == -1 and b"null" in lib().sd_cas_last_error()
    # m == 0: valid with every pointer NULL; counts 0, nothing written
    rc, n, stats = raw_call(None, None, None, None, None, None, None, 0)
    assert rc == 0 and n == 0 and not stats.any()
    # the device entries refuse a missing context before any HIP call
    assert lib().sd_dedup_confirm(None, None, None, None, 0, None, None, None, None, 0, None, None, None) == -1
    assert lib().sd_dedup_confirm_stats(None, None) == -1
    with pytest.raises(ValueError):
        cpu.confirm(k, h[:3])


def test_tuning_key_leaves_the_learned_routes_alone():
    """"confirm_full_sort" is an ordinary key, default 0 (adaptive); sd_dedup_confirm reads it
    per call.  That it moves no learned-route generation is the selftest's to show."""
    import spacedrive_amd as sd
    assert sd.get_tuning("confirm_full_sort") == 0
    sd.set_tuning("confirm_full_sort", 1)
    assert sd.get_tuning("confirm_full_sort") == 1
    sd.set_tuning("confirm_full_sort", 0)


def test_abi_binding_and_rust_declarations():
    hdr = open(_native.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    order = [code.index(s) for s in ("#define SD_CONFIRM_INVALID", "#define SD_CONFIRM_SINGLE", "#define SD_CONFIRM_CONFIRMED",
                                     "#define SD_CONFIRM_REFUTED", "int sd_dedup_confirm(", "int sd_dedup_confirm_stats(",
                                     "int sd_cpu_dedup_confirm(")]
    assert order == sorted(order)
    assert code.index("int sd_dedup_owners(") < order[0] and order[-1] < code.index("sd_object_index")  # the dedup section
    for name, value in (("INVALID", 0), ("SINGLE", 1), ("CONFIRMED", 2), ("REFUTED", 3)):
        assert re.search(rf"#define SD_CONFIRM_{name}\s+{value}\b", hdr)
        assert getattr(_native, f"SD_CONFIRM_{name}") == value == getattr(dc, name)
    bound = {n: len(a) for n, _, a in _native.SIGNATURES}
    assert (bound["sd_dedup_confirm"], bound["sd_dedup_confirm_stats"], bound["sd_cpu_dedup_confirm"]) == (13, 2, 11)
    rust = open(os.path.join(ROOT, "integration", "rust", "sd-cas-sys", "src", "lib.rs")).read()
    for fn, nargs in (("sd_dedup_confirm", 13), ("sd_dedup_confirm_stats", 2), ("sd_cpu_dedup_confirm", 11)):
        decl = re.search(rf"pub fn {fn}\s*\(([^)]*)\)", rust, flags=re.S)
        assert decl, fn
        args = decl.group(1).strip().rstrip(",")
        assert args.count(",") + 1 == nargs, fn
    for name, value in (("INVALID", 0), ("SINGLE", 1), ("CONFIRMED", 2), ("REFUTED", 3)):
        assert re.search(rf"SD_CONFIRM_{name}\b[^;]*= {value};", rust), name
    step = open(os.path.join(ROOT, "integration", "rust", "core", "confirm_step.rs")).read()
    assert "file_checksums(" in step and "sd_cpu_dedup_confirm(" in step and "SD_CONFIRM_CONFIRMED" in step


# ---------------------------------------------------------------- end to end, no device
@pytest.fixture(scope="module")
def planted():
    files = dc.planted_files()
    contents = [cs.synth_bytes(c, t, 0, L) for L, c, t in files]
    return files, contents


def keys_of(cas_ids):
    return np.array([int(c, 16) for c in cas_ids], U)


def rows_of(checksums):
    return np.array([list(bytes.fromhex(c)) for c in checksums], np.uint8).reshape(-1, 32)


def test_end_to_end_from_bytes(planted):
    """Planted bytes -> sd_cpu_fingerprints -> sd_cpu_dedup_confirm: the verdicts follow from the
    plant alone; every twin is refuted or confirmed only with twins of its own tag."""
    files, contents = planted
    offs, off = [], 0
    for b in contents:
        offs.append(off)
        off = (off + len(b) + 127) // 64 * 64
    buf = np.zeros(off + 64, np.uint8)
    for o, b in zip(offs, contents):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    cas_ids, checksums = cpu.fingerprints(buf, offs, [len(b) for b in contents], nthreads=8)
    rep, size, verdict, sets, stats = cpu.confirm(keys_of(cas_ids), rows_of(checksums))
    want_rep, want_size, want_verdict = dc.planted_expectation(files)
    assert rep.tolist() == want_rep and size.tolist() == want_size and verdict.tolist() == want_verdict
    assert sorted(int(r) for r in sets[:, 1]) == sorted({r for r, v in zip(want_rep, want_verdict) if v == dc.CONFIRMED})
    assert stats.tolist() == [28, 20, 4, 23, 4, 9, 3, 3]
    dc.check_identities(stats)
    # the twins share their original's cas_id: without the checksums they are one group
    for (L, c, t), cid in zip(files, cas_ids):
        if t:
            assert cid == cas_ids[files.index((L, c, 0))]


def test_confirm_duplicates_over_files(planted, tmp_path):
    """library.confirm_duplicates on the same contents as files (no context: the CPU path), one
    path unreadable: it comes back INVALID and out of every count."""
    files, contents = planted
    paths = []
    for i, b in enumerate(contents):
        p = tmp_path / f"f{i:02d}"
        p.write_bytes(b)
        paths.append(str(p))
    cas_ids = [cpu.generate_cas_id(p, len(b)) for p, b in zip(paths, contents)]
    gone = next(i for i, f in enumerate(files) if f == (112_640, 500, 0))  # one of the three copies
    paths[gone] = str(tmp_path / "missing")
    out = library.confirm_duplicates(None, paths, cas_ids, nthreads=4)
    kept = [f if i != gone else ("gone", i, 0) for i, f in enumerate(files)]
    want_rep, want_size, want_verdict = [], [], []
    for i, f in enumerate(kept):
        if i == gone:
            want_rep.append(dc.M64), want_size.append(0), want_verdict.append(dc.INVALID)
            continue
        same = [j for j, g in enumerate(kept) if g == f]
        group = [j for j, g in enumerate(kept) if j != gone and g[:2] == f[:2] and (f[0] > dc.MINIMUM_FILE_SIZE or g == f)]
        want_rep.append(same[0]), want_size.append(len(same))
        want_verdict.append(dc.SINGLE if len(group) == 1 else dc.CONFIRMED if len(same) >= 2 else dc.REFUTED)
    assert out["verdict"].tolist() == want_verdict and out["verdict"][gone] == dc.INVALID
    assert out["rep"].tolist() == want_rep and out["class_size"].tolist() == want_size
    assert isinstance(out["checksums"][gone], OSError) and int(out["stats"][0]) == len(files) - 1
    for cid, members in out["sets"]:
        assert len(members) >= 2 and all(cas_ids[i] == cid and out["verdict"][i] == dc.CONFIRMED for i in members)
        assert members == sorted(members) and gone not in members
    assert sorted(i for _, mem in out["sets"] for i in mem) == [i for i, v in enumerate(want_verdict) if v == dc.CONFIRMED]
    assert [c for c, _ in out["sets"]] == sorted(c for c, _ in out["sets"])


def test_dedup_confirm_selftest():
    b = subprocess.run(["make", "-C", CSRC, "-j8", "dedup-confirm-selftest"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    r = subprocess.run([os.path.join(ROOT, "build", "csrc", "plain", "dedup_confirm_selftest")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "dedup_confirm_selftest: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
