"""The CDC deltas on the device (include/sd_cas.h, "Deltas"; csrc/cdc_delta.hip) -- run on an MI355X:
-m gpu.  The cases of tests/cdc_delta_cases.py through sd_cdc_delta_plan, _pack and _apply: the plan
against the numpy restatement and the CPU twin, byte for byte, its outputs between 0xA5 guard rows;
the segment copy through hand-made recipes (every residue pair, the lengths around its units and
pieces, segments that meet inside a unit, 70 000 runs, one run of 64 MiB + 1) with the whole output
buffer compared; the refusals with the whole output untouched; the file-level interface."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import spacedrive_amd as sd  # noqa: E402
from spacedrive_amd import cdc, cpu  # noqa: E402
from spacedrive_amd._native import SD_ERR_CAPACITY, SdCasError, lib  # noqa: E402
from tests import cdc_cases as cc  # noqa: E402
from tests import cdc_delta_cases as dc  # noqa: E402
from tests.test_gpu_object_index import Guarded, dev  # noqa: E402

U = np.uint64
FILL = U(0xA5A5A5A5A5A5A5A5)
SPARE = 3


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = sd.default_context(0)
    assert "spacedrive_amd/libsdcas.so" in open("/proc/self/maps").read()
    return c


def u8(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_rep(ctx, base, chunks, ids):
    """sd_cdc_shared's representatives over the table, left on the device: (d_chunks, d_rep)"""
    m = len(chunks)
    d_chunks, d_ids = dev(chunks.reshape(-1)) if m else torch.zeros(2, dtype=torch.int64, device="cuda"), u8(ids if m else np.zeros((1, 32), np.uint8))
    d_rep = torch.zeros(max(m, 1), dtype=torch.int64, device="cuda")
    cdc.shared(ctx, base, d_chunks, d_ids, d_rep=d_rep)
    return d_chunks, d_rep


def plan_guarded(ctx, base, nb, d_chunks, d_rep, mt, nt, rows, capacity, mask=7):
    g_lit, g_runs, g_files = Guarded(mt, 8, torch.int64), Guarded(rows, 32, torch.int64), Guarded(nt, 48, torch.int64)
    rc = 0
    try:
        n_runs, stats = cdc.delta_plan(ctx, base, nb, d_chunks, d_rep, g_lit.inner if mask & 1 else None,
                                       g_runs.inner if mask & 2 else None, capacity, g_files.inner if mask & 4 else None)
    except SdCasError as e:
        rc, n_runs, stats = e.rc, e.needed, e.stats
    for g in (g_lit, g_runs, g_files):
        assert g.guards_intact()
    return {"lit_off": g_lit.host().view(U).reshape(-1), "runs": g_runs.host().view(U).reshape(-1, 4),
            "files": g_files.host().view(U).reshape(-1, 6), "stats": stats}, n_runs, rc, g_lit, g_runs


def assert_plan(ctx, case):
    """-> (the restatement's answer, rep, d_chunks, d_rep, the guarded lit_off and runs)"""
    name, base, nb, chunks, ids = case[:5]
    rep = dc.rep_of(chunks, ids)
    want = dc.plan_model(base, nb, chunks, rep)
    d_chunks, d_rep = device_rep(ctx, base, chunks, ids)
    m = len(chunks)
    assert np.array_equal(d_rep[:m].cpu().numpy().view(U), rep), name
    mt, nt, rows = len(want["lit_off"]), len(want["files"]), len(want["runs"])
    got, n_runs, rc, g_lit, g_runs = plan_guarded(ctx, base, nb, d_chunks, d_rep, mt, nt, rows + SPARE, rows + SPARE)
    assert rc == 0 and n_runs == rows, name
    for k in ("lit_off", "files", "stats"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got["runs"][:rows], want["runs"]) and (got["runs"][rows:] == FILL).all(), name
    c = dict(zip(("lit_off", "runs", "files", "stats"), cpu.cdc_delta_plan(base, nb, chunks, rep)))  # the twin, byte for byte
    for k in c:
        assert np.array_equal(c[k], want[k]), (name, k)
    # the inputs are not written
    assert np.array_equal(d_rep[:m].cpu().numpy().view(U), rep) and (m == 0 or np.array_equal(d_chunks.cpu().numpy().view(U).reshape(-1, 2), chunks))
    return want, rep, d_chunks, d_rep, g_lit, g_runs


def assert_round_trip(ctx, case):
    name, base, nb, chunks, ids, buf, offs, lens = case
    want, rep, d_chunks, d_rep, g_lit, g_runs = assert_plan(ctx, case)
    d_data = u8(buf)
    lit_bytes, rows = int(want["stats"][5]), len(want["runs"])
    g_out = Guarded(1, (lit_bytes + 63) // 64 * 64 + 64)  # the literals, readable to a 64-byte boundary as a source
    cdc.delta_pack(ctx, base, nb, offs, d_chunks, g_lit.inner, d_rep, d_data, g_out.inner)
    torch.cuda.synchronize()
    lit = g_out.host().reshape(-1)
    assert g_out.guards_intact() and (lit[lit_bytes:] == 0xA5).all(), name
    assert np.array_equal(lit[:lit_bytes], dc.pack_model(buf, offs, base, nb, chunks, rep, want)), name
    assert np.array_equal(d_data.cpu().numpy(), buf), name
    # apply from the same buffer: the base files' ranges of it, the targets rebuilt at odd offsets
    out_lens = lens[nb:]
    rng = np.random.default_rng(8)
    out_offs, size = dc._layout(out_lens, rng, True)
    start = rng.integers(0, 256, size, dtype=np.uint8)
    d_out = u8(start)
    cdc.delta_apply(ctx, g_runs.inner, rows, offs[:nb], lens[:nb], d_data, g_out.inner, lit_bytes, out_offs, out_lens, d_out)
    torch.cuda.synchronize()
    expect = dc.apply_model(want["runs"], buf, offs[:nb], lens[:nb], lit, lit_bytes, start.copy(), out_offs, out_lens)
    assert expect is not dc.INVALID, name
    got = d_out.cpu().numpy()
    assert np.array_equal(got, expect), (name, np.flatnonzero(got != expect)[:8])
    for t, f in enumerate(range(nb, len(lens))):
        a, L = int(offs[f]), int(lens[f])
        assert np.array_equal(got[int(out_offs[t]):int(out_offs[t]) + L], buf[a:a + L]), (name, t)
    assert np.array_equal(g_runs.host().view(U).reshape(-1, 4)[:rows], want["runs"]) and np.array_equal(d_data.cpu().numpy(), buf)


# ---------------------------------------------------------------- the plan
def test_plan_on_tables(ctx):
    for case in dc.table_cases():
        assert_plan(ctx, case)


def test_plan_pack_apply_on_data_cases(ctx):
    for case in dc.data_cases():
        assert_round_trip(ctx, case)


def test_many_target_chunks(ctx):
    """more than 262 144 target chunks: past one trip of a sliced grid"""
    want = assert_plan(ctx, dc.many_table())[0]
    assert int(want["stats"][1]) > 262_144


def test_round_trip_on_every_cdc_case(ctx):
    cases = cc.all_cases()
    assert len(cases) >= 30
    for case in cases:
        assert_round_trip(ctx, dc.split_of(case))


def test_plan_capacity_count_only_and_null_outputs(ctx):
    name, base, nb, chunks, ids = next(c for c in dc.table_cases() if c[0] == "merge_and_not")
    rep = dc.rep_of(chunks, ids)
    want = dc.plan_model(base, nb, chunks, rep)
    d_chunks, d_rep = device_rep(ctx, base, chunks, ids)
    mt, nt, rows = len(want["lit_off"]), len(want["files"]), len(want["runs"])
    assert rows >= 3
    for cap in (rows - 1, 0):  # one short, and none: the requirement, no row, everything else complete
        got, n_runs, rc, _, _ = plan_guarded(ctx, base, nb, d_chunks, d_rep, mt, nt, rows + SPARE, cap)
        assert rc == SD_ERR_CAPACITY and n_runs == rows and (got["runs"] == FILL).all(), cap
        for k in ("lit_off", "files", "stats"):
            assert np.array_equal(got[k], want[k]), (k, cap)
    got, n_runs, rc, _, _ = plan_guarded(ctx, base, nb, d_chunks, d_rep, mt, nt, rows + SPARE, rows)  # exact
    assert rc == 0 and np.array_equal(got["runs"][:rows], want["runs"]) and (got["runs"][rows:] == FILL).all()
    for mask in range(8):
        got, n_runs, rc, _, _ = plan_guarded(ctx, base, nb, d_chunks, d_rep, mt, nt, rows, rows, mask)
        assert rc == 0 and n_runs == rows and np.array_equal(got["stats"], want["stats"]), mask
        for bit, key in ((1, "lit_off"), (2, "runs"), (4, "files")):
            assert np.array_equal(got[key], want[key]) if mask & bit else (got[key] == FILL).all(), (mask, key)
    n_runs, stats = cdc.delta_plan(ctx, base, nb, d_chunks, d_rep)  # every output NULL: only counts
    assert n_runs == rows and np.array_equal(stats, want["stats"])
    n = len(base) - 1
    assert lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data, n, nb, d_chunks.data_ptr(), d_rep.data_ptr(), None, None, 0,
                                   None, None, None, None) == 0
    # n_base == n and n == 0 give zeros; bad arguments are refused
    cnt, st = ctypes.c_uint64(7), np.full(8, 7, U)
    assert lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data, n, n, d_chunks.data_ptr(), d_rep.data_ptr(), None, None, 0,
                                   ctypes.byref(cnt), None, st.ctypes.data, None) == 0 and cnt.value == 0 and not st.any()
    cnt, st = ctypes.c_uint64(7), np.full(8, 7, U)
    assert lib().sd_cdc_delta_plan(ctx.handle, None, 0, 0, None, None, None, None, 0, ctypes.byref(cnt), None, st.ctypes.data,
                                   None) == 0 and cnt.value == 0 and not st.any()
    assert lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data, n, n + 1, d_chunks.data_ptr(), d_rep.data_ptr(), None, None, 0,
                                   None, None, None, None) == -1
    assert lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data, n, nb, None, d_rep.data_ptr(), None, None, 0, None, None, None,
                                   None) == -1
    assert lib().sd_cdc_delta_plan(ctx.handle, base.ctypes.data, n, nb, d_chunks.data_ptr(), None, None, None, 0, None, None,
                                   None, None) == -1
    bad = rep.copy()
    bad[int(base[nb])] = int(base[nb]) + 1  # a representative behind its slot: refused, no access outside the tables
    with pytest.raises(SdCasError):
        cdc.delta_plan(ctx, base, nb, d_chunks, dev(bad))


# ---------------------------------------------------------------- the copy through hand-made recipes
def run_recipe(ctx, case, exact_lit=False):
    name, lit, runs, out_offs, out_lens, size = case
    rng = np.random.default_rng(5)
    start = rng.integers(0, 256, size, dtype=np.uint8)  # random surroundings: they must come back unchanged
    want = dc.apply_model(runs, None, [], [], lit, len(lit), start.copy(), out_offs, out_lens)
    assert want is not dc.INVALID, name
    assert len(lit) % 64 == 0 or not exact_lit
    d_lit = u8(lit if exact_lit else np.concatenate([lit, np.zeros((-len(lit)) % 64 + 64, np.uint8)]))
    d_runs, d_out = dev(runs.reshape(-1)), u8(start)
    cdc.delta_apply(ctx, d_runs, len(runs), [], [], None, d_lit, len(lit), out_offs, out_lens, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
    assert np.array_equal(d_runs.cpu().numpy().view(U).reshape(-1, 4), runs) and np.array_equal(d_lit.cpu().numpy()[:len(lit)], lit)
    cpu_got, _ = cpu.cdc_delta_apply(runs, np.zeros(0, np.uint8), [], [], lit, out_lens, start.copy(), out_offs)
    assert np.array_equal(got, cpu_got), name


@pytest.mark.parametrize("name", ["residues", "lengths", "meeting", "readable_limit", "many_runs"])
def test_recipes(ctx, name):
    case = next(c for c in dc.recipe_cases() if c[0] == name)
    run_recipe(ctx, case, exact_lit=name == "readable_limit")


def test_one_run_of_64_mib_and_1(ctx):
    run_recipe(ctx, dc.recipe_cases(big=True)[0])


# ---------------------------------------------------------------- refusals
def test_bad_recipes_write_nothing(ctx):
    """every out-of-range span of a bad recipe lies inside the slack the buffers carry: a faulty
    validator shows as bytes written, never as an access outside an allocation"""
    bad, good = dc.bad_recipes()
    rng = np.random.default_rng(6)
    S = dc.SLACK
    base = rng.integers(0, 256, S + 4096 + S, dtype=np.uint8)
    bo, bl = np.array([0, 1024], U), np.array(dc.BAD_BASE_LENS, U)
    lit_all = rng.integers(0, 256, S + dc.BAD_LIT + S, dtype=np.uint8)
    oo, ol = np.array([7, 1001], U), np.array(dc.BAD_OUT_LENS, U)
    start = rng.integers(0, 256, S + 4096 + S, dtype=np.uint8)
    d_base_all, d_lit_all = u8(base), u8(lit_all)
    d_base, d_lit = d_base_all[S:], d_lit_all[S:]

    def call(runs):
        g = Guarded(1, len(start))
        g.inner.copy_(torch.from_numpy(start))
        r = np.array(runs, U).reshape(-1, 4)
        d_runs = dev(r.reshape(-1)) if len(r) else None
        rc = 0
        try:
            cdc.delta_apply(ctx, d_runs, len(r), bo, bl, d_base, d_lit, dc.BAD_LIT, oo, ol, g.inner[S:])
        except SdCasError as e:
            rc = e.rc
        torch.cuda.synchronize()
        assert g.guards_intact()
        return rc, g.host().reshape(-1)
    rc, out = call(good)
    want = start.copy()
    want[S:] = dc.apply_model(np.array(good, U), base[S:], bo, bl, lit_all[S:], dc.BAD_LIT, start[S:].copy(), oo, ol)
    assert rc == 0 and np.array_equal(out, want) and not np.array_equal(out, start)
    for name, runs in bad:
        rc, out = call(runs)
        assert rc == -1 and np.array_equal(out, start), name
    assert np.array_equal(d_base_all.cpu().numpy(), base) and np.array_equal(d_lit_all.cpu().numpy(), lit_all)
    # bad arguments, refused before any allocation
    d_runs = dev(np.array(good, U).reshape(-1))
    args = (bo.ctypes.data, bl.ctypes.data, 2, d_base.data_ptr(), d_lit.data_ptr(), dc.BAD_LIT, oo.ctypes.data, ol.ctypes.data, 2)
    d_out = u8(start)
    assert lib().sd_cdc_delta_apply(ctx.handle, None, 3, *args, d_out.data_ptr(), None) == -1
    assert lib().sd_cdc_delta_apply(ctx.handle, d_runs.data_ptr(), 1 << 32, *args, d_out.data_ptr(), None) == -1
    assert lib().sd_cdc_delta_apply(ctx.handle, d_runs.data_ptr(), 3, *args, None, None) == -1
    assert lib().sd_cdc_delta_apply(ctx.handle, d_runs.data_ptr(), 3, bo.ctypes.data, bl.ctypes.data, 2, d_base.data_ptr() + 8,
                                    *args[4:], d_out.data_ptr(), None) == -1  # d_base not 16-byte aligned
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), start)


# ---------------------------------------------------------------- files
def test_delta_and_patch_files_on_both_routes(ctx, tmp_path):
    A, A5 = dc.insert5_files()
    other = cc.synth(31, 9000)
    files = [A, other, A5, np.zeros(0, np.uint8), np.concatenate([other, A[:70000]])]
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / f"f{i}"
        p.write_bytes(f.tobytes())
        paths.append(p)
    d = sd.delta_files(paths[:2], paths[2:], cc.P10, device=True)
    c = sd.delta_files(paths[:2], paths[2:], cc.P10, device=False)
    for k in ("runs", "literals", "target_lens", "checksums", "files", "stats"):
        assert np.array_equal(getattr(d, k), getattr(c, k)), k
    st = [int(x) for x in d.stats]
    assert st[0] == 3 and len(d.literals) == st[5] <= 6 * cc.P10[2] and len(d.runs) == st[7]
    for device in (True, False):
        for got, f in zip(sd.patch_files(paths[:2], d, device=device), files[2:]):
            assert np.array_equal(got, f), device
    flipped = cdc.Delta(d.runs, d.literals.copy(), d.target_lens, d.checksums, d.files, d.stats, d.params)
    flipped.literals[len(flipped.literals) // 2] ^= 0x80
    with pytest.raises(ValueError, match="target"):
        sd.patch_files(paths[:2], flipped, device=True)
    with pytest.raises(SdCasError):  # a recipe for other base files is refused, not applied
        sd.patch_files(paths[1:2], d, device=True)
