"""Level-set obstacles on the MI355X: the three level-set operators bit for bit against the C restatement
(tests/cpu_abi/levelset_abi.c) on odd shapes with mixed lists, analytic-only lists through them against the analytic
operators, 20 steps of the 64^3 level-set scene in both schemes hash for hash against the CPU stand-in, and a moving
level-set sphere whose grid is larger than one L2 at 256^3."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fields as F
import levelset_case as LC
import obstacle_case as OC
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, OC.load_levelsets()


def lists(entries, dev):
    """(Boundary array, host descriptors, device descriptors, n): the device descriptors' phi are device copies"""
    from gpufluidsimulation_amd.solver import LevelSetObstacle, levelset_arrays
    arr, ls_h, n = levelset_arrays(entries)
    _, ls_d, _ = levelset_arrays(entries)
    for o, e in enumerate(entries):
        if isinstance(e, LevelSetObstacle):
            ls_d[o].phi = dev.put(f"phi{o}", e.levelset.phi)
    return arr, ls_h, ls_d, n


def mixed(dims):
    from gpufluidsimulation_amd.solver import LevelSet, LevelSetObstacle, levelset_sphere
    ni, nj, nk = dims
    h = 1.0 / ni
    X, Y, Z = ni * h, nj * h, nk * h
    r = 0.3 * min(Y, Z)
    cut = levelset_sphere(0.2 * min(Y, Z), h)
    m = cut.phi.shape[0]
    rim = LevelSet(cut.phi[2:m - 2, 2:m - 2, 2:m - 2], h, tuple(x + 2 for x in cut.index_min), cut.background)
    return h, [LevelSetObstacle(levelset_sphere(r, 0.7 * h), (0.02 * X, 0.5 * Y, 0.5 * Z)),
               (0, 0.55 * X, 0.45 * Y, 0.5 * Z, 0.25 * min(Y, Z), 0, 0, 0, 0, 0),
               LevelSetObstacle(LC.box_levelset((0.1 * X, 0.2 * Y, 0.15 * Z), 1.3 * h, 2), (0.6 * X + 0.3 * h, 0.5 * Y, 0.45 * Z)),
               (1, 0.62 * X, 0.5 * Y, 0.45 * Z, 0.05 * X, 0.1 * Y, 0.08 * Z, 0, 0, 0),
               LevelSetObstacle(rim, (0.3 * X + 0.1 * h, 0.3 * Y, 0.55 * Z))]


def run_ops(hip, cpu, dev, dims, h, entries, analytic_gpu=False):
    """flags + rows, the band pass on all four node families and the blend, on the device (the _ls operators, or with
    analytic_gpu the analytic ones) and in the C restatement; asserts equality and returns the CPU flags"""
    ni, nj, nk = dims
    arr, ls_h, ls_d, n = lists(entries, dev)
    A, LH, LD = C.addressof(arr), C.addressof(ls_h), C.addressof(ls_d)
    s_c, r_c = np.zeros(ni * nj * nk, np.uint8), np.zeros(nj * nk, np.uint8)
    cpu.gpu_obstacle_flags_ls(s_c.ctypes.data, r_c.ctypes.data, A, n, LH, h, ni, nj, nk)
    sp, rp = dev.put("solid", np.full_like(s_c, 7)), dev.put("rows", np.full_like(r_c, 7))
    if analytic_gpu:
        hip.gpu_obstacle_flags(sp, rp, A, n, h, ni, nj, nk)
    else:
        hip.gpu_obstacle_flags_ls(sp, rp, A, n, LD, h, ni, nj, nk)
    check(hip)
    assert np.array_equal(dev.get("solid"), s_c) and np.array_equal(dev.get("rows"), r_c)
    assert s_c.any() and (r_c == 0).any()
    u, v, w = F.velocity(ni, nj, nk, h)
    cfldt = 0.9 * h / 0.35
    band_nodes = 0
    for (dx, dy, dz), src in (((1, 0, 0), u), ((0, 1, 0), v), ((0, 0, 1), w), ((0, 0, 0), F.scalar(ni, nj, nk, 1.9))):
        base = np.full_like(src, -3.0)
        hb = base.copy()
        cpu.gpu_semilag_band_ls(hb.ctypes.data, src.ctypes.data, u.ctypes.data, v.ctypes.data, w.ctypes.data,
                                dx, dy, dz, h, ni, nj, nk, cfldt, -2.0 * h, A, n, LH)
        args = (dev.put("band", base), dev.put("src", src), dev.put("u0", u), dev.put("v0", v), dev.put("w0", w),
                dx, dy, dz, h, ni, nj, nk, cfldt, -2.0 * h, A, n)
        if analytic_gpu:
            hip.gpu_semilag_band(*args)
        else:
            hip.gpu_semilag_band_ls(*args, LD)
        check(hip)
        got = dev.get("band")
        assert np.array_equal(got, hb), (dx, dy, dz)
        band_nodes += int((got != -3.0).sum())
    assert band_nodes > 0
    rho, T = F.scalar(ni, nj, nk, 0.3), F.scalar(ni, nj, nk, 2.3)
    srcs = [x * np.float32(-1.5) for x in (u, v, w, rho, T)]
    for with_band in (True, False):
        host = [x.copy() for x in (u, v, w, rho, T)]
        cpu.gpu_obstacle_blend_ls(*[x.ctypes.data for x in host], *([x.ctypes.data for x in srcs] if with_band else [None] * 5),
                                  s_c.ctypes.data, A, n, LH, h, ni, nj, nk)
        names = ("bu", "bv", "bw", "brho", "bT")
        dp = [dev.put(nm, x) for nm, x in zip(names, (u, v, w, rho, T))]
        sp2 = [dev.put("s" + nm, x) for nm, x in zip(names, srcs)] if with_band else [None] * 5
        if analytic_gpu:
            hip.gpu_obstacle_blend(*dp, *sp2, sp, A, n, h, ni, nj, nk)
        else:
            hip.gpu_obstacle_blend_ls(*dp, *sp2, sp, A, n, LD, h, ni, nj, nk)
        check(hip)
        for nm, want in zip(names, host):
            assert np.array_equal(dev.get(nm), want), (nm, with_band)
    return s_c


@pytest.mark.parametrize("dims", [(37, 29, 23), (99, 21, 18), (64, 64, 64)])
def test_levelset_operators_match_the_restatement(libs, dims):
    hip, cpu = libs
    h, entries = mixed(dims)
    dev = Dev(hip)
    try:
        s = run_ops(hip, cpu, dev, dims, h, entries)
        owners = set(np.unique(s)) - {0}
        assert {1, 3}.issubset(owners) or {1, 5}.issubset(owners), owners     # level sets do own cells
    finally:
        dev.free()


def test_analytic_lists_through_the_levelset_entries(libs):
    """an analytic-only list: the _ls operators (on the device and in C) = the analytic operators on the device"""
    hip, cpu = libs
    dims = (99, 21, 18)
    h, entries = mixed(dims)
    analytic = [e for e in entries if isinstance(e, tuple)]
    dev = Dev(hip)
    try:
        a = run_ops(hip, cpu, dev, dims, h, analytic)
        b = run_ops(hip, cpu, dev, dims, h, analytic, analytic_gpu=True)
        assert np.array_equal(a, b)
    finally:
        dev.free()


@pytest.mark.parametrize("scheme", [0, 3])
def test_levelset_scene_matches_the_stand_in(libs, scheme):
    """hashes of the CPU stand-in: tests/golden/make_obstacle_hashes.py"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levelset_hashes.json")) as f:
        gold = json.load(f)
    got = OC.run_scene(solver.host_lib(), hip, gold["n"], scheme, gold["steps"], gold["jacobi_iters"], LC.scene)
    want = gold[f"scheme{scheme}"]
    first = next((i for i, (a, b) in enumerate(zip(want["hashes"], got["hashes"])) if a != b), None)
    assert first is None, f"step {first} differs (rho max {got['rho_max']} vs {want['rho_max']})"
    assert want["rho_max"] > 0.1


def test_moving_fine_sphere_at_256(libs):
    """voxel = h / 2: a 161^3 grid (16.7 MB, more than one XCD's L2); 5 steps with updateBoundary, fields finite, flags
    equal to the C restatement's at the moved centre"""
    from gpufluidsimulation_amd.scenes import rising_smoke
    from gpufluidsimulation_amd.solver import BimocqGPUSolver, LevelSetObstacle, levelset_arrays, levelset_sphere
    hip, cpu = libs
    n = 256
    h = 1.0 / n
    ob = LevelSetObstacle(levelset_sphere(0.15, 0.5 * h), (0.5, 0.5, 0.5), (0.3, 0.1, 0.0))
    assert ob.levelset.phi.nbytes > 4 << 20
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(50, 0.5)
    s.setBoundary([ob])
    dt = np.float32(2.0 * h)
    c = [np.float32(x) for x in ob.position]
    for f in range(5):
        s.updateBoundary(f, float(dt))
        s.advance(f, float(dt))
        c = [np.float32(ci + np.float32(vi) * dt) for ci, vi in zip(c, ob.velocity)]
    mask = s.solidMask()
    for name in ("rho", "T", "u", "v", "w", "p"):
        assert np.isfinite(s.field(name)).all(), name
    s.close()
    moved = LevelSetObstacle(ob.levelset, tuple(float(x) for x in c), ob.velocity)
    arr, ls, cnt = levelset_arrays([moved])
    want = np.zeros(n ** 3, np.uint8)
    rows = np.zeros(n * n, np.uint8)
    cpu.gpu_obstacle_flags_ls(want.ctypes.data, rows.ctypes.data, C.addressof(arr), cnt, C.addressof(ls), h, n, n, n)
    assert np.array_equal(mask.ravel(), (want != 0).astype(np.uint8))
    assert mask.sum() > 50000
