"""Solid obstacles on the MI355X: every obstacle operator bit for bit against the C restatement
(tests/cpu_abi/obstacle_abi.c) on odd shapes, the masked multi-sweep against single masked sweeps and, on a grid
without solids, against gpu_jacobi_sweeps; then 20 steps of a 64^3 rising-smoke scene with a static sphere and a moving
box in both schemes, hash for hash against the host solver linked to the CPU stand-in."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fields as F
import obstacle_case as OC
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, OC.load_obstacles()


DIMS = [(100, 21, 18), (64, 64, 64), (128, 36, 20)]


def scene_for(dims):
    ni, nj, nk = dims
    h = 1.0 / ni
    X, Y, Z = ni * h, nj * h, nk * h
    # a sphere cut by the x = 0 wall, a box overlapping a second sphere (later obstacle wins)
    return h, [(0, 0.02 * X, 0.5 * Y, 0.5 * Z, 0.3 * min(Y, Z), 0, 0, 0.3, -0.2, 0.1),
               (0, 0.55 * X, 0.45 * Y, 0.5 * Z, 0.25 * min(Y, Z), 0, 0, 0.0, 0.5, 0.0),
               (1, 0.6 * X, 0.5 * Y, 0.45 * Z, 0.1 * X, 0.2 * Y, 0.15 * Z, -0.4, 0.0, 0.2)]


def flags_both(hip, cpu, dev, dims, bnd, h):
    from gpufluidsimulation_amd.solver import boundary_array
    ni, nj, nk = dims
    arr, n = boundary_array(bnd)
    s_c, r_c = np.zeros(ni * nj * nk, np.uint8), np.zeros(nj * nk, np.uint8)
    cpu.gpu_obstacle_flags(s_c.ctypes.data, r_c.ctypes.data, C.addressof(arr), n, h, ni, nj, nk)
    hip.gpu_obstacle_flags(dev.put("solid", np.full_like(s_c, 7)), dev.put("rows", np.full_like(r_c, 7)),
                           C.addressof(arr), n, h, ni, nj, nk)
    check(hip)
    return s_c, r_c, arr, n


class fused_sweeps:
    """FL_OPT_JACOBI_FUSE = 2 and chunks of 8 planes, so that the three-sweep kernels run on these small grids"""
    def __init__(self, hip):
        self.hip = hip

    def __enter__(self):
        from gpufluidsimulation_amd import _lib
        self.was = [self.hip.fl_get_option(o) for o in (_lib.FL_OPT_JACOBI_FUSE, _lib.FL_OPT_JACOBI_KCHUNK2)]
        self.hip.fl_set_option(_lib.FL_OPT_JACOBI_FUSE, 2)
        self.hip.fl_set_option(_lib.FL_OPT_JACOBI_KCHUNK2, 8)

    def __exit__(self, *exc):
        from gpufluidsimulation_amd import _lib
        self.hip.fl_set_option(_lib.FL_OPT_JACOBI_FUSE, self.was[0])
        self.hip.fl_set_option(_lib.FL_OPT_JACOBI_KCHUNK2, self.was[1])


@pytest.mark.parametrize("dims", DIMS)
def test_operators_match_the_restatement(libs, dims):
    hip, cpu = libs
    ni, nj, nk = dims
    h, bnd = scene_for(dims)
    dev = Dev(hip)
    try:
        s_c, t_c, arr, n = flags_both(hip, cpu, dev, dims, bnd, h)
        assert np.array_equal(dev.get("solid"), s_c) and np.array_equal(dev.get("rows"), t_c)
        assert s_c.any() and (t_c == 0).any()
        solid_p, tiles_p = dev["solid"], dev["rows"]
        u, v, w = F.velocity(ni, nj, nk, h)
        # solid faces (+ delta share)
        for with_d in (True, False):
            hu, hv, hw = u.copy(), v.copy(), w.copy()
            hd = [np.full_like(x, 9.0) for x in (u, v, w)]
            ptrs = [dev.put(nm, x) for nm, x in zip(("u", "v", "w"), (u, v, w))]
            dptrs = [dev.put(nm, x) for nm, x in zip(("du", "dv", "dw"), hd)] if with_d else [None] * 3
            cpu.gpu_obstacle_faces(hu.ctypes.data, hv.ctypes.data, hw.ctypes.data,
                                   *([x.ctypes.data for x in hd] if with_d else [None] * 3),
                                   s_c.ctypes.data, C.addressof(arr), n, ni, nj, nk)
            hip.gpu_obstacle_faces(*ptrs, *dptrs, solid_p, C.addressof(arr), n, ni, nj, nk)
            check(hip)
            for nm, want in zip(("u", "v", "w"), (hu, hv, hw)):
                assert np.array_equal(dev.get(nm), want), nm
            if with_d:
                for nm, want in zip(("du", "dv", "dw"), hd):
                    assert np.array_equal(dev.get(nm), want), nm
        # masked gradient, with and without delta (u, v, w on the device are the face-written ones)
        p = F.scalar(ni, nj, nk, 0.7)
        p[s_c != 0] = 0
        pp = dev.put("p", p)
        for with_d in (True, False):
            hu, hv, hw = dev.get("u"), dev.get("v"), dev.get("w")
            hd = [np.full_like(x, 9.0) for x in (hu, hv, hw)]
            dptrs = [dev.put(nm, x) for nm, x in zip(("du", "dv", "dw"), hd)] if with_d else [None] * 3
            cpu.gpu_gradient_masked(hu.ctypes.data, hv.ctypes.data, hw.ctypes.data, p.ctypes.data,
                                    *([x.ctypes.data for x in hd] if with_d else [None] * 3), s_c.ctypes.data, ni, nj, nk, 0.5)
            hip.gpu_gradient_masked(dev["u"], dev["v"], dev["w"], pp, *dptrs, solid_p, ni, nj, nk, 0.5)
            check(hip)
            for nm, want in zip(("u", "v", "w"), (hu, hv, hw)):
                assert np.array_equal(dev.get(nm), want), nm
            if with_d:
                for nm, want in zip(("du", "dv", "dw"), hd):
                    assert np.array_equal(dev.get(nm), want), nm
        # masked sweeps: 5 on the device = 5 in the restatement = 5 single masked sweeps on the device
        div = F.scalar(ni, nj, nk, 1.9)
        beta = float(np.float32(1 / 6))
        hp, ht = p.copy(), p.copy()
        wc = cpu.gpu_jacobi_sweeps_masked(hp.ctypes.data, div.ctypes.data, ht.ctypes.data, s_c.ctypes.data, t_c.ctypes.data,
                                          ni, nj, nk, 5, -1.0, beta)
        pd, td, dd = dev.put("p", p), dev.put("pt", p), dev.put("div", div)
        wg = hip.gpu_jacobi_sweeps_masked(pd, dd, td, solid_p, tiles_p, ni, nj, nk, 5, -1.0, beta)
        check(hip)
        assert wc == wg == 1
        assert np.array_equal(dev.get("pt"), ht)
        a, b = dev.put("a", p), dev.put("b", p)
        for s in range(5):
            hip.gpu_jacobi_sweep_masked(a, dd, b, solid_p, tiles_p, ni, nj, nk, -1.0, beta)
            a, b = b, a
        check(hip)
        assert np.array_equal(dev.get("b"), ht)          # after 5 swaps the newest iterate sits in the buffer named "b"
        # the fused masked sweeps (two launches of three + one single sweep) against the single masked sweeps
        h7, t7 = p.copy(), p.copy()
        cpu.gpu_jacobi_sweeps_masked(h7.ctypes.data, div.ctypes.data, t7.ctypes.data, s_c.ctypes.data, t_c.ctypes.data,
                                     ni, nj, nk, 7, -1.0, beta)
        one = [dev.put("s1", p), dev.put("s2", p)]
        for s in range(7):
            hip.gpu_jacobi_sweep_masked(one[s % 2], dd, one[(s + 1) % 2], solid_p, tiles_p, ni, nj, nk, -1.0, beta)
        with fused_sweeps(hip):
            wf = hip.gpu_jacobi_sweeps_masked(dev.put("f1", p), dd, dev.put("f2", p), solid_p, tiles_p, ni, nj, nk, 7, -1.0, beta)
            assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_masked_kernel"
        check(hip)
        assert wf == 1
        assert np.array_equal(dev.get("s2"), t7)
        assert np.array_equal(dev.get("f2"), dev.get("s2"))
        # band semi-Lagrangian: band nodes of each buffer, everything else left alone
        cfldt = 0.9 * h / 0.35
        for (dx, dy, dz), src in (((1, 0, 0), u), ((0, 1, 0), v), ((0, 0, 1), w), ((0, 0, 0), div)):
            base = np.full_like(src, -3.0)
            hb = base.copy()
            cpu.gpu_semilag_band(hb.ctypes.data, src.ctypes.data, u.ctypes.data, v.ctypes.data, w.ctypes.data,
                                 dx, dy, dz, h, ni, nj, nk, cfldt, -2.0 * h, C.addressof(arr), n)
            hip.gpu_semilag_band(dev.put("band", base), dev.put("src", src), dev.put("u0", u), dev.put("v0", v),
                                 dev.put("w0", w), dx, dy, dz, h, ni, nj, nk, cfldt, -2.0 * h, C.addressof(arr), n)
            check(hip)
            got = dev.get("band")
            assert np.array_equal(got, hb), (dx, dy, dz)
            assert (got != -3.0).any() and (got == -3.0).any()
        # band blend + density clear
        rho, T = F.scalar(ni, nj, nk, 0.3), F.scalar(ni, nj, nk, 2.3)
        srcs = [x * np.float32(-1.5) for x in (u, v, w, rho, T)]
        host = [x.copy() for x in (u, v, w, rho, T)]
        cpu.gpu_obstacle_blend(*[x.ctypes.data for x in host], *[x.ctypes.data for x in srcs], s_c.ctypes.data,
                               C.addressof(arr), n, h, ni, nj, nk)
        names = ("bu", "bv", "bw", "brho", "bT")
        hip.gpu_obstacle_blend(*[dev.put(nm, x) for nm, x in zip(names, (u, v, w, rho, T))],
                               *[dev.put("s" + nm, x) for nm, x in zip(names, srcs)], solid_p, C.addressof(arr), n, h, ni, nj, nk)
        check(hip)
        for nm, want in zip(names, host):
            assert np.array_equal(dev.get(nm), want), nm
        assert np.all(dev.get("brho")[s_c != 0] == 0)
    finally:
        dev.free()


def test_clean_grid_equals_the_unmasked_sweeps(libs):
    """no solid cell anywhere: every block takes the unmasked stream, the same bits as gpu_jacobi_sweeps -- fused three
    sweeps per launch on both sides, and one sweep per launch"""
    hip, _ = libs
    ni, nj, nk = 128, 40, 24
    dev = Dev(hip)
    try:
        p, div = F.scalar(ni, nj, nk, 0.4), F.scalar(ni, nj, nk, 1.1)
        beta = float(np.float32(1 / 6))
        s = dev.put("solid", np.zeros(ni * nj * nk, np.uint8))
        t = dev.put("rows", np.zeros(nj * nk, np.uint8))
        dd = dev.put("div", div)
        with fused_sweeps(hip):
            wm = hip.gpu_jacobi_sweeps_masked(dev.put("p", p), dd, dev.put("pt", p), s, t, ni, nj, nk, 7, -1.0, beta)
            assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_masked_kernel"
            wr = hip.gpu_jacobi_sweeps(dev.put("q", p), dd, dev.put("qt", p), ni, nj, nk, 7, -1.0, beta)
            assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_kernel"
        w1 = hip.gpu_jacobi_sweeps_masked(dev.put("a", p), dd, dev.put("at", p), s, t, ni, nj, nk, 7, -1.0, beta)
        check(hip)
        assert wm == wr == w1 == 1
        assert np.array_equal(dev.get("pt"), dev.get("qt"))
        assert np.array_equal(dev.get("at"), dev.get("qt"))
    finally:
        dev.free()


@pytest.mark.parametrize("scheme", [0, 3])
def test_rising_smoke_with_obstacles_matches_the_stand_in(libs, scheme):
    """hashes of the CPU stand-in: tests/golden/make_obstacle_hashes.py"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obstacle_hashes.json")) as f:
        gold = json.load(f)
    got = OC.run_scene(solver.host_lib(), hip, gold["n"], scheme, gold["steps"], gold["jacobi_iters"])
    want = gold[f"scheme{scheme}"]
    first = next((i for i, (a, b) in enumerate(zip(want["hashes"], got["hashes"])) if a != b), None)
    assert first is None, f"step {first} differs (rho max {got['rho_max']} vs {want['rho_max']})"
    assert want["rho_max"] > 0.1
