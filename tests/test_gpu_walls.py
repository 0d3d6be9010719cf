"""Closed domain walls on the MI355X: the walled sweep operators bit for bit against single walled
sweeps, the C restatement (tests/cpu_abi/walls_abi.c) and the all-flags path of the existing masked operators, on shapes
the fused kernel takes and shapes it refuses (launch counts say which ran); flags and faces against the restatement; the
PCG operators on solid + walls; whole boxed steps against the stand-in in every scheme with both projections, and the
divergence next to the closed walls after a converged PCG projection; one fused walled launch at a production shape."""
import json
import os

import numpy as np
import pytest

import fields as F
import obstacle_case as OC
import obstacle_ref as R
import pcg_case as PC
import walls_case as WC
from obstacle_case import Dev, check
from test_gpu_obstacle_edges import FUSED, REFUSED, expected_launches, launches, options

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 7)


@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, WC.load_walls()


def touching_mask(dims):
    """obstacle cells on the first / last planes, rows and wall columns plus one on the chunk boundary at plane 8"""
    fams = dict(R.mask_families(dims, kchunk=8))
    return fams["first/last planes, rows, wall columns"] | fams["plane 8+0"]


def sweeps_case(hip, cpu, dev, dims, sol, walls, fused):
    ni, nj, nk = dims
    beta = R.beta32()
    solidw = WC.wall_flags(sol, walls)
    rows = R.rows_of(sol)
    p = R.initial_p(solidw, 3)
    div = np.random.default_rng(17).standard_normal(solidw.shape).astype(np.float32)
    sp, rp, dp = dev.put("solidw", solidw), dev.put("rows", rows), dev.put("div", div)
    ones = dev.put("ones", np.ones_like(rows))
    nmax = max(COUNTS)
    ca, cb = p.copy(), p.copy()
    single = []
    bufs = [dev.put("s0", p), dev.put("s1", p)]
    for n in range(nmax):
        cpu.gpu_jacobi_sweep_masked_walls(ca.ctypes.data, div.ctypes.data, cb.ctypes.data, solidw.ctypes.data, rows.ctypes.data,
                                          walls, ni, nj, nk, R.ALPHA, beta)
        hip.gpu_jacobi_sweep_masked_walls(bufs[n % 2], dp, bufs[(n + 1) % 2], sp, rp, walls, ni, nj, nk, R.ALPHA, beta)
        got = dev.get("s1" if n % 2 == 0 else "s0")
        assert np.array_equal(got, cb), ("single", n + 1)
        single.append(got)
        ca, cb = cb, ca
    check(hip)
    assert not np.array_equal(single[0], p)
    for n in COUNTS:
        ref = single[n - 1]
        launches(hip)
        which = hip.gpu_jacobi_sweeps_masked_walls(dev.put("f0", p), dp, dev.put("f1", p), sp, rp, walls, ni, nj, nk, n, R.ALPHA, beta)
        check(hip)
        nl, ns = launches(hip)
        assert (nl, ns) == (expected_launches(n, fused), n), (n, nl, ns)
        if fused and n >= 3:
            assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_walls_kernel"
        assert which == nl % 2
        got = dev.get("f1" if which else "f0")
        assert np.array_equal(got, ref), ("walled sweeps", n)
        assert np.all(got[solidw != 0] == 0) and not np.signbit(got[solidw != 0]).any()
        # the all-flags path: the existing masked operator on solid + walls with every row marked dirty
        which = hip.gpu_jacobi_sweeps_masked(dev.put("g0", p), dp, dev.put("g1", p), sp, ones, ni, nj, nk, n, R.ALPHA, beta)
        check(hip)
        assert np.array_equal(dev.get("g1" if which else "g0"), ref), ("all flags", n)


@pytest.mark.parametrize("dims", FUSED + REFUSED)
def test_walled_sweeps(libs, dims):
    hip, cpu = libs
    dev = Dev(hip)
    fused = dims in FUSED
    ni, nj, nk = dims
    none, touching = np.zeros((nk, nj, ni), np.uint8), touching_mask(dims)
    assert touching[:, :, 1].any() and touching[8].any()
    try:
        with options(hip, JACOBI_FUSE=2, JACOBI_KCHUNK2=8):
            for walls in WC.MASKS:
                for name, sol in (("none", none), ("touching", touching)):
                    try:
                        sweeps_case(hip, cpu, dev, dims, sol, walls, fused)
                    except AssertionError as e:
                        raise AssertionError(f"walls {walls}, obstacles {name}: {e}") from e
            # walls = 0: the masked operator itself
            rows = R.rows_of(touching)
            p = R.initial_p(touching, 4)
            div = np.random.default_rng(18).standard_normal(p.shape).astype(np.float32)
            sp, rp, dp = dev.put("solidw", touching), dev.put("rows", rows), dev.put("div", div)
            beta = R.beta32()
            for n in (1, 7):
                a = hip.gpu_jacobi_sweeps_masked_walls(dev.put("f0", p), dp, dev.put("f1", p), sp, rp, 0, ni, nj, nk, n, R.ALPHA, beta)
                b = hip.gpu_jacobi_sweeps_masked(dev.put("g0", p), dp, dev.put("g1", p), sp, rp, ni, nj, nk, n, R.ALPHA, beta)
                check(hip)
                assert a == b and np.array_equal(dev.get("f1" if a else "f0"), dev.get("g1" if b else "g0"))
    finally:
        dev.free()


@pytest.mark.parametrize("dims", [(36, 13, 13), (99, 21, 18)])
def test_flags_and_faces_equal_the_restatement(libs, dims):
    hip, cpu = libs
    ni, nj, nk = dims
    sol = touching_mask(dims)
    sol[sol != 0] = 1 + (np.arange(int((sol != 0).sum())) % 3).astype(np.uint8)
    shapes = ((nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni))
    vel = [x.reshape(s) for x, s in zip(F.velocity(ni, nj, nk, 1.0 / ni), shapes)]
    dev = Dev(hip)
    try:
        for walls in WC.MASKS:
            for given in (sol, None):
                want = np.zeros((nk, nj, ni), np.uint8)
                cpu.gpu_wall_flags(want.ctypes.data, None if given is None else given.ctypes.data, walls, ni, nj, nk)
                sp = dev.put("solidw", np.full((nk, nj, ni), 7, np.uint8))
                hip.gpu_wall_flags(sp, None if given is None else dev.put("solid", given), walls, ni, nj, nk)
                check(hip)
                assert np.array_equal(dev.get("solidw"), want), (walls, given is None)
                assert np.array_equal(want, WC.wall_flags(np.zeros_like(sol) if given is None else given, walls))
                for with_d in (True, False):
                    host = [x.copy() for x in vel]
                    hd = [np.full_like(x, 9.0) for x in vel]
                    ptrs = [dev.put(nm, x) for nm, x in zip("uvw", vel)]
                    dptrs = [dev.put("d" + nm, x) for nm, x in zip("uvw", hd)] if with_d else [None] * 3
                    cpu.gpu_wall_faces(*[x.ctypes.data for x in host], *([x.ctypes.data for x in hd] if with_d else [None] * 3),
                                       want.ctypes.data, ni, nj, nk)
                    hip.gpu_wall_faces(*ptrs, *dptrs, sp, ni, nj, nk)
                    check(hip)
                    for nm, w in zip("uvw", host):
                        assert np.array_equal(dev.get(nm), w), (walls, nm)
                    if with_d:
                        for nm, w in zip("uvw", hd):
                            assert np.array_equal(dev.get("d" + nm), w), (walls, "d" + nm)
                    assert any((a != b).any() for a, b in zip(host, vel))
                    # the masked gradient in the walled window (u, v, w on the device are the face-written ones)
                    pr = F.scalar(ni, nj, nk, 0.7).reshape(nk, nj, ni).copy()
                    pr[want != 0] = 0
                    before = [x.copy() for x in host]
                    cpu.gpu_gradient_masked_walls(*[x.ctypes.data for x in host], pr.ctypes.data,
                                                  *([x.ctypes.data for x in hd] if with_d else [None] * 3), want.ctypes.data,
                                                  walls, ni, nj, nk, 0.5)
                    hip.gpu_gradient_masked_walls(*ptrs, dev.put("p", pr), *dptrs, sp, walls, ni, nj, nk, 0.5)
                    check(hip)
                    for nm, w in zip("uvw", host):
                        assert np.array_equal(dev.get(nm), w), (walls, "gradient", nm)
                    if with_d:
                        for nm, w in zip("uvw", hd):
                            assert np.array_equal(dev.get("d" + nm), w), (walls, "gradient d" + nm)
                    if walls & WC.XLO:              # the layer behind the closed side is projected: v faces at i = 1
                        assert (host[1][2:nk - 1, 2:nj - 1, 1] != before[1][2:nk - 1, 2:nj - 1, 1]).any()
                    else:
                        assert np.array_equal(host[1][:, :, 1], before[1][:, :, 1])
    finally:
        dev.free()


def test_pcg_on_solid_plus_walls_equals_the_restatement(libs):
    hip, cpu = libs
    dims = (40, 36, 32)
    ni, nj, nk = dims
    rng = np.random.default_rng(40)
    dev = Dev(hip)
    try:
        for sol in (np.zeros((nk, nj, ni), np.uint8), touching_mask(dims)):
            solidw = WC.wall_flags(sol, WC.REFERENCE_BOX)
            div = rng.standard_normal((nk, nj, ni))
            want_p, want_st = PC.solve(cpu, div, solidw, 1000, 1e-6)
            assert want_st[3] == 0, want_st
            got_p, got_st = PC.solve(hip, div, solidw, 1000, 1e-6, fill=np.nan, dev=dev)
            check(hip)
            assert got_st == want_st and np.array_equal(got_p.view(np.uint64), want_p.view(np.uint64))
            print("PCG in the reference box:", want_st)
            u = rng.standard_normal((nk, nj, ni + 1)).astype(np.float32)
            v = rng.standard_normal((nk, nj + 1, ni)).astype(np.float32)
            w = rng.standard_normal((nk + 1, nj, ni)).astype(np.float32)
            cu, cv, cw = u.copy(), v.copy(), w.copy()
            cpu.gpu_wall_faces(cu.ctypes.data, cv.ctypes.data, cw.ctypes.data, None, None, None, solidw.ctypes.data, ni, nj, nk)
            cpu.gpu_pcg_gradient(cu.ctypes.data, cv.ctypes.data, cw.ctypes.data, want_p.ctypes.data, solidw.ctypes.data, ni, nj, nk, 0.75)
            sp = dev.put("solid", solidw)
            up, vp, wp = dev.put("u", u), dev.put("v", v), dev.put("w", w)
            hip.gpu_wall_faces(up, vp, wp, None, None, None, sp, ni, nj, nk)
            hip.gpu_pcg_gradient(up, vp, wp, dev.put("pp", got_p), sp, ni, nj, nk, 0.75)
            check(hip)
            # ... and the walled window on top of it (a second update: the operators are compared, not the physics)
            cpu.gpu_pcg_gradient_walls(cu.ctypes.data, cv.ctypes.data, cw.ctypes.data, want_p.ctypes.data, solidw.ctypes.data,
                                       WC.REFERENCE_BOX, ni, nj, nk, 0.75)
            hip.gpu_pcg_gradient_walls(up, vp, wp, dev["pp"], sp, WC.REFERENCE_BOX, ni, nj, nk, 0.75)
            check(hip)
            gu, gv, gw = dev.get("u"), dev.get("v"), dev.get("w")
            for a, b in ((gu, cu), (gv, cv), (gw, cw)):
                assert np.array_equal(a, b)
            # the normal faces of the closed sides are exactly 0 after the gradient (where no obstacle cell lies in the border layer)
            if not sol.any():
                for face in (gu[:, :, 0], gu[:, :, 1], gu[:, :, ni - 1], gu[:, :, ni], gv[:, 0], gv[:, 1], gw[0], gw[1], gw[nk - 1], gw[nk]):
                    assert np.all(face == 0)
            assert np.any(gv[:, nj - 1] != 0)
    finally:
        dev.free()


def golden():
    """hashes of the CPU stand-in: tests/golden/make_walls_hashes.py"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walls_hashes.json")) as f:
        return json.load(f)


def walled_divergence_check(s, n, walls):
    """pcg_case.divergence_check with its window widened to the unknowns next to a closed wall: their wall face holds
    exactly 0 (no rounding at all, so the per-face term U (|g| + |u|) of the bound, kept as it is, only over-covers it) and
    their diagonal is 6 - s, so the exact update with halfrdx = 1 leaves div = -r there too."""
    U, UD = PC.U, PC.UD
    st = s.pcgStats()
    p = s.pcgPressure()
    u, v, w = (s.field(c).reshape(sh) for c, sh in (("u", (n, n, n + 1)), ("v", (n, n + 1, n)), ("w", (n + 1, n, n))))
    solidw = WC.wall_flags(s.solidMask(), walls)
    div = (u[:, :, 1:] - u[:, :, :-1].astype(np.float64)) + (v[:, 1:, :] - v[:, :-1, :].astype(np.float64)) + (w[1:] - w[:-1].astype(np.float64))
    gx = np.zeros(u.shape); gx[:, :, 1:n] = np.abs(p[:, :, 1:] - p[:, :, :-1])
    gy = np.zeros(v.shape); gy[:, 1:n, :] = np.abs(p[:, 1:, :] - p[:, :-1, :])
    gz = np.zeros(w.shape); gz[1:n] = np.abs(p[1:] - p[:-1])
    fx, fy, fz = (np.abs(a).astype(np.float64) for a in (u, v, w))
    face = lambda g, f: U * (g + f)
    bound = (face(gx, fx)[:, :, 1:] + face(gx, fx)[:, :, :-1] + face(gy, fy)[:, 1:, :] + face(gy, fy)[:, :-1, :]
             + face(gz, fz)[1:] + face(gz, fz)[:-1]) + UD * 8 * (fx[:, :, 1:] + fx[:, :, :-1] + fy[:, 1:] + fy[:, :-1] + fz[1:] + fz[:-1])
    lo = [1 if walls & bit else 2 for bit in (WC.ZLO, WC.YLO, WC.XLO)]          # a closed low side: the first interior cell too
    win = np.zeros((n, n, n), bool)
    win[lo[0]:n - 1, lo[1]:n - 1, lo[2]:n - 1] = True
    cells = win & PC.unknowns(solidw, solidw.shape)
    walled = np.zeros(solidw.shape, bool)
    walled[1:-1, 1:-1, 1:-1] = R.neighbour_count((solidw == WC.FLAG_WALL).astype(np.uint8)) > 0
    assert (cells & walled).sum() >= 100
    assert st["stop"] == "converged"
    excess = np.abs(div[cells]) - (st["max_r"] + bound[cells])
    assert excess.max() <= 0, (float(excess.max()), st)


@pytest.mark.parametrize("scheme", [0, 2, 3])
@pytest.mark.parametrize("name", ["jacobi", "pcg"])
def test_boxed_steps_match_the_stand_in(libs, scheme, name):
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    gold = golden()
    kind, iters, halfrdx = gold["kinds"][name]
    want = gold[f"scheme{scheme}_{name}"]
    got = WC.run_scene(solver.host_lib(), hip, gold["n"], scheme, gold["steps"], iters, walls=gold["walls"], kind=kind,
                       halfrdx=halfrdx, keep=True)
    s = got["solver"]
    try:
        first = next((i for i, (a, b) in enumerate(zip(want["hashes"], got["hashes"])) if a != b), None)
        assert first is None, f"step {first} differs (rho max {got['rho_max']} vs {want['rho_max']})"
        assert got["finite"] and want["rho_max"] > 0.1
        if kind == 2:
            print("PCG, boxed 64^3:", s.pcgStats())
            walled_divergence_check(s, gold["n"], gold["walls"])
    finally:
        s.close()


def test_production_shape_one_fused_walled_launch(libs):
    """256 x 128 x 40 with the default chunk length in the reference's container: one launch of three sweeps"""
    hip, _ = libs
    ni, nj, nk = 256, 128, 40
    walls = WC.REFERENCE_BOX
    solidw = WC.wall_flags(np.zeros((nk, nj, ni), np.uint8), walls)
    rows = np.zeros((nk, nj), np.uint8)
    p = R.initial_p(solidw, 9)
    div = np.random.default_rng(10).standard_normal(p.shape).astype(np.float32)
    beta = R.beta32()
    dev = Dev(hip)
    try:
        sp, rp, dp = dev.put("solidw", solidw), dev.put("rows", rows), dev.put("div", div)
        with options(hip, JACOBI_FUSE=2):
            which = hip.gpu_jacobi_sweeps_masked_walls(dev.put("f0", p), dp, dev.put("f1", p), sp, rp, walls, ni, nj, nk, 3, R.ALPHA, beta)
            check(hip)
            assert launches(hip) == (1, 3), "the fused walled kernel did not run"
        assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_walls_kernel"
        fused = dev.get("f1" if which else "f0")
        bufs = [dev.put("s0", p), dev.put("s1", p)]
        for s in range(3):
            hip.gpu_jacobi_sweep_masked_walls(bufs[s % 2], dp, bufs[(s + 1) % 2], sp, rp, walls, ni, nj, nk, R.ALPHA, beta)
        check(hip)
        single = dev.get("s1")
        assert np.array_equal(fused, single) and not np.array_equal(single, p)
        want = p
        for s in range(3):
            want = OC.masked_sweep(want, div, solidw, R.ALPHA, np.float32(beta))
        assert np.array_equal(single, want)
    finally:
        dev.free()
