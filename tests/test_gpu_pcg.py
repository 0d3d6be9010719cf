"""BQ_PROJECTION_PCG on the MI355X: gpu_pcg_solve, gpu_pcg_gradient and gpu_divergence_double
equal the C restatement (tests/cpu_abi/pcg_abi.c) bit for bit, whatever the work arrays hold on entry; a sealed pocket
ends with finite values and truthful stats; 20 steps of the 64^3 mixed obstacle + level-set scene equal the stand-in;
a 256^3 moving sphere converges every projection and is divergence-free to the reported residual."""
import json
import os

import numpy as np
import pytest

import obstacle_case as OC
import obstacle_ref as R
import pcg_case as P
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, P.load_pcg()


# 384: rows of more than 256 doubles; 130 x 20 x 24: level 1 takes the tile smoother, level 0 odd-free rows
SHAPES = [(37, 29, 23), (99, 21, 18), (64, 64, 64), (384, 12, 14), (130, 20, 24)]


def shape_masks(dims):
    ni, nj, nk = dims
    h, bnd = R.edge_scene(dims)
    edge = (OC.classify(bnd, h, (nk, nj, ni)) > 0).astype(np.uint8)
    fams = R.mask_families(dims)
    return [("no mask", None), ("edge scene", edge), fams[0], fams[-2], ("random", R.random_mask(dims, 5))]


@pytest.mark.parametrize("dims", SHAPES)
def test_solve_and_gradient_equal_the_restatement(libs, dims):
    hip, cpu = libs
    ni, nj, nk = dims
    rng = np.random.default_rng(ni)
    dev = Dev(hip)
    try:
        for name, solid in shape_masks(dims):
            div = rng.standard_normal((nk, nj, ni))
            want_p, want_st = P.solve(cpu, div, solid, 1000, 1e-6)
            assert want_st[3] == 0, (name, want_st)
            for fill in (np.nan, 0.0):
                got_p, got_st = P.solve(hip, div, solid, 1000, 1e-6, fill=fill, dev=dev)
                check(hip)
                assert got_st == want_st, (name, fill, got_st, want_st)
                assert np.array_equal(got_p.view(np.uint64), want_p.view(np.uint64)), (name, fill)
            # the gradient on random velocities, and the fp64 divergence of the result
            u = rng.standard_normal((nk, nj, ni + 1)).astype(np.float32)
            v = rng.standard_normal((nk, nj + 1, ni)).astype(np.float32)
            w = rng.standard_normal((nk + 1, nj, ni)).astype(np.float32)
            cu, cv, cw = u.copy(), v.copy(), w.copy()
            sol_h = None if solid is None else np.ascontiguousarray(solid, np.uint8)
            cpu.gpu_pcg_gradient(cu.ctypes.data, cv.ctypes.data, cw.ctypes.data, want_p.ctypes.data,
                                 None if sol_h is None else sol_h.ctypes.data, ni, nj, nk, 0.75)
            dsol = None if solid is None else dev.put("solid", sol_h)
            hip.gpu_pcg_gradient(dev.put("u", u), dev.put("v", v), dev.put("w", w), dev.put("pp", got_p), dsol, ni, nj, nk, 0.75)
            check(hip)
            for c, a in (("u", cu), ("v", cv), ("w", cw)):
                assert np.array_equal(dev.get(c), a), (name, c)
            cd = np.zeros((nk, nj, ni))
            cpu.gpu_divergence_double(cu.ctypes.data, cv.ctypes.data, cw.ctypes.data, cd.ctypes.data, ni, nj, nk, 0.75)
            hip.gpu_divergence_double(dev["u"], dev["v"], dev["w"], dev.put("dd", np.full((nk, nj, ni), np.nan)), ni, nj, nk, 0.75)
            check(hip)
            assert np.array_equal(dev.get("dd"), cd), name
    finally:
        dev.free()


def test_sealed_pocket_ends_finite_with_truthful_stats(libs):
    hip, cpu = libs
    dims = (40, 36, 32)
    solid = P.hollow_box(dims, (8, 8, 8), (30, 26, 22))
    div = np.zeros(dims[::-1])
    div[12:18, 12:20, 12:25] = 1.0                      # a net source inside the pocket: no solution there
    dev = Dev(hip)
    try:
        p, st = P.solve(hip, div, solid, 200, 1e-6, fill=np.nan, dev=dev)
        check(hip)
    finally:
        dev.free()
    assert np.isfinite(p).all() and st[0] <= 200
    true_r, maxb, *_ = P.true_residual(div, solid, p)
    if P.STOP[int(st[3])] == "converged":
        assert true_r <= 1e-6 * maxb * (1 + 1e-6)
    else:
        assert P.STOP[int(st[3])] in ("iteration limit", "breakdown")
        assert true_r > 1e-6 * maxb
    cp, cst = P.solve(cpu, div, solid, 200, 1e-6)
    assert cst == st and np.array_equal(cp.view(np.uint64), p.view(np.uint64))


@pytest.mark.parametrize("scheme", [0, 3])
def test_mixed_scene_matches_the_stand_in(libs, scheme):
    """hashes and stats of the CPU stand-in: tests/golden/make_pcg_hashes.py"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_hashes.json")) as f:
        gold = json.load(f)
    want = gold[f"scheme{scheme}"]
    got = P.run_mixed(solver.host_lib(), hip, gold["n"], scheme, gold["steps"])
    first = next((i for i, (a, b) in enumerate(zip(want["hashes"], got["hashes"])) if a != b), None)
    assert first is None, f"step {first} differs: {got['stats'][first]} vs {want['stats'][first]}"
    assert got["stats"] == want["stats"]
    assert all(s["stop"] == "converged" for s in got["stats"]) and got["stats"][-1]["unconverged"] == 0
    assert got["rho_max"] > 0.1
    again = P.run_mixed(solver.host_lib(), hip, gold["n"], scheme, 5)
    assert again["hashes"] == got["hashes"][:5]


def test_moving_sphere_at_256_converges_and_is_divergence_free(libs):
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    n, iters = 256, 1000
    s = solver.BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1000)])
    s.setProjection(iters, 1.0, kind=2)
    s.setBoundary([(0, 0.5, 0.55, 0.5, 0.15, 0.0, 0.0, 0.3, 0.5, 0.0)])
    its = []
    for f in range(10):
        s.updateBoundary(f, 1.0 / n)
        s.advance(f, 1.0 / n)
        st = s.pcgStats()
        assert st["stop"] == "converged" and 0 < st["iterations"] < iters, (f, st)
        its.append(st["iterations"])
    check(hip)
    P.divergence_check(s, n)
    s.close()
    print("iterations per projection:", its)
