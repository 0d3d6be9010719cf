"""Closed domain walls on the CPU stand-in (tests/cpu_abi/walls_abi.c linked with the product's host sources): the
refusals, walls off again is no wall at all, the combined flags and the wall faces against numpy, the walled sweep
against the numpy masked sweep, its fixed point against a sparse direct solve, and boxed steps in every scheme.  No GPU."""
import hashlib

import numpy as np
import pytest

import fields as F
import obstacle_case as OC
import obstacle_ref as R
import walls_case as WC


@pytest.fixture(scope="module")
def lib():
    return WC.load_walls()


def make(lib, n=16, scheme=0, iters=20, **kw):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    _, em, _ = OC.scene(n)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=lib, scheme=scheme, **kw)
    s.setSmoke(0.0, 1.0, em)
    if not kw:
        s.setProjection(iters, 0.5)
    return s


def test_constants_match_the_header():
    from gpufluidsimulation_amd import solver
    assert (solver.WALL_XLO, solver.WALL_XHI, solver.WALL_YLO, solver.WALL_YHI, solver.WALL_ZLO, solver.WALL_ZHI) == WC.SIDES
    assert solver.WALLS_NONE == 0 and solver.WALLS_REFERENCE_BOX == WC.REFERENCE_BOX == 55 and solver.FLAG_WALL == 0x80


def test_refusals_leave_the_previous_setting(lib):
    from gpufluidsimulation_amd import _lib
    s = make(lib)
    assert s.walls() == 0
    s.setWalls(WC.YLO | WC.XHI)
    for bad, text in ((63, "six sides"), (64, "bits"), (-1, "bits"), (1 << 8, "bits")):
        with pytest.raises(_lib.BimocqError, match=f"bimocq error {_lib.FL_ERR_BAD_ARGUMENT}.*{text}"):
            s.setWalls(bad)
        assert s.walls() == (WC.YLO | WC.XHI)
    # multigrid-CG: refused in either order of the two calls, and the refused call changes nothing
    with pytest.raises(_lib.BimocqError, match=f"bimocq error {_lib.FL_ERR_UNSUPPORTED}.*walls"):
        s.setProjection(5, 0.5, kind=1)
    s.advance(0, 0.5 / 16)                              # still the walled Jacobi projection
    assert s.walls() == (WC.YLO | WC.XHI)
    s.setWalls(0)
    s.setProjection(5, 0.5, kind=1)
    with pytest.raises(_lib.BimocqError, match=f"bimocq error {_lib.FL_ERR_UNSUPPORTED}.*MGCG"):
        s.setWalls(WC.REFERENCE_BOX)
    assert s.walls() == 0
    s.setProjection(5, 0.5, kind=2)                     # PCG admits them
    s.setWalls(WC.REFERENCE_BOX)
    assert s.walls() == WC.REFERENCE_BOX
    s.close()
    r = make(lib, rank=0, nranks=2, ghost=3)
    with pytest.raises(_lib.BimocqError, match=f"bimocq error {_lib.FL_ERR_UNSUPPORTED}.*z-slab"):
        r.setWalls(WC.REFERENCE_BOX)
    assert r.walls() == 0
    r.setWalls(0)                                       # nothing to refuse
    r.close()


def test_stand_in_without_wall_operators_refuses():
    """the PCG stand-in has the obstacle operators but not the wall ones: the host solver's weak references are null"""
    import pcg_case as PC
    from gpufluidsimulation_amd import _lib
    lib = PC.load_pcg()
    s = make(lib)
    with pytest.raises(_lib.BimocqError, match=f"bimocq error {_lib.FL_ERR_UNSUPPORTED}.*no wall operators"):
        s.setWalls(WC.REFERENCE_BOX)
    assert s.walls() == 0
    s.close()


@pytest.mark.parametrize("obstacles", [False, True])
def test_walls_off_again_is_no_wall_at_all(lib, obstacles):
    hashes = []
    n = 20
    for call in (False, True):
        s = make(lib, n)
        if obstacles:
            s.setBoundary([OC.scene(n)[2][0]])
        if call:
            s.setWalls(WC.REFERENCE_BOX)
            s.advance(0, 0.5 / n)
            s.setWalls(0)
            s.close()
            s = make(lib, n)                             # the walled step changed the state: same start, walls set and removed
            s.setWalls(WC.REFERENCE_BOX)
            if obstacles:
                s.setBoundary([OC.scene(n)[2][0]])
            s.setWalls(0)
        digest = hashlib.sha256()
        for f in range(3):
            s.updateBoundary(f, 0.5 / n)
            s.advance(f, 0.5 / n)
            for name in ("rho", "T", "u", "v", "w", "p"):
                digest.update(s.field(name).tobytes())
        assert s.walls() == 0
        hashes.append(digest.hexdigest())
        s.close()
    assert hashes[0] == hashes[1]


def test_walls_change_the_flow_and_call_order_does_not(lib):
    n = 16
    res = []
    for order in ("none", "walls first", "boundary first"):
        s = make(lib, n)
        ob = [OC.scene(n)[2][0]]
        if order == "walls first":
            s.setWalls(WC.REFERENCE_BOX); s.setBoundary(ob)
        elif order == "boundary first":
            s.setBoundary(ob); s.setWalls(WC.REFERENCE_BOX)
        else:
            s.setBoundary(ob)
        for f in range(2):
            s.advance(f, 0.5 / n)
        res.append(s.field("v").copy())
        assert np.array_equal(s.solidMask() != 0, OC.classify(ob, 1.0 / n, (n, n, n)) > 0)     # obstacle cells only
        s.close()
    assert not np.array_equal(res[0], res[1])
    assert np.array_equal(res[1], res[2])


DIMS = (9, 7, 6)


def corner_box(dims):
    """obstacle flags (two owners) of boxes that overlap a corner of the border layer and an edge of it"""
    ni, nj, nk = dims
    solid = np.zeros((nk, nj, ni), np.uint8)
    solid[0:3, 0:2, 0:3] = 1
    solid[nk - 2:, 3:5, ni - 1] = 2
    return solid


@pytest.mark.parametrize("walls", WC.MASKS)
def test_flags_and_faces_match_numpy(lib, walls):
    ni, nj, nk = DIMS
    solid = corner_box(DIMS)
    for given in (solid, None):
        got = np.full((nk, nj, ni), 7, np.uint8)
        lib.gpu_wall_flags(got.ctypes.data, None if given is None else given.ctypes.data, walls, ni, nj, nk)
        want = WC.wall_flags(np.zeros_like(solid) if given is None else given, walls)
        assert np.array_equal(got, want)
    solidw = WC.wall_flags(solid, walls)
    assert np.array_equal(solidw[solid != 0], solid[solid != 0])                # the obstacle wins in the border layer
    assert set(np.unique(solidw)) == {0, 1, 2, WC.FLAG_WALL}
    shapes = ((nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni))
    vel = [x.reshape(sh) + np.float32(0.25) for x, sh in zip(F.velocity(ni, nj, nk, 1.0 / ni), shapes)]
    wm, om = WC.wall_face_masks(solidw), WC.obstacle_face_masks(solid)
    for with_d in (True, False):
        out = [x.copy() for x in vel]
        d = [np.full_like(x, 9.0) for x in vel]
        lib.gpu_wall_faces(*[x.ctypes.data for x in out], *([x.ctypes.data for x in d] if with_d else [None] * 3),
                           solidw.ctypes.data, ni, nj, nk)
        for c in range(3):
            assert wm[c].any() and not (wm[c] & om[c]).any()                     # disjoint from the obstacle faces
            assert np.all(out[c][wm[c]] == 0) and np.array_equal(out[c][~wm[c]], vel[c][~wm[c]])
            if with_d:
                assert np.array_equal(d[c][wm[c]], np.float32(0) - vel[c][wm[c]]) and np.all(d[c][~wm[c]] == 9.0)
    # all six faces of a wall cell that touches no obstacle cell are written
    if walls & WC.XHI:
        k, j, i = 1, 1, ni - 1
        assert solidw[k, j, i] == WC.FLAG_WALL
        assert wm[0][k, j, i] and wm[0][k, j, i + 1] and wm[1][k, j, i] and wm[1][k, j + 1, i] and wm[2][k, j, i] and wm[2][k + 1, j, i]


@pytest.mark.parametrize("walls", WC.MASKS)
def test_walled_sweep_matches_numpy(lib, walls):
    ni, nj, nk = 21, 10, 9
    solid = R.random_mask((ni, nj, nk), 3)
    for sol in (np.zeros_like(solid), solid):
        solidw = WC.wall_flags(sol, walls)
        rows = R.rows_of(sol)
        p = R.initial_p(solidw, 5)
        div = np.random.default_rng(6).standard_normal(p.shape).astype(np.float32)
        beta = R.beta32()
        a, b = p.copy(), p.copy()
        want = p
        for n in range(4):
            lib.gpu_jacobi_sweep_masked_walls(a.ctypes.data, div.ctypes.data, b.ctypes.data, solidw.ctypes.data, rows.ctypes.data,
                                              walls, ni, nj, nk, R.ALPHA, beta)
            want = OC.masked_sweep(want, div, solidw, R.ALPHA, np.float32(beta))
            assert np.array_equal(b, want), n
            a, b = b, a
        f, g = p.copy(), p.copy()
        which = lib.gpu_jacobi_sweeps_masked_walls(f.ctypes.data, div.ctypes.data, g.ctypes.data, solidw.ctypes.data,
                                                   rows.ctypes.data, walls, ni, nj, nk, 4, R.ALPHA, beta)
        assert which == 0 and np.array_equal(f, want)
        if not sol.any():        # without obstacles the neighbour count is the positional one
            assert np.array_equal(R.neighbour_count(solidw), WC.positional_count(solidw.shape, walls))


@pytest.mark.parametrize("walls", [WC.XLO, WC.YLO | WC.ZLO, WC.XHI | WC.YHI | WC.ZHI, WC.REFERENCE_BOX])
def test_walled_gradient_window(lib, walls):
    """the faces between two fluid cells from cell 1 on behind a closed low side, from cell 2 on behind an open one, take
    u - halfrdx (p_c - p_left); every other face keeps its value; the deltas say the same"""
    ni, nj, nk = DIMS
    solidw = WC.wall_flags(corner_box(DIMS), walls)
    shapes = ((nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni))
    vel = [x.reshape(sh).copy() for x, sh in zip(F.velocity(ni, nj, nk, 1.0 / ni), shapes)]
    p = np.random.default_rng(2).standard_normal((nk, nj, ni)).astype(np.float32)
    p64 = p.astype(np.float64)
    lo = [1 if walls & b else 2 for b in (WC.ZLO, WC.YLO, WC.XLO)]
    for with_d in (True, False):
        out = [x.copy() for x in vel]
        d = [np.full_like(x, 9.0) for x in vel]
        args = [x.ctypes.data for x in out] + [p.ctypes.data] + ([x.ctypes.data for x in d] if with_d else [None] * 3)
        lib.gpu_gradient_masked_walls(*args, solidw.ctypes.data, walls, ni, nj, nk, 0.5)
        u64 = np.zeros((nk, nj, ni))
        for axis, c in ((2, 0), (1, 1), (0, 2)):
            a, b = WC._pair(solidw, axis)
            fluid = (a == 0) & (b == 0)
            win = np.zeros(shapes[c], bool)
            win[lo[0]:nk, lo[1]:nj, lo[2]:ni] = True
            upd = fluid & win
            g = np.zeros(shapes[c], np.float32)
            sl = [slice(None)] * 3
            sl[axis] = slice(1, None)
            lo_sl = list(sl); lo_sl[axis] = slice(None, -1)
            inner = [slice(None)] * 3; inner[axis] = slice(1, -1)
            g[tuple(inner)] = p[tuple(sl)] - p[tuple(lo_sl)]
            want = np.where(upd, vel[c] - np.float32(0.5) * g, vel[c])
            assert np.array_equal(out[c], want), c
            assert (upd & (out[c] != vel[c])).any()
            if with_d:
                assert np.array_equal(d[c][upd], (out[c] - vel[c])[upd]) and np.all(d[c][fluid & ~upd] == 0) and np.all(d[c][~fluid] == 9.0)
    pd = p64.copy()
    out = [x.copy() for x in vel]
    lib.gpu_pcg_gradient_walls(*[x.ctypes.data for x in out], pd.ctypes.data, solidw.ctypes.data, walls, ni, nj, nk, 0.5)
    ref = [x.copy() for x in vel]
    lib.gpu_gradient_masked_walls(*[x.ctypes.data for x in ref], p.ctypes.data, None, None, None, solidw.ctypes.data, walls, ni, nj, nk, 0.5)
    for c in range(3):
        assert np.array_equal(out[c] != vel[c], ref[c] != vel[c])               # the same faces
        assert np.allclose(out[c], ref[c], rtol=0, atol=4 * 2.0 ** -24 * (np.abs(vel[c]).max() + np.abs(p).max()))


def test_fixed_point_is_the_direct_solve(lib):
    """12 x 10 x 9 in the reference's container: the float32 iterate stays within obstacle_ref's derived bound of the fp64
    one, and that one has converged to the sparse direct solve of the Neumann system of solidw"""
    import scipy.sparse.linalg as spla
    ni, nj, nk = 12, 10, 9
    solidw = WC.wall_flags(np.zeros((nk, nj, ni), np.uint8), WC.REFERENCE_BOX)
    rows = np.zeros((nk, nj), np.uint8)
    div = np.random.default_rng(11).standard_normal(solidw.shape).astype(np.float32)
    A, b, unk = R.neumann_system(div, solidw)
    assert unk.sum() == (ni - 2) * (nj - 2) * (nk - 2)
    x = spla.spsolve(A.tocsc(), b)
    N = 6000
    its, bounds = R.masked_sweeps(np.zeros(solidw.shape), div, solidw, N)
    assert np.abs(its[-1] - its[-2]).max() < 1e-13 * np.abs(x).max()
    assert np.allclose(its[-1][unk], x, rtol=0, atol=1e-10 * np.abs(x).max())
    p, t = np.zeros(solidw.shape, np.float32), np.zeros(solidw.shape, np.float32)
    which = lib.gpu_jacobi_sweeps_masked_walls(p.ctypes.data, div.ctypes.data, t.ctypes.data, solidw.ctypes.data, rows.ctypes.data,
                                               WC.REFERENCE_BOX, ni, nj, nk, N, R.ALPHA, R.beta32())
    got = t if which else p
    err = float(np.abs(got[unk] - x).max())
    print(f"fixed point: error {err:.3g}, bound {bounds[-1]:.3g}, max|x| {np.abs(x).max():.3g}")
    assert err <= bounds[-1] + 1e-10 * np.abs(x).max()
    assert np.all(got[solidw != 0] == 0)


@pytest.mark.parametrize("scheme", [0, 2, 3])
def test_boxed_steps_are_reproducible_and_finite(lib, scheme):
    a = WC.run_scene(lib, lib, 24, scheme, 6, 20)
    b = WC.run_scene(lib, lib, 24, scheme, 6, 20)
    assert a["hashes"] == b["hashes"] and len(set(a["hashes"])) == 6
    assert a["finite"] and a["rho_max"] > 0.1


def test_wall_faces_are_zero_after_a_boxed_step(lib):
    """Jacobi and PCG: the normal faces of the closed sides (and every other face of a wall cell) hold exactly 0 after the
    projection, the open top does not"""
    n = 16
    for kind, iters in ((0, 20), (2, 200)):
        r = WC.run_scene(lib, lib, n, 0, 2, iters, kind=kind, keep=True)
        s = r["solver"]
        u, v, w = s.field("u").reshape(n, n, n + 1), s.field("v").reshape(n, n + 1, n), s.field("w").reshape(n + 1, n, n)
        solidw = WC.wall_flags(np.zeros((n, n, n), np.uint8), WC.REFERENCE_BOX)
        mu, mv, mw = WC.wall_face_masks(solidw)
        ob = WC.obstacle_face_masks(s.solidMask())
        for f, m, o in ((u, mu, ob[0]), (v, mv, ob[1]), (w, mw, ob[2])):
            assert np.all(f[m & ~o] == 0)
        assert np.all(u[:, :, 1] == 0) and np.all(u[:, :, n - 1] == 0) and np.all(v[:, 1, :] == 0) and np.all(w[1] == 0)
        assert np.any(v[:, n - 1, :] != 0) or np.any(v[:, n - 2, :] != 0)
        s.close()
