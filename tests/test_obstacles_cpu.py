"""Solid obstacles on the CPU stand-in (tests/cpu_abi/obstacle_abi.c linked with the product's host sources): the flags
against numpy, the masked sweep against a numpy restatement, the host solver's obstacle path (face velocities after the
projection, cleared density, moving obstacles, n = 0 is no obstacle at all) and the refusals.  No GPU."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import obstacle_case as OC
from build_cpu_host import build as build_cpu_host


@pytest.fixture(scope="module")
def lib():
    return OC.load_obstacles()


def make(lib, n=24, scheme=0, iters=20):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    h, em, _ = OC.scene(n)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=lib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    s.setProjection(iters, 0.5)
    return s


def flags(lib, boundaries, h, dims):
    from gpufluidsimulation_amd.solver import boundary_array
    ni, nj, nk = dims
    arr, n = boundary_array(boundaries)
    solid = np.zeros(ni * nj * nk, np.uint8)
    rows = np.zeros(nj * nk, np.uint8)
    lib.gpu_obstacle_flags(solid.ctypes.data, rows.ctypes.data, C.addressof(arr), n, h, ni, nj, nk)
    return solid.reshape(nk, nj, ni), rows


@pytest.mark.parametrize("boundaries", [
    [(0, 0.41, 0.1, 0.09, 0.08, 0, 0, 0, 0, 0)],
    [(1, 0.5, 0.05, 0.1, 0.15, 0.04, 0.05, 0, 0, 0)],
    [(0, 0.03, 0.1, 0.09, 0.08, 0, 0, 0, 0, 0), (1, 0.1, 0.1, 0.09, 0.08, 0.03, 0.03, 0, 0, 0)],   # cut by the wall, overlapping
])
def test_flags_match_numpy(lib, boundaries):
    dims = (100, 21, 18)
    h = 1.0 / 100
    solid, rows = flags(lib, boundaries, h, dims)
    want = OC.classify(boundaries, h, (18, 21, 100))
    assert np.array_equal(solid, np.maximum(want, 0).astype(np.uint8))
    assert solid.any()
    # rows summary: (j, k) is marked exactly when a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1
    nk, nj, ni = solid.shape
    pad = np.pad((solid != 0).any(axis=2), 1)
    want_r = np.zeros((nk, nj), bool)
    for c in range(3):
        for b in range(3):
            want_r |= pad[c:c + nk, b:b + nj]
    assert np.array_equal(rows.reshape(nk, nj), want_r.astype(np.uint8))
    assert not want_r.all()


def test_masked_sweep_matches_numpy(lib):
    rng = np.random.default_rng(5)
    ni, nj, nk = 37, 22, 19
    h = 1.0 / ni
    b = [(0, 0.5, 0.3, 0.25, 0.11, 0, 0, 0, 0, 0), (1, 0.2, 0.05, 0.3, 0.1, 0.08, 0.06, 0, 0, 0)]
    solid, rows = flags(lib, b, h, (ni, nj, nk))
    p = rng.standard_normal((nk, nj, ni)).astype(np.float32)
    p[solid != 0] = 0
    div = rng.standard_normal((nk, nj, ni)).astype(np.float32)
    out = p.copy()
    lib.gpu_jacobi_sweep_masked(p.ctypes.data, div.ctypes.data, out.ctypes.data, solid.ctypes.data, rows.ctypes.data,
                                ni, nj, nk, -1.0, float(np.float32(1 / 6)))
    want = OC.masked_sweep(p, div, solid, -1.0, np.float32(1 / 6))
    assert np.array_equal(out, want)


def test_solid_faces_carry_the_obstacle_velocity_and_density_is_cleared(lib):
    for scheme in (0, 3):
        n = 24
        s = make(lib, n, scheme)
        _, _, obstacles = OC.scene(n)
        s.setBoundary(obstacles)
        for f in range(3):
            s.updateBoundary(f, 0.5 / n)
            s.advance(f, 0.5 / n)
        solid = s.solidMask().astype(bool)
        assert solid.sum() > 50
        u = s.field("u").reshape(n, n, n + 1)
        v = s.field("v").reshape(n, n + 1, n)
        rho = s.field("rho").reshape(n, n, n)
        assert np.all(rho[solid] == 0)
        # owner ids as the solver sees them: the flags at the moved centres
        moved = [list(o) for o in obstacles]
        dt = np.float32(0.5 / n)
        for _ in range(3):
            for o in moved:
                o[1] = float(np.float32(o[1]) + np.float32(o[7]) * dt)
        own = np.maximum(OC.classify(moved, 1.0 / n, (n, n, n)), 0)
        assert np.array_equal(own > 0, solid)
        left = np.zeros((n, n, n + 1), np.int32); left[:, :, 1:] = own
        right = np.zeros((n, n, n + 1), np.int32); right[:, :, :n] = own
        ou = np.maximum(left, right)
        for o, ob in enumerate(moved):
            assert np.all(u[ou == o + 1] == np.float32(ob[7])), (scheme, o)
        below = np.zeros((n, n + 1, n), np.int32); below[:, 1:, :] = own
        above = np.zeros((n, n + 1, n), np.int32); above[:, :n, :] = own
        assert np.all(v[np.maximum(below, above) > 0] == 0)
        s.close()


def test_moving_box_advances_by_v_dt_per_update(lib):
    n = 32
    s = make(lib, n)
    box = (1, 0.25, 0.5, 0.5, 0.1, 0.1, 0.1, 0.75, 0.0, 0.0)
    s.setBoundary([box])
    m0 = s.solidMask()
    dt = 1.0 / n / 0.75 * 4                        # four cells per update
    cx = np.float32(box[1])
    for f in range(2):
        s.updateBoundary(f, dt)
        cx = np.float32(cx + np.float32(0.75) * np.float32(dt))
    moved = list(box); moved[1] = float(cx)
    assert np.array_equal(s.solidMask(), (OC.classify([moved], 1.0 / n, (n, n, n)) > 0).astype(np.uint8))
    assert np.array_equal(np.roll(m0, 8, axis=2), s.solidMask())
    s.close()


def test_empty_list_is_no_obstacle_at_all(lib):
    hashes = []
    for call in (False, True):
        n = 20
        s = make(lib, n)
        if call:
            s.setBoundary([OC.scene(n)[2][0]])
            s.setBoundary([])
        digest = hashlib.sha256()
        for f in range(3):
            s.updateBoundary(f, 0.5 / n)
            s.advance(f, 0.5 / n)
            for name in ("rho", "T", "u", "v", "w", "p"):
                digest.update(s.field(name).tobytes())
        assert not s.solidMask().any()
        hashes.append(digest.hexdigest())
        s.close()
    assert hashes[0] == hashes[1]


def test_obstacles_change_the_flow(lib):
    n = 20
    a, b = make(lib, n), make(lib, n)
    b.setBoundary([OC.scene(n)[2][0]])
    for f in range(2):
        a.advance(f, 0.5 / n)
        b.advance(f, 0.5 / n)
    assert not np.array_equal(a.field("v"), b.field("v"))


def test_unsupported_configurations_are_refused(lib):
    from gpufluidsimulation_amd import _lib
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    sphere = [OC.scene(16)[2][0]]
    s = make(lib, 16)
    s.setProjection(5, 0.5, kind=1)
    with pytest.raises(_lib.BimocqError, match="Jacobi"):
        s.setBoundary(sphere)
    s.setProjection(5, 0.5, kind=0)
    s.setBoundary(sphere)
    with pytest.raises(_lib.BimocqError, match="Jacobi"):
        s.setProjection(5, 0.5, kind=1)
    with pytest.raises(_lib.BimocqError):
        s.setBoundary([(2, 0.5, 0.5, 0.5, 0.1, 0, 0, 0, 0, 0)])
    with pytest.raises(_lib.BimocqError):
        s.setBoundary(sphere * 17)
    s.close()
    r = BimocqGPUSolver(16, 16, 16, 1.0, lib=lib, errlib=lib, rank=0, nranks=2, ghost=3)
    with pytest.raises(_lib.BimocqError, match="z-slab"):
        r.setBoundary(sphere)
    r.close()


def test_stand_in_without_obstacle_operators_refuses():
    """the first stand-in has no obstacle operators: the host solver's weak references are null there"""
    from gpufluidsimulation_amd import _lib, solver
    lib = OC.bind_errors(solver.bind_host(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL)))
    s = solver.BimocqGPUSolver(16, 16, 16, 1.0, lib=lib, errlib=lib)
    with pytest.raises(_lib.BimocqError, match="no obstacle operators"):
        s.setBoundary([OC.scene(16)[2][0]])
    s.close()
