"""BQ_PROJECTION_PCG on the CPU stand-in (tests/cpu_abi/pcg_abi.c linked with the product's host sources; DESIGN.md
section 15): the solve meets its stopping rule on the masked system recomputed from tests/obstacle_ref.py, agrees with a
sparse direct solve, the refusals, and the divergence after a step with halfrdx = 1.  No GPU."""

import numpy as np
import pytest

import obstacle_case as OC
import obstacle_ref as R
import pcg_case as P
from build_cpu_host import build_levelsets

UD = 2.0 ** -53                 # float64 unit roundoff


@pytest.fixture(scope="module")
def lib():
    return P.load_pcg()


def masks(dims):
    fams = [("no mask", None)] + R.mask_families(dims) + [("random 2", R.random_mask(dims, 2, frac=0.08))]
    return fams


def rhs(dims, seed):
    ni, nj, nk = dims
    return np.random.default_rng(seed).standard_normal((nk, nj, ni))


def drift_bound(p, b, iters):
    """bound on |(b - A p) - r| after `iters` updates of the recursive residual r: each update rounds p + alpha d (at most
    UD |p| per entry, moved by A, whose rows sum |.| to at most 12) and r - alpha q, where alpha q = A(alpha d) is itself
    a 7-term fp64 sum (6 UD of its terms); with |alpha d| <= 2 max|p| per update (the iterates approach p monotonically in
    the energy norm, not in max; factor 2 covers the overshoot seen in practice) one update adds at most
    UD (12 + 2 * 12 * 7) max|p| + 2 UD max|b|"""
    return max(iters, 1) * UD * ((12 + 2 * 12 * 7) * float(np.abs(p).max()) + 2 * float(np.abs(b).max()))


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
@pytest.mark.parametrize("dims", [(20, 14, 12), (16, 16, 16)])
def test_solve_meets_the_stopping_rule(lib, dims, tol):
    for name, solid in masks(dims):
        div = rhs(dims, hash(name) % 1000)
        p, st = P.solve(lib, div, solid, 1000, tol)
        assert lib.fl_last_error() == 0, (name, lib.fl_last_error_string())
        it, maxr, maxb, stop = st
        true_r, true_b, A, b, unk = P.true_residual(div, solid, p)
        assert P.STOP[int(stop)] == "converged", (name, st)
        assert 0 < it < 1000
        assert maxb == true_b
        assert maxr <= tol * maxb
        drift = drift_bound(p, b, it)
        assert abs(true_r - maxr) <= drift, (name, true_r, maxr, drift)
        assert true_r <= tol * maxb + drift, (name, true_r, tol * maxb, drift)
        assert np.all(p[~unk] == 0)


def test_solve_matches_a_direct_solve(lib):
    """on grids small enough for a dense inverse: |p - A^-1 b| <= ||A^-1||_inf max|b - A p| (+ spsolve's own rounding)"""
    import scipy.sparse.linalg as sla
    dims = (12, 10, 9)
    for name, solid in masks(dims):
        div = rhs(dims, 7)
        p, st = P.solve(lib, div, solid, 1000, 1e-10)
        true_r, _, A, b, unk = P.true_residual(div, solid, p)
        xs = sla.spsolve(A.tocsc(), b)
        ainv = np.linalg.inv(A.toarray())
        bound = np.abs(ainv).sum(axis=1).max() * true_r
        err = float(np.abs(p[unk] - xs).max())
        assert err <= bound * (1 + 1e-6) + 1e-12 * float(np.abs(xs).max()), (name, err, bound)


def test_zero_rhs_and_iteration_limit(lib):
    dims = (14, 12, 10)
    p, st = P.solve(lib, np.zeros((10, 12, 14)), None, 50, 1e-6)
    assert st == [0, 0.0, 0.0, 0] and not p.any()
    p, st = P.solve(lib, rhs(dims, 3), R.random_mask(dims, 1), 2, 1e-12)
    assert st[0] == 2 and P.STOP[int(st[3])] == "iteration limit" and np.isfinite(p).all()


def make(lib, n=16, scheme=0):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    _, em, _ = OC.scene(n)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=lib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    return s


def test_refusals(lib):
    from gpufluidsimulation_amd import _lib
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    r = BimocqGPUSolver(16, 16, 16, 1.0, lib=lib, errlib=lib, rank=0, nranks=2, ghost=3)
    with pytest.raises(_lib.BimocqError, match="z-slab"):
        r.setProjection(100, 0.5, kind=2)
    r.close()
    s = make(lib)
    for tol in (0.0, 1.0, -1e-6, 2.0, float("nan"), float("inf")):
        with pytest.raises(_lib.BimocqError, match="tol"):
            s.setPcgTolerance(tol)
    s.setPcgTolerance(1e-8)
    with pytest.raises(_lib.BimocqError, match="iters"):
        s.setProjection(-1, 0.5, kind=2)
    s.close()


def test_stand_in_without_pcg_operators_refuses():
    from gpufluidsimulation_amd import _lib
    lib = OC.load_levelsets()
    assert lib._name == build_levelsets()
    s = make(lib)
    with pytest.raises(_lib.BimocqError, match="no PCG operators") as e:
        s.setProjection(100, 0.5, kind=2)
    assert "bimocq error 4" in str(e.value)             # FL_ERR_UNSUPPORTED
    s.close()


def test_obstacles_are_admitted_in_either_order(lib):
    from gpufluidsimulation_amd import _lib
    sphere = [OC.scene(16)[2][0]]
    a = make(lib)
    a.setProjection(100, 0.5, kind=2)
    a.setBoundary(sphere)
    b = make(lib)
    b.setBoundary(sphere)
    b.setProjection(100, 0.5, kind=2)
    for s in (a, b):
        s.advance(0, 1.0 / 16)
        st = s.pcgStats()
        assert st["stop"] == "converged" and st["projections"] == 1 and st["unconverged"] == 0
        with pytest.raises(_lib.BimocqError, match="Jacobi"):
            s.setProjection(5, 0.5, kind=1)                 # kind 1 keeps its refusal
    assert np.array_equal(a.field("u"), b.field("u")) and np.array_equal(a.pcgPressure(), b.pcgPressure())
    a.close()
    b.close()


@pytest.mark.parametrize("scheme", [0, 3])
def test_one_step_of_the_mixed_scene_is_divergence_free(lib, scheme):
    n = 24
    _, em, entries = P.mixed_scene(n)
    s = make(lib, n, scheme)
    s.setProjection(1000, 1.0, kind=2)
    s.setBoundary(entries)
    s.updateBoundary(0, 1.0 / n)
    s.advance(0, 1.0 / n)
    assert s.solidMask().any()
    P.divergence_check(s, n)
    s.close()
