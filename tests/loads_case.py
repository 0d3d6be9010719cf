"""Shared pieces of the obstacle-load tests: the loader of the CPU stand-in with gpu_obstacle_loads, an
independent numpy implementation of the per-face terms, the bound the tests hold a summation to, the row formula, and the
scenes and checks the CPU and GPU tests share.

The bound.  The kernel and numpy form bit-identical terms and differ in the order of the additions only.  A sum of m terms
taken in ANY order with one rounding per addition differs from the exact sum by at most (m - 1) u sum|term| + O(u^2),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); math.fsum returns the correctly rounded
exact sum, whose own rounding (u |sum| <= u sum|term|) is the m-th share.  So every raw sum of an obstacle with m wetted faces
must lie within m u sum|term| of math.fsum(terms).  FACES is a sum of ones below 2^53: exact.  Derived, not tuned."""
import ctypes as C
import math

import numpy as np

import obstacle_case as OC
import pcg_case as PC
import pose_case as P
import walls_case as WC
from build_cpu_loads import build_loads

U = 2.0 ** -53
f32, f64 = np.float32, np.float64
NB, NL = 16, 8                                   # BQ_MAX_BOUNDARIES, BQ_LOAD_COUNT
PX, PY, PZ, MX, MY, MZ, FACES, PSUM = range(8)
SUMS = (PX, PY, PZ, MX, MY, MZ, PSUM)
FLAG_WALL = 0x80
VP = C.c_void_p


def load_loads():
    """the stand-in with every restated operator, gpu_obstacle_loads among them, and the obstacle_loads_abi_* helpers"""
    from gpufluidsimulation_amd import _lib
    lib = OC._load(build_loads(), OC.OPS + OC.LS_OPS + PC.PCG_OPS + WC.WALL_OPS + P.POSE_OPS +
                   ("gpu_emit_sources", "gpu_maccormack", "gpu_flow_stats", "gpu_obstacle_loads"))
    lib.obstacle_loads_abi_calls.restype, lib.obstacle_loads_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.obstacle_loads_abi_terms.restype = C.c_long
    lib.obstacle_loads_abi_terms.argtypes = [VP, VP, VP, VP, C.c_int, C.c_float] + [C.c_int] * 3 + [C.c_long, VP, VP, VP]
    lib.obstacle_loads_abi_log.restype, lib.obstacle_loads_abi_log.argtypes = C.c_size_t, [C.c_int] + [VP] * 5
    for name in ("fl_memcpy_d2h", "fl_memcpy_h2d"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def centre_list(centres):
    """a bq_boundary array whose centres are `centres` (rows of three floats), the only thing the operator reads"""
    from gpufluidsimulation_amd.solver import boundary_array
    return boundary_array([(0, float(c[0]), float(c[1]), float(c[2]), 1.0, 0.0, 0.0, 0.0, 0.0, 0.0) for c in centres])


# ---- the terms, in numpy -------------------------------------------------------------------------------------------------
def np_terms(p, solid, centres, n, h):
    """every wetted face of the flags `solid` (nk, nj, ni) uint8 with the pressure p (nk, nj, ni), float32 or float64:
    (owner (m,), axis (m,), terms (m, 8) float64, F (m,) flat index of the fluid cell), in the order of the plain triple loop
    over the obstacle cells (k, j, i; then -x, +x, -y, +y, -z, +z).  Every numpy operation below is one IEEE operation."""
    nk, nj, ni = solid.shape
    h = float(f32(h))
    ctr = np.asarray(centres, f32).astype(f64).reshape(-1, 3)
    own = (solid & 0x7f).astype(np.int64)
    obst = (own >= 1) & (own <= n)
    fluid = solid == 0
    K, J, I = np.indices(solid.shape)
    flat = (I + ni * (J + nj * K)).astype(np.int64)
    recs = []
    for a, ax in ((0, 2), (1, 1), (2, 0)):
        for di, d in enumerate((-1, 1)):
            sS, sF = [slice(None)] * 3, [slice(None)] * 3
            sS[ax], sF[ax] = (slice(0, -1), slice(1, None)) if d > 0 else (slice(1, None), slice(0, -1))
            sS, sF = tuple(sS), tuple(sF)
            wet = obst[sS] & fluid[sF]
            o = own[sS][wet] - 1
            pf = p[sF][wet].astype(f64)
            idx = [I[sS][wet], J[sS][wet], K[sS][wet]]
            f = f64(-d) * pf
            x = [idx[c].astype(f64) * h for c in range(3)]
            x[a] = ((2 * idx[a] + d).astype(f64) * 0.5) * h
            r = [x[c] - ctr[o, c] for c in range(3)]
            t = np.zeros((len(o), NL), f64)
            t[:, PX + a] = f
            t[:, MX + (a + 1) % 3] = r[(a + 2) % 3] * f
            t[:, MX + (a + 2) % 3] = -(r[(a + 1) % 3] * f)
            t[:, FACES] = 1.0
            t[:, PSUM] = pf
            recs.append((flat[sS][wet] * 6 + 2 * a + di, o, np.full(len(o), a), t, flat[sF][wet]))
    key = np.concatenate([r[0] for r in recs])
    order = np.argsort(key, kind="stable")
    return (np.concatenate([r[1] for r in recs])[order], np.concatenate([r[2] for r in recs])[order],
            np.concatenate([r[3] for r in recs])[order], np.concatenate([r[4] for r in recs])[order])


def sequential(owner, terms):
    """(16, 8): the terms added one after the other in their order, per owner -- the restatement's own sums, bit for bit"""
    out = np.zeros((NB, NL), f64)
    for o in range(NB):
        t = terms[owner == o]
        if len(t):
            out[o] = np.cumsum(t, axis=0)[-1]          # (accumulate adds sequentially, one rounding per addition)
    return out


def exact(owner, terms):
    """(value (16, 8): math.fsum per obstacle and column, mass (16, 8): fsum of |term|, faces (16,))"""
    val, mass, faces = np.zeros((NB, NL), f64), np.zeros((NB, NL), f64), np.zeros(NB, np.int64)
    for o in range(NB):
        t = terms[owner == o]
        faces[o] = len(t)
        for c in range(NL):
            val[o, c] = math.fsum(t[:, c].tolist())
            mass[o, c] = math.fsum(np.abs(t[:, c]).tolist())
    return val, mass, faces


def assert_within_bound(got, owner, terms, n, what=""):
    """got (16, 8) against the terms: FACES equal, every other sum of obstacle o within faces[o] u sum|term| of the exact sum,
    rows o >= n zero.  Prints each figure before it asserts."""
    val, mass, faces = exact(owner, terms)
    got = np.asarray(got, f64).reshape(NB, NL)
    assert not got[n:].any(), (what, got[n:])
    assert not (owner >= n).any()
    for o in range(n):
        assert got[o, FACES] == faces[o], (what, o, got[o, FACES], faces[o])
        for c in SUMS:
            err, bound = abs(got[o, c] - val[o, c]), faces[o] * U * mass[o, c]
            print(f"{what} obstacle {o} column {c}: |got - exact| = {err:.3e}, bound = {bound:.3e}, faces = {faces[o]}")
            assert err <= bound, (what, o, c, got[o, c], val[o, c], err, bound)


# ---- the operator on host arrays (the stand-in) ------------------------------------------------------------------------
def abi_loads(lib, p, solid, rows, centres, n, h, out=None):
    """gpu_obstacle_loads of the stand-in on host arrays: (rc, (16, 8) float64); p float32 or float64 (nk, nj, ni)"""
    nk, nj, ni = solid.shape
    arr, _ = centre_list(centres)
    out = np.full((NB, NL), -7.0, f64) if out is None else out
    p = np.ascontiguousarray(p)
    solid = np.ascontiguousarray(solid)
    p32, p64 = (p.ctypes.data, None) if p.dtype == f32 else (None, p.ctypes.data)
    rc = lib.gpu_obstacle_loads(p32, p64, solid.ctypes.data, None if rows is None else rows.ctypes.data, C.addressof(arr), n,
                                h, ni, nj, nk, out.ctypes.data)
    return rc, out


def abi_terms(lib, p, solid, centres, n, h):
    """the restatement's per-face terms: (owner, axis, terms (m, 8))"""
    nk, nj, ni = solid.shape
    arr, _ = centre_list(centres)
    p = np.ascontiguousarray(p)
    solid = np.ascontiguousarray(solid)
    p32, p64 = (p.ctypes.data, None) if p.dtype == f32 else (None, p.ctypes.data)
    m = lib.obstacle_loads_abi_terms(p32, p64, solid.ctypes.data, C.addressof(arr), n, h, ni, nj, nk, 0, None, None, None)
    owner, axis, terms = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, NL), f64)
    lib.obstacle_loads_abi_terms(p32, p64, solid.ctypes.data, C.addressof(arr), n, h, ni, nj, nk, m, owner.ctypes.data,
                                 axis.ctypes.data, terms.ctypes.data)
    return owner, axis, terms


def abi_log(lib, back):
    """the call `back` calls before the stand-in's newest: dict(ptr, is64, n, p (nk, nj, ni) float64, solid, out (16, 8),
    centres (16, 3)) or None"""
    meta = (C.c_int * 5)()
    if not lib.obstacle_loads_abi_log(back, meta, None, None, None, None):
        return None
    is64, n, ni, nj, nk = list(meta)
    p, solid = np.zeros((nk, nj, ni), f64), np.zeros((nk, nj, ni), np.uint8)
    out, ctr = np.zeros((NB, NL), f64), np.zeros((NB, 3), f64)
    ptr = lib.obstacle_loads_abi_log(back, meta, p.ctypes.data, solid.ctypes.data, out.ctypes.data, ctr.ctypes.data)
    return {"ptr": ptr, "is64": bool(is64), "n": n, "p": p, "solid": solid, "out": out, "centres": ctr}


# ---- flags ---------------------------------------------------------------------------------------------------------------
def random_flags(dims, seed, n=16, density=0.3):
    """(nk, nj, ni) uint8: each cell solid with probability `density`, owner uniform in 1..n; BQ_FLAG_WALL sprinkled on border
    cells, alone and on top of owners"""
    ni, nj, nk = dims
    rng = np.random.default_rng(seed)
    solid = np.where(rng.random((nk, nj, ni)) < density, rng.integers(1, n + 1, (nk, nj, ni)), 0).astype(np.uint8)
    border = np.ones((nk, nj, ni), bool)
    border[1:-1, 1:-1, 1:-1] = False
    wall = border & (rng.random((nk, nj, ni)) < 0.5)
    return np.where(wall, solid | FLAG_WALL, solid).astype(np.uint8)


def box_flags(dims, lo, size, owner=1):
    """a solid box of size = (Nx, Ny, Nz) cells whose lowest cell is lo = (i, j, k), in fluid"""
    ni, nj, nk = dims
    solid = np.zeros((nk, nj, ni), np.uint8)
    solid[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = owner
    return solid


def linear_pressure(dims, coef):
    """p = a i + b j + c k + d as float32 (nk, nj, ni): small integers, exact"""
    ni, nj, nk = dims
    K, J, I = np.indices((nk, nj, ni))
    a, b, c, d = coef
    return (a * I + b * J + c * K + d).astype(f32)


def linear_box_answer(size, coef):
    """(P (3,), FACES) of the box under the linear pressure: the two faces across the box along x see p differ by a (Nx + 1),
    the outward face on the high side counting negative"""
    Nx, Ny, Nz = size
    a, b, c, _ = coef
    return (-(a * (Nx + 1) * Ny * Nz), -(b * (Ny + 1) * Nx * Nz), -(c * (Nz + 1) * Nx * Ny)), 2 * (Nx * Ny + Ny * Nz + Nz * Nx)


def wall_flags(mask, walls):
    """solidw of gpu_wall_flags for flags whose obstacles do not touch the border: BQ_FLAG_WALL on the border cells of the
    closed sides"""
    from gpufluidsimulation_amd import solver as S
    out = mask.copy()
    for bit, sl in ((S.WALL_XLO, (slice(None), slice(None), 0)), (S.WALL_XHI, (slice(None), slice(None), -1)),
                    (S.WALL_YLO, (slice(None), 0, slice(None))), (S.WALL_YHI, (slice(None), -1, slice(None))),
                    (S.WALL_ZLO, (0, slice(None), slice(None))), (S.WALL_ZHI, (-1, slice(None), slice(None)))):
        if walls & bit:
            assert not mask[sl].any()
            out[sl] = FLAG_WALL
    return out


# ---- the row a caller sees -----------------------------------------------------------------------------------------------
def row_from_raw(raw, halfrdx, h, dt, n):
    """bq_solver_obstacle_loads' row from obstacleLoadsRaw()'s dict, operation for operation: dict(force, torque, area, p_mean)"""
    s0, s1 = raw["slots"][0], raw["slots"][1]
    w0, w1 = raw["weights"]
    halfrdx, h, dt = float(f32(halfrdx)), float(f32(h)), float(f32(dt))
    last = s1 if w1 != 0.0 else s0
    out = {"force": np.zeros((n, 3)), "torque": np.zeros((n, 3)), "area": np.zeros(n), "p_mean": np.zeros(n)}
    kf = halfrdx * (h * h * h) / dt if dt != 0.0 else 0.0
    kp = halfrdx * h / dt if dt != 0.0 else 0.0
    for o in range(n):
        for a in range(3):
            out["force"][o, a] = kf * (w0 * s0[o, PX + a] + w1 * s1[o, PX + a]) if dt != 0.0 else 0.0
            out["torque"][o, a] = kf * (w0 * s0[o, MX + a] + w1 * s1[o, MX + a]) if dt != 0.0 else 0.0
        out["area"][o] = (h * h) * last[o, FACES]
        out["p_mean"][o] = kp * last[o, PSUM] / last[o, FACES] if dt != 0.0 and last[o, FACES] != 0.0 else 0.0
    return out


def assert_row_is_formula(s, halfrdx, dt):
    """obstacleLoads() equals row_from_raw(obstacleLoadsRaw()) bit for bit"""
    row, raw = s.obstacleLoads(), s.obstacleLoadsRaw()
    n = len(row["area"])
    want = row_from_raw(raw, halfrdx, s.h, dt, n)
    assert row["step"] == raw["step"] and row["dt"] == float(f32(dt))
    for k in ("force", "torque", "area", "p_mean"):
        assert row[k].view(np.uint64).tolist() == want[k].view(np.uint64).tolist(), (k, row[k], want[k])
    return row, raw


# ---- the solver scene ----------------------------------------------------------------------------------------------------
SPLIT_X = 0.45          # the sphere stays at x < SPLIT_X, the box at x > SPLIT_X: a cell's owner follows from its column
KINDS = {"jacobi": (0, 24, 0.5), "pcg": (2, 1000, 1.0)}          # projection kind, iterations, halfrdx


def scene():
    """rising smoke between a sphere moving along +x (obstacle 0) and a tilted box spinning about z (obstacle 1), on a grid of
    side 1 along x, 0.75 along y and 0.625 along z"""
    from gpufluidsimulation_amd.solver import Rotating
    em = [(0.45, 0.2, 0.3125, 0.1, 1.0, 1.0, 0.0, 1000)]
    entries = [(0, 0.25, 0.375, 0.3125, 0.09, 0.0, 0.0, 0.3, 0.0, 0.0),
               Rotating((1, 0.68, 0.375, 0.3125, 0.12, 0.05, 0.1, 0.0, 0.0, 0.0), spin=(0.0, 0.0, 2.0), orientation=(0.9, 0.1, 0.2, 0.3))]
    return em, entries


FIELDS = ("rho", "T", "u", "v", "w", "p")


def run_scene(lib, errlib, dims, scheme, kind, every, walls=0, steps=3):
    """`steps` steps of the scene (updateBoundary before every advance) with BQ_OPT_OBSTACLE_LOADS = every: the solver (the
    caller closes it) and the per-step fields (FIELDS, the flags, and the fp64 pressure for PCG)"""
    from gpufluidsimulation_amd import solver
    ni, nj, nk = dims
    dt = 1.0 / ni
    k, iters, halfrdx = KINDS[kind]
    em, entries = scene()
    s = solver.BimocqGPUSolver(ni, nj, nk, 1.0, 0.0, 1.0, lib=lib, errlib=errlib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    s.setProjection(iters, halfrdx, kind=k)
    s.setBoundary(entries)
    if walls:
        s.setWalls(walls)
    if every:
        s.setOption(solver.OPT_OBSTACLE_LOADS, every)
    out = []
    for f in range(steps):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
        s._check()
        rec = {name: s.field(name) for name in FIELDS}
        rec["solid"] = s.solidMask()
        if k == 2:
            rec["p64"] = s.pcgPressure()
        out.append(rec)
    return s, out, halfrdx, dt


def owner_flags(s, walls=0):
    """the flags the last projection used, rebuilt from what the solver lets a caller download: solidMask() (0 / 1), the owner
    from the cell's column (SPLIT_X), the wall cells from the closed sides"""
    mask = s.solidMask()
    i = np.arange(s.nx)[None, None, :]
    owned = np.where(mask != 0, np.where(i * s.h < SPLIT_X, 1, 2), 0).astype(np.uint8)
    assert (owned == 1).any() and (owned == 2).any()
    return wall_flags(owned, walls) if walls else owned


def solver_centres(s):
    return np.array([pose[0] for pose in s.boundaryPoses()], f64)


def final_pressure(s, rec, kind):
    nk, nj, ni = s.nk_local, s.ny, s.nx
    return rec["p64"] if KINDS[kind][0] == 2 else rec["p"].reshape(nk, nj, ni)


def assert_fields_equal(a, b):
    for ra, rb in zip(a, b):
        for name in ra:
            assert np.array_equal(ra[name].view(np.uint8), rb[name].view(np.uint8)), name


# ---- physics ---------------------------------------------------------------------------------------------------------------
PADDLE_N = 32
ADDED_MASS_N, ADDED_MASS_R, ADDED_MASS_U = 32, 5.0, 0.5
# F_x dt / (-1/2 V u) of check_added_mass measured on the CPU stand-in; the tests hold the ratio within
# +-20 % of it: a physics sanity band against finite-domain and voxelisation effects, not parity
ADDED_MASS_RATIO = 1.062


def check_spinning_box_resists(lib, errlib):
    """from rest, scenes.paddle turning about +z, PCG with halfrdx = 1: after the first step the fluid's pressure torque on the
    shaft opposes the spin"""
    from gpufluidsimulation_amd import scenes, solver
    n = PADDLE_N
    s = solver.BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=errlib)
    try:
        s.setSmoke(0.0, 1.0, [])
        s.setProjection(1000, 1.0, kind=2)
        s.setBoundary(scenes.paddle(n, 1.0, spin=2.0))
        s.setOption(solver.OPT_OBSTACLE_LOADS, 1)
        s.updateBoundary(0, 1.0 / n)
        s.advance(0, 1.0 / n)
        s._check()
        row = s.obstacleLoads()
    finally:
        s.close()
    print("paddle torque", row["torque"], "force", row["force"], "area", row["area"])
    assert row["step"] == 1 and row["torque"].shape == (1, 3)
    assert row["torque"][0, 2] < 0.0 and row["area"][0] > 0.0
    return row


def added_mass_ratio(lib, errlib):
    """a sphere of radius 5 cells at the centre of a 32^3 grid set moving with (u, 0, 0) in still fluid, PCG with halfrdx = 1,
    one step: F_x dt over the added-mass impulse -1/2 V u, V the voxelised volume"""
    from gpufluidsimulation_amd import solver
    n, u = ADDED_MASS_N, ADDED_MASS_U
    h = 1.0 / n
    s = solver.BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=errlib)
    try:
        s.setSmoke(0.0, 1.0, [])
        s.setProjection(1000, 1.0, kind=2)
        s.setBoundary([(0, 0.5, 0.5, 0.5, ADDED_MASS_R * h, 0.0, 0.0, u, 0.0, 0.0)])
        s.setOption(solver.OPT_OBSTACLE_LOADS, 1)
        s.advance(0, h)
        s._check()
        row = s.obstacleLoads()
        cells = int(s.solidMask().sum())
    finally:
        s.close()
    impulse = row["force"][0, 0] * row["dt"]
    ratio = impulse / (-0.5 * (h ** 3 * cells) * u)
    print(f"added mass: impulse {impulse:.6e}, solid cells {cells}, ratio {ratio:.4f}")
    assert impulse < 0.0
    return ratio


def check_added_mass(lib, errlib):
    ratio = added_mass_ratio(lib, errlib)
    assert abs(ratio - ADDED_MASS_RATIO) <= 0.2 * ADDED_MASS_RATIO, (ratio, ADDED_MASS_RATIO)
    return ratio
