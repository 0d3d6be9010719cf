"""Shared pieces of the PCG projection tests: the stand-in with the PCG operators, one call of
gpu_pcg_solve on host (stand-in) or device (HIP) arrays, the recomputed residual of the masked system, and the mixed
obstacle + level-set scene."""
import ctypes as C

import numpy as np

import obstacle_case as OC
import obstacle_ref as R
from build_cpu_pcg import build_pcg
from oracle_lib import CoarseLevel

PCG_OPS = ("gpu_divergence_double", "gpu_pcg_solve", "gpu_pcg_gradient")
U, UD = 2.0 ** -24, 2.0 ** -53     # float32, float64 unit roundoff
STOP = {0: "converged", 1: "iteration limit", 2: "breakdown"}


def load_pcg():
    """the stand-in with the obstacle, level-set and PCG operators"""
    return OC._load(build_pcg(), OC.OPS + OC.LS_OPS + PCG_OPS)


def level_dims(dims):
    """the pyramid n -> (n - 1) / 2 of allocMgcg, levels without a cell left out"""
    out, (ni, nj, nk) = [], dims
    for lev in range(6):
        if lev:
            ni, nj, nk = (ni - 1) // 2, (nj - 1) // 2, (nk - 1) // 2
        if min(ni, nj, nk) < 1:
            break
        out.append((ni, nj, nk))
    return out


ARRAYS = ("p", "r", "d", "q", "z", "t", "work")


def solve(lib, div, solid, iters, tol, fill=0.0, dev=None):
    """gpu_pcg_solve on (nk, nj, ni) float64 `div` and uint8 `solid` (None: no obstacles); every work array pre-filled with
    `fill`.  dev: an obstacle_case.Dev to run on device buffers (HIP library), else host arrays (stand-in).
    Returns (p, stats)."""
    nk, nj, ni = div.shape
    n = div.size
    levels = (CoarseLevel * 6)()
    keep = {}

    def buf(name, count, dtype=np.float64, value=None):
        a = np.full(count, fill if value is None else value, dtype)
        if dev is not None:
            return dev.put(name, a)
        keep[name] = a
        return a.ctypes.data

    ptr = {name: buf(name, n) for name in ARRAYS}
    ptr["div"] = buf("div", n, value=0) if dev is None else dev.put("div", np.ascontiguousarray(div, np.float64))
    if dev is None:
        keep["div"][:] = div.ravel()
    sol = None
    if solid is not None:
        sol = dev.put("solid", np.ascontiguousarray(solid, np.uint8)) if dev is not None else None
        if dev is None:
            keep["solid"] = np.ascontiguousarray(solid, np.uint8).ravel()
            sol = keep["solid"].ctypes.data
    dims = level_dims((ni, nj, nk))
    for lev, (a, b, c) in enumerate(dims):
        L = levels[lev]
        L.ni, L.nj, L.nk, L.number, L.alpha, L.beta = a, b, c, a * b * c, -1.0, 1.0 / 6.0
        if lev:
            L.b, L.x, L.r = (buf(f"{k}{lev}", a * b * c) for k in "bxr")
    stats = (C.c_double * 4)()
    lib.gpu_pcg_solve(ptr["div"], ptr["p"], sol, ptr["r"], ptr["d"], ptr["q"], ptr["z"], ptr["t"], ptr["work"], levels,
                      len(dims), iters, tol, stats)
    p = dev.get("p") if dev is not None else keep["p"].copy()
    return p.reshape(nk, nj, ni), list(stats)


def unknowns(solid, shape):
    """interior cells that are fluid with fewer than 6 solid neighbours"""
    s = np.zeros(shape, bool) if solid is None else solid != 0
    unk = np.zeros(shape, bool)
    unk[1:-1, 1:-1, 1:-1] = ~s[1:-1, 1:-1, 1:-1] & (R.neighbour_count(s.astype(np.uint8)) < 6)
    return unk


def true_residual(div, solid, p):
    """(max|b - A p| over the unknowns, max|b|, A, b, unknown mask) recomputed from obstacle_ref.neumann_system"""
    sol = np.zeros(div.shape, np.uint8) if solid is None else np.asarray(solid, np.uint8)
    unk = unknowns(solid, div.shape)
    # obstacle_ref's system also lists fluid cells with s = 6 (a zero row): hold them at 0 by marking them solid
    sealed = (sol == 0) & ~unk
    sealed[0], sealed[-1], sealed[:, 0], sealed[:, -1], sealed[:, :, 0], sealed[:, :, -1] = 0, 0, 0, 0, 0, 0
    A, b, mask = R.neumann_system(div, np.where(sealed, 0, sol), alpha=-1.0)
    keep = unk[mask]
    A = A[keep][:, keep]
    b = b[keep]
    x = p[unk]
    res = b - A @ x
    return float(np.abs(res).max()) if res.size else 0.0, float(np.abs(b).max()) if b.size else 0.0, A, b, unk


def mixed_scene(n):
    """obstacle_case.scene's sphere and moving box plus levelset_case.scene's level sets and box"""
    import levelset_case as LC
    h, em, ob = OC.scene(n)
    return h, em, list(ob) + list(LC.scene(n)[2])


def hollow_box(dims, lo, hi):
    """solid walls of the box [lo, hi] (cell indices, inclusive): a sealed fluid pocket inside"""
    ni, nj, nk = dims
    s = np.zeros((nk, nj, ni), np.uint8)
    (i0, j0, k0), (i1, j1, k1) = lo, hi
    s[k0:k1 + 1, j0:j1 + 1, i0:i1 + 1] = 1
    s[k0 + 1:k1, j0 + 1:j1, i0 + 1:i1] = 0
    return s


def run_mixed(lib, errlib, n, scheme, steps, halfrdx=0.5, iters=1000):
    """`steps` steps of mixed_scene with the kind-2 projection (updateBoundary before every advance): per-step SHA-256 of
    rho, T, u, v, w, p, the flags and pcgPressure(), and every step's pcgStats()"""
    import hashlib
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    _, em, entries = mixed_scene(n)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=errlib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    s.setProjection(iters, halfrdx, kind=2)
    s.setBoundary(entries)
    hashes, stats = [], []
    for f in range(steps):
        s.updateBoundary(f, 1.0 / n)
        s.advance(f, 1.0 / n)
        d = hashlib.sha256()
        for name in ("rho", "T", "u", "v", "w", "p"):
            d.update(s.field(name).tobytes())
        d.update(s.solidMask().tobytes())
        d.update(s.pcgPressure().tobytes())
        hashes.append(d.hexdigest())
        stats.append(s.pcgStats())
    rho_max = float(s.field("rho").max())
    s.close()
    return {"hashes": hashes, "stats": stats, "rho_max": rho_max}


def divergence_check(s, n):
    """at fluid cells whose six faces lie in the gradient window: |div(u)| <= max|r| + the float32 rounding of the face
    updates.  With halfrdx = 1 the exact update leaves div = -r there.  Each updated face value is
    fl(u - fl(g)) with g = p_c - p_left: at most U (|g| + |u_new|) away from u - g, and the fp64 divergence adds its six
    face errors; the divergence of the stored velocity is exact in fp64 up to UD times the sum of |face|."""
    st = s.pcgStats()
    p = s.pcgPressure()
    u, v, w = (s.field(c).reshape(sh) for c, sh in (("u", (n, n, n + 1)), ("v", (n, n + 1, n)), ("w", (n + 1, n, n))))
    sol = s.solidMask()
    du, dv, dw = u[:, :, 1:] - u[:, :, :-1].astype(np.float64), v[:, 1:, :] - v[:, :-1, :].astype(np.float64), w[1:] - w[:-1].astype(np.float64)
    div = du.astype(np.float64) + dv + dw
    gx = np.zeros_like(u, dtype=np.float64); gx[:, :, 1:n] = np.abs(p[:, :, 1:] - p[:, :, :-1])
    gy = np.zeros_like(v, dtype=np.float64); gy[:, 1:n, :] = np.abs(p[:, 1:, :] - p[:, :-1, :])
    gz = np.zeros_like(w, dtype=np.float64); gz[1:n] = np.abs(p[1:] - p[:-1])
    fx, fy, fz = (np.abs(a).astype(np.float64) for a in (u, v, w))
    face = lambda g, f: U * (g + f)
    bound = (face(gx, fx)[:, :, 1:] + face(gx, fx)[:, :, :-1] + face(gy, fy)[:, 1:, :] + face(gy, fy)[:, :-1, :]
             + face(gz, fz)[1:] + face(gz, fz)[:-1]) + UD * 8 * (fx[:, :, 1:] + fx[:, :, :-1] + fy[:, 1:] + fy[:, :-1] + fz[1:] + fz[:-1])
    # unknowns whose six faces are in the window [2, n): 2 <= i <= n - 2 on every axis (next to a solid cell too: the
    # face it shares keeps the obstacle velocity, which the diagonal 6 - s accounts for)
    win = np.zeros((n, n, n), bool)
    win[2:n - 1, 2:n - 1, 2:n - 1] = True
    cells = win & unknowns(sol, sol.shape)
    nbs = np.zeros(sol.shape, np.int32)
    nbs[1:-1, 1:-1, 1:-1] = R.neighbour_count(sol)
    assert cells.sum() > 100 and (cells & (nbs > 0)).any()
    assert st["stop"] == "converged"
    excess = np.abs(div[cells]) - (st["max_r"] + bound[cells])
    assert excess.max() <= 0, (float(excess.max()), st)
    return float(np.abs(div[cells]).max())
