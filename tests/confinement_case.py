"""Shared pieces of the vorticity-confinement tests: the loader of the CPU stand-in with
gpu_vorticity_confinement and its call counter, a caller of the operator on host arrays, and a driver that runs the host
solver with a confinement coefficient on any operator library and keeps every step's fields."""
import ctypes as C

import numpy as np

import diag_case as D
import obstacle_case as OC
from build_cpu_confinement import build_confinement

f32 = np.float32
NAMES = ("rho", "T", "u", "v", "w")
FL_OPT_CONFINE_KCHUNK = 24
BAD_ARGUMENT, UNSUPPORTED = 3, 4
# the rising smoke of the example driver: one warm sphere near the floor, emitted at frame 0 only
RISING = [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)]


def load_confinement():
    """the stand-in with every restated operator, gpu_vorticity_confinement among them, and the *_abi_calls counters"""
    from gpufluidsimulation_amd import _lib
    lib = OC._load(build_confinement(), OC.OPS + OC.LS_OPS + ("gpu_emit_sources", "gpu_maccormack", "gpu_flow_stats",
                                                              "gpu_vorticity_confinement"))
    lib.confinement_abi_calls.restype, lib.confinement_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.flow_stats_abi_calls.restype, lib.flow_stats_abi_calls.argtypes = C.c_long, [C.c_int]
    for name in ("fl_set_option", "fl_get_option"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def apply(lib, u, v, w, h, dims, eps, dt, fill=7.0):
    """the restatement on host arrays: (rc, uo, vo, wo); the outputs start as `fill` everywhere (every element must be written)"""
    uo, vo, wo = (np.full(a.size, fill, f32) for a in (u, v, w))
    rc = lib.gpu_vorticity_confinement(uo.ctypes.data, vo.ctypes.data, wo.ctypes.data, u.ctypes.data, v.ctypes.data, w.ctypes.data,
                                       h, *dims, eps, dt)
    return rc, uo, vo, wo


def centred_energy(u, v, w, dims):
    """sum of uc^2 + vc^2 + wc^2 over all cells, in float64"""
    ni, nj, nk = dims
    u = u.astype(np.float64).reshape(nk, nj, ni + 1)
    v = v.astype(np.float64).reshape(nk, nj + 1, ni)
    w = w.astype(np.float64).reshape(nk + 1, nj, ni)
    uc, vc, wc = 0.5 * (u[:, :, :-1] + u[:, :, 1:]), 0.5 * (v[:, :-1, :] + v[:, 1:, :]), 0.5 * (w[:-1] + w[1:])
    return float((uc * uc + vc * vc + wc * wc).sum())


def run(lib, errlib, dims, L, steps, iters, dt, eps=None, scheme=0, blend=1.0, emitters=RISING, obstacles=None, walls=0, diag=False,
        kw=None):
    """the host solver on `lib` for `steps` steps of `dt` with setVorticityConfinement(eps) (None: the setter is never called):
    [{name: field after step f}], and with diag the diagnostics() after the last step as a second value"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    s = BimocqGPUSolver(*dims, L, 0.0, blend, lib=lib, errlib=errlib, scheme=scheme, **(kw or {}))
    try:
        s.setSmoke(0.0, 1.0, [tuple(e) for e in emitters])
        s.setProjection(iters, 0.5)
        if obstacles:
            s.setBoundary(obstacles)
        if walls:
            s.setWalls(walls)
        if eps is not None:
            s.setVorticityConfinement(eps)
            assert s.vorticityConfinement() == float(f32(eps))
        out = []
        for f in range(steps):
            s.advance(f, dt)
            s._check()
            out.append({n: s.field(n) for n in NAMES})
        return (out, s.diagnostics()) if diag else out
    finally:
        s.close()


def same_fields(a, b):
    """the first (step, name) at which two runs differ in value, or None"""
    import fields as F
    for f, (x, y) in enumerate(zip(a, b)):
        for n in NAMES:
            if not F.same(x[n], y[n]):
                return f, n, F.maxdiff(x[n], y[n])
    return None
