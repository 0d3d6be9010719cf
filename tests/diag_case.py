"""Shared pieces of the flow-diagnostics tests: the loader of the CPU stand-in with gpu_flow_stats,
the exact sums of the restatement's per-cell terms, and the error bounds the tests hold a summation to.

The bound.  A sum of n terms taken in ANY order with one rounding per addition (recursive, pairwise, per-thread partials
combined by a tree: all of them) differs from the exact sum by at most (n - 1) u sum|term| + O(u^2), u = 2^-53 (Higham,
Accuracy and Stability of Numerical Algorithms, section 4.2).  The kernels and the restatement form bit-identical terms
and differ in the order only, so every raw sum must lie within n u sum|term| of math.fsum(terms), the correctly rounded
exact sum (whose own rounding, u |sum| <= u sum|term|, is the n-th share).  Derived, not tuned."""
import ctypes as C
import math

import numpy as np

import maccormack_case as MC
import obstacle_case as OC
from build_cpu_diag import build_diag

U = 2.0 ** -53
STAT = {"e2": 0, "m2": 1, "d2": 2, "div_max": 3, "rho": 4, "rho_i": 5, "rho_j": 6, "rho_k": 7, "T": 8, "vort_max": 9}
SUMS = ("e2", "m2", "d2", "rho", "rho_i", "rho_j", "rho_k", "T")
FP, DP, VP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p


def load_diag():
    """the stand-in with every restated operator, gpu_flow_stats among them, and the flow_stats_abi_* helpers"""
    from gpufluidsimulation_amd import _lib
    lib = OC._load(build_diag(), OC.OPS + OC.LS_OPS + ("gpu_emit_sources", "gpu_maccormack", "gpu_flow_stats"))
    lib.flow_stats_abi_calls.restype, lib.flow_stats_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.maccormack_abi_calls.restype, lib.maccormack_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.flow_stats_abi_set_slab.restype, lib.flow_stats_abi_set_slab.argtypes = None, [C.c_int] * 4
    lib.flow_stats_abi_set_allreduce.restype, lib.flow_stats_abi_set_allreduce.argtypes = None, [VP, C.c_int]
    lib.flow_stats_abi_terms.restype = None
    lib.flow_stats_abi_terms.argtypes = [VP, VP, VP, C.c_float] + [C.c_int] * 5 + [VP] * 4
    for name in ("fl_set_option", "fl_get_option", "fl_memcpy_d2h", "fl_memcpy_h2d"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def terms(lib, u, v, w, h, dims, koff=0, nkg=0):
    """the restatement's per-cell terms of a local buffer: e2, m2 (float64), d, mag (float32), flat, x fastest"""
    ni, nj, nk = dims
    n = ni * nj * nk
    e2, m2 = np.zeros(n, np.float64), np.zeros(n, np.float64)
    d, mag = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib.flow_stats_abi_terms(u.ctypes.data, v.ctypes.data, w.ctypes.data, h, ni, nj, nk, koff, nkg,
                             e2.ctypes.data, m2.ctypes.data, d.ctypes.data, mag.ctypes.data)
    return e2, m2, d, mag


def exact(lib, u, v, w, rho, T, h, dims):
    """one domain: ({stat: exact value}, {stat: sum |term|}, cells, mag) -- sums by math.fsum over the restatement's terms,
    maxima with NaNs skipped as fmaxf skips them"""
    ni, nj, nk = dims
    e2, m2, d, mag = terms(lib, u, v, w, h, dims)
    d64 = d.astype(np.float64)
    t = {"e2": e2, "m2": m2, "d2": d64 * d64}
    k, j, i = np.meshgrid(np.arange(nk, dtype=np.float64), np.arange(nj, dtype=np.float64), np.arange(ni, dtype=np.float64),
                          indexing="ij")
    r = None if rho is None else rho.astype(np.float64)
    z = np.zeros(1)
    t["rho"] = z if r is None else r
    t["rho_i"] = z if r is None else r * i.ravel()
    t["rho_j"] = z if r is None else r * j.ravel()
    t["rho_k"] = z if r is None else r * k.ravel()
    t["T"] = z if T is None else T.astype(np.float64)
    val = {s: math.fsum(t[s].tolist()) for s in SUMS}
    mass = {s: math.fsum(np.abs(t[s]).tolist()) for s in SUMS}
    with np.errstate(invalid="ignore"):
        val["div_max"] = float(np.fmax.reduce(np.abs(d), initial=np.float32(0)))
        val["vort_max"] = float(np.fmax.reduce(mag, initial=np.float32(0)))
    return val, mass, ni * nj * nk, mag


def raw_bound(mass, n):
    """{stat: the largest |computed - exact| a sum of n such terms may show}"""
    return {s: n * U * mass[s] for s in SUMS}


def diag_row(raw, h, step=0):
    """the row bq_solver_diagnostics derives from raw sums (a dict over STAT), operation for operation"""
    h = float(np.float32(h))
    h3 = h * h * h
    any_rho = raw["rho"] != 0.0
    return {"kinetic": 0.5 * h3 * raw["e2"], "enstrophy": 0.5 * h3 * raw["m2"], "div_l2": math.sqrt(h3 * raw["d2"]),
            "div_max": raw["div_max"], "rho_sum": raw["rho"],
            "centroid_x": h * raw["rho_i"] / raw["rho"] if any_rho else 0.0,
            "centroid_y": h * raw["rho_j"] / raw["rho"] if any_rho else 0.0,
            "centroid_z": h * raw["rho_k"] / raw["rho"] if any_rho else 0.0,
            "T_sum": raw["T"], "vort_max": raw["vort_max"], "step": step}


def row_bound(val, mass, n, h):
    """{entry: the largest |row computed from sums in any order - diag_row(exact sums)|}: the raw bounds carried through
    diag_row's operations -- a product by the power-of-two-scaled h^3 keeps the relative error and adds one rounding on
    either side (2u), the square root halves it, a quotient adds the relative errors of both sums and two roundings each
    side (4u; second-order terms are below u and covered by one more)"""
    h = float(np.float32(h))
    h3 = h * h * h
    rb = raw_bound(mass, n)
    row = diag_row(val, h)
    rel = lambda s: rb[s] / abs(val[s]) if val[s] != 0.0 else 0.0
    out = {"kinetic": 0.5 * h3 * rb["e2"] + 2 * U * abs(row["kinetic"]),
           "enstrophy": 0.5 * h3 * rb["m2"] + 2 * U * abs(row["enstrophy"]),
           "div_l2": abs(row["div_l2"]) * (0.5 * rel("d2") + 4 * U),
           "div_max": 0.0, "vort_max": 0.0, "step": 0.0, "rho_sum": rb["rho"], "T_sum": rb["T"]}
    for c, s in (("centroid_x", "rho_i"), ("centroid_y", "rho_j"), ("centroid_z", "rho_k")):
        out[c] = abs(row[c]) * (rel(s) + rel("rho") + 5 * U) if val[s] != 0.0 else h * rb[s] / abs(val["rho"] or 1.0) * (1 + 8 * U)
    return out


def run_with_diagnostics(lib, errlib, dims, L, steps, iters, dt, scheme=0, every=0, sample=None, kw=None):
    """the host solver on `lib`: (solver's per-step fields, {step: diagnostics() taken after it} for the steps in `sample`,
    diagnosticsHistory() at the end, vorticity() at the end)"""
    from gpufluidsimulation_amd import solver
    s = solver.BimocqGPUSolver(*dims, L, 0.0, 1.0, lib=lib, errlib=errlib, scheme=scheme, **(kw or {}))
    try:
        s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(dims, L))
        s.setProjection(iters, 0.5)
        if every:
            s.setOption(solver.OPT_DIAGNOSTICS_EVERY, every)
        taken, out = {}, []
        for f in range(steps):
            s.advance(f, dt)
            s._check()
            if sample and (f + 1) in sample:
                taken[f + 1] = s.diagnostics()
            out.append({n: s.field(n) for n in MC.NAMES})
        return out, taken, s.diagnosticsHistory(), s.vorticity()
    finally:
        s.close()
