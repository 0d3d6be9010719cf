"""Shared pieces of the tracer tests: the loader of the CPU stand-in with the tracer operators, the
oracle's trace of a particle list, numpy restatements of the seeding hash and the brick key written from the text of
include/bimocq_gpu.h alone, test velocities and particle sets, and the invariant run of the issue.

No tolerance anywhere: every comparison is on bits."""
import ctypes as C

import numpy as np

import obstacle_case as OC
from build_cpu_tracers import build_tracers

f32 = np.float32
BAD_ARGUMENT, UNSUPPORTED = 3, 4
OPT_REINIT_POLICY, OPT_NODE_LOOKUPS, OPT_TRACER_SORT_EVERY = 2, 14, 17
TRACER_OPS = ("gpu_trace_particles", "gpu_sample_particles", "gpu_seed_particles", "gpu_sort_particles")
# the five fields tracerSample accepts: name -> (extra dims, stagger axis or None)
SAMPLED = {"rho": ((0, 0, 0), None), "T": ((0, 0, 0), None), "u": ((1, 0, 0), 0), "v": ((0, 1, 0), 1), "w": ((0, 0, 1), 2)}


def load_tracers():
    """the stand-in with every restated operator, the tracer operators among them, and tracers_abi_calls"""
    from gpufluidsimulation_amd import _lib
    lib = OC._load(build_tracers(), OC.OPS + OC.LS_OPS + ("gpu_emit_sources", "gpu_maccormack", "gpu_flow_stats", "gpu_render_density")
                   + TRACER_OPS)
    lib.tracers_abi_calls.restype, lib.tracers_abi_calls.argtypes = C.c_long, [C.c_int]
    for name in ("fl_set_option", "fl_get_option"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def ptr(a):
    return a.ctypes.data if a is not None else None


def velocity(dims, h, cfldt, seed=0):
    """random MAC velocity (u, v, w) scaled so that cfldt * max|u| = h, as float32 arrays (nz, ny, nx + 1) ..."""
    ni, nj, nk = dims
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((nk, nj, ni + 1))
    v = rng.standard_normal((nk, nj + 1, ni))
    w = rng.standard_normal((nk + 1, nj, ni))
    top = max(np.abs(u).max(), np.abs(v).max(), np.abs(w).max())
    scale = float(h) / float(cfldt) / top
    out = [np.ascontiguousarray((a * scale).astype(f32)) for a in (u, v, w)]
    while f32(cfldt) * max(np.abs(a).max() for a in out) > f32(h):      # the float32 roundings must not push it above h
        out = [(a * f32(1.0 - 2.0 ** -23)).astype(f32) for a in out]
    for a in out:
        a.setflags(write=False)
    return out


def box_hi(dims, h):
    """the trace's upper clamp per axis, by its own expression: (float)n * h - h"""
    return [f32(f32(n) * f32(h)) - f32(h) for n in dims]


def particles(dims, h, n, seed=1):
    """n positions (n, 3) float32 that mix, lane by lane, points ON the clamp faces, points within one cell of a wall and
    interior points; for n > 256 the lanes 256 .. 511 are all interior, so that whole waves pass get_velocity_auto's vote
    while the mixed waves fail it (a point on a low face with an inward-pointing stage leaves [h, inf))"""
    rng = np.random.default_rng(seed)
    h = f32(h)
    hi = box_hi(dims, h)
    out = np.empty((n, 3), f32)
    for a in range(n):
        kind = a % 3 if not (256 <= a < 512) else 2
        for c in range(3):
            lo_c, hi_c = h, hi[c]
            t = f32(rng.random())
            if kind == 0:                                   # on a face (each axis picks low face, high face or anywhere)
                pick = rng.integers(0, 3)
                out[a, c] = lo_c if pick == 0 else (hi_c if pick == 1 else lo_c + t * (hi_c - lo_c))
            elif kind == 1:                                 # within one cell of a wall
                out[a, c] = lo_c + t * h if rng.integers(0, 2) == 0 else hi_c - t * h
            else:                                           # interior: at least two cells from every wall
                out[a, c] = lo_c + f32(2) * h + t * (hi_c - lo_c - f32(4) * h)
        out[a] = np.minimum(np.maximum(out[a], h), np.array(hi, f32))
    out.setflags(write=False)
    return out


def oracle_trace(O, vel, pts, h, dims, cfldt, dt):
    """the UNMODIFIED oracle on a particle list: the particles packed into the interior entries (2 <= index < n - 2) of
    three map-shaped arrays, orc_solve_forward, the interior entries read back -- chunk by chunk"""
    import oracle_lib as OL
    ni, nj, nk = dims
    inner = (nk - 4, nj - 4, ni - 4)
    per = inner[0] * inner[1] * inner[2]
    out = np.empty_like(np.asarray(pts, f32))
    u, v, w = (np.ascontiguousarray(a, f32) for a in vel)
    for at in range(0, len(pts), per):
        chunk = np.asarray(pts[at:at + per], f32)
        maps = []
        for c in range(3):
            m = np.zeros((nk, nj, ni), f32)
            flat = np.full(per, f32(h), f32)
            flat[:len(chunk)] = chunk[:, c]
            m[2:nk - 2, 2:nj - 2, 2:ni - 2] = flat.reshape(inner)
            maps.append(m)
        O.orc_solve_forward(OL.fp(u), OL.fp(v), OL.fp(w), OL.fp(maps[0]), OL.fp(maps[1]), OL.fp(maps[2]),
                            float(h), ni, nj, nk, float(cfldt), float(dt))
        for c in range(3):
            out[at:at + len(chunk), c] = maps[c][2:nk - 2, 2:nj - 2, 2:ni - 2].reshape(-1)[:len(chunk)]
    return out


def standin_trace(lib, vel, pts, h, dims, cfldt, dt):
    """gpu_trace_particles of a library that works on host memory (the stand-in): (rc, positions (n, 3))"""
    soa = np.ascontiguousarray(np.asarray(pts, f32).T.copy())
    u, v, w = (np.ascontiguousarray(a, f32) for a in vel)
    n = soa.shape[1]
    rc = lib.gpu_trace_particles(ptr(u), ptr(v), ptr(w), ptr(soa[0]), ptr(soa[1]), ptr(soa[2]), n, float(h), *dims,
                                 float(cfldt), float(dt))
    return rc, np.ascontiguousarray(soa.T)


def stagger(name, h):
    """(dims extra, (ox, oy, oz)) of a sampled field: the stagger of get_velocity, (float)(-0.5 * (double)h) on its own axis"""
    extra, axis = SAMPLED[name]
    off = [0.0, 0.0, 0.0]
    if axis is not None:
        off[axis] = float(f32(-0.5 * float(f32(h))))
    return extra, off


# ---- the seeding rule, restated from the header text --------------------------------------------------------------------
def _mix(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x * np.uint32(0x7feb352d)).astype(np.uint32)
    x = x ^ (x >> np.uint32(15))
    x = (x * np.uint32(0x846ca68b)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def seed_box(lo, hi, dims):
    """the box intersected with the cells 1 .. n - 2: (lo', extents)"""
    lo2 = [max(int(lo[c]), 1) for c in range(3)]
    ext = [max(min(int(hi[c]), dims[c] - 1) - lo2[c], 0) for c in range(3)]
    return lo2, ext


def seed_restate(lo, hi, per_cell, seed, h, dims):
    """(positions (n, 3) float32, cells (n, 3) int, fractions (n, 3) float32) by the header's text"""
    lo2, (bx, by, bz) = seed_box(lo, hi, dims)
    n = bx * by * bz * per_cell
    p = np.arange(n, dtype=np.uint64)
    s = p % np.uint64(per_cell)
    cell = p // np.uint64(per_cell)
    x = cell % np.uint64(max(bx, 1))
    y = (cell // np.uint64(max(bx, 1))) % np.uint64(max(by, 1))
    z = cell // np.uint64(max(bx * by, 1))
    Cc = np.stack([x + np.uint64(lo2[0]), y + np.uint64(lo2[1]), z + np.uint64(lo2[2])], axis=1)
    G = Cc[:, 0] + np.uint64(dims[0]) * (Cc[:, 1] + np.uint64(dims[1]) * Cc[:, 2])
    c = G * np.uint64(per_cell) + s
    with np.errstate(over="ignore"):
        lo32 = (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi32 = (c >> np.uint64(32)).astype(np.uint32)
        base = _mix((_mix(lo32 ^ np.uint32(seed & 0xFFFFFFFF)) + hi32).astype(np.uint32))
        pos = np.empty((n, 3), f32)
        frac = np.empty((n, 3), f32)
        h = f32(h)
        for a in range(3):
            r = _mix((base + np.uint32((a * 0x9e3779b9) & 0xFFFFFFFF)).astype(np.uint32)) >> np.uint32(8)
            frac[:, a] = r.astype(f32) * f32(2.0 ** -24)
            q = (Cc[:, a].astype(f32) + frac[:, a]).astype(f32)
            top = f32(f32(dims[a]) * h) - h
            pos[:, a] = np.minimum(np.maximum((q * h).astype(f32), h), top)
    return pos, Cc.astype(np.int64), frac


def brick_keys(xyz, h, dims):
    """the brick key of every position by the header's text (IEEE float32 division)"""
    xyz = np.asarray(xyz, f32)
    nb = [(n + 3) // 4 for n in dims]
    b = []
    for c in range(3):
        q = np.floor((xyz[:, c] / f32(h)).astype(f32)).astype(np.int64)
        b.append(np.clip(q, 0, dims[c] - 1) >> 2)
    return b[0] + nb[0] * (b[1] + nb[1] * b[2])


# ---- the invariant run of the issue -------------------------------------------------------------------------------------
INV_N, INV_L, INV_DT, INV_ITERS = 24, 1.0, 0.05, 40
INV_EMITTER = [(0.5, 0.3, 0.33, 0.15, 1.0, 2.0, 1.0, 1000)]


def node_positions(s):
    """every node position (i h, j h, k h) as (n, 3) float32, x fastest: tracer id = the node's flat index"""
    h = f32(s.h)
    k, j, i = np.meshgrid(np.arange(s.nz), np.arange(s.ny), np.arange(s.nx), indexing="ij")
    return np.stack([i.astype(f32) * h, j.astype(f32) * h, k.astype(f32) * h], axis=-1).reshape(-1, 3).astype(f32)


def invariant_solver(lib=None, errlib=None, **options):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    kw = {"lib": lib, "errlib": errlib} if lib is not None else {"device": 0}
    s = BimocqGPUSolver(INV_N, INV_N, INV_N, INV_L, 0.0, 1.0, **kw)
    s.setSmoke(0.0, 1.0, INV_EMITTER)
    s.setProjection(INV_ITERS, 0.5)
    s.setOption(OPT_REINIT_POLICY, 1)
    for opt, val in options.items():
        s.setOption(int(opt), val)
    return s


def check_invariant(s, frames_after_reseed=True):
    """node-seeded tracers equal the velocity advector's forward map at every interior node after frames 0, 1, 2 (and, reseeded
    at the frame-3 re-initialisation, after frames 4 and 5); returns the largest displacement in cells at frame 2"""
    n = INV_N
    nodes = node_positions(s)
    s.setTracers(nodes)
    inner = np.zeros((n, n, n), bool)
    inner[2:n - 2, 2:n - 2, 2:n - 2] = True
    inner = inner.reshape(-1)

    def compare(frame):
        t = s.tracers()
        for c, name in enumerate(("fx", "fy", "fz")):
            fwd = s.field(name)
            assert np.array_equal(t[inner, c].view(np.uint32), fwd[inner].view(np.uint32)), (frame, name)
        return t

    count0 = None
    moved = 0.0
    for frame in range(3):
        s.advance(frame, INV_DT)
        s._check()
        if frame == 0:
            count0 = s.reinitCounts()[0]
        assert s.reinitCounts()[0] == count0, (frame, s.reinitCounts())
        t = compare(frame)
        moved = float(np.abs(t[inner] - nodes[inner]).max() / f32(s.h))
    assert moved > 0.1, moved                               # (the oracle moves them up to 0.31 cells by frame 2)
    if frames_after_reseed:
        s.advance(3, INV_DT)
        assert s.reinitCounts()[0] == count0 + 1, s.reinitCounts()     # the maps start again from the identity: so do the tracers
        s.setTracers(nodes)
        for frame in (4, 5):
            s.advance(frame, INV_DT)
            assert s.reinitCounts()[0] == count0 + 1, (frame, s.reinitCounts())
            compare(frame)
    s._check()
    return moved
