"""Shared pieces of the obstacle and level-set tests: a numpy restatement of the classification and of the masked sweep
(DESIGN.md section 14), the scene the step tests run, loaders of the CPU stand-ins with the obstacle and level-set
operators, and device buffers for the GPU tests."""
import ctypes as C
import hashlib

import numpy as np

from build_cpu_host import build_levelsets, build_obstacles

f32 = np.float32


def positions(n, staggered, h):
    return ((np.arange(n, dtype=f32) - f32(0.5 if staggered else 0.0)) * f32(h)).astype(f32)


def classify(boundaries, h, shape, stag=(0, 0, 0)):
    """(nk, nj, ni) int array: o + 1 solid by the last obstacle o, -1 band, 0 elsewhere -- float32 throughout, same
    operation order as the kernels"""
    nk, nj, ni = shape
    x = positions(ni, stag[0], h)[None, None, :]
    y = positions(nj, stag[1], h)[None, :, None]
    z = positions(nk, stag[2], h)[:, None, None]
    solid = np.zeros(shape, dtype=np.int32)
    band = np.zeros(shape, dtype=bool)
    h3 = f32(3.0) * f32(h)
    for o, b in enumerate(boundaries):
        sh, cx, cy, cz, rx, ry, rz = b[:7]
        dx, dy, dz = x - f32(cx), y - f32(cy), z - f32(cz)
        if sh == 0:
            d2 = dx * dx + dy * dy + dz * dz
            R = f32(rx) + h3
            s = d2 <= f32(rx) * f32(rx)
            bb = (~s) & (d2 < R * R)
        else:
            ax, ay, az = np.abs(dx) - f32(rx), np.abs(dy) - f32(ry), np.abs(dz) - f32(rz)
            s = (ax <= 0) & (ay <= 0) & (az <= 0)
            qx, qy, qz = np.maximum(ax, f32(0)), np.maximum(ay, f32(0)), np.maximum(az, f32(0))
            d2 = qx * qx + qy * qy + qz * qz
            bb = (~s) & (d2 > 0) & (d2 < h3 * h3)
        solid = np.where(np.broadcast_to(s, shape), o + 1, solid)
        band |= np.broadcast_to(bb, shape)
    return np.where(solid > 0, solid, np.where(band, -1, 0))


def masked_sweep(p, div, solid, alpha, beta):
    """one masked sweep on (nk, nj, ni) float32 arrays"""
    out = p.copy()
    nk, nj, ni = p.shape
    c = (slice(1, nk - 1), slice(1, nj - 1), slice(1, ni - 1))
    nb = [(slice(1, nk - 1), slice(1, nj - 1), slice(0, ni - 2)), (slice(1, nk - 1), slice(1, nj - 1), slice(2, ni)),
          (slice(1, nk - 1), slice(0, nj - 2), slice(1, ni - 1)), (slice(1, nk - 1), slice(2, nj), slice(1, ni - 1)),
          (slice(0, nk - 2), slice(1, nj - 1), slice(1, ni - 1)), (slice(2, nk), slice(1, nj - 1), slice(1, ni - 1))]
    s = sum((solid[q] != 0).astype(np.int32) for q in nb)
    acc = p[nb[0]]
    for q in nb[1:]:
        acc = acc + p[q]
    acc = acc + f32(alpha) * div[c]
    table = [f32(beta)] + [f32(1.0 / (1.0 / float(f32(beta)) - k)) for k in range(1, 6)] + [f32(0)]
    val = np.where(s == 6, f32(0), acc * np.array(table, dtype=f32)[s])
    out[c] = np.where(solid[c] != 0, p[c], val)
    return out


# the step scene: rising smoke at the bottom, a static sphere above it and a box moving sideways through the plume
def scene(n):
    h = 1.0 / n
    em = [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1000)]
    obstacles = [(0, 0.5, 0.55, 0.5, 0.12, 0.0, 0.0, 0.0, 0.0, 0.0),
                 (1, 0.3, 0.8, 0.45, 0.08, 0.05, 0.1, 0.5, 0.0, 0.0)]
    return h, em, obstacles


def bind_errors(lib):
    for name, res, args in (("fl_last_error", C.c_int, []), ("fl_last_error_string", C.c_char_p, []),
                            ("fl_clear_error", None, [])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def run_scene(lib, errlib, n, scheme, steps, iters, scene=scene):
    """`scene` (this one, or levelset_case.scene) for `steps` steps (updateBoundary before every advance); per-step SHA-256
    of rho, T, u, v, w, p and the flags, and the final max rho"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    _, em, obstacles = scene(n)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=errlib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    s.setProjection(iters, 0.5)
    s.setBoundary(obstacles)
    out = []
    for f in range(steps):
        s.updateBoundary(f, 1.0 / n)
        s.advance(f, 1.0 / n)
        d = hashlib.sha256()
        for name in ("rho", "T", "u", "v", "w", "p"):
            d.update(s.field(name).tobytes())
        d.update(s.solidMask().tobytes())
        out.append(d.hexdigest())
    rho_max = float(s.field("rho").max())
    s.close()
    return {"hashes": out, "rho_max": rho_max}


OPS = ("gpu_obstacle_flags", "gpu_obstacle_faces", "gpu_jacobi_sweep_masked", "gpu_jacobi_sweeps_masked",
       "gpu_gradient_masked", "gpu_semilag_band", "gpu_obstacle_blend")
LS_OPS = ("gpu_obstacle_flags_ls", "gpu_semilag_band_ls", "gpu_obstacle_blend_ls")


def _load(path, ops):
    """a stand-in with the host C API, the error functions and `ops` typed from _lib.HIP_SIGS"""
    from gpufluidsimulation_amd import _lib, solver
    lib = bind_errors(solver.bind_host(C.CDLL(path, mode=C.RTLD_LOCAL)))
    for name in ops:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def load_obstacles():
    """the stand-in with the obstacle operators (not the level-set ones)"""
    return _load(build_obstacles(), OPS)


def load_levelsets():
    """the stand-in with the obstacle and the level-set operators"""
    return _load(build_levelsets(), OPS + LS_OPS)


class Dev:
    """device copies of host arrays for the GPU tests: put(name, a) uploads (reusing the buffer of that name when the size
    matches) and returns the device pointer, dev[name] is that pointer, get(name) downloads in the uploaded shape"""
    def __init__(self, hip):
        self.hip, self.bufs = hip, {}

    def put(self, name, a):
        a = np.ascontiguousarray(a)
        if name in self.bufs and self.bufs[name][2] == a.nbytes:
            p = self.bufs[name][0]
        else:
            if name in self.bufs:
                self.hip.fl_free(self.bufs[name][0])
            p = self.hip.fl_malloc(max(a.nbytes, 4))
            assert p
        self.hip.fl_memcpy_h2d(p, a.ctypes.data, a.nbytes)
        self.bufs[name] = (p, a.dtype, a.nbytes, a.shape)
        return p

    def get(self, name):
        p, dt, nb, shape = self.bufs[name]
        out = np.empty(shape, dt)
        self.hip.fl_sync()
        self.hip.fl_memcpy_d2h(out.ctypes.data, p, nb)
        return out

    def __getitem__(self, name):
        return self.bufs[name][0]

    def free(self):
        for v in self.bufs.values():
            self.hip.fl_free(v[0])
        self.bufs = {}


def check(hip):
    assert hip.fl_last_error() == 0, hip.fl_last_error_string()
