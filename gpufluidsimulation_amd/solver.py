"""Python handle on the C++ host solver (csrc/host/, C view in include/bimocq_solver.h).

Same surface as the reference's BimocqGPUSolver (src/bimocq3D/BimocqGPUSolver.h:27-56):
construct, setSmoke, advance(framenum, dt), outputResult(frame, path).
"""
import ctypes as C
import os

import numpy as np

from . import _lib

FIELD_IDS = {"rho": 0, "T": 1, "u": 2, "v": 3, "w": 4, "uinit": 5, "vinit": 6, "winit": 7,
             "rhoinit": 8, "Tinit": 9, "fx": 10, "fy": 11, "fz": 12, "bx": 13, "by": 14, "bz": 15, "p": 16, "div": 17}


class Emitter(C.Structure):
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("cz", C.c_float), ("radius", C.c_float),
                ("density", C.c_float), ("temperature", C.c_float), ("emiter", C.c_float),
                ("emit_frames", C.c_int)]


SHAPE_SPHERE, SHAPE_BOX, SHAPE_LEVELSET = 0, 1, 2
# closed domain walls (setWalls; include/bimocq_gpu.h): one bit per closed side; the reference's container is open at +y
WALL_XLO, WALL_XHI, WALL_YLO, WALL_YHI, WALL_ZLO, WALL_ZHI = 1, 2, 4, 8, 16, 32
WALLS_NONE, WALLS_REFERENCE_BOX = 0, 1 | 2 | 4 | 16 | 32
FLAG_WALL = 0x80
MAX_BOUNDARIES = 16


class Boundary(C.Structure):
    """bq_boundary: shape, centre, radius (sphere: rx) or half extents (box), velocity"""
    _fields_ = [("shape", C.c_int), ("cx", C.c_float), ("cy", C.c_float), ("cz", C.c_float),
                ("rx", C.c_float), ("ry", C.c_float), ("rz", C.c_float),
                ("vx", C.c_float), ("vy", C.c_float), ("vz", C.c_float)]


def boundary_array(boundaries):
    """(Boundary array, count) from Boundary objects or tuples (shape, cx, cy, cz, rx, ry, rz, vx, vy, vz)"""
    boundaries = list(boundaries)
    arr = (Boundary * max(1, len(boundaries)))()
    for i, b in enumerate(boundaries):
        arr[i] = b if isinstance(b, Boundary) else Boundary(*b)
    return arr, len(boundaries)


class LevelSetDesc(C.Structure):
    """bq_levelset: grid pointer, dimensions, index of phi[0, 0, 0], voxel size, background"""
    _fields_ = [("phi", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("i0", C.c_int), ("j0", C.c_int), ("k0", C.c_int), ("voxel", C.c_float), ("background", C.c_float)]


class LevelSet:
    """A dense signed-distance grid ("Level sets"): phi (nz, ny, nx) float32, negative inside;
    phi[k, j, i] is the value at index (i0 + i, j0 + j, k0 + k) = index_min + (i, j, k) of the level set's own index space,
    whose index (0, 0, 0) sits at the obstacle's position and whose spacing is `voxel`.  Outside the stored nodes the level
    set reads `background` (OpenVDB's half_width * voxel): the stored nodes must enclose the solid and its band."""

    def __init__(self, phi, voxel, index_min=(0, 0, 0), background=None):
        self.phi = np.ascontiguousarray(phi, dtype=np.float32)
        if self.phi.ndim != 3:
            raise ValueError("phi must be a (nz, ny, nx) array")
        self.voxel = float(np.float32(voxel))
        self.index_min = tuple(int(x) for x in index_min)
        self.background = float(np.float32(3 * self.voxel if background is None else background))

    def descriptor(self):
        """bq_levelset with phi pointing at this object's HOST array (valid while the object lives)"""
        nz, ny, nx = self.phi.shape
        return LevelSetDesc(self.phi.ctypes.data, nx, ny, nz, *self.index_min, self.voxel, self.background)


def levelset_sphere(radius, voxel, half_width=3):
    """the dense equivalent of OpenVDB's createLevelSetSphere centred on index 0: indices -m .. m on every axis,
    m = ceil(radius / voxel + half_width), phi = (|index| - radius / voxel) * voxel clamped to +-background"""
    m = int(np.ceil(radius / voxel + half_width))
    bg = np.float32(half_width * voxel)
    i = np.arange(-m, m + 1, dtype=np.float64)
    d = np.sqrt(i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2)
    phi = np.clip((d - radius / voxel) * voxel, -bg, bg).astype(np.float32)
    return LevelSet(phi, voxel, (-m, -m, -m), bg)


def levelset_from_sdf(fn, lo, hi, voxel, half_width=3):
    """a LevelSet sampled from fn(x, y, z) -> signed distance (numpy arrays, world units, in the obstacle's frame): the
    index box that covers [lo, hi] on every axis, widened by half_width + 1 voxels so that it holds the band too, values
    clamped to +-background (background = half_width * voxel)"""
    pad = int(np.ceil(half_width)) + 1
    a = [int(np.floor(lo[d] / voxel)) - pad for d in range(3)]
    b = [int(np.ceil(hi[d] / voxel)) + pad for d in range(3)]
    x, y, z = (np.arange(a[d], b[d] + 1, dtype=np.float64) * voxel for d in range(3))
    bg = np.float32(half_width * voxel)
    phi = np.asarray(fn(x[None, None, :], y[None, :, None], z[:, None, None]), dtype=np.float64)
    phi = np.broadcast_to(phi, (z.size, y.size, x.size))
    return LevelSet(np.clip(phi, -bg, bg).astype(np.float32), voxel, tuple(a), bg)


class LevelSetObstacle:
    """an obstacle whose shape is a LevelSet, placed at `position` (the level set's index origin), moving with `velocity`"""

    def __init__(self, levelset, position, velocity=(0.0, 0.0, 0.0)):
        self.levelset = levelset
        self.position = tuple(float(x) for x in position)
        self.velocity = tuple(float(x) for x in velocity)

    def boundary(self):
        return Boundary(SHAPE_LEVELSET, *self.position, 0.0, 0.0, 0.0, *self.velocity)


def levelset_arrays(boundaries):
    """(Boundary array, LevelSetDesc array, count) for a list mixing Boundary objects, tuples and LevelSetObstacles;
    the descriptors point at the LevelSets' host arrays"""
    boundaries = list(boundaries)
    arr = (Boundary * max(1, len(boundaries)))()
    ls = (LevelSetDesc * max(1, len(boundaries)))()
    for i, b in enumerate(boundaries):
        if isinstance(b, LevelSetObstacle):
            arr[i] = b.boundary()
            ls[i] = b.levelset.descriptor()
        else:
            arr[i] = b if isinstance(b, Boundary) else Boundary(*b)
    return arr, ls, len(boundaries)


class PoseDesc(C.Structure):
    """bq_pose: orientation quaternion (w, x, y, z; body -> world, any non-zero scale), angular velocity about the centre"""
    _fields_ = [("qw", C.c_float), ("qx", C.c_float), ("qy", C.c_float), ("qz", C.c_float),
                ("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float)]


class Rotating:
    """An obstacle with a rigid pose: `obstacle` is an analytic tuple, a Boundary or a
    LevelSetObstacle; `orientation` a quaternion (w, x, y, z), body -> world, of any non-zero scale; `spin` the angular
    velocity about the obstacle's centre in the world frame, rad per time unit.  A sphere ignores its orientation."""

    def __init__(self, obstacle, spin=(0.0, 0.0, 0.0), orientation=(1.0, 0.0, 0.0, 0.0)):
        if isinstance(obstacle, Rotating):
            raise ValueError("a Rotating wraps a plain obstacle")
        self.obstacle = obstacle
        self.spin = tuple(float(x) for x in spin)
        self.orientation = tuple(float(x) for x in orientation)
        if len(self.spin) != 3 or len(self.orientation) != 4:
            raise ValueError("spin has 3 components, orientation 4 (w, x, y, z)")

    def pose(self):
        return PoseDesc(*self.orientation, *self.spin)


def pose_arrays(boundaries):
    """(Boundary array, LevelSetDesc array or None, PoseDesc array, count) for a list that may mix Rotating objects with
    everything levelset_arrays takes; entries without a pose get the identity and no spin"""
    boundaries = list(boundaries)
    plain = [b.obstacle if isinstance(b, Rotating) else b for b in boundaries]
    arr, ls, n = levelset_arrays(plain)
    poses = (PoseDesc * max(1, n))()
    for i, b in enumerate(boundaries):
        poses[i] = b.pose() if isinstance(b, Rotating) else PoseDesc(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    return arr, (ls if any(isinstance(b, LevelSetObstacle) for b in plain) else None), poses, n


SOURCE_VELOCITY = 1
MAX_SOURCES = 16


class SourceDesc(C.Structure):
    """bq_source: shape entry (position, extents, the velocity the source itself moves with), density, temperature,
    emitted velocity, angular velocity of the emitted field, emit_frames, flags"""
    _fields_ = [("shape", Boundary), ("density", C.c_float), ("temperature", C.c_float),
                ("ex", C.c_float), ("ey", C.c_float), ("ez", C.c_float),
                ("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float),
                ("emit_frames", C.c_int), ("flags", C.c_int)]


class Source:
    """A shaped, moving smoke source.  shape: ("sphere", r), ("box", (hx, hy, hz)) or a LevelSet
    whose index origin sits at `position`.  Nodes inside take `density` and `temperature` while framenum < emit_frames;
    with velocity = (ex, ey, ez) the u, v, w nodes inside also take velocity + spin x (node - position), velocity=None
    imposes no velocity at all.  The source itself moves by motion * dt at every emission."""

    def __init__(self, shape, position, density, temperature, emit_frames, velocity=None, spin=(0.0, 0.0, 0.0),
                 motion=(0.0, 0.0, 0.0)):
        self.levelset = shape if isinstance(shape, LevelSet) else None
        if self.levelset is not None:
            self.code, self.extents = SHAPE_LEVELSET, (0.0, 0.0, 0.0)
        elif shape[0] == "sphere":
            self.code, self.extents = SHAPE_SPHERE, (float(shape[1]), 0.0, 0.0)
        elif shape[0] == "box":
            self.code, self.extents = SHAPE_BOX, tuple(float(x) for x in shape[1])
        else:
            raise ValueError('shape must be ("sphere", r), ("box", (hx, hy, hz)) or a LevelSet')
        self.position = tuple(float(x) for x in position)
        self.density, self.temperature, self.emit_frames = float(density), float(temperature), int(emit_frames)
        self.velocity = None if velocity is None else tuple(float(x) for x in velocity)
        self.spin = tuple(float(x) for x in spin)
        self.motion = tuple(float(x) for x in motion)

    def descriptor(self):
        vel = self.velocity if self.velocity is not None else (0.0, 0.0, 0.0)
        return SourceDesc(Boundary(self.code, *self.position, *self.extents, *self.motion), self.density, self.temperature,
                          *vel, *self.spin, self.emit_frames, SOURCE_VELOCITY if self.velocity is not None else 0)


def source_arrays(sources):
    """(SourceDesc array, LevelSetDesc array or None, count) for a list of Sources (or ready SourceDescs); the level-set
    descriptors point at the LevelSets' host arrays"""
    sources = list(sources)
    arr = (SourceDesc * max(1, len(sources)))()
    ls = (LevelSetDesc * max(1, len(sources)))()
    any_ls = False
    for i, s in enumerate(sources):
        if isinstance(s, SourceDesc):
            arr[i] = s
            continue
        arr[i] = s.descriptor()
        if s.levelset is not None:
            ls[i] = s.levelset.descriptor()
            any_ls = True
    return arr, (ls if any_ls else None), len(sources)


HOST_SIGS = {
    "bq_solver_create": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int]),
    "bq_solver_create_slab": (C.c_void_p, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int,
                                          C.c_int, C.c_int, C.c_int]),
    "bq_solver_slab_info": (None, [C.c_void_p, C.POINTER(C.c_int)]),
    "bq_solver_destroy": (None, [C.c_void_p]),
    "bq_solver_set_smoke": (None, [C.c_void_p, C.c_float, C.c_float, C.POINTER(Emitter), C.c_int]),
    "bq_solver_set_projection": (None, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
    "bq_solver_set_option": (None, [C.c_void_p, C.c_int, C.c_int]),
    "bq_solver_get_option": (C.c_int, [C.c_void_p, C.c_int]),
    "bq_solver_advance": (None, [C.c_void_p, C.c_int, C.c_float]),
    "bq_solver_output_result": (C.c_long, [C.c_void_p, C.c_uint, C.c_char_p]),
    "bq_solver_output_result_async": (C.c_int, [C.c_void_p, C.c_uint, C.c_char_p]),
    "bq_solver_output_wait": (C.c_long, [C.c_void_p]),
    "bq_solver_download": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_long]),
    "bq_solver_reinit_counts": (C.c_int, [C.c_void_p, C.c_int]),
    "bq_solver_last_distortion": (C.c_float, [C.c_void_p, C.c_int]),
    "bq_solver_mg_history": (C.c_long, [C.c_void_p, C.POINTER(C.c_double), C.c_long]),
    "bq_solver_last_cfldt": (C.c_float, [C.c_void_p]),
    "bq_solver_last_ms": (C.c_float, [C.c_void_p]),
    "bq_solver_reinit_count": (C.c_int, [C.c_void_p]),
    "bq_solver_phase_ms": (C.c_longlong, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "bq_solver_set_boundary": (C.c_int, [C.c_void_p, C.POINTER(Boundary), C.c_int]),
    "bq_solver_set_boundary_levelsets": (C.c_int, [C.c_void_p, C.POINTER(Boundary), C.POINTER(LevelSetDesc), C.c_int]),
    "bq_solver_update_boundary": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "bq_solver_set_boundary_poses": (C.c_int, [C.c_void_p, C.POINTER(Boundary), C.POINTER(LevelSetDesc), C.POINTER(PoseDesc), C.c_int]),
    "bq_solver_boundary_pose": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    "bq_solver_download_solid": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_set_walls": (C.c_int, [C.c_void_p, C.c_int]),
    "bq_solver_get_walls": (C.c_int, [C.c_void_p]),
    "bq_solver_set_vorticity_confinement": (C.c_int, [C.c_void_p, C.c_float]),
    "bq_solver_get_vorticity_confinement": (C.c_float, [C.c_void_p]),
    "bq_solver_set_sources": (C.c_int, [C.c_void_p, C.POINTER(SourceDesc), C.POINTER(LevelSetDesc), C.c_int]),
    "bq_solver_source_position": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "bq_solver_set_pcg_tolerance": (C.c_int, [C.c_void_p, C.c_double]),
    "bq_solver_pcg_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "bq_solver_pcg_pressure": (C.c_long, [C.c_void_p, C.POINTER(C.c_double), C.c_long]),
    "bq_solver_diagnostics": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "bq_solver_diagnostics_history": (C.c_long, [C.c_void_p, C.POINTER(C.c_double), C.c_long]),
    "bq_solver_obstacle_loads": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "bq_solver_obstacle_loads_history": (C.c_long, [C.c_void_p, C.POINTER(C.c_double), C.c_long]),
    "bq_solver_obstacle_loads_raw": (C.c_long, [C.c_void_p, C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bq_solver_vorticity": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_output_vorticity": (C.c_long, [C.c_void_p, C.c_uint, C.c_char_p, C.c_float]),
    "bq_solver_render_size": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bq_solver_render": (C.c_long, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_output_preview": (C.c_long, [C.c_void_p, C.c_uint, C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                            C.c_float]),
    "bq_solver_render_solids": (C.c_long, [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_output_preview_solids": (C.c_long, [C.c_void_p, C.c_uint, C.c_char_p, C.c_int, C.c_int] + [C.c_float] * 6),
    "bq_solver_set_tracers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_seed_tracers": (C.c_long, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_uint]),
    "bq_solver_tracer_count": (C.c_long, [C.c_void_p]),
    "bq_solver_tracers": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long]),
    "bq_solver_tracer_sample": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_long]),
    "bq_solver_output_tracers": (C.c_long, [C.c_void_p, C.c_uint, C.c_char_p, C.c_int]),
    "bq_solver_tracer_stored": (C.c_long, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]),
}
PROJECTION_JACOBI, PROJECTION_MGCG, PROJECTION_PCG = 0, 1, 2
# enum Scheme of the reference (BimocqSolver.h:29) as far as it is built: SEMILAG (1) is refused
SCHEME_BIMOCQ, SCHEME_MACCORMACK, SCHEME_MAC_REFLECTION = 0, 2, 3
# setOption(OPT_FUSED_MACCORMACK, v): 0 separate launches, 1 (default) gpu_maccormack in scheme 2, 2 in scheme 3 too
OPT_FUSED_MACCORMACK = 15
# setOption(OPT_DIAGNOSTICS_EVERY, N): after every N-th advance() the flow diagnostics go into a device ring (diagnosticsHistory)
OPT_DIAGNOSTICS_EVERY = 16
# setOption(OPT_TRACER_SORT_EVERY, N): the tracers are re-sorted by brick after every N-th advance() (0, the default: never)
OPT_TRACER_SORT_EVERY = 17
# setOption(OPT_OBSTACLE_LOADS, N): on every N-th advance() the pressure loads of every obstacle go into a device ring (obstacleLoads)
OPT_OBSTACLE_LOADS = 18
# a row of obstacleLoads (BQ_OLOAD_* of include/bimocq_solver.h): step, dt, n, then OLOAD_COUNT values per obstacle
OLOAD_COUNT = 8
OLOAD_ROW = 3 + _lib.MAX_BOUNDARIES * OLOAD_COUNT
MAX_TRACERS = 1 << 26
# the entries of a diagnostics row (BQ_DIAG_* of include/bimocq_solver.h), in order
DIAG_NAMES = ("kinetic", "enstrophy", "div_l2", "div_max", "rho_sum", "centroid_x", "centroid_y", "centroid_z", "T_sum",
              "vort_max", "step")
DIAG_COUNT = len(DIAG_NAMES)
# direction codes of render() / outputPreview(): the direction a ray travels (None or "none" as a light: no shadowing)
DIRECTIONS = {"+x": 0, "-x": 1, "+y": 2, "-y": 3, "+z": 4, "-z": 5}
# render(solids=True) / outputPreview(solids=True): the solids' (albedo, ambient)
SOLID_SHADING = (0.6, 0.15)
PCG_STOP = {0: "converged", 1: "iteration limit", 2: "breakdown"}
PHASES = ("maps", "advect_compensate", "forces", "projection", "accumulate_reinit")

_host = None


def bind_host(lib):
    for name, (res, args) in HOST_SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def host_lib():
    """libbimocq_host.so (C++ solver); pulls in libbimocq_hip.so through its rpath."""
    global _host
    if _host is None:
        _lib.hip_lib()
        if not os.path.exists(_lib.HOST_SO):
            raise _lib.BimocqLibraryMissing(f"{_lib.HOST_SO} not found: run `make`")
        _host = bind_host(C.CDLL(_lib.HOST_SO))
    return _host


class BimocqGPUSolver:
    """advance()/outputResult() on the MI355X; `lib`/`errlib` are injectable so the CPU-only tests
    can drive the very same host code linked against a CPU stand-in of the C-ABI."""

    def __init__(self, nx, ny, nz, L=1.0, viscosity=0.0, blend=1.0, device=0, lib=None, errlib=None,
                 rank=0, nranks=1, ghost=0, scheme=0):
        """nz is the GLOBAL plane count; with nranks > 1 (or ghost > 0) this object is one z-slab rank
        (set the communicator up first: gpufluidsimulation_amd.transport).  scheme: SCHEME_BIMOCQ, SCHEME_MACCORMACK or
        SCHEME_MAC_REFLECTION."""
        self.lib = lib or host_lib()
        self.errlib = errlib or (_lib.hip_lib() if lib is None else lib)
        self.nx, self.ny, self.nz = nx, ny, nz
        self.h = float(np.float32(L) / np.float32(nx))
        self.s = self.lib.bq_solver_create_slab(device, nx, ny, nz, L, viscosity, blend, scheme, rank, nranks, ghost)
        if not self.s:
            self._check()
            raise _lib.BimocqError("bq_solver_create failed")
        info = (C.c_int * 8)()
        self.lib.bq_solver_slab_info(self.s, info)
        (self.slab_on, self.rank, self.nranks, _, self.own0, self.own1, self.ghost, self.nk_local) = list(info)

    def _check(self):
        code = self.errlib.fl_last_error()
        if code != 0:
            text = self.errlib.fl_last_error_string()
            text = text.decode(errors="replace") if isinstance(text, bytes) else str(text)
            self.errlib.fl_clear_error()
            raise _lib.BimocqError(f"bimocq error {code}: {text}")

    def setSmoke(self, drop, rise, emitters):
        """emitters: iterable of (cx, cy, cz, radius, density, temperature, emiter, emit_frames)"""
        emitters = list(emitters)
        arr = (Emitter * max(1, len(emitters)))()
        for i, e in enumerate(emitters):
            arr[i] = Emitter(*e)
        self.lib.bq_solver_set_smoke(self.s, drop, rise, arr, len(emitters))

    def setProjection(self, iters, halfrdx, kind=0):
        """kind 0: Jacobi, iters sweeps; kind 1: fp64 multigrid-CG, iters outer iterations (reference: 50); kind 2: fp64
        PCG on the masked system to the tolerance of setPcgTolerance, at most iters CG updates (CPU solver: 1000)"""
        self.lib.bq_solver_set_projection(self.s, kind, iters, halfrdx)
        self._check()

    def setPcgTolerance(self, tol):
        """kind 2 stops after the update with max|r| <= tol * max|b| (default 1e-6; 0 < tol < 1)"""
        rc = self.lib.bq_solver_set_pcg_tolerance(self.s, float(tol))
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_set_pcg_tolerance failed")

    def pcgStats(self):
        """the last kind-2 projection: {iterations, max_r, max_b, stop ("converged" / "iteration limit" / "breakdown"),
        projections, unconverged}, or None before the first one"""
        out = (C.c_double * 6)()
        if not self.lib.bq_solver_pcg_stats(self.s, out):
            return None
        return {"iterations": int(out[0]), "max_r": out[1], "max_b": out[2], "stop": PCG_STOP.get(int(out[3]), "?"),
                "projections": int(out[4]), "unconverged": int(out[5])}

    def pcgPressure(self):
        """the fp64 pressure of the last kind-2 projection as a (nz, ny, nx) array, or None before the first one"""
        n = self.lib.bq_solver_pcg_pressure(self.s, None, 0)
        if not n:
            return None
        out = np.zeros(n, dtype=np.float64)
        self.lib.bq_solver_pcg_pressure(self.s, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        self._check()
        return out.reshape(self.nz, self.ny, self.nx)

    def mgHistory(self):
        """tempResult of the last multigrid-CG projection (4096 doubles), or None before the first one"""
        n = self.lib.bq_solver_mg_history(self.s, None, 0)
        if not n:
            return None
        out = np.zeros(n, dtype=np.float64)
        self.lib.bq_solver_mg_history(self.s, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    def setOption(self, option, value):
        """option 1 = BQ_OPT_KEEP_DMC_BORDER, 2 = BQ_OPT_REINIT_POLICY (0 every frame, 1 distortion-driven),
        3 = BQ_OPT_FULL_STATE, 4 = BQ_OPT_FUSED_HOUSEKEEPING, 5 = BQ_OPT_OVERLAP_EXCHANGES, 6 = BQ_OPT_SHALLOW_BLOCKING_EXCHANGE,
        7 = BQ_OPT_JACOBI_ENDS_FIRST, 8 = BQ_OPT_PROFILE_PHASES, 9 = BQ_OPT_REINIT_MAX_TRAVEL, 10 = BQ_OPT_JACOBI_TRIPLES, 14 = BQ_OPT_NODE_LOOKUPS,
        15 = BQ_OPT_FUSED_MACCORMACK, 16 = BQ_OPT_DIAGNOSTICS_EVERY, 17 = BQ_OPT_TRACER_SORT_EVERY, 18 = BQ_OPT_OBSTACLE_LOADS
        (include/bimocq_solver.h)"""
        self.lib.bq_solver_set_option(self.s, option, value)
        self._check()

    def getOption(self, option):
        return self.lib.bq_solver_get_option(self.s, option)

    def phaseMs(self, reset=True):
        """BQ_OPT_PROFILE_PHASES (option 8): ({phase: ms summed over the profiled steps}, steps)"""
        ms = (C.c_double * len(PHASES))()
        steps = self.lib.bq_solver_phase_ms(self.s, ms, 1 if reset else 0)
        return dict(zip(PHASES, list(ms))), int(steps)

    def reinitCounts(self):
        """(velocity map re-initialisations, scalar map re-initialisations) so far"""
        return self.lib.bq_solver_reinit_counts(self.s, 0), self.lib.bq_solver_reinit_counts(self.s, 1)

    def forcedReinits(self):
        """re-initialisations caused by BQ_OPT_REINIT_MAX_TRAVEL (option 9) rather than by the policy's thresholds"""
        return self.lib.bq_solver_reinit_counts(self.s, 2)

    def lastDistortion(self):
        return self.lib.bq_solver_last_distortion(self.s, 0), self.lib.bq_solver_last_distortion(self.s, 1)

    def setBoundary(self, boundaries):
        """setBoundary: replaces the obstacle list (Boundary objects or (shape, cx, cy, cz, rx, ry, rz, vx, vy, vz)
        tuples, or LevelSetObstacles; [] removes every obstacle) and builds the cell flags at the given centres.  One GPU,
        Jacobi or PCG (kind 2) projection.  A list with a level set goes through bq_solver_set_boundary_levelsets, which copies the grids to
        the device; after a failed call with a level set there are no obstacles.  Entries wrapped in Rotating (in any mix with
        the others) carry an orientation and a spin: such a list goes through
        bq_solver_set_boundary_poses, after whose failure there are no obstacles either."""
        boundaries = list(boundaries)
        if any(isinstance(b, Rotating) for b in boundaries):
            arr, ls, poses, n = pose_arrays(boundaries)
            rc = self.lib.bq_solver_set_boundary_poses(self.s, arr, ls, poses, n)
        elif any(isinstance(b, LevelSetObstacle) for b in boundaries):
            arr, ls, n = levelset_arrays(boundaries)
            rc = self.lib.bq_solver_set_boundary_levelsets(self.s, arr, ls, n)
        else:
            arr, n = boundary_array(boundaries)
            rc = self.lib.bq_solver_set_boundary(self.s, arr, n)
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_set_boundary failed")

    def boundaryPoses(self):
        """one (centre, orientation quaternion (w, x, y, z), angular velocity) triple of tuples per obstacle: the solver's
        current poses, the quaternion being its double master copy"""
        out = []
        buf = (C.c_double * 10)()
        i = 0
        while self.lib.bq_solver_boundary_pose(self.s, i, buf) == 0:
            v = list(buf)
            out.append((tuple(v[0:3]), tuple(v[3:7]), tuple(v[7:10])))
            i += 1
        return out

    def updateBoundary(self, framenum, dt):
        """updateBoundary: every centre moves by v * dt and every spinning entry turns by |spin| dt about its spin, then the
        flags are rebuilt"""
        rc = self.lib.bq_solver_update_boundary(self.s, framenum, dt)
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_update_boundary failed")

    def setWalls(self, mask):
        """closes the sides in `mask` (a sum of WALL_* bits; WALLS_REFERENCE_BOX: every side but +y, WALLS_NONE: all open,
        the default): their border cells become solid cells with velocity 0 for the projection.  One
        GPU, Jacobi or PCG (kind 2) projection, with or without obstacles; a refused mask leaves the previous one."""
        rc = self.lib.bq_solver_set_walls(self.s, int(mask))
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_set_walls failed")

    def walls(self):
        """the closed sides in force (WALL_* bits)"""
        return self.lib.bq_solver_get_walls(self.s)

    def setVorticityConfinement(self, eps):
        """vorticity confinement with the dimensionless coefficient `eps` (0, the default, turns it off): every step adds
        dt eps h (N x omega) to the velocity right after the buoyancy.  One GPU, every scheme and
        projection kind.  The force does not see obstacles or walls.  A refused value leaves the previous one."""
        rc = self.lib.bq_solver_set_vorticity_confinement(self.s, float(eps))
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_set_vorticity_confinement failed")

    def vorticityConfinement(self):
        """the confinement coefficient in force"""
        return float(self.lib.bq_solver_get_vorticity_confinement(self.s))

    def setSources(self, sources):
        """replaces the list of shaped sources (Source objects; [] removes them and releases their grids).  Level-set
        grids are copied to the device once.  Allowed on z-slab ranks, with every projection kind, with and without
        obstacles; after a refused call there are no sources."""
        arr, ls, n = source_arrays(sources)
        rc = self.lib.bq_solver_set_sources(self.s, arr, ls, n)
        self._check()
        if rc != 0:
            raise _lib.BimocqError("bq_solver_set_sources failed")

    def sourcePositions(self):
        """the current position of every source as an (n, 3) float32 array"""
        out = []
        p = (C.c_float * 3)()
        while self.lib.bq_solver_source_position(self.s, len(out), p) == 0:
            out.append(list(p))
        return np.array(out, dtype=np.float32).reshape(-1, 3)

    def solidMask(self):
        """cell flags, 1 = obstacle, as a (nz, ny, nx) uint8 array"""
        count = self.lib.bq_solver_download_solid(self.s, None, 0)
        out = np.zeros(count, dtype=np.uint8)
        self.lib.bq_solver_download_solid(self.s, out.ctypes.data, count)
        self._check()
        return out.reshape(self.nk_local, self.ny, self.nx)

    def advance(self, framenum, dt):
        self.lib.bq_solver_advance(self.s, framenum, dt)

    def outputResult(self, frame, path=None):
        n = self.lib.bq_solver_output_result(self.s, frame, path.encode() if path else None)
        self._check()
        return n

    def diagnostics(self):
        """the flow diagnostics of the current fields as a dict over DIAG_NAMES: kinetic energy and
        enstrophy of the cell-centred velocity, L2 and maximum norm of the divergence, the raw density sum and the density
        centroid in world units, the temperature sum, the largest vorticity magnitude and the step count.  Blocking; on
        z-slab ranks collective, every rank gets the whole grid's values."""
        out = (C.c_double * DIAG_COUNT)()
        rc = self.lib.bq_solver_diagnostics(self.s, out)
        self._check()
        if rc != 0:
            raise _lib.BimocqError(f"bq_solver_diagnostics failed ({rc})")
        d = dict(zip(DIAG_NAMES, list(out)))
        d["step"] = int(d["step"])
        return d

    def diagnosticsHistory(self):
        """the samples OPT_DIAGNOSTICS_EVERY retained (at most the last 1024), oldest first: an (n, DIAG_COUNT) float64
        array whose columns are DIAG_NAMES"""
        n = self.lib.bq_solver_diagnostics_history(self.s, None, 0)
        out = np.zeros((max(n, 0), DIAG_COUNT), dtype=np.float64)
        if n > 0:
            self.lib.bq_solver_diagnostics_history(self.s, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        self._check()
        return out

    @staticmethod
    def _loadsDict(row):
        n = int(row[2])
        per = np.array(row[3:3 + n * OLOAD_COUNT], dtype=np.float64).reshape(n, OLOAD_COUNT)
        return {"step": int(row[0]), "dt": float(row[1]), "force": per[:, 0:3].copy(), "torque": per[:, 3:6].copy(),
                "area": per[:, 6].copy(), "p_mean": per[:, 7].copy()}

    def obstacleLoads(self):
        """the newest row OPT_OBSTACLE_LOADS sampled, or None before the first one: a dict with `step`,
        `dt`, and per obstacle `force` (n, 3) and `torque` (n, 3) about its centre -- what the pressure of the step's
        projection(s) puts on the body, fluid density 1 --, `area` (n,) of its wetted faces and `p_mean` (n,) over them.
        Pressure loads only (no viscous traction); with halfrdx = 1 the projection has its physical strength, the default 0.5
        reports what that projection applied; the Jacobi pressure is as converged as its sweeps make it.  Blocking."""
        row = (C.c_double * OLOAD_ROW)()
        rc = self.lib.bq_solver_obstacle_loads(self.s, row)
        self._check()
        if rc < 0:
            raise _lib.BimocqError("bq_solver_obstacle_loads failed")
        return self._loadsDict(list(row)) if rc else None

    def obstacleLoadsHistory(self):
        """the rows OPT_OBSTACLE_LOADS retained (at most the last 1024), oldest first, as a list of obstacleLoads() dicts"""
        n = self.lib.bq_solver_obstacle_loads_history(self.s, None, 0)
        out = np.zeros((max(n, 0), OLOAD_ROW), dtype=np.float64)
        if n > 0:
            n = self.lib.bq_solver_obstacle_loads_history(self.s, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        self._check()
        if n < 0:
            raise _lib.BimocqError("bq_solver_obstacle_loads_history failed")
        return [self._loadsDict(r) for r in out]

    def obstacleLoadsRaw(self, back=0):
        """for tests and tools: the raw sums of the row `back` rows before the newest as {"step", "slots": (2, 16, 8) float64
        (gpu_obstacle_loads' d_out of the step's first and second projection; a slot the step did not fill is 0), "weights":
        (w0, w1)}, or None when there is no such row"""
        slots = np.zeros((2, _lib.MAX_BOUNDARIES, _lib.LOAD_COUNT), dtype=np.float64)
        w = (C.c_double * 2)()
        step = self.lib.bq_solver_obstacle_loads_raw(self.s, int(back), slots.ctypes.data_as(C.POINTER(C.c_double)), w)
        self._check()
        return None if step < 0 else {"step": int(step), "slots": slots, "weights": (w[0], w[1])}

    def vorticity(self):
        """the cell-centred vorticity magnitude of the local planes as a (nk_local, ny, nx) float32 array"""
        count = self.lib.bq_solver_vorticity(self.s, None, 0)
        out = np.empty(count, dtype=np.float32)
        rc = self.lib.bq_solver_vorticity(self.s, out.ctypes.data, count)
        self._check()
        if rc < 0:
            raise _lib.BimocqError("bq_solver_vorticity failed")
        return out.reshape(self.nk_local, self.ny, self.nx)

    def outputVorticity(self, frame, path, threshold=1e-4):
        """writes <path>/vorticity_render_%04u.bqd for frame + 1 (read_density_dump reads it); returns the voxel count"""
        n = self.lib.bq_solver_output_vorticity(self.s, frame, path.encode(), threshold)
        self._check()
        if n < 0:
            raise _lib.BimocqError("bq_solver_output_vorticity failed")
        return n

    @staticmethod
    def _direction(d, light=False):
        """a direction name of DIRECTIONS or its code; as a light also None / "none" / -1 for no shadowing"""
        if light and (d is None or d == "none" or d == -1):
            return -1
        if isinstance(d, str):
            if d not in DIRECTIONS:
                raise ValueError(f"direction {d!r}: one of {sorted(DIRECTIONS)}")
            return DIRECTIONS[d]
        return int(d)

    def renderSize(self, view="+z"):
        """(W, H) of the image render() returns for a view"""
        w, h = C.c_int(0), C.c_int(0)
        rc = self.lib.bq_solver_render_size(self.s, self._direction(view), C.byref(w), C.byref(h))
        self._check()
        if rc != 0:
            raise _lib.BimocqError(f"bq_solver_render_size failed ({rc})")
        return w.value, h.value

    @staticmethod
    def _solids(solids):
        """the solids' (albedo, ambient) of render() / outputPreview(): True is SOLID_SHADING"""
        if solids is True:
            return SOLID_SHADING
        try:
            albedo, ambient = solids
            return float(albedo), float(ambient)
        except (TypeError, ValueError):
            raise ValueError(f"solids {solids!r}: None, False, True or an (albedo, ambient) pair") from None

    def render(self, view="+z", light="-y", sigma=8.0, albedo=1.0, ambient=0.1, solids=None):
        """a shadowed emission-absorption preview of the current density, drawn on the device: the
        orthographic view along `view`, self-shadowed by one directional light travelling along `light` ("+x" ... "-z", or
        None for no shadowing); sigma is the extinction per unit density and length.  Returns (radiance, transmittance) as
        float32 arrays of shape (H, W): view +-z gives (ny, nx), +-y (nz, nx), +-x (nz, ny), row index = the higher axis.
        Blocking; on z-slab ranks collective, every rank gets the whole image.
        solids (None or False: off): True or an (albedo, ambient) pair (True: (0.6, 0.15)) also draws the solid obstacles as
        opaque, flat-shaded bodies that cast full shadows, and returns (radiance, transmittance, hit): hit is a uint8 (H, W)
        array with the tag o + 1 of the obstacle a pixel's ray meets first, 0 where it meets none; a hit pixel's
        transmittance is 0.  Domain walls are not drawn."""
        w, h = self.renderSize(view)
        rad, tr = np.empty(w * h, dtype=np.float32), np.empty(w * h, dtype=np.float32)
        if solids is not None and solids is not False:
            sa, sb = self._solids(solids)
            hit = np.empty(w * h, dtype=np.uint8)
            n = self.lib.bq_solver_render_solids(self.s, self._direction(view), self._direction(light, True), sigma, albedo, ambient,
                                                 sa, sb, rad.ctypes.data, tr.ctypes.data, hit.ctypes.data, w * h)
            self._check()
            if n != w * h:
                raise _lib.BimocqError("bq_solver_render_solids failed")
            return rad.reshape(h, w), tr.reshape(h, w), hit.reshape(h, w)
        n = self.lib.bq_solver_render(self.s, self._direction(view), self._direction(light, True), sigma, albedo, ambient,
                                      rad.ctypes.data, tr.ctypes.data, w * h)
        self._check()
        if n != w * h:
            raise _lib.BimocqError("bq_solver_render failed")
        return rad.reshape(h, w), tr.reshape(h, w)

    def outputPreview(self, frame, path, view="+z", light="-y", sigma=8.0, albedo=1.0, ambient=0.1, background=0.0, solids=None):
        """writes the preview as <path>/preview_%04u.pgm for frame + 1 (binary 8-bit P5, +y or +z up; on z-slab ranks rank 0
        writes); returns the bytes written.  solids: as for render() -- the obstacles are drawn too"""
        if solids is not None and solids is not False:
            sa, sb = self._solids(solids)
            n = self.lib.bq_solver_output_preview_solids(self.s, frame, path.encode(), self._direction(view),
                                                         self._direction(light, True), sigma, albedo, ambient, sa, sb, background)
            self._check()
            if n < 0:
                raise _lib.BimocqError("bq_solver_output_preview_solids failed")
            return n
        n = self.lib.bq_solver_output_preview(self.s, frame, path.encode(), self._direction(view), self._direction(light, True),
                                              sigma, albedo, ambient, background)
        self._check()
        if n < 0:
            raise _lib.BimocqError("bq_solver_output_preview failed")
        return n

    # ---- passive tracer particles ----
    def setTracers(self, positions):
        """replaces the tracer set with `positions` ((n, 3) float32 world coordinates; an empty array releases everything).
        Finite positions are clamped into [h, (n - 1) h] per axis; a NaN or an Inf is refused and leaves no tracers.  While
        there are tracers every advance() moves them through the velocity the step starts with -- the forward map's own
        trace, so a tracer on a grid node stays bit for bit on that node's forward-map entry until a re-initialisation.
        One GPU; tracers are passive and ignore obstacles."""
        a = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        rc = self.lib.bq_solver_set_tracers(self.s, a.ctypes.data if a.size else None, a.shape[0])
        self._check()
        if rc != 0:
            raise _lib.BimocqError(f"bq_solver_set_tracers failed ({rc})")

    def seedTracers(self, cell_lo, cell_hi, per_cell=1, seed=0):
        """appends per_cell jittered tracers in every cell of the half-open cell box [cell_lo, cell_hi) (cut to the cells
        1 .. n - 2); ids continue from the current count.  Returns the number added."""
        lo, hi = (C.c_int * 3)(*[int(x) for x in cell_lo]), (C.c_int * 3)(*[int(x) for x in cell_hi])
        n = self.lib.bq_solver_seed_tracers(self.s, lo, hi, int(per_cell), int(seed) & 0xFFFFFFFF)
        self._check()
        if n < 0:
            raise _lib.BimocqError("bq_solver_seed_tracers failed")
        return n

    def tracerCount(self):
        return self.lib.bq_solver_tracer_count(self.s)

    def tracers(self):
        """the tracer positions as an (n, 3) float32 array in id order, whatever sorting has happened.  Blocking."""
        n = self.tracerCount()
        out = np.empty((n, 3), dtype=np.float32)
        rc = self.lib.bq_solver_tracers(self.s, out.ctypes.data if n else None, n)
        self._check()
        if rc < 0:
            raise _lib.BimocqError("bq_solver_tracers failed")
        return out

    def tracerSample(self, which):
        """the current field `which` ("rho", "T", "u", "v", "w" or its id) at every tracer, in id order.  Blocking."""
        which = FIELD_IDS[which] if isinstance(which, str) else int(which)
        n = self.tracerCount()
        out = np.empty(n, dtype=np.float32)
        rc = self.lib.bq_solver_tracer_sample(self.s, which, out.ctypes.data if n else None, n)
        self._check()
        if rc < 0:
            raise _lib.BimocqError("bq_solver_tracer_sample failed")
        return out

    def outputTracers(self, frame, path, which=None):
        """writes <path>/tracers_%04u.bqp for frame + 1 (read_tracer_dump reads it): the positions in id order and, with
        `which`, that field sampled at them; returns the bytes written"""
        w = -1 if which is None else (FIELD_IDS[which] if isinstance(which, str) else int(which))
        n = self.lib.bq_solver_output_tracers(self.s, frame, path.encode(), w)
        self._check()
        if n < 0:
            raise _lib.BimocqError("bq_solver_output_tracers failed")
        return n

    def tracersStored(self):
        """(positions (n, 3), ids (n,)) in the STORED order -- what the trace kernel walks; for tests and tools"""
        n = self.tracerCount()
        soa, ids = np.empty((3, n), dtype=np.float32), np.empty(n, dtype=np.uint32)
        self.lib.bq_solver_tracer_stored(self.s, soa.ctypes.data if n else None, ids.ctypes.data if n else None, n)
        self._check()
        return np.ascontiguousarray(soa.T), ids

    def outputResultAsync(self, frame, path=None):
        """start the dump of the current density without stalling the simulation; waitOutput() joins it"""
        ok = self.lib.bq_solver_output_result_async(self.s, frame, path.encode() if path else None)
        self._check()
        return bool(ok)

    def waitOutput(self):
        return self.lib.bq_solver_output_wait(self.s)

    def field(self, name):
        which = FIELD_IDS[name]
        count = self.lib.bq_solver_download(self.s, which, None, 0)
        out = np.empty(count, dtype=np.float32)
        self.lib.bq_solver_download(self.s, which, out.ctypes.data, count)
        self._check()
        return out

    def owned(self, name):
        """the planes this rank owns, as a flat array in global plane order (w on the last rank also
        carries its top plane) -- concatenating owned() over the ranks gives the single-GPU field"""
        a = self.field(name)
        if not self.slab_on:
            return a
        kind = {"u": (self.nx + 1) * self.ny, "uinit": (self.nx + 1) * self.ny,
                "v": self.nx * (self.ny + 1), "vinit": self.nx * (self.ny + 1)}.get(name, self.nx * self.ny)
        extra = 1 if name in ("w", "winit") and self.own1 == self.nz else 0
        return a[kind * self.ghost: kind * (self.ghost + self.own1 - self.own0 + extra)]

    @property
    def cfldt(self):
        return self.lib.bq_solver_last_cfldt(self.s)

    @property
    def last_ms(self):
        return self.lib.bq_solver_last_ms(self.s)

    @property
    def reinit_count(self):
        return self.lib.bq_solver_reinit_count(self.s)

    def close(self):
        if getattr(self, "s", None):
            self.lib.bq_solver_destroy(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_density_dump(path):
    """Reader of the BQDENS01 container written by outputResult (density_dump.cpp)."""
    hdr = np.dtype([("magic", "S8"), ("frame", "<u4"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"),
                    ("k_offset", "<i4"), ("nz_local", "<i4"), ("voxel_size", "<f4"), ("threshold", "<f4"),
                    ("grid_name", "S16"), ("grid_class", "<u4"), ("count", "<u8")])
    rec = np.dtype([("i", "<i4"), ("j", "<i4"), ("k", "<i4"), ("value", "<f4")])
    with open(path, "rb") as f:
        h = np.frombuffer(f.read(hdr.itemsize), dtype=hdr)[0]
        assert h["magic"] == b"BQDENS01", h["magic"]
        r = np.frombuffer(f.read(), dtype=rec)
    assert len(r) == h["count"]
    return h, r


def read_tracer_dump(path):
    """Reader of the BQPART01 container written by outputTracers: (header, positions (n, 3) float32, attribute (n,) or None)"""
    hdr = np.dtype([("magic", "S8"), ("version", "<u4"), ("frame", "<u4"), ("count", "<u8"), ("nx", "<i4"), ("ny", "<i4"),
                    ("nz", "<i4"), ("h", "<f4"), ("attribute", "<i4")])
    with open(path, "rb") as f:
        h = np.frombuffer(f.read(hdr.itemsize), dtype=hdr)[0]
        assert h["magic"] == b"BQPART01" and h["version"] == 1, (h["magic"], h["version"])
        n = int(h["count"])
        xyz = np.frombuffer(f.read(12 * n), dtype="<f4").reshape(n, 3)
        attr = np.frombuffer(f.read(4 * n), dtype="<f4") if h["attribute"] >= 0 else None
        assert f.read() == b"" and xyz.shape[0] == n and (attr is None or attr.size == n)
    return h, xyz, attr
