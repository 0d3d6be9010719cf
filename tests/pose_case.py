"""Shared pieces of the rotating-obstacle tests: an independent numpy restatement of the rotation
matrix (float64 from the four floats, rounded to float32), of the float32 classification of lists with oriented entries and
of the rigid face velocities; the loader of the CPU stand-in with the pose operators; the lists, scenes and runs the CPU
and GPU tests share."""
import ctypes as C
import hashlib

import numpy as np

import fields as F
import levelset_case as LC
import obstacle_case as OC
import pcg_case as PC
import walls_case as WC
from build_cpu_pose import build_pose

f32, f64 = np.float32, np.float64

POSE_OPS = ("gpu_obstacle_flags_pose", "gpu_semilag_band_pose", "gpu_obstacle_blend_pose", "gpu_obstacle_faces_pose")


def load_pose():
    """the stand-in with the obstacle, level-set, PCG, wall and pose operators"""
    return OC._load(build_pose(), OC.OPS + OC.LS_OPS + PC.PCG_OPS + WC.WALL_OPS + POSE_OPS)


def rotation(q):
    """R (3, 3) float32, body -> world, of the quaternion q = (w, x, y, z): its four float32 values promoted to float64, the
    scale-free formula, every entry rounded to float32"""
    w, x, y, z = (f64(f32(c)) for c in q)
    s = w * w + x * x + y * y + z * z
    R = [[1.0 - 2.0 * (y * y + z * z) / s, 2.0 * (x * y - w * z) / s, 2.0 * (x * z + w * y) / s],
         [2.0 * (x * y + w * z) / s, 1.0 - 2.0 * (x * x + z * z) / s, 2.0 * (y * z - w * x) / s],
         [2.0 * (x * z - w * y) / s, 2.0 * (y * z + w * x) / s, 1.0 - 2.0 * (x * x + y * y) / s]]
    return np.array(R, f64).astype(f32)


def split(entry):
    """(plain entry, orientation, spin) of a list entry, Rotating or not"""
    from gpufluidsimulation_amd.solver import Rotating
    if isinstance(entry, Rotating):
        return entry.obstacle, entry.orientation, entry.spin
    return entry, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)


def record(entry):
    """(shape, centre, extents, velocity) of a plain entry"""
    from gpufluidsimulation_amd.solver import Boundary, LevelSetObstacle
    if isinstance(entry, LevelSetObstacle):
        return 2, entry.position, (0.0, 0.0, 0.0), entry.velocity
    if isinstance(entry, Boundary):
        entry = (entry.shape, entry.cx, entry.cy, entry.cz, entry.rx, entry.ry, entry.rz, entry.vx, entry.vy, entry.vz)
    return int(entry[0]), tuple(entry[1:4]), tuple(entry[4:7]), tuple(entry[7:10])


def oriented(entry):
    plain, q, _ = split(entry)
    return record(plain)[0] != 0 and any(f32(c) != 0 for c in q[1:])


def sample_index(ls, g):
    """the level set at the index-space positions g = (gx, gy, gz) (float64 arrays): float32, `background` where every
    corner lies outside the stored nodes"""
    nz, ny, nx = ls.phi.shape
    n, lo = (nx, ny, nz), ls.index_min
    bg = f32(ls.background)
    g = np.broadcast_arrays(*g)
    inside = np.ones(g[0].shape, bool)
    for d in range(3):
        inside &= (g[d] >= lo[d] - 1) & (g[d] < lo[d] + n[d])
    gi = [np.where(inside, gd, f64(lo[d])) for d, gd in enumerate(g)]
    fl = [np.floor(gd) for gd in gi]
    t = [gd - fd for gd, fd in zip(gi, fl)]
    a = [fd.astype(np.int64) - lo[d] for d, fd in enumerate(fl)]
    pad = np.pad(ls.phi, 1, constant_values=bg)

    def node(di, dj, dk):
        return pad[a[2] + dk + 1, a[1] + dj + 1, a[0] + di + 1]

    def lerp(p, q, wgt):
        return p + ((q - p).astype(f64) * wgt).astype(f32)

    y0 = lerp(lerp(node(0, 0, 0), node(0, 0, 1), t[2]), lerp(node(0, 1, 0), node(0, 1, 1), t[2]), t[1])
    y1 = lerp(lerp(node(1, 0, 0), node(1, 0, 1), t[2]), lerp(node(1, 1, 0), node(1, 1, 1), t[2]), t[1])
    return np.where(inside, lerp(y0, y1, t[0]), bg).astype(f32)


def classify(entries, h, shape, stag=(0, 0, 0)):
    """(nk, nj, ni) int array for a list whose entries may be Rotating: o + 1 solid by the last entry o covering the node,
    -1 band, 0 elsewhere.  Entries that are not oriented go through the restatements of the earlier features."""
    nk, nj, ni = shape
    x = OC.positions(ni, stag[0], h)[None, None, :]
    y = OC.positions(nj, stag[1], h)[None, :, None]
    z = OC.positions(nk, stag[2], h)[:, None, None]
    h3 = f32(3.0) * f32(h)
    solid = np.zeros(shape, np.int32)
    band = np.zeros(shape, bool)
    for o, e in enumerate(entries):
        plain, q, _ = split(e)
        if not oriented(e):
            c = LC.classify([plain], h, shape, stag)
            cov, bb = c == 1, c == -1
        else:
            sh, ctr, ext, _ = record(plain)
            R = rotation(q)
            dx, dy, dz = np.broadcast_arrays(x - f32(ctr[0]), y - f32(ctr[1]), z - f32(ctr[2]))
            b = [R[0, a] * dx + R[1, a] * dy + R[2, a] * dz for a in range(3)]           # R^T d, left to right, float32
            assert all(v.dtype == f32 for v in b)
            if sh == 2:
                vox = f64(f32(plain.levelset.voxel))
                s = sample_index(plain.levelset, [v.astype(f64) / vox for v in b])
                cov, bb = s <= 0, (s > 0) & (s < f32(plain.levelset.background))
            else:
                a = [np.abs(v) - f32(r) for v, r in zip(b, ext)]
                cov = (a[0] <= 0) & (a[1] <= 0) & (a[2] <= 0)
                qq = [np.maximum(v, f32(0)) for v in a]
                d2 = qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2]
                bb = (~cov) & (d2 > 0) & (d2 < h3 * h3)
        solid = np.where(cov, o + 1, solid)
        band |= bb
    return np.where(solid > 0, solid, np.where(band, -1, 0))


def rows_summary(solid):
    """(nk, nj) uint8: 1 where a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1"""
    any_row = np.pad((solid != 0).any(axis=2), 1)
    nk, nj = solid.shape[:2]
    out = np.zeros((nk, nj), bool)
    for dk in range(3):
        for dj in range(3):
            out |= any_row[dk:dk + nk, dj:dj + nj]
    return out.astype(np.uint8)


def faces(u, v, w, solid, entries, h):
    """(u, v, w, du, dv, dw) after the solid-face write: a face of a solid cell takes the velocity of its owner (the larger
    flag of its two cells) -- the rigid velocity at the face's own position when the owner spins; d*: new - old there, the
    incoming value elsewhere.  u, v, w: (nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni) float32; solid (nk, nj, ni)."""
    nk, nj, ni = solid.shape
    out = []
    for axis, (field, sh) in enumerate(((u, (nk, nj, ni + 1)), (v, (nk, nj + 1, ni)), (w, (nk + 1, nj, ni)))):
        a, b = WC._pair(solid, 2 - axis)
        owner = np.maximum(a, b)
        stag = [int(axis == d) for d in range(3)]
        x = np.broadcast_to(OC.positions(sh[2], stag[0], h)[None, None, :], sh)
        y = np.broadcast_to(OC.positions(sh[1], stag[1], h)[None, :, None], sh)
        z = np.broadcast_to(OC.positions(sh[0], stag[2], h)[:, None, None], sh)
        new = field.copy()
        for o, e in enumerate(entries):
            plain, _, spin = split(e)
            _, ctr, _, vel = record(plain)
            val = np.full(sh, f32(vel[axis]), f32)
            ox, oy, oz = (f32(c) for c in spin)
            if ox != 0 or oy != 0 or oz != 0:
                dx, dy, dz = x - f32(ctr[0]), y - f32(ctr[1]), z - f32(ctr[2])
                cross = (oy * dz - oz * dy, oz * dx - ox * dz, ox * dy - oy * dx)[axis]
                val = f32(vel[axis]) + cross
            new = np.where(owner == o + 1, val.astype(f32), new)
        out.append((new, np.where(owner != 0, new - field, f32(0)).astype(f32), owner != 0))
    return out


def arrays(entries, dev=None):
    """(Boundary array, LevelSetDesc array, PoseDesc array, n) for the operators; with dev (obstacle_case.Dev) the
    descriptors' phi are device copies"""
    from gpufluidsimulation_amd.solver import LevelSetDesc, LevelSetObstacle, pose_arrays
    arr, ls, poses, n = pose_arrays(entries)
    if ls is None:
        ls = (LevelSetDesc * max(1, n))()
    if dev is not None:
        for o, e in enumerate(entries):
            plain = split(e)[0]
            if isinstance(plain, LevelSetObstacle):
                ls[o].phi = dev.put(f"phi{o}", plain.levelset.phi)
    return arr, ls, poses, n


def mixed(dims, posed=True):
    """the mixed list of the operator tests on a grid of `dims` cells: a (spinning) sphere, an oriented box, an oriented level
    set with voxel != h and a negative index_min, an unoriented box touching the oriented one, and an unoriented level set;
    generic quaternions, none of unit length.  posed=False: the same entries with identity orientations and no spin."""
    from gpufluidsimulation_amd.solver import LevelSetObstacle, Rotating, levelset_sphere
    ni, nj, nk = dims
    h = 1.0 / ni
    X, Y, Z = ni * h, nj * h, nk * h
    m = min(Y, Z)
    plain = [(0, 0.2 * X, 0.45 * Y, 0.5 * Z, 0.22 * m, 0, 0, 0.1, 0.0, -0.2),
             (1, 0.55 * X, 0.5 * Y, 0.5 * Z, 0.16 * X, 0.1 * m, 0.2 * m, 0.0, 0.3, 0.0),
             LevelSetObstacle(LC.box_levelset((0.12 * X, 0.18 * m, 0.1 * m), 1.3 * h, 2), (0.8 * X + 0.3 * h, 0.5 * Y, 0.45 * Z), (0.2, 0.0, 0.1)),
             (1, 0.55 * X + 0.05 * X, 0.5 * Y + 0.15 * m, 0.5 * Z, 0.05 * X, 0.1 * m, 0.08 * m, -0.4, 0.0, 0.0),
             LevelSetObstacle(levelset_sphere(0.15 * m, 0.7 * h), (0.35 * X, 0.7 * Y, 0.4 * Z))]
    assert plain[2].levelset.index_min[0] < 0 and plain[2].levelset.voxel != h
    if not posed:
        return h, [Rotating(e) for e in plain]
    return h, [Rotating(plain[0], spin=(0.3, -0.2, 0.5), orientation=(0.3, 0.2, -0.5, 0.9)),
               Rotating(plain[1], spin=(0.0, 0.0, 1.5), orientation=(1.7, 0.4, -0.3, 1.1)),
               Rotating(plain[2], spin=(-0.7, 0.4, 0.2), orientation=(-0.8, 0.5, 1.3, 0.6)),
               Rotating(plain[3]),
               plain[4]]


def box(half, centre, velocity=(0.0, 0.0, 0.0)):
    return (1, *centre, *half, *velocity)


def scene(n):
    """the hashed step scene on a 24 x 20 x 16 style grid of spacing h = 1 / n: rising smoke, a spinning, tilted level-set
    box (voxel 0.75 h) above it and a translating sphere"""
    from gpufluidsimulation_amd.solver import LevelSetObstacle, Rotating
    h = 1.0 / n
    em = [(0.5, 0.2, 0.33, 0.1, 1.0, 1.0, 0.0, 1000)]
    entries = [Rotating(LevelSetObstacle(LC.box_levelset((0.16, 0.04, 0.08), 0.75 * h), (0.5, 0.5, 0.33)),
                        spin=(0.0, 0.6, 2.0), orientation=(0.9, 0.1, 0.2, 0.3)),
               (0, 0.25, 0.62, 0.3, 0.09, 0.0, 0.0, 0.4, 0.0, 0.0)]
    return h, em, entries


SCENE_DIMS, SCENE_STEPS = (24, 20, 16), 6
SCENE_KINDS = {"jacobi": (0, 40, 0.5), "pcg": (2, 1000, 1.0)}         # projection kind, iterations, halfrdx


def run_scene(lib, errlib, scheme, kind, walls):
    """SCENE_STEPS steps of `scene` (updateBoundary before every advance): per-step SHA-256 of rho, T, u, v, w, p, the flags
    and the poses' quaternions rounded to float32"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    ni, nj, nk = SCENE_DIMS
    h, em, entries = scene(ni)
    k, iters, halfrdx = SCENE_KINDS[kind]
    s = BimocqGPUSolver(ni, nj, nk, 1.0, 0.0, 1.0, lib=lib, errlib=errlib, scheme=scheme)
    s.setSmoke(0.0, 1.0, em)
    s.setProjection(iters, halfrdx, kind=k)
    s.setBoundary(entries)
    if walls:
        s.setWalls(walls)
    out = []
    for f in range(SCENE_STEPS):
        s.updateBoundary(f, h)
        s.advance(f, h)
        d = hashlib.sha256()
        for name in ("rho", "T", "u", "v", "w", "p"):
            d.update(s.field(name).tobytes())
        d.update(s.solidMask().tobytes())
        d.update(np.array([p[1] for p in s.boundaryPoses()], f64).astype(f32).tobytes())
        out.append(d.hexdigest())
    rho = s.field("rho")
    res = {"hashes": out, "rho_max": float(rho.max()), "solid_cells": int(s.solidMask().sum())}
    s.close()
    return res


def scene_cases():
    return [(scheme, kind, walls) for scheme in (0, 2, 3) for kind in SCENE_KINDS for walls in (0, WC.REFERENCE_BOX)]


def case_key(scheme, kind, walls):
    return f"scheme{scheme}_{kind}_{'box' if walls else 'open'}"


# ---- the paddle on still fluid ------------------------------------------------------------------------------------------
PADDLE_N, PADDLE_STEPS = 32, 6
# the tip of the paddle (0.3 L from the axis, 2 h off it) moves |omega| * r * dt per step: with dt = h and omega0 = 2 that
# is 2 * hypot(0.3, 2 / 32) * h = 0.61 h, less than one cell
PADDLE_OMEGA = 2.0


def run_paddle(lib, errlib, omega):
    """6 steps of updateBoundary; advance on still fluid (no emitters) with scenes.paddle turning at `omega` about z, PCG
    projection with halfrdx = 1.  Returns the solver (the caller closes it) after the last step."""
    from gpufluidsimulation_amd import scenes
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    n = PADDLE_N
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=errlib)
    s.setSmoke(0.0, 1.0, [])
    s.setProjection(1000, 1.0, kind=2)
    s.setBoundary(scenes.paddle(n, 1.0, spin=omega))
    for f in range(PADDLE_STEPS):
        s.updateBoundary(f, h)
        s.advance(f, h)
    return s


def angular_momentum(s):
    """Lz = sum over fluid cell centres of (x - cx) v_c - (y - cy) u_c, the face values averaged to the centres, float64"""
    n = PADDLE_N
    h = 1.0 / n
    u = s.field("u").reshape(n, n, n + 1).astype(f64)
    v = s.field("v").reshape(n, n + 1, n).astype(f64)
    uc, vc = 0.5 * (u[:, :, 1:] + u[:, :, :-1]), 0.5 * (v[:, 1:, :] + v[:, :-1, :])
    fluid = s.solidMask().reshape(n, n, n) == 0
    x = (np.arange(n) * h - 0.5)[None, None, :]
    y = (np.arange(n) * h - 0.5)[None, :, None]
    return float(((x * vc - y * uc) * fluid).sum())


# ---- checks the CPU and the GPU tests share, parametrised by how the operators are called ---------------------------------
TURN_DIMS = (19, 14, 11)
TURNS = [((1, 0, 0, 1), (1, 0, 2)), ((1, 1, 0, 0), (0, 2, 1)), ((1, 0, 1, 0), (2, 1, 0))]     # quarter turn -> extents permutation


def turn_cases():
    h = 1.0 / TURN_DIMS[0]
    ext = (0.21, 0.11, 0.15)
    ctr = (0.47, 0.36, 0.3)
    for q, perm in TURNS:
        yield q, box(ext, ctr), box(tuple(ext[a] for a in perm), ctr), h
        half = tuple(0.0 if c == 1 and i == 0 else c for i, c in enumerate(q))        # (0, axis): the half turn
        yield half, box(ext, ctr), box(ext, ctr), h


def check_turns(flags_fn, band_fn):
    from gpufluidsimulation_amd.solver import Rotating
    for q, body, world, h in turn_cases():
        a, b = flags_fn(TURN_DIMS, h, [Rotating(body, orientation=q)]), flags_fn(TURN_DIMS, h, [Rotating(world)])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), q
        assert a[0].any() and not a[0].all()
        for x, y in zip(band_fn(TURN_DIMS, h, [Rotating(body, orientation=q)]), band_fn(TURN_DIMS, h, [Rotating(world)])):
            assert np.array_equal(x, y) and x.any(), q


def face_lists(dims):
    """two touching boxes (the second owns the shared faces) and a sphere, with linear velocities"""
    ni, nj, nk = dims
    h = 1.0 / ni
    X, Y, Z = ni * h, nj * h, nk * h
    return h, [box((0.15 * X, 0.2 * Y, 0.25 * Z), (0.3 * X, 0.5 * Y, 0.5 * Z), (0.1, -0.2, 0.05)),
               box((0.15 * X, 0.15 * Y, 0.2 * Z), (0.6 * X, 0.5 * Y, 0.5 * Z), (0.0, 0.3, 0.0)),
               (0, 0.75 * X, 0.25 * Y, 0.3 * Z, 0.12 * min(Y, Z), 0, 0, -0.1, 0.0, 0.2)]


SPINS = [((0.7, 0.0, 0.0), (0.0, -1.1, 0.0), (0.0, 0.0, 0.9)), ((0.0, 0.0, 1.3), (0.4, 0.0, 0.0), (0.0, 0.8, 0.0)),
         ((0.3, -0.6, 0.9), (-0.2, 0.5, 0.1), (0.0, 0.0, 0.0))]


def check_faces(dims, call_pose, call_plain, flags_fn):
    """call_pose(u, v, w, du, dv, dw, solid, entries, h) and call_plain(..., analytic entries, h) write in place (du may be
    None); flags_fn(dims, h, entries) -> solid with owners"""
    from gpufluidsimulation_amd.solver import Rotating
    ni, nj, nk = dims
    h, plain = face_lists(dims)
    solid = flags_fn(dims, h, [Rotating(e) for e in plain])
    assert {1, 2, 3}.issubset(set(np.unique(solid)))
    a, b = WC._pair(solid, 2)
    assert ((a == 1) & (b == 2)).any()                      # the boxes touch: faces between two owners
    u0, v0, w0 = F.velocity(ni, nj, nk, h)
    shapes = ((nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni))
    for spins in SPINS:
        entries = [Rotating(e, spin=s, orientation=(0.8, 0.1, 0.3, -0.2)) for e, s in zip(plain, spins)]
        want = faces(*(x.reshape(sh) for x, sh in zip((u0, v0, w0), shapes)), solid, entries, h)
        for with_delta in (True, False):
            vel = [x.copy() for x in (u0, v0, w0)]
            dl = [np.full_like(x, 5.0) for x in vel] if with_delta else [None, None, None]
            call_pose(*vel, *dl, solid, entries, h)
            for name, got, d, (new, delta, owned) in zip("uvw", vel, dl, want):
                assert np.array_equal(got.reshape(new.shape), new), (name, spins)
                if with_delta:
                    assert np.array_equal(d.reshape(new.shape), np.where(owned, delta, f32(5.0))), (name, spins)
            assert any((x != y).any() for x, y in zip(vel, (u0, v0, w0)))
    # zero spin (oriented or not): the values of gpu_obstacle_faces
    still = [Rotating(e, orientation=(0.8, 0.1, 0.3, -0.2)) for e in plain]
    vel, ref = [x.copy() for x in (u0, v0, w0)], [x.copy() for x in (u0, v0, w0)]
    d1, d2 = [np.full_like(x, 5.0) for x in vel], [np.full_like(x, 5.0) for x in vel]
    call_pose(*vel, *d1, solid, still, h)
    call_plain(*ref, *d2, solid, plain, h)
    for x, y in zip(vel + d1, ref + d2):
        assert np.array_equal(x, y)


def check_paddle(lib, errlib):
    """still fluid, the paddle of scenes.paddle: no spin, no motion; +omega and -omega stir the fluid their own way; the
    projected velocity is divergence-free on the fluid cells (DESIGN.md section 15's check)"""
    s = run_paddle(lib, errlib, 0.0)
    for name in ("u", "v", "w"):
        assert not s.field(name).any(), name
    assert s.solidMask().sum() > 100
    s.close()
    lz = {}
    for omega in (PADDLE_OMEGA, -PADDLE_OMEGA):
        s = run_paddle(lib, errlib, omega)
        lz[omega] = angular_momentum(s)
        assert all(np.isfinite(s.field(name)).all() for name in ("u", "v", "w", "rho"))
        PC.divergence_check(s, PADDLE_N)
        s.close()
    assert lz[PADDLE_OMEGA] > 0 > lz[-PADDLE_OMEGA], lz
    return lz
