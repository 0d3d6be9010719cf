"""Shared pieces of the tests of the density preview with solid obstacles: the loader of the CPU
stand-in with gpu_render_density_solids, calls of the restatement, a seeded flag generator whose forced solids make every
image hold every kind of pixel, and a second, independent restatement of one ray in numpy scalars.

No tolerance anywhere: every accumulated quantity of the contract is an integer below 2^53, so every comparison is on bits."""
import ctypes as C
import struct

import numpy as np

import obstacle_case as OC
import render_case as R
from build_cpu_render_solids import build_render_solids

f32 = np.float32
TWO32 = R.TWO32
VP = C.c_void_p
WALL = 0x80
SOLID_ALBEDO, SOLID_AMBIENT = 0.625, 0.1875


def load_render_solids():
    """the stand-in with every restated operator, gpu_render_density and gpu_render_density_solids among them"""
    from gpufluidsimulation_amd import _lib
    lib = OC._load(build_render_solids(), OC.OPS + OC.LS_OPS + ("gpu_emit_sources", "gpu_maccormack", "gpu_flow_stats",
                                                                "gpu_render_density", "gpu_render_density_solids"))
    lib.render_abi_calls.restype, lib.render_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.render_solids_abi_calls.restype, lib.render_solids_abi_calls.argtypes = C.c_long, [C.c_int]
    lib.render_solids_abi_set_slab.restype, lib.render_solids_abi_set_slab.argtypes = None, [C.c_int]
    lib.orc_expf.restype, lib.orc_expf.argtypes = C.c_float, [C.c_float]
    for name in ("fl_set_option", "fl_get_option", "fl_memcpy_d2h", "fl_memcpy_h2d"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.HIP_SIGS[name]
    return lib


def solid_params(albedo=SOLID_ALBEDO, ambient=SOLID_AMBIENT):
    """fl_render_solid_params as a host buffer (keep the returned object alive for the call)"""
    return C.create_string_buffer(struct.pack("ff", albedo, ambient))


def restate(lib, rho, flags, dims, h, view, light, sigma=6.0, albedo=1.0, ambient=0.1, sa=SOLID_ALBEDO, sb=SOLID_AMBIENT, rows=None):
    """the restatement on host arrays: (rc, image (3, H, W) float64, shadow (nk, nj, ni) float32 or None)"""
    ni, nj, nk = dims
    H, W = R.image_shape(dims, view)
    img = np.full((3, H, W), -1.0)
    shadow = np.full((nk, nj, ni), 7.0, f32) if light >= 0 else None
    p, sp = R.params(sigma, albedo, ambient), solid_params(sa, sb)
    rc = lib.gpu_render_density_solids(rho.ctypes.data, flags.ctypes.data, None if rows is None else rows.ctypes.data,
                                       None if shadow is None else shadow.ctypes.data, h, ni, nj, nk, view, light,
                                       C.cast(p, VP), C.cast(sp, VP), img.ctypes.data)
    return rc, img, shadow


def travel_coords(nt, x_axis):
    """the coordinates of the forced solids along an axis of nt cells: travel positions 0, nt - 1, 4 and 5 (they straddle a
    chunk of 5) of both directions, along x also 63 and 64 (the seam of two wave segments)"""
    pos = [0, nt - 1, 4, 5] + ([63, 64] if x_axis else [])
    out = []
    for t in pos:
        for c in (t, nt - 1 - t):
            if 0 <= c < nt and c not in out:
                out.append(c)
    return out


def reserved_rays(dims):
    """the rays that hold ONE forced solid each (or none: coordinate None), as (axis, (a, b), coordinate) with (a, b) the two
    other coordinates in increasing axis order.  Rays of different axes never cross: x rays use k in 0..2 and j in 0..3, y
    rays k in 3..5 and i in 0..2, z rays j in 4..7 and i in 3..5"""
    ni, nj, nk = dims
    assert ni >= 6 and nj >= 8 and nk >= 6
    slots = {0: [(j, k) for k in range(3) for j in range(4)],           # (j, k)
             1: [(i, k) for k in range(3, 6) for i in range(3)],        # (i, k)
             2: [(i, j) for j in range(4, 8) for i in range(3, 6)]}     # (i, j)
    out = []
    for axis in range(3):
        coords = travel_coords(dims[axis], axis == 0) + [None]
        assert len(coords) <= len(slots[axis])
        out += [(axis, slots[axis][n], c) for n, c in enumerate(coords)]
    return out


def _ray_index(axis, ab, c):
    """the numpy index (k, j, i) of cell c (or slice(None): the whole ray) of a reserved ray"""
    a, b = ab
    return {0: (b, a, c), 1: (b, c, a), 2: (c, b, a)}[axis]


def flags(dims, seed=0):
    """flags (nk, nj, ni) uint8: sparse clusters of up to 2 x 2 x 2 cells with tags 1..16, some of them with the wall bit on
    top, some cells with the wall bit ONLY (not solid), and the forced solids of reserved_rays on otherwise empty rays; frozen"""
    ni, nj, nk = dims
    rng = np.random.default_rng(1000 + seed)
    fl = np.zeros((nk, nj, ni), np.uint8)
    for n in range(max(4, ni * nj * nk // 1500)):
        k, j, i = (int(rng.integers(0, n)) for n in (nk, nj, ni))
        ek, ej, ei = (int(rng.integers(1, 3)) for _ in range(3))
        fl[k:k + ek, j:j + ej, i:i + ei] = int(rng.integers(1, 17)) | (WALL if n % 4 == 0 else 0)
    wall_only = (rng.random((nk, nj, ni)) < 0.03) & (fl == 0)
    fl[wall_only] = WALL
    rays = reserved_rays(dims)
    for axis, ab, c in rays:
        fl[_ray_index(axis, ab, slice(None))] = 0
    for n, (axis, ab, c) in enumerate(rays):
        if c is not None:
            fl[_ray_index(axis, ab, c)] = (1 + n % 16) | (WALL if n % 5 == 0 else 0)
    for axis, ab, c in rays:
        assert int(((fl[_ray_index(axis, ab, slice(None))] & 0x7f) != 0).sum()) == (c is not None)
    fl.setflags(write=False)
    return fl


def density(dims, seed=0):
    """render_case.density with smoke (0.25) all along the reserved rays, so that a forced solid past the first cell has smoke
    in front, and with a NaN and a huge value inside two of the forced solids; frozen"""
    rho = R.density(dims, seed).copy()
    for n, (axis, ab, c) in enumerate(reserved_rays(dims)):
        rho[_ray_index(axis, ab, slice(None))] = 0.25
        if c is not None and n % 3 == 0:
            rho[_ray_index(axis, ab, c)] = np.nan if n % 2 else 1e30
    rho.setflags(write=False)
    return rho


def rows_summary(fl):
    """the obstacles' rows summary (nk, nj) uint8: 1 when a solid cell lies in rows j - 1 .. j + 1 of the plane"""
    has = ((fl & 0x7f) != 0).any(axis=2)
    out = has.copy()
    out[:, 1:] |= has[:, :-1]
    out[:, :-1] |= has[:, 1:]
    return np.ascontiguousarray(out.astype(np.uint8))


def travel(a, code):
    """the volume (nk, nj, ni) with the ray axis of a direction code last and in travel order: [row, col, t]"""
    axis = {0: 2, 1: 1, 2: 0}[code // 2]
    moved = np.moveaxis(a, axis, -1)
    return moved[..., ::-1] if code & 1 else moved


def pixel_kinds(rho, fl, sh, view):
    """per pixel of a view, from the arrays alone: (hit, first, last, front) boolean (H, W) images -- the ray meets a solid;
    its first solid is the ray's first cell; its first solid is the ray's last cell; a fluid cell with D != 0 lies before it"""
    s = (travel(fl, view) & 0x7f) != 0
    with np.errstate(all="ignore"):
        d = np.minimum(f32(sh) * np.maximum(np.nan_to_num(travel(rho, view), nan=0.0), f32(0)), f32(32))
    dense = (np.trunc(d.astype(np.float64) * TWO32) != 0) & ~s
    hit = s.any(axis=-1)
    first_at = np.where(hit, s.argmax(axis=-1), s.shape[-1])
    before = np.arange(s.shape[-1])[None, None, :] < first_at[..., None]
    return hit, hit & (first_at == 0), hit & (first_at == s.shape[-1] - 1), hit & (dense & before).any(axis=-1)


def ray(expf, rhos, tags, sh, shadows=None, albedo=1.0, ambient=0.1, sa=SOLID_ALBEDO, sb=SOLID_AMBIENT):
    """one ray restated a second time, cell by cell in travel order: (Cfix, Afix, Hfix, [att'(A, B) per cell]) as Python ints
    / float32; tags: the flag bytes; shadows: s per cell (None: 1.0f)"""
    sh, albedo, ambient, sa, sb = f32(sh), f32(albedo), f32(ambient), f32(sa), f32(sb)
    A, B, Cfix, Hfix, tvs = 0, False, 0, 0, []
    with np.errstate(all="ignore"):
        for n, rho in enumerate(rhos):
            Tv = f32(0.0) if B else R.att(expf, float(A))
            tvs.append(Tv)
            s = f32(1.0) if shadows is None else f32(shadows[n])
            tag = int(tags[n]) & 0x7f
            if tag:
                qs = f32(f32(sa * s) + sb)
                Cfix += int(np.trunc(float(Tv) * float(qs) * TWO32))
                if not Hfix:
                    Hfix = tag
                B = True
                continue
            r = f32(rho) if f32(rho) > 0 else f32(0.0)
            t = f32(sh * r)
            d = f32(32.0) if not (t <= f32(32.0)) else t
            D = int(np.trunc(float(d) * TWO32))
            a = f32(f32(1.0) - f32(expf(float(-d))))
            q = f32(a * f32(f32(albedo * s) + ambient))
            Cfix += int(np.trunc(float(Tv) * float(q) * TWO32))
            A += D
    return Cfix, A, Hfix, tvs


def convert(expf, img):
    """the host's conversion of the planes (Cfix, Afix, Hfix): (radiance, transmittance float32, hit uint8), each (H, W)"""
    rad, tr = R.convert(expf, img[:2])
    tr = np.where(img[2] != 0, f32(0.0), tr).astype(f32)
    return rad, tr, img[2].astype(np.uint8)
