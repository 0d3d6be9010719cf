"""Inputs shared by the FL_OPT_SKIP_EMPTY_BRICKS tests (GPU and CPU): sparse scalar pairs, maps, and the numpy restatement
of the skip criterion (gpufluidsimulation_amd/csrc/bq_sparse.hip.h)."""
import numpy as np

import fields as F
from host_entry_case import wild_maps

SHAPES = [(80, 24, 16), (24, 20, 16), (32, 32, 32)]
H = float(np.float32(1.0 / 32))
BRICK = 8


def cube(ni, nj, nk, lo, hi, phase):
    """a smooth non-zero blob on the nodes lo <= i, j, k < hi (hi cut to the array), flat"""
    a = np.zeros((nk, nj, ni), np.float32)
    full = (F.scalar(ni, nj, nk, phase).reshape(nk, nj, ni) + np.float32(2.0)).astype(np.float32)      # never zero
    a[lo:hi, lo:hi, lo:hi] = full[lo:hi, lo:hi, lo:hi]
    return a


def sources(name, ni, nj, nk):
    """the two sampled fields of a case, flat float32"""
    a = np.zeros((nk, nj, ni), np.float32)
    b = np.zeros((nk, nj, ni), np.float32)
    if name == "zero":
        pass
    elif name == "node777":
        a[7, 7, 7] = 1.0
    elif name == "node888":
        a[8, 8, 8] = 1.0; b[8, 8, 8] = -3.0
    elif name == "blob_face":            # support ends exactly on brick faces
        a = cube(ni, nj, nk, 8, 16, 0.4); b = cube(ni, nj, nk, 8, 16, 1.9)
    elif name == "blob_inside":          # ... and inside a brick
        a = cube(ni, nj, nk, 9, 14, 0.4); b = cube(ni, nj, nk, 9, 14, 1.9)
    elif name == "one_field":
        b = cube(ni, nj, nk, 9, 14, 1.9)
    elif name == "specials":             # words that are not 0x00000000 but compare equal to zero, or poison a lerp
        a[3, 4, 5] = -0.0
        a[9, 10, 11] = np.float32(1e-42)
        b[4, 12, 14] = np.nan
        b[12, 5, 20 % ni] = np.inf
    elif name == "row_end":              # the last index of a row and of a plane
        a[6:10, 9:13, ni - 3:ni] = 1.5
        b[5:9, nj - 2:nj, 2:9] = -2.5
    elif name == "dense":
        a = (F.scalar(ni, nj, nk, 0.4).reshape(nk, nj, ni) + np.float32(2.0)).astype(np.float32)
        b = (F.scalar(ni, nj, nk, 1.9).reshape(nk, nj, ni) - np.float32(3.0)).astype(np.float32)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(a.ravel()), np.ascontiguousarray(b.ravel())


CASES = ["zero", "node777", "node888", "blob_face", "blob_inside", "one_field", "specials", "row_end", "dense"]


def targets(ni, nj, nk, src_a, src_b):
    """what the accumulate adds into / the error stage subtracts: dense, with -0.0f and NaN on nodes where the sources are empty"""
    d1, d2 = F.scalar(ni, nj, nk, 0.7), F.scalar(ni, nj, nk, 2.9, amp=0.5)
    empty = np.flatnonzero((src_a.view(np.uint32) == 0) & (src_b.view(np.uint32) == 0))
    d1[empty[::7]] = -0.0
    d1[empty[3::11]] = np.nan
    d2[empty[1::5]] = -0.0
    return d1, d2


def jump_maps(ni, nj, nk, h, phase):
    """a smooth map whose x component jumps by more than a brick in the middle of every row (inside one block)"""
    maps = F.warped_maps(ni, nj, nk, h, 0.8, phase)
    x = maps[0].reshape(nk, nj, ni).copy()
    lo, hi = ni // 2 - 2, ni // 2 + 2
    x[2:nk - 2, 2:nj - 2, lo:hi] = np.minimum(x[2:nk - 2, 2:nj - 2, lo:hi] + np.float32(10 * h), np.float32((ni - 1) * h))
    return [np.ascontiguousarray(x.ravel()), maps[1], maps[2]]


def maps_of(kind, ni, nj, nk, h, phase):
    if kind == "smooth":
        return F.warped_maps(ni, nj, nk, h, 0.8, phase)
    if kind == "wild":
        return wild_maps(ni, nj, nk, h, phase)
    return jump_maps(ni, nj, nk, h, phase)


def brick_flags(fields, ni, nj, nk):
    """numpy statement of the flag pass: [bz, by, bx] = 1 when any word of any field in the brick is not 0x00000000"""
    nbx, nby, nbz = -(-ni // BRICK), -(-nj // BRICK), -(-nk // BRICK)
    occ = np.zeros((nk, nj, ni), bool)
    for f in fields:
        occ |= f.view(np.uint32).reshape(nk, nj, ni) != 0
    pad = np.zeros((nbz * BRICK, nby * BRICK, nbx * BRICK), bool)
    pad[:nk, :nj, :ni] = occ
    return pad.reshape(nbz, BRICK, nby, BRICK, nbx, BRICK).any(axis=(1, 3, 5)).astype(np.uint8)


def block_skips(maps, flags, ni, nj, nk, h, win, lo, hi):
    """The criterion, block by block: tile range -> clamp -> cells -> widened brick range -> flags.
    win: the operator's index window is win < i < n - 1 - win (2 for the advection, 1 for the other two); lo / hi: its clamp
    (per axis).  Returns {(bx, by, k): skipped} for every block that has a node inside the window."""
    f32 = np.float32
    m3 = [m.reshape(nk, nj, ni) for m in maps]
    dims = (ni, nj, nk)
    out = {}
    for k in range(win + 1, nk - 1 - win):
        for j0 in range(0, nj, 4):
            for i0 in range(0, ni, 64):
                ys = [j for j in range(j0, min(j0 + 4, nj)) if win < j < nj - 1 - win]
                xs = [i for i in range(i0, min(i0 + 64, ni)) if win < i < ni - 1 - win]
                if not ys or not xs:
                    continue
                sl = (slice(k - 1, k + 2), slice(ys[0] - 1, ys[-1] + 2), slice(xs[0] - 1, xs[-1] + 2))
                rng, ok = [], True
                for a in range(3):
                    v = m3[a][sl]
                    if not np.isfinite(v).all():
                        ok = False
                        break
                    mn, mx = f32(v.min()), f32(v.max())
                    with np.errstate(over="ignore", invalid="ignore"):
                        e = f32(2.0 ** -21) * f32(f32(mx - mn) + max(abs(mn), abs(mx)))
                        pa = min(max(f32(mn - e), f32(lo[a])), f32(hi[a]))
                        pb = min(max(f32(mx + e), f32(lo[a])), f32(hi[a]))
                    if np.isnan(pa) or np.isnan(pb):
                        ok = False
                        break
                    rng.append((int(np.floor(f32(pa) / f32(h))), int(np.floor(f32(pb) / f32(h)))))      # h = 2^-m: exact
                if not ok:
                    out[(i0 // 64, j0 // 4, k)] = False
                    continue
                (x0, x1), (y0, y1), (z0, z1) = [(max(c0 - 1, 0), c1 + 2) for c0, c1 in rng]
                if x1 > ni - 1:
                    x0, x1, y1 = 0, ni - 1, y1 + 1
                if y1 > nj - 1:
                    y0, y1, z1 = 0, nj - 1, z1 + 1
                z1 = min(z1, nk - 1)
                if x0 > x1 or y0 > y1 or z0 > z1:
                    out[(i0 // 64, j0 // 4, k)] = False
                    continue
                bx0, bx1, by0, by1, bz0, bz1 = x0 >> 3, x1 >> 3, y0 >> 3, y1 >> 3, z0 >> 3, z1 >> 3
                if (by1 - by0 + 1) * (bz1 - bz0 + 1) * ((bx1 - bx0 + 64) >> 6) > 8:
                    out[(i0 // 64, j0 // 4, k)] = False
                    continue
                out[(i0 // 64, j0 // 4, k)] = not flags[bz0:bz1 + 1, by0:by1 + 1, bx0:bx1 + 1].any()
    return out
