"""fp64 reference of the obstacle operators, written from the definitions of DESIGN.md section 14 and not from the kernels
or their restatements (tests/cpu_abi/obstacle_abi.c, tests/obstacle_case.py): exact geometry with a near-tie mask, the
rows summary as a dilation, the masked Jacobi sweep as the Neumann stencil (sum over the fluid neighbours divided by
6 - s, no beta table), the solid faces, divergence, masked gradient, and host-built masks for the sweep operators.

Every operation below is float64; inputs are first rounded to the float32 values the C ABI receives.  Arrays are
(nk, nj, ni) (x fastest), like the device buffers.

Error bound of the float32 sweeps (derived, not fitted).  With u = 2^-24 and w_s = 1 / (6 - s), one float32 sweep of a
fluid cell computes fl(fl(sum of 7 terms) * beta_s): the seven-term left-to-right sum errs by at most 6 u * sum|terms|,
the product by u * |result|, and beta_s = (float)(1 / (1/beta - s)) with beta = (float)(1/6) differs from w_s by at most
(6 / (6 - s) + 1) u <= 7 u relatively.  So a sweep's own rounding is at most 14 u * M, M = max over written cells of
w_s * (sum|p_nb| + |alpha * div|), plus second-order terms.  The exact sweep is an average of the fluid neighbours with
weights w_s that sum to 1, so it does not amplify an error already present: after N sweeps the float32 iterate lies
within sum_n 16 u * M_n of the float64 one (M_n taken on the n-th float64 iterate; 16 instead of 14 covers the
second-order terms and the difference between M on the two iterates).  A perturbation d of div moves each sweep by at
most w_s |alpha d| <= |alpha d|, so a div that is itself off by D adds N |alpha| D.
"""
import numpy as np

U = 2.0 ** -24                 # float32 unit roundoff
TIE_ULPS = 16                  # near-tie width, in units of U times the magnitude scale of the compared quantity
ALPHA = -1.0


def f32(x):
    """the float an argument becomes at the C ABI, as a Python float"""
    return float(np.float32(x))


def beta32():
    return f32(1.0 / 6.0)


# ---- classification from geometry ------------------------------------------------------------------------------------
def _axis(n, staggered, h):
    return (np.arange(n, dtype=np.float64) - (0.5 if staggered else 0.0)) * f32(h)


def classify(boundaries, h, shape, stag=(0, 0, 0)):
    """(flag, tie) on a buffer of `shape` (nk, nj, ni) whose axis d is staggered when stag[d]: flag = o + 1 for the last
    obstacle o covering the node, -1 for a node in some obstacle's 3h band and inside none, 0 elsewhere; tie = the node
    lies within TIE_ULPS float32 ulps of some obstacle's solid or band threshold, where float32 may decide either way"""
    nk, nj, ni = shape
    x = _axis(ni, stag[0], h)[None, None, :]
    y = _axis(nj, stag[1], h)[None, :, None]
    z = _axis(nk, stag[2], h)[:, None, None]
    h3 = 3.0 * f32(h)
    owner = np.zeros(shape, np.int32)
    band = np.zeros(shape, bool)
    tie = np.zeros(shape, bool)
    for o, b in enumerate(boundaries):
        sh = int(b[0])
        c = [f32(v) for v in b[1:4]]
        r = [f32(v) for v in b[4:7]]
        d = [x - c[0], y - c[1], z - c[2]]
        mag = [np.abs(p) + abs(cc) for p, cc in zip((x, y, z), c)]          # |position| + |centre| per axis
        if sh == 0:
            d2 = d[0] ** 2 + d[1] ** 2 + d[2] ** 2
            scale = mag[0] ** 2 + mag[1] ** 2 + mag[2] ** 2
            R = r[0] + h3
            solid = d2 <= r[0] * r[0]
            inband = ~solid & (d2 < R * R)
            t = (np.abs(d2 - r[0] * r[0]) <= TIE_ULPS * U * (scale + r[0] * r[0])) | \
                (np.abs(d2 - R * R) <= TIE_ULPS * U * (scale + R * R))
        else:
            a = [np.abs(dd) - rr for dd, rr in zip(d, r)]
            amax = np.maximum(np.maximum(a[0], a[1]), a[2])
            solid = amax <= 0
            q = [np.maximum(aa, 0.0) for aa in a]
            d2 = q[0] ** 2 + q[1] ** 2 + q[2] ** 2
            inband = ~solid & (d2 > 0) & (d2 < h3 * h3)
            ta = TIE_ULPS * U * np.maximum(np.maximum(mag[0] + r[0], mag[1] + r[1]), mag[2] + r[2])
            qs = sum((m + rr) ** 2 for m, rr in zip(mag, r))
            t = (np.abs(amax) <= ta) | (np.abs(d2 - h3 * h3) <= TIE_ULPS * U * (qs + h3 * h3))
        owner = np.where(np.broadcast_to(solid, shape), o + 1, owner)
        band |= np.broadcast_to(inband, shape)
        tie |= np.broadcast_to(t, shape)
    return np.where(owner > 0, owner, np.where(band, -1, 0)), tie


def rows_of(solid):
    """rows summary, (nk, nj) uint8: 1 where a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1"""
    nk, nj, _ = solid.shape
    pad = np.pad((solid != 0).any(axis=2), 1)
    out = np.zeros((nk, nj), bool)
    for c in range(3):
        for b in range(3):
            out |= pad[c:c + nk, b:b + nj]
    return out.astype(np.uint8)


def rows_tie(tie):
    """(nk, nj): summary entries that a near-tie cell could flip"""
    return rows_of(tie) != 0


# ---- host-built masks ---------------------------------------------------------------------------------------------------
def mask_from_cells(dims, cells, value=1):
    """solid (nk, nj, ni) uint8 from (i, j, k) index triples"""
    ni, nj, nk = dims
    solid = np.zeros((nk, nj, ni), np.uint8)
    for i, j, k in cells:
        solid[k, j, i] = value
    return solid


def initial_p(solid, seed):
    """a float32 start iterate that meets the fused kernels' precondition: +0 in every solid cell and on the border
    layer (both ping-pong buffers start as copies of it)"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(solid.shape).astype(np.float32)
    p[solid != 0] = 0
    p[0], p[-1], p[:, 0], p[:, -1], p[:, :, 0], p[:, :, -1] = 0, 0, 0, 0, 0, 0
    return p


def neighbour_count(solid):
    """(nk-2, nj-2, ni-2) int: solid neighbours of each interior cell"""
    s = (solid != 0).astype(np.int32)
    return (s[1:-1, 1:-1, :-2] + s[1:-1, 1:-1, 2:] + s[1:-1, :-2, 1:-1] + s[1:-1, 2:, 1:-1]
            + s[:-2, 1:-1, 1:-1] + s[2:, 1:-1, 1:-1])


def codes(solid):
    """the per-cell code of the masked sweep on the interior: 7 for a solid cell, else its number of solid neighbours"""
    return np.where(solid[1:-1, 1:-1, 1:-1] != 0, 7, neighbour_count(solid))


def mask_families(dims, kchunk=8, rows_per_block=8, seed=0):
    """[(name, solid)]: the masks where this kernel family can go wrong.  Single solid cells at the row offsets
    jb - 4 .. jb + 4 around the first and the last row-block edge jb, and at the planes kb - 4 .. kb + 4 around the first
    chunk boundary kb (one cell per mask, so that the blocks around it are otherwise clean); solids on the first and last
    interior planes and rows and on the columns 0, 1, ni - 2, ni - 1; solids at i = 0 and i = 3 (mod 4) (and at 252 .. 255
    when ni = 256); a random mask of about 3 % with planted cells so that every code s = 0 .. 6 occurs"""
    ni, nj, nk = dims
    ic, kc, jc = ni // 2 + 1, nk // 2, nj // 2
    out = []
    edges = sorted({e for e in (rows_per_block, (nj - 1) // rows_per_block * rows_per_block) if 0 < e < nj})
    for jb in edges:
        for d in range(-4, 5):
            if 0 <= jb + d < nj:
                out.append((f"row {jb}{d:+d}", mask_from_cells(dims, [(ic, jb + d, kc)])))
    if kchunk < nk:
        for d in range(-4, 5):
            if 0 <= kchunk + d < nk:
                out.append((f"plane {kchunk}{d:+d}", mask_from_cells(dims, [(ic, jc, kchunk + d)])))
    walls = [(ic, jc, 1), (ic - 1, jc + 1, nk - 2), (ic, 1, kc), (ic + 1, nj - 2, kc)]
    walls += [(i, jc, kc) for i in (0, 1, ni - 2, ni - 1)] + [(i, 1, 1) for i in (0, 1, ni - 2, ni - 1)]
    out.append(("first/last planes, rows, wall columns", mask_from_cells(dims, walls)))
    for res in (0, 3):
        cells = [(i, 1 + (i // 4) % max(nj - 2, 1), 1 + (i // 8) % max(nk - 2, 1)) for i in range(res, ni, 4)]
        if ni == 256:
            cells += [(i, jc, kc) for i in range(252, 256)]
        out.append((f"i = {res} mod 4", mask_from_cells(dims, cells)))
    out.append(("random", random_mask(dims, seed)))
    return out


def random_mask(dims, seed, frac=0.03):
    """about `frac` solid cells at random, plus planted fluid cells with 4, 5 and 6 solid neighbours"""
    ni, nj, nk = dims
    rng = np.random.default_rng(seed)
    solid = (rng.random((nk, nj, ni)) < frac).astype(np.uint8)
    nbs = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    for s in (6, 5, 4, 6, 5, 4):
        i, j, k = (int(rng.integers(2, n - 2)) for n in (ni, nj, nk))
        solid[k, j, i] = 0
        for di, dj, dk in nbs[:s]:
            solid[k + dk, j + dj, i + di] = 1
        for di, dj, dk in nbs[s:]:
            solid[k + dk, j + dj, i + di] = 0
    return solid


# ---- the masked sweep ---------------------------------------------------------------------------------------------------
_NB = [(slice(1, -1), slice(1, -1), slice(None, -2)), (slice(1, -1), slice(1, -1), slice(2, None)),
       (slice(1, -1), slice(None, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1)),
       (slice(None, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1))]
_C = (slice(1, -1), slice(1, -1), slice(1, -1))


def masked_sweep(p, div, solid, alpha=ALPHA):
    """one sweep of the Neumann problem: an interior fluid cell with s solid neighbours takes (sum of its fluid
    neighbours + alpha div) / (6 - s), 0 when s = 6; solid and border cells keep their value.  Also returns
    M = max over the written cells of (sum|p_nb| + |alpha div|) / (6 - s), the scale of the float32 sweep's rounding."""
    p = np.asarray(p, np.float64)
    fluid = solid == 0
    acc = np.zeros(p[_C].shape)
    mag = np.zeros(p[_C].shape)
    for q in _NB:
        acc += np.where(fluid[q], p[q], 0.0)
        mag += np.abs(p[q])
    ad = alpha * np.asarray(div, np.float64)[_C]
    s = neighbour_count(solid)
    w = 1.0 / np.maximum(6 - s, 1)
    val = np.where(s == 6, 0.0, (acc + ad) * w)
    out = p.copy()
    out[_C] = np.where(fluid[_C], val, p[_C])
    written = fluid[_C] & (s < 6)
    m = float(((mag + np.abs(ad)) * w)[written].max()) if written.any() else 0.0
    return out, m


def masked_sweeps(p, div, solid, n, alpha=ALPHA):
    """[iterate 1, ..., iterate n] and the float32 error bound after each (module docstring)"""
    its, bounds, acc = [], [], 0.0
    cur = np.asarray(p, np.float64)
    for _ in range(n):
        cur, m = masked_sweep(cur, div, solid, alpha)
        acc += 16 * U * m
        its.append(cur)
        bounds.append(acc)
    return its, bounds


def neumann_system(div, solid, alpha=ALPHA, p_border=None):
    """(A, b, index) of the linear system whose fixed point the masked sweeps approach, on the interior fluid cells:
    (6 - s) p_c - sum over interior fluid neighbours p_nb = alpha div_c + sum over border neighbours p_border"""
    import scipy.sparse as sp
    nk, nj, ni = solid.shape
    interior = np.zeros(solid.shape, bool)
    interior[_C] = True
    unk = interior & (solid == 0)
    idx = -np.ones(solid.shape, np.int64)
    idx[unk] = np.arange(unk.sum())
    pb = np.zeros(solid.shape) if p_border is None else np.asarray(p_border, np.float64)
    rows, cols, vals = [], [], []
    b = alpha * np.asarray(div, np.float64)[unk]
    s = np.zeros(solid.shape, np.int64)
    s[_C] = neighbour_count(solid)
    kk, jj, ii = np.nonzero(unk)
    me = idx[unk]
    rows.append(me); cols.append(me); vals.append((6 - s[unk]).astype(np.float64))
    for dk, dj, di in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)):
        k2, j2, i2 = kk + dk, jj + dj, ii + di
        nb_unk = unk[k2, j2, i2]
        rows.append(me[nb_unk]); cols.append(idx[k2, j2, i2][nb_unk]); vals.append(-np.ones(nb_unk.sum()))
        on_border = ~interior[k2, j2, i2] & (solid[k2, j2, i2] == 0)
        np.add.at(b, me[on_border], pb[k2, j2, i2][on_border])
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(me.size, me.size))
    return A, b, unk


# ---- the rest of the projection -----------------------------------------------------------------------------------------
def face_owners(owner):
    """(ou, ov, ow): per face of the (ni+1, nj, nk), (ni, nj+1, nk), (ni, nj, nk+1) buffers the obstacle whose velocity
    it takes -- of the solid cell on either side, the later obstacle where both are solid -- or 0"""
    o = np.maximum(np.asarray(owner), 0)
    nk, nj, ni = o.shape
    ou = np.zeros((nk, nj, ni + 1), o.dtype); ou[:, :, 1:] = o; ou[:, :, :ni] = np.maximum(ou[:, :, :ni], o)
    ov = np.zeros((nk, nj + 1, ni), o.dtype); ov[:, 1:, :] = o; ov[:, :nj, :] = np.maximum(ov[:, :nj, :], o)
    ow = np.zeros((nk + 1, nj, ni), o.dtype); ow[1:] = o; ow[:nk] = np.maximum(ow[:nk], o)
    return ou, ov, ow


def face_cells(owner, comp):
    """(lo, hi): the owners of the two cells of every face of component comp (0 for a fluid cell or outside the grid)"""
    o = np.maximum(np.asarray(owner), 0)
    ax = 2 - comp
    shape = list(o.shape)
    shape[ax] += 1
    lo, hi = np.zeros(shape, o.dtype), np.zeros(shape, o.dtype)
    sl = [slice(None)] * 3
    sl[ax] = slice(1, None)
    lo[tuple(sl)] = o
    sl[ax] = slice(None, -1)
    hi[tuple(sl)] = o
    return lo, hi


def solid_faces(u, v, w, owner, boundaries):
    """step 1 of the projection: (u, v, w, du, dv, dw) after the solid face write, du = v_obstacle - u_before on the
    solid faces and NaN elsewhere (the operator leaves those delta entries alone)"""
    out, deltas = [], []
    for comp, (f, own) in enumerate(zip((u, v, w), face_owners(owner))):
        f = np.asarray(f, np.float64)
        vo = np.array([0.0] + [f32(b[7 + comp]) for b in boundaries])[own]
        out.append(np.where(own > 0, vo, f))
        deltas.append(np.where(own > 0, vo - f, np.nan))
    return out + deltas


def divergence(u, v, w, halfrdx):
    """div = halfrdx ((u_r - u_l) + (v_b - v_f) + (w_u - w_d)) and its float32 error bound per cell"""
    u, v, w = (np.asarray(a, np.float64) for a in (u, v, w))
    d = halfrdx * ((u[:, :, 1:] - u[:, :, :-1]) + (v[:, 1:, :] - v[:, :-1, :]) + (w[1:] - w[:-1]))
    mag = np.abs(halfrdx) * (np.abs(u[:, :, 1:]) + np.abs(u[:, :, :-1]) + np.abs(v[:, 1:, :]) + np.abs(v[:, :-1, :])
                             + np.abs(w[1:]) + np.abs(w[:-1]))
    return d, 7 * U * mag                  # three differences, two sums, one product


def gradient_masked(u, v, w, p, solid, halfrdx):
    """step 4: u -= halfrdx (p_c - p_left) on the faces of the window i, j, k in [2, n) whose two cells are fluid, every
    other face unchanged; returns (u, v, w, du, dv, dw, window masks): d = new - old on the updated faces, 0 on the
    other fluid faces, NaN on solid faces (left alone)"""
    p = np.asarray(p, np.float64)
    nk, nj, ni = p.shape
    fl = solid == 0
    res, deltas, wins = [], [], []
    for ax, f in zip((2, 1, 0), (u, v, w)):
        f = np.asarray(f, np.float64)
        n = f.shape[ax]
        both = np.zeros(f.shape, bool)               # both cells fluid (outside cells count as fluid)
        sl_lo = [slice(None)] * 3; sl_lo[ax] = slice(1, None)
        sl_hi = [slice(None)] * 3; sl_hi[ax] = slice(None, n - 1)
        lo = np.ones(f.shape, bool); lo[tuple(sl_lo)] = fl
        hi = np.ones(f.shape, bool); hi[tuple(sl_hi)] = fl
        both = lo & hi
        win = np.zeros(f.shape, bool)
        win[2:nk, 2:nj, 2:ni] = True                 # face index in [2, n) on every axis (the staggered one included)
        upd = win & both
        grad = np.zeros(f.shape)
        cut = [slice(2, nk), slice(2, nj), slice(2, ni)]
        prev = list(cut); prev[ax] = slice(cut[ax].start - 1, cut[ax].stop - 1)
        grad[tuple(cut)] = p[tuple(cut)] - p[tuple(prev)]
        new = np.where(upd, f - halfrdx * grad, f)
        res.append(new)
        deltas.append(np.where(upd, new - f, np.where(both, 0.0, np.nan)))
        wins.append(upd)
    return res + deltas + wins


# ---- scenes for the flags, the band and the projection ------------------------------------------------------------------
def edge_scene(dims):
    """(h, boundaries) on `dims`: centres off the grid, a sphere cut by the x = 0 wall, a box cut by the y = top wall, and
    a box overlapping a sphere (the later one owns the shared cells); every obstacle has its own velocity on every axis"""
    ni, nj, nk = dims
    h = 1.0 / ni
    X, Y, Z = ni * h, nj * h, nk * h
    m = min(Y, Z)
    return h, [(0, 0.0317 * X, 0.4713 * Y, 0.5291 * Z, 0.21 * m, 0, 0, 0.31, -0.22, 0.13),
               (0, 0.6093 * X, 0.4687 * Y, 0.5213 * Z, 0.2317 * m, 0, 0, -0.05, 0.47, 0.02),
               (1, 0.6611 * X, 0.5349 * Y, 0.4471 * Z, 0.0913 * X, 0.1713 * Y, 0.1287 * Z, -0.41, 0.06, 0.23),
               (1, 0.2977 * X, 0.9683 * Y, 0.3917 * Z, 0.0731 * X, 0.1109 * Y, 0.2043 * Z, 0.17, -0.33, -0.29)]
