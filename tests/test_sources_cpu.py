"""Shaped, moving smoke sources without a GPU: the C restatement of gpu_emit_sources
(tests/cpu_abi/source_abi.c) against the numpy restatement (tests/source_case.py), and the host solver's source path --
motion, activity, state elision, re-initialisation policy, obstacles, refusals -- on the CPU stand-in that has the
operator (tests/build_cpu_sources.py)."""
import ctypes as C
import hashlib
import re

import numpy as np
import pytest

import levelset_case as LC
import obstacle_case as OC
import source_case as SC

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return SC.load_sources()


def make(lib, n=24, scheme=0, iters=20, dims=None):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    ni, nj, nk = dims or (n, n, n)
    s = BimocqGPUSolver(ni, nj, nk, 1.0, 0.0, 1.0, lib=lib, errlib=lib, scheme=scheme)
    s.setSmoke(0.0, 1.0, [])
    s.setProjection(iters, 0.5)
    return s


def both(lib, dims, h, sources):
    """(numpy restatement, C restatement, untouched pattern) on pre-filled fields"""
    return SC.emit(SC.pattern(dims), sources, h, dims), SC.emit_c(lib, SC.pattern(dims), sources, h, dims), SC.pattern(dims)


@pytest.mark.parametrize("dims", [(37, 29, 23), (99, 21, 18)])
def test_c_restatement_equals_numpy(lib, dims):
    h, sources = SC.mixed(dims)
    a, b, p = both(lib, dims, h, sources)
    for name in SC.NAMES:
        assert np.array_equal(a[name], b[name]), name
        touched = a[name] != p[name]
        assert 100 < touched.sum() < 0.5 * touched.size, name       # something written, most nodes untouched
    # every entry alone writes what the contract says, and the last one (wholly outside the domain) writes nothing
    for o, s in enumerate(sources):
        a, b, p = both(lib, dims, h, [s])
        for name in SC.NAMES:
            assert np.array_equal(a[name], b[name]), (o, name)
            changed = bool((a[name] != p[name]).any())
            if o == len(sources) - 1 or (name in "uvw" and s.velocity is None):
                assert not changed, (o, name)
            else:
                assert changed, (o, name)


@pytest.mark.parametrize("dims", [(37, 29, 23), (99, 21, 18)])
def test_last_source_wins_and_unflagged_sources_leave_velocity_alone(lib, dims):
    """entries 0 (sphere, flag), 1 (box, no flag), 2 (level-set sphere, flag) of the mixed list overlap"""
    h, sources = SC.mixed(dims)
    s0, s1, s2 = sources[:3]
    shp = SC.shapes(dims)
    got = SC.emit_c(lib, SC.pattern(dims), [s0, s1, s2], h, dims)
    only0 = SC.emit_c(lib, SC.pattern(dims), [s0], h, dims)
    win = {}
    ins = {}
    for name in SC.NAMES:
        nk, nj, ni = shp[name]
        w = np.zeros(shp[name], bool)
        w[2:nk - 2, 2:nj - 2, 2:ni - 2] = True
        win[name] = w
        ins[name] = [SC.inside(s, s.position, h, shp[name], SC.STAG[name]) & w for s in (s0, s1, s2)]
    i0, i1, i2 = ins["rho"]
    assert (i0 & i1 & ~i2).sum() > 5 and (i1 & i2).sum() > 5 and (i0 & i2).sum() > 0
    rho = got["rho"].reshape(shp["rho"])
    assert np.all(rho[i2] == f32(s2.density)) and np.all(rho[i1 & ~i2] == f32(s1.density))
    assert np.all(rho[i0 & ~i1 & ~i2] == f32(s0.density))
    for name in "uvw":
        j0, j1, j2 = ins[name]
        a, b = got[name].reshape(shp[name]), only0[name].reshape(shp[name])
        m = j0 & j1 & ~j2
        assert m.sum() > 5
        assert np.array_equal(a[m], b[m]), name                       # the unflagged box left the sphere's velocity alone
        m = j1 & ~j0 & ~j2
        assert m.sum() > 5
        assert np.array_equal(a[m], SC.pattern(dims)[name].reshape(shp[name])[m]), name    # and wrote none of its own
        m = j0 & j2
        assert not np.array_equal(a[m], b[m]), name                   # the later flagged source overwrote it


def test_window_cut_and_order_of_the_velocity_expression(lib):
    dims = (37, 29, 23)
    h, sources = SC.mixed(dims)
    shp = SC.shapes(dims)
    cut = sources[3]                                                   # the level-set box at the x = 0 wall
    got = SC.emit_c(lib, SC.pattern(dims), [cut], h, dims)
    p = SC.pattern(dims)
    for name in SC.NAMES:
        nk, nj, ni = shp[name]
        touched = (got[name] != p[name]).reshape(shp[name])
        inside = SC.inside(cut, cut.position, h, shp[name], SC.STAG[name])
        assert inside[:, :, :2].any(), name                           # the shape does reach the two wall layers
        assert not touched[:, :, :2].any() and touched[:, :, 2].any(), name
    # v = ey + (oz dx - ox dz), one float operation each
    nk, nj, ni = shp["v"]
    k, j, i = np.argwhere((got["v"] != p["v"]).reshape(shp["v"]))[7]
    x, z = f32(f32(i) * f32(h)), f32(f32(k) * f32(h))
    dx, dz = f32(x - f32(cut.position[0])), f32(z - f32(cut.position[2]))
    want = f32(f32(cut.velocity[1]) + f32(f32(f32(cut.spin[2]) * dx) - f32(f32(cut.spin[0]) * dz)))
    assert got["v"].reshape(shp["v"])[k, j, i] == want


def test_levelset_sphere_source_equals_the_analytic_sphere_source(lib):
    """Bound (tests/test_levelsets_cpu.py): trilinear interpolation of d = |x| - r errs by at most
    E = voxel^2 / (4 (r - sqrt(3) voxel)); nodes farther than E from the surface must agree.  n = 64, r = 0.2, position
    (0.5, 0.45, 0.52): the excluded shell holds at most 2 % of the nodes inside the sphere on each node kind."""
    from gpufluidsimulation_amd.solver import Source, levelset_sphere
    n = 64
    h = 1.0 / n
    dims = (n, n, n)
    r, c = 0.2, (0.5, 0.45, 0.52)
    kw = dict(velocity=(0.1, 0.4, -0.2), spin=(0.2, 0.0, 1.0))
    a = SC.emit_c(lib, SC.pattern(dims), [Source(("sphere", r), c, 1.0, 2.0, 1, **kw)], h, dims)
    b = SC.emit_c(lib, SC.pattern(dims), [Source(levelset_sphere(r, h), c, 1.0, 2.0, 1, **kw)], h, dims)
    E = h * h / (4 * (r - np.sqrt(3) * h))
    shp = SC.shapes(dims)
    for name in SC.NAMES:
        nk, nj, ni = shp[name]
        st = SC.STAG[name]
        x, y, z = (OC.positions(m, s, h).astype(np.float64) for m, s in zip((ni, nj, nk), st))
        d = np.sqrt((x[None, None, :] - c[0]) ** 2 + (y[None, :, None] - c[1]) ** 2 + (z[:, None, None] - c[2]) ** 2) - r
        keep = np.abs(d) > E
        inside = int((d <= 0).sum())
        excluded = int((~keep).sum())
        print(f"{name}: E = {E / h:.4f} h, excluded {excluded} = {100.0 * excluded / inside:.2f} % of {inside} nodes inside")
        assert excluded <= 0.02 * inside, name
        A, B = a[name].reshape(shp[name]), b[name].reshape(shp[name])
        assert np.array_equal(A[keep], B[keep]), name
        assert (A != SC.pattern(dims)[name].reshape(shp[name])).sum() > 0.9 * inside


def footprint(lib, n, scheme, source, dt):
    """rho == density after advance(0) of a solver at rest without buoyancy: exactly the cells the source wrote"""
    s = make(lib, n, scheme, iters=4)
    s.setSmoke(0.0, 0.0, [])
    s.setSources([source])
    s.advance(0, dt)
    m = s.field("rho").reshape(n, n, n) == f32(source.density)
    pos = s.sourcePositions()[0]
    s.close()
    return m, pos


@pytest.mark.parametrize("scheme", [0, 3])
def test_emission_happens_at_the_moved_position(lib, scheme):
    """move first, then emit: dyadic h, voxel = h, v dt = h, so after advance(0) the footprint is the start position's
    shifted by exactly one cell -- the numpy restatement at start + v dt, not the one at the start, and what a static
    source placed at start + v dt writes"""
    from gpufluidsimulation_amd.solver import Source, levelset_sphere
    n = 32
    h = 1.0 / n
    dt = 2 * h
    start = (0.40625, 0.5, 0.53125)
    ls = levelset_sphere(0.15, h)
    moving = Source(ls, start, 1.0, 1.0, 1, motion=(0.5, 0.0, 0.0))
    got, pos = footprint(lib, n, scheme, moving, dt)
    end = tuple(f32(f32(c) + f32(v) * f32(dt)) for c, v in zip(start, moving.motion))
    assert np.array_equal(pos, np.array(end, f32)) and float(end[0]) == start[0] + h
    win = np.zeros((n, n, n), bool)
    win[2:n - 2, 2:n - 2, 2:n - 2] = True
    at_start = SC.inside(moving, start, h, (n, n, n), (0, 0, 0)) & win
    at_end = SC.inside(moving, end, h, (n, n, n), (0, 0, 0)) & win
    assert at_start.sum() > 400 and not np.array_equal(at_start, at_end)
    assert np.array_equal(got, at_end)
    assert np.array_equal(got[:, :, 1:], at_start[:, :, :-1]) and not got[:, :, 0].any()
    static, _ = footprint(lib, n, scheme, Source(ls, tuple(float(c) for c in end), 1.0, 1.0, 1), dt)
    assert np.array_equal(got, static)


@pytest.mark.parametrize("scheme", [0, 3])
def test_sources_move_once_per_step_active_or_not(lib, scheme):
    """k float accumulations of v dt after k steps, in both schemes; a source past emit_frames still moves and writes
    nothing"""
    from gpufluidsimulation_amd.solver import Source, levelset_sphere
    n = 32
    h = 1.0 / n
    dt = 2 * h
    motion = (0.5, 0.0, 0.0)
    srcs = [Source(levelset_sphere(0.15, h), (0.40625, 0.5, 0.53125), 1.0, 1.0, 2, motion=motion),
            Source(("sphere", 0.05), (0.3, 0.31, 0.29), 1.0, 1.0, 100, motion=(0.013, -0.007, 0.0031))]
    s = make(lib, n, scheme, iters=4)
    s.setSources(srcs)
    assert np.array_equal(s.sourcePositions(), np.array([src.position for src in srcs], f32))
    want = np.array([src.position for src in srcs], f32)
    mot = np.array([src.motion for src in srcs], f32)
    for f in range(6):
        if f == 5:
            before = {nm: s.field(nm).copy() for nm in ("rho", "T")}
            s.setSources([Source(srcs[0].levelset, tuple(want[0]), 7.0, 7.0, 2, velocity=(1.0, 1.0, 1.0), motion=motion)])
            want, mot = want[:1], mot[:1]
        s.advance(f, dt)
        want = (want + mot * f32(dt)).astype(f32)
        assert np.array_equal(s.sourcePositions(), want), f
    assert not (s.field("rho") == 7.0).any() and not (s.field("T") == 7.0).any()
    assert before["rho"].max() > 0
    s.close()


VEL_SOURCE = dict(shape=("box", (0.12, 0.1, 0.1)), position=(0.5, 0.3, 0.33), density=1.0, temperature=1.0, emit_frames=1000,
                  velocity=(0.3, 0.5, -0.2), spin=(0.0, 2.0, 1.0))


def run_velocity_source(lib, scheme, full=0, policy=0, emitters=()):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver, Source
    dims = (24, 20, 16)
    s = BimocqGPUSolver(*dims, 1.0, 0.0, 1.0, lib=lib, errlib=lib, scheme=scheme)
    s.setSmoke(0.0, 1.0, list(emitters))
    s.setProjection(20, 0.5)
    s.setOption(3, full)
    s.setOption(2, policy)
    s.setSources([Source(**VEL_SOURCE)])
    for f in range(6):
        s.advance(f, 0.5 / dims[0])
    out = {nm: s.field(nm) for nm in SC.NAMES}
    s.close()
    return out


@pytest.mark.parametrize("scheme", [0, 3])
def test_state_elision_keeps_a_velocity_source(lib, scheme):
    """with a velocity source the default state elision and BQ_OPT_FULL_STATE = 1 give the same fields.  This is NOT the
    guard of forces_touch_uw: BQ_OPT_FULL_STATE does not force the u and w force deltas, so both runs would drop them
    alike.  test_velocity_source_keeps_the_u_and_w_force_deltas below is the one that fails without that line."""
    a, b = run_velocity_source(lib, scheme, full=0), run_velocity_source(lib, scheme, full=1)
    for nm in SC.NAMES:
        assert np.array_equal(a[nm], b[nm], equal_nan=True), nm
        assert np.isfinite(a[nm]).all()
    assert np.abs(a["u"]).max() > 0.05 and np.abs(a["w"]).max() > 0.05


def test_velocity_source_keeps_the_u_and_w_force_deltas(lib):
    """forces_touch_uw: with maps that live for several steps (policy 1) the u and w changes a velocity source makes must
    reach the accumulation.  The yardstick is the same run with a legacy emitter that is active and lies wholly outside the
    domain: it writes nothing, and it has always kept the u and w snapshots and deltas alive."""
    outside = [(0.5, 9.0, 0.5, 0.1, 1.0, 1.0, 0.0, 1000)]
    a = run_velocity_source(lib, 0, policy=1)
    b = run_velocity_source(lib, 0, policy=1, emitters=outside)
    for nm in SC.NAMES:
        assert np.array_equal(a[nm], b[nm], equal_nan=True), nm
    assert np.abs(a["u"]).max() > 0.05


@pytest.mark.parametrize("scheme", [0, 3])
def test_policy_one_and_obstacles(lib, scheme):
    n = 24
    h, sources, obstacles = SC.scene(n)
    # policy 1: emission reaches DensityInit through the accumulation
    s = make(lib, dims=(24, 20, 16), scheme=scheme)
    s.setOption(2, 1)
    s.setSources(sources[1:])
    for f in range(3):
        s.advance(f, 0.5 / 24)
    assert s.field("rho").max() > 0.4
    if scheme == 0:
        assert s.field("rhoinit").max() > 0.4
    s.close()
    # sources together with a level-set obstacle
    from gpufluidsimulation_amd.solver import LevelSetObstacle
    dims = (24, 20, 16)
    for src in sources:                                                # the scene of the cube, centred in this grid's z
        src.position = src.position[:2] + (0.33,)
    s = make(lib, dims=dims, scheme=scheme)
    s.setBoundary([LevelSetObstacle(obstacles[0].levelset, (0.5, 0.55, 0.33))])
    s.setSources(sources)
    for f in range(4):
        s.advance(f, 0.5 / n)
    solid = s.solidMask().astype(bool)
    rho = s.field("rho").reshape(dims[::-1])
    assert solid.sum() > 50 and np.all(rho[solid] == 0) and rho.max() >= 1.0
    for nm in SC.NAMES:
        assert np.isfinite(s.field(nm)).all()
    s.close()


def raw(lib, s, sources, edit=None, ls_edit=None, ls_null=False):
    """bq_solver_set_sources with entry 0 (and its descriptor) edited; (rc, error code, error text)"""
    from gpufluidsimulation_amd.solver import LevelSetDesc, source_arrays
    arr, ls, n = source_arrays(sources)
    for k, v in (edit or {}).items():
        obj = arr[0].shape if k in ("shape", "cx", "rx", "ry", "rz", "vx") else arr[0]
        setattr(obj, k, v)
    if ls is None and ls_edit:
        ls = (LevelSetDesc * max(1, n))()
    for k, v in (ls_edit or {}).items():
        setattr(ls[0], k, v)
    rc = lib.bq_solver_set_sources(s.s, arr, None if ls_null else ls, n)
    code, text = lib.fl_last_error(), lib.fl_last_error_string().decode()
    lib.fl_clear_error()
    return rc, code, text


def test_every_refusal_leaves_no_sources(lib):
    from gpufluidsimulation_amd import _lib
    from gpufluidsimulation_amd.solver import Source, levelset_sphere
    n = 16
    sph = Source(("sphere", 0.1), (0.5, 0.5, 0.5), 1.0, 1.0, 5, velocity=(0, 1, 0))
    box = Source(("box", (0.1, 0.1, 0.1)), (0.5, 0.5, 0.5), 1.0, 1.0, 5)
    lsrc = Source(levelset_sphere(0.2, 1.0 / n), (0.5, 0.5, 0.5), 1.0, 1.0, 5)
    s = make(lib, n)
    cases = [([sph], {"shape": 3}, None), ([sph], {"flags": 2}, None), ([sph], {"flags": -1}, None),
             ([sph], {"cx": float("nan")}, None), ([sph], {"vx": float("inf")}, None), ([sph], {"density": float("nan")}, None),
             ([sph], {"temperature": float("inf")}, None), ([sph], {"ey": float("nan")}, None), ([sph], {"oz": float("inf")}, None),
             ([sph], {"rx": 0.0}, None), ([sph], {"rx": -1.0}, None), ([box], {"ry": 0.0}, None), ([box], {"rz": float("nan")}, None),
             ([sph], {"emit_frames": -1}, None), ([sph] * 17, None, None),
             ([lsrc], None, {"phi": None}), ([lsrc], None, {"nx": 1}), ([lsrc], None, {"voxel": 0.0}),
             ([lsrc], None, {"background": float("inf")}), ([lsrc], None, {"i0": 2 ** 31 - 3}),
             ([lsrc], None, {"nx": 512, "ny": 512, "nz": 300})]
    for sources, edit, ls_edit in cases:
        s.setSources([sph])
        rc, code, text = raw(lib, s, sources, edit, ls_edit)
        assert rc != 0 and code == _lib.FL_ERR_BAD_ARGUMENT and text, (edit, ls_edit, text)
        assert lib.bq_solver_source_position(s.s, 0, (C.c_float * 3)()) != 0, (edit, ls_edit)     # no sources are left
    for ls_edit, match in (({"nx": 1}, "setSources: .*below 2"), ({"nx": 512, "ny": 512, "nz": 300}, "setSources: .*256 MiB")):
        assert re.search(match, raw(lib, s, [lsrc], None, ls_edit)[2])
    rc, code, text = raw(lib, s, [lsrc], ls_null=True)
    assert rc != 0 and code == _lib.FL_ERR_BAD_ARGUMENT and "descriptors" in text
    # a step after a refusal runs without sources
    s.advance(0, 0.5 / n)
    assert s.field("rho").max() == 0
    # n = 0 releases the list; the grids of sources are counted apart from the obstacles'
    s.setSources([lsrc, sph])
    assert s.sourcePositions().shape == (2, 3)
    s.setSources([])
    assert s.sourcePositions().shape == (0, 3)
    s.close()
    # the operator's own checks
    fields = SC.pattern((n, n, n))
    ptrs = {nm: fields[nm].ctypes.data for nm in SC.NAMES}
    from gpufluidsimulation_amd.solver import source_arrays
    for srcs, edit, null_ls in (([sph] * 17, None, False), ([sph], {"flags": 4}, False), ([lsrc], None, True)):
        arr, ls, cnt = source_arrays(srcs)
        for k, v in (edit or {}).items():
            setattr(arr[0], k, v)
        lib.gpu_emit_sources(ptrs["u"], ptrs["v"], ptrs["w"], ptrs["rho"], ptrs["T"], C.addressof(arr),
                             None if (null_ls or ls is None) else C.addressof(ls), cnt, 1.0 / n, n, n, n)
        assert lib.fl_last_error() == _lib.FL_ERR_BAD_ARGUMENT
        lib.fl_clear_error()
    for nm in SC.NAMES:
        assert np.array_equal(fields[nm], SC.pattern((n, n, n))[nm])


@pytest.mark.parametrize("scheme", [0, 3])
def test_emptied_list_is_no_source_at_all(lib, scheme):
    from gpufluidsimulation_amd.scenes import rising_smoke
    hashes = []
    for call in (False, True):
        n = 20
        s = make(lib, n, scheme)
        s.setSmoke(0.0, 1.0, rising_smoke(n, 1.0 / n))
        if call:
            s.setSources(SC.scene(n)[1])
            s.setSources([])
        digest = hashlib.sha256()
        for f in range(3):
            s.advance(f, 0.5 / n)
            for name in ("rho", "T", "u", "v", "w", "p"):
                digest.update(s.field(name).tobytes())
        hashes.append(digest.hexdigest())
        s.close()
    assert hashes[0] == hashes[1]


@pytest.mark.parametrize("loader", ["host", "obstacles", "levelsets"])
def test_stand_ins_without_the_operator_refuse(loader):
    """the three older stand-ins have no gpu_emit_sources: the host's weak reference is null there"""
    from build_cpu_host import build
    from gpufluidsimulation_amd import _lib, solver
    if loader == "host":
        lib = OC.bind_errors(solver.bind_host(C.CDLL(build(), mode=C.RTLD_LOCAL)))
    else:
        lib = {"obstacles": OC.load_obstacles, "levelsets": OC.load_levelsets}[loader]()
    s = solver.BimocqGPUSolver(16, 16, 16, 1.0, lib=lib, errlib=lib)
    from gpufluidsimulation_amd.solver import source_arrays
    arr, ls, n = source_arrays([solver.Source(("sphere", 0.1), (0.5, 0.5, 0.5), 1.0, 1.0, 5)])
    assert lib.bq_solver_set_sources(s.s, arr, ls, n) != 0
    assert lib.fl_last_error() == _lib.FL_ERR_UNSUPPORTED and "gpu_emit_sources" in lib.fl_last_error_string().decode()
    lib.fl_clear_error()
    s.setSources([])                                                   # an empty list is fine everywhere
    s.advance(0, 0.5 / 16)
    assert lib.fl_last_error() == 0
    s.close()


@pytest.mark.parametrize("dims", [(37, 29, 23), (99, 21, 18)])
def test_a_source_node_is_exactly_a_solid_node(lib, dims):
    """section 16's promise: inside the node window the cells a source list writes are the cells gpu_obstacle_flags_ls calls
    solid for the same shapes, owner for owner (the C restatements here; tests/test_gpu_sources.py does it on the device)"""
    from gpufluidsimulation_amd.solver import LevelSetObstacle, levelset_arrays
    ni, nj, nk = dims
    h, sources = SC.mixed(dims)
    for o, s in enumerate(sources):
        s.density = float(o + 1)
    rho = SC.emit_c(lib, {nm: np.zeros_like(a) for nm, a in SC.pattern(dims).items()}, sources, h, dims)["rho"]
    entries = [LevelSetObstacle(s.levelset, s.position) if s.levelset is not None else (s.code, *s.position, *s.extents, 0, 0, 0)
               for s in sources]
    arr, ls, n = levelset_arrays(entries)
    solid, rows = np.zeros(ni * nj * nk, np.uint8), np.zeros(nj * nk, np.uint8)
    lib.gpu_obstacle_flags_ls(solid.ctypes.data, rows.ctypes.data, C.addressof(arr), n, C.addressof(ls), h, ni, nj, nk)
    assert lib.fl_last_error() == 0
    win = np.zeros((nk, nj, ni), bool)
    win[2:nk - 2, 2:nj - 2, 2:ni - 2] = True
    want = np.where(win, solid.reshape(nk, nj, ni), 0)
    assert np.array_equal(rho.reshape(nk, nj, ni), want.astype(f32)) and len(np.unique(want)) >= 5
