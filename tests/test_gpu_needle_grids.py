"""The operators on needle-shaped grids, on the smallest grids they accept and at their size limits (include/bimocq_gpu.h,
"Limits"), against the references every other GPU test uses: the CPU oracle, bit for bit in value over the whole array.

The shapes, inputs, cases and the non-vacuity condition live in tests/needle_case.py; tests/test_needle_grids_cpu.py runs the same
cases on the CPU stand-in.  Each needle runs at h = 1/8 (the power-of-two structured path) and at h = 0.1 (per-axis tables of
stride max(dim) + 2, or the generic path).  Every compute case asserts non-vacuity on the reference (needle_case.reference) before
the device result is looked at.

What the HIP runtime answered about grid.y on gfx950 (recorded in "Limits"): a launch with grid.y = 65540 / 65541 is
accepted and computes what the oracle computes, so nj has no limit of its own and LONG_Y is a compute case here.

Cost.  The oracle is what takes the time.  A case on LONG_X or LONG_Z (6.5 M cells) takes a fraction of a second, on LONG_Y
(26 M cells) one to four seconds; two whole steps against OracleSolver (some fifty passes over every cell per step) take 5 to 7 s
on LONG_X and LONG_Z and about 20 s on LONG_Y, the slow tests here.  The shapes are the smallest at which the index in question
exists.

The operators with size rules of their own.  gpu_flow_stats and gpu_emit_sources have no rule for nj and compute on all three
needles, the source list with a box along the whole needle so that the launch has grid.y = 65540 on LONG_Y.  gpu_obstacle_loads
and gpu_vorticity_confinement compute on LONG_X and LONG_Z and refuse LONG_Y; gpu_render_density takes no dimension above 65534
(a ray's optical depth must stay below 2^53), so it computes on LONG_Z and refuses LONG_X and LONG_Y.  Every refusal is held to
FL_ERR_BAD_ARGUMENT, its text, and outputs still at 7.0."""
import ctypes as C

import numpy as np
import pytest

import confinement_case as CC
import fields as F
import host_entry_case as H
import needle_case as N
from oracle_lib import fp, lib as oracle

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD = H.FL_ERR_BAD_ARGUMENT
FL_OPT_DIAG_KCHUNK, FL_OPT_RENDER_KCHUNK = 22, 23


@pytest.fixture(scope="module")
def be():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0, lib.fl_last_error_string()
    old = {o: lib.fl_get_option(o) for o in (H.OPT_FAST_LERP, H.OPT_FIELD_WINDOW, CC.FL_OPT_CONFINE_KCHUNK, FL_OPT_DIAG_KCHUNK,
                                             FL_OPT_RENDER_KCHUNK)}
    backend = H.Backend(lib, lambda on: lib.fl_set_option(H.OPT_FAST_LERP, on), "hip")
    yield backend
    for o, v in old.items():
        lib.fl_set_option(o, v)
    oracle().orc_set_fast_lerp(0)
    backend.check()


def _id(p):
    return "%s-h%g" % (N.ident(p[0]), p[1])


@pytest.fixture(scope="module", params=[(d, h) for d in N.NEEDLES for h in N.SPACINGS], ids=_id)
def needle(be, request):
    """one needle at one spacing: the inputs generated and uploaded once for all cases of it"""
    r = N.Runner(be, *request.param)
    yield r
    r.free()


def windows_of(r):
    """FL_OPT_FIELD_WINDOW off and on where the marching window exists (power-of-two spacing); as it is elsewhere"""
    return (0, 1) if r.c.h == N.H_POW2 else (None,)


# ---- the families on the needles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("name", N.MAPS[1:])
def test_map_updates(needle, name, fast):
    N.run_case(needle, name, fast)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("name", N.GATHERS)
def test_gathers(needle, name, fast):
    N.run_case(needle, name, fast, windows_of(needle))


@pytest.mark.parametrize("name", ["init_maps"] + N.STREAMING + N.PROJECTION)
def test_streaming_and_projection(needle, name):
    N.run_case(needle, name)


def test_max_abs3(needle):
    """the CFL reduction over the whole needle, then with the maximum planted in the last element of each component"""
    c, lib = needle.c, needle.be.lib
    want = oracle().orc_max_abs3(*map(fp, c.vel), *c.dims)
    assert 0.99 < want < 1.0
    assert lib.gpu_max_abs3(*needle.d("vel"), *c.dims) == want
    for axis in range(3):
        a = c.cur[axis].copy()
        a[-1] = -3.0 - axis
        assert N.far_end(a, c.dims, axis).ravel()[-1] == a[-1]
        (buf,) = needle.be.dev(a)
        p = needle.d("cur")
        p[axis] = buf.ptr
        assert lib.gpu_max_abs3(*p, *c.dims) == f32(3.0 + axis), axis
    needle.be.check()


def test_map_travel_z(needle):
    """tests/host_entry_case.py's case: the window's corners, the far ones among them, and the border nodes around it"""
    H.run_map_travel(needle.be, *needle.c.dims, needle.c.h)


# ---- SMALL: accepted dimensions whose interior is empty or a handful of cells ----------------------------------------------------
@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", N.SMALL, ids=N.ident)
def test_small_shapes(be, dims, h):
    """every case in both lerp variants; the gathers with the marching window off and on: the window stages seven planes before
    its first node, and nk < 7 on three of these shapes.  None of these entry points refuses a dimension >= 1; the families that
    do are in test_small_shapes_of_the_other_families and test_small_shapes_refused below."""
    r = N.Runner(be, dims, h)
    for name in N.CASES:
        for fast in ((0, 1) if N.CASES[name].lerp else (0,)):
            N.run_case(r, name, fast, windows_of(r) if name in N.GATHERS else (None,))
    if min(dims) >= 5:
        H.run_map_travel(be, *dims, r.c.h)


# ---- operators with an nj rule of their own --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    return CC.load_confinement()


OWN_RULE_SMALL = [d for d in N.SMALL if min(d) >= 3]             # these operators take no dimension below 3
REFUSED_SMALL = [d for d in N.SMALL if min(d) < 3]


def confinement(be, restated, dims, h):
    """gpu_vorticity_confinement against its C restatement (tests/confinement_case.py), marching and one-thread-per-node kernel"""
    c = N.inputs(dims, h)
    rc, *want = CC.apply(restated, *c.vel, c.h, dims, 0.6, 0.3)
    assert rc == 0
    for axis, a in enumerate(want):
        N.assert_not_vacuous(a, H.PREFILL, dims, axis, "vorticity_confinement")
    r = N.Runner(be, dims, h)
    for kchunk in (0, -1):
        with H.options(be, {CC.FL_OPT_CONFINE_KCHUNK: kchunk}):
            out = be.dev(*N.fill(c.sizes[1:]))
            assert be.lib.gpu_vorticity_confinement(*H.ptrs(out), *r.d("vel"), c.h, *dims, 0.6, 0.3) == 0
            be.check()
            for axis, (a, b) in enumerate(zip(want, out)):
                got = b.numpy()
                assert F.same(a, got), (kchunk, axis, int((a != got).sum()), F.maxdiff(a, got))


@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", [N.LONG_X, N.LONG_Z], ids=N.ident)
def test_vorticity_confinement_computes(be, restated, dims, h):
    confinement(be, restated, dims, h)


@pytest.fixture(scope="module")
def stand_ins():
    """the CPU stand-ins that restate gpu_flow_stats, gpu_emit_sources, gpu_obstacle_loads and gpu_render_density"""
    import diag_case as D
    import loads_case as LC
    import render_case as RC
    import source_case as SC
    return {"diag": D.load_diag(), "sources": SC.load_sources(), "loads": LC.load_loads(), "render": RC.load_render()}


def flow_stats(be, dims, h, val, bound, mag):
    """gpu_flow_stats, marching and one-thread-per-cell kernel, through the caller of tests/test_gpu_diagnostics.py: the
    vorticity magnitude and the two maxima bit for bit, every sum within `bound` of the exact sum `val`"""
    import diag_case as D
    import obstacle_case as OC
    import test_gpu_diagnostics as TD
    c = N.inputs(dims, h)
    dev = OC.Dev(be.lib)
    try:
        for name, a in zip(("u", "v", "w", "rho", "T"), (*c.vel, c.rho, c.rho2)):
            dev.put(name, a)
        for kc in (0, -1):
            with H.options(be, {FL_OPT_DIAG_KCHUNK: kc}):
                got, field = TD.call(be.lib, dev, c.h, dims, True)
            for s in D.SUMS:
                err = abs(N.LD(got[s]) - N.LD(val[s]))
                print(f"{dims} h {c.h} kchunk {kc} {s}: {got[s]!r} |diff| {float(err):.3e} bound {bound[s]:.3e}")
                assert err <= bound[s], (kc, s, got[s], val[s], bound[s])
            assert TD.bits([got["div_max"], got["vort_max"]]) == TD.bits([val["div_max"], val["vort_max"]]), (kc, got)
            assert np.array_equal(field.view(np.uint32), mag.view(np.uint32)), (kc, F.maxdiff(field, mag))
    finally:
        dev.free()


@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", N.NEEDLES, ids=N.ident)
def test_flow_stats_computes(be, stand_ins, dims, h):
    """no rule for nj: on LONG_Y both kernels run with grid.y = 65540.  The sums are held to diag_case's bound n 2^-53 sum|term|
    around the exact sum (needle_case.blocked_sum: exact to the share the bound keeps for the reference's own rounding)"""
    flow_stats(be, dims, h, *N.flow_stats_reference(stand_ins["diag"], N.inputs(dims, h)))


def emit_sources(be, dims, h, sources, want):
    """gpu_emit_sources on fields that start as 7.0, through tests/source_case.py's call: every field equal to the restatement's"""
    import obstacle_case as OC
    import source_case as SC
    c = N.inputs(dims, h)
    dev = OC.Dev(be.lib)
    try:
        ptrs = {nm: dev.put(nm, a) for nm, a in zip(SC.NAMES, N.fill([c.n, c.n, c.nu, c.nv, c.nw]))}
        SC.call(be.lib, ptrs, sources, c.h, dims)
        be.check()
        for nm in SC.NAMES:
            got = dev.get(nm)
            assert np.array_equal(got, want[nm]), (nm, int((got != want[nm]).sum()))
    finally:
        dev.free()


@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", N.NEEDLES, ids=N.ident)
def test_emit_sources_computes(be, stand_ins, dims, h):
    """a box with a jet along the whole needle under the far-end sphere: the launch spans every block row, grid.y = 65540 on LONG_Y"""
    emit_sources(be, dims, h, *N.sources_reference(stand_ins["sources"], N.inputs(dims, h)))


def obstacle_loads(be, dims, h, p, solid, rows, centres, n, owner, terms):
    """gpu_obstacle_loads through the caller of tests/test_gpu_loads.py, held to loads_case's bound around the exact sums"""
    import loads_case as LC
    import obstacle_case as OC
    import test_gpu_loads as TL
    dev = OC.Dev(be.lib)
    try:
        for r in (rows, None):
            rc, got = TL.gpu_loads(be.lib, dev, p, solid, r, centres, n, h)
            be.check()
            assert rc == 0
            LC.assert_within_bound(got, owner, terms, n, f"{dims} rows {r is not None}")
    finally:
        dev.free()


@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", [N.LONG_X, N.LONG_Z], ids=N.ident)
def test_obstacle_loads_computes(be, stand_ins, dims, h):
    c = N.inputs(dims, h)
    obstacle_loads(be, dims, c.h, *N.loads_reference(stand_ins["loads"], c))


def render(be, dims, h, view, light, sigma_h, rho, img, shadow):
    """gpu_render_density through the caller of tests/test_gpu_render.py, marching at its own chunk length and one thread per ray:
    both image planes and the shadow field bit for bit"""
    import obstacle_case as OC
    import test_gpu_render as TR
    dev = OC.Dev(be.lib)
    try:
        dev.put("rho", rho)
        for kc in (0, -1):
            with H.options(be, {FL_OPT_RENDER_KCHUNK: kc}):
                got, sh = TR.render(be.lib, dev, dims, h, view, light, float(f32(sigma_h) / f32(h)), 1.0, 0.1)
            assert TR.same_bits(got, img), (dims, view, light, kc, int((got != img).sum()))
            assert light < 0 or TR.same_bits(sh, shadow), (dims, view, light, kc)
    finally:
        dev.free()


@pytest.mark.parametrize("case", N.RENDER_CASES, ids=lambda v: "view%d-light%d-%g" % v)
def test_render_density_computes_on_the_tallest_grid(be, stand_ins, case):
    """nk = 65534 is the largest dimension gpu_render_density takes: rays of 65534 cells along z, columns of that many along x"""
    render(be, N.LONG_Z, N.H_POW2, *case, *N.render_reference(stand_ins["render"], N.LONG_Z, N.H_POW2, *case))


def pool_of(be, floats):
    (pool,) = be.dev(np.full(floats, H.PREFILL, f32))
    return pool


def refuses(be, rc, text, what):
    message = be.lib.fl_last_error_string()
    assert be.refused() == BAD and rc in (None, 0, BAD) and text in message, (what, rc, message)


def test_own_nj_rule_refuses_long_y(be):
    """gpu_vorticity_confinement and gpu_obstacle_loads put (nj + 4) / 4 blocks on grid.y of kernels that were never run beyond
    65535 and say so: FL_ERR_BAD_ARGUMENT, the outputs left as they were"""
    ni, nj, nk = N.LONG_Y
    lib = be.lib
    n, nu, nv, nw = F.sizes(ni, nj, nk)
    pool = pool_of(be, nu + nv + nw + 8192)
    uo, vo, wo = pool.ptr, pool.ptr + 4 * nu, pool.ptr + 4 * (nu + nv)
    tail = pool.ptr + 4 * (nu + nv + nw)
    (src,) = be.dev(np.zeros(max(nu, nv, nw), f32))
    assert lib.gpu_vorticity_confinement(uo, vo, wo, src.ptr, src.ptr, src.ptr, N.H_POW2, ni, nj, nk, 0.6, 0.3) == BAD
    refuses(be, BAD, b"nj too large for grid.y", "gpu_vorticity_confinement")
    assert lib.gpu_obstacle_loads(src.ptr, None, src.ptr, None, None, 0, N.H_POW2, ni, nj, nk, tail) == BAD
    refuses(be, BAD, b"nj too large for grid.y", "gpu_obstacle_loads")
    assert bool(np.all(pool.numpy() == H.PREFILL))


@pytest.mark.parametrize("dims", [N.LONG_X, N.LONG_Y], ids=N.ident)
def test_render_density_refuses_a_dimension_above_65534(be, dims):
    """bq_render.hip: "dims outside 1..65534", in front of every launch: the image and the shadow field stay as they were.  Small
    buffers: the check was read in the source (gpu_render_density, the fifth test of its arguments)"""
    import render_case as RC
    pool = pool_of(be, 3 * 4096)
    rho, shadow, img = pool.ptr, pool.ptr + 4 * 4096, pool.ptr + 8 * 4096
    p = RC.params(6.0, 1.0, 0.1)
    for view, light in ((0, -1), (3, 4), (5, 1)):
        rc = be.lib.gpu_render_density(rho, shadow, N.H_POW2, *dims, view, light, C.cast(p, C.c_void_p), img)
        assert rc == BAD
        refuses(be, rc, b"dims outside 1..65534", ("gpu_render_density", view, light))
    assert bool(np.all(pool.numpy() == H.PREFILL))


# ---- SMALL on the families that ask for three cells per axis, and their refusals below that ------------------------------------------
@pytest.mark.parametrize("dims", OWN_RULE_SMALL, ids=N.ident)
def test_small_shapes_of_the_other_families(be, restated, stand_ins, dims):
    """confinement, flow statistics, sources, loads and the preview on grids whose interior is a handful of cells, each against
    the reference its own test file uses (diag_case.exact and loads_case.np_terms at these sizes)"""
    import diag_case as D
    import loads_case as LC
    import obstacle_case as OC
    import test_gpu_loads as TL
    for h in N.SPACINGS:
        c = N.inputs(dims, h)
        confinement(be, restated, dims, h)
        val, mass, n, mag = D.exact(stand_ins["diag"], *c.vel, c.rho, c.rho2, c.h, dims)
        flow_stats(be, dims, h, val, D.raw_bound(mass, n), mag)
        emit_sources(be, dims, h, *N.sources_reference(stand_ins["sources"], c))
    dev = OC.Dev(be.lib)
    try:
        p, solid, rows, ctr, n, h = TL.case(be.lib, dev, dims, "a")
        owner, _, terms, _ = LC.np_terms(p, solid, ctr, n, h)
        assert len(owner) > 0
    finally:
        dev.free()
    obstacle_loads(be, dims, h, p, solid, rows, ctr, n, owner, terms)


@pytest.mark.parametrize("dims", N.SMALL, ids=N.ident)
def test_small_shapes_rendered(be, stand_ins, dims):
    """gpu_render_density takes every dimension from 1: three views, without and with a light"""
    for view, light in ((0, -1), (3, 4), (4, 1)):
        render(be, dims, N.H_TABLED, view, light, 0.4, *N.render_reference(stand_ins["render"], dims, N.H_TABLED, view, light, 0.4))


@pytest.mark.parametrize("dims", REFUSED_SMALL, ids=N.ident)
def test_small_shapes_refused(be, dims):
    """(1, 1, 1) and (2, 3, 4): every operator whose kernels need three cells per axis says "dims below 3" and writes nothing.
    One buffer of 7.0 stands for every pointer; it is larger than any buffer of these grids."""
    pool = pool_of(be, 4096)
    calls = own_calls(be.lib, pool.ptr, dims)
    for name, (_, texts) in OWN_CHECKS.items():
        if texts is not FP64_LIKE and name != "gpu_render_density":          # those two families take every dimension from 1
            refuses(be, calls[name](), b"dims below 3", name)
    assert bool(np.all(pool.numpy() == H.PREFILL))


# ---- obstacles and the fp64 operators ----------------------------------------------------------------------------------------------
# every needle at both spacings; the SMALL shapes these operators take (three cells per axis) at one
OBSTACLE_CASES = [(d, h) for d in N.NEEDLES for h in N.SPACINGS] + [(d, N.H_POW2) for d in OWN_RULE_SMALL]


@pytest.mark.parametrize("dims,h", OBSTACLE_CASES, ids=list(map(_id, OBSTACLE_CASES)))
def test_obstacle_operators(be, restated, dims, h):
    """one moving sphere of radius 3 h centred 6 cells from the far end: gpu_obstacle_flags, gpu_obstacle_faces, gpu_gradient_masked,
    gpu_jacobi_sweeps_masked and gpu_obstacle_blend against the C restatement (tests/cpu_abi/obstacle_abi.c), through the callers of
    tests/test_gpu_obstacles.py"""
    import obstacle_case as OC
    import test_gpu_obstacles as TO
    hip, cpu = be.lib, restated
    c = N.inputs(dims, h)
    hp = lambda arrays: [x.ctypes.data for x in arrays]
    dev = OC.Dev(hip)
    needle = N.long_axis(dims) is not None
    try:
        bnd = [(0, *N.far_emitter(dims, c.h), 0.0, 0.0, 0.3, -0.2, 0.1)]
        s_c, t_c, arr, n = TO.flags_both(hip, cpu, dev, dims, bnd, c.h)
        if needle:
            assert int((N.far_end(s_c, dims) != 0).sum()) >= N.MIN_MOVED and (t_c == 0).any() and (t_c != 0).any()
        assert np.array_equal(dev.get("solid"), s_c) and np.array_equal(dev.get("rows"), t_c)
        solid_p, rows_p = dev["solid"], dev["rows"]
        # faces, with the delta share
        vel, hd = [a.copy() for a in c.vel], N.fill(c.sizes[1:])
        cpu.gpu_obstacle_faces(*hp(vel), *hp(hd), s_c.ctypes.data, C.addressof(arr), n, *dims)
        for axis in range(3):
            N.assert_not_vacuous(vel[axis], c.vel[axis], dims, axis, "obstacle_faces")
        up = [dev.put(nm, x) for nm, x in zip("uvw", c.vel)]
        dp_ = [dev.put("d" + nm, x) for nm, x in zip("uvw", N.fill(c.sizes[1:]))]
        hip.gpu_obstacle_faces(*up, *dp_, solid_p, C.addressof(arr), n, *dims)
        OC.check(hip)
        for nm, want, dwant in zip("uvw", vel, hd):
            assert np.array_equal(dev.get(nm), want) and np.array_equal(dev.get("d" + nm), dwant), ("faces", nm)
        # masked gradient on the face-written velocity
        p = c.rho.copy()
        p[s_c != 0] = 0
        before = [a.copy() for a in vel]
        cpu.gpu_gradient_masked(*hp(vel), p.ctypes.data, None, None, None, s_c.ctypes.data, *dims, 0.5)
        for axis in range(3):
            N.assert_not_vacuous(vel[axis], before[axis], dims, axis, "gradient_masked")
        hip.gpu_gradient_masked(*up, dev.put("p", p), None, None, None, solid_p, *dims, 0.5)
        OC.check(hip)
        for nm, want in zip("uvw", vel):
            assert np.array_equal(dev.get(nm), want), ("gradient_masked", nm)
        # five masked sweeps
        beta = float(f32(1 / 6))
        hpp, ht = p.copy(), p.copy()
        assert cpu.gpu_jacobi_sweeps_masked(hpp.ctypes.data, c.rho2.ctypes.data, ht.ctypes.data, s_c.ctypes.data, t_c.ctypes.data, *dims, 5, -1.0, beta) == 1
        N.assert_not_vacuous(ht, p, dims, -1, "jacobi_sweeps_masked")
        assert hip.gpu_jacobi_sweeps_masked(dev.put("p", p), dev.put("div", c.rho2), dev.put("pt", p), solid_p, rows_p, *dims, 5, -1.0, beta) == 1
        OC.check(hip)
        assert np.array_equal(dev.get("pt"), ht) and np.array_equal(dev.get("p"), hpp)
        # band blend and density clear
        fields_ = list(c.vel) + [c.rho, c.rho2]
        srcs = [x * f32(-1.5) for x in fields_]
        host = [x.copy() for x in fields_]
        cpu.gpu_obstacle_blend(*hp(host), *hp(srcs), s_c.ctypes.data, C.addressof(arr), n, c.h, *dims)
        for axis, (a, b) in zip((0, 1, 2), zip(host, fields_)):
            N.assert_not_vacuous(a, b, dims, axis, "obstacle_blend")
        names = ("bu", "bv", "bw", "brho", "bT")
        hip.gpu_obstacle_blend(*[dev.put(nm, x) for nm, x in zip(names, fields_)], *[dev.put("s" + nm, x) for nm, x in zip(names, srcs)],
                               solid_p, C.addressof(arr), n, c.h, *dims)
        OC.check(hip)
        for nm, want in zip(names, host):
            assert np.array_equal(dev.get(nm), want), ("blend", nm)
    finally:
        dev.free()


@pytest.mark.parametrize("dims,h", OBSTACLE_CASES, ids=list(map(_id, OBSTACLE_CASES)))
def test_walled_operators(be, dims, h):
    """the reference's solid box with an open top (BQ_WALLS_REFERENCE_BOX) around the sphere at the far end: gpu_wall_flags,
    gpu_wall_faces, five gpu_jacobi_sweeps_masked_walls and gpu_gradient_masked_walls against the C restatement
    (tests/cpu_abi/walls_abi.c)"""
    import obstacle_case as OC
    import test_gpu_obstacles as TO
    import walls_case as WC
    hip, cpu = be.lib, WC.load_walls()
    c = N.inputs(dims, h)
    hp = lambda arrays: [x.ctypes.data for x in arrays]
    walls = WC.REFERENCE_BOX
    dev = OC.Dev(hip)
    needle = N.long_axis(dims) is not None
    try:
        bnd = [(0, *N.far_emitter(dims, c.h), 0.0, 0.0, 0.3, -0.2, 0.1)]
        s_c, t_c, arr, n = TO.flags_both(hip, cpu, dev, dims, bnd, c.h)
        sw = np.full_like(s_c, 7)
        cpu.gpu_wall_flags(sw.ctypes.data, s_c.ctypes.data, walls, *dims)
        far = N.far_end(sw, dims)
        assert not needle or (int((far == WC.FLAG_WALL).sum()) >= N.MIN_MOVED and int(((far != 0) & (far != WC.FLAG_WALL)).sum()) >= N.MIN_MOVED)
        hip.gpu_wall_flags(dev.put("solidw", np.full_like(s_c, 7)), dev["solid"], walls, *dims)
        OC.check(hip)
        assert np.array_equal(dev.get("solidw"), sw), "wall_flags"
        sw_p, rows_p = dev["solidw"], dev["rows"]
        vel, hd = [a.copy() for a in c.vel], N.fill(c.sizes[1:])
        cpu.gpu_wall_faces(*hp(vel), *hp(hd), sw.ctypes.data, *dims)
        for axis in range(3):
            N.assert_not_vacuous(hd[axis], H.PREFILL, dims, axis, "wall_faces")
        up = [dev.put(nm, x) for nm, x in zip("uvw", c.vel)]
        dp_ = [dev.put("d" + nm, x) for nm, x in zip("uvw", N.fill(c.sizes[1:]))]
        hip.gpu_wall_faces(*up, *dp_, sw_p, *dims)
        OC.check(hip)
        for nm, want, dwant in zip("uvw", vel, hd):
            assert np.array_equal(dev.get(nm), want) and np.array_equal(dev.get("d" + nm), dwant), ("wall_faces", nm)
        p = c.rho.copy()
        p[sw != 0] = 0
        beta = float(f32(1 / 6))
        hpp, ht = p.copy(), p.copy()
        assert cpu.gpu_jacobi_sweeps_masked_walls(hpp.ctypes.data, c.rho2.ctypes.data, ht.ctypes.data, sw.ctypes.data, t_c.ctypes.data, walls,
                                                  *dims, 5, -1.0, beta) == 1
        N.assert_not_vacuous(ht, p, dims, -1, "jacobi_sweeps_masked_walls")
        assert hip.gpu_jacobi_sweeps_masked_walls(dev.put("p", p), dev.put("div", c.rho2), dev.put("pt", p), sw_p, rows_p, walls,
                                                  *dims, 5, -1.0, beta) == 1
        OC.check(hip)
        assert np.array_equal(dev.get("pt"), ht) and np.array_equal(dev.get("p"), hpp), "jacobi_sweeps_masked_walls"
        before = [a.copy() for a in vel]
        cpu.gpu_gradient_masked_walls(*hp(vel), ht.ctypes.data, None, None, None, sw.ctypes.data, walls, *dims, 0.5)
        for axis in range(3):
            N.assert_not_vacuous(vel[axis], before[axis], dims, axis, "gradient_masked_walls")
        hip.gpu_gradient_masked_walls(*up, dev["pt"], None, None, None, sw_p, walls, *dims, 0.5)
        OC.check(hip)
        for nm, want in zip("uvw", vel):
            assert np.array_equal(dev.get(nm), want), ("gradient_masked_walls", nm)
    finally:
        dev.free()


@pytest.mark.parametrize("dims", N.NEEDLES + N.SMALL, ids=N.ident)
def test_fp64_operators(be, dims):
    """gpu_divergence_double and gpu_pcg_gradient against their restatement (tests/cpu_abi/pcg_abi.c), gpu_smoothing_jacobi with 1
    and 4 iterations against the oracle's orc_mg_smooth"""
    import obstacle_case as OC
    import pcg_case as PC
    from oracle_lib import dp
    hip, cpu = be.lib, PC.load_pcg()
    c = N.inputs(dims, N.H_POW2)
    hp = lambda arrays: [x.ctypes.data for x in arrays]
    dev = OC.Dev(hip)
    needle = N.long_axis(dims) is not None
    try:
        up = [dev.put(nm, x) for nm, x in zip("uvw", c.vel)]
        want = np.full(c.n, np.nan)
        cpu.gpu_divergence_double(*hp(c.vel), want.ctypes.data, *dims, 0.75)
        assert (not needle or int((N.far_end(want, dims) != 0).sum()) >= N.MIN_MOVED) and np.isfinite(want).all()
        hip.gpu_divergence_double(*up, dev.put("dd", np.full(c.n, np.nan)), *dims, 0.75)
        OC.check(hip)
        assert np.array_equal(dev.get("dd"), want), "divergence_double"
        p64 = c.rho.astype(np.float64)
        vel = [a.copy() for a in c.vel]
        cpu.gpu_pcg_gradient(*hp(vel), p64.ctypes.data, None, *dims, 0.75)
        for axis in range(3):
            N.assert_not_vacuous(vel[axis], c.vel[axis], dims, axis, "pcg_gradient")
        hip.gpu_pcg_gradient(*up, dev.put("p64", p64), None, *dims, 0.75)
        OC.check(hip)
        for nm, a in zip("uvw", vel):
            assert np.array_equal(dev.get(nm), a), ("pcg_gradient", nm)
        b = c.rho2.astype(np.float64)
        x0 = p64.reshape(dims[2], dims[1], dims[0])
        t0 = np.zeros_like(x0)                               # temp carries x's boundary shell, as the V-cycle keeps it
        t0[0], t0[-1], t0[:, 0], t0[:, -1], t0[:, :, 0], t0[:, :, -1] = x0[0], x0[-1], x0[:, 0], x0[:, -1], x0[:, :, 0], x0[:, :, -1]
        for iters in (1, 4):
            xr, tr = p64.copy(), t0.ravel().copy()
            oracle().orc_mg_smooth(dp(xr), dp(b), dp(tr), -8.0, 1.0 / 6.0, *dims, iters)
            N.assert_not_vacuous(xr, p64, dims, -1, "smoothing_jacobi")
            hip.gpu_smoothing_jacobi(dev.put("x", p64), dev.put("b", b), dev.put("t", t0.ravel()), -8.0, 1.0 / 6.0, *dims, iters)
            OC.check(hip)
            assert np.array_equal(dev.get("x"), xr), ("smoothing_jacobi", iters)      # temp is scratch: no contract on what it is left as
    finally:
        dev.free()


# ---- whole steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [0, 3])
@pytest.mark.parametrize("dims", N.NEEDLES, ids=N.ident)
def test_whole_steps(be, dims, scheme):
    """two steps of BimocqGPUSolver against OracleSolver, the emitter at the far end, 8 Jacobi sweeps: every field of both steps.
    Schemes 0 (BiMocq) and 3 (reflection): the two OracleSolver implements; MacCormack (scheme 2) has no oracle state machine, its
    kernel is held to the oracle's composition in the gpu_maccormack cases above."""
    N.run_steps(dims, scheme, device=0)
    be.check()


def test_viscous_reflection_steps_on_the_tallest_grid(be):
    """scheme 3 with viscosity on nk + 1 = 65535: the MacCormack limiter and the diffusion sweeps run on the w buffer's own dims,
    65535 planes, which their size check used to read as a grid of 65536 and refuse"""
    N.run_steps(N.LONG_Z, 3, viscosity=1e-3, device=0)
    be.check()


# ---- the plane limit -------------------------------------------------------------------------------------------------------------
def test_advect_field_just_below_the_plane_limit(be):
    """(2047, 4094, 8), h = 1/2048: the staggered plane is 2048 x 4095 = 2^23 - 2048 elements, the size the 24-bit multiplies of
    the flat index are documented for.  Judged non-vacuous on the last 16 rows and the last 4 planes.  One case, 1.5 s measured (the
    oracle's pass over 67 M cells is most of it)."""
    ni, nj, nk = dims = (2047, 4094, 8)
    h = float(f32(1.0 / 2048))
    assert (ni + 1) * (nj + 1) == 2 ** 23 - 2048 and 4 * (ni + 1) * (nj + 1) * (nk + 1) < 2 ** 31
    n = ni * nj * nk
    rng = np.random.default_rng(20471)
    rho = rng.random(n, dtype=f32)
    amp = f32(1.3) * f32(h)
    axes = (np.arange(ni, dtype=f32)[None, None, :], np.arange(nj, dtype=f32)[None, :, None], np.arange(nk, dtype=f32)[:, None, None])
    back = [(np.broadcast_to(a * f32(h), (nk, nj, ni)).reshape(-1) + amp * (f32(2) * rng.random(n, dtype=f32) - f32(1))).astype(f32)
            for a in axes]
    ref = np.full(n, H.PREFILL, f32)
    oracle().orc_advect_field(fp(ref), fp(rho), *map(fp, back), h, ni, nj, nk, 0)
    r3 = ref.reshape(nk, nj, ni)
    for part in (r3[:, nj - 16:, :], r3[nk - 4:]):
        assert int(((part != H.PREFILL) & (part != 0)).sum()) >= N.MIN_MOVED
    dback, (drho, out) = be.dev(*back), be.dev(rho, np.full(n, H.PREFILL, f32))
    be.lib.gpu_advect_field(out.ptr, drho.ptr, *H.ptrs(dback), h, ni, nj, nk, False)
    be.check()
    got = out.numpy()
    bad = np.flatnonzero(ref != got)
    assert bad.size == 0, (bad.size, bad[:4].tolist(), bad[-4:].tolist(), F.maxdiff(ref, got))


# ---- refusals at the edge --------------------------------------------------------------------------------------------------------
# entry point -> (family, where its size check is, the call on one pointer p that stands for every buffer).  A family names the
# limits its check enforces: "gather" 2 GiB, the plane limit and grid.z (bq_advect.hip: dims_ok :811, buffer_dims_ok :826);
# "projection" 4 GiB and grid.z (bq_project.hip: dims_ok :1582, buffer_dims_ok :1593); "stream" grid.z only (bq_host.h: planes_ok;
# these kernels index with size_t).  The calls take the dims of a GRID; an entry point that takes a component's own dims gets the
# grid's largest buffer, (ni + 1, nj + 1, nk + 1).  Only entry points listed here are called with buffers smaller than their dims.
A, B_ = N.ALPHA, N.BETA


def buf(d):
    return [x + 1 for x in d]


CHECKS = {
    "gpu_solve_forward": ("gather", "bq_advect.hip:1282", lambda l, p, h, d: l.gpu_solve_forward(*[p] * 6, h, *d, h, h)),
    "gpu_solve_forward_hint": ("gather", "bq_advect.hip:1282", lambda l, p, h, d: l.gpu_solve_forward_hint(*[p] * 6, h, *d, h, h, 1)),
    "gpu_solve_backwardDMC": ("gather", "bq_advect.hip:1303", lambda l, p, h, d: l.gpu_solve_backwardDMC(*[p] * 9, h, *d, h)),
    "gpu_solve_backwardDMC_hint": ("gather", "bq_advect.hip:1303", lambda l, p, h, d: l.gpu_solve_backwardDMC_hint(*[p] * 9, h, *d, h, 1)),
    "gpu_advect_velocity": ("gather", "bq_advect.hip:1358", lambda l, p, h, d: l.gpu_advect_velocity(*[p] * 9, h, *d, False)),
    "gpu_advect_vel_double": ("gather", "bq_advect.hip:1370", lambda l, p, h, d: l.gpu_advect_vel_double(*[p] * 12, h, *d, False, 0.6)),
    "gpu_advect_field": ("gather", "bq_advect.hip:1381", lambda l, p, h, d: l.gpu_advect_field(*[p] * 5, h, *d, False)),
    "gpu_accumulate_velocity": ("gather", "bq_advect.hip:1427", lambda l, p, h, d: l.gpu_accumulate_velocity(*[p] * 9, h, *d, False, 1.0)),
    "gpu_accumulate_field": ("gather", "bq_advect.hip:1437", lambda l, p, h, d: l.gpu_accumulate_field(*[p] * 5, h, *d, False, 1.0)),
    "gpu_estimate_distortion": ("gather", "bq_advect.hip:1522", lambda l, p, h, d: l.gpu_estimate_distortion(*[p] * 7, h, *d)),
    "gpu_compensate_velocity": ("gather", "bq_advect.hip:1533", lambda l, p, h, d: l.gpu_compensate_velocity(*[p] * 15, h, *d, False)),
    "gpu_compensate_field": ("gather", "bq_advect.hip:1562", lambda l, p, h, d: l.gpu_compensate_field(*[p] * 9, h, *d, False)),
    "gpu_semilag": ("gather", "bq_advect.hip:1573", lambda l, p, h, d: l.gpu_semilag(*[p] * 5, 0, 0, 1, h, *d, h, h)),
    "gpu_clamp_extrema": ("gather", "bq_advect.hip:1635", lambda l, p, h, d: l.gpu_clamp_extrema(*[p] * 5, d[0], d[1], d[2] + 1, 0, 0, 1, 0.0, 0.0, 0.5, h, h)),
    "gpu_maccormack": ("gather", "bq_advect.hip:1647", lambda l, p, h, d: l.gpu_maccormack(*[p] * 7, 0, 0, 1, h, *d, h, h, h)),
    "gpu_clamp_extrema_box": ("gather", "bq_advect.hip:1658", lambda l, p, h, d: l.gpu_clamp_extrema_box(p, p, *buf(d))),
    "gpu_clamp_extrema_box_w": ("gather", "bq_advect.hip:1664", lambda l, p, h, d: l.gpu_clamp_extrema_box_w(p, p, *buf(d))),
    "gpu_divergence": ("projection", "bq_project.hip:1864", lambda l, p, h, d: l.gpu_divergence(*[p] * 4, *d, 0.5)),
    "gpu_jacobi_sweeps": ("projection", "bq_project.hip:1872", lambda l, p, h, d: l.gpu_jacobi_sweeps(p, p, p, *d, 4, A, B_)),
    "gpu_gradient": ("projection", "bq_project.hip:1947", lambda l, p, h, d: l.gpu_gradient(*[p] * 4, *d, 0.5)),
    "gpu_projection_jacobi": ("projection", "bq_project.hip:2024", lambda l, p, h, d: l.gpu_projection_jacobi(*[p] * 6, None, *d, 5, 0.5, A, B_)),
    "gpu_diffuse_field": ("projection", "bq_project.hip:2094", lambda l, p, h, d: l.gpu_diffuse_field(p, p, p, *buf(d), 3, 0.37)),
    "gpu_diffuse_sweeps": ("projection", "bq_project.hip:2115", lambda l, p, h, d: l.gpu_diffuse_sweeps(p, p, p, *buf(d), 3, 0.37)),
    "gpu_emit_smoke": ("stream", "bq_misc.hip:296", lambda l, p, h, d: l.gpu_emit_smoke(*[p] * 5, h, *d, h, h, h, h, 1.0, 1.0, 0.0)),
    "gpu_add_buoyancy": ("stream", "bq_misc.hip:311", lambda l, p, h, d: l.gpu_add_buoyancy(p, p, p, *d, 0.3, 1.1, h)),
    "gpu_init_maps": ("stream", "bq_misc.hip:349", lambda l, p, h, d: l.gpu_init_maps(p, p, p, h, *d)),
    "gpu_map_travel_z": ("stream", "bq_misc.hip:434", lambda l, p, h, d: l.gpu_map_travel_z(p, p, h, *d, (C.c_float * 2)())),
}
# The families with a size check of their own: entry point -> (where the check is, {limit: the text it latches}).  Limits they do
# not have are absent: no plane limit and 4 GiB in the obstacle and source operators (one predicate, bq_host.h: obstacle_dims_ok,
# reached through bq_obstacle.hip: obs_args_ok); grid.z alone in the two fp64 launchers that put planes on it (BQ_REQUIRE latches
# the condition's own text); gpu_render_density turns nk = 65535 away under its rule for every dimension.
GATHER_LIKE = {"planes": b"nk too large for grid.z", "plane": b"plane of 2^23 elements or more", "2gib": b"field larger than 2 GiB"}
OBSTACLE_LIKE = {"planes": b"nk too large for grid.z", "4gib": b"field larger than 4 GiB"}
FP64_LIKE = {"planes": b"nk < 65535"}
OWN_CHECKS = {
    "gpu_vorticity_confinement": ("bq_confine.hip:237", GATHER_LIKE),
    "gpu_flow_stats": ("bq_diag.hip:280", GATHER_LIKE),
    "gpu_obstacle_loads": ("bq_loads.hip:264", GATHER_LIKE),
    "gpu_render_density": ("bq_render.hip:285", dict(GATHER_LIKE, planes=b"dims outside 1..65534")),
    "gpu_emit_sources": ("bq_source.hip:112", OBSTACLE_LIKE),
    "gpu_pcg_gradient": ("bq_pcg.hip:322", FP64_LIKE),
    "gpu_smoothing_jacobi": ("bq_mgcg.hip:1813", FP64_LIKE),
}
OWN_CHECKS.update({name: ("bq_host.h:136", OBSTACLE_LIKE) for name in (
    "gpu_obstacle_flags", "gpu_obstacle_faces", "gpu_obstacle_blend", "gpu_gradient_masked", "gpu_jacobi_sweeps_masked", "gpu_wall_flags",
    "gpu_wall_faces", "gpu_jacobi_sweeps_masked_walls", "gpu_gradient_masked_walls")})


def own_calls(lib, p, dims, h=N.H_POW2):
    """the entry points of OWN_CHECKS on one buffer at address p (4096 floats at least) that stands for every pointer, apart
    from pairs the check in front of the size check wants distinct"""
    import render_case as RC
    import walls_case as WC
    from gpufluidsimulation_amd.solver import boundary_array
    walls = WC.REFERENCE_BOX
    arr, n = boundary_array([(0, 0.2, 0.2, 0.2, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0)])
    b = C.addressof(arr)
    rp = RC.params(6.0, 1.0, 0.1)
    keep = (arr, rp)
    return {
        "gpu_obstacle_flags": lambda: lib.gpu_obstacle_flags(p, p, b, n, h, *dims),
        "gpu_obstacle_faces": lambda: lib.gpu_obstacle_faces(*[p] * 7, b, n, *dims),
        "gpu_obstacle_blend": lambda: lib.gpu_obstacle_blend(*[p] * 11, b, n, h, *dims),
        "gpu_gradient_masked": lambda: lib.gpu_gradient_masked(*[p] * 4, None, None, None, p, *dims, 0.5),
        "gpu_jacobi_sweeps_masked": lambda: lib.gpu_jacobi_sweeps_masked(p, p, p + 2048, p, p, *dims, 5, A, B_),
        "gpu_wall_flags": lambda: lib.gpu_wall_flags(p, p + 2048, walls, *dims),
        "gpu_wall_faces": lambda: lib.gpu_wall_faces(*[p] * 7, *dims),
        "gpu_jacobi_sweeps_masked_walls": lambda: lib.gpu_jacobi_sweeps_masked_walls(p, p, p + 2048, p, p, walls, *dims, 5, A, B_),
        "gpu_gradient_masked_walls": lambda: lib.gpu_gradient_masked_walls(*[p] * 4, None, None, None, p, walls, *dims, 0.5),
        "gpu_vorticity_confinement": lambda: lib.gpu_vorticity_confinement(p, p + 1024, p + 2048, *[p + 3072] * 3, h, *dims, 0.6, 0.3),
        "gpu_obstacle_loads": lambda: lib.gpu_obstacle_loads(p, None, p + 1024, None, b, n, h, *dims, p + 2048),
        "gpu_flow_stats": lambda: lib.gpu_flow_stats(p, p, p, p, p, None, h, *dims, p + 2048),
        "gpu_emit_sources": lambda: lib.gpu_emit_sources(*[p] * 5, None, None, 0, h, *dims),
        "gpu_render_density": lambda: lib.gpu_render_density(p, p + 1024, h, *dims, 0, 4, C.cast(rp, C.c_void_p), p + 2048),
        "gpu_pcg_gradient": lambda: lib.gpu_pcg_gradient(p, p, p, p, None, *dims, 0.75),
        "gpu_smoothing_jacobi": lambda: lib.gpu_smoothing_jacobi(p, p, p + 2048, -8.0, 1.0 / 6.0, *dims, 2),
        "keep": keep,
    }


def own_refused(be, limit, dims, floats):
    """every entry point of OWN_CHECKS that has `limit`, at `dims`: FL_ERR_BAD_ARGUMENT under its text, nothing written"""
    pool = pool_of(be, max(floats, 4096))
    calls = own_calls(be.lib, pool.ptr, dims)
    for name, (_, texts) in OWN_CHECKS.items():
        if limit in texts:
            refuses(be, calls[name](), texts[limit], name)
    assert bool(np.all(pool.numpy() == H.PREFILL))


TOO_MANY_PLANES = (10, 10, 65535)               # nk + 1 = 65536
PLANE_AT_LIMIT = (2047, 4095, 3)                # (ni + 1)(nj + 1) = 2^23 exactly
TWO_GIB = (1023, 1023, 511)                     # 4 (ni + 1)(nj + 1)(nk + 1) = 2^31 exactly
FOUR_GIB = (1023, 1023, 1023)                   # ... = 2^32 exactly


def refused_with(be, names, dims, text, floats):
    """every entry point of `names` at `dims` on one buffer of `floats` floats: FL_ERR_BAD_ARGUMENT, the limit named, nothing written"""
    (buf,) = be.dev(np.full(floats, H.PREFILL, f32))
    for name in names:
        CHECKS[name][2](be.lib, buf.ptr, N.H_POW2, dims)
        message = be.lib.fl_last_error_string()
        assert be.refused() == BAD, name
        assert text in message and name.replace("_hint", "").encode() in message, (name, message)
    assert bool(np.all(buf.numpy() == H.PREFILL))


def true_size(dims):
    return (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1)


def test_refused_one_plane_too_many(be):
    assert TOO_MANY_PLANES[2] + 1 == 65536
    refused_with(be, list(CHECKS), TOO_MANY_PLANES, b"nk too large for grid.z", true_size(TOO_MANY_PLANES))
    own_refused(be, "planes", TOO_MANY_PLANES, true_size(TOO_MANY_PLANES))


def test_refused_plane_of_2_to_the_23(be):
    assert (PLANE_AT_LIMIT[0] + 1) * (PLANE_AT_LIMIT[1] + 1) == 2 ** 23
    gathers = [n for n, v in CHECKS.items() if v[0] == "gather"]
    refused_with(be, gathers, PLANE_AT_LIMIT, b"plane larger than 2^23 elements", true_size(PLANE_AT_LIMIT))
    own_refused(be, "plane", PLANE_AT_LIMIT, true_size(PLANE_AT_LIMIT))


def test_refused_field_of_2_gib(be):
    """small buffers: only entry points whose check is in the tables above"""
    assert 4 * true_size(TWO_GIB) == 2 ** 31 and (TWO_GIB[0] + 1) * (TWO_GIB[1] + 1) < 2 ** 23 and TWO_GIB[2] + 1 <= 65535
    gathers = [n for n, v in CHECKS.items() if v[0] == "gather"]
    refused_with(be, gathers, TWO_GIB, b"field larger than 2 GiB", 4096)
    own_refused(be, "2gib", TWO_GIB, 4096)


def test_refused_field_of_4_gib(be):
    """the projection family's own bound; between 2 and 4 GiB it accepts a field, which no test covers (the oracle needs minutes)"""
    assert 4 * true_size(FOUR_GIB) == 2 ** 32
    projection = [n for n, v in CHECKS.items() if v[0] == "projection"]
    refused_with(be, projection, FOUR_GIB, b"field larger than 4 GiB", 4096)
    own_refused(be, "4gib", FOUR_GIB, 4096)
