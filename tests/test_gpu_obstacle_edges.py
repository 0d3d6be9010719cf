"""Obstacles on the MI355X where this kernel family can go wrong, against the fp64 reference (tests/obstacle_ref.py):
the sweep operators on host-built masks at row-block edges, chunk boundaries, walls and float4 lane seams, on shapes the
fused masked kernel takes and shapes it refuses (launch counts say which ran); the shape production runs (256^3 and a
non-cubic grid, default chunking) and the step there with and without the fused kernel; the projection pipeline against
an fp64 pipeline; flags, rows and the band pass against fp64 geometry."""
import ctypes as C

import numpy as np
import pytest

import fields as F
import obstacle_case as OC
import obstacle_ref as R
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu

FUSED = [(32, 8, 12), (36, 13, 13), (252, 17, 40), (256, 24, 27)]
REFUSED = [(99, 21, 18), (384, 12, 14), (40, 5, 16), (40, 16, 11)]
COUNTS = (1, 2, 3, 4, 6, 7)


@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, OC.load_obstacles()


class options:
    """fl_set_option for the duration of a block; FL_OPT_PROFILE_JACOBI on, so that launches() counts the sweep launches"""
    def __init__(self, hip, **kv):
        from gpufluidsimulation_amd import _lib
        self.hip = hip
        self.kv = {getattr(_lib, "FL_OPT_" + k): v for k, v in kv.items()}
        self.kv[_lib.FL_OPT_PROFILE_JACOBI] = 1

    def __enter__(self):
        self.was = {o: self.hip.fl_get_option(o) for o in self.kv}
        for o, v in self.kv.items():
            self.hip.fl_set_option(o, v)
        launches(self.hip)
        return self

    def __exit__(self, *exc):
        for o, v in self.was.items():
            self.hip.fl_set_option(o, v)


def launches(hip):
    """(launches, sweeps) of the sweep loops since the last call"""
    ms, n, s = C.c_double(), C.c_longlong(), C.c_longlong()
    hip.fl_jacobi_profile(C.byref(ms), C.byref(n), C.byref(s))
    return n.value, s.value


def expected_launches(n, fused):
    return n // 3 + n % 3 if fused else n


def sweeps_case(hip, cpu, dev, dims, solid, seed, fused, counts=COUNTS):
    """fused = single masked sweeps = C restatement bit for bit after each count, all within the fp64 bound; returns the
    largest error / bound ratio"""
    ni, nj, nk = dims
    beta = R.beta32()
    rows = R.rows_of(solid)
    p = R.initial_p(solid, seed)
    div = np.random.default_rng(100 + seed).standard_normal(solid.shape).astype(np.float32)
    nmax = max(counts)
    its, bounds = R.masked_sweeps(p, div, solid, nmax)
    sp, rp, dp = dev.put("solid", solid), dev.put("rows", rows), dev.put("div", div)
    # the C restatement and single masked sweeps on the device, iterate by iterate
    ca, cb = p.copy(), p.copy()
    single = []
    bufs = [dev.put("s0", p), dev.put("s1", p)]
    for n in range(nmax):
        cpu.gpu_jacobi_sweep_masked(ca.ctypes.data, div.ctypes.data, cb.ctypes.data, solid.ctypes.data, rows.ctypes.data,
                                    ni, nj, nk, R.ALPHA, beta)
        hip.gpu_jacobi_sweep_masked(bufs[n % 2], dp, bufs[(n + 1) % 2], sp, rp, ni, nj, nk, R.ALPHA, beta)
        got = dev.get("s1" if n % 2 == 0 else "s0")
        assert np.array_equal(got, cb), ("single", n + 1)
        single.append(got)
        ca, cb = cb, ca
    check(hip)
    worst = 0.0
    for n in counts:
        ref = single[n - 1]
        err = float(np.abs(ref - its[n - 1]).max())
        assert err <= bounds[n - 1], (n, err, bounds[n - 1])
        worst = max(worst, err / bounds[n - 1])
        a, b = dev.put("f0", p), dev.put("f1", p)
        launches(hip)
        which = hip.gpu_jacobi_sweeps_masked(a, dp, b, sp, rp, ni, nj, nk, n, R.ALPHA, beta)
        check(hip)
        nl, ns = launches(hip)
        assert (nl, ns) == (expected_launches(n, fused), n), (n, nl, ns)
        assert which == nl % 2
        got = dev.get("f1" if which else "f0")
        assert np.array_equal(got, ref), ("fused", n)
        assert np.all(got[solid != 0] == 0) and not np.signbit(got[solid != 0]).any()
    return worst


@pytest.mark.parametrize("dims", FUSED + REFUSED)
def test_sweeps_on_adversarial_masks(libs, dims):
    """every mask family of obstacle_ref.mask_families, sweep counts 1 .. 7, KCHUNK2 = 8 so that chunk boundaries fall
    inside these grids; the fused kernel must run on the first four shapes and must not on the others"""
    hip, cpu = libs
    dev = Dev(hip)
    fused = dims in FUSED
    fams = R.mask_families(dims, kchunk=8)
    codes = R.codes(fams[-1][1])
    assert set(np.unique(codes[codes < 7])) == set(range(7))
    try:
        worst = 0.0
        with options(hip, JACOBI_FUSE=2, JACOBI_KCHUNK2=8):
            for seed, (name, solid) in enumerate(fams):
                counts = COUNTS if name in ("random", "i = 3 mod 4") or seed == 0 else (3, 7)
                try:
                    worst = max(worst, sweeps_case(hip, cpu, dev, dims, solid, seed, fused, counts))
                except AssertionError as e:
                    raise AssertionError(f"mask {name!r}: {e}") from e
        print(f"{dims}: largest error / bound {worst:.3g}")
    finally:
        dev.free()


def production_case(hip, cpu, dims, bnd, with_c):
    """default chunking: nine fused sweeps = nine single masked sweeps (= the C restatement when with_c)"""
    from gpufluidsimulation_amd.solver import boundary_array
    ni, nj, nk = dims
    h = 1.0 / ni
    arr, n = boundary_array(bnd)
    dev = Dev(hip)
    try:
        sp = dev.put("solid", np.zeros((nk, nj, ni), np.uint8))
        rp = dev.put("rows", np.zeros((nk, nj), np.uint8))
        hip.gpu_obstacle_flags(sp, rp, C.addressof(arr), n, h, ni, nj, nk)
        check(hip)
        solid, rows = dev.get("solid"), dev.get("rows")
        assert np.array_equal(rows, R.rows_of(solid))
        assert 0 < rows.mean() < 0.6
        p = R.initial_p(solid, 7)
        div = np.random.default_rng(8).standard_normal(solid.shape).astype(np.float32)
        dp = dev.put("div", div)
        beta = R.beta32()
        with options(hip, JACOBI_FUSE=2):        # what projectionObstacles sets; chunk length: auto
            which = hip.gpu_jacobi_sweeps_masked(dev.put("f0", p), dp, dev.put("f1", p), sp, rp, ni, nj, nk, 9, R.ALPHA, beta)
            check(hip)
            assert launches(hip) == (3, 9), "the fused masked kernel did not run"
        assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_masked_kernel"
        fused = dev.get("f1" if which else "f0")
        bufs = [dev.put("s0", p), dev.put("s1", p)]
        for s in range(9):
            hip.gpu_jacobi_sweep_masked(bufs[s % 2], dp, bufs[(s + 1) % 2], sp, rp, ni, nj, nk, R.ALPHA, beta)
        check(hip)
        single = dev.get("s1")
        assert np.array_equal(fused, single)
        assert not np.array_equal(single, p)
        if with_c:
            a, b = p.copy(), p.copy()
            assert cpu.gpu_jacobi_sweeps_masked(a.ctypes.data, div.ctypes.data, b.ctypes.data, solid.ctypes.data,
                                                rows.ctypes.data, ni, nj, nk, 9, R.ALPHA, beta) == 1
            assert np.array_equal(b, single)
    finally:
        dev.free()


def test_production_shape_256_cubed(libs):
    """the bench's central sphere (radius 0.15 L) and a box straddling the chunk boundary at plane 128 (chunks of 32)"""
    hip, cpu = libs
    bnd = [(0, 0.5, 0.5, 0.5, 0.15, 0, 0, 0, 0, 0),
           (1, 0.2, 0.75, 128.0 / 256, 0.05, 0.04, 4.3 / 256, 0, 0, 0)]
    production_case(hip, cpu, (256, 256, 256), bnd, with_c=True)


def test_production_shape_non_cubic(libs):
    """256 x 204 x 250: 26 row blocks with a remainder of 4 rows, chunks of 28 planes with a remainder of 26"""
    hip, cpu = libs
    h = 1.0 / 256
    bnd = [(0, 0.5, 0.45 * 204 * h, 0.5 * 250 * h, 0.12, 0, 0, 0, 0, 0),
           (1, 0.8, 199.6 * h, 0.3, 0.05, 0.03, 0.06, 0, 0, 0)]
    production_case(hip, cpu, (256, 204, 250), bnd, with_c=False)


@pytest.mark.parametrize("scheme", [0, 3])
def test_steps_at_256_cubed_fused_equals_single(libs, scheme):
    """five steps of the rising-smoke scene at 256^3, with defaults (the fused masked kernel runs) and with
    FL_OPT_JACOBI_FUSE = 0 (single masked sweeps only): identical hashes at every step"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    res = []
    for fuse in (None, 0):
        kv = {} if fuse is None else {"JACOBI_FUSE": fuse}
        with options(hip, **kv):
            res.append(OC.run_scene(solver.host_lib(), hip, 256, scheme, 5, 31))
            nl, ns = launches(hip)
        assert ns >= 5 * 30 and ns % 30 == 0, ns           # 30 masked sweeps per projection, one or two projections per step
        assert nl == (ns // 3 if fuse is None else ns), (fuse, nl, ns)
    assert res[0]["hashes"] == res[1]["hashes"]
    assert res[0]["rho_max"] > 0.1


@pytest.mark.parametrize("with_delta", [False, True])
def test_projection_pipeline_against_fp64(libs, with_delta):
    """the operators in projectionObstacles' order on 48 x 40 x 36 with a sphere and an overlapping box that move
    differently; exact where the contract is exact, within the derived bound elsewhere"""
    from gpufluidsimulation_amd.solver import boundary_array
    hip, _ = libs
    dims = (48, 40, 36)
    ni, nj, nk = dims
    h, bnd = R.edge_scene(dims)
    halfrdx = R.f32(0.5 / h)
    iters = 20
    arr, n = boundary_array(bnd)
    shapes = ((nk, nj, ni + 1), (nk, nj + 1, ni), (nk + 1, nj, ni))
    vel = [x.reshape(s) for x, s in zip(F.velocity(ni, nj, nk, h), shapes)]
    dev = Dev(hip)
    try:
        sp = dev.put("solid", np.zeros((nk, nj, ni), np.uint8))
        rp = dev.put("rows", np.zeros((nk, nj), np.uint8))
        hip.gpu_obstacle_flags(sp, rp, C.addressof(arr), n, h, ni, nj, nk)
        check(hip)
        solid, rows = dev.get("solid"), dev.get("rows")
        geo, tie = R.classify(bnd, h, (nk, nj, ni))
        assert tie.mean() < 1e-3
        assert np.array_equal(solid[~tie], np.maximum(geo, 0)[~tie].astype(np.uint8))
        flag = solid.astype(np.int32)                   # owners as built (equal to the geometry away from near ties)
        vp = [dev.put(nm, x) for nm, x in zip("uvw", vel)]
        dp3 = [dev.put("d" + nm, np.full(s, 9.0, np.float32)) for nm, s in zip("uvw", shapes)] if with_delta else [None] * 3
        pp = dev.put("p", np.zeros((nk, nj, ni), np.float32))
        pt = dev.put("pt", np.zeros((nk, nj, ni), np.float32))
        dv = dev.put("div", np.zeros((nk, nj, ni), np.float32))
        hip.gpu_obstacle_faces(*vp, *dp3, sp, C.addressof(arr), n, ni, nj, nk)
        faced = [dev.get(nm) for nm in "uvw"]
        if with_delta:
            dfaced = [dev.get("d" + nm) for nm in "uvw"]
        hip.gpu_divergence(*vp, dv, ni, nj, nk, halfrdx)
        div32 = dev.get("div")
        with options(hip, JACOBI_FUSE=2, JACOBI_KCHUNK2=8):
            which = hip.gpu_jacobi_sweeps_masked(pp, dv, pt, sp, rp, ni, nj, nk, iters - 1, R.ALPHA, R.beta32())
            assert launches(hip) == ((iters - 1) // 3 + (iters - 1) % 3, iters - 1)
        p32 = dev.get("pt" if which else "p")
        hip.gpu_gradient_masked(*vp, pt if which else pp, *dp3, sp, ni, nj, nk, halfrdx)
        check(hip)
        out = [dev.get(nm) for nm in "uvw"]
        dout = [dev.get("d" + nm) for nm in "uvw"] if with_delta else None

        # fp64 pipeline
        ref = R.solid_faces(*vel, flag, bnd)
        owners = R.face_owners(flag)
        shared = 0
        for c in range(3):
            sf = owners[c] > 0
            vtab = np.array([0.0] + [R.f32(b[7 + c]) for b in bnd], np.float32)
            vo = vtab[owners[c]]
            assert np.array_equal(faced[c][sf], vo[sf]) and np.array_equal(out[c][sf], vo[sf]), c
            assert np.array_equal(faced[c][~sf], vel[c][~sf])
            if with_delta:
                assert np.array_equal(dfaced[c][sf], vo[sf] - vel[c][sf]), c
                assert np.array_equal(dout[c][sf], vo[sf] - vel[c][sf]), c
            lo, hi = R.face_cells(flag, c)
            shared += int(((lo > 0) & (hi > 0) & (vtab[lo] != vtab[hi])).sum())
        assert shared > 0, "no face between two obstacles that move differently"
        div64, div_err = R.divergence(*ref[:3], halfrdx)
        assert np.all(np.abs(div32 - div64) <= div_err)
        its, bounds = R.masked_sweeps(np.zeros_like(div64), div64, solid, iters - 1)
        p_bound = bounds[-1] + (iters - 1) * abs(R.ALPHA) * float(div_err.max())
        p_err = float(np.abs(p32 - its[-1]).max())
        assert p_err <= p_bound
        assert np.all(p32[solid != 0] == 0) and not np.signbit(p32[solid != 0]).any()
        g = R.gradient_masked(*ref[:3], its[-1], solid, halfrdx)
        worst = p_err / p_bound
        for c in range(3):
            upd = g[6 + c]
            untouched = ~upd
            assert np.array_equal(out[c][untouched], faced[c][untouched]), c
            # |u - halfrdx (p0 - p1)|: the p error twice through halfrdx, three float32 roundings of the operands' size
            pmax = float(np.abs(its[-1]).max()) + p_bound
            bound = 2 * halfrdx * p_bound + 3 * R.U * (np.abs(g[c]) + 2 * halfrdx * pmax)
            err = np.abs(out[c] - g[c])
            assert np.all(err[upd] <= bound[upd]), c
            worst = max(worst, float((err[upd] / bound[upd]).max()))
            if with_delta:
                fluid_face = ~np.isnan(g[3 + c])
                assert np.all(dout[c][fluid_face & ~upd] == 0)
                derr = np.abs(dout[c] - g[3 + c])
                dbound = bound + R.U * np.abs(g[3 + c])
                assert np.all(derr[upd] <= dbound[upd] * (1 + 1e-6)), c
        print(f"pipeline: p error {p_err:.3g} of {p_bound:.3g}; largest error / bound {worst:.3g}")
    finally:
        dev.free()


@pytest.mark.parametrize("dims", [(99, 37, 23), (48, 40, 36), (64, 21, 30)])
def test_flags_rows_and_band_against_fp64_geometry(libs, dims):
    from gpufluidsimulation_amd.solver import boundary_array
    hip, _ = libs
    ni, nj, nk = dims
    h, bnd = R.edge_scene(dims)
    arr, n = boundary_array(bnd)
    dev = Dev(hip)
    try:
        sp = dev.put("solid", np.full((nk, nj, ni), 7, np.uint8))
        rp = dev.put("rows", np.full((nk, nj), 7, np.uint8))
        hip.gpu_obstacle_flags(sp, rp, C.addressof(arr), n, h, ni, nj, nk)
        check(hip)
        solid, rows = dev.get("solid"), dev.get("rows")
        flag, tie = R.classify(bnd, h, (nk, nj, ni))
        assert tie.mean() < 1e-3
        assert np.array_equal(solid[~tie], np.maximum(flag, 0)[~tie].astype(np.uint8))
        assert set(np.unique(solid)) == {0, 1, 2, 3, 4}
        ok = ~R.rows_tie(tie)
        assert np.array_equal(rows[ok], R.rows_of(np.maximum(flag, 0))[ok])
        assert np.array_equal(rows, R.rows_of(solid))
        # the band pass: gpu_semilag into a cleared field at the band nodes, every other node untouched
        u, v, w = F.velocity(ni, nj, nk, h)
        up, vp, wp = dev.put("u", u), dev.put("v", v), dev.put("w", w)
        cfldt = 0.9 * h / 0.35
        src_s = F.scalar(ni, nj, nk, 1.3)
        edge_zeros = 0
        for stag, src in (((1, 0, 0), u), ((0, 1, 0), v), ((0, 0, 1), w), ((0, 0, 0), src_s)):
            shape = (nk + stag[2], nj + stag[1], ni + stag[0])
            bflag, btie = R.classify(bnd, h, shape, stag)
            assert btie.mean() < 1e-3
            band = bflag == -1
            assert band.any()
            srcp = dev.put("src", src)
            full = dev.put("full", np.zeros(shape, np.float32))
            hip.gpu_semilag(full, srcp, up, vp, wp, *stag, h, ni, nj, nk, cfldt, -2.0 * h)
            got = dev.put("band", np.full(shape, -3.0, np.float32))
            hip.gpu_semilag_band(got, srcp, up, vp, wp, *stag, h, ni, nj, nk, cfldt, -2.0 * h, C.addressof(arr), n)
            check(hip)
            full, got = dev.get("full"), dev.get("band")
            sure = ~btie
            assert np.array_equal(got[band & sure], full[band & sure]), stag
            assert np.all(got[~band & sure] == -3.0), stag
            assert np.all((got[btie] == -3.0) | (got[btie] == full[btie]))
            # Q16: semilag_kernel writes only i, j, k in (1, n - 2 - stagger); band nodes outside that window are 0
            win = np.zeros(shape, bool)
            win[2:shape[0] - 2 - stag[2], 2:shape[1] - 2 - stag[1], 2:shape[2] - 2 - stag[0]] = True
            outside = band & sure & ~win
            assert np.all(got[outside] == 0) and not np.signbit(got[outside]).any(), stag
            edge_zeros += int(outside.sum())
            assert np.any(got[band & sure & win] != 0)
        assert edge_zeros > 0
    finally:
        dev.free()
