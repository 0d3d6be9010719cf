"""Passive tracer particles on the GPU: the four HIP operators against the C stand-in
(tests/cpu_abi/tracers_abi.c, itself checked against the oracle in tests/test_tracers_cpu.py), and the host solver's tracers on
the HIP library -- the invariant run, seeding, sorting, sampling.  Every comparison is on bits; every output is poisoned
before the call."""
import functools

import numpy as np
import pytest

import oracle_lib as OL
import tracers_case as TC

pytestmark = pytest.mark.gpu
f32 = np.float32
FL_OPT_FAST_LERP = 11
# power-of-two spacing; a spacing that is none; a long z axis with short rows (row and plane wraps near the walls)
GRIDS = [(16, 16, 16, 1.0 / 16), (40, 36, 30, 0.01), (12, 10, 67, 1.0 / 8)]
COUNTS = (1, 63, 64, 65, 257, 1000)                         # wave and block tails


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    lib.fl_set_option(FL_OPT_FAST_LERP, 0)
    yield lib
    lib.fl_set_option(FL_OPT_FAST_LERP, 0)
    bq.check()


@pytest.fixture(scope="module")
def cpu():
    return TC.load_tracers()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dev(a):
    from gpufluidsimulation_amd import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(a).view(f32) if a.dtype != f32 else a)


def dev_soa(pts):
    return [dev(np.ascontiguousarray(pts[:, c])) for c in range(3)]


@functools.lru_cache(maxsize=None)
def reference(grid):
    """velocity, particle sets and the stand-in's traces for a grid: computed once, frozen"""
    ni, nj, nk, h = grid
    h = float(f32(h))
    cfldt = 0.02
    cpu = TC.load_tracers()
    vel = TC.velocity((ni, nj, nk), h, cfldt)
    cases = {}
    for n in COUNTS:
        pts = TC.particles((ni, nj, nk), h, n, seed=n)
        for dt in (cfldt, 2.5 * cfldt, -2.5 * cfldt, 0.0):
            rc, want = TC.standin_trace(cpu, vel, pts, h, (ni, nj, nk), cfldt, dt)
            assert rc == 0
            want.setflags(write=False)
            cases[(n, dt)] = (pts, want)
    return h, cfldt, vel, cases


@pytest.mark.parametrize("grid", GRIDS)
def test_trace_equals_the_standin(hip, grid):
    import gpufluidsimulation_amd as bq
    ni, nj, nk, _ = grid
    h, cfldt, vel, cases = reference(grid)
    du, dv, dw = (dev(a) for a in vel)
    moved = False
    for (n, dt), (pts, want) in cases.items():
        px, py, pz = dev_soa(pts)
        rc = hip.gpu_trace_particles(du.ptr, dv.ptr, dw.ptr, px.ptr, py.ptr, pz.ptr, n, h, ni, nj, nk, cfldt, dt)
        assert rc == 0
        got = np.stack([px.numpy(), py.numpy(), pz.numpy()], axis=1)
        assert np.array_equal(bits(got), bits(want)), (grid, n, dt)
        moved = moved or not np.array_equal(bits(got), bits(pts))
    assert moved
    bq.check()


def test_trace_with_fast_lerp_equals_the_standins_fast_arithmetic(hip, cpu):
    """FL_OPT_FAST_LERP = 1: the twin build of the kernel, against the oracle's one-fma lerps"""
    grid = GRIDS[0]
    ni, nj, nk, _ = grid
    h, cfldt, vel, cases = reference(grid)
    pts, exact = cases[(1000, 2.5 * cfldt)]
    O = OL.lib()
    O.orc_set_fast_lerp(1)
    cpu.orc_set_fast_lerp(1)
    try:
        rc, want = TC.standin_trace(cpu, vel, pts, h, (ni, nj, nk), cfldt, 2.5 * cfldt)
    finally:
        O.orc_set_fast_lerp(0)
        cpu.orc_set_fast_lerp(0)
    assert rc == 0 and not np.array_equal(bits(want), bits(exact))
    du, dv, dw = (dev(a) for a in vel)
    px, py, pz = dev_soa(pts)
    hip.fl_set_option(FL_OPT_FAST_LERP, 1)
    try:
        assert hip.gpu_trace_particles(du.ptr, dv.ptr, dw.ptr, px.ptr, py.ptr, pz.ptr, 1000, h, ni, nj, nk, cfldt, 2.5 * cfldt) == 0
    finally:
        hip.fl_set_option(FL_OPT_FAST_LERP, 0)
    got = np.stack([px.numpy(), py.numpy(), pz.numpy()], axis=1)
    assert np.array_equal(bits(got), bits(want))


def test_trace_refusals_launch_nothing(hip):
    import gpufluidsimulation_amd as bq
    grid = GRIDS[0]
    ni, nj, nk, _ = grid
    h, cfldt, vel, cases = reference(grid)
    pts, _ = cases[(65, cfldt)]
    du, dv, dw = (dev(a) for a in vel)
    px, py, pz = dev_soa(pts)

    def call(u=du.ptr, x=px.ptr, n=65, dims=(ni, nj, nk), c=cfldt, dt=cfldt):
        rc = hip.gpu_trace_particles(u, dv.ptr, dw.ptr, x, py.ptr, pz.ptr, n, h, *dims, c, dt)
        err = hip.fl_last_error()
        hip.fl_clear_error()
        return rc, err

    bad = (TC.BAD_ARGUMENT, TC.BAD_ARGUMENT)
    assert call(u=None) == bad and call(x=None) == bad and call(n=-1) == bad and call(dims=(4, nj, nk)) == bad
    assert call(c=0.0) == bad and call(c=-1.0) == bad and call(x=du.ptr) == bad
    assert call(c=0.0, dt=0.0) == (0, 0) and call(n=0) == (0, 0)
    hip.fl_set_slab(0, nk, 0, nk, nk)
    try:
        assert call() == (TC.UNSUPPORTED, TC.UNSUPPORTED)
    finally:
        hip.fl_set_slab(0, 0, 0, 0, 0)
    assert np.array_equal(bits(px.numpy()), bits(pts[:, 0]))    # nothing ran
    bq.check()


@pytest.mark.parametrize("grid", GRIDS)
def test_sample_equals_the_standin_for_all_five_staggers(hip, cpu, grid):
    ni, nj, nk, h = grid
    h = float(f32(h))
    dims = (ni, nj, nk)
    rng = np.random.default_rng(11)
    n = 1000
    span = np.array(dims, f32) * f32(h)
    pts = np.ascontiguousarray((rng.random((n, 3)).astype(f32) * f32(1.6) - f32(0.3)) * span)   # inside, on and outside the grid
    soa = np.ascontiguousarray(pts.T.copy())
    px, py, pz = dev_soa(pts)
    for name in TC.SAMPLED:
        extra, off = TC.stagger(name, h)
        nx, ny, nz = (dims[c] + extra[c] for c in range(3))
        field = np.ascontiguousarray(rng.standard_normal((nz, ny, nx)).astype(f32))
        want = np.full(n, 7.0, f32)
        assert cpu.gpu_sample_particles(TC.ptr(field), nx, ny, nz, h, *off, TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]), TC.ptr(want), n) == 0
        df, out = dev(field), dev(np.full(n, np.nan, f32))
        assert hip.gpu_sample_particles(df.ptr, nx, ny, nz, h, *off, px.ptr, py.ptr, pz.ptr, out.ptr, n) == 0
        assert np.array_equal(bits(out.numpy()), bits(want)), (grid, name)
        assert (want == 0).any() and (want != 0).any()


@pytest.mark.parametrize("grid", GRIDS)
def test_seed_equals_the_standin(hip, cpu, grid):
    ni, nj, nk, h = grid
    h = float(f32(h))
    for lo, hi, per_cell, seed in [((0, 0, 0), (ni, nj, nk), 2, 7), ((3, 2, 5), (9, 4, 40), 5, 0xFFFFFFFF), ((-5, 1, 1), (2, 3, 3), 1, 0)]:
        lo2, ext = TC.seed_box(lo, hi, (ni, nj, nk))
        n = ext[0] * ext[1] * ext[2] * per_cell
        assert n > 0
        want = np.full((3, n), -1.0, f32)
        assert cpu.gpu_seed_particles(TC.ptr(want[0]), TC.ptr(want[1]), TC.ptr(want[2]), lo[0], hi[0], lo[1], hi[1], lo[2], hi[2],
                                      per_cell, seed, h, ni, nj, nk) == 0
        poison = np.full(n + 64, np.nan, f32)                   # 64 floats past the end must stay untouched
        px, py, pz = dev(poison), dev(poison), dev(poison)
        assert hip.gpu_seed_particles(px.ptr, py.ptr, pz.ptr, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], per_cell, seed, h, ni, nj, nk) == 0
        for c, b in enumerate((px, py, pz)):
            got = b.numpy()
            assert np.array_equal(bits(got[:n]), bits(want[c])), (grid, lo, c)
            assert np.isnan(got[n:]).all()
        pos, _, _ = TC.seed_restate(lo, hi, per_cell, seed, h, (ni, nj, nk))
        assert np.array_equal(bits(want.T), bits(pos))


@pytest.mark.parametrize("grid", GRIDS)
def test_sort_groups_by_brick_and_keeps_pairs(hip, cpu, grid):
    ni, nj, nk, h = grid
    h = float(f32(h))
    dims = (ni, nj, nk)
    for n, with_ids in ((1, True), (65, False), (3000, True)):
        pts = TC.particles(dims, h, n, seed=3 + n)
        ids = np.random.default_rng(n).permutation(n).astype(np.uint32)
        px, py, pz = dev_soa(pts)
        did = dev(ids) if with_ids else None
        out = [dev(np.full(n, np.nan, f32)) for _ in range(3)]
        oid = dev(np.full(n, 0xFFFFFFFF, np.uint32))
        rc = hip.gpu_sort_particles(px.ptr, py.ptr, pz.ptr, did.ptr if with_ids else None, out[0].ptr, out[1].ptr, out[2].ptr, oid.ptr,
                                    n, h, ni, nj, nk)
        assert rc == 0
        got = np.stack([b.numpy() for b in out], axis=1)
        gid = oid.numpy().view(np.uint32)
        keys = TC.brick_keys(got, h, dims)
        assert (np.diff(keys) >= 0).all()
        assert sorted(gid.tolist()) == list(range(n))
        src = np.argsort(ids) if with_ids else np.arange(n)     # id -> input slot
        assert np.array_equal(bits(got), bits(pts[src[gid]]))
        # the stand-in's stable sort holds the same particles in every brick
        want = np.full((3, n), -1.0, f32)
        wid = np.zeros(n, np.uint32)
        soa = np.ascontiguousarray(pts.T.copy())
        assert cpu.gpu_sort_particles(TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]), TC.ptr(ids) if with_ids else None,
                                      TC.ptr(want[0]), TC.ptr(want[1]), TC.ptr(want[2]), TC.ptr(wid), n, h, ni, nj, nk) == 0
        assert np.array_equal(keys, TC.brick_keys(want.T, h, dims))
        a, b = np.lexsort((gid, keys)), np.lexsort((wid, keys))
        assert np.array_equal(gid[a], wid[b]) and np.array_equal(bits(got[a]), bits(want.T[b]))


@pytest.mark.parametrize("node_lookups", [0, 1])
def test_node_seeded_tracers_stay_on_the_forward_map(hip, node_lookups):
    """the invariant run of tests/test_tracers_cpu.py on the HIP library, with the hinted map kernels off and on"""
    s = TC.invariant_solver(**{str(TC.OPT_NODE_LOOKUPS): node_lookups})
    assert TC.check_invariant(s) > 0.1
    s.close()


def run_sorted(every, steps=6):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    n = 24
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, TC.INV_EMITTER)
    s.setProjection(TC.INV_ITERS, 0.5)
    s.setOption(TC.OPT_TRACER_SORT_EVERY, every)
    assert s.seedTracers((0, 0, 0), (n, n, n), 2, 1) == 2 * (n - 2) ** 3
    out = []
    for frame in range(steps):
        s.advance(frame, TC.INV_DT)
        if frame == 2:
            s.seedTracers((5, 5, 5), (12, 9, 11), 1, 9)         # appended after the first sort
        out.append((s.tracers(), s.tracerSample("rho")))
    stored, ids = s.tracersStored()
    fields = {name: s.field(name).reshape([d + e for d, e in zip((n, n, n), TC.SAMPLED[name][0])][::-1]) for name in TC.SAMPLED}
    samples = {name: s.tracerSample(name) for name in TC.SAMPLED}
    s._check()
    s.close()
    return out, stored, ids, fields, samples, s.h


def test_sorting_changes_no_public_bit_and_sorts_the_stored_order(hip, cpu):
    base, stored0, ids0, _, _, _ = run_sorted(0)
    got, stored, ids, fields, samples, h = run_sorted(2)
    assert np.array_equal(ids0, np.arange(len(ids0)))
    for frame, (a, b) in enumerate(zip(base, got)):
        for x, y in zip(a, b):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), frame
    assert sorted(ids.tolist()) == list(range(len(ids))) and not np.array_equal(ids, np.arange(len(ids)))
    assert np.array_equal(bits(stored), bits(got[-1][0][ids]))
    keys = TC.brick_keys(stored, h, (24, 24, 24))              # 6 steps, every 2: the last step ended with a sort
    assert (np.diff(keys) >= 0).all() and len(np.unique(keys)) > 100
    # tracerSample of all five fields against orc_sample on the downloaded fields
    O = OL.lib()
    pts = got[-1][0]
    pick = np.random.default_rng(0).choice(len(pts), 1500, replace=False)
    for name, field in fields.items():
        extra, off = TC.stagger(name, h)
        nz, ny, nx = field.shape
        f = np.ascontiguousarray(field, f32)
        want = np.array([O.orc_sample(OL.fp(f), nx, ny, nz, float(h), *off, float(p[0]), float(p[1]), float(p[2])) for p in pts[pick]], f32)
        assert np.array_equal(bits(samples[name][pick]), bits(want)), name
        # ... and at EVERY tracer through the stand-in's loop over orc_sample
        soa = np.ascontiguousarray(pts.T.copy())
        every = np.full(len(pts), 7.0, f32)
        assert cpu.gpu_sample_particles(TC.ptr(f), nx, ny, nz, float(h), *off, TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]),
                                        TC.ptr(every), len(pts)) == 0
        assert np.array_equal(bits(samples[name]), bits(every)), name
    assert np.abs(samples["rho"]).max() > 0 and np.abs(samples["v"]).max() > 0
