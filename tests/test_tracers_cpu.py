"""Passive tracer particles without a GPU: the C stand-in of the four operators
(tests/cpu_abi/tracers_abi.c) against the unmodified oracle and against numpy restatements written from the header's text,
and the host solver's tracers on that stand-in -- the invariant run (a tracer seeded on a grid node stays, bit for bit, on
the forward map's entry of that node), seeding, sorting, refusals, the dump.  Every comparison is on bits."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle_lib as OL
import tracers_case as TC

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [((16, 16, 16), 1.0 / 16), ((14, 12, 11), 0.01)]


@pytest.fixture(scope="module")
def standin():
    return TC.load_tracers()


@pytest.fixture(scope="module")
def plain():
    """the render stand-in, WITHOUT the tracer operators: the host solver's weak references stay null"""
    import obstacle_case as OC
    from build_cpu_render import build_render
    from gpufluidsimulation_amd import solver
    return OC.bind_errors(solver.bind_host(C.CDLL(build_render(), mode=C.RTLD_LOCAL)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. the operators against the unmodified oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("dims,h", GRIDS)
def test_trace_equals_the_oracle_forward_map(standin, dims, h):
    O = OL.lib()
    h = float(f32(h))
    cfldt = 0.02
    vel = TC.velocity(dims, h, cfldt)
    for n in (1, 65, 700):                                  # 700 needs two chunks of the 7 x 8 x 10 interior of the small grid
        pts = TC.particles(dims, h, n)
        for dt in (cfldt, 2.5 * cfldt, -2.5 * cfldt, 0.0):
            want = TC.oracle_trace(O, vel, pts, h, dims, cfldt, dt)
            rc, got = TC.standin_trace(standin, vel, pts, h, dims, cfldt, dt)
            assert rc == 0
            assert np.array_equal(bits(got), bits(want)), (n, dt)
            if dt == 0.0:
                assert np.array_equal(bits(got), bits(pts))
            else:
                assert not np.array_equal(bits(got), bits(pts))
            lo, hi = f32(h), np.array(TC.box_hi(dims, h), f32)
            assert (got >= lo).all() and (got <= hi).all()


@pytest.mark.parametrize("dims,h", GRIDS)
def test_sample_equals_orc_sample_for_all_five_staggers(standin, dims, h):
    O = OL.lib()
    h = float(f32(h))
    rng = np.random.default_rng(5)
    n = 300
    # inside, on the faces and OUTSIDE the grid on every side: taps outside the allocation read zero
    span = np.array(dims, f32) * f32(h)
    pts = (rng.random((n, 3)).astype(f32) * f32(1.6) - f32(0.3)) * span
    soa = np.ascontiguousarray(pts.T.copy())
    saw_zero_tap = False
    for name in TC.SAMPLED:
        extra, off = TC.stagger(name, h)
        nx, ny, nz = (dims[c] + extra[c] for c in range(3))
        field = np.ascontiguousarray(rng.standard_normal((nz, ny, nx)).astype(f32))
        out = np.full(n, 7.0, f32)
        rc = standin.gpu_sample_particles(TC.ptr(field), nx, ny, nz, h, *off, TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]), TC.ptr(out), n)
        assert rc == 0
        want = np.array([O.orc_sample(OL.fp(field), nx, ny, nz, h, *off, float(p[0]), float(p[1]), float(p[2])) for p in pts], f32)
        assert np.array_equal(bits(out), bits(want)), name
        saw_zero_tap = saw_zero_tap or bool((want == 0).any())
    assert saw_zero_tap


# ---- 2. the invariant run -----------------------------------------------------------------------------------------------
def test_node_seeded_tracers_stay_on_the_forward_map(standin):
    s = TC.invariant_solver(standin, standin)
    moved = TC.check_invariant(s)
    assert moved > 0.1
    s.close()


@pytest.mark.parametrize("scheme", [2, 3])
def test_other_schemes_trace_through_the_old_velocity(standin, scheme):
    """MacCormack and reflection: the tracers take the oracle's trace over dt through the velocity the step starts with,
    with that step's getCFL() value"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    O = OL.lib()
    n = 12
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=standin, errlib=standin, scheme=scheme)
    s.setSmoke(0.0, 1.0, [(0.5, 0.3, 0.5, 0.2, 1.0, 2.0, 1.0, 1000)])
    s.setProjection(20, 0.5)
    assert s.seedTracers((0, 0, 0), (n, n, n), 1, 3) == (n - 2) ** 3
    for frame in range(3):
        vel = [s.field(c).reshape(shape) for c, shape in (("u", (n, n, n + 1)), ("v", (n, n + 1, n)), ("w", (n + 1, n, n)))]
        before = s.tracers()
        s.advance(frame, 0.05)
        s._check()
        want = TC.oracle_trace(O, vel, before, s.h, (n, n, n), s.cfldt, 0.05)
        assert np.array_equal(bits(s.tracers()), bits(want)), frame
    assert not np.array_equal(bits(s.tracers()), bits(before))
    s.close()


# ---- 3. seeding ---------------------------------------------------------------------------------------------------------
def test_seeding_matches_the_header_text(standin):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    dims, L = (16, 16, 16), 1.0
    s = BimocqGPUSolver(*dims, L, 0.0, 1.0, lib=standin, errlib=standin)
    h = s.h
    # a box that sticks out of the grid on both sides is cut to the cells 1 .. n - 2
    added = s.seedTracers((-3, 2, 5), (40, 9, 11), 3, 77)
    pos, cells, frac = TC.seed_restate((-3, 2, 5), (40, 9, 11), 3, 77, h, dims)
    assert added == 14 * 7 * 6 * 3 == len(pos) and s.tracerCount() == added
    got = s.tracers()
    assert np.array_equal(bits(got), bits(pos))
    # k outermost, then j, then i, then the sample
    assert cells[0].tolist() == [1, 2, 5] and cells[3].tolist() == [2, 2, 5] and cells[3 * 14].tolist() == [1, 3, 5]
    # every particle in its own (closed) cell and in the clamp box
    hf = f32(h)
    assert (got >= (cells.astype(f32) * hf)).all() and (got <= ((cells + 1).astype(f32) * hf)).all()
    assert (got >= hf).all() and (got <= np.array(TC.box_hi(dims, h), f32)).all()
    # appended ids continue; the same cell gets the same jitter from another box
    added2 = s.seedTracers((4, 4, 6), (8, 6, 9), 3, 77)
    pos2, cells2, _ = TC.seed_restate((4, 4, 6), (8, 6, 9), 3, 77, h, dims)
    assert added2 == 4 * 2 * 3 * 3 and s.tracerCount() == added + added2
    both = s.tracers()
    assert np.array_equal(bits(both[:added]), bits(pos)) and np.array_equal(bits(both[added:]), bits(pos2))
    key = {tuple(c) + (a % 3,): a for a, c in enumerate(cells.tolist())}
    for a, c in enumerate(cells2.tolist()):
        assert np.array_equal(bits(pos2[a]), bits(pos[key[tuple(c) + (a % 3,)]]))
    # another seed moves them; an empty box adds nothing
    assert not np.array_equal(TC.seed_restate((4, 4, 6), (8, 6, 9), 3, 78, h, dims)[0], pos2)
    assert s.seedTracers((5, 5, 5), (5, 9, 9), 2, 0) == 0 and s.tracerCount() == added + added2
    s.close()


def test_jitter_is_uniform_enough(standin):
    """per_cell = 4 on 16^3, seed 2024: the mean of the 3 n fractions lies within four standard errors of 1/2"""
    dims, h = (16, 16, 16), 1.0 / 16
    n = 14 ** 3 * 4
    soa = np.full((3, n), -1.0, f32)
    assert standin.gpu_seed_particles(TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]), 0, 16, 0, 16, 0, 16, 4, 2024, h, *dims) == 0
    pos, cells, frac = TC.seed_restate((0, 0, 0), (16, 16, 16), 4, 2024, h, dims)
    assert np.array_equal(bits(soa.T), bits(pos))
    for c in range(3):
        assert abs(float(frac[:, c].astype(np.float64).mean()) - 0.5) <= 4.0 / math.sqrt(12.0 * n), c
        # the stored positions carry those fractions, rounded once by the float sum (h a power of two: the product is exact)
        assert np.array_equal((pos[:, c] / f32(h)).astype(f32), (cells[:, c].astype(f32) + frac[:, c]).astype(f32))
    assert len(np.unique(frac.view(np.uint32))) > 0.99 * frac.size


# ---- 4. sorting ---------------------------------------------------------------------------------------------------------
def test_sort_operator_groups_by_brick_and_keeps_pairs(standin):
    dims, h = (14, 12, 11), float(f32(0.01))
    n = 500
    pts = TC.particles(dims, h, n, seed=9)
    soa = np.ascontiguousarray(pts.T.copy())
    ids = np.ascontiguousarray(np.random.default_rng(2).permutation(n).astype(np.uint32))
    for given in (ids, None):
        out, oid = np.full((3, n), -1.0, f32), np.full(n, 0xFFFFFFFF, np.uint32)
        rc = standin.gpu_sort_particles(TC.ptr(soa[0]), TC.ptr(soa[1]), TC.ptr(soa[2]), TC.ptr(given), TC.ptr(out[0]), TC.ptr(out[1]),
                                        TC.ptr(out[2]), TC.ptr(oid), n, h, *dims)
        assert rc == 0
        keys = TC.brick_keys(out.T, h, dims)
        assert (np.diff(keys) >= 0).all() and len(np.unique(keys)) > 10
        src = np.arange(n) if given is None else np.argsort(ids)       # id -> input slot
        assert sorted(oid.tolist()) == list(range(n))
        assert np.array_equal(bits(out.T), bits(pts[src[oid]]))


def run_sorted(lib, every, steps=6):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    n = 16
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=lib, errlib=lib)
    s.setSmoke(0.0, 1.0, [(0.5, 0.3, 0.4, 0.2, 1.0, 2.0, 1.0, 1000)])
    s.setProjection(20, 0.5)
    s.setOption(TC.OPT_TRACER_SORT_EVERY, every)
    assert s.getOption(TC.OPT_TRACER_SORT_EVERY) == every
    s.seedTracers((2, 2, 2), (14, 10, 14), 2, 1)
    out = []
    for frame in range(steps):
        s.advance(frame, 0.05)
        if frame == 3:
            s.seedTracers((3, 3, 3), (9, 9, 9), 1, 5)          # appended after a sort has run (every = 1 and 3)
        out.append((s.tracers(), s.tracerSample("rho"), s.tracerSample("u")))
    stored, ids = s.tracersStored()
    s._check()
    s.close()
    return out, stored, ids


def test_sorting_changes_no_public_bit(standin):
    base, stored0, ids0 = run_sorted(standin, 0)
    assert np.array_equal(ids0, np.arange(len(ids0)))           # never sorted: no id array, the identity
    assert np.abs(base[-1][1]).max() > 0
    for every in (1, 3):
        got, stored, ids = run_sorted(standin, every)
        for frame, (a, b) in enumerate(zip(base, got)):
            for x, y in zip(a, b):
                assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (every, frame)
        assert sorted(ids.tolist()) == list(range(len(ids))) and not np.array_equal(ids, np.arange(len(ids)))
        assert np.array_equal(bits(stored), bits(got[-1][0][ids]))
        keys = TC.brick_keys(stored, 1.0 / 16, (16, 16, 16))
        if every in (1, 3):                                     # 6 steps: both have just sorted
            assert (np.diff(keys) >= 0).all()


# ---- 5. refusals and edges ----------------------------------------------------------------------------------------------
def test_refusals_and_edges(standin, tmp_path):
    from gpufluidsimulation_amd import BimocqError, solver
    n = 12
    s = solver.BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, lib=standin, errlib=standin)
    good = np.array([[0.5, 0.5, 0.5], [0.25, 0.3, 0.7]], f32)
    s.setTracers(good)
    assert s.tracerCount() == 2 and np.array_equal(s.tracers(), good)
    for bad in (np.nan, np.inf, -np.inf):
        broken = good.copy()
        broken[1, 2] = bad
        with pytest.raises(BimocqError, match="error 3"):
            s.setTracers(broken)
        assert s.tracerCount() == 0                              # a failure leaves no tracers
        s.setTracers(good)
    # an out-of-box position is clamped componentwise into [h, (n - 1) h]
    h = f32(s.h)
    hi = np.array(TC.box_hi((n, n, n), h), f32)
    s.setTracers(np.array([[-4.0, 0.5, 99.0], [0.0, float(h) / 2, 1.0]], f32))
    assert np.array_equal(s.tracers(), np.array([[h, f32(0.5), hi[2]], [h, h, hi[2]]], f32))
    # n = 0 releases
    s.setTracers(np.empty((0, 3), f32))
    assert s.tracerCount() == 0 and s.tracers().shape == (0, 3) and s.tracerSample("rho").shape == (0,)
    # the cap: one more than BQ_MAX_TRACERS is refused before anything is read or uploaded (the pointer is never touched)
    assert solver.MAX_TRACERS == 1 << 26
    assert standin.bq_solver_set_tracers(s.s, good.ctypes.data, solver.MAX_TRACERS + 1) == TC.BAD_ARGUMENT
    assert standin.fl_last_error() == TC.BAD_ARGUMENT
    standin.fl_clear_error()
    with pytest.raises(BimocqError, match="error 3"):
        s.seedTracers((0, 0, 0), (n, n, n), (solver.MAX_TRACERS // (n - 2) ** 3) + 1, 0)
    assert s.tracerCount() == 0
    with pytest.raises(BimocqError, match="error 3"):
        s.seedTracers((0, 0, 0), (n, n, n), 0, 0)
    with pytest.raises(BimocqError, match="error 3"):
        s.setOption(TC.OPT_TRACER_SORT_EVERY, -1)
    s.setTracers(good)
    with pytest.raises(BimocqError, match="error 3"):
        s.tracerSample("p")
    # the dump parses back to tracers() and the attribute
    s.setSmoke(0.0, 1.0, [(0.5, 0.3, 0.5, 0.2, 1.0, 2.0, 1.0, 1000)])
    s.setProjection(10, 0.5)
    s.seedTracers((3, 2, 3), (9, 8, 9), 2, 4)
    for frame in range(2):
        s.advance(frame, 0.05)
    out = str(tmp_path / "dump")
    nbytes = s.outputTracers(1, out, "T")
    path = os.path.join(out, "tracers_0002.bqp")
    assert os.path.getsize(path) == nbytes == 44 + 16 * s.tracerCount()
    hd, xyz, attr = solver.read_tracer_dump(path)
    assert (hd["frame"], hd["count"], hd["nx"], hd["ny"], hd["nz"], hd["attribute"]) == (2, s.tracerCount(), n, n, n, solver.FIELD_IDS["T"])
    assert f32(hd["h"]) == h
    assert np.array_equal(bits(xyz), bits(s.tracers())) and np.array_equal(bits(attr), bits(s.tracerSample("T")))
    assert np.abs(attr).max() > 0
    assert s.outputTracers(2, out) == 44 + 12 * s.tracerCount()
    hd, xyz, attr = solver.read_tracer_dump(os.path.join(out, "tracers_0003.bqp"))
    assert hd["attribute"] == -1 and attr is None and np.array_equal(bits(xyz), bits(s.tracers()))
    s.close()


def test_a_slab_solver_refuses_tracers(standin):
    from gpufluidsimulation_amd import BimocqError, solver
    s = solver.BimocqGPUSolver(16, 16, 16, 1.0, 0.0, 1.0, lib=standin, errlib=standin, rank=0, nranks=1, ghost=4)
    assert s.slab_on
    with pytest.raises(BimocqError, match="error 4"):
        s.setTracers(np.full((1, 3), 0.5, f32))
    with pytest.raises(BimocqError, match="error 4"):
        s.seedTracers((2, 2, 2), (4, 4, 4))
    with pytest.raises(BimocqError, match="error 4"):
        s.setOption(TC.OPT_TRACER_SORT_EVERY, 2)
    assert s.tracerCount() == 0
    s.close()


def test_a_standin_without_the_operators_is_unsupported(plain):
    from gpufluidsimulation_amd import BimocqError, solver
    s = solver.BimocqGPUSolver(12, 12, 12, 1.0, 0.0, 1.0, lib=plain, errlib=plain)
    with pytest.raises(BimocqError, match="error 4"):
        s.setTracers(np.full((1, 3), 0.5, f32))
    assert s.tracerCount() == 0
    s.setTracers(np.empty((0, 3), f32))                         # releasing nothing is always fine
    s.advance(0, 0.05)
    s._check()
    s.close()


def test_tracers_set_and_removed_leave_the_run_alone(standin):
    """a run that sets tracers and removes them before frame 0 equals, field by field, a run that never had any -- and
    without tracers advance() calls none of the four operators"""
    from gpufluidsimulation_amd import solver
    fields = ("rho", "T", "u", "v", "w", "p", "fx", "fy", "fz", "bx", "by", "bz")

    def run(touch):
        s = TC.invariant_solver(standin, standin)
        if touch:
            s.setOption(TC.OPT_TRACER_SORT_EVERY, 1)
            s.setTracers(TC.node_positions(s))
            s.seedTracers((2, 2, 2), (6, 6, 6), 2, 1)
            s.setTracers(np.empty((0, 3), f32))
        standin.tracers_abi_calls(1)
        for frame in range(3):
            s.advance(frame, TC.INV_DT)
        s._check()
        assert standin.tracers_abi_calls(1) == 0
        out = {name: s.field(name) for name in fields}
        s.close()
        return out

    a, b = run(False), run(True)
    for name in fields:
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    assert np.abs(a["v"]).max() > 0.01
    assert solver.OPT_TRACER_SORT_EVERY == 17
    assert "BQ_OPT_TRACER_SORT_EVERY = 17" in open(os.path.join(ROOT, "include", "bimocq_solver.h")).read()
