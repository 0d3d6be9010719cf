"""The needle-shaped grids and the smallest accepted grids (tests/needle_case.py) on a machine without a GPU:

* every operator case of the needles is non-vacuous -- computed on the oracle alone, so that a shape whose far end holds nothing
  is caught here and not on the GPU machine;
* the same cases, SMALL shapes included, on the CPU stand-in of the C-ABI (tests/cpu_abi/oracle_abi.c): the stand-in calls the
  oracle, so this checks the cases themselves -- argument order, output lists, the start of every output -- before a GPU sees them;
* two whole steps of the C++ host solver on the stand-in against OracleSolver on each needle: the host side's size arithmetic
  (allocation sizes, plane strides, reductions over 26 M elements) at these shapes.

Whole steps run scheme 0 (BiMocq) on the needles and schemes 0 and 3 (reflection) on the SMALL shapes the solver accepts: they are
the two schemes OracleSolver implements; MacCormack (scheme 2) has no oracle state machine (tests/test_maccormack_cpu.py holds it
to its own restatement).

Cost.  The host's size arithmetic depends on the length of the needle, not on its cross-section, so the step cases run the
thinnest needles bq_solver_create takes (needle_case.STEP_NEEDLES: a cross-section of 8 x 8, which still holds the emitter of
radius 3 h).  A step of the oracle visits every cell some fifty times and is what the time goes to: measured on 8 cores, one
oracle step of the scene takes 7 s at 4.2 M cells (65560 x 8 x 8) and the stand-in's step as long again, so two steps of both
take about 27 s on the x and z needles and about 100 s on 8 x 262160 x 8 (16.8 M cells).  They are the slow tests of this file;
everything else in it takes a few seconds or less per test."""
import ctypes as C

import pytest

import host_entry_case as H
import needle_case as N
from build_cpu_host import build as build_cpu_host

# the stand-in has neither the *_hint entry points nor gpu_maccormack; their references are judged here all the same
STAND_IN = [n for n in N.CASES if not n.endswith("_hint") and not n.startswith("maccormack")]
ACCEPTED_BY_THE_SOLVER = [d for d in N.SMALL if min(d) >= 8]          # bq_solver_create: every dimension >= 8


@pytest.fixture(scope="module")
def be():
    lib = H.bind(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL))
    lib.orc_set_fast_lerp.restype, lib.orc_set_fast_lerp.argtypes = None, [C.c_int]
    backend = H.Backend(lib, lib.orc_set_fast_lerp, "cpu stand-in")
    yield backend
    backend.lib.orc_set_fast_lerp(0)
    backend.check()


@pytest.fixture(scope="module")
def cpu_host():
    from gpufluidsimulation_amd import solver
    lib = solver.bind_host(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL))
    for name, res, args in (("fl_last_error", C.c_int, []), ("fl_last_error_string", C.c_char_p, []), ("fl_clear_error", None, [])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def test_shapes_are_what_the_cases_need():
    """the far end is not empty and holds interior cells of the gather operators (3 .. n - 4); the limits the needles sit at;
    the emitter of the step scene lies within the last 16 cells and is at least 2.5 h wide"""
    import numpy as np
    for dims in N.NEEDLES:
        la = N.long_axis(dims)
        assert la == N.NEEDLES.index(dims)
        assert 4.0 * (dims[0] + 1) * (dims[1] + 1) * (dims[2] + 1) < 2.0 ** 31 and (dims[0] + 1) * (dims[1] + 1) < 2 ** 23
        assert dims[2] + 1 <= 65535
        for axis in (-1, 0, 1, 2):
            bi, bj, bk = H.stag(*dims, axis)
            far = N.far_end(np.zeros(bi * bj * bk, np.float32), dims, axis)
            first = (bk, bj, bi)[2 - la] - far.shape[2 - la]
            assert far.size > 0 and first == (N.FAR_FROM[la] if la < 2 else bk - N.FAR_PLANES)
            assert dims[la] - 3 - first >= 8                        # eight interior indices (3 .. n - 4) at least, 4 x 4 cells each
        centre = N.far_emitter(dims, N.H_POW2)
        assert dims[la] - 16 <= centre[la] / N.H_POW2 < dims[la] and centre[3] >= 2.5 * N.H_POW2
    for dims, full in zip(N.STEP_NEEDLES, N.NEEDLES):
        la = N.long_axis(dims)
        centre = N.far_emitter(dims, N.H_POW2)
        assert dims[la] == full[la] and sorted(dims)[:2] == [8, 8] and dims[la] - 16 <= centre[la] / N.H_POW2 < dims[la]
        assert centre[3] >= 2.5 * N.H_POW2 and all(centre[3] <= centre[a] <= dims[a] * N.H_POW2 - centre[3] for a in range(3) if a != la)
    assert N.LONG_X[0] > 1024 * 64 and (N.LONG_Y[1] + 3) // 4 > 65535 and (N.LONG_Y[1] + 4) // 4 == 65541 and N.LONG_Z[2] + 1 == 65535
    for dims in N.SMALL:
        assert N.long_axis(dims) is None and max(dims) - 6 <= 4     # four interior cells per axis at the most


@pytest.mark.parametrize("dims,name", [(d, n) for d in N.NEEDLES for n in N.CASES], ids=lambda v: v if isinstance(v, str) else N.ident(v))
def test_needle_case_is_not_vacuous(dims, name):
    """the oracle's output differs from what it started as, and from zero, in at least 16 elements of the far end (asserted inside
    needle_case.reference); h = 1/8, exact lerps: the condition does not depend on the spacing or the lerp variant"""
    N.reference(N.inputs(dims, N.H_POW2), name)


@pytest.mark.parametrize("h", N.SPACINGS)
@pytest.mark.parametrize("dims", N.SMALL, ids=N.ident)
def test_small_shapes_on_the_stand_in(be, dims, h):
    """every case, both lerp variants, on shapes whose interior is empty or a handful of cells"""
    r = N.Runner(be, dims, h)
    for name in STAND_IN:
        for fast in ((0, 1) if N.CASES[name].lerp else (0,)):
            N.run_case(r, name, fast)


@pytest.mark.parametrize("dims", [N.LONG_X, N.LONG_Z], ids=N.ident)
def test_needle_cases_on_the_stand_in(be, dims):
    """one gather, one map update, one streaming and one projection case through the stand-in at a needle: the call side of the
    cases at the sizes the GPU test uses them"""
    r = N.Runner(be, dims, N.H_TABLED)
    for name in ("advect_field", "solve_backwardDMC", "emit_smoke", "jacobi_sweeps_4"):
        N.run_case(r, name, 0)


@pytest.mark.parametrize("scheme", [0, 3])
@pytest.mark.parametrize("dims", ACCEPTED_BY_THE_SOLVER, ids=N.ident)
def test_host_solver_steps_on_small_shapes(cpu_host, dims, scheme):
    N.run_steps(dims, scheme, lib=cpu_host, errlib=cpu_host)


@pytest.mark.parametrize("dims", [d for d in N.SMALL if d not in ACCEPTED_BY_THE_SOLVER], ids=N.ident)
def test_host_solver_refuses_the_smallest_shapes(cpu_host, dims):
    """bq_solver_create takes no dimension below 8 (the operators do: see the cases above): a null handle before anything is
    allocated or called, so nothing is latched either"""
    cpu_host.fl_clear_error()
    assert not cpu_host.bq_solver_create(0, *dims, dims[0] * N.H_POW2, 0.0, 1.0, 0)
    assert cpu_host.fl_last_error() == 0


@pytest.mark.parametrize("dims", N.STEP_NEEDLES, ids=N.ident)
def test_host_solver_steps_on_needles(cpu_host, dims):
    """emitter at the far end, 8 Jacobi sweeps, two steps: every field of both steps equals OracleSolver's, and rho and v are
    non-zero inside the far end after the second"""
    N.run_steps(dims, 0, lib=cpu_host, errlib=cpu_host)


OWN_RULE = [("flow_stats", d) for d in N.NEEDLES] + [("sources", d) for d in N.NEEDLES] + \
           [("loads", d) for d in (N.LONG_X, N.LONG_Z)]                  # gpu_obstacle_loads refuses LONG_Y


@pytest.mark.parametrize("op,dims", OWN_RULE, ids=["%s-%s" % (o, N.ident(d)) for o, d in OWN_RULE])
def test_own_rule_operators_are_not_vacuous_on_needles(op, dims):
    """gpu_flow_stats, gpu_emit_sources and gpu_obstacle_loads: the references the GPU test compares against, computed here by
    the restatements alone with their non-vacuity asserted (inside needle_case's *_reference)"""
    c = N.inputs(dims, N.H_POW2)
    if op == "flow_stats":
        import diag_case as D
        N.flow_stats_reference(D.load_diag(), c)
    elif op == "sources":
        import source_case as SC
        N.sources_reference(SC.load_sources(), c)
    else:
        import loads_case as LC
        N.loads_reference(LC.load_loads(), c)


@pytest.mark.parametrize("case", N.RENDER_CASES, ids=lambda v: "view%d-light%d-%g" % v)
def test_render_cases_are_not_vacuous_on_the_tallest_grid(case):
    import render_case as RC
    N.render_reference(RC.load_render(), N.LONG_Z, N.H_POW2, *case)
