"""The pool backend of tests/align_case.py on a machine without a GPU, against the CPU stand-ins of the C-ABI (tests/cpu_abi):

* the placement itself: every array where its mode says, never below element alignment, at least 64 sentinel bytes on either
  side, arrays that do not overlap, the one-at-a-time modes;
* the guard check: a write one element before or past an array fails check() and the read-back, and a stand-in whose call is
  wrapped (in Python, here only) to write one element before its output fails the very case the GPU test runs;
* the non-vacuity conditions of tests/test_gpu_alignment.py at its shapes, on the oracle alone;
* the cases themselves through the pool on the stand-in: argument order, dtypes, the start of every output.

The stand-ins call the oracle, so nothing here says anything about a kernel; it says that a failure of the GPU file is the
library's."""
import ctypes as C

import numpy as np
import pytest

import align_case as A
import fields as F
import host_entry_case as H
import needle_case as N
from build_cpu_host import build as build_cpu_host

STAND_IN = [n for n in N.CASES if not n.endswith("_hint") and not n.startswith("maccormack")]      # (as tests/test_needle_grids_cpu.py)


@pytest.fixture(scope="module")
def be():
    lib = H.bind(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL))
    lib.orc_set_fast_lerp.restype, lib.orc_set_fast_lerp.argtypes = None, [C.c_int]
    backend = A.PoolBackend(lib, lib.orc_set_fast_lerp, "cpu stand-in, pooled")
    yield backend
    backend.mode = A.CONTROL
    backend.lib.orc_set_fast_lerp(0)
    backend.check()


ALL_MODES = A.MODES + A.FLAGS_ONLY + A.FLOATS_ONLY + A.one_at_a_time(4)


# ---- the placement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES, ids=repr)
def test_pool_places_every_array_where_the_mode_says(be, mode):
    be.mode = mode
    rng = np.random.default_rng(5)
    arrays = [rng.random(37, dtype=np.float32), rng.random(40), rng.integers(0, 255, 41, dtype=np.uint8),
              rng.random(4, dtype=np.float32), rng.integers(0, 9, 5, dtype=np.int32), rng.integers(0, 255, 3, dtype=np.uint8)]
    bufs = be.dev(*arrays)
    pool = bufs[0].pool
    spans = sorted((b.ptr, b.ptr + b.nbytes) for b in bufs)
    assert spans[0][0] - pool.base >= A.GUARD and pool.base + pool.size - spans[-1][1] >= A.GUARD
    assert all(b0 - a1 >= 2 * A.GUARD for (_, a1), (b0, _) in zip(spans, spans[1:]))          # a band of each array's own in between
    for k, (b, a) in enumerate(zip(bufs, arrays)):
        size = a.dtype.itemsize
        assert b.ptr % size == 0 and (b.ptr % 16) == mode.offset(k, a.dtype) * size
        assert b.numpy().dtype == a.dtype and np.array_equal(b.numpy(), a)
    if mode.aligned:
        assert all(b.ptr % 16 == 0 for b in bufs)
    elif mode.rotate:
        assert [b.ptr % 16 for b in bufs] == [4, 0, 3, 0, 4, 2]                              # neighbours differ
    elif mode.only is not None:
        assert [k for k, b in enumerate(bufs) if b.ptr % 16] == [mode.only]
    if mode in A.FLAGS_ONLY:
        assert all((b.ptr % 16 != 0) == (a.dtype == np.uint8) for b, a in zip(bufs, arrays))
    if mode in A.FLOATS_ONLY:
        assert all((b.ptr % 16 != 0) == (a.dtype.itemsize == 4) for b, a in zip(bufs, arrays))
    be.check()


def test_modes_cover_what_the_contract_names():
    assert [m.f for m in A.SAME] == [1, 2, 3] and [m.b for m in A.SAME] == [1, 2, 3] and 1 in [m.d for m in A.SAME]
    assert A.CONTROL.aligned and not any(m.aligned for m in ALL_MODES[1:])
    for m in ALL_MODES:
        for k in range(6):
            assert 0 <= m.offset(k, np.float32) < 4 and 0 <= m.offset(k, np.float64) < 2 and 0 <= m.offset(k, np.uint8) < 16
    assert sorted((m.only, m.f) for m in A.one_at_a_time(3)) == [(k, o) for k in range(3) for o in (1, 2, 3)]
    assert all(m.d == 1 for m in A.one_at_a_time(3))


# ---- the guard check -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [A.CONTROL, A.SAME[0], A.ROTATING], ids=repr)
@pytest.mark.parametrize("where", ["one before", "one past", "63 bytes before", "64 bytes past the end"])
def test_a_write_outside_an_array_is_caught(be, mode, where):
    be.mode = mode
    a, b = np.arange(50, dtype=np.float32), np.arange(9, dtype=np.float64)
    bufs = be.dev(a, b)
    be.check()
    target = bufs[1]
    at = {"one before": target.ptr - 8, "one past": target.ptr + target.nbytes, "63 bytes before": target.ptr - 63,
          "64 bytes past the end": target.ptr + target.nbytes + 63}[where]
    old = (C.c_ubyte * 1)()
    be.lib.fl_memcpy_d2h(old, at, 1)
    bad = (C.c_ubyte * 1)(old[0] ^ 1)                      # one bit of one byte
    be.lib.fl_memcpy_h2d(at, bad, 1)
    with pytest.raises(AssertionError, match="written outside an array"):
        be.check()
    with pytest.raises(AssertionError, match="written outside an array"):
        bufs[0].numpy()                                    # any read-back of the pool sees it
    be.lib.fl_memcpy_h2d(at, old, 1)
    be.check()
    assert np.array_equal(bufs[0].numpy(), a) and np.array_equal(bufs[1].numpy(), b)


class WritesBefore:
    """the stand-in with ONE entry point broken on purpose: after the real call, element -1 of its argument `arg` is overwritten
    with the element's own neighbour (a vector store that rounds its address down does this).  Python, the stand-in only."""

    def __init__(self, lib, fn, arg, size=4):
        self._lib, self._fn, self._arg, self._size = lib, fn, arg, size

    def __getattr__(self, name):
        real = getattr(self._lib, name)
        if name != self._fn:
            return real

        def broken(*args):
            ret = real(*args)
            self._lib.fl_memcpy_d2d(args[self._arg] - self._size, args[self._arg], self._size)
            return ret
        return broken


@pytest.mark.parametrize("mode", [A.CONTROL, A.SAME[2]], ids=repr)
def test_a_broken_stand_in_call_fails_its_case(be, mode):
    """gpu_divergence writing one float before `div`, gpu_jacobi_sweeps one before p_temp: the values of every array are still
    the oracle's, only the guard check can tell"""
    broken = A.PoolBackend(WritesBefore(be.lib, "gpu_divergence", 3), be.fast_lerp, "broken", mode)
    r = N.Runner(broken, A.ROW32, N.H_POW2)
    with pytest.raises(AssertionError, match="written outside an array"):
        A.run_case(r, "divergence")
    A.run_case(r, "gradient")                              # the entry points left alone still pass on the same backend
    broken = A.PoolBackend(WritesBefore(be.lib, "gpu_jacobi_sweeps", 2), be.fast_lerp, "broken", mode)
    with pytest.raises(AssertionError, match="written outside an array"):
        A.run_abi(be.lib, broken, "gpu_jacobi_sweeps", A.sweeps_args(A.ROW32, 4))
    be.mode = mode
    A.run_abi(be.lib, be, "gpu_jacobi_sweeps", A.sweeps_args(A.ROW32, 4))


def test_wrong_values_fail_run_abi(be):
    """run_abi compares every array: a backend that sweeps twice less (the newest iterate in the same buffer) fails it"""
    class TwoSweepsLess(WritesBefore):
        def __getattr__(self, name):
            real = getattr(self._lib, name)
            if name != "gpu_jacobi_sweeps":
                return real
            return lambda p, d, t, ni, nj, nk, s, a, b: real(p, d, t, ni, nj, nk, s - 2, a, b)
    wrong = A.PoolBackend(TwoSweepsLess(be.lib, "", 0), be.fast_lerp, "wrong", A.CONTROL)
    with pytest.raises(AssertionError, match="differing"):
        A.run_abi(be.lib, wrong, "gpu_jacobi_sweeps", A.sweeps_args(A.ROW32, 4))


# ---- non-vacuity of the GPU file's cases, on the oracle alone ------------------------------------------------------------------
@pytest.mark.parametrize("dims", A.SHAPES, ids=N.ident)
def test_needle_cases_are_not_vacuous_at_these_shapes(dims):
    """every case of needle_case.CASES moves at least 16 elements of every judged output (asserted inside align_case.reference);
    both spacings: the maps are displaced by multiples of h"""
    for h in A.SPACINGS:
        c = N.inputs(dims, h)
        for name in N.CASES:
            A.reference(c, name)


@pytest.mark.parametrize("dims", A.SHAPES, ids=N.ident)
def test_projection_arguments_are_not_vacuous(be, dims):
    """the argument lists of the projection entry points (align_case.*_args) on the stand-in through an aligned pool: run_abi
    asserts that the reference moves at least 16 elements"""
    be.mode = A.CONTROL
    for fn, args, judged in A.projection_calls(dims):
        A.run_abi(be.lib, be, fn, args, judged, N.ident(dims))


# ---- the cases through the pool on the stand-in --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.MODES, ids=repr)
@pytest.mark.parametrize("dims", [A.ROW32, A.ROW33, A.GENERIC], ids=N.ident)
def test_needle_cases_through_the_pool(be, dims, mode):
    be.mode = mode
    r = N.Runner(be, dims, N.H_TABLED)
    for name in STAND_IN:
        A.run_case(r, name, 0)
    for name in ("advect_velocity", "solve_forward", "clamp_extrema_u"):
        A.run_case(r, name, 1)
    r.free()


@pytest.mark.parametrize("mode", A.one_at_a_time(3), ids=repr)
def test_sweeps_one_argument_at_a_time(be, mode):
    be.mode = mode
    for fn, args, judged in A.projection_calls(A.ROW32):
        A.run_abi(be.lib, be, fn, args, judged, mode)


@pytest.fixture(scope="module")
def wide():
    """(library, pool backend) of the stand-in with the obstacle, wall, PCG, source, flow-statistics and load restatements"""
    from build_cpu_loads import build_loads
    lib = H.bind(C.CDLL(build_loads(), mode=C.RTLD_LOCAL))
    lib.orc_set_fast_lerp.restype, lib.orc_set_fast_lerp.argtypes = None, [C.c_int]
    return lib, A.PoolBackend(lib, lib.orc_set_fast_lerp, "wide cpu stand-in, pooled")


@pytest.mark.parametrize("dims", A.SHAPES, ids=N.ident)
def test_argument_lists_of_the_other_families(wide, dims):
    """the sparse-field gathers, the vector updates, and the obstacle and wall operators with their scene: every argument list is
    accepted by the restatement and moves at least 16 elements (AbiCase), and runs through a rotating pool"""
    lib, pooled = wide
    pooled.mode = A.ROTATING
    for fn, args, judged in A.sparse_calls(dims) + A.vector_calls(dims):
        A.run_abi(lib, pooled, fn, args, judged, N.ident(dims))
    calls, keep = A.masked_calls(lib, dims)
    for fn, args, judged, form in calls:
        A.run_abi(lib, pooled, fn, args, judged, N.ident(dims))
    calls, keep = A.posed_calls(lib, dims)                 # the _ls and _pose variants: phi grids from a pool of their own
    for mode in (A.ROTATING, A.FLAGS_ONLY[0], A.FLOATS_ONLY[2]):
        pooled.mode = mode
        for fn, args, judged in calls:
            A.run_abi(lib, pooled, fn, args, judged, N.ident(dims))
    pooled.check()


@pytest.mark.parametrize("mode", [A.CONTROL] + A.FLAGS_ONLY + A.FLOATS_ONLY, ids=repr)
def test_masked_sweeps_with_flags_or_floats_off_their_boundary(wide, mode):
    lib, pooled = wide
    pooled.mode = mode
    calls, keep = A.masked_calls(lib, A.ROW32)
    for fn, args, judged, form in calls:
        got, bufs = A.run_abi(lib, pooled, fn, args, judged, mode)
        flags = [b for b in bufs if b.dtype == np.uint8]
        floats = [b for b in bufs if b.dtype == np.float32]
        assert all((b.ptr % 4 != 0) == (mode in A.FLAGS_ONLY) for b in flags) and all((b.ptr % 16 != 0) == (mode in A.FLOATS_ONLY) for b in floats)


@pytest.mark.parametrize("mode", [A.CONTROL, A.SAME[0], A.ROTATING], ids=repr)
def test_host_entry_cases_through_the_pool(be, mode):
    """the cases of tests/host_entry_case.py that the GPU file runs on pool arrays"""
    be.mode = mode
    H.run_residual_norms(be, 65, 7, 9)
    H.run_gradient_delta(be, 65, 6, 5)
    H.run_diffuse_sweeps(be, 25, 20, 16)
    H.run_clamp_box_w(be, 33, 6, 6)
    for one in A.one_at_a_time(2, (1,)):                   # `before` alone off its boundary, then `after` alone
        be.mode = one
        H.run_clamp_box_w(be, 32, 6, 6)
    be.mode = mode
    H.run_max_abs3(be, 5, 5, 5, 1.0 / 8)
    for name in ("corners", "overlap", "65 boxes"):
        H.run_box_lists(be, 5, name)
