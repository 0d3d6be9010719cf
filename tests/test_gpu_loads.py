"""Per-obstacle pressure loads on the MI355X: gpu_obstacle_loads against the numpy terms of
tests/loads_case.py with the derived summation bound, on grids of one block, of several blocks along y and z-chunks and of two blocks along a
row, each with rows of a multiple of four cells (the kernel reads a lane's four flags as one word) and of another length (it
reads them byte by byte and the last lane is partly filled), and on flags at an address that is no multiple of four; the same bits with and without the rows summary, for float and double pressure, from call to call, and with NaN in every
pressure the contract says is not read; exact answers for linear pressure on a box; the refusals; and the host solver's
sampling on the real library."""
import ctypes as C

import numpy as np
import pytest

import loads_case as LC
import pose_case as P
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
# ni % 4 == 0: the word variant of the kernel; (21, ..), (70, ..), (262, ..): the byte variant, whose last lane holds 1 or 2 cells;
# ni > 256: two blocks along a row, the -x / +x neighbours of the cells 255 and 256 lie in another block's cells
GRIDS = [(20, 13, 11), (64, 12, 9), (72, 40, 37), (21, 13, 11), (70, 13, 11), (264, 8, 9), (262, 8, 9)]
SENTINEL = -7.0


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    return lib


@pytest.fixture(scope="module")
def dev(hip):
    d = Dev(hip)
    yield d
    d.free()


def bits(a):
    return np.ascontiguousarray(a, f64).view(np.uint64).tolist()


def gpu_loads(hip, dev, p, solid, rows, centres, n, h, dims=None, both=False, out_ptr=None, list_ptr=0, shift=0):
    """gpu_obstacle_loads on device copies: (rc, (16, 8)); the outputs start as SENTINEL; the flags start `shift` bytes into
    their allocation"""
    nk, nj, ni = solid.shape
    ni, nj, nk = dims or (ni, nj, nk)
    arr, _ = LC.centre_list(centres)
    p32 = dev.put("p32", p) if p is not None and p.dtype == f32 else None
    p64 = dev.put("p64", p) if p is not None and p.dtype == f64 else None
    if both:
        p64 = dev.put("p64", p.astype(f64))
    sp = dev.put("lsolid", np.concatenate([np.full(shift, 0xff, np.uint8), solid.ravel()])) + shift
    rp = None if rows is None else dev.put("lrows", rows)
    op = dev.put("lout", np.full((LC.NB, LC.NL), SENTINEL, f64))
    rc = hip.gpu_obstacle_loads(p32, p64, sp, rp, C.addressof(arr) if list_ptr == 0 else list_ptr, n, h, ni, nj, nk,
                                op if out_ptr is None else out_ptr)
    return rc, dev.get("lout")


def gpu_flags(hip, dev, dims, h, boundaries):
    ni, nj, nk = dims
    from gpufluidsimulation_amd.solver import boundary_array
    arr, n = boundary_array(boundaries)
    sp, rp = dev.put("fsolid", np.full(ni * nj * nk, 7, np.uint8)), dev.put("frows", np.zeros(nj * nk, np.uint8))
    hip.gpu_obstacle_flags(sp, rp, C.addressof(arr), n, h, ni, nj, nk)
    check(hip)
    return dev.get("fsolid").reshape(nk, nj, ni), dev.get("frows").reshape(nk, nj)


def case(hip, dev, dims, which):
    """(p, solid, rows, centres, n, h) of the cases (a) random flags, (b) the same with a list of 5, (c) a voxelised sphere, an
    overlapping box and a one-cell obstacle in the corner cell (0, 0, nk - 1), flags and rows from gpu_obstacle_flags itself"""
    ni, nj, nk = dims
    h = 1.0 / ni
    rng = np.random.default_rng(ni * 1000 + nk)
    p = rng.standard_normal((nk, nj, ni)).astype(f32)
    if which in "ab":
        solid = LC.random_flags(dims, ni + nj)
        rows = P.rows_summary((solid & 0x7f) != 0)
        return p, solid, rows, rng.random((16, 3)).astype(f32), (16 if which == "a" else 5), h
    X, Y, Z = ni * h, nj * h, nk * h
    m = min(Y, Z)
    blist = [(0, 0.4 * X, 0.5 * Y, 0.5 * Z, 0.3 * m, 0, 0, 0, 0, 0),
             (1, 0.55 * X, 0.55 * Y, 0.45 * Z, 0.2 * X, 0.15 * m, 0.25 * m, 0, 0, 0),
             (0, 0.0, 0.0, (nk - 1) * h, 0.3 * h, 0, 0, 0, 0, 0)]
    solid, rows = gpu_flags(hip, dev, dims, h, blist)
    assert solid[nk - 1, 0, 0] == 3 and (solid == 3).sum() == 1 and (solid == 1).any() and (solid == 2).any()
    assert not rows.all() or ni < 72
    return p, solid, rows, np.array([b[1:4] for b in blist], f32), 3, h


@pytest.mark.parametrize("which", ["a", "b", "c"])
@pytest.mark.parametrize("dims", GRIDS)
def test_operator_against_the_numpy_terms(hip, dev, dims, which):
    p, solid, rows, ctr, n, h = case(hip, dev, dims, which)
    owner, _, terms, F = LC.np_terms(p, solid, ctr, n, h)
    assert len(owner) > 0
    rc, got = gpu_loads(hip, dev, p, solid, rows, ctr, n, h)
    check(hip)
    assert rc == 0
    LC.assert_within_bound(got, owner, terms, n, f"{dims} {which}")
    # without the rows summary, with the double pressure, a second time: the same bits
    for name, kw in (("no rows", dict(p=p, rows=None)), ("p64", dict(p=p.astype(f64), rows=rows)), ("again", dict(p=p, rows=rows))):
        rc, other = gpu_loads(hip, dev, kw["p"], solid, kw["rows"], ctr, n, h)
        assert rc == 0 and bits(other) == bits(got), name
    # NaN in every cell that is not the F cell of a wetted face leaves no trace
    poisoned = np.full(p.size, np.nan, f32)
    poisoned[F] = p.ravel()[F]
    for r in (rows, None):
        rc, other = gpu_loads(hip, dev, poisoned.reshape(p.shape), solid, r, ctr, n, h)
        assert rc == 0 and bits(other) == bits(got)
    # and a NaN at an F cell propagates into that obstacle's sums
    poisoned = p.copy().ravel()
    poisoned[F[0]] = np.nan
    rc, other = gpu_loads(hip, dev, poisoned.reshape(p.shape), solid, rows, ctr, n, h)
    assert rc == 0 and np.isnan(other[owner[0], LC.PSUM])
    check(hip)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_flags_at_any_alignment(hip, dev, shift):
    """flags that do not start at a multiple of four bytes go through the byte variant: the same bits as the aligned ones"""
    dims = (20, 13, 11)
    p, solid, rows, ctr, n, h = case(hip, dev, dims, "a")
    rc, want = gpu_loads(hip, dev, p, solid, rows, ctr, n, h)
    assert rc == 0
    owner, _, terms, _ = LC.np_terms(p, solid, ctr, n, h)
    LC.assert_within_bound(want, owner, terms, n, f"{dims} aligned")
    for r in (rows, None):
        rc, got = gpu_loads(hip, dev, p, solid, r, ctr, n, h, shift=shift)
        assert rc == 0 and bits(got) == bits(want)
    check(hip)


# the last three: a box whose +x fluid neighbours are the row's last cell, alone in its lane; boxes across the cells 255 | 256
@pytest.mark.parametrize("dims,size,lo", [((20, 13, 11), (3, 4, 2), (5, 3, 4)), ((64, 12, 9), (1, 1, 1), (62, 10, 7)),
                                          ((72, 40, 37), (66, 9, 20), (3, 2, 5)), ((21, 13, 11), (3, 4, 2), (17, 3, 4)),
                                          ((264, 8, 9), (20, 3, 4), (240, 2, 2)), ((262, 8, 9), (12, 3, 4), (249, 2, 2))])
def test_linear_pressure_on_a_box_is_exact(hip, dev, dims, size, lo):
    coef = (3, -2, 5, 7)
    h = 0.125
    assert all(l > 0 and l + s < n for l, s, n in zip(lo, size, dims))         # fluid on every side of the box
    solid = LC.box_flags(dims, lo, size, owner=2)
    ctr = np.zeros((2, 3), f32)
    ctr[1] = [(lo[c] + 0.5 * (size[c] - 1)) * h for c in range(3)]
    rows = P.rows_summary(solid != 0)
    rc, out = gpu_loads(hip, dev, LC.linear_pressure(dims, coef), solid, rows, ctr, 2, h)
    want, faces = LC.linear_box_answer(size, coef)
    assert rc == 0 and out[1, :3].tolist() == [float(x) for x in want] and out[1, LC.FACES] == faces
    assert not out[0].any() and not out[2:].any()
    rc, out = gpu_loads(hip, dev, LC.linear_pressure(dims, (0, 0, 0, 3)), solid, None, ctr, 2, h)
    assert rc == 0 and out[1, :6].tolist() == [0.0] * 6 and out[1, LC.PSUM] == 3 * faces and out[1, LC.FACES] == faces
    check(hip)


def test_refusals_leave_the_outputs_alone(hip, dev):
    dims = (20, 13, 11)
    ni, nj, nk = dims
    solid = LC.box_flags(dims, (5, 3, 4), (3, 4, 2))
    p = LC.linear_pressure(dims, (1, 0, 0, 0))
    ctr = np.zeros((1, 3), f32)
    bad, _ = LC.centre_list(np.full((1, 3), np.inf))
    pp = dev.put("p32", p)
    cases = [dict(both=True), dict(p=None), dict(n=-1), dict(n=17), dict(list_ptr=None), dict(list_ptr=C.addressof(bad)),
             dict(h=0.0), dict(h=float("nan")), dict(dims=(2, nj, nk)), dict(dims=(ni, nj, 2)), dict(out_ptr=pp)]
    for kw in cases:
        args = dict(p=p, n=1, h=0.1)
        args.update(kw)
        rc, out = gpu_loads(hip, dev, args.pop("p"), solid, None, ctr, args.pop("n"), args.pop("h"), **args)
        assert rc == 3 and hip.fl_last_error() == 3, kw
        hip.fl_clear_error()
        assert (out == SENTINEL).all(), kw
    assert np.array_equal(dev.get("p32"), p)
    arr, _ = LC.centre_list(ctr)
    op = dev.put("lout", np.full((LC.NB, LC.NL), SENTINEL, f64))
    for null_solid, null_out in ((True, False), (False, True)):
        rc = hip.gpu_obstacle_loads(pp, None, None if null_solid else dev.put("lsolid", solid), None, C.addressof(arr), 1, 0.1, ni, nj, nk,
                                    None if null_out else op)
        assert rc == 3
        hip.fl_clear_error()
    assert (dev.get("lout") == SENTINEL).all()
    # a z-slab context is unsupported
    hip.fl_set_slab(0, 2 * nk, 0, nk, nk)
    try:
        rc, out = gpu_loads(hip, dev, p, solid, None, ctr, 1, 0.1)
        assert rc == 4 and hip.fl_last_error() == 4 and (out == SENTINEL).all()
    finally:
        hip.fl_clear_error()
        hip.fl_set_slab(0, 0, 0, 0, 0)
    rc, out = gpu_loads(hip, dev, p, solid, None, ctr, 1, 0.1)
    assert rc == 0 and out[0, LC.FACES] == 52


def test_an_empty_list_writes_128_zeros(hip, dev):
    dims = (20, 13, 11)
    solid = LC.random_flags(dims, 3)
    p = np.full(solid.shape, np.nan, f32)
    rc, out = gpu_loads(hip, dev, p, solid, None, np.zeros((1, 3), f32), 0, 0.1, list_ptr=None)
    check(hip)
    assert rc == 0 and not out.any() and np.isfinite(out).all()


# ---- the host solver on the real library -------------------------------------------------------------------------------
SOLVER_DIMS = (32, 24, 20)


# the last case: rows of 30 cells, the byte variant of the kernel behind the solver's own flags and rows summary
@pytest.mark.parametrize("dims,scheme,kind,walls", [(SOLVER_DIMS, 0, "jacobi", 0), (SOLVER_DIMS, 0, "pcg", 0), (SOLVER_DIMS, 2, "pcg", 55),
                                                    (SOLVER_DIMS, 2, "jacobi", 0), (SOLVER_DIMS, 3, "jacobi", 0), (SOLVER_DIMS, 3, "pcg", 0),
                                                    ((30, 24, 20), 0, "jacobi", 0)])
def test_solver_rows(dims, scheme, kind, walls):
    """3 steps with a moving sphere and a spinning oriented box: fields bit-identical with the option on and off; the row is the
    formula on the raw slots; the slot of the step's last projection lies within the derived bound of the numpy terms on the
    downloaded final pressure, mask and centres"""
    from gpufluidsimulation_amd import solver
    assert walls in (0, solver.WALLS_REFERENCE_BOX)
    s0, off, _, _ = LC.run_scene(None, None, dims, scheme, kind, 0, walls=walls)
    s0.close()
    s, on, halfrdx, dt = LC.run_scene(None, None, dims, scheme, kind, 1, walls=walls)
    try:
        LC.assert_fields_equal(on, off)
        row, raw = LC.assert_row_is_formula(s, halfrdx, dt)
        assert row["step"] == 3 and [r["step"] for r in s.obstacleLoadsHistory()] == [1, 2, 3]
        flags, ctr = LC.owner_flags(s, walls), LC.solver_centres(s)
        owner, _, terms, _ = LC.np_terms(LC.final_pressure(s, on[-1], kind), flags, ctr, 2, s.h)
        last = 1 if scheme == 3 else 0
        LC.assert_within_bound(raw["slots"][last], owner, terms, 2, f"{dims} scheme {scheme} {kind} walls {walls}")
        assert raw["weights"] == ((2.0, 1.0) if scheme == 3 else (1.0, 0.0))
        if scheme == 3:
            first = raw["slots"][0]
            assert np.isfinite(first).all() and first[:2, :6].any() and (first[:2, LC.FACES] == raw["slots"][1][:2, LC.FACES]).all()
            assert bits(first) != bits(raw["slots"][1])
        else:
            assert not raw["slots"][1].any()
        assert np.isfinite(row["force"]).all() and row["force"].any() and row["torque"].any() and (row["area"] > 0).all()
    finally:
        s.close()


def test_a_spinning_box_is_resisted():
    LC.check_spinning_box_resists(None, None)


def test_an_impulsively_started_sphere_feels_its_added_mass():
    LC.check_added_mass(None, None)
