"""The projection's default launch sequence: four Jacobi sweeps per launch (jacobi_lds_kernel<.., 4>) wherever
FL_OPT_JACOBI_ROWS = 0 (auto) admits them -- whole unmasked arrays, rows of 32 .. 256 floats, chunks of at least 24 planes,
not a z-slab rank -- and the launch sequence from before on every other grid and with FL_OPT_JACOBI_ROWS = 7.

gpu_jacobi_sweeps fuses sweeps only on the caller's word that both ping-pong buffers carry the same boundary layer
(FL_OPT_JACOBI_FUSE = 2; the solver's projection sets it after clearing both), so "default options" here means that word
given and every tuning option (rows, chunk lengths, block shape, variant) at 0.  The reference is the same library with
FL_OPT_JACOBI_FUSE = 0: one sweep per launch.  Equality is on the raw bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALPHA, BETA = -1.0, float(np.float32(1.0 / 6.0))
QUAD_GRID = (64, 256, 192)          # rows of 64 floats: 32 row blocks -> 8 chunks of 24 planes fill the 256 CUs once
QUAD, TRIPLE = "jacobi_lds_kernel<4 sweeps>", "jacobi_lds3_kernel"
SWEEPS = (3, 4, 7, 198, 199)


def dev(*arrays):
    from gpufluidsimulation_amd import DeviceBuffer
    return [DeviceBuffer.from_numpy(a) for a in arrays]


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    L = bq._lib
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0, lib.fl_last_error_string()
    tuning = (L.FL_OPT_JACOBI_VARIANT, L.FL_OPT_JACOBI_ROWS, L.FL_OPT_JACOBI_KCHUNK, L.FL_OPT_JACOBI_KCHUNK2)
    for o in tuning:
        lib.fl_set_option(o, 0)
    yield lib
    for o in tuning:
        lib.fl_set_option(o, 0)
    lib.fl_set_option(L.FL_OPT_JACOBI_FUSE, 1)
    bq.check()


def seeded(ni, nj, nk, seed):
    rng = np.random.default_rng(seed)
    n = ni * nj * nk
    return rng.standard_normal(n, dtype=np.float32), (0.2 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(hip, p0, div, dims, sweeps, fuse, rows=0):
    """`sweeps` sweeps from p0 (both buffers start as p0: the same boundary layer); returns (newest iterate, kernel name).
    The newest iterate sits where gpu_jacobi_sweeps says: one buffer change per LAUNCH, so with fused launches of two or
    four sweeps that is not the parity of `sweeps` (one sweep per launch: it is)."""
    import gpufluidsimulation_amd as bq
    L = bq._lib
    ni, nj, nk = dims
    dp, dd, dt = dev(p0, div, p0)
    hip.fl_set_option(L.FL_OPT_JACOBI_FUSE, fuse)
    hip.fl_set_option(L.FL_OPT_JACOBI_ROWS, rows)
    try:
        where = hip.gpu_jacobi_sweeps(dp.ptr, dd.ptr, dt.ptr, ni, nj, nk, sweeps, ALPHA, BETA)
        name = (hip.fl_jacobi_kernel_name() or b"").decode()
    finally:
        hip.fl_set_option(L.FL_OPT_JACOBI_FUSE, 1)
        hip.fl_set_option(L.FL_OPT_JACOBI_ROWS, 0)
    assert where in (0, 1) and (fuse != 0 or where == sweeps % 2), (where, sweeps, fuse)
    out = (dt if where else dp).numpy()
    bq.check()
    return out, name


@pytest.fixture(scope="module")
def single_sweeps(hip):
    """the iterates after each count in SWEEPS, one sweep per launch, on QUAD_GRID"""
    p0, div = seeded(*QUAD_GRID, 20261017)
    return p0, div, {s: run(hip, p0, div, QUAD_GRID, s, fuse=0)[0] for s in SWEEPS}


@pytest.mark.parametrize("sweeps", SWEEPS)
def test_default_sequence_equals_single_sweeps(hip, single_sweeps, sweeps):
    p0, div, ref = single_sweeps
    got, name = run(hip, p0, div, QUAD_GRID, sweeps, fuse=2)
    assert np.array_equal(bits(got), bits(ref[sweeps])), sweeps
    assert name == (TRIPLE if sweeps == 3 else QUAD), (sweeps, name)


def test_kernel_name_is_the_most_launched_kernel(hip, single_sweeps):
    """199 sweeps: 49 launches of four + 1 of three where quads apply; today's kernels at 128^3 (chunks of 8 planes: 99 launches
    of the short-march two-sweep kernel) and on rows of 320 floats (the two-segment three-sweep kernel)"""
    p0, div, _ = single_sweeps
    assert run(hip, p0, div, QUAD_GRID, 199, fuse=2)[1] == QUAD
    for dims, want in (((128, 128, 128), "jacobi_lean2r_kernel"), ((320, 256, 192), "jacobi_lds2seg_kernel")):
        q0, d0 = seeded(*dims, 7)
        got, name = run(hip, q0, d0, dims, 199, fuse=2)
        assert name == want, (dims, name)
        before, name7 = run(hip, q0, d0, dims, 199, fuse=2, rows=7)
        assert name7 == want, (dims, name7)
        assert np.array_equal(bits(got), bits(before)), dims


@pytest.mark.parametrize("sweeps", SWEEPS)
def test_rows_7_is_the_sequence_without_quads(hip, single_sweeps, sweeps):
    p0, div, ref = single_sweeps
    got, name = run(hip, p0, div, QUAD_GRID, sweeps, fuse=2, rows=7)
    assert name == TRIPLE, (sweeps, name)
    assert np.array_equal(bits(got), bits(ref[sweeps])), sweeps
