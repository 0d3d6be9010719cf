"""The map updates with caller promises (gpu_solve_backwardDMC_hint / gpu_solve_forward_hint, include/bimocq_gpu.h):
velocity look-ups at grid nodes as the mean of two values, identity-map corners computed instead of loaded.

Bars: value equality with the CPU oracle (fields.same) and RAW BIT equality with the plain entry points -- the closed
forms may differ from the trilinear chain in the sign of a zero sample only, and that sign cannot reach an output.

Grids: 32^3 with h = 1/32 (the smallest power-of-two grid with interior nodes on every block edge), 1024 x 12 x 10 with
h = 1/1024 (16 x-blocks per row, six interior planes), and 24 x 20 x 16 with h = 1/24, where the promises must be ignored.
"""
import functools

import numpy as np
import pytest

import fields as F
from oracle_lib import fp, lib as oracle

pytestmark = pytest.mark.gpu

P2_GRIDS = [(32, 32, 32, 1.0 / 32), (1024, 12, 10, 1.0 / 1024)]
GRIDS = P2_GRIDS + [(24, 20, 16, 1.0 / 24)]
FINITE, IDENTITY = 1, 2
FL_OPT_FAST_LERP = 11


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    lib.fl_nonfinite_seen(1)
    yield lib
    lib.fl_set_option(FL_OPT_FAST_LERP, 0)
    lib.fl_nonfinite_seen(1)
    bq.check()


def dev(*arrays):
    from gpufluidsimulation_amd import DeviceBuffer
    return [DeviceBuffer.from_numpy(a) for a in arrays]


def ptrs(bufs):
    return [b.ptr for b in bufs]


def bits(bufs):
    return [b.numpy().view(np.uint32) for b in bufs]


def pow2(h):
    return np.frexp(np.float32(h))[0] == 0.5


@functools.lru_cache(maxsize=None)
def carved_velocity(ni, nj, nk, h):
    """fields.velocity with exact zeros in one octant, negative zeros in the opposite one and the sign flipped in a slab
    across y: zero samples of both signs, and an upwind neighbour that differs from axis to axis"""
    out = []
    for a, (nx, ny, nz) in zip(F.velocity(ni, nj, nk, h), ((ni + 1, nj, nk), (ni, nj + 1, nk), (ni, nj, nk + 1))):
        a = a.reshape(nz, ny, nx).copy()
        a[:nz // 2, :ny // 2, :nx // 2] = 0.0
        a[nz // 2:, ny // 2:, nx // 2:] = -0.0
        a[:, ny // 2 - 3:ny // 2 + 2, :] *= np.float32(-1)
        a = np.ascontiguousarray(a.ravel())
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dmc_reference(ni, nj, nk, h, which, subscale):
    """(velocity, input maps, oracle output) of one DMC sub-step; which: 'warped' (carved velocity) or 'identity'"""
    hf = float(np.float32(h))
    if which == "warped":
        vel = carved_velocity(ni, nj, nk, hf)
        maps = F.warped_maps(ni, nj, nk, hf, -0.7, 1.1)
    else:
        vel = tuple(F.velocity(ni, nj, nk, hf))
        maps = F.identity_maps(ni, nj, nk, hf)
    ref = [a.copy() for a in maps]
    oracle().orc_solve_backwardDMC(*map(fp, vel), *map(fp, maps), *map(fp, ref), hf, ni, nj, nk, subscale * hf / 0.35)
    for a in list(maps) + ref:
        a.setflags(write=False)
    return vel, tuple(maps), tuple(ref)


def run_dmc(hip, vel, maps, h, ni, nj, nk, sub, hints):
    """one sub-step through the hinted (hints is not None) or the plain entry point; out starts as the input (border nodes)"""
    dv, di, do = dev(*vel), dev(*maps), dev(*maps)
    if hints is None:
        hip.gpu_solve_backwardDMC(*ptrs(dv), *ptrs(di), *ptrs(do), h, ni, nj, nk, sub)
    else:
        hip.gpu_solve_backwardDMC_hint(*ptrs(dv), *ptrs(di), *ptrs(do), h, ni, nj, nk, sub, hints)
    return do, (hip.fl_map_kernel_name(0) or b"").decode()


@pytest.mark.parametrize("ni,nj,nk,h", GRIDS)
def test_dmc_node_lookups(hip, ni, nj, nk, h):
    """finiteness promise alone, warped input maps, zeros of both signs in the velocity"""
    hf = float(np.float32(h))
    vel, maps, ref = dmc_reference(ni, nj, nk, h, "warped", 0.8)
    sub = 0.8 * hf / 0.35
    plain, name0 = run_dmc(hip, vel, maps, hf, ni, nj, nk, sub, None)
    hinted, name1 = run_dmc(hip, vel, maps, hf, ni, nj, nk, sub, FINITE)
    assert name0 == "dmc_kernel"
    assert name1 == ("dmc_node_kernel" if pow2(hf) else "dmc_kernel")
    for r, a, b in zip(ref, plain, hinted):
        assert F.same(r, a.numpy()) and F.same(r, b.numpy())
    for a, b in zip(bits(plain), bits(hinted)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("ni,nj,nk,h", GRIDS)
def test_dmc_identity_input(hip, ni, nj, nk, h):
    """both promises from the identity map: a CFL-sized sub-step, and one so large that departure points leave the plain
    interior near every wall (out-of-range cells, negative bases, row wraps): those waves read the real buffers"""
    hf = float(np.float32(h))
    outs = {}
    for subscale in (0.8, 6.5):
        vel, maps, ref = dmc_reference(ni, nj, nk, h, "identity", subscale)
        sub = subscale * hf / 0.35
        plain, _ = run_dmc(hip, vel, maps, hf, ni, nj, nk, sub, None)
        hinted, name = run_dmc(hip, vel, maps, hf, ni, nj, nk, sub, FINITE | IDENTITY)
        assert name == ("dmc_node_identity_kernel" if pow2(hf) else "dmc_kernel")
        for r, a, b in zip(ref, plain, hinted):
            assert F.same(r, a.numpy()) and F.same(r, b.numpy())
        for a, b in zip(bits(plain), bits(hinted)):
            assert np.array_equal(a, b)
        outs[subscale] = [b.numpy() for b in hinted]
    assert any(np.any(a != b) for a, b in zip(outs[0.8], outs[6.5]))


@functools.lru_cache(maxsize=None)
def forward_reference(ni, nj, nk, h, dtscale):
    hf = float(np.float32(h))
    vel = tuple(F.velocity(ni, nj, nk, hf))
    maps = F.identity_maps(ni, nj, nk, hf)
    ref = [a.copy() for a in maps]
    oracle().orc_solve_forward(*map(fp, vel), *map(fp, ref), hf, ni, nj, nk, 0.9 * hf / 0.35, dtscale * 2 * hf)
    return vel, tuple(maps), tuple(ref)


@pytest.mark.parametrize("ni,nj,nk,h", GRIDS)
@pytest.mark.parametrize("dtscale", [1.0, -1.0, 2.7])
def test_forward_identity_start(hip, ni, nj, nk, h, dtscale):
    hf = float(np.float32(h))
    vel, maps, ref = forward_reference(ni, nj, nk, h, dtscale)
    cfldt, dt = 0.9 * hf / 0.35, dtscale * 2 * hf
    dv, plain, hinted = dev(*vel), dev(*maps), dev(*maps)
    hip.gpu_solve_forward(*ptrs(dv), *ptrs(plain), hf, ni, nj, nk, cfldt, dt)
    assert hip.fl_map_kernel_name(1) == b"forward_kernel"
    hip.gpu_solve_forward_hint(*ptrs(dv), *ptrs(hinted), hf, ni, nj, nk, cfldt, dt, FINITE | IDENTITY)
    assert hip.fl_map_kernel_name(1) == (b"forward_identity_kernel" if pow2(hf) else b"forward_kernel")
    for r, a, b in zip(ref, plain, hinted):
        assert F.same(r, a.numpy()) and F.same(r, b.numpy())
    for a, b in zip(bits(plain), bits(hinted)):
        assert np.array_equal(a, b)
    # the identity promise without the finiteness one is of no use to the forward update
    hip.gpu_solve_forward_hint(*ptrs(dv), *ptrs(dev(*maps)), hf, ni, nj, nk, cfldt, dt, IDENTITY)
    assert hip.fl_map_kernel_name(1) == b"forward_kernel"


def test_fast_lerp_twin(hip):
    """FL_OPT_FAST_LERP = 1: the hinted kernels reproduce the fast build's own arithmetic"""
    ni = nj = nk = 32
    hf = 1.0 / 32
    hip.fl_set_option(FL_OPT_FAST_LERP, 1)
    try:
        vel, maps, _ = dmc_reference(ni, nj, nk, hf, "warped", 0.8)
        plain, _ = run_dmc(hip, vel, maps, hf, ni, nj, nk, 0.8 * hf / 0.35, None)
        hinted, name = run_dmc(hip, vel, maps, hf, ni, nj, nk, 0.8 * hf / 0.35, FINITE)
        assert name == "dmc_node_kernel"
        assert all(np.array_equal(a, b) for a, b in zip(bits(plain), bits(hinted)))
        for subscale in (0.8, 6.5):
            vel, maps, _ = dmc_reference(ni, nj, nk, hf, "identity", subscale)
            plain, _ = run_dmc(hip, vel, maps, hf, ni, nj, nk, subscale * hf / 0.35, None)
            hinted, name = run_dmc(hip, vel, maps, hf, ni, nj, nk, subscale * hf / 0.35, FINITE | IDENTITY)
            assert name == "dmc_node_identity_kernel"
            assert all(np.array_equal(a, b) for a, b in zip(bits(plain), bits(hinted)))
        for dtscale in (1.0, -1.0, 2.7):
            vel, maps, _ = forward_reference(ni, nj, nk, hf, dtscale)
            dv, plain, hinted = dev(*vel), dev(*maps), dev(*maps)
            hip.gpu_solve_forward(*ptrs(dv), *ptrs(plain), hf, ni, nj, nk, 0.9 * hf / 0.35, dtscale * 2 * hf)
            hip.gpu_solve_forward_hint(*ptrs(dv), *ptrs(hinted), hf, ni, nj, nk, 0.9 * hf / 0.35, dtscale * 2 * hf, FINITE | IDENTITY)
            assert hip.fl_map_kernel_name(1) == b"forward_identity_kernel"
            assert all(np.array_equal(a, b) for a, b in zip(bits(plain), bits(hinted)))
    finally:
        hip.fl_set_option(FL_OPT_FAST_LERP, 0)


def test_plane_window_ignores_the_promises(hip):
    """a launch restricted to a plane window runs the plain kernel whatever the caller promised"""
    ni = nj = nk = 32
    hf = 1.0 / 32
    vel, maps, ref = dmc_reference(ni, nj, nk, hf, "identity", 0.8)
    assert hip.fl_set_plane_window(4, 20) == 1
    try:
        _, name = run_dmc(hip, vel, maps, hf, ni, nj, nk, 0.8 * hf / 0.35, FINITE | IDENTITY)
    finally:
        hip.fl_set_plane_window(-1, -1)
    assert name == "dmc_kernel"


def test_nonfinite_velocity_keeps_the_plain_kernels(hip):
    """One NaN and one Inf in u: the plain entry point still equals the oracle (NaNs in the same places), and a solver
    that runs once the library's reduction has met them does not promise anything.  (The hinted call is not defined on
    such input and is not compared.)"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    ni = nj = nk = 32
    hf = 1.0 / 32
    vel = [a.copy() for a in F.velocity(ni, nj, nk, hf)]
    u = vel[0].reshape(nk, nj, ni + 1)
    u[9, 11, 13] = np.nan
    u[20, 17, 6] = np.inf
    maps = F.warped_maps(ni, nj, nk, hf, -0.7, 1.1)
    ref = [a.copy() for a in maps]
    oracle().orc_solve_backwardDMC(*map(fp, vel), *map(fp, maps), *map(fp, ref), hf, ni, nj, nk, 0.8 * hf / 0.35)
    plain, name = run_dmc(hip, vel, maps, hf, ni, nj, nk, 0.8 * hf / 0.35, None)
    assert name == "dmc_kernel"
    assert any(np.isnan(r).any() for r in ref)
    for r, a in zip(ref, plain):
        assert F.same(r, a.numpy())
    try:
        dv = dev(*vel)
        hip.gpu_max_abs3(*ptrs(dv), ni, nj, nk)
        assert hip.fl_nonfinite_seen(0) == 1
        hip.fl_map_kernels_seen(1)
        s = BimocqGPUSolver(ni, nj, nk, 1.0, 0.0, 1.0, device=0)
        s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)])
        s.setProjection(10, 0.5)
        assert s.getOption(14) == 1
        s.advance(0, 2.0 / ni)
        s.field("rho")
        assert hip.fl_map_kernel_name(0) == b"dmc_kernel" and hip.fl_map_kernel_name(1) == b"forward_kernel"
        assert hip.fl_map_kernels_seen(1) == (1 | 8)
        s.close()
    finally:
        hip.fl_nonfinite_seen(1)
