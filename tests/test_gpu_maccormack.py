"""gpu_maccormack and the MacCormack scheme (scheme 2) on the GPU: the HIP kernel against the
literal composition of its definition on the CPU oracle and against the library's own separate launches, the host solver
on the HIP library against the same host solver on the CPU stand-in.  Value for value (fields.same)."""
import os
import subprocess

import numpy as np
import pytest

import fields as F
import maccormack_case as MC
import obstacle_case as OC
from oracle_lib import fp, lib as oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FL_OPT_FAST_LERP = 11
BAD_ARGUMENT = 3
# rows crossing a 64-wide block, a power-of-two and three other spacings (0.002 and 0.01: the tabled look-ups' spacings)
SHAPES = [(24, 20, 16, 1.0 / 24), (72, 68, 66, 1.0 / 64), (130, 24, 20, 0.002), (40, 36, 30, 0.01)]
STAGGERS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
DT_CELLS = (1.7, 2.6)


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    yield lib
    lib.fl_set_option(FL_OPT_FAST_LERP, 0)
    oracle().orc_set_fast_lerp(0)
    bq.check()


def inputs(ni, nj, nk, h, stag, dt_cells):
    """velocity, cfldt, dt, the advected field, the first pass + a perturbation, another limiter field (oracle mode as set)"""
    o = oracle()
    dx, dy, dz = stag
    bi, bj, bk = ni + dx, nj + dy, nk + dz
    h = float(f32(h))
    vel = F.velocity(ni, nj, nk, h)
    cfldt = float(f32(h) / f32(o.orc_max_abs3(*map(fp, vel), ni, nj, nk)))
    dt = float(f32(dt_cells * cfldt))
    field = F.scalar(bi, bj, bk, 0.7)
    f1 = np.zeros_like(field)
    o.orc_semilag(fp(f1), fp(field), *map(fp, vel), dx, dy, dz, h, ni, nj, nk, cfldt, -dt)
    f1 = np.ascontiguousarray(f1 + F.scalar(bi, bj, bk, 2.3, amp=0.6))
    other = F.scalar(bi, bj, bk, 1.1, amp=0.8)
    return h, vel, cfldt, dt, field, f1, other


def compose(f1, f_adv, f_lim, vel, stag, h, dims, cfldt, dt, dtc):
    """the definition of gpu_maccormack on the oracle: (out, how many values the limiter changed)"""
    o = oracle()
    ni, nj, nk = dims
    dx, dy, dz = stag
    back = np.zeros_like(f1)
    o.orc_semilag(fp(back), fp(f1), *map(fp, vel), dx, dy, dz, h, ni, nj, nk, cfldt, dt)
    out = f1.copy()
    o.orc_add(fp(out), fp(back), -0.5, out.size)
    o.orc_add(fp(out), fp(f_adv), 0.5, out.size)
    before = out.copy()
    o.orc_clamp_extrema(fp(f_lim), fp(out), *map(fp, vel), ni + dx, nj + dy, nk + dz, dx, dy, dz, 0.5 * dx, 0.5 * dy, 0.5 * dz, h, dtc)
    return out, int(np.count_nonzero(before.view(np.uint32) != out.view(np.uint32)))


def fused(hip, d, stag, h, dims, cfldt, dt, dtc, lim="f_lim"):
    dx, dy, dz = stag
    hip.gpu_maccormack(d["out"], d["f1"], d["f_adv"], d[lim], d["u"], d["v"], d["w"], dx, dy, dz, h, *dims, cfldt, dt, dtc)


def unfused(hip, d, stag, h, dims, cfldt, dt, dtc, n, lim="f_lim"):
    """the separate launches of the library, result in d["tmp"]"""
    ni, nj, nk = dims
    dx, dy, dz = stag
    hip.fl_memset(d["back"], 0, 4 * n)
    hip.gpu_semilag(d["back"], d["f1"], d["u"], d["v"], d["w"], dx, dy, dz, h, ni, nj, nk, cfldt, dt)
    hip.fl_memcpy_d2d(d["tmp"], d["f1"], 4 * n)
    hip.gpu_add(d["tmp"], d["back"], -0.5, n)
    hip.gpu_add(d["tmp"], d["f_adv"], 0.5, n)
    hip.gpu_clamp_extrema(d[lim], d["tmp"], d["u"], d["v"], d["w"], ni + dx, nj + dy, nk + dz, dx, dy, dz,
                          0.5 * dx, 0.5 * dy, 0.5 * dz, h, dtc)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("ni,nj,nk,h", SHAPES)
def test_operator_equals_its_definition(hip, ni, nj, nk, h, fast):
    """every stagger, dt of 1.7 and 2.6 cells (two and three trace sub-steps), f_lim = f_adv and another field: the
    oracle composition, the library's separate launches, the inputs left alone, both limiter branches taken"""
    dev = OC.Dev(hip)
    hip.fl_set_option(FL_OPT_FAST_LERP, fast)
    oracle().orc_set_fast_lerp(fast)
    try:
        for stag in STAGGERS:
            for dt_cells in DT_CELLS:
                hh, vel, cfldt, dt, field, f1, other = inputs(ni, nj, nk, h, stag, dt_cells)
                n = field.size
                host = {"u": vel[0], "v": vel[1], "w": vel[2], "f1": f1, "f_adv": field, "f_lim": other}
                for name, a in host.items():
                    dev.put(name, a)
                for name in ("out", "back", "tmp"):
                    dev.put(name, np.full(n, 7.0, f32))                 # the operator must write every node
                for lim in ("f_adv", "f_lim"):
                    want, changed = compose(f1, field, host[lim], vel, stag, hh, (ni, nj, nk), cfldt, dt, dt)
                    print(f"{ni}x{nj}x{nk} stagger {stag} dt {dt_cells} cells, limiter field {lim}, fast {fast}: limiter changed {changed} of {n}")
                    assert 0 < changed < n, (stag, dt_cells, lim, changed, n)
                    fused(hip, dev, stag, hh, (ni, nj, nk), cfldt, dt, dt, lim)
                    unfused(hip, dev, stag, hh, (ni, nj, nk), cfldt, dt, dt, n, lim)
                    OC.check(hip)
                    got = dev.get("out")
                    assert F.same(want, got), (stag, dt_cells, lim, F.maxdiff(want, got), int((want != got).sum()))
                    assert F.same(dev.get("tmp"), got), (stag, dt_cells, lim, "separate launches")
                for name, a in host.items():
                    assert np.array_equal(dev.get(name).view(np.uint32), a.view(np.uint32)), (stag, dt_cells, name)
    finally:
        hip.fl_set_option(FL_OPT_FAST_LERP, 0)
        oracle().orc_set_fast_lerp(0)
        dev.free()


def plant(a, shape, values, seed):
    """`values` at a handful of nodes of the flat array `a` of (bk, bj, bi) = shape: corners, faces, inside"""
    bk, bj, bi = shape
    nodes = [(0, 0, 0), (bk - 1, bj - 1, bi - 1), (0, bj // 2, bi // 2), (bk // 2, 0, 3), (bk // 2, bj - 1, bi - 2), (2, 2, 0),
             (bk // 2, bj // 2, bi // 2), (bk // 2 + 1, bj // 3, bi // 3), (3, bj - 3, bi - 4), (bk - 2, 4, bi // 2 + 1)]
    a = a.copy().reshape(shape)
    for q, (k, j, i) in enumerate(nodes):
        a[k, j, i] = values[(q + seed) % len(values)]
    return np.ascontiguousarray(a.ravel())


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("ni,nj,nk,h", [SHAPES[0], SHAPES[3]])
def test_operator_with_non_finite_values(hip, ni, nj, nk, h, fast):
    """NaN and +-Inf in f1, f_adv and f_lim (values that are sampled, never turned into an address), border nodes
    included; the velocity stays finite"""
    dev = OC.Dev(hip)
    hip.fl_set_option(FL_OPT_FAST_LERP, fast)
    oracle().orc_set_fast_lerp(fast)
    bad = [f32(np.nan), f32(np.inf), f32(-np.inf)]
    try:
        for stag in STAGGERS:
            hh, vel, cfldt, dt, field, f1, other = inputs(ni, nj, nk, h, stag, 1.7)
            shape = (nk + stag[2], nj + stag[1], ni + stag[0])
            f1, field, other = plant(f1, shape, bad, 0), plant(field, shape, bad, 1), plant(other, shape, bad, 2)
            with np.errstate(invalid="ignore"):
                want, _ = compose(f1, field, other, vel, stag, hh, (ni, nj, nk), cfldt, dt, dt)
            assert np.isnan(want).any() and np.isfinite(want).any()
            for name, a in {"u": vel[0], "v": vel[1], "w": vel[2], "f1": f1, "f_adv": field, "f_lim": other,
                            "out": np.full(field.size, 7.0, f32)}.items():
                dev.put(name, a)
            fused(hip, dev, stag, hh, (ni, nj, nk), cfldt, dt, dt)
            OC.check(hip)
            got = dev.get("out")
            assert F.same(want, got), (stag, int((np.isnan(want) != np.isnan(got)).sum()), int((want != got).sum()))
    finally:
        hip.fl_set_option(FL_OPT_FAST_LERP, 0)
        oracle().orc_set_fast_lerp(0)
        dev.free()


def test_operator_refusals(hip):
    """`out` aliasing any input, a bad stagger triple and cfldt <= 0 with dt != 0 latch FL_ERR_BAD_ARGUMENT and launch nothing"""
    ni, nj, nk, h = 24, 20, 16, float(f32(1.0 / 24))
    dev = OC.Dev(hip)
    u, v, w = F.velocity(ni, nj, nk, h)
    big = max(u.size, v.size, w.size)
    for name, a in {"u": u, "v": v, "w": w, "f1": F.scalar(ni, nj, nk, 0.1), "f_adv": F.scalar(ni, nj, nk, 0.7),
                    "f_lim": F.scalar(ni, nj, nk, 1.1), "out": np.full(big, 7.0, f32)}.items():
        dev.put(name, a)
    d = {k: dev[k] for k in dev.bufs}
    base = dict(out=d["out"], f1=d["f1"], f_adv=d["f_adv"], f_lim=d["f_lim"], u=d["u"], v=d["v"], w=d["w"],
                stag=(0, 0, 0), cfldt=0.1, dt=0.05)
    cases = [dict(out=d[k]) for k in ("f1", "f_adv", "f_lim", "u", "v", "w")]
    cases += [dict(stag=(1, 1, 0)), dict(stag=(2, -1, 0)), dict(stag=(0, 0, 2)), dict(stag=(-1, 1, 1)), dict(cfldt=0.0), dict(cfldt=-1.0)]
    try:
        for case in cases:
            a = dict(base, **case)
            before = {k: dev.get(k) for k in dev.bufs}
            hip.gpu_maccormack(a["out"], a["f1"], a["f_adv"], a["f_lim"], a["u"], a["v"], a["w"], *a["stag"], h, ni, nj, nk,
                               a["cfldt"], a["dt"], a["dt"])
            assert hip.fl_last_error() == BAD_ARGUMENT, case
            hip.fl_clear_error()
            for k in dev.bufs:
                assert np.array_equal(before[k].view(np.uint32), dev.get(k).view(np.uint32)), (case, k)
        # dt == 0 needs no cfldt: the trace does not move
        hip.gpu_maccormack(d["out"], d["f1"], d["f_adv"], d["f_lim"], d["u"], d["v"], d["w"], 0, 0, 0, h, ni, nj, nk, 0.0, 0.0, 0.0)
        OC.check(hip)
    finally:
        hip.fl_clear_error()
        dev.free()


# ---- the scheme --------------------------------------------------------------------------------------------------------
SOLVER_CASES = [((32, 32, 32), 1.0), ((40, 36, 30), 0.4)]          # h = 1/32 and h = 0.01
STEPS, ITERS = 8, 16


@pytest.fixture(scope="module")
def standin():
    lib = MC.load_maccormack()
    lib.orc_set_fast_lerp.restype, lib.orc_set_fast_lerp.argtypes = None, [MC.C.c_int]
    yield lib
    lib.orc_set_fast_lerp(0)


def same_steps(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        for n in MC.NAMES:
            assert F.same(a[n], b[n]), (what, f, n, F.maxdiff(a[n], b[n]))


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("dims,L", SOLVER_CASES)
def test_scheme_2_equals_the_host_solver_on_the_standin(hip, standin, dims, L, fast):
    """8 steps of 4 cells each (the traces take several sub-steps by the end), 16 Jacobi iterations, exact and one-fma
    arithmetic: fused and unfused give the stand-in's fields after every step"""
    from gpufluidsimulation_amd import solver
    dt = 4.0 * L / dims[0]
    standin.orc_set_fast_lerp(fast)
    hip.fl_set_option(FL_OPT_FAST_LERP, fast)
    try:
        want, cfl = MC.run(standin, standin, dims, L, STEPS, ITERS, dt, scheme=2)
        assert f32(dt) / f32(cfl[-1]) > 1.0, cfl
        assert all(np.isfinite(want[-1][n]).all() for n in MC.NAMES) and np.abs(want[-1]["u"]).max() > 0.01
        for option in (1, 0):
            got, got_cfl = MC.run(solver.host_lib(), hip, dims, L, STEPS, ITERS, dt, scheme=solver.SCHEME_MACCORMACK, fused=option)
            assert got_cfl == cfl, option
            same_steps(got, want, f"option {option}, fast {fast}")
    finally:
        standin.orc_set_fast_lerp(0)
        hip.fl_set_option(FL_OPT_FAST_LERP, 0)


def test_scheme_2_with_an_obstacle_and_a_box_source(hip, standin):
    from gpufluidsimulation_amd import solver
    n = 32
    obstacles, sources = MC.obstacle_scene(n)
    want, _ = MC.run(standin, standin, (n, n, n), 1.0, 4, ITERS, 2.0 / n, scheme=2, obstacles=obstacles, sources=sources)
    assert want[-1]["rho"].max() > 0.5 and np.abs(want[-1]["w"]).max() > 0.01
    obstacles, sources = MC.obstacle_scene(n)
    got, _ = MC.run(solver.host_lib(), hip, (n, n, n), 1.0, 4, ITERS, 2.0 / n, scheme=2, obstacles=obstacles, sources=sources)
    same_steps(got, want, "obstacle + source")


def test_reflection_fused_equals_unfused(hip):
    from gpufluidsimulation_amd import solver
    n = 32
    runs = {o: MC.run(solver.host_lib(), hip, (n, n, n), 1.0, 3, ITERS, 4.0 / n, scheme=3, fused=o, viscosity=1e-3)[0] for o in (0, 2)}
    same_steps(runs[2], runs[0], "reflection, option 2")
    assert np.abs(runs[0][-1]["v"]).max() > 0.01


@pytest.mark.parametrize("fused_option", (1, 0))
def test_two_ranks_sharing_the_gpu(tmp_path, hip, fused_option):
    """scheme 2 on two z-slab ranks (processes) of 24 x 20 x 32 sharing the GPU: the stitched owned planes equal the
    one-GPU run after each of 3 steps"""
    import maccormack_slab_worker as W
    from test_maccormack_cpu import launch_slabs
    ref = str(tmp_path / "ref.npz")
    W.reference("gpu", fused_option, ref)
    rc, out = launch_slabs("gpu", fused_option, ref, threads=4)
    assert rc == 0, out
    assert out.count("mismatches=0") == 2


def test_example_driver_runs_scheme_2(tmp_path):
    from gpufluidsimulation_amd.solver import read_density_dump
    exe = os.path.join(ROOT, "build", "bimocq3d")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "example"], cwd=ROOT)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "48", "4", out, "2", "0", "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    assert "Frame 3 Starts !!!" in r.stdout and "[Bimocq GPU Time:" in r.stdout and "last dump ok" in r.stdout
    files = sorted(os.listdir(out))
    assert files == [f"density_render_{i:04d}.bqd" for i in range(1, 5)], files
    hd, rec = read_density_dump(os.path.join(out, files[-1]))
    assert hd["nx"] == 48 and hd["count"] == len(rec) and len(rec) > 50
    assert np.all(rec["value"] > 1e-4)
    r = subprocess.run([exe, "48", "1", out, "1"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 2 and "2 MacCormack" in r.stdout            # SEMILAG stays refused, the usage text lists scheme 2
