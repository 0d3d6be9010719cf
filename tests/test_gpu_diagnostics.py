"""Flow diagnostics on the GPU: gpu_flow_stats -- the marching kernel at its own and at forced chunk
lengths, the one-thread-per-cell kernel, all four instances of each -- against the C restatement (tests/cpu_abi/
flow_stats_abi.c), and the host solver's diagnostics, history ring, vorticity and dumps on the HIP library.

vort_mag and the two maxima must equal the restatement bit for bit.  The sums are sums of bit-identical terms in another
order, so each must lie within n 2^-53 sum|term| of math.fsum(terms) (tests/diag_case.py: the bound for a summation in
any order, derived, not tuned)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import diag_case as D
import fields as F
import obstacle_case as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FL_OPT_DIAG_KCHUNK = 22
BAD_ARGUMENT = 3
# the minimum; one partial x-block; an x seam at 64 with a ragged y block; a spacing that makes / q a real division; wide rows
SHAPES = [(8, 8, 8, 1.0 / 8), (24, 20, 16, 1.0 / 24), (72, 68, 66, 1.0 / 64), (130, 24, 20, 0.002), (1024, 12, 10, 1.0 / 1024)]
KCHUNKS = (0, 3, 11, -1)
INSTANCES = [(True, True), (True, False), (False, True), (False, False)]       # (writes vort_mag, has scalars)


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    yield lib
    lib.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
    bq.check()


@pytest.fixture(scope="module")
def cpu():
    return D.load_diag()


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs and the restatement's exact answers for a shape, computed once and frozen"""
    ni, nj, nk, h = shape
    h = float(f32(h))
    cpu = D.load_diag()
    u, v, w = F.velocity(ni, nj, nk, h)
    rho, T = F.scalar(ni, nj, nk, 0.7), F.scalar(ni, nj, nk, 2.1, amp=0.6)
    val, mass, n, mag = D.exact(cpu, u, v, w, rho, T, h, (ni, nj, nk))
    for a in (u, v, w, rho, T, mag):
        a.setflags(write=False)
    return h, (u, v, w, rho, T), val, mass, n, mag


def call(hip, dev, h, dims, vort, rho="rho", T="T"):
    dev.put("out", np.full(10, -1.0))
    if vort:
        dev.put("vort", np.full(int(np.prod(dims)), 7.0, f32))         # every cell must be written
    rc = hip.gpu_flow_stats(dev["u"], dev["v"], dev["w"], dev[rho] if rho else None, dev[T] if T else None,
                            dev["vort"] if vort else None, h, *dims, dev["out"])
    OC.check(hip)
    assert rc == 0
    return dict(zip(D.STAT, dev.get("out"))), (dev.get("vort") if vort else None)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_operator_equals_the_restatement(hip, shape):
    """every chunk option and kernel instance: vort_mag and the maxima bit for bit -- hence equal between the options --,
    every sum within the summation bound of the exact sum, two calls the same bits, absent scalars 0"""
    h, arrays, val, mass, n, mag = case(shape)
    dims = shape[:3]
    bound = D.raw_bound(mass, n)
    dev = OC.Dev(hip)
    try:
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            dev.put(name, a)
        assert val["vort_max"] > 0 and val["div_max"] > 0 and val["m2"] > 0
        for kc in KCHUNKS:
            hip.fl_set_option(FL_OPT_DIAG_KCHUNK, kc)
            assert hip.fl_get_option(FL_OPT_DIAG_KCHUNK) == kc
            for vort, scal in INSTANCES:
                got, field = call(hip, dev, h, dims, vort, "rho" if scal else None, "T" if scal else None)
                again, field2 = call(hip, dev, h, dims, vort, "rho" if scal else None, "T" if scal else None)
                for s in D.SUMS:
                    want = val[s] if (scal or s in ("e2", "m2", "d2")) else 0.0
                    err = abs(got[s] - want)
                    print(f"{dims} kchunk {kc} vort {vort} scalars {scal} {s}: {got[s]!r} exact {want!r} |diff| {err:.3e} bound {bound[s]:.3e}")
                for s in D.SUMS:
                    if scal or s in ("e2", "m2", "d2"):
                        assert abs(got[s] - val[s]) <= bound[s], (kc, vort, scal, s, got[s], val[s], bound[s])
                    else:
                        assert got[s] == 0.0, (kc, vort, scal, s, got[s])
                assert bits([got["div_max"], got["vort_max"]]) == bits([val["div_max"], val["vort_max"]]), (kc, vort, scal, got)
                assert bits(list(got.values())) == bits(list(again.values())), (kc, vort, scal, "repeat call")
                if vort:
                    assert np.array_equal(field.view(np.uint32), mag.view(np.uint32)), (kc, scal, F.maxdiff(field, mag))
                    assert np.array_equal(field.view(np.uint32), field2.view(np.uint32))
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            assert np.array_equal(dev.get(name).view(np.uint32), a.view(np.uint32)), name
    finally:
        hip.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
        dev.free()


def test_many_partial_rows_are_folded(hip):
    """8 x 260 x 66 leaves 4290 partial rows with one plane per block (above the 4096 that go straight into the final pass):
    the folding launch in front of it keeps the bound, the maxima and the repeatability"""
    shape = (8, 260, 66, 1.0 / 8)
    h, arrays, val, mass, n, mag = case(shape)
    dims = shape[:3]
    bound = D.raw_bound(mass, n)
    dev = OC.Dev(hip)
    try:
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            dev.put(name, a)
        for kc in (-1, 1):
            hip.fl_set_option(FL_OPT_DIAG_KCHUNK, kc)
            got, field = call(hip, dev, h, dims, True)
            again, _ = call(hip, dev, h, dims, True)
            for s in D.SUMS:
                print(f"{dims} kchunk {kc} {s}: {got[s]!r} exact {val[s]!r} |diff| {abs(got[s] - val[s]):.3e} bound {bound[s]:.3e}")
                assert abs(got[s] - val[s]) <= bound[s], (kc, s, got[s], val[s], bound[s])
            assert bits([got["div_max"], got["vort_max"]]) == bits([val["div_max"], val["vort_max"]])
            assert bits(list(got.values())) == bits(list(again.values()))
            assert np.array_equal(field.view(np.uint32), mag.view(np.uint32))
    finally:
        hip.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
        dev.free()


def test_density_and_temperature_are_optional_one_by_one(hip):
    h, arrays, val, mass, n, _ = case(SHAPES[1])
    dims = SHAPES[1][:3]
    bound = D.raw_bound(mass, n)
    dev = OC.Dev(hip)
    try:
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            dev.put(name, a)
        for kc in (0, -1):
            hip.fl_set_option(FL_OPT_DIAG_KCHUNK, kc)
            got, _ = call(hip, dev, h, dims, False, "rho", None)
            assert got["T"] == 0.0 and abs(got["rho_j"] - val["rho_j"]) <= bound["rho_j"] and abs(got["rho"] - val["rho"]) <= bound["rho"]
            got, _ = call(hip, dev, h, dims, False, None, "T")
            assert [got[s] for s in ("rho", "rho_i", "rho_j", "rho_k")] == [0.0] * 4 and abs(got["T"] - val["T"]) <= bound["T"]
    finally:
        hip.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
        dev.free()


def test_a_nan_in_the_velocity_reaches_the_sums_and_latches_nothing(hip, cpu):
    """sums propagate non-finite values, maxima skip NaNs as fmaxf does -- exactly as the restatement"""
    shape = SHAPES[1]
    h, arrays, *_ = case(shape)
    dims = shape[:3]
    ni, nj, nk = dims
    u = arrays[0].copy()
    u[(ni + 1) * (nj * 7 + 9) + 11] = np.nan
    want = np.zeros(10)
    mag = np.zeros(ni * nj * nk, f32)
    assert cpu.gpu_flow_stats(u.ctypes.data, arrays[1].ctypes.data, arrays[2].ctypes.data, None, None, mag.ctypes.data, h, *dims,
                              want.ctypes.data) == 0
    want = dict(zip(D.STAT, want))
    dev = OC.Dev(hip)
    try:
        for name, a in zip(("u", "v", "w"), (u,) + arrays[1:3]):
            dev.put(name, a)
        for kc in KCHUNKS:
            hip.fl_set_option(FL_OPT_DIAG_KCHUNK, kc)
            got, field = call(hip, dev, h, dims, True, None, None)
            assert math.isnan(got["e2"]) and math.isnan(got["m2"]) and math.isnan(got["d2"])
            assert bits([got["div_max"], got["vort_max"]]) == bits([want["div_max"], want["vort_max"]]) and got["vort_max"] > 0
            assert F.same(field, mag) and np.isnan(field).any()         # (value equality: NaN payloads are no part of the contract)
        assert hip.fl_last_error() == 0
    finally:
        hip.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
        dev.free()


def test_refusals_launch_nothing(hip):
    """NULL velocity or d_out, a dimension below 3, vort_mag aliasing an input: FL_ERR_BAD_ARGUMENT, d_out and vort_mag untouched"""
    shape = SHAPES[1]
    h, arrays, *_ = case(shape)
    dims = shape[:3]
    dev = OC.Dev(hip)
    try:
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            dev.put(name, a)
        dev.put("out", np.full(10, -1.0))
        dev.put("vort", np.full(int(np.prod(dims)), 7.0, f32))
        u, v, w, rho, T, out, vort = (dev[k] for k in ("u", "v", "w", "rho", "T", "out", "vort"))
        bad = [(None, v, w, rho, T, vort, h, *dims, out), (u, None, w, rho, T, vort, h, *dims, out), (u, v, None, rho, T, vort, h, *dims, out),
               (u, v, w, rho, T, vort, h, *dims, None), (u, v, w, rho, T, vort, h, 2, dims[1], dims[2], out),
               (u, v, w, rho, T, vort, h, dims[0], 2, dims[2], out), (u, v, w, rho, T, vort, h, dims[0], dims[1], 2, out),
               (u, v, w, rho, T, rho, h, *dims, out), (u, v, w, rho, T, T, h, *dims, out), (u, v, w, rho, T, u, h, *dims, out),
               (u, v, w, rho, T, w, h, *dims, out)]
        for kc in (0, -1):
            hip.fl_set_option(FL_OPT_DIAG_KCHUNK, kc)
            for args in bad:
                assert hip.gpu_flow_stats(*args) == BAD_ARGUMENT
                assert hip.fl_last_error() == BAD_ARGUMENT
                hip.fl_clear_error()
        assert (dev.get("out") == -1.0).all() and (dev.get("vort") == 7.0).all()
        for name, a in zip(("u", "v", "w", "rho", "T"), arrays):
            assert np.array_equal(dev.get(name).view(np.uint32), a.view(np.uint32)), name
    finally:
        hip.fl_set_option(FL_OPT_DIAG_KCHUNK, 0)
        dev.free()


def test_survey_recorded_trajectory(hip):
    """the 32^3 scene of SURVEY 8(c) (tests/test_oracle_kat.py: 8 steps of dt = 2h, 50 sweeps, halfrdx 0.5) read through
    diagnostics(): sum(rho) 134.00 -> 136.20, rho-centroid y 0.1985 -> 0.2439 -- recorded from the reference"""
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    N = 32
    s = BimocqGPUSolver(N, N, N, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)])
    s.setProjection(50, 0.5)
    rows = []
    for f in range(8):
        s.advance(f, 2.0 / N)
        rows.append(s.diagnostics())
    s._check()
    s.close()
    first, last = rows[0], rows[-1]
    print(first, last)
    assert round(first["rho_sum"], 2) == 134.00 and round(last["rho_sum"], 2) == 136.20
    assert round(first["centroid_y"], 4) == 0.1985 and round(last["centroid_y"], 4) == 0.2439
    assert [r["step"] for r in rows] == list(range(1, 9)) and last["kinetic"] > first["kinetic"] > 0 and last["enstrophy"] > 0


@pytest.mark.parametrize("scheme", (0, 2, 3))
def test_history_ring_equals_the_blocking_calls(hip, cpu, scheme):
    """option 1 over 5 steps: five rows, each bit for bit what diagnostics() returned after that step; the last one within
    the summation bound of the exact sums over the downloaded fields; vorticity() equals the restatement's field"""
    from gpufluidsimulation_amd import solver
    dims, L = (40, 24, 20), 1.0
    out, taken, hist, vort = D.run_with_diagnostics(solver.host_lib(), hip, dims, L, 5, 20, 1.0 / dims[0], scheme=scheme, every=1,
                                                    sample={1, 2, 3, 4, 5})
    assert hist.shape == (5, solver.DIAG_COUNT) and hist[:, -1].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    for r in range(5):
        assert bits(hist[r]) == bits([taken[r + 1][k] for k in solver.DIAG_NAMES]), (r, hist[r], taken[r + 1])
    h = float(f32(L) / f32(dims[0]))
    last = out[-1]
    val, mass, n, mag = D.exact(cpu, last["u"], last["v"], last["w"], last["rho"], last["T"], h, dims)
    row, bound = D.diag_row(val, h, 5), D.row_bound(val, mass, n, h)
    for name in solver.DIAG_NAMES:
        print(f"scheme {scheme} {name}: {taken[5][name]!r} exact {row[name]!r} bound {bound[name]:.3e}")
        assert abs(taken[5][name] - row[name]) <= bound[name], (name, taken[5][name], row[name], bound[name])
    assert row["kinetic"] > 0 and row["enstrophy"] > 0 and row["rho_sum"] > 1
    assert np.array_equal(vort.ravel().view(np.uint32), mag.view(np.uint32))


def test_vorticity_dump_on_the_gpu(hip, tmp_path):
    from gpufluidsimulation_amd import solver
    dims = (40, 24, 20)
    s = solver.BimocqGPUSolver(*dims, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.05, 1.0, [(0.5, 0.3, 0.33, 0.15, 1.0, 2.0, 1.0, 1000)])
    s.setProjection(20, 0.5)
    for f in range(3):
        s.advance(f, 1.0 / dims[0])
    n = s.outputVorticity(2, str(tmp_path), 0.05)
    vort = s.vorticity()
    s._check()
    s.close()
    hd, rec = solver.read_density_dump(str(tmp_path / "vorticity_render_0003.bqd"))
    keep = vort.astype(np.float64) > float(f32(0.05))
    assert hd["grid_name"] == b"vorticity" and n == len(rec) == keep.sum() > 0
    back = np.zeros_like(vort)
    back[rec["k"], rec["j"], rec["i"]] = rec["value"]
    assert np.array_equal(back, np.where(keep, vort, 0))


def test_two_slab_ranks_on_the_gpu(tmp_path):
    """two z-slab ranks (processes) of 24 x 20 x 32 sharing the GPU over the stream-ordered stand-in for librccl, so that the
    all-reduce of the sums runs inside the compute stream: diagnostics within the bound of the exact single-domain sums on
    every rank, history rows, stitched vorticity bit-equal (tests/diag_slab_worker.py)"""
    import sys
    import diag_slab_worker as W
    from build_fake_rccl import build
    from test_diagnostics_cpu import free_port
    ref = str(tmp_path / "ref.npz")
    W.reference("gpu", ref)
    env = dict(os.environ, OMP_NUM_THREADS="4", MASTER_ADDR="127.0.0.1", BQ_RCCL_LIBRARY=build("async"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "diag_slab_worker.py"), "--backend", "gpu",
           "--transport", "rccl", "--reference", ref]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    lines = "\n".join(l for l in r.stdout.splitlines() if l.startswith("[rank")) or r.stdout[-3000:]
    assert r.returncode == 0, lines
    assert lines.count("mismatches=0") == 2


def test_example_driver_with_diagnostics(tmp_path):
    """build/bimocq3d with diag_every = 2: exits 0, prints one line per sampled frame, writes the vorticity files next to
    the density dumps"""
    from gpufluidsimulation_amd.solver import read_density_dump
    exe = os.path.join(ROOT, "build", "bimocq3d")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "example"], cwd=ROOT)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "48", "4", out, "0", "0", "1", "0", "0", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout
    assert "[diag step 2]" in r.stdout and "[diag step 4]" in r.stdout and "[diag step 3]" not in r.stdout and "last dump ok" in r.stdout
    files = sorted(os.listdir(out))
    assert files == [f"density_render_{i:04d}.bqd" for i in range(1, 5)] + ["vorticity_render_0002.bqd", "vorticity_render_0004.bqd"], files
    hd, rec = read_density_dump(os.path.join(out, files[-1]))
    assert hd["grid_name"] == b"vorticity" and hd["nx"] == 48 and hd["count"] == len(rec) > 50
