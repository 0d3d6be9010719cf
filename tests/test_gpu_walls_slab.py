"""Closed domain walls on z-slab ranks on the MI355X.

  - the walled sweeps on plane ranges under fl_set_slab, in one process: every rank's window of a grid cut into 2 and 3 slabs
    with G = 6 and 8 against the same planes of 1 and 3 whole-array walled sweeps on the one domain, bit for bit over the
    planes the depth rule calls correct; everything else untouched (ghost planes outside the grid stay zero); what the call
    returns and the kernel it names say which kernel ran; a poisoned solidw proves that no flag is loaded;
  - gpu_wall_flags, gpu_wall_faces and gpu_gradient_masked_walls under the context against the window of the one-domain result;
  - two and three ranks sharing the GPU against the one-GPU walled run, every scheme;
  - two ranks of examples/bimocq3d_ranks.cpp in the container."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fields as F
import obstacle_ref as R
import walls_case as WC
import walls_slab_case as WS
from obstacle_case import Dev, check
from test_gpu_obstacle_edges import FUSED, REFUSED, options

pytestmark = pytest.mark.gpu
ROOT = WS.ROOT


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    lib.fl_set_slab.restype, lib.fl_set_slab.argtypes = None, [C.c_int] * 5
    yield lib
    lib.fl_set_slab(0, 0, 0, 0, 0)


def windows(nkg):
    """(koff, nk, own0, own1, G) of every rank of 2 and 3 slabs with 6 and 8 ghost planes"""
    out = []
    for nranks in (2, 3):
        for G in (6, 8):
            for r in range(nranks):
                own0, own1 = r * nkg // nranks, (r + 1) * nkg // nranks
                out.append((own0 - G, own1 - own0 + 2 * G, own0, own1, G))
    return out


def window(full, koff, nk, extra=0):
    """the rank's array of a one-domain field: its planes inside the grid, zeros outside"""
    nkg = full.shape[0] - extra
    lo, hi = max(koff, 0), min(koff + nk, nkg)
    out = np.zeros((nk + extra,) + full.shape[1:], full.dtype)
    out[lo - koff: hi - koff + extra] = full[lo: hi + extra]
    return out


def triple_applies(ni, nj, nk):
    """the shapes the walled three-sweep kernel takes (bq_jacobi_plan.h: plan_lds, masked): float4 rows of one wave, at least
    8 rows and 12 planes"""
    return ni % 4 == 0 and 32 <= ni <= 256 and nj >= 8 and nk >= 12


@pytest.mark.parametrize("dims", FUSED + REFUSED)
def test_range_sweeps_under_the_slab_context(hip, dims):
    ni, nj, nkg = dims
    beta = R.beta32()
    dev = Dev(hip)
    rng = np.random.default_rng(21)
    try:
        with options(hip, JACOBI_FUSE=2):
            for walls in (WC.REFERENCE_BOX, 62):
                solidw = WC.wall_flags(np.zeros((nkg, nj, ni), np.uint8), walls)
                p = R.initial_p(solidw, 3)
                div = rng.standard_normal(p.shape).astype(np.float32)
                # one domain, the existing operator: 1 and 3 whole-array walled sweeps
                hip.fl_set_slab(0, 0, 0, 0, 0)
                rows1 = dev.put("rows1", np.zeros((nkg, nj), np.uint8))
                bufs = [dev.put("a", p), dev.put("b", p)]
                d1, s1 = dev.put("div1", div), dev.put("solidw1", solidw)
                level = []
                for n in range(3):
                    hip.gpu_jacobi_sweep_masked_walls(bufs[n % 2], d1, bufs[(n + 1) % 2], s1, rows1, walls, ni, nj, nkg, R.ALPHA, beta)
                    level.append(dev.get("b" if n % 2 == 0 else "a"))
                check(hip)
                assert not np.array_equal(level[0], p) and not np.array_equal(level[2], level[0])
                for koff, nk, own0, own1, G in windows(nkg):
                    where = (dims, walls, koff, nk)
                    hip.fl_set_slab(koff, nkg, own0, own1, nk)
                    wp, wd = window(p, koff, nk), window(div, koff, nk)
                    want = [window(level[0], koff, nk), None, window(level[2], koff, nk)]
                    inside = np.array([0 <= k + koff < nkg for k in range(nk)])
                    sw = np.full((nk, nj, ni), 0xFF, np.uint8)          # poisoned: a clean `rows` must keep every flag unread
                    pin, pdiv = dev.put("win", wp), dev.put("wdiv", wd)
                    psw, prow = dev.put("wsolid", sw), dev.put("wrows", np.zeros((nk, nj), np.uint8))
                    # the planes a sweep of S levels gets right: everything its stencil needs lies in the window or outside the grid
                    def correct(S):
                        lo = 0 if koff <= 0 else S
                        hi = nk if koff + nk >= nkg else nk - S
                        return lo, hi
                    a, b = nk // 3, nk - nk // 3
                    ranges = {"whole": (0, nk, 0, 0), "ends": (0, a, b, nk), "interior": (a, b, 0, 0), "two planes": (a, a + 2, 0, 0),
                              "beyond the array": (-3, a, b, nk + 5)}
                    for name, (k0a, k1a, k0b, k1b) in ranges.items():
                        sel = np.zeros(nk, bool)
                        sel[max(k0a, 0):max(k1a, 0)] = True
                        sel[max(k0b, 0):max(k1b, 0)] = True
                        # ---- one sweep per launch (two calls for two ranges)
                        pout = dev.put("wout", wp)
                        for k0, k1 in ((k0a, k1a), (k0b, k1b)):
                            if k1 > k0:
                                assert hip.gpu_jacobi_sweep_masked_walls_range(pin, pdiv, pout, psw, prow, walls, ni, nj, nk, k0, k1, R.ALPHA, beta) == 1
                        check(hip)
                        got = dev.get("wout")
                        lo, hi = correct(1)
                        ok = sel & inside
                        ok[:lo] = False; ok[hi:] = False
                        assert np.array_equal(got[ok], want[0][ok]), (where, name, "single")
                        assert np.array_equal(got[~sel], wp[~sel]), (where, name, "single: planes outside the range")
                        assert not got[~inside].any()
                        # ---- three sweeps in one launch
                        pout = dev.put("wout", wp)
                        ran = hip.gpu_jacobi_sweep_masked_walls_triple_ranges(pin, pdiv, pout, psw, prow, walls, ni, nj, nk,
                                                                              k0a, k1a, k0b, k1b, R.ALPHA, beta)
                        check(hip)
                        got = dev.get("wout")
                        assert ran == (1 if triple_applies(ni, nj, nk) else 0), (where, name, ran)
                        if not ran:
                            assert np.array_equal(got, wp), (where, name, "a refused launch wrote")
                            continue
                        assert hip.fl_jacobi_kernel_name() == b"jacobi_lds3_walls_kernel"
                        lo, hi = correct(3)
                        ok = sel & inside
                        ok[:lo] = False; ok[hi:] = False
                        assert np.array_equal(got[ok], want[2][ok]), (where, name, "triple")
                        assert np.array_equal(got[~sel], wp[~sel]), (where, name, "triple: planes outside the ranges")
                        assert not got[~inside].any()
                    # the true flags give the same floats (one range suffices: the flags are not read either way)
                    psw = dev.put("wsolid", window(solidw, koff, nk))
                    pout = dev.put("wout", wp)
                    assert hip.gpu_jacobi_sweep_masked_walls_range(pin, pdiv, pout, psw, prow, walls, ni, nj, nk, 0, nk, R.ALPHA, beta) == 1
                    got = dev.get("wout")
                    lo, hi = correct(1)
                    ok = inside.copy()
                    ok[:lo] = False; ok[hi:] = False
                    assert np.array_equal(got[ok], want[0][ok]), (where, "true flags")
                    # ... and the whole-array operators under the context are the range operators on [0, nk)
                    pout2 = dev.put("wout2", wp)
                    hip.gpu_jacobi_sweep_masked_walls(pin, pdiv, pout2, psw, prow, walls, ni, nj, nk, R.ALPHA, beta)
                    check(hip)
                    assert np.array_equal(dev.get("wout2"), got), (where, "whole-array single under the context")
            # refusals launch nothing and say so
            hip.fl_set_slab(0, 0, 0, 0, 0)
            pin, pout = dev.put("a", p), dev.put("b", p)
            for bad in (0, 63, 64, -1):
                assert hip.gpu_jacobi_sweep_masked_walls_range(pin, d1, pout, s1, rows1, bad, ni, nj, nkg, 0, nkg, R.ALPHA, beta) == 0
                assert hip.fl_last_error() != 0
                hip.fl_clear_error()
                assert hip.gpu_jacobi_sweep_masked_walls_triple_ranges(pin, d1, pout, s1, rows1, bad, ni, nj, nkg, 0, nkg, 0, 0, R.ALPHA, beta) == 0
                assert hip.fl_last_error() != 0
                hip.fl_clear_error()
            assert np.array_equal(dev.get("b"), p)
        with options(hip, JACOBI_FUSE=0):                                # the triple is switched off: 0, nothing launched, no error
            assert hip.gpu_jacobi_sweep_masked_walls_triple_ranges(pin, d1, pout, s1, rows1, 55, ni, nj, nkg, 0, nkg, 0, 0, R.ALPHA, beta) == 0
            check(hip)
            assert np.array_equal(dev.get("b"), p)
    finally:
        hip.fl_set_slab(0, 0, 0, 0, 0)
        dev.free()


@pytest.mark.parametrize("dims", [(36, 13, 13), (99, 21, 18)])
def test_flags_faces_and_gradient_under_the_slab_context(hip, dims):
    ni, nj, nkg = dims
    shapes = ((nkg, nj, ni + 1), (nkg, nj + 1, ni), (nkg + 1, nj, ni))
    vel = [x.reshape(s) + np.float32(0.25) for x, s in zip(F.velocity(ni, nj, nkg, 1.0 / ni), shapes)]
    p = F.scalar(ni, nj, nkg, 0.7).reshape(nkg, nj, ni).copy()
    dev = Dev(hip)
    try:
        for walls in WC.MASKS:
            # one domain
            hip.fl_set_slab(0, 0, 0, 0, 0)
            ps = dev.put("solidw1", np.full((nkg, nj, ni), 7, np.uint8))
            hip.gpu_wall_flags(ps, None, walls, ni, nj, nkg)
            solidw = dev.get("solidw1")
            assert np.array_equal(solidw, WC.wall_flags(np.zeros_like(solidw), walls))
            ref = {}
            for with_d in (True, False):
                ptrs = [dev.put(nm + "1", x) for nm, x in zip("uvw", vel)]
                dptrs = [dev.put("d" + nm + "1", np.full_like(x, 9.0)) for nm, x in zip("uvw", vel)] if with_d else [None] * 3
                hip.gpu_wall_faces(*ptrs, *dptrs, ps, ni, nj, nkg)
                faced = [dev.get(nm + "1") for nm in "uvw"]
                dfaced = [dev.get("d" + nm + "1") for nm in "uvw"] if with_d else None
                hip.gpu_gradient_masked_walls(*ptrs, dev.put("p1", p), *dptrs, ps, walls, ni, nj, nkg, 0.5)
                check(hip)
                ref[with_d] = (faced, dfaced, [dev.get(nm + "1") for nm in "uvw"], [dev.get("d" + nm + "1") for nm in "uvw"] if with_d else None)
            for koff, nk, own0, own1, G in windows(nkg):
                where = (dims, walls, koff, nk)
                hip.fl_set_slab(koff, nkg, own0, own1, nk)
                pw = dev.put("wsolid", np.full((nk, nj, ni), 7, np.uint8))
                hip.gpu_wall_flags(pw, None, walls, ni, nj, nk)
                check(hip)
                assert np.array_equal(dev.get("wsolid"), window(solidw, koff, nk)), (where, "flags")
                # the w faces the window cannot decide or update: its first plane's lower face and its last plane's upper face,
                # where the cell beyond lies in the grid
                edge = np.ones(nk + 1, bool)
                if koff > 0:
                    edge[0] = False
                if koff + nk < nkg:
                    edge[nk] = False
                undecided = np.ones(nk + 1, bool)
                if koff == 1 and walls & WC.ZLO:
                    undecided[0] = False
                if koff + nk == nkg - 1 and walls & WC.ZHI:
                    undecided[nk] = False
                for with_d in (True, False):
                    faced, dfaced, grad, dgrad = ref[with_d]
                    start = [window(vel[0], koff, nk), window(vel[1], koff, nk), window(vel[2], koff, nk, 1)]
                    ptrs = [dev.put(nm, x) for nm, x in zip("uvw", start)]
                    dptrs = [dev.put("d" + nm, np.full_like(x, 9.0)) for nm, x in zip("uvw", start)] if with_d else [None] * 3
                    hip.gpu_wall_faces(*ptrs, *dptrs, pw, ni, nj, nk)
                    check(hip)
                    for c, nm in enumerate("uvw"):
                        keep = undecided if c == 2 else slice(None)
                        assert np.array_equal(dev.get(nm)[keep], window(faced[c], koff, nk, c == 2)[keep]), (where, "faces", nm)
                        if with_d:
                            wd = window(dfaced[c], koff, nk, c == 2)
                            got = dev.get("d" + nm)
                            inside = np.array([0 <= k + koff < nkg + (c == 2) for k in range(nk + (c == 2))])
                            sel = inside & undecided if c == 2 else inside
                            assert np.array_equal(got[sel], wd[sel]), (where, "face deltas", nm)
                            assert np.all(got[~inside] == 9.0)                                  # nothing written outside the grid
                    # the gradient, from the one-domain faces
                    start = [window(faced[0], koff, nk), window(faced[1], koff, nk), window(faced[2], koff, nk, 1)]
                    ptrs = [dev.put(nm, x) for nm, x in zip("uvw", start)]
                    hip.gpu_gradient_masked_walls(*ptrs, dev.put("wp", window(p, koff, nk)), *dptrs, pw, walls, ni, nj, nk, 0.5)
                    check(hip)
                    for c, nm in enumerate("uvw"):
                        keep = edge if c == 2 else slice(None)
                        assert np.array_equal(dev.get(nm)[keep], window(grad[c], koff, nk, c == 2)[keep]), (where, "gradient", nm)
                        if c == 2:                                              # left alone where the plane below is not in the window
                            assert np.array_equal(dev.get(nm)[~edge], start[2][~edge])
                        if with_d:
                            inside = np.array([0 <= k + koff < nkg for k in range(nk)])
                            got, wd = dev.get("d" + nm)[:nk][inside], window(dgrad[c], koff, nk, c == 2)[:nk][inside]
                            if c == 2:
                                got, wd = got[edge[:nk][inside]], wd[edge[:nk][inside]]
                            # (solid faces keep the 9.0 or the face pass's value: both runs started from the same fill)
                            assert np.array_equal(got, wd), (where, "gradient deltas", nm)
    finally:
        hip.fl_set_slab(0, 0, 0, 0, 0)
        dev.free()


_refs = {}


@pytest.mark.parametrize("scheme", [0, 2, 3])
@pytest.mark.parametrize("nranks,dims", [(2, (24, 20, 32)), (3, (24, 20, 36))])
def test_ranks_sharing_the_gpu_equal_the_one_gpu_walled_run(hip, tmp_path_factory, nranks, dims, scheme):
    from gpufluidsimulation_amd import solver
    key = (dims, scheme)
    if key not in _refs:
        path = str(tmp_path_factory.mktemp("walls_slab_gpu") / "ref.npz")
        hip.fl_set_slab(0, 0, 0, 0, 0)
        WS.reference(solver.host_lib(), hip, dims, 30, scheme, WS.BOX, 3, path)
        _refs[key] = path
    rc, out = WS.launch(nranks, "--backend", "gpu", "--dims", *dims, "--ghost", 6, "--iters", 30, "--scheme", scheme, "--walls", WS.BOX,
                        "--reference", _refs[key], timeout=240)
    assert rc == 0, out
    assert out.count("mismatches=0") == nranks, out


def test_cpp_rank_driver_two_ranks_in_the_container(tmp_path):
    """examples/bimocq3d_ranks.cpp with the walls argument: two ranks on this GPU through the stream-ordered stand-in for
    librccl run to the end and write per-slab dumps that stitch to the dumps of the same program as one rank"""
    from build_fake_rccl import build
    from gpufluidsimulation_amd.solver import read_density_dump
    exe = os.path.join(ROOT, "build", "bimocq3d_ranks")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "example"], cwd=ROOT)
    fake = build("async")
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    args = ["48", "40", "48", "3", None, "0", "6", "40", "0", "55"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([exe] + [one if a is None else a for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "last dump ok" in r.stdout, r.stdout[-2000:]
    procs = [subprocess.Popen([exe] + [two if a is None else a for a in args],
                              env=dict(env, RANK=str(rk), WORLD_SIZE="2", LOCAL_RANK="0", BQ_JOB_ID="w1", BQ_RCCL_LIBRARY=fake),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for rk in (1, 0)]
    outs = [q.communicate(timeout=120)[0] for q in procs]
    assert all(q.returncode == 0 for q in procs), outs
    assert "[rank 0/2]" in outs[1] and "last dump ok" in outs[0] and "last dump ok" in outs[1]
    files = sorted(x for x in os.listdir(one) if x.endswith(".bqd"))
    assert len(files) == 3
    for f in files:
        _, rec = read_density_dump(os.path.join(one, f))
        parts = sorted(q for q in os.listdir(two) if q.startswith(f[:-4] + ".k"))
        assert len(parts) == 2, (f, os.listdir(two))
        stitched = np.concatenate([read_density_dump(os.path.join(two, q))[1] for q in parts])
        assert len(rec) > 50 and stitched.tobytes() == rec.tobytes(), f
    # a closed mask of all six sides is a usage error
    r = subprocess.run([exe] + [one if a is None else a for a in args[:-1]] + ["63"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
