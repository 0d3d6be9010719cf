"""The shadowed density preview on the GPU: gpu_render_density -- the marches along y and z at the
kernels' own and at forced chunk lengths, the wave-scan kernels along x -- against the C restatement (tests/cpu_abi/
render_abi.c), and the host solver's render() and outputPreview() on the HIP library.

Every accumulated quantity of the contract is an integer below 2^53: both image planes and the shadow field must equal the
restatement BIT FOR BIT, for every axis, direction, chunking and rank count.  No tolerance anywhere."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import obstacle_case as OC
import render_case as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
# the base case; the spacing that is not a power of two; a wave plus six lanes along x; three wave segments with a remainder
# and rows shorter than a block; chunk seams along z
SHAPES = [(16, 16, 16, 1.0 / 16), (40, 36, 30, 0.01), (70, 33, 20, 1.0 / 64), (130, 12, 9, 1.0 / 128), (12, 10, 67, 1.0 / 8)]
KCHUNKS = (0, 1, 5, -1)
ALBEDO, AMBIENT = 0.875, 0.125


def lights_for(shape, view):
    """16^3: none, the view's own direction, its opposite, two perpendicular ones; else three lights, one on every axis"""
    a = view // 2
    p1, p2 = 2 * ((a + 1) % 3), 2 * ((a + 2) % 3) + 1
    return (-1, view, view ^ 1, p1, p2) if shape[:3] == (16, 16, 16) else (view, p1, p2)


def sigma_for(shape):
    """sigma h = 0.4 (as near as float gets): a ray of random cells passes optical depths from 0 to a few units"""
    return float(f32(0.4) / f32(shape[3]))


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    yield lib
    lib.fl_set_option(R.FL_OPT_RENDER_KCHUNK, 0)
    bq.check()


@functools.lru_cache(maxsize=None)
def cpu():
    return R.load_render()


@functools.lru_cache(maxsize=None)
def case(shape, view, light, sigma=None, seed=0):
    """the restatement's image and shadow field for a shape, computed once and frozen"""
    dims, h = shape[:3], float(f32(shape[3]))
    rc, img, shadow = R.restate(cpu(), R.density(dims, seed), dims, h, view, light, sigma or sigma_for(shape), ALBEDO, AMBIENT)
    assert rc == 0
    img.setflags(write=False)
    return img, shadow


def render(hip, dev, dims, h, view, light, sigma, albedo=ALBEDO, ambient=AMBIENT, rho="rho"):
    """the operator on dev[rho]: (image (2, H, W), shadow or None); the outputs are poisoned first, every element must be written"""
    ni, nj, nk = dims
    H, W = R.image_shape(dims, view)
    dev.put("img", np.full((2, H, W), -1.0))
    if light >= 0:
        dev.put("shadow", np.full((nk, nj, ni), 7.0, f32))
    p = R.params(sigma, albedo, ambient)
    rc = hip.gpu_render_density(dev[rho], dev["shadow"] if light >= 0 else None, h, ni, nj, nk, view, light, C.cast(p, C.c_void_p), dev["img"])
    OC.check(hip)
    assert rc == 0
    return dev.get("img"), (dev.get("shadow") if light >= 0 else None)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                  b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_operator_equals_the_restatement(hip, shape):
    """all six views, the lights of lights_for, chunk options 0, 1, 5 and -1: both image planes and the shadow field bit
    for bit; the density is left alone"""
    dims, h = shape[:3], float(f32(shape[3]))
    rho = R.density(dims)
    dev = OC.Dev(hip)
    try:
        dev.put("rho", rho)
        lit = 0
        for view in range(6):
            for light in lights_for(shape, view):
                want, want_shadow = case(shape, view, light)
                lit += int(want[0].max() > 0 and want[1].max() > 0)
                for kc in KCHUNKS:
                    hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, kc)
                    assert hip.fl_get_option(R.FL_OPT_RENDER_KCHUNK) == kc
                    img, shadow = render(hip, dev, dims, h, view, light, sigma_for(shape))
                    assert same_bits(img[1], want[1]), (view, light, kc, "Afix", np.abs(img[1] - want[1]).max())
                    assert same_bits(img[0], want[0]), (view, light, kc, "Cfix", np.abs(img[0] - want[0]).max())
                    if light >= 0:
                        assert same_bits(shadow, want_shadow), (view, light, kc, "shadow", np.abs(shadow - want_shadow).max())
        assert lit == 6 * len(lights_for(shape, 0))
        assert same_bits(dev.get("rho"), rho)
    finally:
        hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, 0)
        dev.free()


def test_opaque_media_reach_the_cut_off(hip):
    """sigma h = 40 at 16^3: most non-empty cells clamp at d = 32 and four of them in a row pass 128 * 2^32, where att is
    exactly 0 -- bit for bit again, and some shadow cells and pixels really are 0"""
    shape = SHAPES[0]
    dims, h = shape[:3], float(f32(shape[3]))
    sigma = float(f32(40.0) / f32(h))
    dev = OC.Dev(hip)
    try:
        dev.put("rho", R.density(dims))
        for view, light in ((4, 3), (0, 5), (3, 1), (1, 0)):
            want, want_shadow = case(shape, view, light, sigma)
            assert (want_shadow == 0).any() and (want[1] >= 128 * R.TWO32).any()
            for kc in KCHUNKS:
                hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, kc)
                img, shadow = render(hip, dev, dims, h, view, light, sigma)
                assert same_bits(img, np.asarray(want)) and same_bits(shadow, want_shadow), (view, light, kc)
    finally:
        hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, 0)
        dev.free()


def permuted(rho, dims, perm):
    """the volume with grid axis a moved to axis perm[a] (0 = x): (copy (nk', nj', ni'), dims')"""
    xyz = rho.transpose(2, 1, 0)
    axes = [0, 0, 0]
    for a in range(3):
        axes[perm[a]] = a
    out = np.ascontiguousarray(np.transpose(xyz, axes).transpose(2, 1, 0))
    d2 = [0, 0, 0]
    for a in range(3):
        d2[perm[a]] = dims[a]
    return out, tuple(d2)


@pytest.mark.parametrize("perm", [(1, 2, 0), (2, 1, 0)], ids=["cycle", "swap-xz"])
def test_axis_permutation_permutes_the_image(hip, perm):
    """independent of the restatement: the axis-permuted copy of the volume rendered along the permuted view and light gives
    the permuted image bit for bit -- the wave scan along x against the marches along y and z"""
    shape = SHAPES[2]
    dims, h, sigma = shape[:3], float(f32(shape[3])), sigma_for(shape)
    rho = R.density(dims)
    rho2, dims2 = permuted(rho, dims, perm)
    code = lambda d: d if d < 0 else 2 * perm[d // 2] + (d & 1)
    dev = OC.Dev(hip)
    try:
        dev.put("rho", rho)
        dev.put("rho2", rho2)
        for view in range(6):
            for light in lights_for(shape, view):
                img, _ = render(hip, dev, dims, h, view, light, sigma)
                img2, _ = render(hip, dev, dims2, h, code(view), code(light), sigma, rho="rho2")
                lo, hi = sorted({0, 1, 2} - {view // 2})
                if perm[lo] > perm[hi]:
                    img2 = img2.transpose(0, 2, 1)
                assert img[0].max() > 0 and same_bits(np.ascontiguousarray(img2), img), (view, light)
    finally:
        dev.free()


def test_z_mirror_under_minus_z_equals_plus_z(hip):
    """independent of the restatement: the z-mirrored volume seen along -z is the original seen along +z"""
    shape = SHAPES[4]
    dims, h, sigma = shape[:3], float(f32(shape[3])), sigma_for(shape)
    rho = R.density(dims)
    dev = OC.Dev(hip)
    try:
        dev.put("rho", rho)
        dev.put("mirror", np.ascontiguousarray(rho[::-1]))
        for light in (-1, 0, 3, 4, 5):
            mirrored = light ^ 1 if light >= 4 else light
            for kc in (0, 5):
                hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, kc)
                img, _ = render(hip, dev, dims, h, 4, light, sigma)
                img2, _ = render(hip, dev, dims, h, 5, mirrored, sigma, rho="mirror")
                assert img[0].max() > 0 and same_bits(img, img2), (light, kc)
    finally:
        hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, 0)
        dev.free()


def test_refusals_launch_nothing(hip):
    shape = SHAPES[1]
    dims, h = shape[:3], float(f32(shape[3]))
    ni, nj, nk = dims
    dev = OC.Dev(hip)
    try:
        rho = R.density(dims)
        dev.put("rho", rho)
        dev.put("img", np.full((2, nk, nj), -1.0))
        dev.put("shadow", np.full((nk, nj, ni), 7.0, f32))
        r, sh, img = dev["rho"], dev["shadow"], dev["img"]
        ok = R.params(4.0, 1.0, 0.1)
        P = lambda *a: R.params(*a)
        nan, inf = float("nan"), float("inf")
        bad = [(None, sh, h, *dims, 4, 3, ok, img), (r, sh, h, *dims, 4, 3, None, img), (r, sh, h, *dims, 4, 3, ok, None),
               (r, sh, h, *dims, 6, 3, ok, img), (r, sh, h, *dims, -1, 3, ok, img), (r, sh, h, *dims, 4, 6, ok, img),
               (r, sh, h, *dims, 4, -2, ok, img), (r, None, h, *dims, 4, 3, ok, img), (r, r, h, *dims, 4, 3, ok, img),
               (r, sh, h, *dims, 4, 3, ok, r), (r, sh, h, *dims, 4, 3, P(-1.0, 1.0, 0.1), img), (r, sh, h, *dims, 4, 3, P(nan, 1.0, 0.1), img),
               (r, sh, h, *dims, 4, 3, P(inf, 1.0, 0.1), img), (r, sh, h, *dims, 4, 3, P(4.0, -0.5, 0.1), img),
               (r, sh, h, *dims, 4, 3, P(4.0, nan, 0.1), img), (r, sh, h, *dims, 4, 3, P(4.0, 1.0, -0.1), img),
               (r, sh, h, *dims, 4, 3, P(4.0, 1.0, inf), img), (r, sh, h, *dims, 4, 3, P(4.0, 3.0, 1.5), img),
               (r, sh, 0.0, *dims, 4, 3, ok, img), (r, sh, -h, *dims, 4, 3, ok, img), (r, sh, nan, *dims, 4, 3, ok, img),
               (r, sh, h, 0, nj, nk, 4, 3, ok, img), (r, sh, h, ni, nj, 65535, 4, 3, ok, img), (r, sh, h, 65535, nj, nk, 4, 3, ok, img),
               (r, sh, h, 2048, 2048, 128, 4, 3, ok, img), (r, sh, h, 4096, 2048, 2, 4, 3, ok, img)]
        for kc in (0, -1):
            hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, kc)
            for args in bad:
                args = [C.cast(a, C.c_void_p) if isinstance(a, C.Array) else a for a in args]
                assert hip.gpu_render_density(*args) == R.BAD_ARGUMENT, args
                assert hip.fl_last_error() == R.BAD_ARGUMENT
                hip.fl_clear_error()
        assert (dev.get("img") == -1.0).all() and (dev.get("shadow") == 7.0).all() and same_bits(dev.get("rho"), rho)
    finally:
        hip.fl_set_option(R.FL_OPT_RENDER_KCHUNK, 0)
        dev.free()


def test_solver_render_after_rising_smoke(hip, tmp_path):
    """a few rising-smoke steps at 32^3: render() equals the restatement applied to field("rho"), converted as the header
    says; outputPreview's pixels equal the formula"""
    from gpufluidsimulation_amd.solver import DIRECTIONS, BimocqGPUSolver
    N = 32
    s = BimocqGPUSolver(N, N, N, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1000)])
    s.setProjection(30, 0.5)
    for f in range(4):
        s.advance(f, 2.0 / N)
    rho = s.field("rho")
    h = float(f32(1.0) / f32(N))
    for view, light in (("+z", "-y"), ("-x", "+z"), ("+y", None), ("-z", "+x")):
        rad, tr = s.render(view, light, sigma=16.0, albedo=1.0, ambient=0.1)
        rc, img, _ = R.restate(cpu(), rho, (N, N, N), h, DIRECTIONS[view], -1 if light is None else DIRECTIONS[light], 16.0, 1.0, 0.1)
        want_rad, want_tr = R.convert(cpu().orc_expf, img)
        assert rc == 0 and rad.shape == (N, N) and same_bits(rad, want_rad) and same_bits(tr, want_tr), (view, light)
        assert rad.max() > 0.05 and tr.min() < 0.9 and tr.max() == 1.0
    n = s.outputPreview(3, str(tmp_path), "+z", "-y", 16.0, 1.0, 0.1, 0.25)
    rad, tr = s.render("+z", "-y", 16.0, 1.0, 0.1)
    s._check()
    s.close()
    w, hh, px = R.pgm(str(tmp_path / "preview_0004.pgm"))
    assert (w, hh) == (N, N) and n == os.path.getsize(str(tmp_path / "preview_0004.pgm"))
    assert np.array_equal(px, R.pgm_pixels(rad, tr, 0.25)) and px.max() > px.min()


def test_two_slab_ranks_on_the_gpu(tmp_path):
    """two z-slab ranks (processes) of 16^3 sharing the GPU over the stream-ordered stand-in for librccl, so that the gather
    of the column totals and the image's all-reduce run inside the compute stream: all six views with lights -y and +z
    equal the single domain's images bit for bit on every rank (tests/render_slab_worker.py).  16^3 because the stand-in
    reduces at most 4096 bytes per call: the gather and the images are 512 doubles each"""
    import render_slab_worker as W
    from build_fake_rccl import build
    from test_diagnostics_cpu import free_port
    ref = str(tmp_path / "ref.npz")
    W.reference("gpu", ref, (16, 16, 16))
    os.makedirs(str(tmp_path / "out"))
    env = dict(os.environ, OMP_NUM_THREADS="4", MASTER_ADDR="127.0.0.1", BQ_RCCL_LIBRARY=build("async"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "render_slab_worker.py"), "--backend", "gpu",
           "--transport", "rccl", "--reference", ref, "--outdir", str(tmp_path / "out"), "--dims", "16", "16", "16"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    lines = "\n".join(l for l in r.stdout.splitlines() if l.startswith("[rank")) or r.stdout[-3000:]
    assert r.returncode == 0, lines
    assert lines.count("mismatches=0") == 2


def test_example_driver_with_previews(tmp_path):
    """build/bimocq3d with preview_every = 2: exits 0 and writes a preview next to the density dumps for every second frame"""
    exe = os.path.join(ROOT, "build", "bimocq3d")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "example"], cwd=ROOT)
    out = str(tmp_path / "out")
    r = subprocess.run([exe, "48", "4", out, "0", "0", "1", "0", "0", "0", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("[ Preview bytes:") == 2 and "last dump ok" in r.stdout
    files = sorted(os.listdir(out))
    assert files == [f"density_render_{i:04d}.bqd" for i in range(1, 5)] + ["preview_0002.pgm", "preview_0004.pgm"], files
    w, h, px = R.pgm(os.path.join(out, files[-1]))
    assert (w, h) == (48, 48) and px.max() > 32 and px.min() == 0
