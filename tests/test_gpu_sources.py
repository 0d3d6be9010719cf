"""Shaped, moving smoke sources on the MI355X: gpu_emit_sources bit for bit against the C
restatement (tests/cpu_abi/source_abi.c) on odd shapes with mixed lists and at 256^3 with a level-set grid larger than one
L2, under a z-slab context against the one-GPU call, 20 steps of the 64^3 plume scene hash for hash against the CPU
stand-in, and two z-slab ranks sharing the GPU against the one-GPU run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import source_case as SC
from obstacle_case import Dev, check

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return hip, SC.load_sources()


def emit_gpu(hip, dev, fields, sources, h, dims):
    """gpu_emit_sources on device copies of {name: flat array}; returns the downloaded fields"""
    ptrs = {nm: dev.put(nm, fields[nm]) for nm in SC.NAMES}
    SC.call(hip, ptrs, sources, h, dims, phi_ptr=lambda o, s: dev.put(f"phi{o}", s.levelset.phi))
    check(hip)
    return {nm: dev.get(nm) for nm in SC.NAMES}


@pytest.mark.parametrize("dims", [(37, 29, 23), (99, 21, 18), (64, 64, 64)])
def test_operator_matches_the_restatement(libs, dims):
    hip, cpu = libs
    h, sources = SC.mixed(dims)
    dev = Dev(hip)
    try:
        for lst in (sources, sources[:2] + sources[4:], sources[2:4], list(reversed(sources))):     # mixed, analytic only, level sets only
            want = SC.emit_c(cpu, SC.pattern(dims), lst, h, dims)
            got = emit_gpu(hip, dev, SC.pattern(dims), lst, h, dims)
            for nm in SC.NAMES:
                assert np.array_equal(got[nm], want[nm]), (nm, len(lst))
            assert (want["rho"] != SC.pattern(dims)["rho"]).sum() > 100
        # an empty list and a list wholly outside the domain launch nothing and change nothing
        for lst in ([], sources[5:]):
            got = emit_gpu(hip, dev, SC.pattern(dims), lst, h, dims)
            for nm in SC.NAMES:
                assert np.array_equal(got[nm], SC.pattern(dims)[nm]), nm
    finally:
        dev.free()


def test_mapper_wrapper_and_solid_footprint(libs):
    """GpuMapper.emitSources (its own upload of the level-set grids; a generator argument) equals the restatement, and inside
    the node window the cells the list writes are the cells gpu_obstacle_flags_ls calls solid for the same shapes, owner
    for owner (section 16: a source node is exactly a solid node)"""
    import ctypes as C

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd.mapper import DeviceBuffer
    from gpufluidsimulation_amd.solver import LevelSetObstacle, levelset_arrays
    hip, cpu = libs
    dims = (37, 29, 23)
    ni, nj, nk = dims
    h, sources = SC.mixed(dims)
    for o, s in enumerate(sources):
        s.density = float(o + 1)
    want = SC.emit_c(cpu, SC.pattern(dims), sources, h, dims)
    m = bq.GpuMapper(ni, nj, nk, h)
    bufs = {nm: DeviceBuffer.from_numpy(a) for nm, a in SC.pattern(dims).items()}
    m.emitSources(bufs["u"], bufs["v"], bufs["w"], bufs["rho"], bufs["T"], (s for s in sources))
    check(hip)
    got = {nm: b.numpy() for nm, b in bufs.items()}
    for nm in SC.NAMES:
        assert np.array_equal(got[nm], want[nm]), nm
    rho = DeviceBuffer(ni * nj * nk)
    m.emitSources(bufs["u"], bufs["v"], bufs["w"], rho, bufs["T"], sources)
    check(hip)
    dev = Dev(hip)
    try:
        entries = [LevelSetObstacle(s.levelset, s.position) if s.levelset is not None else (s.code, *s.position, *s.extents, 0, 0, 0)
                   for s in sources]
        arr, ls, n = levelset_arrays(entries)
        for o, s in enumerate(sources):
            if s.levelset is not None:
                ls[o].phi = dev.put(f"phi{o}", s.levelset.phi)
        sp, rp = dev.put("solid", np.zeros(ni * nj * nk, np.uint8)), dev.put("rows", np.zeros(nj * nk, np.uint8))
        hip.gpu_obstacle_flags_ls(sp, rp, C.addressof(arr), n, C.addressof(ls), h, ni, nj, nk)
        check(hip)
        solid = dev.get("solid").reshape(nk, nj, ni)
    finally:
        dev.free()
    win = np.zeros((nk, nj, ni), bool)
    win[2:nk - 2, 2:nj - 2, 2:ni - 2] = True
    flags = np.where(win, solid, 0)
    assert np.array_equal(rho.numpy().reshape(nk, nj, ni), flags.astype(np.float32)) and len(np.unique(flags)) >= 5


def test_fine_levelset_source_at_256(libs):
    """voxel = h / 2: a 161^3 grid (16.7 MB, more than one XCD's L2), beside an analytic box and an overlapping sphere"""
    from gpufluidsimulation_amd.solver import Source, levelset_sphere
    hip, cpu = libs
    n = 256
    h = 1.0 / n
    dims = (n, n, n)
    ls = levelset_sphere(0.15, 0.5 * h)
    assert ls.phi.shape == (161, 161, 161)
    sources = [Source(("box", (0.1, 0.05, 0.2)), (0.3, 0.3, 0.5), 0.5, 1.5, 1, velocity=(0.0, 1.0, 0.0)),
               Source(ls, (0.5 + 0.3 * h, 0.45, 0.52), 1.0, 2.0, 1, velocity=(0.1, 0.5, -0.2), spin=(0.3, 1.5, -0.7)),
               Source(("sphere", 0.08), (0.62, 0.5, 0.5), 0.25, 0.75, 1)]
    cnt = {"rho": n ** 3, "T": n ** 3, "u": (n + 1) * n * n, "v": n * (n + 1) * n, "w": n * n * (n + 1)}
    fill = {nm: np.full(c, -3.0 - i, np.float32) for i, (nm, c) in enumerate(cnt.items())}
    want = SC.emit_c(cpu, {nm: a.copy() for nm, a in fill.items()}, sources, h, dims)
    dev = Dev(hip)
    try:
        got = emit_gpu(hip, dev, fill, sources, h, dims)
        for nm in SC.NAMES:
            assert np.array_equal(got[nm], want[nm]), nm
            assert (want[nm] != fill[nm]).sum() > 200000, nm
    finally:
        dev.free()


@pytest.mark.parametrize("nranks", [2, 3])
def test_slab_context_writes_the_global_planes(libs, nranks):
    """under fl_set_slab every stored plane receives what the one-GPU call writes on that global plane; stored planes
    outside the global grid stay untouched"""
    hip, _ = libs
    dims = (32, 32, 96)
    ni, nj, nkg = dims
    G = 6
    h, sources = SC.mixed(dims)
    sources = sources + [SC.mixed(dims)[1][0]]
    sources[-1].position = (0.5 * ni * h, 0.5 * nj * h, (nkg // nranks) * h + 0.2 * h)       # astride a slab boundary
    plane = {"rho": ni * nj, "T": ni * nj, "u": (ni + 1) * nj, "v": ni * (nj + 1), "w": ni * nj}
    dev = Dev(hip)
    try:
        whole = emit_gpu(hip, dev, SC.pattern(dims), sources, h, dims)
        base = SC.pattern(dims)
        touched = 0
        for r in range(nranks):
            own0, own1 = r * nkg // nranks, (r + 1) * nkg // nranks
            koff, nkl = own0 - G, own1 - own0 + 2 * G
            local, valid = {}, {}
            for nm in SC.NAMES:
                planes = nkl + (1 if nm == "w" else 0)
                gk = np.arange(koff, koff + planes)
                ok = (gk >= 0) & (gk < nkg + (1 if nm == "w" else 0))
                a = np.full((planes, plane[nm]), -7.0, np.float32)
                a[ok] = base[nm].reshape(-1, plane[nm])[gk[ok]]
                local[nm], valid[nm] = a.ravel(), (gk, ok)
            hip.fl_set_slab(koff, nkg, own0, own1, nkl)
            try:
                got = emit_gpu(hip, dev, local, sources, h, (ni, nj, nkl))
            finally:
                hip.fl_set_slab(0, 0, 0, 0, 0)
            for nm in SC.NAMES:
                gk, ok = valid[nm]
                g = got[nm].reshape(-1, plane[nm])
                assert np.array_equal(g[ok], whole[nm].reshape(-1, plane[nm])[gk[ok]]), (r, nm)
                assert np.all(g[~ok] == -7.0), (r, nm)
                touched += int((g[ok] != base[nm].reshape(-1, plane[nm])[gk[ok]]).sum())
        assert touched > 1000
    finally:
        dev.free()


@pytest.mark.parametrize("scheme,kind", [(0, 0), (3, 0), (0, 2)])
def test_plume_scene_matches_the_stand_in(libs, scheme, kind):
    """hashes of the CPU stand-in: tests/golden/make_source_hashes.py"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    with open(os.path.join(ROOT, "tests", "golden", "source_hashes.json")) as f:
        gold = json.load(f)
    want = gold[f"scheme{scheme}_kind{kind}"]
    iters = gold["pcg_iters"] if kind == 2 else gold["jacobi_iters"]
    got = SC.run_scene(solver.host_lib(), hip, gold["n"], scheme, len(want["hashes"]), iters, kind=kind)
    first = next((i for i, (a, b) in enumerate(zip(want["hashes"], got["hashes"])) if a != b), None)
    assert first is None, f"step {first} differs (rho max {got['rho_max']} vs {want['rho_max']})"
    assert want["rho_max"] >= 1.0


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_slab_ranks_reproduce_the_one_gpu_plume(libs, tmp_path):
    """two z-slab ranks sharing the GPU over the host-staged transport (tests/source_slab_worker.py), each a child under
    its own time limit, against the one-GPU run of the same scene: owned planes bit for bit"""
    from gpufluidsimulation_amd import solver
    hip, _ = libs
    import source_slab_worker as W
    ref = str(tmp_path / "one_gpu.npz")
    s = W.make_solver(solver.host_lib(), hip)
    out = {}
    for f in range(W.STEPS):
        s.advance(f, W.DT)
        s._check()
        for nm in W.FIELDS:
            out[f"{nm}{f}"] = s.field(nm)
    assert np.abs(out[f"w{W.STEPS - 1}"]).max() > 0.01 and out[f"rho{W.STEPS - 1}"].max() >= 1.0
    s.close()
    np.savez(ref, **out)
    port = str(free_port())
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                   OMP_NUM_THREADS="2")
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "source_slab_worker.py"), ref]
        procs.append(subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=400)[0] for p in procs]
    for rank, (p, text) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {rank}: exit {p.returncode}\n{text[-3000:]}"
