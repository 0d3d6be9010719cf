"""Flow diagnostics without a GPU: the restatement of gpu_flow_stats against known answers, and the
C++ host solver's diagnostics, history ring, vorticity field and vorticity dump on the CPU stand-ins of the operator ABI."""
import ctypes as C
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import diag_case as D
import maccormack_case as MC
from build_cpu_host import build as build_cpu_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, H = (12, 10, 9), 0.125
SOLVER_DIMS, L, ITERS = (16, 12, 10), 1.0, 8
DT = 1.0 / SOLVER_DIMS[0]
f32 = np.float32


@pytest.fixture(scope="module")
def standin():
    return D.load_diag()


@pytest.fixture(scope="module")
def plain():
    """the stand-in WITHOUT gpu_flow_stats: the host solver's weak reference stays null"""
    import obstacle_case as OC
    from gpufluidsimulation_amd import solver
    return OC.bind_errors(solver.bind_host(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL)))


def mac(ufun, vfun, wfun, dims=DIMS, h=H):
    """a MAC velocity from functions of the face positions (cell centres at i h: the u face at (i - 1/2) h)"""
    ni, nj, nk = dims
    out = []
    for (nx, ny, nz), off, fn in (((ni + 1, nj, nk), (-0.5, 0, 0), ufun), ((ni, nj + 1, nk), (0, -0.5, 0), vfun),
                                 ((ni, nj, nk + 1), (0, 0, -0.5), wfun)):
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        x, y, z = (i + off[0]) * h, (j + off[1]) * h, (k + off[2]) * h
        out.append(np.ascontiguousarray(np.broadcast_to(fn(x, y, z), x.shape).astype(f32).ravel()))
    return out


def stats(lib, u, v, w, rho=None, T=None, vort=None, dims=DIMS, h=H):
    out = np.full(10, -1.0)
    p = lambda a: None if a is None else a.ctypes.data
    rc = lib.gpu_flow_stats(p(u), p(v), p(w), p(rho), p(T), p(vort), h, *dims, out.ctypes.data)
    return rc, dict(zip(D.STAT, out))


def interior(dims=DIMS):
    ni, nj, nk = dims
    m = np.zeros((nk, nj, ni), dtype=bool)
    m[1:-1, 1:-1, 1:-1] = True
    return m


def test_rigid_rotation_has_vorticity_two_omega(standin):
    """u = -Omega y, v = Omega x with values that are exact in float: wz = 2 Omega in every interior cell, wx = wy = 0,
    no divergence; border cells hold 0"""
    omega = 0.5
    u, v, w = mac(lambda x, y, z: -omega * y, lambda x, y, z: omega * x, lambda x, y, z: 0.0 * x)
    vort = np.full(np.prod(DIMS), 7.0, dtype=f32)
    rc, s = stats(standin, u, v, w, vort=vort)
    assert rc == 0
    m = interior()
    vort = vort.reshape(m.shape)
    assert (vort[m] == f32(2 * omega)).all() and (vort[~m] == 0).all()
    assert s["div_max"] == 0.0 and s["d2"] == 0.0
    assert s["vort_max"] == 2 * omega and s["m2"] == m.sum() * (2 * omega) ** 2
    _, m2, _, _ = D.terms(standin, u, v, w, H, DIMS)
    assert (m2.reshape(m.shape)[m] == (2 * omega) ** 2).all()


def test_uniform_flow_has_its_kinetic_energy_and_no_enstrophy(standin):
    U = (0.5, -0.25, 1.5)
    u, v, w = mac(lambda x, y, z: U[0] + 0 * x, lambda x, y, z: U[1] + 0 * x, lambda x, y, z: U[2] + 0 * x)
    rc, s = stats(standin, u, v, w)
    n = int(np.prod(DIMS))
    assert rc == 0 and s["e2"] == n * sum(c * c for c in U)
    assert s["m2"] == 0.0 and s["vort_max"] == 0.0 and s["d2"] == 0.0
    row = D.diag_row(s, H)
    assert row["kinetic"] == 0.5 * H ** 3 * n * sum(c * c for c in U) and row["enstrophy"] == 0.0


def test_a_single_density_cell_is_the_centroid(standin):
    u, v, w = mac(lambda x, y, z: 0 * x, lambda x, y, z: 0 * x, lambda x, y, z: 0 * x)
    ni, nj, nk = DIMS
    rho = np.zeros((nk, nj, ni), dtype=f32)
    rho[6, 3, 7] = 2.5
    T = np.full((nk, nj, ni), 0.25, dtype=f32)
    rc, s = stats(standin, u, v, w, rho=rho.ravel(), T=T.ravel())
    assert rc == 0
    row = D.diag_row(s, H)
    assert (row["rho_sum"], row["centroid_x"], row["centroid_y"], row["centroid_z"]) == (2.5, 7 * H, 3 * H, 6 * H)
    assert row["T_sum"] == 0.25 * ni * nj * nk
    rc, s = stats(standin, u, v, w)                    # no scalars: their entries are 0, and so is the centroid
    assert [s[k] for k in ("rho", "rho_i", "rho_j", "rho_k", "T")] == [0.0] * 5
    assert D.diag_row(s, H)["centroid_y"] == 0.0


def test_the_restatement_refuses_what_the_contract_refuses(standin):
    import fields as F
    u, v, w = F.velocity(*DIMS, H)
    vort = np.zeros(np.prod(DIMS), dtype=f32)
    calls = standin.flow_stats_abi_calls(1)
    for kw in (dict(u=None), dict(dims=(2, 10, 9)), dict(dims=(12, 10, 2))):
        args = dict(u=u, v=v, w=w)
        args.update(kw)
        rc, s = stats(standin, **args)
        assert rc == 3 and standin.fl_last_error() == 3 and s["e2"] == -1.0
        standin.fl_clear_error()
    rho = np.zeros(np.prod(DIMS), dtype=f32)
    rc, s = stats(standin, u, v, w, rho=rho, vort=rho)
    assert rc == 3 and s["e2"] == -1.0
    standin.fl_clear_error()
    assert standin.flow_stats_abi_calls(1) == 0


def test_option_zero_launches_nothing(standin):
    from gpufluidsimulation_amd import solver
    standin.flow_stats_abi_calls(1)
    _, _, hist, _ = D.run_with_diagnostics(standin, standin, SOLVER_DIMS, L, 3, ITERS, DT)
    assert hist.shape == (0, solver.DIAG_COUNT)
    assert standin.flow_stats_abi_calls(1) == 1        # the vorticity() at the end of the helper, nothing from the steps
    s = solver.BimocqGPUSolver(*SOLVER_DIMS, L, 0.0, 1.0, lib=standin, errlib=standin)
    assert s.getOption(solver.OPT_DIAGNOSTICS_EVERY) == 0
    for f in range(3):
        s.advance(f, DT)
    s._check()
    assert standin.flow_stats_abi_calls(1) == 0
    s.close()


@pytest.mark.parametrize("scheme", (0, 2, 3))
def test_history_rows_equal_the_blocking_calls(standin, scheme):
    """option 2 over six steps: three rows with STEP 2, 4, 6, each equal to bq_solver_diagnostics taken at that step"""
    from gpufluidsimulation_amd import solver
    standin.flow_stats_abi_calls(1)
    out, taken, hist, _ = D.run_with_diagnostics(standin, standin, SOLVER_DIMS, L, 6, ITERS, DT, scheme=scheme, every=2,
                                                 sample={2, 4, 6})
    assert standin.flow_stats_abi_calls(1) == 3 + 3 + 1
    assert hist.shape == (3, solver.DIAG_COUNT) and hist[:, -1].tolist() == [2.0, 4.0, 6.0]
    for r, step in enumerate((2, 4, 6)):
        want = np.array([taken[step][k] for k in solver.DIAG_NAMES], dtype=np.float64)
        assert hist[r].view(np.uint64).tolist() == want.view(np.uint64).tolist(), (step, hist[r], want)
    assert hist[-1, 0] > 0 and hist[-1, 1] > 0 and hist[-1, 4] > 0
    # and the rows are the restatement's sums of the downloaded fields, carried through diag_row
    h = float(f32(L) / f32(SOLVER_DIMS[0]))
    last = out[-1]
    _, s = stats(standin, last["u"], last["v"], last["w"], rho=last["rho"], T=last["T"], dims=SOLVER_DIMS, h=h)
    want = D.diag_row(s, h, 6)
    assert [taken[6][k] for k in solver.DIAG_NAMES] == [want[k] for k in solver.DIAG_NAMES]


def test_the_ring_keeps_the_last_1024_rows(standin):
    from gpufluidsimulation_amd import solver
    s = solver.BimocqGPUSolver(8, 8, 8, 1.0, 0.0, 1.0, lib=standin, errlib=standin)
    s.setProjection(1, 0.5)
    s.setOption(solver.OPT_DIAGNOSTICS_EVERY, 1)
    for f in range(1030):
        s.advance(f, 0.01)
    hist = s.diagnosticsHistory()
    s._check()
    s.close()
    assert hist.shape == (1024, solver.DIAG_COUNT)
    assert hist[:, -1].tolist() == [float(a) for a in range(7, 1031)]


def test_a_standin_without_the_operator_is_unsupported(plain):
    from gpufluidsimulation_amd import BimocqError, solver
    s = solver.BimocqGPUSolver(*SOLVER_DIMS, L, 0.0, 1.0, lib=plain, errlib=plain)
    out = (C.c_double * solver.DIAG_COUNT)()
    assert plain.bq_solver_diagnostics(s.s, out) == 4 and plain.fl_last_error() == 4
    plain.fl_clear_error()
    with pytest.raises(BimocqError, match="error 4"):
        s.diagnostics()
    with pytest.raises(BimocqError, match="error 4"):
        s.setOption(solver.OPT_DIAGNOSTICS_EVERY, 2)
    assert s.getOption(solver.OPT_DIAGNOSTICS_EVERY) == 0
    with pytest.raises(BimocqError, match="error 4"):
        s.vorticity()
    s.advance(0, DT)
    s._check()
    s.close()


def test_bad_option_value_is_refused(standin):
    from gpufluidsimulation_amd import BimocqError, solver
    s = solver.BimocqGPUSolver(*SOLVER_DIMS, L, 0.0, 1.0, lib=standin, errlib=standin)
    with pytest.raises(BimocqError, match="error 3"):
        s.setOption(solver.OPT_DIAGNOSTICS_EVERY, -1)
    assert s.getOption(solver.OPT_DIAGNOSTICS_EVERY) == 0
    s.close()


def test_python_names():
    from gpufluidsimulation_amd import _lib, solver
    assert solver.OPT_DIAGNOSTICS_EVERY == 16 and _lib.FL_OPT_DIAG_KCHUNK == 22
    assert solver.DIAG_COUNT == 11 and _lib.STAT_COUNT == 10
    text = open(os.path.join(ROOT, "include", "bimocq_solver.h")).read()
    assert "BQ_OPT_DIAGNOSTICS_EVERY = 16" in text
    assert "FL_OPT_DIAG_KCHUNK     = 22" in open(os.path.join(ROOT, "include", "bimocq_gpu.h")).read()


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_vorticity_dump_round_trips_and_leaves_the_density_dump_alone(standin, tmp_path):
    from gpufluidsimulation_amd import solver
    s = solver.BimocqGPUSolver(*SOLVER_DIMS, L, 0.0, 1.0, lib=standin, errlib=standin)
    s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(SOLVER_DIMS, L))
    s.setProjection(ITERS, 0.5)
    for f in range(3):
        s.advance(f, DT)
    path = str(tmp_path)
    n_rho = s.outputResult(2, path)
    before = sha(os.path.join(path, "density_render_0003.bqd"))
    cut = 0.05
    n = s.outputVorticity(2, path, cut)
    vort = s.vorticity()
    s.outputResult(2, path)
    assert sha(os.path.join(path, "density_render_0003.bqd")) == before
    s.close()
    hd, rec = solver.read_density_dump(os.path.join(path, "vorticity_render_0003.bqd"))
    assert hd["grid_name"] == b"vorticity" and hd["frame"] == 3 and hd["threshold"] == f32(cut)
    assert (hd["nx"], hd["ny"], hd["nz"], hd["k_offset"], hd["nz_local"]) == (*SOLVER_DIMS, 0, SOLVER_DIMS[2])
    keep = vort.astype(np.float64) > float(f32(cut))
    assert n == len(rec) == keep.sum() > 0 and n < vort.size
    back = np.zeros_like(vort)
    back[rec["k"], rec["j"], rec["i"]] = rec["value"]
    assert np.array_equal(back, np.where(keep, vort, 0))
    # the density dump is still the container it was: header fields and records of the density field
    hd, rec = solver.read_density_dump(os.path.join(path, "density_render_0003.bqd"))
    assert hd["grid_name"] == b"density" and hd["threshold"] == f32(1e-4) and len(rec) == n_rho > 0


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_slabs(backend, ref_path, nproc=2, threads=2):
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "diag_slab_worker.py"), "--backend", backend, "--reference", ref_path]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("[rank")]
    return r.returncode, "\n".join(lines[-40:]) or r.stdout[-3000:]


def test_two_slab_ranks_agree_with_one_domain(tmp_path):
    """two z-slab ranks of 24 x 20 x 32 after 4 steps: every rank's diagnostics lie within the summation bound of the exact
    sums over the single-domain fields, the stitched vorticity() is bit-equal"""
    import diag_slab_worker as W
    ref = str(tmp_path / "ref.npz")
    W.reference("cpu", ref)
    rc, out = launch_slabs("cpu", ref)
    assert rc == 0, out
    assert out.count("mismatches=0") == 2
