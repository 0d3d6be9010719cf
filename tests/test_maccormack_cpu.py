"""The MacCormack scheme (scheme 2) without a GPU: the C++ host solver on the CPU stand-ins of the
operator ABI against tests/scheme_ref.py, the step written out on the oracle's operators.  Value for value (fields.same)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fields as F
import maccormack_case as MC
from build_cpu_host import build as build_cpu_host
from scheme_ref import MacCormackRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, L, STEPS, ITERS = (24, 20, 16), 1.0, 8, 16
DT = 4.0 / DIMS[0]
VISCOSITIES = (0.0, 1e-3)


@pytest.fixture(scope="module")
def plain():
    """the stand-in WITHOUT gpu_maccormack: the host solver's weak reference stays null"""
    import obstacle_case as OC
    from gpufluidsimulation_amd import solver
    return OC.bind_errors(solver.bind_host(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL)))


@pytest.fixture(scope="module")
def standin():
    return MC.load_maccormack()


@pytest.fixture(scope="module")
def reference():
    """{viscosity: ([fields after each step], [cfldt], limiter counts)} of the Python restatement, computed once"""
    out = {}
    for nu in VISCOSITIES:
        r = MacCormackRef(*DIMS, L, nu)
        r.set_smoke(MC.DROP, MC.RISE, MC.emitters_for(DIMS, L))
        r.set_projection(ITERS, 0.5)
        steps, cfl = [], []
        for f in range(STEPS):
            r.advance(f, DT)
            steps.append({n: r.field(n).copy() for n in MC.NAMES})
            cfl.append(float(r.cfldt))
        for a in steps[-1].values():
            a.setflags(write=False)
        out[nu] = (steps, cfl, dict(r.limited))
    return out


def same_steps(got, want, what):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        for n in MC.NAMES:
            assert F.same(a[n], b[n]), (what, f, n, F.maxdiff(a[n], b[n]))


def test_the_reference_run_is_a_real_test(reference):
    """the trajectory moves, stays finite, takes more than one trace sub-step and exercises both limiter branches"""
    for nu in VISCOSITIES:
        steps, cfl, limited = reference[nu]
        last = steps[-1]
        assert all(np.isfinite(last[n]).all() for n in MC.NAMES)
        assert np.abs(last["u"]).max() > 0.05 and last["rho"].sum() > 50.0
        assert np.float32(DT) / np.float32(cfl[-1]) > 1.0, cfl
        n_scalar = 2 * STEPS * last["rho"].size
        n_vel = STEPS * (last["u"].size + last["v"].size + last["w"].size)
        assert 0 < limited["scalar"] < n_scalar and 0 < limited["velocity"] < n_vel, limited


def test_create_accepts_scheme_2_and_still_refuses_scheme_1(plain):
    s = plain.bq_solver_create(0, *DIMS, L, 0.0, 1.0, 2)
    assert s
    plain.bq_solver_destroy(s)
    assert not plain.bq_solver_create(0, *DIMS, L, 0.0, 1.0, 1)
    s = plain.bq_solver_create_slab(0, *DIMS, L, 0.0, 1.0, 2, 0, 1, 0)
    assert s
    plain.bq_solver_destroy(s)
    assert not plain.bq_solver_create_slab(0, *DIMS, L, 0.0, 1.0, 1, 0, 1, 0)
    plain.fl_clear_error()


@pytest.mark.parametrize("nu", VISCOSITIES)
def test_unfused_body_equals_the_reference(plain, reference, nu):
    """a stand-in without gpu_maccormack: the host solver runs the separate launches, whatever the option says"""
    want, cfl, _ = reference[nu]
    got, got_cfl = MC.run(plain, plain, DIMS, L, STEPS, ITERS, DT, scheme=2, viscosity=nu)
    assert got_cfl == cfl
    assert np.float32(DT) / np.float32(got_cfl[-1]) > 1.0
    same_steps(got, want, "unfused")


@pytest.mark.parametrize("nu", VISCOSITIES)
def test_fused_body_equals_the_reference(standin, reference, nu):
    want, cfl, _ = reference[nu]
    for option in (1, 0):
        standin.maccormack_abi_calls(1)
        got, got_cfl = MC.run(standin, standin, DIMS, L, STEPS, ITERS, DT, scheme=2, fused=option, viscosity=nu)
        calls = standin.maccormack_abi_calls(1)
        assert got_cfl == cfl
        same_steps(got, want, f"option {option}")
        assert (calls == 5 * STEPS) if option else (calls == 0), (option, calls)


def test_default_option_is_fused_in_scheme_2_only(standin):
    standin.maccormack_abi_calls(1)
    MC.run(standin, standin, DIMS, L, 2, ITERS, DT, scheme=2)
    assert standin.maccormack_abi_calls(1) == 10
    MC.run(standin, standin, DIMS, L, 2, ITERS, DT, scheme=3)
    assert standin.maccormack_abi_calls(1) == 0


def test_reflection_with_the_option(standin):
    """MAC_REFLECTION: option 2 fuses both of its velocity advections and the scalars' and leaves every value alone;
    option 1 does not touch it"""
    runs, calls = {}, {}
    for option in (0, 1, 2):
        standin.maccormack_abi_calls(1)
        runs[option], _ = MC.run(standin, standin, DIMS, L, 3, ITERS, DT, scheme=3, fused=option, viscosity=1e-3)
        calls[option] = standin.maccormack_abi_calls(1)
    assert calls == {0: 0, 1: 0, 2: 3 * 8}, calls
    same_steps(runs[2], runs[0], "reflection, option 2")
    same_steps(runs[1], runs[0], "reflection, option 1")
    assert np.abs(runs[0][-1]["v"]).max() > 0.01


def test_bad_option_value_is_refused(standin):
    from gpufluidsimulation_amd import BimocqError
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    s = BimocqGPUSolver(*DIMS, L, 0.0, 1.0, lib=standin, errlib=standin, scheme=2)
    with pytest.raises(BimocqError):
        s.setOption(MC.OPT_FUSED_MACCORMACK, 3)
    assert s.getOption(MC.OPT_FUSED_MACCORMACK) == 1
    s.close()


def test_python_names():
    from gpufluidsimulation_amd import solver
    assert (solver.SCHEME_BIMOCQ, solver.SCHEME_MACCORMACK, solver.SCHEME_MAC_REFLECTION) == (0, 2, 3)
    assert solver.OPT_FUSED_MACCORMACK == 15


def test_operator_standin_refuses_what_the_contract_refuses(standin):
    """the restatement the GPU tests compare against keeps the operator's refusals"""
    ni, nj, nk = 8, 8, 8
    h = 1.0 / ni
    u, v, w = F.velocity(ni, nj, nk, h)
    f = F.scalar(ni, nj, nk, 0.7)
    out = np.full_like(f, 7.0)
    p = lambda a: a.ctypes.data
    for args in ((p(f), p(f), p(f), p(f)), (p(out), p(out), p(f), p(f))):
        standin.gpu_maccormack(args[0], args[1], args[2], args[3], p(u), p(v), p(w), 0, 0, 0, h, ni, nj, nk, 0.1, 0.1, 0.1)
        assert standin.fl_last_error() == 3
        standin.fl_clear_error()
    standin.gpu_maccormack(p(out), p(f), p(f), p(f), p(u), p(v), p(w), 1, 1, 0, h, ni, nj, nk, 0.1, 0.1, 0.1)
    assert standin.fl_last_error() == 3
    standin.fl_clear_error()
    assert (out == 7.0).all()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_slabs(backend, fused, ref_path, nproc=2, threads=2):
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "maccormack_slab_worker.py"), "--backend", backend, "--fused", str(fused),
           "--reference", ref_path]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("[rank")]
    return r.returncode, "\n".join(lines[-30:]) or r.stdout[-3000:]


@pytest.mark.parametrize("fused", (1, 0))
def test_two_slab_ranks_equal_one_domain(tmp_path, fused):
    """scheme 2 on two z-slab ranks of 24 x 20 x 32 (6 ghost planes, dt of one cell, 12 Jacobi iterations): the stitched
    owned planes equal the single-domain stand-in run after each of 3 steps"""
    import maccormack_slab_worker as W
    ref = str(tmp_path / "ref.npz")
    W.reference("cpu", fused, ref)
    rc, out = launch_slabs("cpu", fused, ref)
    assert rc == 0, out
    assert out.count("mismatches=0") == 2
