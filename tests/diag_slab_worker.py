"""One z-slab rank of the flow-diagnostics tests (tests/test_diagnostics_cpu.py, tests/test_gpu_diagnostics.py), launched by
torch.distributed.run with the gloo backend.

    --backend cpu : the host solver on the CPU stand-in with gpu_flow_stats (tests/build_cpu_diag.py)
    --backend gpu : the HIP kernels, all ranks sharing GPU 0; --transport host: ghost planes and all-reduces staged through
                    the host over gloo; --transport rccl: the library's own RCCL path, in-stream all-reduces included, which
                    on one GPU needs BQ_RCCL_LIBRARY = the tests' stand-in (tests/fake_rccl)

Scheme 2 on the grid of tests/maccormack_slab_worker.py, BQ_OPT_DIAGNOSTICS_EVERY = 2, four steps.  Then, on every rank:
diagnostics() lies within the summation bound (tests/diag_case.py) of the exact sums over the single-domain fields, which
the test recorded in the .npz given by --reference; the last history row equals diagnostics() bit for bit and the rows
carry steps 2 and 4; the owned planes of vorticity() equal the single-domain field bit for bit.  Exit code 0 = all of it
on every rank."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

DIMS, L, GHOST, STEPS, ITERS, EVERY = (24, 20, 32), 0.75, 6, 4, 12, 2
DT = 1.0 * (L / DIMS[0])                # one cell


def load(backend):
    """(host library, operator library) of a backend"""
    import diag_case as D
    if backend == "cpu":
        lib = D.load_diag()
        return lib, lib
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return solver.host_lib(), hip


def reference(backend, path):
    """the single-domain run of `backend`: the exact diagnostics row of its final fields (math.fsum over the restatement's
    terms), the bound a computed row must keep to it, and its vorticity field, saved in the .npz `path`; the
    single-domain solver's own diagnostics() is held to the same bound here"""
    import diag_case as D
    from gpufluidsimulation_amd import solver
    hostlib, abilib = load(backend)
    cpu = D.load_diag()
    out, taken, hist, vort = D.run_with_diagnostics(hostlib, abilib, DIMS, L, STEPS, ITERS, DT, scheme=2, every=EVERY, sample={STEPS})
    last = out[-1]
    h = float(np.float32(L) / np.float32(DIMS[0]))
    val, mass, n, mag = D.exact(cpu, last["u"], last["v"], last["w"], last["rho"], last["T"], h, DIMS)
    row, bound = D.diag_row(val, h, STEPS), D.row_bound(val, mass, n, h)
    got = taken[STEPS]
    for name in solver.DIAG_NAMES:
        assert abs(got[name] - row[name]) <= bound[name], (name, got[name], row[name], bound[name])
    assert np.array_equal(vort.ravel().view(np.uint32), mag.view(np.uint32))
    assert hist.shape == (STEPS // EVERY, solver.DIAG_COUNT) and row["kinetic"] > 0 and row["enstrophy"] > 0 and row["rho_sum"] > 1
    np.savez(path, row=np.array([row[k] for k in solver.DIAG_NAMES]), bound=np.array([bound[k] for k in solver.DIAG_NAMES]), vort=mag)
    return row, bound


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--transport", choices=["host", "rccl"], default="host")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    import maccormack_case as MC
    from gpufluidsimulation_amd import solver, transport
    ref = np.load(a.reference)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.set_num_threads(1)
    hostlib, abilib = load(a.backend)
    if a.transport == "rccl":
        assert a.backend == "gpu"
        transport.init_rccl(abilib, dist)
        assert abilib.fl_comm_size() == world and abilib.fl_comm_rank() == rank

        class _Stats:                               # the RCCL path keeps no Python-side counters
            exchanges = -1
        tr = _Stats()
    else:
        tr = transport.HostStagedTransport(abilib, dist)
    s = solver.BimocqGPUSolver(*DIMS, L, 0.0, 1.0, lib=hostlib, errlib=abilib, rank=rank, nranks=world, ghost=GHOST, scheme=2)
    if a.backend == "cpu":      # the restatement takes the slab context and the all-reduce the stand-in keeps to itself
        abilib.flow_stats_abi_set_slab(s.own0 - s.ghost, DIMS[2], s.own0, s.own1)
        abilib.flow_stats_abi_set_allreduce(C.cast(tr._ar, C.c_void_p), world)
    s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(DIMS, L))
    s.setProjection(ITERS, 0.5)
    s.setOption(solver.OPT_DIAGNOSTICS_EVERY, EVERY)
    for f in range(STEPS):
        s.advance(f, DT)
        s._check()
    bad = 0
    got = s.diagnostics()
    for a_, name in enumerate(solver.DIAG_NAMES):
        err = abs(got[name] - float(ref["row"][a_]))
        print(f"[rank {rank}] {name}: {got[name]!r} exact {float(ref['row'][a_])!r} |diff| {err:.3e} bound {float(ref['bound'][a_]):.3e}", flush=True)
        if not err <= float(ref["bound"][a_]):
            bad += 1
    hist = s.diagnosticsHistory()
    if hist.shape != (STEPS // EVERY, solver.DIAG_COUNT) or hist[:, -1].tolist() != [2.0, 4.0]:
        print(f"[rank {rank}] history rows {hist.shape}, steps {hist[:, -1].tolist()}", flush=True)
        bad += 1
    elif hist[-1].view(np.uint64).tolist() != np.array([got[k] for k in solver.DIAG_NAMES], dtype=np.float64).view(np.uint64).tolist():
        print(f"[rank {rank}] the last history row differs from diagnostics()", flush=True)
        bad += 1
    plane = DIMS[0] * DIMS[1]
    mine = s.vorticity().ravel()[plane * s.ghost: plane * (s.ghost + s.own1 - s.own0)]
    want = ref["vort"][plane * s.own0: plane * s.own1]
    if not np.array_equal(mine.view(np.uint32), want.view(np.uint32)):
        print(f"[rank {rank}] vorticity differs on the owned planes, max|diff| {np.abs(mine - want).max():.3e}", flush=True)
        bad += 1
    s._check()
    print(f"[rank {rank}/{world}] steps={STEPS} exchanges={tr.exchanges} mismatches={bad}", flush=True)
    ok = torch.tensor([bad])
    dist.all_reduce(ok)
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if int(ok.item()) == 0 and tr.exchanges != 0 else 1)


if __name__ == "__main__":
    main()
