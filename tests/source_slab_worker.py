"""One z-slab rank of the source parity test (tests/test_gpu_sources.py): the HIP kernels, all ranks sharing GPU 0, ghost
planes through the host-staged transport.  The plume scene (scenes.plume, its source drifting along +z across the slab
boundary, beside a static sphere source without velocity), BiMocq scheme, no obstacle.  After every step the planes this
rank owns must equal the one-GPU run's, which the test recorded in the .npz given as the only argument.  RANK, WORLD_SIZE,
MASTER_ADDR and MASTER_PORT come from the environment.  Exit code 0 = parity on this rank."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

DIMS, L, GHOST, STEPS, ITERS, BLEND = (32, 32, 96), 1.0, 6, 5, 30, 0.8
H = L / DIMS[0]
DT = 1.5 * H
FIELDS = ("rho", "T", "u", "v", "w", "p")


def make_solver(hostlib, errlib, rank=0, nranks=1, ghost=0):
    from gpufluidsimulation_amd import scenes, solver
    s = solver.BimocqGPUSolver(*DIMS, L, 0.0, BLEND, lib=hostlib, errlib=errlib, rank=rank, nranks=nranks, ghost=ghost)
    s.setSmoke(0.05, 1.0, [])
    s.setProjection(ITERS, 0.5)
    sources = scenes.plume(DIMS[2], H)
    sources[0].motion = (0.0, 0.0, 0.4)
    sources.append(solver.Source(("sphere", 0.1), (0.35, 0.4, 0.5 * DIMS[2] * H - 0.12), 0.5, 0.5, 3))
    s.setSources(sources)
    return s


def main():
    import torch
    import torch.distributed as dist

    import fields as F
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver, transport
    ref = np.load(sys.argv[1])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.set_num_threads(1)
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    tr = transport.HostStagedTransport(hip, dist)
    s = make_solver(solver.host_lib(), hip, rank, world, GHOST)
    ni, nj, _ = DIMS
    plane = {"u": (ni + 1) * nj, "v": ni * (nj + 1)}
    bad = 0
    for f in range(STEPS):
        s.advance(f, DT)
        s._check()
        for nm in FIELDS:
            pe = plane.get(nm, ni * nj)
            mine = s.owned(nm)
            want = ref[f"{nm}{f}"][pe * s.own0: pe * s.own0 + mine.size]
            if not F.same(want, mine):
                d = np.abs(want.astype(np.float64) - mine.astype(np.float64))
                planes = sorted(set((np.nonzero(d)[0] // pe + s.own0).tolist()))
                print(f"[rank {rank}] step {f}: {nm} differs, max|diff| {d.max():.3e} in global planes {planes[:12]}", flush=True)
                bad += 1
    print(f"[rank {rank}/{world}] steps={STEPS} exchanges={tr.exchanges} mismatches={bad}", flush=True)
    ok = torch.tensor([bad])
    dist.all_reduce(ok)
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if int(ok.item()) == 0 and tr.exchanges != 0 else 1)


if __name__ == "__main__":
    main()
