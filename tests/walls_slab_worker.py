"""One z-slab rank of the walled parity tests (tests/test_walls_slab_cpu.py, tests/test_gpu_walls_slab.py), launched by
torch.distributed.run with the gloo backend.

    --backend cpu : the host solver on the CPU stand-in of tests/build_cpu_walls_slab.py
    --backend gpu : the HIP kernels, all ranks sharing GPU 0, ghost planes through the host-staged transport

After every step the planes this rank owns must equal the one-domain walled run of the same library, which the test recorded
in the .npz given by --reference.  --walls-off-again: the walls are set and removed before the first step (the reference is
then the one-domain run without walls).  Exit code 0 = parity on this rank."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--dims", type=int, nargs=3, required=True)
    ap.add_argument("--ghost", type=int, default=6)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--scheme", type=int, default=0)
    ap.add_argument("--walls", type=int, required=True)
    ap.add_argument("--walls-off-again", type=int, default=0)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--overlap", type=int, default=1, help="BQ_OPT_OVERLAP_EXCHANGES")
    ap.add_argument("--ends-first", type=int, default=1, help="BQ_OPT_JACOBI_ENDS_FIRST (2: walled chunks too)")
    ap.add_argument("--triples", type=int, default=1, help="BQ_OPT_JACOBI_TRIPLES")
    ap.add_argument("--walled-triples", type=int, default=1, help="cpu backend: 0 = the stand-in refuses the walled triple")
    ap.add_argument("--jacobi-log", default=None, help="cpu backend: the stand-in's log of the projections' launches; {rank} = the rank")
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    import fields as F
    import walls_slab_case as WS
    from gpufluidsimulation_amd import transport
    ref = np.load(a.reference)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.set_num_threads(1)
    hostlib, abilib = WS.load(a.backend)
    if a.backend == "cpu":
        abilib.abi_walled_triples(a.walled_triples)
        if a.jacobi_log:
            abilib.abi_jacobi_log(a.jacobi_log.format(rank=rank).encode())
    tr = transport.HostStagedTransport(abilib, dist)
    dims = tuple(a.dims)
    s = WS.make(hostlib, abilib, dims, a.iters, a.scheme, a.walls, rank=rank, nranks=world, ghost=a.ghost)
    assert s.walls() == a.walls
    if a.walls_off_again:
        s.setWalls(0)
        assert s.walls() == 0
    s.setOption(5, a.overlap)
    s.setOption(7, a.ends_first)
    s.setOption(10, a.triples)
    ni, nj, _ = dims
    plane = {"u": (ni + 1) * nj, "v": ni * (nj + 1)}
    bad = 0
    for f in range(a.steps):
        s.advance(f, WS.DT_CELLS * WS.L / ni)
        s._check()
        for nm in WS.NAMES:
            pe = plane.get(nm, ni * nj)
            mine = s.owned(nm)
            want = ref[f"{nm}{f}"][pe * s.own0: pe * s.own0 + mine.size]
            if not F.same(want, mine):
                d = np.abs(want.astype(np.float64) - mine.astype(np.float64))
                planes = sorted(set((np.nonzero(d)[0] // pe + s.own0).tolist()))
                print(f"[rank {rank}] step {f}: {nm} differs, max|diff| {d.max():.3e} in global planes {planes[:12]}", flush=True)
                bad += 1
    if a.backend == "cpu" and a.jacobi_log:
        abilib.abi_jacobi_log(None)
    print(f"[rank {rank}/{world}] walls={a.walls} scheme={a.scheme} steps={a.steps} exchanges={tr.exchanges} mismatches={bad}", flush=True)
    ok = torch.tensor([bad])
    dist.all_reduce(ok)
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if int(ok.item()) == 0 and tr.exchanges != 0 else 1)


if __name__ == "__main__":
    main()
