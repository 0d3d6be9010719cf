"""One z-slab rank of the MacCormack parity tests (tests/test_maccormack_cpu.py, tests/test_gpu_maccormack.py), launched by
torch.distributed.run with the gloo backend.

    --backend cpu : the host solver on the CPU stand-in with gpu_maccormack (tests/build_cpu_maccormack.py)
    --backend gpu : the HIP kernels, all ranks sharing GPU 0, ghost planes through the host-staged transport

Scheme 2 with BQ_OPT_FUSED_MACCORMACK = --fused.  After every step the planes this rank owns must equal the single-domain
run of the same library, which the test recorded in the .npz given by --reference.  Exit code 0 = parity on this rank."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

DIMS, L, GHOST, STEPS, ITERS = (24, 20, 32), 0.75, 6, 3, 12
DT = 1.0 * (L / DIMS[0])                # one cell


def load(backend):
    """(host library, operator library) of a backend"""
    import maccormack_case as MC
    if backend == "cpu":
        lib = MC.load_maccormack()
        for name, res, args in (("fl_memcpy_d2h", None, [C.c_void_p, C.c_void_p, C.c_size_t]),
                                ("fl_memcpy_h2d", None, [C.c_void_p, C.c_void_p, C.c_size_t])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        return lib, lib
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return solver.host_lib(), hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--fused", type=int, required=True)
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    import fields as F
    import maccormack_case as MC
    from gpufluidsimulation_amd import solver, transport
    ref = np.load(a.reference)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.set_num_threads(1)
    hostlib, abilib = load(a.backend)
    tr = transport.HostStagedTransport(abilib, dist)
    s = solver.BimocqGPUSolver(*DIMS, L, 0.0, 1.0, lib=hostlib, errlib=abilib, rank=rank, nranks=world, ghost=GHOST, scheme=2)
    s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(DIMS, L))
    s.setProjection(ITERS, 0.5)
    s.setOption(MC.OPT_FUSED_MACCORMACK, a.fused)
    if a.backend == "cpu":
        abilib.maccormack_abi_calls(1)
    ni, nj, _ = DIMS
    plane = {"u": (ni + 1) * nj, "v": ni * (nj + 1)}
    bad = 0
    for f in range(STEPS):
        s.advance(f, DT)
        s._check()
        for nm in MC.NAMES:
            pe = plane.get(nm, ni * nj)
            mine = s.owned(nm)
            want = ref[f"{nm}{f}"][pe * s.own0: pe * s.own0 + mine.size]
            if not F.same(want, mine):
                d = np.abs(want.astype(np.float64) - mine.astype(np.float64))
                planes = sorted(set((np.nonzero(d)[0] // pe + s.own0).tolist()))
                print(f"[rank {rank}] step {f}: {nm} differs, max|diff| {d.max():.3e} in global planes {planes[:12]}", flush=True)
                bad += 1
    if a.backend == "cpu":
        calls = abilib.maccormack_abi_calls(0)
        if (calls > 0) != (a.fused >= 1):
            print(f"[rank {rank}] gpu_maccormack calls {calls} with BQ_OPT_FUSED_MACCORMACK = {a.fused}", flush=True)
            bad += 1
    print(f"[rank {rank}/{world}] steps={STEPS} fused={a.fused} exchanges={tr.exchanges} mismatches={bad}", flush=True)
    ok = torch.tensor([bad])
    dist.all_reduce(ok)
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if int(ok.item()) == 0 and tr.exchanges != 0 else 1)


def reference(backend, fused, path):
    """the single-domain run of `backend`, every step's fields saved as <name><step> in the .npz `path`"""
    import maccormack_case as MC
    hostlib, abilib = load(backend)
    out, _ = MC.run(hostlib, abilib, DIMS, L, STEPS, ITERS, DT, scheme=2, fused=fused)
    np.savez(path, **{f"{nm}{f}": out[f][nm] for f in range(STEPS) for nm in MC.NAMES})
    assert float(np.abs(out[-1]["v"]).max()) > 0.01
    return out


if __name__ == "__main__":
    main()
