"""Shared pieces of the tests of closed walls on z-slab ranks: the loader of the CPU stand-in whose
wall operators honour the slab context (tests/build_cpu_walls_slab.py), the scene, the one-domain reference run and the
launcher of tests/walls_slab_worker.py."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, BLEND, DT_CELLS = 0.75, 0.8, 1.0
NAMES = ("rho", "T", "u", "v", "w", "p")
BOX, ZLO = 55, 16
RANGE_OPS = ("gpu_jacobi_sweep_masked_walls_range", "gpu_jacobi_sweep_masked_walls_triple_ranges")


def load(backend):
    """(host library, operator library) of a backend"""
    from gpufluidsimulation_amd import solver
    if backend == "cpu":
        import obstacle_case as OC
        import pcg_case as PC
        import walls_case as WC
        from build_cpu_walls_slab import build_walls_slab
        lib = OC._load(build_walls_slab(), OC.OPS + OC.LS_OPS + PC.PCG_OPS + WC.WALL_OPS + RANGE_OPS)
        for name, res, args in (("fl_memcpy_d2h", None, [C.c_void_p, C.c_void_p, C.c_size_t]),
                                ("fl_memcpy_h2d", None, [C.c_void_p, C.c_void_p, C.c_size_t]),
                                ("fl_set_option", None, [C.c_int, C.c_int]), ("fl_get_option", C.c_int, [C.c_int]),
                                ("fl_set_slab", None, [C.c_int] * 5),
                                ("abi_jacobi_log", None, [C.c_char_p]), ("abi_walled_triples", None, [C.c_int])):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        return lib, lib
    import gpufluidsimulation_amd as bq
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return solver.host_lib(), hip


def emitters(dims, nranks=2):
    """two sources: one straddling the middle of the grid along z, one low in the first rank's slab next to the z-low wall
    (centres between the nodes: a node on a centre would get 0/0 from the emitter's direction normalisation)"""
    ni, nj, nk = dims
    h = L / ni
    return [(0.5 * ni * h, 0.3 * nj * h, 0.5 * nk * h + 0.3 * h, 0.16 * ni * h, 1.0, 2.0, 0.0, 2),
            (0.4 * ni * h + 0.37 * h, 0.35 * nj * h, 0.16 * nk * h + 0.41 * h, 0.12 * ni * h, 0.7, 1.0, 0.0, 1)]


def make(hostlib, abilib, dims, iters, scheme, walls, **slab):
    from gpufluidsimulation_amd import solver
    s = solver.BimocqGPUSolver(*dims, L, 0.0, BLEND, lib=hostlib, errlib=abilib, scheme=scheme, **slab)
    s.setSmoke(0.05, 1.0, emitters(dims))
    s.setProjection(iters, 0.5)
    if walls:
        s.setWalls(walls)
    return s


def reference(hostlib, abilib, dims, iters, scheme, walls, steps, path):
    """the one-domain run, every step's fields saved as <name><step> in the .npz `path`"""
    s = make(hostlib, abilib, dims, iters, scheme, walls)
    out = {}
    for f in range(steps):
        s.advance(f, DT_CELLS * L / dims[0])
        s._check()
        for nm in NAMES:
            out[f"{nm}{f}"] = s.field(nm).copy()
    s.close()
    vmax = float(np.abs(out[f"v{steps - 1}"]).max())
    assert np.isfinite(vmax) and vmax > 0.0                     # the smoke rises
    np.savez(path, **out)
    return out


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(nproc, *args, threads=2, timeout=300):
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "walls_slab_worker.py"), *map(str, args)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("[rank")]
    return r.returncode, "\n".join(lines[-30:]) or r.stdout[-3000:]
