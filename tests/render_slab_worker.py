"""One z-slab rank of the density-preview tests (tests/test_render_cpu.py, tests/test_gpu_render.py), launched by
torch.distributed.run with the gloo backend.

    --backend cpu : the host solver on the CPU stand-in with gpu_render_density (tests/build_cpu_render.py)
    --backend gpu : the HIP kernels, all ranks sharing GPU 0; --transport host: ghost planes and all-reduces staged through
                    the host over gloo; --transport rccl: the library's own RCCL path, in-stream all-reduces included, which
                    on one GPU needs BQ_RCCL_LIBRARY = the tests' stand-in (tests/fake_rccl)

Scheme 2, four steps, on the grid of tests/diag_slab_worker.py, or on --dims: the stand-in for librccl reduces at most 4096
bytes per call, so the GPU test runs 16^3, whose gather (2 x 16 x 16 doubles) and images (2 x 16 x 16) just fit.  Then, on every rank: render() for all six views with the
lights -y and +z (one crosses no rank boundary, the other does) must equal the single-domain images bit for bit -- the
test recorded them in the .npz given by --reference --, and rank 0 alone writes the preview file.  Exit code 0 = all of it
on every rank."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

DIMS, L, GHOST, STEPS, ITERS = (24, 20, 32), 0.75, 6, 4, 12
SIGMA, ALBEDO, AMBIENT = 24.0, 1.0, 0.125
LIGHTS = ("-y", "+z")


def load(backend):
    """(host library, operator library) of a backend"""
    import render_case as R
    if backend == "cpu":
        lib = R.load_render()
        return lib, lib
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver
    hip = bq.hip_lib()
    assert hip.fl_init(0) == 0
    return solver.host_lib(), hip


def keys():
    import render_case as R
    return [(v, l) for v in R.DIRS for l in LIGHTS]


def reference(backend, path, dims=DIMS):
    """the single-domain run of `backend`: its twelve images, checked against the restatement applied to its density and
    converted as the header says, saved in the .npz `path`"""
    import maccormack_case as MC
    import render_case as R
    from gpufluidsimulation_amd import solver
    hostlib, abilib = load(backend)
    cpu = R.load_render()
    s = solver.BimocqGPUSolver(*dims, L, 0.0, 1.0, lib=hostlib, errlib=abilib, scheme=2)
    s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(dims, L))
    s.setProjection(ITERS, 0.5)
    for f in range(STEPS):
        s.advance(f, L / dims[0])               # one cell
    rho = s.field("rho")
    h = float(np.float32(L) / np.float32(dims[0]))
    out = {}
    for v, l in keys():
        rad, tr = s.render(v, l, SIGMA, ALBEDO, AMBIENT)
        rc, img, _ = R.restate(cpu, rho, dims, h, solver.DIRECTIONS[v], solver.DIRECTIONS[l], SIGMA, ALBEDO, AMBIENT)
        want_rad, want_tr = R.convert(cpu.orc_expf, img)
        assert rc == 0 and np.array_equal(rad.view(np.uint32), want_rad.view(np.uint32)), (v, l)
        assert np.array_equal(tr.view(np.uint32), want_tr.view(np.uint32)), (v, l)
        assert rad.max() > 0 and tr.min() < 1
        out[f"rad{v}{l}"], out[f"tr{v}{l}"] = rad, tr
    s._check()
    s.close()
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["cpu", "gpu"], required=True)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--transport", choices=["host", "rccl"], default="host")
    ap.add_argument("--dims", type=int, nargs=3, default=list(DIMS))
    a = ap.parse_args()

    import torch
    import torch.distributed as dist

    import maccormack_case as MC
    import render_case as R
    from gpufluidsimulation_amd import solver, transport
    ref = np.load(a.reference)
    dims = tuple(a.dims)
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
        tr_ = _Stats()
    else:
        tr_ = transport.HostStagedTransport(abilib, dist)
    s = solver.BimocqGPUSolver(*dims, L, 0.0, 1.0, lib=hostlib, errlib=abilib, rank=rank, nranks=world, ghost=GHOST, scheme=2)
    if a.backend == "cpu":      # the restatement takes the slab context and the all-reduce the stand-in keeps to itself
        abilib.render_abi_set_slab(s.own0 - s.ghost, dims[2], s.own0, s.own1)
        abilib.render_abi_set_allreduce(C.cast(tr_._ar, C.c_void_p), world, rank)
    s.setSmoke(MC.DROP, MC.RISE, MC.emitters_for(dims, L))
    s.setProjection(ITERS, 0.5)
    for f in range(STEPS):
        s.advance(f, L / dims[0])
        s._check()
    bad = 0
    for v, l in keys():
        rad, tr = s.render(v, l, SIGMA, ALBEDO, AMBIENT)
        for name, got in (("rad", rad), ("tr", tr)):
            want = ref[f"{name}{v}{l}"]
            if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                diff = np.abs(got - want).max() if got.shape == want.shape else -1.0
                print(f"[rank {rank}] view {v} light {l}: {name} differs from the single domain's, max|diff| {diff:.3e}", flush=True)
                bad += 1
    n = s.outputPreview(STEPS - 1, a.outdir, "+z", "-y", SIGMA, ALBEDO, AMBIENT, 0.25)
    if (n > 0) != (rank == 0):
        print(f"[rank {rank}] outputPreview returned {n}", flush=True)
        bad += 1
    s._check()
    dist.barrier()
    files = sorted(os.listdir(a.outdir))
    if files != [f"preview_{STEPS:04d}.pgm"]:
        print(f"[rank {rank}] files {files}", flush=True)
        bad += 1
    else:
        w, h, px = R.pgm(os.path.join(a.outdir, files[0]))
        if not np.array_equal(px, R.pgm_pixels(ref["rad+z-y"], ref["tr+z-y"], 0.25)):
            print(f"[rank {rank}] the preview file's pixels differ from the formula", flush=True)
            bad += 1
    print(f"[rank {rank}/{world}] steps={STEPS} exchanges={tr_.exchanges} mismatches={bad}", flush=True)
    ok = torch.tensor([bad])
    dist.all_reduce(ok)
    s.close()
    dist.destroy_process_group()
    sys.exit(0 if int(ok.item()) == 0 and tr_.exchanges != 0 else 1)


if __name__ == "__main__":
    main()
