"""Cost of closed domain walls on the GPU step: the rising-smoke scene of bench.py at 256^3, 200
Jacobi iterations, steps 20-200, library defaults -- the setup of tools/obstacle_bench.py.  Legs:
  A  no walls (the path without this feature)
  B  the reference's container (walls closed but +y): positional path
  C  the same walls through flags only, at operator level: gpu_jacobi_sweeps_masked on solid + walls with every row of the
     rows summary marked dirty, against gpu_jacobi_sweeps_masked_walls on the same arrays, three alternating runs each
  D  the container + the sphere of section 14 (radius 0.15 L at the centre)
  E  BQ_PROJECTION_PCG in the container: iterations, final max|r| / max|b| and stop reason of every projection
  S  one GPU playing ONE z-slab rank of 4 (64 owned + 2 x 8 ghost planes) with a transport that moves nothing, as
     bench.py --emulate-slab does: a middle rank (x and y walls only) and rank 0 (the z-low wall too) in the container with the
     walled plan's ends-first order on and off, next to the unwalled emulated middle rank; three alternating runs each:
     projection ms per step and projection us per sweep (the range launches are not inside the sweep loops' event pairs)
A, B, D: step ms, projection ms, us per sweep launch.  Writes profiles/walls_bench.json and prints the same JSON line.
Usage: python tools/walls_bench.py [--n 256] [--steps 180] [--warmup 20] [--jacobi-iters 200] [--pcg-steps 20] [--slab-steps 30] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpufluidsimulation_amd as bq                                  # noqa: E402
from gpufluidsimulation_amd import _lib                              # noqa: E402
from gpufluidsimulation_amd.scenes import rising_smoke               # noqa: E402
from gpufluidsimulation_amd.solver import WALLS_REFERENCE_BOX, BimocqGPUSolver   # noqa: E402

SPHERE = (0, 0.5, 0.5, 0.5, 0.15, 0.0, 0.0, 0.0, 0.0, 0.0)


def step_leg(name, n, walls, obstacle, args):
    lib = bq.hip_lib()
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(args.jacobi_iters, 0.5)
    if obstacle:
        s.setBoundary([SPHERE])
    s.setWalls(walls)
    dt = 2.0 * h
    for f in range(args.warmup):
        s.advance(f, dt)
    lib.fl_sync()
    s.setOption(8, 1)
    s.phaseMs(reset=True)
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 1)
    ms, launches, sweeps = C.c_double(), C.c_longlong(), C.c_longlong()
    lib.fl_jacobi_profile(C.byref(ms), C.byref(launches), C.byref(sweeps))      # reset
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.steps):
        s.advance(f, dt)
    lib.fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    phases, psteps = s.phaseMs(reset=True)
    lib.fl_jacobi_profile(C.byref(ms), C.byref(launches), C.byref(sweeps))
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 0)
    bq.check()
    rho = s.field("rho")
    out = {"leg": name, "n": n, "walls": walls, "obstacle": obstacle, "step_ms": round(wall, 3),
           "projection_ms": round(phases["projection"] / max(1, psteps), 3),
           "launch_us": round(ms.value * 1e3 / max(1, launches.value), 2), "sweep_us": round(ms.value * 1e3 / max(1, sweeps.value), 2),
           "sweep_launches_per_step": round(launches.value / args.steps, 1), "kernel": lib.fl_jacobi_kernel_name().decode(),
           "rho_finite": bool(np.isfinite(rho).all())}
    s.close()
    return out


def operator_legs(n, walls, sweeps, runs=3):
    """B against C on the same arrays: launch us of the positional path and of the all-flags path, alternating"""
    lib = bq.hip_lib()
    cells = n * n * n
    solidw = np.zeros((n, n, n), np.uint8)
    for bit, sl in ((1, (slice(None), slice(None), 0)), (2, (slice(None), slice(None), -1)), (4, (slice(None), 0)),
                    (8, (slice(None), -1)), (16, (0,)), (32, (-1,))):
        if walls & bit:
            solidw[sl] = 0x80
    rng = np.random.default_rng(1)
    div = rng.standard_normal((n, n, n)).astype(np.float32)
    bufs = {}
    for name, a in (("solidw", solidw), ("clean", np.zeros((n, n), np.uint8)), ("dirty", np.ones((n, n), np.uint8)), ("div", div),
                    ("p", np.zeros(cells, np.float32)), ("t", np.zeros(cells, np.float32))):
        a = np.ascontiguousarray(a)
        bufs[name] = lib.fl_malloc(a.nbytes)
        lib.fl_memcpy_h2d(bufs[name], a.ctypes.data, a.nbytes)
    was = lib.fl_get_option(_lib.FL_OPT_JACOBI_FUSE)
    lib.fl_set_option(_lib.FL_OPT_JACOBI_FUSE, 2)
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 1)
    ms, nl, ns = C.c_double(), C.c_longlong(), C.c_longlong()
    res = {"B": [], "C": []}

    def run(which):
        lib.fl_memset(bufs["p"], 0, cells * 4)
        lib.fl_memset(bufs["t"], 0, cells * 4)
        lib.fl_jacobi_profile(C.byref(ms), C.byref(nl), C.byref(ns))
        if which == "B":
            lib.gpu_jacobi_sweeps_masked_walls(bufs["p"], bufs["div"], bufs["t"], bufs["solidw"], bufs["clean"], walls, n, n, n, sweeps, -1.0, 1.0 / 6.0)
        else:
            lib.gpu_jacobi_sweeps_masked(bufs["p"], bufs["div"], bufs["t"], bufs["solidw"], bufs["dirty"], n, n, n, sweeps, -1.0, 1.0 / 6.0)
        lib.fl_sync()
        lib.fl_jacobi_profile(C.byref(ms), C.byref(nl), C.byref(ns))
        return ms.value * 1e3 / max(1, nl.value)

    run("B"); run("C")                              # warm-up
    for _ in range(runs):
        res["B"].append(round(run("B"), 2))
        res["C"].append(round(run("C"), 2))
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 0)
    lib.fl_set_option(_lib.FL_OPT_JACOBI_FUSE, was)
    bq.check()
    for p in bufs.values():
        lib.fl_free(p)
    return {"leg": "B vs C (operator level)", "n": n, "sweeps": sweeps, "launch_us_B": res["B"], "launch_us_C": res["C"],
            "B_faster_beyond_spread": max(res["B"]) < min(res["C"])}


def slab_legs(n, walls, args, runs=3, nranks=4, ghost=8):
    """the emulated slab ranks, alternating: {name: [projection ms per step, ...]} and the same as us per sweep"""
    from gpufluidsimulation_amd import transport
    lib = bq.hip_lib()
    h = 1.0 / n
    # BQ_OPT_JACOBI_ENDS_FIRST: 2 = the walled chunks too, 1 (the default) = walled chunks in the plain order
    cases = (("unwalled middle rank", 0, nranks // 2, 1), ("walled middle rank, ends first", walls, nranks // 2, 2),
             ("walled middle rank, plain order", walls, nranks // 2, 1), ("walled rank 0, ends first", walls, 0, 2),
             ("walled rank 0, plain order", walls, 0, 1))

    def run(w, rank, ends_first):
        keep = transport.NullTransport(lib, rank, nranks)
        s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0, rank=rank, nranks=nranks, ghost=ghost)
        s.setSmoke(0.0, 1.0, rising_smoke(n, h))
        s.setProjection(args.jacobi_iters, 0.5)
        s.setWalls(w)
        s.setOption(7, ends_first)
        for f in range(5):
            s.advance(f, 2.0 * h)
        lib.fl_sync()
        s.setOption(8, 1)
        s.phaseMs(reset=True)
        for f in range(5, 5 + args.slab_steps):
            s.advance(f, 2.0 * h)
        lib.fl_sync()
        phases, psteps = s.phaseMs(reset=True)
        bq.check()
        s.close()
        del keep
        return phases["projection"] / max(1, psteps)
    res = {name: [] for name, *_ in cases}
    for _ in range(runs):
        for name, w, rank, ef in cases:
            res[name].append(round(run(w, rank, ef), 3))
    sweeps = max(1, args.jacobi_iters - 1)
    return {"leg": "S (emulated slab rank of %d, %d owned + 2 x %d ghost planes)" % (nranks, n // nranks, ghost), "n": n, "walls": walls,
            "steps": args.slab_steps, "projection_ms": res,
            "projection_us_per_sweep": {k: [round(v * 1e3 / sweeps, 2) for v in vs] for k, vs in res.items()}}


def pcg_leg(n, walls, args):
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(1000, 0.5, kind=2)
    s.setWalls(walls)
    stats = []
    t0 = time.perf_counter()
    for f in range(args.pcg_steps):
        s.advance(f, 2.0 * h)
        st = s.pcgStats()
        stats.append({"iterations": st["iterations"], "rel": st["max_r"] / st["max_b"] if st["max_b"] else 0.0, "stop": st["stop"]})
    bq.hip_lib().fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / max(1, args.pcg_steps)
    bq.check()
    s.close()
    return {"leg": "E", "n": n, "walls": walls, "steps": args.pcg_steps, "step_ms": round(wall, 2),
            "iterations": [x["iterations"] for x in stats], "final_rel_residual": [float(f"{x['rel']:.3g}") for x in stats],
            "stops": sorted({x["stop"] for x in stats})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--pcg-steps", type=int, default=20)
    ap.add_argument("--slab-steps", type=int, default=30, help="timed steps of each run of the emulated slab ranks (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walls_bench.json"))
    args = ap.parse_args()
    box = WALLS_REFERENCE_BOX
    legs = []
    for name, walls, obstacle in (("A", 0, False), ("B", box, False), ("D", box, True)):
        legs.append(step_leg(name, args.n, walls, obstacle, args))
        print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    legs.append(operator_legs(args.n, box, args.jacobi_iters - 1))
    print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    if args.pcg_steps > 0:
        legs.append(pcg_leg(args.n, box, args))
        print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    if args.slab_steps > 0:
        legs.append(slab_legs(args.n, box, args))
        print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    a, b = legs[0], legs[1]
    out = {"tool": "walls_bench", "jacobi_iters": args.jacobi_iters, "window": [args.warmup, args.warmup + args.steps], "legs": legs,
           "B_over_A": {"step": round(b["step_ms"] / a["step_ms"], 3), "projection": round(b["projection_ms"] / a["projection_ms"], 3),
                        "sweep_us": round(b["sweep_us"] / a["sweep_us"], 3)}}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
