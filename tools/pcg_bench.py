"""Cost of the converged fp64 PCG projection (BQ_PROJECTION_PCG): the rising-smoke scene of bench.py
at 256^3 (and 512^3 with --sizes 256,512), steps [warmup, warmup + steps), in four legs:
  pcg            no obstacle, kind 2 (tol 1e-6, at most 1000 updates)
  pcg_sphere     a static sphere of radius 0.15 L at the centre, kind 2
  jacobi_sphere  the same sphere, Jacobi 200 sweeps
  mgcg           no obstacle, kind 1 with 50 iterations (the reference GPU solver's default)
Per leg: step_ms (wall), projection_ms (BQ_OPT_PROFILE_PHASES), PCG iterations per projection (mean, max) and the
final max|r| / max|b| of the last projection.  Writes the JSON line to profiles/pcg_bench.json and prints it.
The kernel table comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--legs pcg_sphere).
Usage: python tools/pcg_bench.py [--sizes 256] [--steps 180] [--warmup 20] [--legs pcg,pcg_sphere,jacobi_sphere,mgcg]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpufluidsimulation_amd as bq                                  # noqa: E402
from gpufluidsimulation_amd.scenes import rising_smoke               # noqa: E402
from gpufluidsimulation_amd.solver import BimocqGPUSolver            # noqa: E402

LEGS = {"pcg": (2, 1000, False), "pcg_sphere": (2, 1000, True), "jacobi_sphere": (0, 200, True), "mgcg": (1, 50, False)}


def leg(n, name, args):
    kind, iters, sphere = LEGS[name]
    lib = bq.hip_lib()
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(iters, 0.5, kind=kind)
    if sphere:
        s.setBoundary([(0, 0.5, 0.5, 0.5, 0.15, 0.0, 0.0, 0.0, 0.0, 0.0)])
    dt = 2.0 * h
    for f in range(args.warmup):
        s.advance(f, dt)
    lib.fl_sync()
    s.setOption(8, 1)
    s.phaseMs(reset=True)
    its = []
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.steps):
        s.advance(f, dt)
        if kind == 2:
            its.append(s.pcgStats()["iterations"])          # (the solve is blocking: reading its stats adds no sync)
    lib.fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    phases, psteps = s.phaseMs(reset=True)
    bq.check()
    out = {"n": n, "leg": name, "kind": kind, "iters": iters, "sphere": sphere, "step_ms": round(wall, 3),
           "projection_ms": round(phases["projection"] / max(1, psteps), 3)}
    if kind == 2:
        st = s.pcgStats()
        out.update({"pcg_iters_mean": round(sum(its) / len(its), 2), "pcg_iters_max": max(its),
                    "final_rel_residual": st["max_r"] / st["max_b"] if st["max_b"] else 0.0,
                    "unconverged": st["unconverged"]})
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256")
    ap.add_argument("--steps", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_bench.json"))
    args = ap.parse_args()
    res = []
    for n in (int(x) for x in args.sizes.split(",")):
        for name in args.legs.split(","):
            res.append(leg(n, name, args))
            print(json.dumps(res[-1]), flush=True)
    line = json.dumps({"tool": "pcg_bench", "steps": args.steps, "warmup": args.warmup, "legs": res})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
