"""Cost of a level-set obstacle on the GPU step: the rising-smoke scene of bench.py at 256^3 with no obstacle, with the
analytic sphere of tools/obstacle_bench.py (radius 0.15 L at the centre), with the same sphere as levelset_sphere(r, h),
and with that level-set sphere moving (updateBoundary every frame).  Writes profiles/levelset_bench.json and prints it:
  step_ms          mean step time over steps [warmup, warmup + steps) (bench.py's extra.survey_metric window: 20-200),
                   updateBoundary included
  phase_ms         the step's phases per step (BQ_OPT_PROFILE_PHASES), over the same window
  rebuild_ms       one updateBoundary (flags + rows summary rebuild), mean of 50 calls with dt = 0 after the window
Usage: python tools/levelset_bench.py [--n 256] [--steps 180] [--warmup 20] [--jacobi-iters 200] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpufluidsimulation_amd as bq                                  # noqa: E402
from gpufluidsimulation_amd.scenes import rising_smoke               # noqa: E402
from gpufluidsimulation_amd.solver import (BimocqGPUSolver, LevelSetObstacle,  # noqa: E402
                                           levelset_sphere)

R, CENTRE = 0.15, (0.5, 0.5, 0.5)


def leg(name, args):
    lib = bq.hip_lib()
    n = args.n
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(args.jacobi_iters, 0.5)
    if name == "analytic":
        s.setBoundary([(0, *CENTRE, R, 0.0, 0.0, 0.0, 0.0, 0.0)])
    elif name in ("levelset", "levelset_moving"):
        vel = (0.1, 0.0, 0.0) if name == "levelset_moving" else (0.0, 0.0, 0.0)
        s.setBoundary([LevelSetObstacle(levelset_sphere(R, h), CENTRE, vel)])
    dt = 2.0 * h
    for f in range(args.warmup):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    lib.fl_sync()
    s.setOption(8, 1)
    s.phaseMs(reset=True)
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.steps):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    lib.fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    phases, psteps = s.phaseMs(reset=True)
    rebuild = None
    if name != "none":
        lib.fl_sync()
        t0 = time.perf_counter()
        for f in range(50):
            s.updateBoundary(f, 0.0)
        lib.fl_sync()
        rebuild = round((time.perf_counter() - t0) * 1e3 / 50, 4)
    bq.check()
    out = {"case": name, "n": n, "step_ms": round(wall, 3),
           "phase_ms": {k: round(v / max(1, psteps), 3) for k, v in phases.items()},
           "rebuild_ms": rebuild, "solid_cells": int(s.solidMask().sum())}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levelset_bench.json"))
    args = ap.parse_args()
    legs = []
    for name in ("none", "analytic", "levelset", "levelset_moving"):
        legs.append(leg(name, args))
        print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {g["case"]: g for g in legs}
    ratios = {k: round(by[k]["step_ms"] / by["analytic"]["step_ms"], 3) for k in ("levelset", "levelset_moving")}
    result = {"tool": "levelset_bench", "jacobi_iters": args.jacobi_iters, "window": [args.warmup, args.warmup + args.steps],
              "legs": legs, "step_over_analytic": ratios,
              "budget": {"step_over_analytic": 1.05, "rebuild_ms": 0.2},
              "met": {"step": all(r <= 1.05 for r in ratios.values()),
                      "rebuild": all(by[k]["rebuild_ms"] <= 0.2 for k in ("levelset", "levelset_moving"))}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
