"""Cost of a solid obstacle on the GPU step: the rising-smoke scene of bench.py at 256^3 and 512^3, without and with a
static sphere of radius 0.15 L at the centre of the domain.  Prints one JSON line:
  step_ms             mean step time over steps [warmup, warmup + steps) (bench.py's extra.survey_metric window: 20-200)
  projection_ms       the projection phase per step (BQ_OPT_PROFILE_PHASES), over the same window
  sweep_us            Jacobi time per sweep (FL_OPT_PROFILE_JACOBI: gpu_jacobi_sweeps, or the masked sweeps with the obstacle)
  sweep_launches      sweep-kernel launches per step (both paths fuse three sweeps per launch)
  sweep_frac_peak     compulsory bytes per launch (12 B per cell: read p and div once, write p once; 13 B with the flag
                      byte) x launches / sweep-loop time / 8 TB/s -- bench.py's roofline convention
  masked_block_frac   fraction of the fused sweep's blocks that take the masked path (the rest run the unmasked stream)
Usage: python tools/obstacle_bench.py [--sizes 256,512] [--steps 180] [--warmup 20] [--jacobi-iters 200]"""
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
from gpufluidsimulation_amd.solver import BimocqGPUSolver            # noqa: E402

HBM_PEAK = 8.0e12


def masked_block_fraction(mask, ncus=256):
    """fraction of the blocks of the fused masked sweep (jacobi_lds_kernel<8, 1, 3, true>: 8 output rows, chunks of planes
    sized to fill the CUs once, bq_project.hip jacobi_sweep_lds) that find a solid cell within three cells of their outputs
    and take the masked path -- the kernel's own block test, restated on the downloaded flags"""
    nk, nj, ni = mask.shape
    rowsolid = (mask != 0).any(axis=2)
    pad = np.pad(rowsolid, 1)
    rows = np.zeros((nk, nj), bool)
    for c in range(3):
        for b in range(3):
            rows |= pad[c:c + nk, b:b + nj]
    nby = (nj + 7) // 8
    kc = max(2, (nk + max(1, ncus // nby) - 1) // max(1, ncus // nby))
    dirty = total = 0
    for bz in range((nk + kc - 1) // kc):
        kbeg, kend = max(1, bz * kc), min(nk - 1, (bz + 1) * kc)
        if kbeg >= kend:
            continue
        for by in range(nby):
            jb = 8 * by
            total += 1
            dirty += bool(rows[max(kbeg - 3, 0):min(kend + 3, nk), max(jb - 3, 0):min(jb + 11, nj)].any())
    return dirty / max(1, total)


def leg(n, obstacle, args):
    lib = bq.hip_lib()
    h = 1.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, h))
    s.setProjection(args.jacobi_iters, 0.5)
    if obstacle:
        s.setBoundary([(0, 0.5, 0.5, 0.5, 0.15, 0.0, 0.0, 0.0, 0.0, 0.0)])
    dt = 2.0 * h
    for f in range(args.warmup):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    lib.fl_sync()
    s.setOption(8, 1)
    s.phaseMs(reset=True)
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 1)
    ms, launches, sweeps = C.c_double(), C.c_longlong(), C.c_longlong()
    lib.fl_jacobi_profile(C.byref(ms), C.byref(launches), C.byref(sweeps))      # reset
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.steps):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    lib.fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    phases, psteps = s.phaseMs(reset=True)
    lib.fl_jacobi_profile(C.byref(ms), C.byref(launches), C.byref(sweeps))
    lib.fl_set_option(_lib.FL_OPT_PROFILE_JACOBI, 0)
    bq.check()
    sweep_us = ms.value * 1e3 / max(1, sweeps.value)
    cells = float(n) ** 3
    bytes_moved = (13.0 if obstacle else 12.0) * cells * launches.value
    frac = masked_block_fraction(s.solidMask()) if obstacle else 0.0
    out = {"n": n, "obstacle": obstacle, "step_ms": round(wall, 3),
           "projection_ms": round(phases["projection"] / max(1, psteps), 3),
           "sweep_us": round(sweep_us, 2), "sweep_launches": round(launches.value / args.steps, 1),
           "sweep_frac_peak": round(bytes_moved / (ms.value * 1e-3) / HBM_PEAK, 3),
           "masked_block_frac": round(frac, 4), "solid_cells": int(s.solidMask().sum()) if obstacle else 0}
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--steps", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    args = ap.parse_args()
    legs = []
    for n in [int(x) for x in args.sizes.split(",")]:
        for obstacle in (False, True):
            legs.append(leg(n, obstacle, args))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    ratios = {}
    for n in sorted({g["n"] for g in legs}):
        a = next(g for g in legs if g["n"] == n and not g["obstacle"])
        b = next(g for g in legs if g["n"] == n and g["obstacle"])
        ratios[str(n)] = {"projection": round(b["projection_ms"] / a["projection_ms"], 3), "step": round(b["step_ms"] / a["step_ms"], 3)}
    print(json.dumps({"tool": "obstacle_bench", "jacobi_iters": args.jacobi_iters, "window": [args.warmup, args.warmup + args.steps],
                      "legs": legs, "with_over_without": ratios,
                      "targets": {"projection_256": 1.15, "step": 1.15, "masked_sweep_frac_peak_512": 0.6}}))


if __name__ == "__main__":
    main()
