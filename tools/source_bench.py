"""Cost of the shaped sources on the GPU step: the rising-smoke scene of bench.py at 256^3, 200 Jacobi
sweeps, library defaults, source of radius 0.1 L at the rising-smoke position, active on every frame, emitted velocity zero
(every leg computes the same kind of flow).  Legs:
  legacy           the legacy emitter with emiter = 0 (gpu_emit_smoke: four launches over all nodes) -- the yardstick
  sphere           an analytic sphere source with the velocity flag (gpu_emit_sources)
  levelset         levelset_sphere(0.1 L, h) with the flag
  levelset_moving  the same moving at 0.1 L / s
  none             no source at all after frame 0 (the legacy emitter of bench.py, emit_frames = 1)
Per leg: step_ms (wall mean over steps [warmup, warmup + steps)), phase_ms (BQ_OPT_PROFILE_PHASES over the same window), and
emit_us_per_step -- the summed duration of the emission kernels per step from one `rocprofv3 --kernel-trace --stats` child
run of this tool (kernel trace only, a process of its own, under its own time limit).  Writes profiles/source_bench.json.
Usage: python tools/source_bench.py [--n 256] [--steps 180] [--warmup 20] [--jacobi-iters 200] [--trace-steps 40] [--out PATH]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("legacy", "sphere", "levelset", "levelset_moving", "none")
EMIT_KERNELS = ("emit_velocity_kernel", "emit_field_kernel", "emit_sources_kernel")
R = 0.1


def make(name, n, jacobi_iters):
    from gpufluidsimulation_amd.scenes import SMOKE, rising_smoke
    from gpufluidsimulation_amd.solver import BimocqGPUSolver, Source, levelset_sphere
    h = 1.0 / n
    always = 1 << 30
    pos = (SMOKE[0], SMOKE[1], 0.5 * n * h)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    em = rising_smoke(n, h)
    if name == "legacy":
        em = [pos + (R, 1.0, 1.0, 0.0, always)]
    s.setSmoke(0.0, 1.0, em if name in ("legacy", "none") else [])
    s.setProjection(jacobi_iters, 0.5)
    vel = dict(velocity=(0.0, 0.0, 0.0))
    if name == "sphere":
        s.setSources([Source(("sphere", R), pos, 1.0, 1.0, always, **vel)])
    elif name in ("levelset", "levelset_moving"):
        motion = (0.1, 0.0, 0.0) if name == "levelset_moving" else (0.0, 0.0, 0.0)
        s.setSources([Source(levelset_sphere(R, h), pos, 1.0, 1.0, always, motion=motion, **vel)])
    return s, 2.0 * h


def leg(name, args):
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    s, dt = make(name, args.n, args.jacobi_iters)
    for f in range(args.warmup):
        s.advance(f, dt)
    lib.fl_sync()
    s.setOption(8, 1)
    s.phaseMs(reset=True)
    t0 = time.perf_counter()
    for f in range(args.warmup, args.warmup + args.steps):
        s.advance(f, dt)
    lib.fl_sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    phases, psteps = s.phaseMs(reset=True)
    bq.check()
    out = {"case": name, "n": args.n, "step_ms": round(wall, 3),
           "phase_ms": {k: round(v / max(1, psteps), 3) for k, v in phases.items()},
           "rho_max": float(s.field("rho").max())}
    s.close()
    return out


def child(name, args):
    """what runs under rocprofv3: the leg's steps and nothing else"""
    import gpufluidsimulation_amd as bq
    s, dt = make(name, args.n, args.jacobi_iters)
    for f in range(args.trace_steps):
        s.advance(f, dt)
    bq.hip_lib().fl_sync()
    bq.check()
    s.close()


class ChildFailed(RuntimeError):
    pass


def trace(name, args):
    """{kernel: [calls, total ns]} of the emission kernels from one kernel-trace child run, or a reason"""
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    work = tempfile.mkdtemp(prefix="source_bench_")
    try:
        cmd = ["timeout", "-k", "10", str(args.trace_timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", work, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", name, "--n", str(args.n),
               "--jacobi-iters", str(args.jacobi_iters), "--trace-steps", str(args.trace_steps)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:       # a time limit, an abort, a fault: nothing more is started on the GPU by this tool
            raise ChildFailed(f"rocprofv3 child of leg {name} ended with {r.returncode}: {r.stdout[-300:]}")
        files = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "the rocprofv3 child left no kernel stats file"
        found = {}
        for row in csv.DictReader(open(files[0])):
            for k in EMIT_KERNELS:
                if k in row["Name"]:
                    c = found.setdefault(k, [0, 0.0])
                    c[0] += int(row["Calls"])
                    c[1] += float(row["TotalDurationNs"])
        return found, None
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--trace-steps", type=int, default=40)
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--legs", nargs="*", default=list(LEGS))
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_bench.json"))
    args = ap.parse_args()
    if args.child:
        child(args.child, args)
        return
    legs, failed = [], None
    for name in args.legs:
        g = leg(name, args)
        try:
            kernels, why = trace(name, args)
        except ChildFailed as e:    # write what there is and stop: no further leg, no further child
            g["emit_kernels"], g["emit_us_per_step"], g["trace_note"] = None, None, str(e)
            legs.append(g)
            failed = str(e)
            break
        if kernels is None:
            g["emit_kernels"], g["emit_us_per_step"], g["trace_note"] = None, None, why
        else:
            g["emit_kernels"] = {k: {"calls_per_step": v[0] / args.trace_steps, "us_per_call": round(v[1] / max(1, v[0]) / 1e3, 3)}
                                 for k, v in kernels.items()}
            g["emit_us_per_step"] = round(sum(v[1] for v in kernels.values()) / args.trace_steps / 1e3, 3)
        legs.append(g)
        print(json.dumps(g), file=sys.stderr, flush=True)
    by = {g["case"]: g for g in legs}
    result = {"tool": "source_bench", "jacobi_iters": args.jacobi_iters, "window": [args.warmup, args.warmup + args.steps],
              "trace_steps": args.trace_steps, "legs": legs}
    if failed:
        result["stopped"] = failed
    if "legacy" in by and not failed:
        result["step_over_legacy"] = {k: round(g["step_ms"] / by["legacy"]["step_ms"], 4) for k, g in by.items() if k != "legacy"}
        a = by["legacy"]["emit_us_per_step"]
        result["emit_over_legacy"] = {k: (round(g["emit_us_per_step"] / a, 4) if a and g["emit_us_per_step"] is not None else None)
                                      for k, g in by.items() if k not in ("legacy", "none")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
