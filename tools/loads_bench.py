"""Times the per-obstacle pressure loads on the GPU and writes profiles/loads_bench.json.

    python tools/loads_bench.py [--n 128 256] [--steps 6] [--repeats 3] [--op-repeats 20] [--parent-libs DIR]

Per grid size n^3, the scene is scenes.paddle plus one sphere moving along +x in rising smoke, Jacobi projection.  The
pressure, the flags and the rows summary after `steps` steps stay on the device, and `repeats` alternating
rounds time every leg with events on the compute stream around `op-repeats` back-to-back calls:
    loads_rows           gpu_obstacle_loads with the rows summary
    loads_no_rows        gpu_obstacle_loads with rows = NULL
    gpu_gradient_masked  the yardstick: the projection's own pass over the same flags (it also reads p and rewrites u, v, w)
The operator must read one flag byte per cell of the rows the summary does not rule out; each leg's figure is microseconds.
Then the whole step with BQ_OPT_OBSTACLE_LOADS at 1 against the same step with it at 0: two solvers alive in this process,
timed in alternating blocks of steps, the host clock between two device synchronisations.
--parent-libs DIR: for scale, the same step (option 0 -- the libraries there know no other) on the libbimocq_hip.so /
libbimocq_host.so found in DIR (a build of the parent commit), timed in a child process of its own.
No test asserts a time."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(n):
    from gpufluidsimulation_amd import scenes
    return scenes.paddle(n, 1.0, spin=2.0) + [(0, 0.25, 0.75, 0.5, 0.08, 0.0, 0.0, 0.3, 0.0, 0.0)]


def make_solver(n, iters, lib=None, errlib=None):
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0, lib=lib, errlib=errlib)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)])
    s.setProjection(iters, 0.5)
    s.setBoundary(scene(n))
    return s


def timed_steps(s, sync, first, count, dt):
    sync()
    t0 = time.perf_counter()
    for f in range(first, first + count):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    sync()
    return round((time.perf_counter() - t0) * 1e3 / count, 4)


def parent_child(args):
    """the step time on the libraries in args.parent_libs, printed as one JSON line"""
    from gpufluidsimulation_amd import _lib, solver
    hip = C.CDLL(os.path.join(args.parent_libs, "libbimocq_hip.so"), mode=C.RTLD_GLOBAL)
    for name, (res, argtypes) in _lib.HIP_SIGS.items():
        if hasattr(hip, name):
            fn = getattr(hip, name)
            fn.restype, fn.argtypes = res, argtypes
    host = C.CDLL(os.path.join(args.parent_libs, "libbimocq_host.so"))
    solver.HOST_SIGS = {k: v for k, v in solver.HOST_SIGS.items() if hasattr(host, k)}
    solver.bind_host(host)
    assert hip.fl_init(0) == 0
    n = args.n[0]
    dt = 2.0 / n
    s = make_solver(n, args.jacobi_iters, lib=host, errlib=hip)
    for f in range(args.steps):
        s.updateBoundary(f, dt)
        s.advance(f, dt)
    out = []
    for r in range(args.repeats):
        out.append(timed_steps(s, hip.fl_sync, args.steps + r * args.block, args.block, dt))
    s._check()
    s.close()
    print(json.dumps({"parent_ms_per_step": out}))


def bench(n, args):
    import numpy as np

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    dt = 2.0 / n
    h = float(np.float32(1.0) / np.float32(n))
    solvers = {"option_0": make_solver(n, args.jacobi_iters), "option_1": make_solver(n, args.jacobi_iters)}
    solvers["option_1"].setOption(solver.OPT_OBSTACLE_LOADS, 1)
    for s in solvers.values():
        for f in range(args.steps):
            s.updateBoundary(f, dt)
            s.advance(f, dt)
        s._check()
    s = solvers["option_1"]
    host = {k: s.field(k) for k in ("u", "v", "w", "p")}
    poses = s.boundaryPoses()
    entries = scene(n)
    entries = [solver.Rotating((1, *poses[0][0], *entries[0].obstacle[4:7], 0.0, 0.0, 0.0), spin=poses[0][2], orientation=poses[0][1]),
               (0, *poses[1][0], *entries[1][4:10])]
    arr, ls, pose, nb = solver.pose_arrays(entries)
    dev = {k: lib.fl_malloc(a.nbytes) for k, a in host.items()}
    for k, a in host.items():
        assert dev[k]
        lib.fl_memcpy_h2d(dev[k], a.ctypes.data, a.nbytes)
    dev["solid"], dev["rows"], dev["out"] = lib.fl_malloc(n ** 3), lib.fl_malloc(n * n), lib.fl_malloc(128 * 8)
    assert dev["solid"] and dev["rows"] and dev["out"]
    lib.fl_memset(dev["rows"], 0, n * n)
    lib.gpu_obstacle_flags_pose(dev["solid"], dev["rows"], C.addressof(arr), nb, None, C.addressof(pose), h, n, n, n)
    bq.check()
    rows = np.empty(n * n, np.uint8)
    solid = np.empty(n ** 3, np.uint8)
    lib.fl_sync()
    lib.fl_memcpy_d2h(rows.ctypes.data, dev["rows"], rows.nbytes)
    lib.fl_memcpy_d2h(solid.ctypes.data, dev["solid"], solid.nbytes)
    assert np.array_equal(solid != 0, s.solidMask().ravel() != 0)
    ev = [lib.fl_event_create() for _ in range(2)]

    def timed(fn):
        fn()                                    # warm-up: code object, caches, the scratch buffer
        lib.fl_sync()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        return round(lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats, 2)

    def loads(with_rows):
        return lambda: lib.gpu_obstacle_loads(dev["p"], None, dev["solid"], dev["rows"] if with_rows else None, C.addressof(arr), nb,
                                              h, n, n, n, dev["out"])

    legs = {"loads_rows": loads(True), "loads_no_rows": loads(False),
            "gpu_gradient_masked": lambda: lib.gpu_gradient_masked(dev["u"], dev["v"], dev["w"], dev["p"], None, None, None, dev["solid"],
                                                                   n, n, n, 0.5)}
    runs = {k: [] for k in legs}
    for r in range(args.repeats):
        for k, fn in legs.items():
            runs[k].append(timed(fn))
            print(f"n {n} round {r} {k}: {runs[k][-1]} us", file=sys.stderr, flush=True)
    outs = []
    for with_rows in (True, False):
        loads(with_rows)()
        got = np.empty((16, 8), np.float64)
        lib.fl_sync()
        lib.fl_memcpy_d2h(got.ctypes.data, dev["out"], got.nbytes)
        outs.append(got)
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for p in dev.values():
        lib.fl_free(p)

    step_ms = {k: [] for k in solvers}
    for r in range(args.repeats):
        for k, sv in solvers.items():
            step_ms[k].append(timed_steps(sv, lib.fl_sync, args.steps + r * args.block, args.block, dt))
            print(f"n {n} round {r} step {k}: {step_ms[k][-1]} ms", file=sys.stderr, flush=True)
    row = solvers["option_1"].obstacleLoads()
    for sv in solvers.values():
        sv._check()
        sv.close()

    def stat(v, nd):
        return {"runs": v, "mean": round(sum(v) / len(v), nd), "spread": round(max(v) - min(v), nd)}

    res = {"n": n, "obstacle_cells": int((solid != 0).sum()), "wetted_faces": [int(x) for x in outs[0][:nb, 6]],
           "rows_marked": int(rows.sum()), "rows_total": int(rows.size),
           "same_bits_with_and_without_rows": outs[0].tobytes() == outs[1].tobytes(),
           "legs_us_per_call": {k: stat(v, 2) for k, v in runs.items()},
           "step_ms": {k: stat(v, 4) for k, v in step_ms.items()},
           "last_row": {"step": row["step"], "paddle_torque_z": float(row["torque"][0, 2]), "sphere_force_x": float(row["force"][1, 0])}}
    res["step_ms"]["added_by_option_1"] = round(res["step_ms"]["option_1"]["mean"] - res["step_ms"]["option_0"]["mean"], 4)
    if args.parent_libs:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--steps", str(args.steps), "--repeats", str(args.repeats),
               "--block", str(args.block), "--jacobi-iters", str(args.jacobi_iters), "--parent-libs", args.parent_libs]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
        if r.returncode == 0:
            res["step_ms"]["parent_commit_option_0"] = stat(json.loads(r.stdout.strip().splitlines()[-1])["parent_ms_per_step"], 4)
        else:
            res["step_ms"]["parent_commit_option_0"] = f"child failed with status {r.returncode}"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--steps", type=int, default=6, help="steps before anything is timed")
    ap.add_argument("--block", type=int, default=10, help="steps per timed block")
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--op-repeats", type=int, default=20)
    ap.add_argument("--parent-libs", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loads_bench.json"))
    args = ap.parse_args()
    if args.child:
        return parent_child(args)
    result = {"tool": "loads_bench", "scene": "scenes.paddle (spin 2) and a sphere of radius 0.08 moving along +x, rising smoke, Jacobi",
              "jacobi_iters": args.jacobi_iters, "repeats": args.repeats, "op_repeats": args.op_repeats, "block": args.block,
              "timing": "legs: events on the compute stream around back-to-back calls; steps: host clock between two device "
                        "synchronisations around a block of steps (updateBoundary + advance), the two solvers alternating",
              "grids": [bench(n, args) for n in args.n]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
