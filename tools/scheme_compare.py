"""The comparison the three advection schemes were built for: kinetic energy, enstrophy and the
density centroid over a run of BiMocq (0), MacCormack (2) and MAC reflection (3), read from the device through
BQ_OPT_DIAGNOSTICS_EVERY -- no field leaves the GPU.

  default   the leapfrogging vortex rings (N x N x N/2, no buoyancy) and the rising smoke (N^3) for each scheme, `--steps`
            steps of dt = 2h with `--jacobi-iters` sweeps, sampled every `--every` steps
            -> profiles/scheme_compare.json: per scene and scheme the curves step / kinetic / enstrophy / centroid / vort_max,
               the ratio last / first sample of energy and enstrophy, and ms per step
  --bench   gpu_flow_stats itself at N^3 on the flow after `--bench-steps` rising-smoke steps, one process, the legs
            alternating `--repeats` times, each the mean event time of `--op-repeats` back-to-back calls after a warm-up:
              gpu_divergence          same three inputs, one output: the streaming yardstick
              flow_stats              the marching kernel, statistics only (with density and temperature)
              flow_stats_vort         ... and vort_mag
              flow_stats_cell         the one-thread-per-cell kernel (FL_OPT_DIAG_KCHUNK = -1), statistics only
              flow_stats_cell_vort    ... and vort_mag
            -> profiles/flow_stats_bench.json: us per call of every run, mean and spread (max - min), the ratios to
               gpu_divergence, and the rule the default rests on: the march stays the default only if its mean beats the
               cell form's by more than the march leg's own spread

Usage: python tools/scheme_compare.py [--n 128] [--steps 120] [--every 4] [--jacobi-iters 200] [--out PATH]
       python tools/scheme_compare.py --bench [--n 256] [--bench-steps 40] [--repeats 3] [--op-repeats 20] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCHEMES = {"bimocq": 0, "maccormack": 2, "reflection": 3}


def make(scene, scheme, n, iters):
    from gpufluidsimulation_amd import scenes
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    h = 1.0 / n
    if scene == "leapfrog":
        s = BimocqGPUSolver(n, n, n // 2, 1.0, 0.0, 1.0, device=0, scheme=scheme)
        s.setSmoke(0.0, 0.0, scenes.leapfrog(n // 2, h))
    else:
        s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0, scheme=scheme)
        s.setSmoke(0.0, 1.0, scenes.rising_smoke(n, h))
    s.setProjection(iters, 0.5)
    return s, 2.0 * h


def curves(scene, scheme, args):
    from gpufluidsimulation_amd import solver
    s, dt = make(scene, scheme, args.n, args.jacobi_iters)
    s.setOption(solver.OPT_DIAGNOSTICS_EVERY, args.every)
    t0 = time.perf_counter()
    for f in range(args.steps):
        s.advance(f, dt)
    hist = s.diagnosticsHistory()                # the first host synchronisation of the run
    sec = time.perf_counter() - t0
    s._check()
    s.close()
    col = {name: hist[:, a].tolist() for a, name in enumerate(solver.DIAG_NAMES)}
    first, last = hist[0], hist[-1]
    keep = lambda a, b: float(b / a) if a else None
    return {"step": [int(x) for x in col["step"]], "kinetic": col["kinetic"], "enstrophy": col["enstrophy"], "vort_max": col["vort_max"],
            "div_l2": col["div_l2"], "rho_sum": col["rho_sum"], "centroid": [col["centroid_x"], col["centroid_y"], col["centroid_z"]],
            "kinetic_last_over_first": keep(first[0], last[0]), "enstrophy_last_over_first": keep(first[1], last[1]),
            "ms_per_step_wall": round(sec * 1e3 / args.steps, 3)}


def compare(args):
    out = {"tool": "scheme_compare", "n": args.n, "steps": args.steps, "every": args.every, "jacobi_iters": args.jacobi_iters,
           "dt": "2h", "scenes": {}}
    for scene in ("leapfrog", "rising_smoke"):
        out["scenes"][scene] = {}
        for name, scheme in SCHEMES.items():
            out["scenes"][scene][name] = c = curves(scene, scheme, args)
            print(f"{scene} {name}: kinetic x{c['kinetic_last_over_first']}, enstrophy x{c['enstrophy_last_over_first']}, "
                  f"{c['ms_per_step_wall']} ms/step", file=sys.stderr, flush=True)
    return out


def bench(args):
    import numpy as np

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import _lib
    lib = bq.hip_lib()
    n = args.n
    s, dt = make("rising_smoke", 0, n, args.jacobi_iters)
    for f in range(args.bench_steps):
        s.advance(f, dt)
    s._check()
    host = {k: s.field(k) for k in ("u", "v", "w", "rho", "T")}
    s.close()
    h = float(np.float32(1.0) / np.float32(n))
    dev = {}
    for k, a in host.items():
        dev[k] = lib.fl_malloc(a.nbytes)
        assert dev[k]
        lib.fl_memcpy_h2d(dev[k], a.ctypes.data, a.nbytes)
    dev["out"], dev["stats"] = lib.fl_malloc(4 * n ** 3), lib.fl_malloc(8 * _lib.STAT_COUNT)
    assert dev["out"] and dev["stats"]
    ev = [lib.fl_event_create() for _ in range(2)]

    def timed(fn):
        fn()                                    # warm-up: code object, workspace, caches
        lib.fl_sync()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        return round(lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats, 2)

    def stats(kchunk, vort):
        def fn():
            lib.fl_set_option(_lib.FL_OPT_DIAG_KCHUNK, kchunk)
            lib.gpu_flow_stats(dev["u"], dev["v"], dev["w"], dev["rho"], dev["T"], dev["out"] if vort else None, h, n, n, n, dev["stats"])
        return fn

    legs = {"gpu_divergence": lambda: lib.gpu_divergence(dev["u"], dev["v"], dev["w"], dev["out"], n, n, n, 0.5),
            "flow_stats": stats(0, False), "flow_stats_vort": stats(0, True),
            "flow_stats_cell": stats(-1, False), "flow_stats_cell_vort": stats(-1, True)}
    runs = {k: [] for k in legs}
    for r in range(args.repeats):
        for k, fn in legs.items():
            runs[k].append(timed(fn))
            print(f"run {r} {k}: {runs[k][-1]} us", file=sys.stderr, flush=True)
    lib.fl_set_option(_lib.FL_OPT_DIAG_KCHUNK, 0)
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for p in dev.values():
        lib.fl_free(p)
    res = {k: {"us_per_call": v, "mean": round(sum(v) / len(v), 2), "spread": round(max(v) - min(v), 2)} for k, v in runs.items()}
    base = res["gpu_divergence"]["mean"]
    for k in res:
        res[k]["ratio_to_divergence"] = round(res[k]["mean"] / base, 3)
    rule = {}
    for a, b in (("flow_stats", "flow_stats_cell"), ("flow_stats_vort", "flow_stats_cell_vort")):
        rule[a] = {"march_mean": res[a]["mean"], "cell_mean": res[b]["mean"], "march_spread": res[a]["spread"],
                   "march_stays_default": res[a]["mean"] + res[a]["spread"] < res[b]["mean"]}
    return {"tool": "scheme_compare --bench", "n": n, "flow": f"rising smoke after {args.bench_steps} steps", "repeats": args.repeats,
            "op_repeats": args.op_repeats, "timing": "events on the compute stream around back-to-back calls",
            "bytes_streamed_MB": {"velocity": round(sum(host[k].nbytes for k in "uvw") / 1e6, 1), "scalars": round(2 * host["rho"].nbytes / 1e6, 1),
                                  "vort_mag": round(host["rho"].nbytes / 1e6, 1)},
            "legs": res, "default_rule": rule}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--bench-steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--op-repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpufluidsimulation_amd as bq
    assert bq.hip_lib().fl_init(0) == 0
    if args.bench:
        args.n = args.n or 256
        result, name = bench(args), "flow_stats_bench.json"
    else:
        args.n = args.n or 128
        result, name = compare(args), "scheme_compare.json"
    out = args.out or os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result if args.bench else {k: v for k, v in result.items() if k != "scenes"}))


if __name__ == "__main__":
    main()
