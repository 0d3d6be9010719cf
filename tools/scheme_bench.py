"""What the fused MacCormack operator buys on the GPU step: the rising-smoke scene of bench.py at 256^3,
200 Jacobi sweeps, one process.  Legs (scheme, BQ_OPT_FUSED_MACCORMACK):
  maccormack_unfused (2, 0)   maccormack_fused (2, 1)   reflection_unfused (3, 0: the launches the scheme always issued)
  reflection_fused (3, 2)
Every run starts from a fresh solver, advances `--warmup` steps and sums the event time of advance() (events on the compute
stream around the step, bq_solver_last_ms) over the next `--steps`; the legs alternate, `--repeats` runs each.  Per leg:
every run's ms per step, their mean and spread (max - min).  `operator`: gpu_maccormack on one scalar and on the u component
of the flow the last maccormack_fused run ended with, next to the launches it replaces (clear + gpu_semilag, two gpu_add,
gpu_clamp_extrema, the copy back), each as the mean event time of `--op-repeats` back-to-back issues after one warm-up.
`default_rule`: scheme 2 stays fused if its mean is not above the unfused mean by more than the unfused leg's spread.
Writes profiles/scheme_bench.json.
Usage: python tools/scheme_bench.py [--n 256] [--warmup 20] [--steps 40] [--repeats 3] [--jacobi-iters 200] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"maccormack_unfused": (2, 0), "maccormack_fused": (2, 1), "reflection_unfused": (3, 0), "reflection_fused": (3, 2)}


def make(name, args):
    from gpufluidsimulation_amd.scenes import rising_smoke
    from gpufluidsimulation_amd.solver import OPT_FUSED_MACCORMACK, BimocqGPUSolver
    scheme, option = LEGS[name]
    n = args.n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0, scheme=scheme)
    s.setSmoke(0.0, 1.0, rising_smoke(n, 1.0 / n))
    s.setProjection(args.jacobi_iters, 0.5)
    s.setOption(OPT_FUSED_MACCORMACK, option)
    return s, 2.0 / n


def run(name, args, keep=False):
    """ms per step over the window; keep: also the solver (for the operator timing)"""
    import gpufluidsimulation_amd as bq
    s, dt = make(name, args)
    for f in range(args.warmup):
        s.advance(f, dt)
    total = 0.0
    for f in range(args.warmup, args.warmup + args.steps):
        s.advance(f, dt)
        total += s.last_ms                      # blocking: the elapsed time of the step's two events
    bq.check()
    if keep:
        return total / args.steps, s, dt
    s.close()
    return total / args.steps


def operator(s, dt, args):
    """event times (us) of the fused launch and of the launches it replaces, on the solver's current flow"""
    import numpy as np

    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    n = args.n
    h = float(np.float32(1.0) / np.float32(n))
    host = {k: s.field(k) for k in ("rho", "u", "v", "w")}
    cfldt = float(s.cfldt)
    bufs = {}

    def dev(name, count, src=None):
        p = lib.fl_malloc(4 * count)
        assert p
        bufs[name] = p
        if src is not None:
            lib.fl_memcpy_h2d(p, src.ctypes.data, 4 * count)
        else:
            lib.fl_memset(p, 0, 4 * count)
        return p

    for k, a in host.items():
        dev(k, a.size, a)
    ev = [lib.fl_event_create() for _ in range(2)]

    def timed(fn):
        fn()                                    # warm-up: code object, caches
        lib.fl_sync()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        return round(lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats, 2)

    out = {"dt_over_cfldt": round(dt / cfldt, 3), "repeats": args.op_repeats}
    for field, stag in (("rho", (0, 0, 0)), ("u", (1, 0, 0))):
        count = host[field].size
        first, back, tmp, res = (dev(f"{field}_{x}", count) for x in ("first", "back", "tmp", "out"))
        vel = (bufs["u"], bufs["v"], bufs["w"])
        lib.gpu_semilag(first, bufs[field], *vel, *stag, h, n, n, n, cfldt, -dt)
        dims = (n + stag[0], n + stag[1], n + stag[2])
        off = tuple(0.5 * d for d in stag)
        steps = {
            "fused": lambda: lib.gpu_maccormack(res, first, bufs[field], bufs[field], *vel, *stag, h, n, n, n, cfldt, dt, dt),
            "clear": lambda: lib.fl_memset(back, 0, 4 * count),
            "semilag": lambda: lib.gpu_semilag(back, first, *vel, *stag, h, n, n, n, cfldt, dt),
            "add": lambda: lib.gpu_add(tmp, back, -0.5, count),
            "clamp_extrema": lambda: lib.gpu_clamp_extrema(bufs[field], tmp, *vel, *dims, *stag, *off, h, dt),
            "copy": lambda: lib.fl_memcpy_d2d(res, tmp, 4 * count),
        }
        lib.fl_memcpy_d2d(tmp, first, 4 * count)
        us = {k: timed(fn) for k, fn in steps.items()}
        us["replaced_sum"] = round(us["clear"] + us["semilag"] + 2 * us["add"] + us["clamp_extrema"] + us["copy"], 2)
        out[field] = us
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for p in bufs.values():
        lib.fl_free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--op-repeats", type=int, default=20)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scheme_bench.json"))
    args = ap.parse_args()
    import gpufluidsimulation_amd as bq
    assert bq.hip_lib().fl_init(0) == 0
    runs = {name: [] for name in LEGS}
    op = None
    for r in range(args.repeats):
        for name in LEGS:
            last = r == args.repeats - 1 and name == "maccormack_fused"
            if last:
                ms, s, dt = run(name, args, keep=True)
                op = operator(s, dt, args)
                s.close()
            else:
                ms = run(name, args)
            runs[name].append(round(ms, 4))
            print(f"run {r} {name}: {ms:.4f} ms/step", file=sys.stderr, flush=True)
    legs = {name: {"scheme": LEGS[name][0], "option": LEGS[name][1], "ms_per_step": v, "mean": round(sum(v) / len(v), 4),
                   "spread": round(max(v) - min(v), 4)} for name, v in runs.items()}
    a, b = legs["maccormack_unfused"], legs["maccormack_fused"]
    result = {"tool": "scheme_bench", "n": args.n, "jacobi_iters": args.jacobi_iters,
              "window": [args.warmup, args.warmup + args.steps], "repeats": args.repeats, "timing": "events on the compute stream around advance()",
              "legs": legs, "operator_us": op,
              "default_rule": {"fused_mean": b["mean"], "unfused_mean": a["mean"], "unfused_spread": a["spread"],
                               "scheme_2_stays_fused": b["mean"] <= a["mean"] + a["spread"]}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
