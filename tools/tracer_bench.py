"""Times the tracer operators on the GPU and writes profiles/tracer_bench.json.

    python tools/tracer_bench.py [--n 256] [--steps 100] [--repeats 3] [--op-repeats 5] [--parent DIR]

The velocity of the headline scene (bench.py: rising smoke at n^3, 200 Jacobi iterations, dt = 2 h) after `steps` steps, with
that step's cfldt and dt.  One process, `repeats` alternating runs of every leg, each the event time on the compute stream
around `op-repeats` back-to-back calls from the same start positions (restored before every batch):

    forward                 gpu_solve_forward on identity maps: n^3 nodes, the same trace per element, perfectly coherent --
                            existing code, the yardstick of the tracer kernel (ns per traced node: the (n - 4)^3 interior ones)
    nodes                   gpu_trace_particles on the n^3 node positions in lattice order (2^24 at n = 256): the forward map's
                            work as a particle list
    seeded_<N>              gpu_trace_particles on the first N = 2^20, 2^22, 2^24 particles of gpu_seed_particles (2 per cell,
                            whole planes, k outermost)
    shuffled_<N>            the same set under a fixed random permutation: the fully mixed case
    sorted_<N>              that shuffled set after one gpu_sort_particles
    sort_<N>                gpu_sort_particles of the shuffled set itself
    advected / advected_sorted   the solver's own set: 1 tracer per cell seeded at step 0 and carried through the `steps` steps of
                            the real flow, traced in the order the arrays are in, and again after one sort: what a run that
                            never sorts has actually lost by then

The rule for the default of BQ_OPT_TRACER_SORT_EVERY: it stays 0 unless the mixed case gains more per N
steps than one sort costs, by more than the run-to-run spread -- and the advected set, which is what a run really holds, gains
more than its spread as well.  The tool reports the break-even N; it asserts no time.

--parent DIR: a built tree of the parent commit.  bench.py of both trees (no tracers anywhere) is then run alternately,
`--ab-rounds` times each (which of the two goes first alternates as well), as fresh child processes, and the difference of the
means is set against the spread of the runs.  --ab-only: nothing but that comparison; its block replaces the one in --out."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_line(tree, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--no-extra", "--no-cpu-baseline", "--no-measure-traffic"], cwd=tree, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def compare_with_parent(args):
    """bench.py of the parent tree and of this one, alternating, as fresh child processes"""
    this, parent = [], []
    for r in range(args.ab_rounds):
        for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):      # who goes first alternates too
            if who == "parent":
                parent.append(bench_line(os.path.abspath(args.parent), args.ab_steps, 20))
            else:
                this.append(bench_line(ROOT, args.ab_steps, 20))
        print(f"A/B round {r}: parent {parent[-1]} ms, this {this[-1]} ms per step", file=sys.stderr, flush=True)
    mp, mt = sum(parent) / len(parent), sum(this) / len(this)
    spread = max(max(parent) - min(parent), max(this) - min(this))
    return {
        "command": f"bench.py --gpus 1 --steps {args.ab_steps} --warmup 20 --no-extra --no-cpu-baseline --no-measure-traffic, alternating",
        "parent_ms_per_step": parent, "this_ms_per_step": this, "parent_mean": round(mp, 4), "this_mean": round(mt, 4),
        "difference_ms": round(mt - mp, 4), "run_to_run_spread_ms": round(spread, 4), "inside_spread": abs(mt - mp) <= spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--op-repeats", type=int, default=5)
    ap.add_argument("--counts", type=int, nargs="*", default=[1 << 20, 1 << 22, 1 << 24])
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: alternate its bench.py with this tree's")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-only", action="store_true", help="with --parent: only the comparison with the parent tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracer_bench.json"))
    args = ap.parse_args()

    if args.ab_only:
        assert args.parent, "--ab-only needs --parent"
        with open(args.out) as f:
            result = json.load(f)
        result["advance_without_tracers_vs_parent"] = compare_with_parent(args)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["advance_without_tracers_vs_parent"]))
        return

    import numpy as np

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd.scenes import rising_smoke
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    n = args.n
    h = float(np.float32(1.0) / np.float32(n))
    dt = 2.0 / n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, 1.0 / n))
    s.setProjection(args.jacobi_iters, 0.5)
    s.seedTracers((0, 0, 0), (n, n, n), 1, 1)               # the advected set: carried by the real flow from step 0
    for f in range(args.steps):
        s.advance(f, dt)
    s._check()
    cfldt = float(s.cfldt)
    host = {k: s.field(k) for k in ("u", "v", "w")}
    advected, _ = s.tracersStored()
    s.close()

    ev = [lib.fl_event_create() for _ in range(2)]

    def upload(a):
        a = np.ascontiguousarray(a)
        p = lib.fl_malloc(a.nbytes)
        assert p
        lib.fl_memcpy_h2d(p, a.ctypes.data, a.nbytes)
        return p

    vel = [upload(host[k]) for k in ("u", "v", "w")]

    def timed(fn, restore):
        restore()
        fn()                                    # warm-up: code object, workspace, caches
        lib.fl_sync()
        restore()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        lib.fl_sync()
        return lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats         # microseconds per call

    class Set:
        """a particle set on the device: start positions kept aside, restored before every batch"""
        def __init__(self, pts):
            self.n = len(pts)
            self.start = [upload(pts[:, c]) for c in range(3)]
            self.cur = [lib.fl_malloc(4 * self.n) for _ in range(3)]
            self.alt = [lib.fl_malloc(4 * self.n) for _ in range(4)]
            assert all(self.cur) and all(self.alt)

        def restore(self):
            for a, b in zip(self.cur, self.start):
                lib.fl_memcpy_d2d(a, b, 4 * self.n)

        def trace(self):
            rc = lib.gpu_trace_particles(*vel, *self.cur, self.n, h, n, n, n, cfldt, dt)
            assert rc == 0, rc

        def sort(self):
            rc = lib.gpu_sort_particles(*self.cur, None, *self.alt, self.n, h, n, n, n)
            assert rc == 0, rc

        def sorted_points(self):
            self.restore()
            self.sort()
            lib.fl_sync()
            out = np.empty((3, self.n), np.float32)
            for c in range(3):
                lib.fl_memcpy_d2h(out[c].ctypes.data, self.alt[c], 4 * self.n)
            return np.ascontiguousarray(out.T)

        def free(self):
            for p in self.start + self.cur + self.alt:
                lib.fl_free(p)

    legs = {}           # name -> (elements, callable returning microseconds)

    # the yardstick: the forward map update on identity maps
    maps = [lib.fl_malloc(4 * n ** 3) for _ in range(3)]
    assert all(maps)

    def maps_restore():
        lib.gpu_init_maps(*maps, h, n, n, n)

    legs["forward"] = ((n - 4) ** 3, lambda: timed(lambda: lib.gpu_solve_forward(*vel, *maps, h, n, n, n, cfldt, dt), maps_restore))

    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    nodes = np.stack([ii, jj, kk], axis=-1).reshape(-1, 3).astype(np.float32) * np.float32(h)
    nodes = np.clip(nodes, np.float32(h), np.float32(n) * np.float32(h) - np.float32(h)).astype(np.float32)
    del kk, jj, ii
    sets = {"nodes": Set(nodes)}
    del nodes
    legs["nodes"] = (sets["nodes"].n, lambda: timed(sets["nodes"].trace, sets["nodes"].restore))

    rng = np.random.default_rng(2024)
    for N in args.counts:
        planes = -(-N // (2 * (n - 2) ** 2))
        assert planes <= n - 2, "count too large for this grid at 2 per cell"
        soa = [lib.fl_malloc(4 * planes * 2 * (n - 2) ** 2) for _ in range(3)]
        assert all(soa)
        assert lib.gpu_seed_particles(*soa, 0, n, 0, n, 1, 1 + planes, 2, 7, h, n, n, n) == 0
        lib.fl_sync()
        pts = np.empty((3, N), np.float32)
        for c in range(3):
            lib.fl_memcpy_d2h(pts[c].ctypes.data, soa[c], 4 * N)
            lib.fl_free(soa[c])
        pts = np.ascontiguousarray(pts.T)
        seeded = Set(pts)
        shuffled = Set(pts[rng.permutation(N)])
        resorted = Set(shuffled.sorted_points())
        sets[f"seeded_{N}"], sets[f"shuffled_{N}"], sets[f"sorted_{N}"] = seeded, shuffled, resorted
        for name in ("seeded", "shuffled", "sorted"):
            st = sets[f"{name}_{N}"]
            legs[f"{name}_{N}"] = (N, (lambda st=st: timed(st.trace, st.restore)))
        legs[f"sort_{N}"] = (N, (lambda st=shuffled: timed(st.sort, st.restore)))
        del pts

    adv = Set(advected)
    adv_sorted = Set(adv.sorted_points())
    sets["advected"], sets["advected_sorted"] = adv, adv_sorted
    legs["advected"] = (adv.n, lambda: timed(adv.trace, adv.restore))
    legs["advected_sorted"] = (adv.n, lambda: timed(adv_sorted.trace, adv_sorted.restore))
    legs["advected_sort"] = (adv.n, lambda: timed(adv.sort, adv.restore))

    runs = {k: [] for k in legs}
    for r in range(args.repeats):
        for k, (_, fn) in legs.items():
            runs[k].append(round(fn(), 2))
            print(f"run {r} {k}: {runs[k][-1]} us", file=sys.stderr, flush=True)
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for st in sets.values():
        st.free()
    for p in vel + maps:
        lib.fl_free(p)

    res = {}
    for k, v in runs.items():
        mean = sum(v) / len(v)
        res[k] = {"elements": legs[k][0], "us_per_call": v, "mean": round(mean, 2), "spread": round(max(v) - min(v), 2),
                  "ns_per_element": round(mean * 1e3 / legs[k][0], 4)}
    yard = {"forward_ns_per_node": res["forward"]["ns_per_element"], "nodes_ns_per_particle": res["nodes"]["ns_per_element"],
            "ratio_particles_over_forward": round(res["nodes"]["ns_per_element"] / res["forward"]["ns_per_element"], 3)}
    rule = {}
    for N in args.counts:
        sh, so, st = res[f"shuffled_{N}"], res[f"sorted_{N}"], res[f"sort_{N}"]
        gain = sh["mean"] - so["mean"]
        spread = max(sh["spread"], so["spread"], st["spread"])
        rule[str(N)] = {"gain_us_per_step": round(gain, 2), "sort_us": st["mean"], "spread_us": spread,
                        "break_even_steps": (round((st["mean"] + spread) / gain, 2) if gain > 0 else None),
                        "seeded_over_sorted": round(res[f"seeded_{N}"]["mean"] / so["mean"], 3)}
    a, b, c = res["advected"], res["advected_sorted"], res["advected_sort"]
    again = a["mean"] - b["mean"]
    aspread = max(a["spread"], b["spread"])
    rule["advected"] = {"steps_carried": args.steps, "gain_us_per_step": round(again, 2), "sort_us": c["mean"], "spread_us": aspread,
                        "gain_exceeds_spread": again > aspread,
                        "break_even_steps": (round((c["mean"] + aspread) / again, 2) if again > aspread else None)}
    result = {"tool": "tracer_bench", "n": n, "velocity": f"headline rising smoke after {args.steps} steps", "cfldt": cfldt, "dt": dt,
              "substeps_per_trace": int(np.ceil(dt / cfldt)) if cfldt > 0 else None, "repeats": args.repeats, "op_repeats": args.op_repeats,
              "timing": "events on the compute stream around back-to-back calls from restored start positions, microseconds per call",
              "legs": res, "yardstick_forward": yard, "sort_rule": rule}

    if args.parent:
        result["advance_without_tracers_vs_parent"] = compare_with_parent(args)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
