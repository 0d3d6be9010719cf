"""Times the shadowed density preview on the GPU and writes profiles/render_bench.json.

    python tools/render_bench.py [--n 256] [--steps 40] [--repeats 3] [--op-repeats 20]

The density after `steps` rising-smoke steps at n^3, one process, `repeats` alternating runs of every leg, each the event
time on the compute stream around `op-repeats` back-to-back calls:
    gpu_divergence              three inputs, one output: the streaming yardstick of DESIGN.md section 20
    view_<axis>[_seq]           gpu_render_density with light = -1 along +axis: the view pass alone (it reads rho only: 4 B per
                                cell compulsory); _seq with FL_OPT_RENDER_KCHUNK = -1 (one sequential march per ray)
    lit_<axis>[_seq]            view and light along +axis: shadow pass + view pass (8 B + 8 B per cell compulsory)
The operator issues both passes in one call, so the shadow pass is reported as lit - view of the same axis: an upper estimate,
because the lit view pass also reads the shadow field (4 B per cell more than the unlit one).
Shares of the streaming ceiling: compulsory bytes / time against gpu_divergence's bytes / time.

The two rules the defaults rest on:
    chunks    the chunk rule stays the default for an axis only if its mean beats the sequential march's by more than its own
              run-to-run spread
    x-march   the wave-scan kernels are kept as built if lit_x is not slower than lit_z by more than lit_z's spread

    python tools/render_bench.py --only z [--seq]    (under rocprofv3 --kernel-trace --stats, a run of its own)
runs nothing but lit_<axis> (--seq: with one sequential march per ray), so that the trace's per-kernel times are the shadow
pass and the view pass of that axis; it writes no file.

    python tools/render_bench.py --solids [--plain-only] [--root CHECKOUT] [--out FILE]
The preview with solid obstacles, written to profiles/render_solids_bench.json: the density and the
obstacle flags after `steps` rising-smoke steps with scenes.paddle turning (updateBoundary every step), then the legs
view_<axis> and lit_<axis> of gpu_render_density ("plain") and of gpu_render_density_solids ("solid", "solid_norows") in
alternating runs, and the ratios to the plain leg.  By compulsory bytes (a pass moves 8 B per cell and 4 B in the totals; the flags add one
byte to each) a solid leg is expected at 1.13 - 1.25 x its plain leg.  "solid" passes the rows summary, with which the
x kernels skip the flag loads of rows without a solid cell, "solid_norows" passes NULL (the marches never read it).  With --only <axis> (under rocprofv3 --kernel-trace --stats, a run of its own) nothing but the
plain and the solid lit leg (with the rows summary) of that axis run, so that the trace's per-kernel times say which kernel holds a solid leg's
time; it writes no file.  --plain-only times the plain legs alone, and --root CHECKOUT takes the package (and its built
libraries) from another checkout: the parent commit's, for the A/B of the plain legs (profiles/render_solids_{parent,this}_run*.json).
No test asserts a time."""
import argparse
import ctypes as C
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solids_main(args):
    """the legs of the preview with and without solid obstacles on the paddle scene"""
    if args.root:
        sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import _lib, scenes
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    if args.plain_only:                         # a checkout without the solid operator binds what it has
        _lib.HIP_SIGS.pop("gpu_render_density_solids", None)
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    n = args.n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)])
    s.setProjection(args.jacobi_iters, 0.5)
    s.setBoundary(scenes.paddle(n, 1.0))
    for f in range(args.steps):
        s.updateBoundary(f, 2.0 / n)
        s.advance(f, 2.0 / n)
    s._check()
    rho, flags = s.field("rho"), s.solidMask()
    s.close()
    has = (flags != 0).any(axis=2)
    rows = has.copy()
    rows[:, 1:] |= has[:, :-1]
    rows[:, :-1] |= has[:, 1:]
    host = {"rho": rho, "flags": flags, "rows": np.ascontiguousarray(rows.astype(np.uint8))}
    h = float(np.float32(1.0) / np.float32(n))
    dev = {}
    for k, a in host.items():
        dev[k] = lib.fl_malloc(a.nbytes)
        assert dev[k]
        lib.fl_memcpy_h2d(dev[k], a.ctypes.data, a.nbytes)
    dev["shadow"], dev["img"] = lib.fl_malloc(4 * n ** 3), lib.fl_malloc(24 * n * n)
    assert dev["shadow"] and dev["img"]
    prm = C.create_string_buffer(struct.pack("fff", args.sigma, 1.0, 0.1))
    sprm = C.create_string_buffer(struct.pack("ff", 0.6, 0.15))
    ev = [lib.fl_event_create() for _ in range(2)]

    def timed(fn):
        fn()                                    # warm-up: code object, workspace, caches
        lib.fl_sync()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        return round(lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats, 2)

    def leg(axis, lit, kind):
        shadow, light = (dev["shadow"] if lit else None), (2 * axis if lit else -1)
        rows = dev["rows"] if kind == "solid" else None
        if kind != "plain":
            return lambda: lib.gpu_render_density_solids(dev["rho"], dev["flags"], rows, shadow, h, n, n, n, 2 * axis, light,
                                                         C.cast(prm, C.c_void_p), C.cast(sprm, C.c_void_p), dev["img"])
        return lambda: lib.gpu_render_density(dev["rho"], shadow, h, n, n, n, 2 * axis, light, C.cast(prm, C.c_void_p), dev["img"])

    if args.only:                               # for a kernel trace: the plain and the solid lit leg of one axis, no file
        axis = "xyz".index(args.only)
        us = {kind: timed(leg(axis, True, kind)) for kind in ("plain", "solid")}
        lib.fl_sync()
        bq.check()
        print(json.dumps({"tool": "render_bench --solids --only", "leg": f"lit_{args.only}", "us_per_call": us}))
        return
    legs = {}
    for axis, name in enumerate("xyz"):
        for lit in (False, True):
            for kind in (("plain",) if args.plain_only else ("plain", "solid", "solid_norows")):
                legs[f"{kind}_{'lit' if lit else 'view'}_{name}"] = leg(axis, lit, kind)
    runs = {k: [] for k in legs}
    for r in range(args.repeats):
        for k, fn in legs.items():
            runs[k].append(timed(fn))
            print(f"run {r} {k}: {runs[k][-1]} us", file=sys.stderr, flush=True)
    lib.fl_sync()
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for p in dev.values():
        lib.fl_free(p)
    res = {k: {"us_per_call": v, "mean": round(sum(v) / len(v), 2), "spread": round(max(v) - min(v), 2)} for k, v in runs.items()}
    result = {"tool": "render_bench --solids", "n": n, "scene": f"rising smoke and scenes.paddle after {args.steps} steps with updateBoundary",
              "sigma": args.sigma, "nonzero_cells": int((rho > 0).sum()), "solid_cells": int((flags != 0).sum()),
              "repeats": args.repeats, "op_repeats": args.op_repeats,
              "timing": "events on the compute stream around back-to-back calls, microseconds per call", "legs": res}
    if not args.plain_only:
        result["expected_ratio_by_compulsory_bytes"] = [1.13, 1.25]
        for kind in ("solid", "solid_norows"):
            result[kind + "_over_plain"] = {k[len("plain_"):]: round(res[kind + "_" + k[len("plain_"):]]["mean"] / v["mean"], 3)
                                            for k, v in res.items() if k.startswith("plain_")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--op-repeats", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=12.0)
    ap.add_argument("--only", choices=["x", "y", "z"], default=None, help="only the lit leg of this axis, for a kernel trace")
    ap.add_argument("--seq", action="store_true", help="with --only: FL_OPT_RENDER_KCHUNK = -1")
    ap.add_argument("--solids", action="store_true", help="the paddle scene: plain legs against gpu_render_density_solids")
    ap.add_argument("--plain-only", action="store_true", help="with --solids: only the plain legs (any checkout has them)")
    ap.add_argument("--root", default=None, help="with --solids: the checkout whose package and libraries are timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "render_solids_bench.json" if args.solids else "render_bench.json")
    if args.solids:
        return solids_main(args)

    import numpy as np

    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import _lib
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    n = args.n
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0)
    s.setSmoke(0.0, 1.0, [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)])
    s.setProjection(args.jacobi_iters, 0.5)
    for f in range(args.steps):
        s.advance(f, 2.0 / n)
    s._check()
    host = {k: s.field(k) for k in ("u", "v", "w", "rho")}
    s.close()
    h = float(np.float32(1.0) / np.float32(n))
    dev = {}
    for k, a in host.items():
        dev[k] = lib.fl_malloc(a.nbytes)
        assert dev[k]
        lib.fl_memcpy_h2d(dev[k], a.ctypes.data, a.nbytes)
    dev["out"], dev["shadow"], dev["img"] = lib.fl_malloc(4 * n ** 3), lib.fl_malloc(4 * n ** 3), lib.fl_malloc(16 * n * n)
    assert dev["out"] and dev["shadow"] and dev["img"]
    prm = C.create_string_buffer(struct.pack("fff", args.sigma, 1.0, 0.1))
    ev = [lib.fl_event_create() for _ in range(2)]

    def timed(fn):
        fn()                                    # warm-up: code object, workspace, caches
        lib.fl_sync()
        lib.fl_event_record(ev[0])
        for _ in range(args.op_repeats):
            fn()
        lib.fl_event_record(ev[1])
        return round(lib.fl_event_elapsed_ms(ev[0], ev[1]) * 1e3 / args.op_repeats, 2)

    def render(axis, lit, kchunk):
        def fn():
            lib.fl_set_option(_lib.FL_OPT_RENDER_KCHUNK, kchunk)
            lib.gpu_render_density(dev["rho"], dev["shadow"] if lit else None, h, n, n, n, 2 * axis, 2 * axis if lit else -1,
                                   C.cast(prm, C.c_void_p), dev["img"])
        return fn

    if args.only:
        us = timed(render("xyz".index(args.only), True, -1 if args.seq else 0))
        lib.fl_sync()
        bq.check()
        print(json.dumps({"tool": "render_bench --only", "leg": f"lit_{args.only}{'_seq' if args.seq else ''}", "us_per_call": us}))
        return
    legs = {"gpu_divergence": lambda: lib.gpu_divergence(dev["u"], dev["v"], dev["w"], dev["out"], n, n, n, 0.5)}
    for axis, name in enumerate("xyz"):
        for lit in (False, True):
            legs[f"{'lit' if lit else 'view'}_{name}"] = render(axis, lit, 0)
            if axis:                            # marches along x take no chunks
                legs[f"{'lit' if lit else 'view'}_{name}_seq"] = render(axis, lit, -1)
    runs = {k: [] for k in legs}
    for r in range(args.repeats):
        for k, fn in legs.items():
            runs[k].append(timed(fn))
            print(f"run {r} {k}: {runs[k][-1]} us", file=sys.stderr, flush=True)
    # not a timing: at this size too the chunked and the sequential marches must leave the same bits
    same = {}
    for axis, name in ((1, "y"), (2, "z")):
        imgs = []
        for kchunk in (0, -1):
            render(axis, True, kchunk)()
            img = np.empty(2 * n * n)
            lib.fl_sync()
            lib.fl_memcpy_d2h(img.ctypes.data, dev["img"], img.nbytes)
            imgs.append(img)
        same[name] = bool(np.array_equal(imgs[0].view(np.uint64), imgs[1].view(np.uint64))) and bool(imgs[0][:n * n].max() > 0)
    lib.fl_set_option(_lib.FL_OPT_RENDER_KCHUNK, 0)
    bq.check()
    for e in ev:
        lib.fl_event_destroy(e)
    for p in dev.values():
        lib.fl_free(p)

    res = {k: {"us_per_call": v, "mean": round(sum(v) / len(v), 2), "spread": round(max(v) - min(v), 2)} for k, v in runs.items()}
    cells = n ** 3
    div_bytes = sum(host[k].nbytes for k in "uvw") + 4 * cells
    ceiling = div_bytes / res["gpu_divergence"]["mean"]                      # bytes per microsecond
    res["gpu_divergence"]["bytes"] = div_bytes
    for k in res:
        if k == "gpu_divergence":
            continue
        res[k]["compulsory_bytes"] = (16 if k.startswith("lit") else 4) * cells
        res[k]["share_of_streaming_ceiling"] = round(res[k]["compulsory_bytes"] / res[k]["mean"] / ceiling, 3)
    shadow = {a: round(res[f"lit_{a}"]["mean"] - res[f"view_{a}"]["mean"], 2) for a in "xyz"}
    rules = {"chunks": {}, "x_march": {}}
    for a in "yz":
        for kind in ("view", "lit"):
            c, q = res[f"{kind}_{a}"], res[f"{kind}_{a}_seq"]
            rules["chunks"][f"{kind}_{a}"] = {"chunk_mean": c["mean"], "chunk_spread": c["spread"], "sequential_mean": q["mean"],
                                              "chunk_rule_stays_default": c["mean"] + c["spread"] < q["mean"]}
    zbest = min(res["lit_z"], res["lit_z_seq"], key=lambda v: v["mean"])
    rules["x_march"] = {"lit_x_mean": res["lit_x"]["mean"], "lit_z_mean": zbest["mean"], "lit_z_spread": zbest["spread"],
                        "kept_as_built": res["lit_x"]["mean"] <= zbest["mean"] + zbest["spread"]}
    result = {"tool": "render_bench", "n": n, "density": f"rising smoke after {args.steps} steps", "sigma": args.sigma,
              "nonzero_cells": int((host["rho"] > 0).sum()), "repeats": args.repeats, "op_repeats": args.op_repeats,
              "timing": "events on the compute stream around back-to-back calls, microseconds per call",
              "chunked_equals_sequential_bits": same, "legs": res, "shadow_pass_us_upper_estimate (lit - view)": shadow, "rules": rules}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
