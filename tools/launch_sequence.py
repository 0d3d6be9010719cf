#!/usr/bin/env python3
"""The kernel launches of the stencil launchers over a table of shapes and option settings, for comparing two builds of the
library launch by launch (a refactor of the launchers must leave the list unchanged).

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/launch_sequence.py run [--log calls.txt] [--extended]
    python tools/launch_sequence.py reduce <dir> > launches.txt

`run` calls each launcher once per case through the C-ABI of the tree this file sits in (zeroed buffers: no launcher reads a
value back, so the sequence does not depend on the data) and writes what every call returned and which fused kernel it
reports to --log.  `reduce` turns the kernel trace into the ordered list of launches -- kernel name with its template
arguments, grid size, workgroup size -- written as a table of the distinct launches and the sequence of their numbers.
Two builds agree when both files are equal line for line.  --extended adds the shape and the option combinations of EXTENDED below
to the table (the lists without it are those of profiles/launch_geom_launches_*.txt, with it of profiles/jacobi_plan_launches_*.txt,
both from before the walled sweeps joined the table; with them: profiles/jacobi_family_launches_*.txt).

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/launch_sequence.py step --scene box --scheme reflection

`step` runs three steps of the rising-smoke scene at 64^3 with 20 Jacobi iterations through the host solver -- scene plain, sphere (one
sphere obstacle) or box (the closed container), scheme bimocq or reflection -- for the same comparison at the level of a solver step.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FP32_SHAPES = [(256, 256, 256), (128, 128, 128), (64, 256, 192), (320, 64, 48), (512, 512, 64)]
FP64_SHAPES = FP32_SHAPES + [(127, 127, 127)]
VARIANT, KCHUNK, ROWS, FUSE, KCHUNK2, RESERVE_CUS, MGCG_FUSE = 3, 5, 6, 8, 9, 16, 20
BOX = 1 | 2 | 4 | 16 | 32           # BQ_WALL_*: the reference's container, open at +y
# (option, value) pairs on top of FL_OPT_JACOBI_FUSE = 2
FP32_SETTINGS = ([[(ROWS, r)] for r in range(1, 8)] + [[(VARIANT, v)] for v in (1, 2)] +
                 [[(KCHUNK, k)] for k in (1, 2, 18, 19, 24, 25, 26)] + [[(KCHUNK2, 8)], [(RESERVE_CUS, 8)]])
FP64_SETTINGS = [[], [(FUSE, 0)], [(FUSE, 2)], [(FUSE, 2), (ROWS, 3)], [(ROWS, 5)], [(FUSE, 2), (ROWS, 8)], [(KCHUNK, 14)],
                 [(KCHUNK, 1)], [(KCHUNK, 2)], [(KCHUNK2, 8)], [(RESERVE_CUS, 8)]]
# --extended: what the tests and tools set and the table above lacks -- a shape on which only jacobi_lean3r_kernel takes the triples, the
# marching one-sweep kernel and both one-sweep kernels' readings of ROWS, the LDS block shapes and the four-sweep kernel under a forced
# chunk length, ROWS = 8 on fp32, and FUSE = 4 (last: resetting it leaves FL_OPT_JACOBI_FUSE at its default of 1)
EXTENDED_SHAPES = [(256, 256, 128)]
EXTENDED_SETTINGS = ([[(VARIANT, 3)]] + [[(VARIANT, 2), (ROWS, r)] for r in (1, 2, 4)] + [[(VARIANT, 3), (ROWS, r)] for r in (8, 16)] +
                     [[(ROWS, 4), (KCHUNK, k), (KCHUNK2, 8)] for k in (24, 26, 18, 19)] +
                     [[(ROWS, 6), (KCHUNK, k), (KCHUNK2, 8)] for k in (18, 24)] + [[(ROWS, 8)]] +
                     [[(FUSE, 4), (ROWS, 2), (KCHUNK, k)] for k in (1, 2)])


class Level(C.Structure):
    _fields_ = [("ni", C.c_int), ("nj", C.c_int), ("nk", C.c_int), ("number", C.c_int), ("alpha", C.c_double),
                ("beta", C.c_double), ("b", C.c_void_p), ("x", C.c_void_p), ("r", C.c_void_p)]


def run(log_path, extended=False):
    if extended:
        FP32_SHAPES.extend(EXTENDED_SHAPES)
        FP64_SHAPES.extend(EXTENDED_SHAPES)
        FP32_SETTINGS.extend(EXTENDED_SETTINGS)
    sys.path.insert(0, ROOT)
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    log = open(log_path, "w") if log_path else sys.stdout
    owned = []

    def dev(nbytes):
        p = lib.fl_malloc(nbytes)
        assert p, nbytes
        owned.append(p)
        return p

    def release():
        lib.fl_sync()
        for p in owned:
            lib.fl_free(p)
        owned.clear()

    def options(pairs):
        for opt, val in pairs:
            lib.fl_set_option(opt, val)

    def reset(pairs):
        for opt, _ in pairs:
            lib.fl_set_option(opt, 1 if opt == FUSE else (-1 if opt == MGCG_FUSE else 0))

    def note(what, ret=None):
        lib.fl_sync()
        err = ""
        if lib.fl_last_error():             # a refusal is part of the record, not the end of the run
            err = " error: " + lib.fl_last_error_string().decode(errors="replace")
            lib.fl_clear_error()
        print(what, "->", ret, lib.fl_jacobi_kernel_name().decode(), lib.fl_mg_smooth_kernel_name().decode() + err, file=log, flush=True)

    a, b6 = -1.0, 1.0 / 6.0
    for ni, nj, nk in FP32_SHAPES:
        n, nv = ni * nj * nk, (ni + 1) * (nj + 1) * (nk + 1)
        p, t, d = dev(4 * n), dev(4 * n), dev(4 * n)
        u, v, w = dev(4 * nv), dev(4 * nv), dev(4 * nv)
        solid, rows = dev(n), dev(nj * nk)
        tag = f"{ni}x{nj}x{nk}"

        def sweeps(label, counts=(11, 12, 8)):
            for s in counts:
                note(f"{tag} {label} gpu_jacobi_sweeps {s}", lib.gpu_jacobi_sweeps(p, d, t, ni, nj, nk, s, a, b6))

        def projection(label):
            lib.gpu_projection_jacobi(u, v, w, d, p, t, None, ni, nj, nk, 12, 0.5, a, b6)
            note(f"{tag} {label} gpu_projection_jacobi 12")

        def ranges(label):
            for k0, k1 in ((5, nk - 5), (0, 7), (nk - 9, nk), (-3, nk + 3)):
                lib.gpu_jacobi_sweep_range(p, d, t, ni, nj, nk, k0, k1, a, b6)
                note(f"{tag} {label} gpu_jacobi_sweep_range {k0} {k1}")
            for r in ((8, nk - 8, 0, 0), (0, 8, nk - 8, nk), (0, nk, 0, 0), (3, 11, nk - 20, nk - 2), (4, 4, 0, 0), (0, 1 << 30, 0, 0)):
                note(f"{tag} {label} pair_ranges {r}", lib.gpu_jacobi_sweep_pair_ranges(p, d, t, ni, nj, nk, *r, a, b6))
                note(f"{tag} {label} triple_ranges {r}", lib.gpu_jacobi_sweep_triple_ranges(p, d, t, ni, nj, nk, *r, a, b6))

        sweeps("default")
        projection("default")
        ranges("default")
        for f in (0, 2, 4):
            options([(FUSE, f)])
            sweeps(f"fuse={f}")
            projection(f"fuse={f}")
            ranges(f"fuse={f}")
        options([(FUSE, 2)])
        for setting in FP32_SETTINGS:
            options(setting)
            # (FL_OPT_JACOBI_KCHUNK doubles as the one-sweep kernels' chunk length: even sweep counts there, no odd one left over)
            sweeps(f"{setting}", (12, 8) if setting[0][0] == KCHUNK else (11, 12, 8))
            if setting[0][0] != KCHUNK:
                projection(f"{setting}")
            ranges(f"{setting}")
            reset(setting)
        # the masked sweeps (no solid cell: the flags are all zero)
        for f in (1, 2):
            options([(FUSE, f)])
            note(f"{tag} fuse={f} gpu_jacobi_sweeps_masked 11", lib.gpu_jacobi_sweeps_masked(p, d, t, solid, rows, ni, nj, nk, 11, a, b6))
        for k in (19, 24):
            options([(KCHUNK, k)])
            note(f"{tag} kchunk={k} gpu_jacobi_sweeps_masked 9", lib.gpu_jacobi_sweeps_masked(p, d, t, solid, rows, ni, nj, nk, 9, a, b6))
        options([(KCHUNK, 0)])
        lib.gpu_jacobi_sweep_masked(p, d, t, solid, rows, ni, nj, nk, a, b6)
        note(f"{tag} gpu_jacobi_sweep_masked")

        # the walled sweeps on the same zero flags, every side closed but +y: the whole array, plane ranges, the fused triple on ranges
        def walled(label):
            lib.gpu_jacobi_sweep_masked_walls(p, d, t, solid, rows, BOX, ni, nj, nk, a, b6)
            note(f"{tag} {label} gpu_jacobi_sweep_masked_walls")
            for k0, k1 in ((5, nk - 5), (0, 7), (nk - 9, nk), (-3, nk + 3), (4, 4)):
                note(f"{tag} {label} gpu_jacobi_sweep_masked_walls_range {k0} {k1}",
                     lib.gpu_jacobi_sweep_masked_walls_range(p, d, t, solid, rows, BOX, ni, nj, nk, k0, k1, a, b6))
            for r in ((8, nk - 8, 0, 0), (0, 8, nk - 8, nk), (0, nk, 0, 0), (3, 11, nk - 20, nk - 2), (4, 4, 0, 0)):
                note(f"{tag} {label} walls_triple_ranges {r}",
                     lib.gpu_jacobi_sweep_masked_walls_triple_ranges(p, d, t, solid, rows, BOX, ni, nj, nk, *r, a, b6))

        for f in (1, 2):
            options([(FUSE, f)])
            note(f"{tag} fuse={f} gpu_jacobi_sweeps_masked_walls 11", lib.gpu_jacobi_sweeps_masked_walls(p, d, t, solid, rows, BOX, ni, nj, nk, 11, a, b6))
            walled(f"fuse={f}")
        for k in (19, 24):
            options([(KCHUNK, k)])
            note(f"{tag} kchunk={k} gpu_jacobi_sweeps_masked_walls 9", lib.gpu_jacobi_sweeps_masked_walls(p, d, t, solid, rows, BOX, ni, nj, nk, 9, a, b6))
        options([(KCHUNK, 0)])
        note(f"{tag} walls=0 gpu_jacobi_sweeps_masked_walls 9", lib.gpu_jacobi_sweeps_masked_walls(p, d, t, solid, rows, 0, ni, nj, nk, 9, a, b6))
        # a z-slab rank: the same buffers as planes [16, 16 + nk) of nk + 32
        lib.fl_set_slab(16, nk + 32, 24, 8 + nk, nk)
        sweeps("slab")
        ranges("slab")
        note(f"{tag} slab gpu_jacobi_sweeps_masked_walls 11", lib.gpu_jacobi_sweeps_masked_walls(p, d, t, solid, rows, BOX, ni, nj, nk, 11, a, b6))
        walled("slab")
        lib.fl_set_slab(0, 0, 0, 0, 0)
        options([(FUSE, 1)])
        # the other launchers that share the block shape and the lane rule
        lib.gpu_divergence(u, v, w, d, ni, nj, nk, 0.5)
        lib.gpu_gradient(u, v, w, p, ni, nj, nk, 0.5)
        lib.gpu_diffuse_sweeps(d, p, t, ni, nj, nk, 3, 0.1)
        lib.gpu_clamp_extrema_box(p, t, ni, nj, nk)
        lib.gpu_clamp_extrema_box(u, v, ni + 1, nj, nk)
        lib.gpu_clamp_extrema_box_w(u, v, ni, nj, nk + 1)
        lib.gpu_init_maps(p, t, d, 1.0 / ni, ni, nj, nk)
        lib.gpu_add_buoyancy(v, p, t, ni, nj, nk, 0.1, 0.2, 0.01)
        lib.gpu_emit_smoke(u, v, w, p, t, 1.0 / ni, ni, nj, nk, 0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0)
        note(f"{tag} streaming operators")
        release()

    for ni, nj, nk in FP64_SHAPES:
        n = ni * nj * nk
        x, b, t = dev(8 * n), dev(8 * n), dev(8 * n)
        for setting in FP64_SETTINGS:
            options(setting)
            for it in (32, 4, 6):
                lib.gpu_smoothing_jacobi(x, b, t, a, b6, ni, nj, nk, it)
                note(f"{ni}x{nj}x{nk} {setting} gpu_smoothing_jacobi {it}")
            reset(setting)
        release()

    # the multigrid-CG projection with the level-0 vector updates fused into the stencil passes
    ni = nj = nk = 256
    n, levels = ni * nj * nk, 6
    u, v, w = dev(4 * (ni + 1) * nj * nk), dev(4 * ni * (nj + 1) * nk), dev(4 * ni * nj * (nk + 1))
    div, p, dirv, res, t0, t1 = (dev(8 * n) for _ in range(6))
    result = dev(8 * 4096)
    table = (Level * levels)()
    dims = (ni, nj, nk)
    for l in range(levels):
        m = dims[0] * dims[1] * dims[2]
        table[l].ni, table[l].nj, table[l].nk, table[l].number = *dims, m
        table[l].alpha, table[l].beta = -1.0, 1.0 / 6.0
        table[l].b, table[l].x, table[l].r = dev(8 * m), dev(8 * m), dev(8 * m)
        dims = tuple((c - 1) // 2 for c in dims)
    for f in (1, 3):
        options([(MGCG_FUSE, f)])
        lib.gpu_multi_grid_conjugate_gradient(u, v, w, div, p, dirv, res, t0, t1, result, C.addressof(table), levels, 2, 0.5)
        note(f"gpu_multi_grid_conjugate_gradient 256^3 fuse={f}", lib.fl_mg_fused_launches())
    options([(MGCG_FUSE, -1)])
    release()
    print("done", file=log, flush=True)


def step(scene, scheme):
    sys.path.insert(0, ROOT)
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd.scenes import rising_smoke
    from gpufluidsimulation_amd.solver import SCHEME_BIMOCQ, SCHEME_MAC_REFLECTION, BimocqGPUSolver
    n = 64
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0, device=0, scheme=SCHEME_MAC_REFLECTION if scheme == "reflection" else SCHEME_BIMOCQ)
    s.setSmoke(0.0, 1.0, rising_smoke(n, 1.0 / n))
    s.setProjection(20, 0.5)
    if scene == "sphere":
        s.setBoundary([(0, 0.5, 0.5, 0.5, 0.15, 0.0, 0.0, 0.0, 0.0, 0.0)])
    if scene == "box":
        s.setWalls(BOX)
    for f in range(3):
        s.advance(f, 2.0 / n)
    bq.hip_lib().fl_sync()
    bq.check()
    s.close()


def strip_parameters(name):
    """the demangled kernel name without its parameter list (template arguments stay)"""
    if not name.endswith(")"):
        return name
    depth = 0
    for at in range(len(name) - 1, -1, -1):
        depth += (name[at] == ")") - (name[at] == "(")
        if depth == 0:
            return name[:at]
    return name


def reduce(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    launches = [" ".join([strip_parameters(r["Kernel_Name"]), "grid", r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                          "block", r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]]) for r in rows]
    ids, runs = {}, []                          # numbered by first appearance; consecutive repeats as id*count
    for l in launches:
        k = ids.setdefault(l, len(ids))
        if runs and runs[-1][0] == k:
            runs[-1][1] += 1
        else:
            runs.append([k, 1])
    print(f"# {len(launches)} launches, {len(ids)} distinct (kernel, grid, block); the table, then the launches in start order as id*count")
    for l, k in ids.items():
        print(k, l)
    print("#")
    tokens = [f"{k}*{n}" if n > 1 else str(k) for k, n in runs]
    for at in range(0, len(tokens), 24):
        print(" ".join(tokens[at:at + 24]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "step", "reduce"])
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--log", default="")
    ap.add_argument("--extended", action="store_true")
    ap.add_argument("--scene", choices=["plain", "sphere", "box"], default="plain")
    ap.add_argument("--scheme", choices=["bimocq", "reflection"], default="bimocq")
    args = ap.parse_args()
    if args.mode == "run":
        run(args.log, args.extended)
    elif args.mode == "step":
        step(args.scene, args.scheme)
    else:
        reduce(args.trace_dir)
