"""CPU tests of csrc/bq_jacobi_plan.h: the decoder of FL_OPT_JACOBI_VARIANT / _ROWS / _KCHUNK / _KCHUNK2 / _FUSE and the pure
planners by which the sweep launchers (bq_project.hip, bq_obstacle.hip, bq_mgcg.hip) choose kernel, template arguments and
geometry.  The header is compiled with g++ behind tests/cpu_abi/jacobi_plan_shim.cpp and called through ctypes.

test_decoder_matches_scattered_conditions compares the decoder, exhaustively over the option values, with the conditions the
launchers carried at their call sites before the header existed -- restated here in Python from those call sites,
independently of the header.
test_recorded_plans pins the decompositions of the shapes the launchers' comments, the tests and the benchmark run.
test_mg_lds3_split compares the fp64 parity rule with the loop mg_smooth carried."""
import ctypes as C
import itertools

import numpy as np
import pytest

from build_cpu_host import build_jacobi_plan

I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")

FIELDS = ["single", "march_waves", "tile_rows", "single_kchunk", "fused_ok", "pair_rows", "keep_march2r", "prefetch", "fused_kchunk",
          "lds_min_kc", "lds_triple", "lean_triple", "lean_triple_short", "quad", "lds_w3", "lds_r3", "lds_w4", "lds_r4", "masked_triple",
          "triple_ranges", "pair_ranges", "trust", "beyond_pairs", "sweeps_fuse", "mg_keep_smooth2", "mg_smooth2_threads", "mg_lds3_off",
          "mg_lds3_rows"]
PLAN = ["kernel", "wide", "pf", "W", "R", "S", "cw", "col_blocks", "row_blocks", "nbz", "kc", "nblk", "grid", "block"]
# the enums of the header
AUTO, GENERIC, TILE, MARCH = 0, 1, 2, 3                 # Single
P_AUTO, P_NEVER, P_ALWAYS = 0, 1, 2                     # Pair
Q_AUTO, Q_FORCED, Q_NEVER = 0, 1, 2                     # Quad
T_NEVER, T_CHECKED, T_VOUCHED = 0, 1, 2                 # Trust
F_NONE, F_PAIRS, F_ALL = 0, 1, 2                        # SweepsFuse
K = dict(none=0, empty=1, generic=2, march=3, tile=4, lean2r=5, march2r=6, march2=7, lds=8, lds2seg=9, lean3r=10)
SINGLE, PAIR, LDS, QUAD, LEAN3, TRIPLE, MASKED, TRIPLE_RANGES = range(8)        # the planners of the shim


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(build_jacobi_plan(), mode=C.RTLD_LOCAL)
    for name in ("plan_decode", "plan_launch", "plan_mg_lds3_split"):
        fn = getattr(so, name)
        fn.restype, fn.argtypes = None, [C.c_int, I32P, I32P]

    def call(name, rows, width):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((rows.shape[0], width), dtype=np.int32)
        getattr(so, name)(rows.shape[0], rows, out)
        return out
    return call


# ---- the conditions as the launchers carried them, one expression per reader ---------------------------------------------------
def scattered(variant, rows, kchunk, kchunk2, fuse):
    f = {}
    # jacobi_sweep: variant 0 -> 3 where float4 rows apply, else 1; 1 generic; 3 march; the rest falls through to the tile kernel
    f["single"] = {0: AUTO, 1: GENERIC, 3: MARCH}.get(variant, TILE)
    f["march_waves"] = rows if rows in (4, 8, 16) else 4                 # if (waves != 4 && waves != 8 && waves != 16) waves = 4
    f["tile_rows"] = rows if rows in (1, 2, 4) else 4                    # if (R != 1 && R != 2 && R != 4) R = 4
    f["single_kchunk"] = kchunk if kchunk > 0 else 0                     # if (opt_jacobi_kchunk > 0) kchunk = opt_jacobi_kchunk
    fused_ok = variant in (0, 3)                                         # if (variant != 0 && variant != 3) return false
    f["fused_ok"] = fused_ok
    # jacobi_sweep_pair: if (nj >= 4 && rows != 1) ...; if (pays || rows == 2); if (rows != 3) lean2r else march2r
    f["pair_rows"] = P_NEVER if rows == 1 else P_ALWAYS if rows == 2 else P_AUTO
    f["keep_march2r"] = rows == 3
    f["prefetch"] = kchunk if kchunk in (1, 2) else 0                    # pf = forced == 1 || forced == 2 ? forced : (in_cache ? 1 : 2)
    f["fused_kchunk"] = kchunk2 if kchunk2 > 0 else 0
    f["lds_min_kc"] = 8 if kchunk2 > 0 else 24                           # kc >= (opt_jacobi_kchunk2 > 0 ? 8 : 24)
    # jacobi_sweep_triple: (rows == 4 || 6 || 0 || 7) && fused variant && jacobi_sweep_lds(...); then rows == 1 || rows == 3 -> false;
    # kc < 16 && rows != 2 -> false
    f["lds_triple"] = rows in (4, 6, 0, 7)
    f["lean_triple"] = rows not in (1, 3)
    f["lean_triple_short"] = rows == 2
    # jacobi_sweep_quad: (rows != 6 && rows != 0) || not a fused variant -> false; rows == 6 -> no minimum
    f["quad"] = Q_NEVER if (rows not in (6, 0) or not fused_ok) else Q_FORCED if rows == 6 else Q_AUTO
    # jacobi_sweep_lds: shape = 10 R + W
    for S in (3, 4):
        shape = kchunk
        if shape not in (24, 25, 26, 18, 19):
            shape = 24 if S == 4 else 18
        if S == 4 and shape not in (24, 18):
            shape = 24
        f[f"lds_r{S}"] = shape // 10
        f[f"lds_w{S}"] = 12 if shape == 19 else (6 if S == 4 and shape == 18 else shape % 10)
    f["masked_triple"] = kchunk not in (24, 25, 26, 19)
    # gpu_jacobi_sweep_triple_ranges / _pair_ranges
    f["triple_ranges"] = not (fuse == 0 or fuse == 4 or rows == 5) and fused_ok
    f["pair_ranges"] = not fuse == 0
    # gpu_projection_jacobi: fuse >= 2 || (fuse == 1 && shells match); triples: fuse != 4
    f["trust"] = T_VOUCHED if fuse >= 2 else T_CHECKED if fuse == 1 else T_NEVER
    f["beyond_pairs"] = fuse != 4
    # gpu_jacobi_sweeps: quads and triples fuse >= 2 && fuse != 4, pairs fuse >= 2
    f["sweeps_fuse"] = F_ALL if (fuse >= 2 and fuse != 4) else F_PAIRS if fuse >= 2 else F_NONE
    # mg_smooth
    f["mg_keep_smooth2"] = not (rows != 3 and rows != 8)
    f["mg_smooth2_threads"] = 512 if rows == 8 else 256
    f["mg_lds3_off"] = not rows != 5
    f["mg_lds3_rows"] = 4 if kchunk == 14 else 8
    return [int(f[name]) for name in FIELDS]


def test_decoder_matches_scattered_conditions(lib):
    cases = list(itertools.product(range(-1, 6), range(-1, 18), [0, 1, 2, 3, 8, 14, 16, 18, 19, 24, 25, 26, 27, 32],
                                   [0, 1, 8, 16, 24, 40], range(-1, 6)))
    got = lib("plan_decode", cases, len(FIELDS))
    want = np.array([scattered(*c) for c in cases], dtype=np.int32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(cases[r], FIELDS[c], int(got[r, c]), int(want[r, c])) for r, c in bad[:5]]
    # every listed meaning of every field occurs in the sweep
    for col, name in enumerate(FIELDS):
        assert len(np.unique(want[:, col])) >= 2, name


def plan(lib, planner, dims, *, aligned=True, ranges=(0, 1 << 30, 0, 0), variant=0, rows=0, kchunk=0, kchunk2=0, fuse=2, cus=256, slab=False,
         S=3, masked=False, min_kc=0):
    row = [planner, *dims, int(aligned), *ranges, variant, rows, kchunk, kchunk2, fuse, cus, int(slab), S, int(masked), min_kc]
    return dict(zip(PLAN, (int(v) for v in lib("plan_launch", [row], len(PLAN))[0])))


def check(p, kernel, **want):
    assert p["kernel"] == K[kernel], (p, kernel)
    for name, value in want.items():
        assert p[name] == value, (name, p)


def test_recorded_plans(lib):
    """256 CUs, default options unless stated"""
    n256, n128, n512 = (256, 256, 256), (128, 128, 128), (512, 512, 512)
    # 256^3: quad <4, 2, 4> and triple <8, 1, 3> on 32 row blocks x 8 chunks of 32 planes
    check(plan(lib, QUAD, n256), "lds", W=4, R=2, S=4, row_blocks=32, nbz=8, kc=32, grid=256, block=512)
    check(plan(lib, TRIPLE, n256), "lds", W=8, R=1, S=3, row_blocks=32, nbz=8, kc=32, grid=256, block=768)
    check(plan(lib, PAIR, n256), "lean2r", wide=0, pf=1, row_blocks=32, nbz=8, kc=32, grid=256, block=256)
    check(plan(lib, SINGLE, n256), "march", W=4, cw=64, col_blocks=1, row_blocks=64, kc=16, nbz=16, grid=1024, block=256)
    # 128^3: the LDS kernels' chunks come out at 8 planes, the lean triple's at 4: neither applies; the pair runs 8 x 32 chunks of 4
    check(plan(lib, QUAD, n128), "none")
    check(plan(lib, TRIPLE, n128), "none")
    assert plan(lib, LDS, n128, S=3, kchunk2=8)["kc"] == 8 and plan(lib, LDS, n128, S=3)["kernel"] == K["none"]
    check(plan(lib, LEAN3, n128, rows=2), "lean3r", kc=4)           # (what the rule gives, shown by admitting short chunks)
    check(plan(lib, LEAN3, n128), "none")
    check(plan(lib, PAIR, n128), "lean2r", wide=0, pf=1, row_blocks=8, nbz=32, kc=4, grid=256, block=256)
    # 256 x 256 x 128: the LDS kernels refuse with chunks of 16 planes, jacobi_lean3r_kernel<1> runs 32 x 8 chunks of 16
    d = (256, 256, 128)
    check(plan(lib, QUAD, d), "none")
    check(plan(lib, LDS, d, S=3), "none")
    check(plan(lib, LDS, d, S=3, kchunk2=16), "lds", kc=16)         # (the rule's own chunk length, admitted when forced)
    check(plan(lib, LDS, d, S=3, ranges=(8, 120, 0, 0)), "lds", kc=14)     # (plane ranges know no minimum)
    check(plan(lib, TRIPLE, d), "lean3r", pf=1, S=3, row_blocks=32, nbz=8, kc=16, grid=256, block=256)
    check(plan(lib, TRIPLE, d, kchunk=2), "lean3r", pf=2)
    # 64 x 256 x 192: quad with chunks of 24, the threshold of the auto rule
    check(plan(lib, QUAD, (64, 256, 192)), "lds", W=4, R=2, S=4, row_blocks=32, nbz=8, kc=24, grid=256, block=512)
    # 512^3: the two-segment kernel, 64 row blocks x 4 chunks of 128 planes; pair <true, 2>: 128 x 6 chunks of 86
    check(plan(lib, TRIPLE, n512), "lds2seg", W=8, R=1, S=3, row_blocks=64, nbz=4, kc=128, grid=256, block=768)
    check(plan(lib, QUAD, n512), "none")
    check(plan(lib, PAIR, n512), "lean2r", wide=1, pf=2, cw=128, row_blocks=128, nbz=6, kc=86, grid=768, block=256)
    # 512 x 512 x 64: the two-segment kernel refuses with chunks of 16; pair <true, 1>: 128 x 2 chunks of 32
    d = (512, 512, 64)
    check(plan(lib, TRIPLE, d), "none")
    check(plan(lib, LDS, d, S=3, kchunk2=16), "lds2seg", kc=16)
    check(plan(lib, PAIR, d), "lean2r", wide=1, pf=1, row_blocks=128, nbz=2, kc=32, grid=256)
    # 320 x 64 x 48 and 1024 x 1024 x 80
    check(plan(lib, PAIR, (320, 64, 48)), "lean2r", wide=1, pf=1, row_blocks=16, nbz=16, kc=3, grid=256)
    check(plan(lib, PAIR, (1024, 1024, 80)), "lean2r", wide=1, pf=2, cw=256, row_blocks=512, nbz=1, kc=80, grid=512)

    # FL_OPT_JACOBI_ROWS = 6: quads wherever the kernel applies, also on a z-slab rank and below 24 planes per chunk once forced
    check(plan(lib, QUAD, n256, rows=6, slab=True), "lds", S=4, kc=32)
    check(plan(lib, QUAD, n256, slab=True), "none")
    check(plan(lib, QUAD, n256, rows=6, kchunk2=8), "lds", S=4, kc=8, nbz=32, grid=1024)
    check(plan(lib, QUAD, n256, kchunk2=8), "none")                  # auto: a forced chunk length below 24 keeps the triples
    check(plan(lib, TRIPLE, n256, kchunk2=8), "lds", S=3, kc=8, nbz=32, grid=1024)
    check(plan(lib, QUAD, n128, rows=6), "none")
    # ROWS = 7: auto without quads; 5: no LDS triple; 1 / 3: no lean triple either
    check(plan(lib, QUAD, n256, rows=7), "none")
    check(plan(lib, TRIPLE, n256, rows=7), "lds", S=3)
    check(plan(lib, TRIPLE, n256, rows=5), "lean3r", kc=32, nbz=8, row_blocks=32)
    check(plan(lib, TRIPLE, n256, rows=1), "none")
    check(plan(lib, TRIPLE, n256, rows=3), "none")
    check(plan(lib, TRIPLE_RANGES, n256, rows=5), "none")
    check(plan(lib, TRIPLE_RANGES, n256, rows=1), "lds", S=3)       # (it honours 5 only)
    check(plan(lib, TRIPLE_RANGES, n256, fuse=4), "none")
    check(plan(lib, TRIPLE_RANGES, n256, ranges=(4, 4, 0, 0)), "empty")
    # each block-shape code of FL_OPT_JACOBI_KCHUNK, three and four sweeps: (W, R, rows per block -> row blocks, threads)
    for code, (w, r, blk) in {18: (8, 1, 768), 19: (12, 1, 1024), 24: (4, 2, 384), 25: (5, 2, 448), 26: (6, 2, 512), 0: (8, 1, 768)}.items():
        nby = (256 + w * r - 1) // (w * r)
        kc = (256 + 256 // nby - 1) // (256 // nby)
        check(plan(lib, TRIPLE, n256, kchunk=code), "lds", W=w, R=r, S=3, row_blocks=nby, kc=kc, block=blk, nblk=nby * ((256 + kc - 1) // kc))
    for code, (w, r, blk) in {18: (6, 1, 768), 19: (4, 2, 512), 24: (4, 2, 512), 25: (4, 2, 512), 26: (4, 2, 512), 0: (4, 2, 512)}.items():
        check(plan(lib, QUAD, n256, rows=6, kchunk=code), "lds", W=w, R=r, S=4, block=blk)
    check(plan(lib, TRIPLE, n256, kchunk=26), "lds", row_blocks=22, kc=24, nbz=11, nblk=242, grid=248)
    # the masked triple: the default shape only, never on a z-slab rank, whatever ROWS says
    check(plan(lib, MASKED, n256, rows=5), "lds", W=8, R=1, S=3, block=768, kc=32)
    check(plan(lib, MASKED, n256, kchunk=18), "lds", W=8, R=1)
    for code in (19, 24, 25, 26):
        check(plan(lib, MASKED, n256, kchunk=code), "none")
    check(plan(lib, MASKED, n256, slab=True), "none")
    check(plan(lib, MASKED, n512), "none")
    # 248 CUs (FL_OPT_RESERVE_CUS = 8) at 256^3: one block per CU becomes 7 chunks of 37 planes; the pair takes chunks_for_cus
    check(plan(lib, QUAD, n256, cus=248), "lds", S=4, row_blocks=32, kc=37, nbz=7, nblk=224, grid=224)
    check(plan(lib, TRIPLE, n256, cus=248), "lds", S=3, kc=37, nbz=7)
    p = plan(lib, PAIR, n256, cus=248)
    check(p, "lean2r", row_blocks=32)
    assert p["nbz"] == (256 + p["kc"] - 1) // p["kc"] and 32 * p["nbz"] <= 248
    # the short-range rule (longest <= 48) on a two-range launch: 2 ranges x 32 row blocks x 4 chunks of 2 planes fill 256 CUs once
    check(plan(lib, PAIR, n256, ranges=(0, 8, 248, 256)), "lean2r", row_blocks=32, kc=2, nbz=8, grid=256)
    check(plan(lib, PAIR, n256, ranges=(3, 11, 236, 254)), "lean2r", kc=5, nbz=6, grid=192)
    check(plan(lib, PAIR, n256, ranges=(8, 248, 0, 0)), "lean2r", kc=30, nbz=8)         # a long range: the whole-round rule on 240 planes
    check(plan(lib, PAIR, n256, ranges=(0, 8, 248, 256), rows=1), "march2", kc=8, nbz=2, row_blocks=64, grid=128)
    check(plan(lib, PAIR, n256, ranges=(4, 4, 0, 0)), "empty")
    # the pair's other codes, and what keeps every fused kernel off
    check(plan(lib, PAIR, n256, rows=3), "march2r", wide=0, row_blocks=32, kc=32, grid=256)
    check(plan(lib, PAIR, n256, rows=1), "march2", wide=0, row_blocks=64, kc=32, nbz=8, grid=512)
    check(plan(lib, PAIR, n256, kchunk=2), "lean2r", pf=2)
    check(plan(lib, PAIR, n256, kchunk2=8), "lean2r", kc=8, nbz=32, grid=1024)
    for planner in (PAIR, TRIPLE, QUAD, TRIPLE_RANGES):
        check(plan(lib, planner, n256, variant=1), "none")
        check(plan(lib, planner, n256, variant=2), "none")
        assert plan(lib, planner, n256, variant=3) == plan(lib, planner, n256)
        check(plan(lib, planner, n256, aligned=False), "none")
    check(plan(lib, PAIR, (30, 30, 30)), "none")
    # one sweep: the variants, ROWS as waves per block / rows per thread, KCHUNK as the chunk length -- 24 included
    check(plan(lib, SINGLE, n256, variant=1), "generic")
    check(plan(lib, SINGLE, n256, aligned=False), "generic")
    check(plan(lib, SINGLE, n256, variant=3, aligned=False), "generic")
    check(plan(lib, SINGLE, (30, 30, 30)), "generic")
    check(plan(lib, SINGLE, (2, 30, 30)), "empty")
    check(plan(lib, SINGLE, n256, variant=3, rows=8), "march", W=8, cw=64, row_blocks=32, block=512)
    check(plan(lib, SINGLE, n256, variant=3, rows=16), "march", W=16, row_blocks=16, block=1024)
    check(plan(lib, SINGLE, n256, variant=3, rows=2), "march", W=4, block=256)
    check(plan(lib, SINGLE, n256, kchunk=24), "march", kc=24, nbz=11, grid=704)
    check(plan(lib, SINGLE, n128), "march", cw=32, row_blocks=16, kc=4, nbz=32, grid=512)      # (halved from 16 while under 1024 blocks)
    check(plan(lib, SINGLE, n256, variant=2), "tile", wide=1, R=4, col_blocks=1, row_blocks=16, kc=8, nbz=32, grid=512, block=256)
    check(plan(lib, SINGLE, n256, variant=2, rows=1), "tile", R=1, row_blocks=64, kc=16, nbz=16)
    check(plan(lib, SINGLE, n256, variant=2, rows=2), "tile", R=2, row_blocks=32)
    check(plan(lib, SINGLE, n128, variant=2, kchunk=24), "tile", wide=0, R=4, row_blocks=4, kc=24, nbz=6)
    check(plan(lib, SINGLE, n256, variant=5), "tile")


def test_mg_lds3_split(lib):
    def loop(it, s, zin):
        """mg_smooth: for (a = (iter - s) / 3; a >= 0 && triples < 0; a--) { rest = iter - s - 3 a;
        if (rest % 2 == 0 && (zin || (rest / 2 + a) % 2 == 0)) triples = a; } pairs = (iter - s - 3 triples) / 2;
        if (zin && (pairs + triples) % 2 == 1) swap"""
        triples = -1
        a = (it - s) // 3
        while a >= 0 and triples < 0:
            rest = it - s - 3 * a
            if rest % 2 == 0 and (zin or (rest // 2 + a) % 2 == 0):
                triples = a
            a -= 1
        if triples < 0:
            return [-1, 0, 0]
        pairs = (it - s - 3 * triples) // 2
        return [triples, pairs, int(zin and (pairs + triples) % 2 == 1)]
    cases = [(it, 0, z) for it in range(0, 41) for z in (0, 1)] + [(it, 2, z) for it in range(2, 41) for z in (0, 1)]
    got = lib("plan_mg_lds3_split", cases, 3)
    assert got.tolist() == [loop(*c) for c in cases]
    by_case = {c: tuple(int(v) for v in g) for c, g in zip(cases, got)}
    assert by_case[(32, 0, 1)] == (10, 1, 1)        # from a cleared x: 10 triples + 1 pair, the first launch writes into x
    assert by_case[(4, 0, 0)] == (0, 2, 0)          # 4 sweeps = 2 pairs
    assert by_case[(32, 0, 0)] == (8, 4, 0)         # an even number of launches
    assert by_case[(7, 0, 1)] == (1, 2, 1)          # free of the parity rule: 3 + 2 + 2
    assert by_case[(7, 0, 0)] == (-1, 0, 0)         # 3 + 2 + 2 is an odd number of launches, and nothing else makes 7
    for (it, s, z), (t, p, sw) in by_case.items():
        if t >= 0:
            assert 3 * t + 2 * p == it - s and (z or (t + p) % 2 == 0)
