"""CPU tests of csrc/host/slab_jacobi_plan.hpp: one chunk of the z-slab Jacobi projection as a list of passes (DESIGN.md section
7.2) and the plane ranges of a pass.  The header is compiled with g++ behind tests/cpu_abi/slab_jacobi_plan_shim.cpp and called
through ctypes.  Exhaustive over G 1..8, 5..40 owned planes, 1..3 G sweeps left and every combination of the five flags; that the
host solver issues the plan the way it did before the header existed is tests/test_slab_jacobi_trace_cpu.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

from build_cpu_host import build_slab_jacobi_plan

I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
IN = ["left", "G", "owned", "pairs_ok", "triples_ok", "overlap", "ends_first_on", "triples_on"]
OUT = ["sweeps", "first", "S", "fused", "rest", "ends_first", "d_first", "d_last"]
PLANES = ["whole", "end_a", "end_b", "interior", "first_interior", "first_end_a", "first_end_b"]


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(build_slab_jacobi_plan(), mode=C.RTLD_LOCAL)

    def call(name, rows, width):
        fn = getattr(so, name)
        fn.restype, fn.argtypes = None, [C.c_int, I32P, I32P]
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((rows.shape[0], width), dtype=np.int32)
        fn(rows.shape[0], rows, out)
        return out
    return call


@pytest.fixture(scope="module")
def every(lib):
    """every case, inputs and plan as dicts of columns"""
    rows = [(left, G, owned, *flags) for G in range(1, 9) for owned in range(5, 41) for left in range(1, 3 * G + 1)
            for flags in itertools.product((0, 1), repeat=5)]
    rows = np.array(rows, dtype=np.int32)
    out = lib("slab_plan_chunk", rows, len(OUT))
    return {**{n: rows[:, i] for i, n in enumerate(IN)}, **{n: out[:, i] for i, n in enumerate(OUT)}}


def planes(lib, G, owned, d, first=2):
    row = lib("slab_pass_planes", [(G, owned, d, first)], 14)[0]
    return {n: (int(row[2 * i]), int(row[2 * i + 1])) for i, n in enumerate(PLANES)}


def test_passes_add_up_to_the_chunk(every):
    e = every
    assert np.all(e["first"] + e["fused"] * e["S"] + e["rest"] == e["sweeps"])
    assert np.all((e["sweeps"] >= 1) & (e["sweeps"] <= np.minimum(e["left"], e["G"])))
    assert np.all(np.isin(e["first"], (1, 2)) & np.isin(e["S"], (2, 3)) & (e["fused"] >= 0) & (e["rest"] >= 0))
    assert np.all(e["first"] <= e["sweeps"])
    # two-sweep launches only where they are allowed; the single-sweep mode fuses nothing
    assert np.all((e["first"] == 1) | (e["pairs_ok"] == 1))
    assert np.all((e["first"] == 2) | (e["fused"] == 0))
    # what the tail takes is less than one fused pass wherever passes are planned
    assert np.all((e["first"] == 1) | (e["rest"] < e["S"]))


def test_every_pass_has_the_ghost_depth_it_needs(every):
    """the exchange leaves G correct ghost planes; a pass of S sweeps whose output is correct to depth d needs its input correct to
    d + S; the tail's gpu_jacobi_sweeps must leave the owned planes (depth 0) correct"""
    e = every
    have = e["G"] - e["first"]                                  # after the first pass
    assert np.all(have >= 0)
    some = e["fused"] > 0
    assert np.all(e["d_first"][some] + e["S"][some] <= have[some])                      # the first fused pass reads what the first pass left
    assert np.all(e["d_first"][some] - e["d_last"][some] == (e["fused"][some] - 1) * e["S"][some])      # each next one S planes less
    assert np.all(e["d_last"][some] >= 0)
    left_for_tail = np.where(some, e["d_last"], have)
    assert np.all(e["rest"] <= left_for_tail)
    # a full chunk uses the exchange up: its last pass ends on the owned planes
    full_fused = some & (e["sweeps"] == e["G"]) & (e["rest"] == 0)
    assert np.all(e["d_last"][full_fused] == 0)


def test_triples_only_for_full_chunks_of_eight(every):
    e = every
    want = (e["first"] == 2) & (e["triples_on"] == 1) & (e["triples_ok"] == 1) & (e["G"] == 8) & (e["sweeps"] == 8)
    assert np.array_equal(e["S"] == 3, want)
    assert np.all(e["fused"][e["S"] == 3] == 2) and np.all(e["rest"][e["S"] == 3] == 0)


def test_single_sweep_mode_takes_an_odd_chunk(every):
    e = every
    single = e["first"] == 1
    cap = np.where((e["G"] % 2 == 0) & (e["G"] > 1), e["G"] - 1, e["G"])
    assert np.all(e["sweeps"][single] == np.minimum(e["left"], cap)[single])
    assert np.all(e["sweeps"][~single] == np.minimum(e["left"], e["G"])[~single])
    assert np.array_equal(single, (e["pairs_ok"] == 0) | (np.minimum(e["left"], e["G"]) < 2))


def test_ends_first_only_under_its_preconditions(every):
    e = every
    want = ((e["overlap"] == 1) & (e["ends_first_on"] == 1) & (e["first"] == 2) & (e["G"] >= 6) & (e["G"] % 2 == 0) &
            (e["owned"] >= 2 * e["G"] + 8) & (e["sweeps"] == e["G"]) & (e["left"] > e["sweeps"]))
    assert np.array_equal(e["ends_first"] == 1, want)
    ef = e["ends_first"] == 1
    assert ef.any()
    # the group is the last two passes, and they end exactly on the owned planes
    assert np.all(e["fused"][ef] >= 2) and np.all(e["rest"][ef] == 0) and np.all(e["d_last"][ef] == 0)


def test_ends_and_interiors_tile_the_pass(every, lib):
    e = every
    ef = e["ends_first"] == 1
    shapes = sorted(set(zip(e["G"][ef].tolist(), e["owned"][ef].tolist(), e["S"][ef].tolist())))
    assert (8, 24, 3) in shapes and (8, 24, 2) in shapes and (6, 20, 2) in shapes
    for G, owned, S in shapes:
        own0, own1 = G, G + owned
        a, b = planes(lib, G, owned, S), planes(lib, G, owned, 0)            # the second-to-last and the last pass
        for pl, d in ((a, S), (b, 0)):
            assert pl["whole"] == (own0 - d, own1 + d)
            assert pl["end_a"][0] == pl["whole"][0] and pl["end_a"][1] == pl["interior"][0]          # no gap, no overlap
            assert pl["interior"][1] == pl["end_b"][0] and pl["end_b"][1] == pl["whole"][1]
            assert pl["interior"][0] < pl["interior"][1]
            assert pl["whole"][0] >= 0 and pl["whole"][1] <= owned + 2 * G
        # the last pass's ends are the planes the neighbours receive
        assert b["end_a"] == (own0, own0 + G) and b["end_b"] == (own1 - G, own1)
        # the last pass's ends overwrite the buffer the second-to-last pass's interior still has to read: that interior's
        # S-sweep stencil must stay clear of them
        assert a["interior"][0] - S >= b["end_a"][1] and a["interior"][1] + S <= b["end_b"][0]
    # the edge: 2 G + 8 owned planes leave interiors of 2 (triples) / 4 (pairs) and 8 planes
    assert planes(lib, 8, 24, 3)["interior"] == (19, 21) and planes(lib, 8, 24, 2)["interior"] == (18, 22)
    assert planes(lib, 8, 24, 0)["interior"] == (16, 24)


def test_first_pass_planes(lib):
    """the part out of the ghost planes' reach while they travel, then both ends in whole (the kernels clip at the array's ends)"""
    for G, owned, first in ((8, 24, 2), (8, 24, 1), (5, 11, 2), (2, 5, 2)):
        pl = planes(lib, G, owned, 0, first)
        assert pl["first_interior"] == (G + first, G + owned - first) and pl["first_interior"][0] < pl["first_interior"][1]
        assert pl["first_end_a"] == (0, G + first) and pl["first_end_b"] == (G + owned - first, owned + 2 * G)


def test_chunk_shapes_of_the_design_table(lib):
    def chunk(left, G, owned, pairs_ok=1, triples_ok=1, overlap=1, ends_first=1, triples=1):
        r = lib("slab_plan_chunk", [(left, G, owned, pairs_ok, triples_ok, overlap, ends_first, triples)], len(OUT))[0]
        sweeps, first, S, fused, rest, ef = (int(x) for x in r[:6])
        return [first] + [S] * fused + ([rest] if rest else []), bool(ef)
    assert chunk(35, 8, 24) == ([2, 3, 3], True)
    assert chunk(35, 8, 23) == ([2, 3, 3], False)
    assert chunk(35, 8, 24, triples=0) == ([2, 2, 2, 2], True)
    assert chunk(35, 8, 24, triples_ok=0) == ([2, 2, 2, 2], True)               # the first triple was refused
    assert chunk(8, 8, 24) == ([2, 3, 3], False)                                # no chunk follows
    assert chunk(19, 6, 20) == ([2, 2, 2], True)
    assert chunk(15, 6, 12) == ([2, 2, 2], False)
    assert chunk(35, 8, 24, pairs_ok=0) == ([1, 6], False)                      # single-sweep mode: 1 + 6
    assert chunk(11, 5, 11) == ([2, 2, 1], False)                               # odd G: two pairs and a tail
    # short last chunks, as they fall out of the rules
    assert chunk(3, 8, 24) == ([2, 1], False)
    assert chunk(7, 8, 24) == ([2, 2, 2, 1], False)
    assert chunk(6, 8, 24) == ([2, 2, 2], False)
    assert chunk(2, 8, 24) == ([2], False)
    assert chunk(1, 8, 24) == ([1], False)
