"""CPU tests of the WALLED mode of csrc/host/slab_jacobi_plan.hpp (DESIGN.md sections 7.2 and 18): a chunk of the z-slab Jacobi
projection for the walled kernel family, which has one sweep or three per launch and no pairs.  Exhaustive over G 1..10, 5..40
owned planes, 1..30 sweeps left and the option bits; inputs without the walled flag must give what the function gave before the
mode existed, restated here from that version."""
import ctypes as C
import itertools

import numpy as np
import pytest

from build_cpu_walls_slab import build_slab_jacobi_plan_walled

I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
IN = ["left", "G", "owned", "pairs_ok", "triples_ok", "overlap", "ends_first_on", "triples_on", "walled"]
OUT = ["sweeps", "first", "S", "fused", "rest", "ends_first", "d_first", "d_last"]


@pytest.fixture(scope="module")
def plan():
    so = C.CDLL(build_slab_jacobi_plan_walled(), mode=C.RTLD_LOCAL)
    so.slab_plan_chunk_walled.restype, so.slab_plan_chunk_walled.argtypes = None, [C.c_int, I32P, I32P]

    def call(rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((rows.shape[0], len(OUT)), dtype=np.int32)
        so.slab_plan_chunk_walled(rows.shape[0], rows, out)
        return {**{n: rows[:, i] for i, n in enumerate(IN)}, **{n: out[:, i] for i, n in enumerate(OUT)}}
    return call


def cases(walled):
    return np.array([(left, G, owned, *flags, walled) for G in range(1, 11) for owned in range(5, 41) for left in range(1, 31)
                     for flags in itertools.product((0, 1), repeat=5)], dtype=np.int32)


@pytest.fixture(scope="module")
def every(plan):
    return plan(cases(1))


def test_passes_add_up_and_are_singles_and_triples(every):
    e = every
    assert np.all(e["first"] + 3 * e["fused"] + e["rest"] == e["sweeps"])
    assert np.all((e["sweeps"] >= 1) & (e["sweeps"] <= np.minimum(e["left"], e["G"])))
    assert np.all(e["first"] == 1) and np.all(e["S"] == 3) and np.all(e["fused"] >= 0)
    assert np.all((e["rest"] >= 0) & ((e["rest"] < 3) | (e["fused"] == 0)))
    # the pairs permission is not read
    a, b = e["pairs_ok"] == 0, e["pairs_ok"] == 1
    for n in OUT:
        assert np.array_equal(e[n][a], e[n][b])
    # triples unless switched off or refused
    on = (e["triples_on"] == 1) & (e["triples_ok"] == 1)
    assert np.all(e["fused"][~on] == 0) and np.all(e["fused"][on & (e["sweeps"] >= 4)] >= 1)


def test_every_pass_has_the_ghost_depth_it_needs(every):
    e = every
    have = e["G"] - 1                                           # after the first single sweep
    some = e["fused"] > 0
    assert np.all(e["d_first"][some] + 3 == have[some])         # the first triple uses what the single sweep left
    assert np.all(e["d_first"][some] - e["d_last"][some] == 3 * (e["fused"][some] - 1))
    assert np.all(e["d_last"][some] >= 0)
    assert np.all(e["rest"] <= np.where(some, e["d_last"], have))      # the whole-array tail leaves the owned planes correct
    assert np.all(e["G"] - e["sweeps"] >= 0)                    # the depth after the last pass


def test_ends_first_only_under_its_preconditions(every):
    """two triples that close the chunk, a full exchange used up to the `cut` sweeps the chunk gives up, another chunk that
    would follow anyway (the cut must not buy an exchange of its own), and a slab tall enough for two ends and an interior of 2 planes at the depth 3 + cut the first triple leaves"""
    e = every
    cut = (e["G"] - 1) % 3
    want = ((e["overlap"] == 1) & (e["ends_first_on"] == 1) & (e["triples_on"] == 1) & (e["triples_ok"] == 1) & (e["G"] >= 7) &
            (e["left"] > e["G"]) & (e["owned"] >= 2 * e["G"] + 2 * (3 + cut) + 2))
    assert np.array_equal(e["ends_first"] == 1, want)
    ef = e["ends_first"] == 1
    assert ef.any()
    assert np.all(e["fused"][ef] >= 2) and np.all(e["rest"][ef] == 0) and np.all(e["sweeps"][ef] == (e["G"] - cut)[ef])
    assert np.all(e["d_last"][ef] == cut[ef])
    # the interior of the second-to-last pass, [own0 + G + d, own1 - G - d) with d = d_last + 3, keeps two planes
    assert np.all(e["owned"][ef] - 2 * e["G"][ef] - 2 * (e["d_last"][ef] + 3) >= 2)
    # without ends first a chunk takes all it can
    assert np.all(e["sweeps"][~ef] == np.minimum(e["left"], e["G"])[~ef])


def test_chunk_shapes_of_the_design_table(plan):
    def chunk(left, G, owned, triples_ok=1, overlap=1, ends_first=1, triples=1):
        r = plan([(left, G, owned, 1, triples_ok, overlap, ends_first, triples, 1)])
        return [1] + [3] * int(r["fused"][0]) + ([int(r["rest"][0])] if r["rest"][0] else []), bool(r["ends_first"][0])
    assert chunk(199, 8, 64) == ([1, 3, 3], True)               # G = 8: 7 sweeps per exchange, as the unwalled single-sweep mode
    assert chunk(199, 8, 25) == ([1, 3, 3, 1], False)           # too short for two ends and an interior: the whole chunk, plain
    assert chunk(199, 8, 26) == ([1, 3, 3], True)
    assert chunk(8, 8, 64) == ([1, 3, 3, 1], False)             # no chunk follows
    assert chunk(7, 8, 64) == ([1, 3, 3], False)
    assert chunk(199, 8, 64, ends_first=0) == ([1, 3, 3, 1], False)
    assert chunk(199, 8, 64, overlap=0) == ([1, 3, 3, 1], False)
    assert chunk(199, 8, 64, triples=0) == ([1, 7], False)
    assert chunk(199, 8, 64, triples_ok=0) == ([1, 7], False)
    assert chunk(29, 6, 16) == ([1, 3, 2], False)               # the multi-rank tests' shape
    assert chunk(5, 6, 16) == ([1, 3, 1], False)
    assert chunk(199, 7, 64) == ([1, 3, 3], True)               # G = 7 ends exactly on the owned planes
    assert chunk(199, 10, 64) == ([1, 3, 3, 3], True)
    assert chunk(1, 8, 64) == ([1], False)


def parent_plan_chunk(left, G, owned, pairs_ok, triples_ok, overlap, ends_first, triples):
    """plan_chunk as it was before the walled mode, line for line"""
    sweeps = min(left, G)
    first = 2 if pairs_ok and sweeps >= 2 else 1
    if first == 1:
        sweeps = min(left, G - 1 if G % 2 == 0 and G > 1 else G)
    after = sweeps - first
    full = sweeps == G
    S = 3 if first == 2 and triples and triples_ok and G == 8 and full else 2
    fused = after // S if first == 2 else 0
    rest = after - fused * S
    ef = bool(overlap and ends_first and first == 2 and G >= 6 and G % 2 == 0 and owned >= 2 * G + 8 and full and left > sweeps)
    return sweeps, first, S, fused, rest, int(ef), G - first - S, G - first - fused * S


def test_inputs_without_the_flag_give_what_they_gave(plan):
    rows = cases(0)
    e = plan(rows)
    want = np.array([parent_plan_chunk(*(int(x) for x in r[:8])) for r in rows], dtype=np.int32)
    for i, n in enumerate(OUT):
        assert np.array_equal(e[n], want[:, i]), n
