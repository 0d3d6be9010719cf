"""The z-slab Jacobi projection's schedule, call for call: which sweep launches on which plane ranges, which exchanges and which
waits a projection issues, in order, on every rank.  Bit-identical fields do not show that a schedule is unchanged -- one that
hides the exchange less well computes the same values -- so the CPU stand-in logs the calls (tests/cpu_abi/oracle_abi.c:
abi_jacobi_log) and every case is compared with tests/golden/slab_jacobi_traces.json, rank by rank.

The fixture records the host solver as it was BEFORE the schedule moved into csrc/host/slab_jacobi_plan.hpp (this file, run as
`python tests/test_slab_jacobi_trace_cpu.py --record` in a checkout of that commit with this file, the stand-in's log and the
worker's two flags added).  It is a record of that commit: a change of the schedule on purpose edits it by hand, with the reason.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_slab_multirank import ROOT, launch

GOLDEN = os.path.join(ROOT, "tests", "golden", "slab_jacobi_traces.json")

# 24 x 20 rows; 36 iterations = 35 sweeps = 8 + 8 + 8 + 8 + 3
EDGE = ("--dims", 24, 20, 48, "--ghost", 8, "--iters", 36)          # 24 owned planes = 2 G + 8: ends-first interiors of 2 and 8 planes
CASES = {
    "edge_g8_triples_ends_first": (2, EDGE),
    "g8_owned23_triples_plain": (2, ("--dims", 24, 20, 46, "--ghost", 8, "--iters", 36)),
    "edge_g8_pairs_ends_first": (2, EDGE + ("--triples", 0)),
    "edge_g8_triples_no_ends_first": (2, EDGE + ("--ends-first", 0)),
    "edge_g8_no_overlap": (2, EDGE + ("--overlap", 0)),
    "g6_owned20_pairs_ends_first": (2, ("--dims", 24, 20, 40, "--ghost", 6, "--iters", 20)),
    "g6_three_ranks_plain_pairs": (3, ("--dims", 24, 20, 36, "--ghost", 6, "--iters", 16)),
    "g5_two_pairs_and_a_tail": (2, ("--dims", 24, 20, 32, "--ghost", 5, "--iters", 12)),
    "edge_g8_first_pair_refused": (2, EDGE + ("--jacobi-fuse", 0)),
    "edge_g8_first_triple_refused": (2, EDGE + ("--jacobi-fuse", 4)),
    "edge_g8_one_sweep": (2, ("--dims", 24, 20, 48, "--ghost", 8, "--iters", 2)),
    "edge_g8_no_sweep": (2, ("--dims", 24, 20, 48, "--ghost", 8, "--iters", 1)),
}


def run_case(name, tmp):
    """the case's log, one list of lines per rank; the run itself must agree with the oracle on every rank"""
    nranks, args = CASES[name]
    log = os.path.join(str(tmp), name + ".{rank}.log")
    rc, out = launch(nranks, "--backend", "cpu", "--steps", 2, "--dt-cells", 1.0, *args, "--jacobi-log", log)
    assert rc == 0, out
    assert out.count("mismatches=0") == nranks, out
    return [open(log.format(rank=r)).read().splitlines() for r in range(nranks)]


@pytest.fixture(scope="module", autouse=True)
def built_cpu_host():
    from build_cpu_host import build
    build()
    import oracle_lib
    oracle_lib.build()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", sorted(CASES))
def test_slab_projection_issues_the_recorded_calls(name, golden, tmp_path):
    got = run_case(name, tmp_path)
    want = golden[name]
    assert len(got) == len(want)
    for rank, (g, w) in enumerate(zip(got, want)):
        assert w and w[0] == "projection", (name, rank)
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        assert g == w, f"{name}, rank {rank}: call {first} is {g[first:first + 1]}, recorded {w[first:first + 1]}"


def test_the_recorded_cases_show_what_they_are_named_for(golden):
    """the fixture itself: every case reaches the path it stands for (a case that silently ran another schedule would pin nothing)"""
    def lines(name): return golden[name][0]
    def ends_first(ls, what): return any(l.startswith(what) and l.split()[4:6] != ["0", "0"] and "exchange" in ls[i + 2]
                                         for i, l in enumerate(ls[:-2]))
    assert ends_first(lines("edge_g8_triples_ends_first"), "triple")
    assert not any(l.split()[4:6] != ["0", "0"] for l in lines("g8_owned23_triples_plain") if l.startswith("triple"))
    assert any(l.startswith("triple") for l in lines("g8_owned23_triples_plain"))
    assert ends_first(lines("edge_g8_pairs_ends_first"), "pair") and not any(l.startswith("triple") for l in lines("edge_g8_pairs_ends_first"))
    assert any(l.startswith("triple") for l in lines("edge_g8_triples_no_ends_first")) and not ends_first(lines("edge_g8_triples_no_ends_first"), "triple")
    # (BQ_OPT_OVERLAP_EXCHANGES = 0 takes the ends-first order away; a chunk's first pass still runs while its exchange travels)
    assert lines("edge_g8_no_overlap") == lines("edge_g8_triples_no_ends_first")
    assert ends_first(lines("g6_owned20_pairs_ends_first"), "pair")
    assert not ends_first(lines("g6_three_ranks_plain_pairs"), "pair") and any(l.startswith("pair") for l in lines("g6_three_ranks_plain_pairs"))
    assert any(l.startswith("sweeps") and l.endswith(" 1") for l in lines("g5_two_pairs_and_a_tail"))
    refused = lines("edge_g8_first_pair_refused")
    assert sum(l.startswith("pair") for l in refused) == 2 and all(l.endswith("= 0") for l in refused if l.startswith("pair"))   # once per projection
    assert any(l.startswith("range") for l in refused) and any(l.startswith("sweeps") and l.endswith(" 6") for l in refused)
    refused = lines("edge_g8_first_triple_refused")
    assert sum(l.startswith("triple") for l in refused) == 2 and ends_first(refused, "pair")
    assert sum(l.startswith("sweeps") for l in lines("edge_g8_one_sweep")) == 2
    assert lines("edge_g8_no_sweep") == ["projection", "projection"]


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:] == ["--record"], "usage: --record (in a checkout of the commit whose schedule is to be recorded)"
    from build_cpu_host import build
    import oracle_lib
    build(); oracle_lib.build()
    with tempfile.TemporaryDirectory() as tmp:
        rec = {name: run_case(name, tmp) for name in sorted(CASES)}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print({name: [len(r) for r in ranks] for name, ranks in rec.items()})
