"""CPU tests of csrc/bq_mgcg_slab_plan.h: the decomposition of the slab-shared fp64 multigrid-CG projection
(gpu_multi_grid_conjugate_gradient_slab) -- which geometries it takes, how deep the pyramid is shared, the planes a rank owns and
stores of every level and every count and offset the cycle derives from them.  The header is compiled with g++ behind
tests/cpu_abi/mgcg_slab_plan_shim.cpp and called through ctypes, one call per sweep.

The reference is REF below: a restatement written from the comment block at the head of csrc/bq_mgcg_slab.hip.inc and the
reference's pyramid n -> (n - 1) / 2, with ownership as explicit per-plane owner lists (a coarse plane K takes the owner of fine
plane 2 K + 1) instead of the header's closed-form ranges.  Its predicate knows the geometry conditions only: that the plan's
`supported` equals it on the whole domain is the proof that neither "levels too thin to share" nor "coarse ghost range too shallow"
can refuse a geometry the predicate admits -- on one rank or on all.

Domain: seven plane shapes, 16 .. 200 global planes, 2 .. 8 ranks, every rank, ghost depths 6 / 8 / 12."""
import ctypes as C

import numpy as np
import pytest

from build_cpu_host import build_mgcg_slab_plan

I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
# 64 x 20: a plane of five dot blocks (1280 cells); 24 x 20: a plane of no multiple of 256 cells (480), refused throughout
SHAPES = [(16, 16), (32, 8), (8, 32), (48, 16), (32, 32), (64, 20), (24, 20)]
NKG = range(16, 201)
RANKS = range(2, 9)
GHOSTS = (6, 8, 12)
HEAD = ["supported", "nlevels", "LS", "dot_first", "dot_nb_own", "dot_nb", "k_first", "k_end"]
LEVEL = ["ni", "nj", "nk", "own0", "own1", "lo", "hi", "G", "rest_c0", "rest_ck", "rest_fine0", "rest_fine_planes", "prol_c0", "prol_ck",
         "xch_shift", "xch_nk_local"]
NLEV, MAXSHARED = 6, 3


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(build_mgcg_slab_plan(), mode=C.RTLD_LOCAL)
    assert so.mgcg_slab_plan_levels() == NLEV and so.mgcg_slab_plan_row_ints() == len(HEAD) + NLEV * len(LEVEL)

    def call(name, rows, width):
        fn = getattr(so, name)
        fn.restype, fn.argtypes = None, [C.c_int, I32P, I32P]
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.zeros((rows.shape[0], width), dtype=np.int32)
        fn(rows.shape[0], rows, out)
        return out
    call.table_width = so.mgcg_slab_table_row_ints()
    return call


class Plan:
    """one row of mgcg_slab_plan_rows"""
    def __init__(self, row):
        for i, n in enumerate(HEAD):
            setattr(self, n, int(row[i]))
        self.lv = [dict(zip(LEVEL, map(int, row[len(HEAD) + l * len(LEVEL): len(HEAD) + (l + 1) * len(LEVEL)]))) for l in range(NLEV)]

    @property
    def G(self):
        return tuple(self.lv[l]["G"] for l in range(self.LS))


def plans(lib, ni, nj, nkg, ghost, nranks):
    rows = [(ni, nj, nkg, ghost, r, nranks) for r in range(nranks)]
    return [Plan(row) for row in lib("mgcg_slab_plan_rows", rows, len(HEAD) + NLEV * len(LEVEL))]


@pytest.fixture(scope="module")
def sweep(lib):
    """every (shape, nkg, ghost, nranks, rank) of the domain: the input rows and the plans, as arrays"""
    rows = np.array([(ni, nj, nkg, ghost, r, n) for ni, nj in SHAPES for nkg in NKG for ghost in GHOSTS for n in RANKS for r in range(n)],
                    dtype=np.int32)
    return rows, lib("mgcg_slab_plan_rows", rows, len(HEAD) + NLEV * len(LEVEL))


# ---- the independent restatement -------------------------------------------------------------------------------------------------
def ref_supported(ni, nj, nkg, ghost, nranks):
    """the requirements of the header comment: planes of whole 256-cell dot blocks, equal slabs of a multiple of 8 planes and at
    least 17 of them, 8 ghost planes on level 0 inside the velocity's, slab arrays (own + 16 planes of doubles) below 2 GiB"""
    if nranks < 2 or min(ni, nj, nkg) < 8 or (ni * nj) % 256 or nkg % nranks:
        return False
    per = nkg // nranks
    return per % 8 == 0 and per >= 17 and ghost >= 8 and ni * nj * (per + 16) * 8 < 2 ** 31


class Ref:
    def __init__(self, ni, nj, nkg, ghost, nranks):
        self.supported = ref_supported(ni, nj, nkg, ghost, nranks)
        if not self.supported:
            return
        # the reference's pyramid: at most six levels, a level exists while every dimension has a cell
        self.dims = [(ni, nj, nkg)]
        while len(self.dims) < NLEV and min((d - 1) // 2 for d in self.dims[-1]) >= 1:
            self.dims.append(tuple((d - 1) // 2 for d in self.dims[-1]))
        self.nlevels = len(self.dims)
        # who owns which plane: level 0 in equal slabs, coarse plane K with the owner of fine plane 2 K + 1
        per = nkg // nranks
        self.owner = [[k // per for k in range(nkg)]]
        for l in range(1, self.nlevels):
            self.owner.append([self.owner[l - 1][2 * K + 1] for K in range(self.dims[l][2])])
        # shared while the thinnest rank has G + 1 planes for an even G of 4 .. 8; at most three levels, never the coarsest
        self.G = []
        for l in range(min(MAXSHARED, self.nlevels - 1)):
            fewest = min(self.owner[l].count(r) for r in range(nranks))
            G = min(8, fewest - 1) // 2 * 2
            if G < 4:
                break
            self.G.append(G)
        self.LS = len(self.G)

    def own(self, r, l):
        ks = [k for k, o in enumerate(self.owner[l]) if o == r]
        assert ks == list(range(ks[0], ks[-1] + 1))
        return ks[0], ks[-1] + 1


def supported_geometries():
    return [(ni, nj, nkg, ghost, n) for ni, nj in SHAPES for nkg in NKG for ghost in GHOSTS for n in RANKS if ref_supported(ni, nj, nkg, ghost, n)]


# ---- agreement ------------------------------------------------------------------------------------------------------------------
def test_every_rank_gets_the_same_answer_and_the_same_pyramid(sweep):
    """supported, nlevels, LS and every G_l over the WHOLE domain, refused geometries included: equal to rank 0's row"""
    rows, out = sweep
    first = np.arange(len(rows)) - rows[:, 4]                  # the row of rank 0 of the same geometry
    assert np.all(rows[first, 4] == 0) and np.all(rows[first, :4] == rows[:, :4]) and np.all(rows[first, 5] == rows[:, 5])
    same = ["supported", "nlevels", "LS"]
    for n in same:
        assert np.array_equal(out[:, HEAD.index(n)], out[first, HEAD.index(n)]), n
    for l in range(NLEV):
        for n in ("ni", "nj", "nk", "G"):
            col = len(HEAD) + l * len(LEVEL) + LEVEL.index(n)
            assert np.array_equal(out[:, col], out[first, col]), (l, n)
    assert 0 < out[:, 0].sum() < len(out)


def test_supported_is_the_geometry_predicate_and_nothing_else(sweep):
    """the plan refuses exactly what the restated predicate refuses: no geometry it admits is "too thin to share" or has a "coarse
    ghost range too shallow", on any rank; 24 x 20 planes and 6 ghost planes are refused throughout"""
    rows, out = sweep
    want = np.array([ref_supported(ni, nj, nkg, ghost, n) for ni, nj, nkg, ghost, r, n in rows.tolist()])
    assert np.array_equal(out[:, 0] != 0, want)
    assert not out[(rows[:, 0] == 24) | (rows[:, 3] == 6), 0].any()
    assert len(supported_geometries()) > 150


def test_the_entry_point_predicate_is_rank_independent(lib):
    """gpu_mgcg_slab_supported's own arguments (own0, own1, rank) over the domain at ghost 8: one answer per geometry, the
    restated predicate's; slabs that are not the plan's equal ones are refused"""
    geos = [(ni, nj, nkg, n) for ni, nj in SHAPES for nkg in NKG for n in RANKS]
    rows = [(ni, nj, nkg, r * nkg // n, (r + 1) * nkg // n, 8, r, n) for ni, nj, nkg, n in geos for r in range(n)]
    got = lib("mgcg_slab_supported_rows", rows, 1)[:, 0]
    want = [int(ref_supported(ni, nj, nkg, 8, n)) for ni, nj, nkg, n in geos for r in range(n)]
    assert got.tolist() == want
    wrong = [(32, 32, 96, 40, 88, 8, 1, 2), (32, 32, 96, 48, 96, 8, 0, 2), (32, 32, 96, 48, 96, 8, 2, 2), (32, 32, 96, 48, 96, 8, -1, 2)]
    assert lib("mgcg_slab_supported_rows", wrong, 1)[:, 0].tolist() == [0, 0, 0, 0]
    assert lib("mgcg_slab_supported_rows", [(32, 32, 96, 48, 96, 8, 1, 2)], 1)[0, 0] == 1


@pytest.mark.parametrize("ni,nj,nkg,nranks", [(32, 32, 80, 4), (16, 16, 40, 2), (16, 16, 100, 4)])
def test_planes_per_rank_of_no_multiple_of_8_take_the_replicated_solve_on_every_rank(lib, ni, nj, nkg, nranks):
    """the geometries on which `own0 % 8` split the ranks between the two collectives ([1, 0, 1, 0], [1, 0], [1, 0, 0, 0]): 20 and
    25 planes per rank answer 0 everywhere"""
    per = nkg // nranks
    rows = [(ni, nj, nkg, r * per, (r + 1) * per, 8, r, nranks) for r in range(nranks)]
    assert lib("mgcg_slab_supported_rows", rows, 1)[:, 0].tolist() == [0] * nranks
    assert [p.supported for p in plans(lib, ni, nj, nkg, 8, nranks)] == [0] * nranks


# ---- the plan against the restatement, and the invariants of the cycle ------------------------------------------------------------
def test_plan_matches_the_restatement_and_keeps_every_invariant(lib):
    checked = 0
    for ni, nj, nkg, ghost, nranks in supported_geometries():
        ref = Ref(ni, nj, nkg, ghost, nranks)
        ps = plans(lib, ni, nj, nkg, ghost, nranks)
        tables = lib("mgcg_slab_plan_tables", [(ni, nj, nkg, ghost, r, nranks) for r in range(nranks)], lib.table_width)
        where = (ni, nj, nkg, ghost, nranks)
        LS = ref.LS
        assert LS >= 1, where
        for r, p in enumerate(ps):
            assert p.supported == 1 and p.nlevels == ref.nlevels and p.LS == LS and p.G == tuple(ref.G), (where, r)
            assert [(L["ni"], L["nj"], L["nk"]) for L in p.lv[:p.nlevels]] == ref.dims, (where, r)
            # ---- partition: the plan's ranges are the owner lists' (disjoint, in rank order, covering, nested by 2 K + 1)
            for l in range(LS + 1):
                assert (p.lv[l]["own0"], p.lv[l]["own1"]) == ref.own(r, l), (where, r, l)
            # the tables of all ranks, as this rank holds them
            t = tables[r].reshape(8, 2 * (MAXSHARED + 1) + 2)
            for q in range(nranks):
                for l in range(LS + 1):
                    assert (int(t[q, 2 * l]), int(t[q, 2 * l + 1])) == ref.own(q, l), (where, r, q, l)
        for l in range(LS + 1):
            edges = [ref.own(r, l) for r in range(nranks)]
            assert edges[0][0] == 0 and edges[-1][1] == ref.dims[l][2], (where, l)
            assert all(edges[r][1] == edges[r + 1][0] and edges[r][0] < edges[r][1] for r in range(nranks - 1)), (where, l)
        # ---- depths
        assert ref.G[0] == 8 and ref.G[0] <= ghost, where
        for l in range(LS):
            G = ref.G[l]
            assert G % 2 == 0 and 4 <= G <= 8, (where, l)
            assert all(G + 1 <= ref.own(r, l)[1] - ref.own(r, l)[0] for r in range(nranks)), (where, l)
        for r, p in enumerate(ps):
            for l in range(LS):
                L, nk, G = p.lv[l], p.lv[l]["nk"], p.lv[l]["G"]
                own0, own1, lo, hi = L["own0"], L["own1"], L["lo"], L["hi"]
                at = (where, r, l)
                # ---- ranges
                assert (lo, hi) == (max(0, own0 - G) // 2 * 2, min(nk, own1 + G)), at
                assert lo % 2 == 0, at                          # (the header keeps lo even on the last shared level too)
                assert lo <= own0 - G or lo == 0, at
                assert 0 <= lo and hi >= min(nk, own1 + G) and hi <= nk, at
                C = p.lv[l + 1]
                if l + 1 < LS:
                    assert C["lo"] <= lo // 2, at
                else:
                    assert (C["lo"], C["hi"], C["G"]) == (0, C["nk"], 0), at       # the first replicated level: stored in full
                # ---- restriction: coarse planes K of this rank read the fine planes 2 K .. 2 K + 2 of the range it is handed
                assert (L["rest_c0"], L["rest_c0"] + L["rest_ck"]) == (C["own0"], C["own1"]), at
                assert L["rest_fine0"] == 2 * L["rest_c0"] and lo <= L["rest_fine0"], at
                assert L["rest_fine0"] + L["rest_fine_planes"] == hi, at
                for K in range(C["own0"], C["own1"]):
                    assert lo <= 2 * K and 2 * K + 2 < hi, (at, K)
                # ---- prolongation: the fine range [lo, hi) reads the coarse planes from lo / 2 on, all stored
                assert L["prol_c0"] == lo // 2 and L["prol_ck"] >= 1, at
                assert C["lo"] <= L["prol_c0"] and L["prol_c0"] + L["prol_ck"] <= C["hi"], at
                # (what an OWNED fine plane samples -- the ghost planes are exchanged right after: interior plane k reads the coarse
                # planes floor(k / 2 - 1 / 2) and the next one; both are in the range handed over, or beyond the level's last plane,
                # where the range ends with the level and the kernel clips as it does on one GPU)
                end = L["prol_c0"] + L["prol_ck"]
                for k in range(max(own0, 1), min(own1, nk - 1)):
                    c = (k - 1) // 2
                    assert L["prol_c0"] <= c and (c + 1 < end or end == C["nk"]), (at, k)
                # ---- exchange: fl_halo_exchange sees a buffer of own + 2 G planes whose plane q is the global plane own0 - G + q; the
                # array's plane 0 is the global plane lo, and the base handed over lies xch_shift planes below it
                assert L["xch_nk_local"] == own1 - own0 + 2 * G, at
                first_plane = lo - L["xch_shift"]               # the global plane of the buffer's plane 0
                assert first_plane == own0 - G, at
                touched = []
                if r > 0:
                    touched += [first_plane + G, first_plane + 2 * G - 1, first_plane, first_plane + G - 1]            # send, receive
                if r + 1 < nranks:
                    own = own1 - own0
                    touched += [first_plane + own, first_plane + G + own - 1, first_plane + G + own, first_plane + 2 * G + own - 1]
                assert all(lo <= k < hi for k in touched), (at, touched)
            # ---- the gradient writes [k_first, k_end) and reads one plane below
            L0 = p.lv[0]
            assert p.k_first == max(L0["lo"] + 1, 2) and p.k_end == min(L0["hi"], nkg), (where, r)
            assert all(k - 1 >= L0["lo"] and k < L0["hi"] for k in range(p.k_first, p.k_end)), (where, r)
            assert p.k_first <= max(L0["own0"], 2) and p.k_end >= L0["own1"], (where, r)     # the owned planes are projected
            # level 0 inside the velocity's buffers, planes [own0 - ghost, own1 + ghost)
            assert L0["own0"] - ghost <= L0["lo"] or L0["lo"] == 0, (where, r)
        # ---- dot blocks: the ranks' [first, first + nb_own) tile the blocks of the global array, in rank order
        blocks = ni * nj * nkg // 256
        at = 0
        for r, p in enumerate(ps):
            assert p.dot_nb == blocks and p.dot_first == at and p.dot_nb_own == ni * nj * (nkg // nranks) // 256, (where, r)
            for q in range(nranks):
                t = tables[q].reshape(8, 2 * (MAXSHARED + 1) + 2)
                assert (int(t[r, -2]), int(t[r, -1])) == (p.dot_first, p.dot_nb_own), (where, r, q)
            at += p.dot_nb_own
        assert at == blocks, where
        checked += 1
    assert checked == len(supported_geometries())


@pytest.mark.parametrize("ni,nj,nkg,nranks,G,nlevels,blocks_per_plane", [
    (16, 16, 48, 2, (8, 8, 4), 4, 1),           # a ghost depth of 4 on a shared level, one dot block per plane
    (16, 16, 72, 3, (8, 8, 4), 4, 1),           # ... with a middle rank
    (32, 8, 48, 2, (8, 8), 3, 1),               # a three-level pyramid: two shared levels
    (48, 16, 48, 2, (8, 8, 4), 4, 3),           # a plane of three dot blocks
])
def test_the_gpu_cases_reach_the_classes_they_are_there_for(lib, ni, nj, nkg, nranks, G, nlevels, blocks_per_plane):
    """tests/test_gpu_rccl_path.py::test_multigrid_shared_levels_at_the_small_geometries runs these grids; here: what the plan makes
    of them.  (The older cases: 32 x 32 x 96 on 2 ranks gives (8, 8, 8), on 3 ranks (8, 8, 6), 32 x 16 x 128 on 4 ranks (8, 8, 6).)"""
    for p in plans(lib, ni, nj, nkg, 8, nranks):
        assert p.supported == 1 and p.G == G and p.LS == len(G) and p.nlevels == nlevels
        assert ni * nj // 256 == blocks_per_plane and ni * nj % 256 == 0
        assert p.lv[0]["own1"] - p.lv[0]["own0"] == 24
    if (ni, nj, nkg) == (16, 16, 48):
        # one replicated level only: the fused bottom launch of the two coarsest levels has nothing to run on
        assert nlevels - len(G) == 1
    assert [p.G for p in plans(lib, 32, 32, 96, 8, 2)] == [(8, 8, 8)] * 2 and [p.G for p in plans(lib, 32, 32, 96, 8, 3)] == [(8, 8, 6)] * 3
    assert [p.G for p in plans(lib, 32, 16, 128, 8, 4)] == [(8, 8, 6)] * 4
