// bq_mgcg_slab_plan.h -- the decomposition of the slab-shared multigrid-CG projection (bq_mgcg_slab.hip.inc), stated once: which
// geometries it takes, how deep the pyramid is shared, which planes of every level a rank owns and stores, and every plane
// count and offset the cycle derives from those.  Pure integer arithmetic on (ni, nj, nkg, ghost, rank, nranks): no HIP, no
// allocation, no runtime state, so that tests/test_mgcg_slab_plan_cpu.py can compile it with a plain C++ compiler and sweep it
// without a GPU.  slab_mg_setup, slab_v_cycle, slab_exchange, slab_dot, slab_gather_planes and the entry point read the plan;
// the host solver reads the predicate (BimocqGPUSolver::projectionMgcgShared through gpu_mgcg_slab_supported).
//
// The host chooses between two COLLECTIVES by `supported` -- the shared solve or the replicated one -- so everything that
// decides it depends on (ni, nj, nkg, ghost, nranks) alone: the per-rank quantities that enter (fewest owned planes of a
// level, the nesting of the stored ranges) are evaluated for every rank, on every rank.
//
//   level l, global planes [0, nk_l):  rank r owns [own0, own1), stores [lo, hi) = own +- G_l clipped to the grid, lo even.
//   pyramid n -> (n - 1) / 2; coarse plane K belongs to the owner of fine plane 2 K + 1.
//   Levels [0, LS) are shared (LS <= 3, never the coarsest), level LS is the first replicated one: a rank's planes of it are
//   what it contributes to the gather.
#pragma once
#include <algorithm>

namespace bq {
namespace mgslab {

constexpr int kLevels = 6;              // LEVEL_COUNT (include/bimocq_gpu.h)
constexpr int kMaxShared = 3;           // at most this many levels are shared
constexpr int kDotBlock = 256;          // cells per block of the float-narrowed dot products
constexpr int kDepth = 8;               // ghost depth of level 0; deeper levels take what their thinnest rank allows, down to 4
constexpr int kMinOwned = 17;           // owned planes of level 0 per rank

struct Range { int a, b; };

// planes of level l + 1 owned by the owner of the fine planes [a, b): K with 2 K + 1 in [a, b), inside [0, nkc)
inline Range coarse_own(Range f, int nkc)
{
    // 2 K + 1 >= a  <=>  K >= (a - 1) / 2, rounded up: a / 2 for either parity; 2 K + 1 < b  <=>  K < (b - 1) / 2 rounded up = b / 2
    return Range{ std::min(nkc, std::max(0, f.a / 2)), std::min(nkc, std::max(0, f.b / 2)) };
}

// level 0: equal slabs in rank order
inline Range fine_own(int nkg, int r, int nranks)
{
    return Range{ (int)((long long)r * nkg / nranks), (int)((long long)(r + 1) * nkg / nranks) };
}

// What the size of the grid and of the communicator admit -- the same answer on every rank.  Planes of a multiple of 256 cells
// (slab boundaries are dot-block boundaries), equal slabs of a multiple of 8 planes (even ranges on three levels) and at least
// 17 of them, G = 8 on level 0 inside the velocity's ghost planes, slab arrays below 2^31 bytes.
inline bool geometry_supported(int ni, int nj, int nkg, int ghost, int nranks)
{
    if (nranks < 2 || ni < 8 || nj < 8 || nkg < 8) return false;
    if (((long long)ni * nj) % kDotBlock != 0) return false;
    if (nkg % nranks != 0) return false;
    const int per = nkg / nranks;
    if (per % 8 != 0 || per < kMinOwned || ghost < kDepth) return false;
    if ((double)ni * nj * (per + 2 * kDepth) * 8.0 >= 2147483648.0) return false;
    return true;
}

struct Level {
    int ni = 0, nj = 0, nk = 0;         // global dims of the level
    int own0 = 0, own1 = 0;             // planes this rank owns          (levels [0, LS])
    int lo = 0, hi = 0;                 // planes it stores               (level LS: the whole level)
    int G = 0;                          // ghost depth both neighbours exchange at (0: not shared)
    // ---- levels [0, LS) only
    // restriction onto this rank's planes [rest_c0, rest_c0 + rest_ck) of level l + 1: the fine range handed to the kernel starts
    // at plane rest_fine0 = 2 rest_c0 and has rest_fine_planes planes (up to hi)
    int rest_c0 = 0, rest_ck = 0, rest_fine0 = 0, rest_fine_planes = 0;
    // prolongation onto [lo, hi): the coarse range handed to the kernel starts at plane prol_c0 = lo / 2 and has prol_ck planes
    int prol_c0 = 0, prol_ck = 0;
    // fl_halo_exchange addresses a buffer of own + 2 G planes that starts G planes below the first owned one: the array's base
    // is moved back by xch_shift planes (negative: forward) and the exchange is told xch_nk_local planes
    int xch_shift = 0, xch_nk_local = 0;
};

struct Plan {
    bool supported = false;             // identical on every rank
    int ni = 0, nj = 0, nkg = 0, ghost = 0, rank = 0, nranks = 1;
    int nlevels = 0;                    // levels of the pyramid with at least one cell
    int LS = 0;                         // levels [0, LS) are shared, [LS, nlevels) replicated
    Level lv[kLevels];
    // this rank's blocks of the dot products' partial array (one per 256 cells of the GLOBAL level 0): [dot_first, + dot_nb_own) of dot_nb
    long long dot_first = 0, dot_nb_own = 0, dot_nb = 0;
    // the gradient writes the global planes [k_first, k_end) (it reads p one plane below)
    int k_first = 0, k_end = 0;

    // planes rank r owns of level l (l <= LS)
    Range own(int r, int l) const
    {
        Range o = fine_own(nkg, r, nranks);
        for (int q = 0; q < l; q++) o = coarse_own(o, lv[q + 1].nk);
        return o;
    }
    long long dot_first_of(int r) const { return (long long)lv[0].ni * lv[0].nj * own(r, 0).a / kDotBlock; }
    long long dot_nb_of(int r) const { const Range o = own(r, 0); return (long long)lv[0].ni * lv[0].nj * (o.b - o.a) / kDotBlock; }
};

// the range rank r stores of a shared level with ghost depth G
inline Range stored(Range own, int G, int nk)
{
    Range s{ std::max(0, own.a - G), std::min(nk, own.b + G) };
    if (s.a % 2) s.a -= 1;              // transfer operators pair a fine range that starts at an even plane with the coarse range at half of it
    return s;
}

inline Plan make_plan(int ni, int nj, int nkg, int ghost, int rank, int nranks)
{
    Plan p;
    p.ni = ni; p.nj = nj; p.nkg = nkg; p.ghost = ghost; p.rank = rank; p.nranks = nranks;
    if (rank < 0 || rank >= nranks || !geometry_supported(ni, nj, nkg, ghost, nranks)) return p;
    int di = ni, dj = nj, dk = nkg;
    for (int l = 0; l < kLevels; l++) {
        if (l) { di = (di - 1) / 2; dj = (dj - 1) / 2; dk = (dk - 1) / 2; }
        if (di < 1 || dj < 1 || dk < 1) break;
        p.lv[l].ni = di; p.lv[l].nj = dj; p.lv[l].nk = dk;
        p.nlevels++;
    }
    // how deep the pyramid can be shared: every rank needs G_l + 1 owned planes on a shared level (fl_halo_exchange), G_l even
    // and at least 4; the coarsest level is never shared
    for (int l = 0; l < p.nlevels && l < kMaxShared; l++) {
        int fewest = 1 << 30;
        for (int r = 0; r < nranks; r++) { const Range o = p.own(r, l); fewest = std::min(fewest, o.b - o.a); }
        int G = std::min(kDepth, fewest - 1);
        G -= G % 2;
        if (G < 4 || l + 1 >= p.nlevels) break;
        p.lv[l].G = G;
        p.LS = l + 1;
    }
    if (p.LS < 1 || p.lv[0].G > ghost) return p;
    // a fine range [lo, hi) samples the coarse range that starts at lo / 2: it must be stored, on every rank (follows from
    // G_{l+1} >= 4 >= G_l / 2; tests/test_mgcg_slab_plan_cpu.py sweeps it)
    for (int r = 0; r < nranks; r++)
        for (int l = 0; l + 1 < p.LS; l++)
            if (stored(p.own(r, l + 1), p.lv[l + 1].G, p.lv[l + 1].nk).a > stored(p.own(r, l), p.lv[l].G, p.lv[l].nk).a / 2) return p;
    p.supported = true;

    for (int l = 0; l <= p.LS; l++) {
        Level &L = p.lv[l];
        const Range o = p.own(rank, l);
        L.own0 = o.a; L.own1 = o.b;
        if (l == p.LS) { L.lo = 0; L.hi = L.nk; break; }       // the first replicated level as the gather sees it
        const Range s = stored(o, L.G, L.nk);
        L.lo = s.a; L.hi = s.b;
        L.xch_shift = L.G - (L.own0 - L.lo);
        L.xch_nk_local = (L.own1 - L.own0) + 2 * L.G;
    }
    for (int l = 0; l < p.LS; l++) {
        Level &L = p.lv[l];
        const Level &C = p.lv[l + 1];
        L.rest_c0 = C.own0; L.rest_ck = C.own1 - C.own0;
        L.rest_fine0 = 2 * C.own0; L.rest_fine_planes = L.hi - 2 * C.own0;
        L.prol_c0 = L.lo / 2; L.prol_ck = C.hi - L.lo / 2;
    }
    const Level &L0 = p.lv[0];
    const long long pd = (long long)L0.ni * L0.nj;
    p.dot_first = pd * L0.own0 / kDotBlock;
    p.dot_nb_own = (pd * (L0.own1 - L0.own0) + kDotBlock - 1) / kDotBlock;
    p.dot_nb = (pd * L0.nk + kDotBlock - 1) / kDotBlock;
    p.k_first = std::max(L0.lo + 1, 2);
    p.k_end = std::min(L0.hi, nkg);
    return p;
}

// the arguments a rank passes describe the decomposition the plan assumes: equal slabs in rank order
inline bool rank_args_match(int nkg, int own0, int own1, int rank, int nranks)
{
    if (nranks < 1 || rank < 0 || rank >= nranks) return false;
    const Range o = fine_own(nkg, rank, nranks);
    return own0 == o.a && own1 == o.b;
}

// gpu_mgcg_slab_supported: the plan's answer for a rank whose arguments describe the plan's slabs
inline bool supported(int ni, int nj, int nkg, int own0, int own1, int ghost, int rank, int nranks)
{
    return rank_args_match(nkg, own0, own1, rank, nranks) && make_plan(ni, nj, nkg, ghost, rank, nranks).supported;
}

} // namespace mgslab
} // namespace bq
