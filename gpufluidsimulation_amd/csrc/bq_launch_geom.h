// bq_launch_geom.h -- launch geometry shared by the marching stencil kernels: the fp32 Jacobi sweeps (bq_project.hip) and the
// fp64 multigrid smoothers (bq_mgcg.hip, bq_mgcg_fused.hip.inc).  Pure integer arithmetic on the host: no HIP, no runtime
// state, so that tests/test_launch_geom_cpu.py can compile it with a plain C++ compiler and check every rule without a GPU.
// The clamps, overrides and refusals that differ between the launchers: bq_jacobi_plan.h for the fp32 sweeps, the launchers for fp64.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace bq {
namespace geom {

// Lanes per row of a kernel whose lanes hold `per_lane` cells each (float4: 4, double2: 2): the power of two >= 16 that
// covers ni cells, at most `cap`.
inline int pow2_lanes(int ni, int per_lane, int cap = 1 << 30)
{
    int cw = 16;
    while (cw * per_lane < ni && cw < cap) cw *= 2;
    return cw;
}

// How many k-chunks cut `planes` planes so that row_blocks x chunks blocks fill the chip in whole rounds.  A marching
// kernel only pays when no CU waits for a partly filled last round (256^3, two blocks per CU: 512 blocks run 19.1 us per
// sweep, 576 or 448 blocks 22.7), so the chunk count is the multiple of round / gcd(row_blocks, round) -- the counts that
// make row_blocks x chunks a multiple of `round` -- nearest to planes / target, and at least one such multiple.
// round: blocks per round on 256 CUs, 256 for the kernels that run one block per CU, 512 for two.  The caller derives the
// chunk length ceil(planes / chunks) and applies its own limits.
inline int whole_round_chunks(int row_blocks, int planes, int target, int round)
{
    int gcd = row_blocks, rem = round;
    while (rem) { const int t = gcd % rem; gcd = rem; rem = t; }
    const int quantum = round / gcd;
    const int nchunks = ((2 * planes + target) / (2 * target) + quantum / 2) / quantum * quantum;
    return std::max(nchunks, quantum);
}

// How many k-chunks a fused launch cuts `nkr` planes into when the compute stream does not own the whole chip
// (FL_OPT_RESERVE_CUS): the rule above fills 256 CUs in whole rounds; with another CU count no chunk count divides evenly, so
// take the one that minimises rounds x planes marched per block (chunk + `warm` warm-up planes), nearest to the target
// chunk length among near-equal candidates.  per_cu: resident blocks per CU.
inline int chunks_for_cus(int nkr, int nrow, int target, int warm, int ncus, int per_cu)
{
    double best = 1e30; int best_n = 1, best_gap = 1 << 30;
    for (int n = 1; n <= std::max(1, nkr / 4); n++) {
        const int kc = (nkr + n - 1) / n;
        const long blocks = (long)nrow * ((nkr + kc - 1) / kc);
        const long rounds = (blocks + (long)ncus * per_cu - 1) / ((long)ncus * per_cu);
        const double cost = (double)rounds * (kc + warm);
        const int gap = std::abs(kc - target);
        if (cost < best * 0.97 || (cost <= best * 1.03 && gap < best_gap)) { best = std::min(best, cost); best_n = n; best_gap = gap; }
    }
    return best_n;
}

// Chunk length that gives every CU one block: `nranges` plane ranges, the longest of `longest` planes, each cut into
// ncus / (row_blocks x nranges) chunks.
inline int once_per_cu_len(int longest, int row_blocks, int nranges, int ncus)
{
    const int per_range = std::max(1, ncus / std::max(1, row_blocks * nranges));
    return (longest + per_range - 1) / per_range;
}

// The output planes of a fused launch: up to two ranges [k0a, k1a) and [k0b, k1b), clipped to the nk planes of the array
// (the pieces of a z-slab chunk; either may be empty).  whole: one range that covers the array.
struct PlaneRanges {
    int k0a, k1a, k0b, k1b;
    int lenA, lenB, planes, nranges, longest;
    bool whole;
    PlaneRanges(int k0a_, int k1a_, int k0b_, int k1b_, int nk)
        : k0a(std::max(k0a_, 0)), k1a(std::min(k1a_, nk)), k0b(std::max(k0b_, 0)), k1b(std::min(k1b_, nk)),
          lenA(std::max(k1a - k0a, 0)), lenB(std::max(k1b - k0b, 0)), planes(lenA + lenB), nranges((lenA > 0) + (lenB > 0)),
          longest(std::max(lenA, lenB)), whole(lenB == 0 && lenA == nk) {}
    // the ranges in chunks of kc planes: chunks bz < nchA march the first range, the other nbz - nchA the second
    struct Chunks { int k0a, k1a, k0b, k1b, nchA, nbz; };
    Chunks chunks(int kc) const
    {
        const int nchA = lenA > 0 ? (lenA + kc - 1) / kc : 0, nchB = lenB > 0 ? (lenB + kc - 1) / kc : 0;
        return Chunks{k0a, k1a, k0b, k1b, nchA, nchA + nchB};
    }
};

} // namespace geom
} // namespace bq
