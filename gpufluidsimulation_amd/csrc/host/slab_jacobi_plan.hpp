// slab_jacobi_plan.hpp -- one chunk of the z-slab Jacobi projection as a list of passes.  An exchange of
// G ghost planes of the pressure buys up to G sweeps: every sweep leaves one ghost plane less correct on each side.  A chunk is
//   the overlapped first pass   2 sweeps in one fused launch per piece, or 1 sweep where the fused kernel is refused: the planes
//                               out of the ghost planes' reach while they travel, the two ends after the wait;
//   `fused` passes of S sweeps  S = 2 or 3, one launch each, on the planes that are still correct after the pass;
//   a tail of `rest` sweeps     through gpu_jacobi_sweeps.
// Where another chunk follows, the last two fused passes may run ENDS FIRST: their planes next to the slab ends, then the
// exchange for the next chunk starts, then their interiors (BimocqGPUSolver::projectionJacobiSlabs issues the sequence).
// With d the ghost depth still correct after a pass, every plane range below is [own0 - d, own1 + d), plus G for the ends.
// WALLED (closed domain walls): the walled kernel family has one sweep or three per launch and no pairs, so
// a walled chunk is one overlapped single sweep, triples, and a tail of `rest` sweeps through gpu_jacobi_sweeps_masked_walls.
// Pure integer arithmetic: no HIP, no solver state, no operator calls (tests/test_slab_jacobi_plan_cpu.py checks it exhaustively).
#pragma once
#include <algorithm>

namespace bq {
namespace slab {

struct ChunkIn {
    int left;               // sweeps the projection still has to do (> 0)
    int G, owned;           // ghost depth, owned planes: the rank's planes are [0, owned + 2 G), the owned ones [G, G + owned)
    bool pairs_ok;          // the grid admits two-sweep launches and none was refused in this projection
    bool triples_ok;        // no three-sweep launch was refused in this projection
    bool overlap_exchanges, ends_first, triples;        // BQ_OPT_OVERLAP_EXCHANGES, BQ_OPT_JACOBI_ENDS_FIRST, BQ_OPT_JACOBI_TRIPLES
    bool walled = false;    // the walled kernel family: singles and triples only (pairs_ok is not read)
};

struct Chunk {
    int sweeps;             // first + fused * S + rest, at most min(left, G)
    int first;              // sweeps of the overlapped first pass: 2, or 1 (the single-sweep mode)
    int S, fused;           // then `fused` passes of S sweeps each
    int rest;               // then gpu_jacobi_sweeps with `rest`
    bool ends_first;        // the last two fused passes run ends first
    int depth_after(int G, int pass) const { return G - first - (pass + 1) * S; }      // ghost planes still correct after fused pass `pass`
};

// The walled chunk: 1 + 3 * fused + rest.  Ends first needs two triples that close the chunk (no tail behind them: the planes
// the neighbours receive must be final), so a full chunk that another one follows anyway gives up its `rest` sweeps -- G = 8 runs
// 1, 3, 3 and exchanges every 7 sweeps, as the unwalled single-sweep mode does.  The interior between the two ends of the first
// of the two triples, which leaves 3 + (G - sweeps) ghost planes correct, must keep at least 2 planes.
inline Chunk plan_chunk_walled(const ChunkIn &in)
{
    Chunk c{};
    c.sweeps = std::min(in.left, in.G);
    c.first = 1;
    c.S = 3;
    const bool triples = in.triples && in.triples_ok;
    c.fused = triples ? (c.sweeps - 1) / 3 : 0;
    c.rest = c.sweeps - 1 - 3 * c.fused;
    c.ends_first = in.overlap_exchanges && in.ends_first && c.fused >= 2 && in.left > in.G &&
                   in.owned >= 2 * in.G + 2 * (3 + c.rest) + 2;
    if (c.ends_first) { c.sweeps -= c.rest; c.rest = 0; }
    return c;
}

inline Chunk plan_chunk(const ChunkIn &in)
{
    if (in.walled) return plan_chunk_walled(in);
    Chunk c{};
    c.sweeps = std::min(in.left, in.G);
    c.first = in.pairs_ok && c.sweeps >= 2 ? 2 : 1;
    // the single-sweep mode takes an odd chunk (G - 1 for even G), so that what follows it stays fusable in pairs
    if (c.first == 1) c.sweeps = std::min(in.left, in.G % 2 == 0 && in.G > 1 ? in.G - 1 : in.G);
    const int after = c.sweeps - c.first;
    const bool full = c.sweeps == in.G;
    // two triples where the fused pair left six sweeps of a full chunk (G = 8), pairs else; nothing fused in the single-sweep mode
    c.S = c.first == 2 && in.triples && in.triples_ok && in.G == 8 && full ? 3 : 2;
    c.fused = c.first == 2 ? after / c.S : 0;
    c.rest = after - c.fused * c.S;
    // ends first: an even G >= 6 leaves a full chunk at least two passes that end exactly on the owned planes; the slab must be
    // tall enough for two ends of G + S planes and an interior; and there must be a next chunk for the early exchange to serve
    c.ends_first = in.overlap_exchanges && in.ends_first && c.first == 2 && in.G >= 6 && in.G % 2 == 0 && in.owned >= 2 * in.G + 8 &&
                   full && in.left > c.sweeps;
    return c;
}

// ---- plane ranges [k0, k1) of the rank's array; own0 = G, own1 = G + owned ----
struct Planes { int k0, k1; };
struct Ends { Planes a, b; };

// a whole pass that leaves d ghost planes correct
inline Planes whole(int own0, int own1, int d) { return Planes{own0 - d, own1 + d}; }
// the same pass in three pieces: the G output planes next to either slab end with their d ghost planes, and what lies between.
// The last pass of a chunk has d = 0: its ends are the planes the neighbours receive.
inline Ends ends(int own0, int own1, int G, int d) { return Ends{Planes{own0 - d, own0 + G + d}, Planes{own1 - G - d, own1 + d}}; }
inline Planes interior(int own0, int own1, int G, int d) { return Planes{own0 + G + d, own1 - G - d}; }
// the first pass of `first` sweeps: the outputs whose stencil stays inside the owned planes, and after the wait everything else
inline Planes first_interior(int own0, int own1, int first) { return Planes{own0 + first, own1 - first}; }
inline Ends first_ends(int own0, int own1, int nk, int first) { return Ends{Planes{0, own0 + first}, Planes{own1 - first, nk}}; }

} // namespace slab
} // namespace bq
