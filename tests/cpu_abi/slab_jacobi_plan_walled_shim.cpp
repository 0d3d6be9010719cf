// C entry point over csrc/host/slab_jacobi_plan.hpp with the walled mode for tests/test_walls_slab_plan_cpu.py: n cases given as
// rows of ints, so that an exhaustive sweep is one call.  Test infrastructure.
#include "host/slab_jacobi_plan.hpp"

using namespace bq::slab;

extern "C" {

// in: rows of (left, G, owned, pairs_ok, triples_ok, overlap_exchanges, ends_first, triples, walled)
// out: rows of (sweeps, first, S, fused, rest, ends_first, depth_after(0), depth_after(fused - 1))
void slab_plan_chunk_walled(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 9, out += 8) {
        ChunkIn ci{};
        ci.left = in[0]; ci.G = in[1]; ci.owned = in[2]; ci.pairs_ok = in[3] != 0; ci.triples_ok = in[4] != 0;
        ci.overlap_exchanges = in[5] != 0; ci.ends_first = in[6] != 0; ci.triples = in[7] != 0; ci.walled = in[8] != 0;
        const Chunk k = plan_chunk(ci);
        const int row[8] = {k.sweeps, k.first, k.S, k.fused, k.rest, k.ends_first, k.depth_after(ci.G, 0), k.depth_after(ci.G, k.fused - 1)};
        for (int m = 0; m < 8; m++) out[m] = row[m];
    }
}

} // extern "C"
