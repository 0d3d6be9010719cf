// C entry points over csrc/host/slab_jacobi_plan.hpp for tests/test_slab_jacobi_plan_cpu.py, each for n cases given as rows of
// ints, so that an exhaustive sweep is one call.  Test infrastructure.
#include "host/slab_jacobi_plan.hpp"

using namespace bq::slab;

extern "C" {

// in: rows of (left, G, owned, pairs_ok, triples_ok, overlap_exchanges, ends_first, triples)
// out: rows of (sweeps, first, S, fused, rest, ends_first, depth_after(0), depth_after(fused - 1))
void slab_plan_chunk(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 8, out += 8) {
        const ChunkIn ci{in[0], in[1], in[2], in[3] != 0, in[4] != 0, in[5] != 0, in[6] != 0, in[7] != 0};
        const Chunk k = plan_chunk(ci);
        const int row[8] = {k.sweeps, k.first, k.S, k.fused, k.rest, k.ends_first, k.depth_after(ci.G, 0), k.depth_after(ci.G, k.fused - 1)};
        for (int m = 0; m < 8; m++) out[m] = row[m];
    }
}

// in: rows of (G, owned, d, first); out: rows of whole(d), ends(d).a, ends(d).b, interior(d), first_interior(first),
// first_ends(first).a, first_ends(first).b -- k0, k1 each
void slab_pass_planes(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 4, out += 14) {
        const int G = in[0], own0 = G, own1 = G + in[1], nk = own1 + G, d = in[2], first = in[3];
        const Ends e = ends(own0, own1, G, d), fe = first_ends(own0, own1, nk, first);
        const Planes row[7] = {whole(own0, own1, d), e.a, e.b, interior(own0, own1, G, d), first_interior(own0, own1, first), fe.a, fe.b};
        for (int m = 0; m < 7; m++) { out[2 * m] = row[m].k0; out[2 * m + 1] = row[m].k1; }
    }
}

} // extern "C"
