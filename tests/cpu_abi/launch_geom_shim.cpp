// C entry points over csrc/bq_launch_geom.h for tests/test_launch_geom_cpu.py: each evaluates one rule of the header for n
// cases given as parallel arrays, so that an exhaustive sweep is one call.  Test infrastructure.
#include "bq_launch_geom.h"

using namespace bq::geom;

extern "C" {

void geom_pow2_lanes(int n, const int *ni, const int *per_lane, const int *cap, int *out)
{
    for (int c = 0; c < n; c++) out[c] = cap[c] > 0 ? pow2_lanes(ni[c], per_lane[c], cap[c]) : pow2_lanes(ni[c], per_lane[c]);
}

void geom_whole_round_chunks(int n, const int *row_blocks, const int *planes, const int *target, const int *round, int *out)
{
    for (int c = 0; c < n; c++) out[c] = whole_round_chunks(row_blocks[c], planes[c], target[c], round[c]);
}

void geom_chunks_for_cus(int n, const int *nkr, const int *nrow, const int *target, const int *warm, const int *ncus,
                         const int *per_cu, int *out)
{
    for (int c = 0; c < n; c++) out[c] = chunks_for_cus(nkr[c], nrow[c], target[c], warm[c], ncus[c], per_cu[c]);
}

void geom_once_per_cu_len(int n, const int *longest, const int *row_blocks, const int *nranges, const int *ncus, int *out)
{
    for (int c = 0; c < n; c++) out[c] = once_per_cu_len(longest[c], row_blocks[c], nranges[c], ncus[c]);
}

// in: rows of (k0a, k1a, k0b, k1b, nk, kc); out: rows of (k0a, k1a, k0b, k1b, lenA, lenB, planes, whole, nranges, longest, nchA, nbz)
void geom_plane_ranges(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 6, out += 12) {
        const PlaneRanges pr(in[0], in[1], in[2], in[3], in[4]);
        const PlaneRanges::Chunks ch = pr.chunks(in[5]);
        const int row[12] = {ch.k0a, ch.k1a, ch.k0b, ch.k1b, pr.lenA, pr.lenB, pr.planes, pr.whole ? 1 : 0, pr.nranges, pr.longest,
                             ch.nchA, ch.nbz};
        for (int m = 0; m < 12; m++) out[m] = row[m];
    }
}

} // extern "C"
