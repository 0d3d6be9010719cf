// C entry points over csrc/bq_jacobi_plan.h for tests/test_jacobi_plan_cpu.py: the decoder, the planners and the fp64 split, each
// for n cases given as rows of ints, so that an exhaustive sweep is one call.  Test infrastructure.
#include "bq_jacobi_plan.h"

using namespace bq;
using namespace bq::plan;

extern "C" {

// in: rows of (variant, rows, kchunk, kchunk2, fuse); out: rows of the 28 fields in the order of tests/test_jacobi_plan_cpu.py: FIELDS
void plan_decode(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 5, out += 28) {
        const JacobiTuning t = decode_jacobi_tuning(in[0], in[1], in[2], in[3], in[4]);
        const int row[28] = {(int)t.single, t.march_waves, t.tile_rows, t.single_kchunk, t.fused_ok, (int)t.pair_rows, t.keep_march2r, t.prefetch,
                             t.fused_kchunk, t.lds_min_kc, t.lds_triple, t.lean_triple, t.lean_triple_short, (int)t.quad, t.lds_w[0], t.lds_r[0],
                             t.lds_w[1], t.lds_r[1], t.masked_triple, t.triple_ranges, t.pair_ranges, (int)t.trust, t.beyond_pairs,
                             (int)t.sweeps_fuse, t.mg_keep_smooth2, t.mg_smooth2_threads, t.mg_lds3_off, t.mg_lds3_rows};
        for (int m = 0; m < 28; m++) out[m] = row[m];
    }
}

// in: rows of (planner, ni, nj, nk, aligned16, k0a, k1a, k0b, k1b, variant, rows, kchunk, kchunk2, fuse, num_cus, slab_on, S, masked, min_kc)
// planner: 0 single, 1 pair, 2 lds, 3 quad, 4 lean triple, 5 triple, 6 masked triple, 7 triple on ranges
// out: rows of (kernel, wide, pf, W, R, S, cw, col_blocks, row_blocks, nbz, kc, nblk, grid, block)
void plan_launch(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 19, out += 14) {
        const int ni = in[1], nj = in[2], nk = in[3], cus = in[14];
        const bool al = in[4] != 0, slab = in[15] != 0;
        const geom::PlaneRanges pr(in[5], in[6], in[7], in[8], nk);
        const JacobiTuning t = decode_jacobi_tuning(in[9], in[10], in[11], in[12], in[13]);
        LaunchPlan p;
        switch (in[0]) {
        case 0: p = plan_single(ni, nj, nk, al, t); break;
        case 1: p = plan_pair(ni, nj, nk, al, pr, t, cus); break;
        case 2: p = plan_lds(ni, nj, nk, al, pr, t, cus, in[16], in[17] != 0, in[18]); break;
        case 3: p = plan_quad(ni, nj, nk, al, t, cus, slab); break;
        case 4: p = plan_lean_triple(ni, nj, nk, al, t, cus); break;
        case 5: p = plan_triple(ni, nj, nk, al, t, cus); break;
        case 6: p = plan_triple_masked(ni, nj, nk, al, t, cus, slab); break;
        default: p = plan_triple_ranges(ni, nj, nk, al, pr, t, cus); break;
        }
        const int row[14] = {(int)p.kernel, p.wide, p.pf, p.W, p.R, p.S, p.cw, p.col_blocks, p.row_blocks, p.nbz, p.kc, p.nblk, p.grid, p.block};
        for (int m = 0; m < 14; m++) out[m] = row[m];
    }
}

// in: rows of (iter, s, zin); out: rows of (triples, pairs, swap_first)
void plan_mg_lds3_split(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 3, out += 3) {
        const MgLds3Split sp = mg_lds3_split(in[0], in[1], in[2] != 0);
        out[0] = sp.triples; out[1] = sp.pairs; out[2] = sp.swap_first;
    }
}

} // extern "C"
