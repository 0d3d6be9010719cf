// C entry points over csrc/bq_mgcg_slab_plan.h for tests/test_mgcg_slab_plan_cpu.py, each for n cases given as rows of ints, so
// that a sweep over every geometry and rank is one call.  Test infrastructure.
#include "bq_mgcg_slab_plan.h"

using namespace bq::mgslab;

extern "C" {

int mgcg_slab_plan_levels(void) { return kLevels; }
int mgcg_slab_plan_row_ints(void) { return 8 + 16 * kLevels; }
int mgcg_slab_table_row_ints(void) { return 8 * (2 * (kMaxShared + 1) + 2); }

// in: rows of (ni, nj, nkg, ghost, rank, nranks)
// out: rows of (supported, nlevels, LS, dot_first, dot_nb_own, dot_nb, k_first, k_end), then per level 0 .. kLevels - 1
//      (ni, nj, nk, own0, own1, lo, hi, G, rest_c0, rest_ck, rest_fine0, rest_fine_planes, prol_c0, prol_ck, xch_shift, xch_nk_local)
void mgcg_slab_plan_rows(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 6) {
        const Plan p = make_plan(in[0], in[1], in[2], in[3], in[4], in[5]);
        const int head[8] = { p.supported, p.nlevels, p.LS, (int)p.dot_first, (int)p.dot_nb_own, (int)p.dot_nb, p.k_first, p.k_end };
        for (int m = 0; m < 8; m++) *out++ = head[m];
        for (int l = 0; l < kLevels; l++) {
            const Level &L = p.lv[l];
            const int row[16] = { L.ni, L.nj, L.nk, L.own0, L.own1, L.lo, L.hi, L.G, L.rest_c0, L.rest_ck, L.rest_fine0, L.rest_fine_planes,
                                  L.prol_c0, L.prol_ck, L.xch_shift, L.xch_nk_local };
            for (int m = 0; m < 16; m++) *out++ = row[m];
        }
    }
}

// the tables of all ranks as the plan of rank in[4] holds them.  in: rows as above (nranks <= 8)
// out: per rank r = 0 .. 7 (zeros from nranks on): own(r, l).a, own(r, l).b for l = 0 .. kMaxShared, dot_first_of(r), dot_nb_of(r)
void mgcg_slab_plan_tables(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 6) {
        const Plan p = make_plan(in[0], in[1], in[2], in[3], in[4], in[5]);
        for (int r = 0; r < 8; r++) {
            const bool live = p.supported && r < p.nranks;
            for (int l = 0; l <= kMaxShared; l++) {
                const Range o = live && l <= p.LS ? p.own(r, l) : Range{ 0, 0 };
                *out++ = o.a; *out++ = o.b;
            }
            *out++ = live ? (int)p.dot_first_of(r) : 0;
            *out++ = live ? (int)p.dot_nb_of(r) : 0;
        }
    }
}

// gpu_mgcg_slab_supported's answer.  in: rows of (ni, nj, nkg, own0, own1, ghost, rank, nranks); out: one int per row
void mgcg_slab_supported_rows(int n, const int *in, int *out)
{
    for (int c = 0; c < n; c++, in += 8) out[c] = supported(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7]) ? 1 : 0;
}

} // extern "C"
