/*
 * flow_stats_abi.c -- TEST-ONLY C restatement of gpu_flow_stats of include/bimocq_gpu.h.
 *
 * Linked on top of the MacCormack stand-in's list into tests/_build/libbimocq_host_cpu_diag.so (tests/build_cpu_diag.py): the
 * CPU stand-in on which the host solver's diagnostics run without a GPU, and against which the GPU tests compare the HIP
 * kernels.  Written from the header's definitions, one statement per IEEE operation, cells visited in k, j, i order and the
 * sums taken in that order (the kernels sum in another one: the tests bound the difference).
 *
 *   flow_stats_abi_terms     the per-cell terms on their own: e2, m2 (double), d, mag (float) of every cell of the local buffer
 *                            under an explicit slab context (nkg <= 0: one domain) -- what a test sums exactly
 *   flow_stats_abi_set_slab  the z-slab context gpu_flow_stats evaluates under (nkg <= 0: off).  oracle_abi.c keeps the one
 *                            the host solver sets (fl_set_slab) to itself, so a slab worker hands the same numbers over
 *                            (bq_solver_slab_info); flow_stats_abi_set_allreduce likewise for the transport's all-reduce
 *   flow_stats_abi_calls     how many calls have been made (reset != 0: back to 0) -- a test's proof that a step with
 *                            BQ_OPT_DIAGNOSTICS_EVERY = 0 launches nothing
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/bimocq_gpu.h"

static long g_calls = 0;
static int s_on = 0, s_koff = 0, s_nkg = 0, s_own0 = 0, s_own1 = 0;
static fl_allreduce_cb s_allreduce = NULL;
static int s_nranks = 1;

long flow_stats_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

void flow_stats_abi_set_slab(int koff, int nk_global, int own0, int own1)
{
    s_on = nk_global > 0; s_koff = koff; s_nkg = nk_global; s_own0 = own0; s_own1 = own1;
}

void flow_stats_abi_set_allreduce(fl_allreduce_cb cb, int nranks)
{
    s_allreduce = cb; s_nranks = nranks;
}

#define IU(i, j, k) ((size_t)(i) + (size_t)(ni + 1) * ((size_t)(j) + (size_t)nj * (size_t)(k)))
#define IV(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)(nj + 1) * (size_t)(k)))
#define IC(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)nj * (size_t)(k)))

static float cen_u(const float *u, int ni, int nj, int i, int j, int k) { float s = u[IU(i, j, k)] + u[IU(i + 1, j, k)]; return 0.5f * s; }
static float cen_v(const float *v, int ni, int nj, int i, int j, int k) { float s = v[IV(i, j, k)] + v[IV(i, j + 1, k)]; return 0.5f * s; }
static float cen_w(const float *w, int ni, int nj, int i, int j, int k) { float s = w[IC(i, j, k)] + w[IC(i, j, k + 1)]; return 0.5f * s; }

/* one cell of the local buffer; returns 0 when its plane lies outside the global grid (nothing defined there) */
static int cell_terms(const float *u, const float *v, const float *w, float h, int ni, int nj, int nk, int koff, int nkg,
                      int i, int j, int k, double *e2, double *m2, float *d, float *mag)
{
    const int kg = k + koff;
    *e2 = 0.0; *m2 = 0.0; *d = 0.f; *mag = 0.f;
    if (kg < 0 || kg >= nkg) return 0;
    const float uc = cen_u(u, ni, nj, i, j, k), vc = cen_v(v, ni, nj, i, j, k), wc = cen_w(w, ni, nj, i, j, k);
    const float du = u[IU(i + 1, j, k)] - u[IU(i, j, k)];
    const float dv = v[IV(i, j + 1, k)] - v[IV(i, j, k)];
    const float dw = w[IC(i, j, k + 1)] - w[IC(i, j, k)];
    const float s1 = du + dv;
    const float s2 = s1 + dw;
    *d = s2 / h;
    float wx = 0.f, wy = 0.f, wz = 0.f;
    /* (a stored plane whose neighbour plane is not stored counts as border; owned planes always have both) */
    if (i >= 1 && i <= ni - 2 && j >= 1 && j <= nj - 2 && kg >= 1 && kg <= nkg - 2 && k >= 1 && k <= nk - 2) {
        const float q = 2.0f * h;
        const float a1 = cen_w(w, ni, nj, i, j + 1, k) - cen_w(w, ni, nj, i, j - 1, k);
        const float b1 = cen_v(v, ni, nj, i, j, k + 1) - cen_v(v, ni, nj, i, j, k - 1);
        const float c1 = a1 - b1;
        wx = c1 / q;
        const float a2 = cen_u(u, ni, nj, i, j, k + 1) - cen_u(u, ni, nj, i, j, k - 1);
        const float b2 = cen_w(w, ni, nj, i + 1, j, k) - cen_w(w, ni, nj, i - 1, j, k);
        const float c2 = a2 - b2;
        wy = c2 / q;
        const float a3 = cen_v(v, ni, nj, i + 1, j, k) - cen_v(v, ni, nj, i - 1, j, k);
        const float b3 = cen_u(u, ni, nj, i, j + 1, k) - cen_u(u, ni, nj, i, j - 1, k);
        const float c3 = a3 - b3;
        wz = c3 / q;
    }
    double t = (double)wx * (double)wx;
    t = t + (double)wy * (double)wy;
    t = t + (double)wz * (double)wz;
    *m2 = t;
    double e = (double)uc * (double)uc;
    e = e + (double)vc * (double)vc;
    e = e + (double)wc * (double)wc;
    *e2 = e;
    *mag = (float)sqrt(t);
    return 1;
}

void flow_stats_abi_terms(const float *u, const float *v, const float *w, float h, int ni, int nj, int nk, int koff, int nkg,
                          double *e2, double *m2, float *d, float *mag)
{
    if (nkg <= 0) { koff = 0; nkg = nk; }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                double e, m; float dd, mg;
                cell_terms(u, v, w, h, ni, nj, nk, koff, nkg, i, j, k, &e, &m, &dd, &mg);
                const size_t ic = IC(i, j, k);
                if (e2) e2[ic] = e;
                if (m2) m2[ic] = m;
                if (d) d[ic] = dd;
                if (mag) mag[ic] = mg;
            }
}

static int ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return 0;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

int gpu_flow_stats(const float *u, const float *v, const float *w, const float *rho, const float *T, float *vort_mag,
                   float h, int ni, int nj, int nk, double *d_out)
{
    if (!u || !v || !w || !d_out) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_flow_stats: null velocity or d_out"); return FL_ERR_BAD_ARGUMENT; }
    if (ni < 3 || nj < 3 || nk < 3) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_flow_stats: dims below 3"); return FL_ERR_BAD_ARGUMENT; }
    const size_t nc = (size_t)ni * nj * nk * sizeof(float);
    if (vort_mag && (ranges_overlap(vort_mag, nc, u, (size_t)(ni + 1) * nj * nk * sizeof(float)) ||
                     ranges_overlap(vort_mag, nc, v, (size_t)ni * (nj + 1) * nk * sizeof(float)) ||
                     ranges_overlap(vort_mag, nc, w, (size_t)ni * nj * (nk + 1) * sizeof(float)) ||
                     ranges_overlap(vort_mag, nc, rho, nc) || ranges_overlap(vort_mag, nc, T, nc) ||
                     ranges_overlap(vort_mag, nc, d_out, BQ_STAT_COUNT * sizeof(double)))) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_flow_stats: vort_mag aliases an input");
        return FL_ERR_BAD_ARGUMENT;
    }
    g_calls++;
    const int koff = s_on ? s_koff : 0, nkg = s_on ? s_nkg : nk;
    const int own0 = s_on ? s_own0 : 0, own1 = s_on ? s_own1 : nk;
    double S[BQ_STAT_COUNT];
    for (int a = 0; a < BQ_STAT_COUNT; a++) S[a] = 0.0;
    float dmax = 0.f, mmax = 0.f;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                double e, m; float dd, mg;
                const int inside = cell_terms(u, v, w, h, ni, nj, nk, koff, nkg, i, j, k, &e, &m, &dd, &mg);
                const size_t ic = IC(i, j, k);
                const int kg = k + koff;
                if (vort_mag) vort_mag[ic] = mg;
                if (!inside || kg < own0 || kg >= own1) continue;
                S[BQ_STAT_E2] += e;
                S[BQ_STAT_M2] += m;
                S[BQ_STAT_D2] += (double)dd * (double)dd;
                dmax = fmaxf(dmax, fabsf(dd));
                mmax = fmaxf(mmax, mg);
                if (rho) {
                    const double r = (double)rho[ic];
                    S[BQ_STAT_RHO] += r;
                    S[BQ_STAT_RHO_I] += r * (double)i;
                    S[BQ_STAT_RHO_J] += r * (double)j;
                    S[BQ_STAT_RHO_K] += r * (double)kg;
                }
                if (T) S[BQ_STAT_T] += (double)T[ic];
            }
    S[BQ_STAT_DIV_MAX] = (double)dmax;
    S[BQ_STAT_VORT_MAX] = (double)mmax;
    if (s_nranks > 1 && s_allreduce) {          /* owned planes -> the grid: sums and maxima lie interleaved */
        s_allreduce(S + 0, 3, 1, 0);
        s_allreduce(S + 3, 1, 1, 1);
        s_allreduce(S + 4, 5, 1, 0);
        s_allreduce(S + 9, 1, 1, 1);
    }
    for (int a = 0; a < BQ_STAT_COUNT; a++) d_out[a] = S[a];
    return FL_OK;
}
