/*
 * pcg_abi.c -- TEST-ONLY C restatement of the PCG projection operators of include/bimocq_gpu.h:
 * gpu_divergence_double, gpu_pcg_solve, gpu_pcg_gradient.
 *
 * Linked with oracle_abi.c, obstacle_abi.c, levelset_abi.c and the oracle into tests/_build/libbimocq_host_cpu_pcg.so
 * (tests/build_cpu_pcg.py): the CPU stand-in on which the host solver's kind-2 projection runs without a GPU, and against
 * which the GPU tests compare the HIP kernels bit for bit.  Written from the section 15 contract: level 0 and the CG
 * recurrences are restated here, the coarse levels call the oracle's orc_mg_smooth / orc_mg_residual / orc_mg_restrict /
 * orc_mg_prolong, and the reductions follow the contract's fixed trees (a block of 256 lanes per 2048 cells, lane t
 * taking cells t, t + 256, ...; the lanes' values meet pairwise at distances 128, 64, ..., 1).
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

void fl_report_error(int code, const char *text);

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))
#define LANES 256
#define CELLS (LANES * 8)
#define UNKNOWN 0x8000u
#define DMAX 1.7976931348623157e308

void gpu_divergence_double(const float *u, const float *v, const float *w, double *div, int ni, int nj, int nk, double halfrdx)
{
    if (!u || !v || !w || !div || ni < 1 || nj < 1 || nk < 1) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_divergence_double"); return; }
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                double ul = u[IDX(i, j, k, ni + 1, nj)], ur = u[IDX(i + 1, j, k, ni + 1, nj)];
                double vf = v[IDX(i, j, k, ni, nj + 1)], vb = v[IDX(i, j + 1, k, ni, nj + 1)];
                double wd = w[IDX(i, j, k, ni, nj)], wu = w[IDX(i, j, k + 1, ni, nj)];
                div[IDX(i, j, k, ni, nj)] = halfrdx * ((ur - ul) + (vb - vf) + (wu - wd));
            }
}

void gpu_pcg_gradient(float *u, float *v, float *w, const double *p, const unsigned char *solid, int ni, int nj, int nk, double halfrdx)
{
    if (!u || !v || !w || !p || ni < 1 || nj < 1 || nk < 1) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_pcg_gradient"); return; }
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 2; k < nk; k++)
        for (int j = 2; j < nj; j++)
            for (int i = 2; i < ni; i++) {
                size_t c = IDX(i, j, k, ni, nj);
                int fc = !solid || solid[c] == 0;
                double p0 = p[c];
                if (fc && (!solid || solid[IDX(i - 1, j, k, ni, nj)] == 0))
                    u[IDX(i, j, k, ni + 1, nj)] -= (float)(halfrdx * (p0 - p[IDX(i - 1, j, k, ni, nj)]));
                if (fc && (!solid || solid[IDX(i, j - 1, k, ni, nj)] == 0))
                    v[IDX(i, j, k, ni, nj + 1)] -= (float)(halfrdx * (p0 - p[IDX(i, j - 1, k, ni, nj)]));
                if (fc && (!solid || solid[IDX(i, j, k - 1, ni, nj)] == 0))
                    w[IDX(i, j, k, ni, nj)] -= (float)(halfrdx * (p0 - p[IDX(i, j, k - 1, ni, nj)]));
            }
}

/* ---- the solve --------------------------------------------------------------------------------------------------- */
typedef struct { int ni, nj, nk; size_t n; int nparts; const uint16_t *code; double w[7], omw; } Grid;

static int interior(const Grid *g, int i, int j, int k) { return i > 0 && i < g->ni - 1 && j > 0 && j < g->nj - 1 && k > 0 && k < g->nk - 1; }

/* bit 15: unknown (interior, fluid, s < 6); bits 8..10: s solid neighbours; bit q: neighbour q (-x +x -y +y -z +z) unknown */
static void make_codes(const Grid *g, const unsigned char *solid, uint16_t *code)
{
    const int ni = g->ni, nj = g->nj, nk = g->nk;
#pragma omp parallel for collapse(2) schedule(static)
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                size_t c = IDX(i, j, k, ni, nj);
                if (!interior(g, i, j, k) || (solid && solid[c])) { code[c] = 0; continue; }
                int nb[6][3] = { { i - 1, j, k }, { i + 1, j, k }, { i, j - 1, k }, { i, j + 1, k }, { i, j, k - 1 }, { i, j, k + 1 } };
                unsigned s = 0, bits = 0;
                for (int q = 0; q < 6; q++) {
                    if (solid && solid[IDX(nb[q][0], nb[q][1], nb[q][2], ni, nj)]) s++;
                    else if (interior(g, nb[q][0], nb[q][1], nb[q][2])) bits |= 1u << q;
                }
                code[c] = (uint16_t)(s == 6 ? 0u : (UNKNOWN | (s << 8) | bits));
            }
}

static double nb_sum(const Grid *g, const double *x, size_t c, unsigned code)
{
    size_t sj = (size_t)g->ni, sk = (size_t)g->ni * g->nj;
    double acc = 0.0;
    acc = acc + ((code & 1u) ? x[c - 1] : 0.0);
    acc = acc + ((code & 2u) ? x[c + 1] : 0.0);
    acc = acc + ((code & 4u) ? x[c - sj] : 0.0);
    acc = acc + ((code & 8u) ? x[c + sj] : 0.0);
    acc = acc + ((code & 16u) ? x[c - sk] : 0.0);
    acc = acc + ((code & 32u) ? x[c + sk] : 0.0);
    return acc;
}

static double a_times(const Grid *g, const double *x, size_t c, unsigned code)
{
    return (double)(6 - (int)((code >> 8) & 7u)) * x[c] - nb_sum(g, x, c, code);
}

/* one weighted-Jacobi sweep of A z = rhs; first: from z = 0 */
static void smooth(const Grid *g, const double *in, const double *rhs, double *out, int first)
{
#pragma omp parallel for schedule(static)
    for (size_t c = 0; c < g->n; c++) {
        unsigned code = g->code[c];
        if (!(code & UNKNOWN)) { out[c] = 0.0; continue; }
        double w = g->w[(code >> 8) & 7u];
        if (first) { out[c] = rhs[c] * w; continue; }
        double acc = nb_sum(g, in, c, code);
        out[c] = g->omw * in[c] + (acc + rhs[c]) * w;
    }
}

static double tree(double *v, int is_max)
{
    for (int s = LANES / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; t++) v[t] = is_max ? fmax(v[t], v[t + s]) : v[t] + v[t + s];
    return v[0];
}

/* the final reduction of nparts partials */
static double final_reduce(const double *part, int nparts, int is_max)
{
    double v[LANES];
    for (int t = 0; t < LANES; t++) {
        double s = 0.0;
        for (int q = t; q < nparts; q += LANES) s = is_max ? fmax(s, part[q]) : s + part[q];
        v[t] = s;
    }
    return tree(v, is_max);
}

/* per reduction block: lane values over cells b*2048 + e*256 + t, e = 0..7, then the tree.  kind: 0 max|b| of init,
 * 1 apply (q = A d, d.q), 2 update (max|r|), 3 z.r, 4 z.q */
static void init_blocks(const Grid *g, const double *div, double *r, double *p, double *part)
{
#pragma omp parallel for schedule(static)
    for (int b = 0; b < g->nparts; b++) {
        double v[LANES];
        for (int t = 0; t < LANES; t++) {
            double m = 0.0;
            for (int e = 0; e < 8; e++) {
                size_t c = (size_t)b * CELLS + (size_t)e * LANES + t;
                if (c >= g->n) break;
                double bb = (g->code[c] & UNKNOWN) ? -div[c] : 0.0;
                r[c] = bb;
                p[c] = 0.0;
                m = fmax(m, fabs(bb));
            }
            v[t] = m;
        }
        part[b] = tree(v, 1);
    }
}

static void apply_blocks(const Grid *g, const double *d, double *q, double *part)
{
#pragma omp parallel for schedule(static)
    for (int b = 0; b < g->nparts; b++) {
        double v[LANES];
        for (int t = 0; t < LANES; t++) {
            double s = 0.0;
            for (int e = 0; e < 8; e++) {
                size_t c = (size_t)b * CELLS + (size_t)e * LANES + t;
                if (c >= g->n) break;
                unsigned code = g->code[c];
                double val = (code & UNKNOWN) ? a_times(g, d, c, code) : 0.0;
                q[c] = val;
                s = s + d[c] * val;
            }
            v[t] = s;
        }
        part[b] = tree(v, 0);
    }
}

static void update_blocks(const Grid *g, double *p, double *r, const double *d, const double *q, double alpha, double *part)
{
#pragma omp parallel for schedule(static)
    for (int b = 0; b < g->nparts; b++) {
        double v[LANES];
        for (int t = 0; t < LANES; t++) {
            double m = 0.0;
            for (int e = 0; e < 8; e++) {
                size_t c = (size_t)b * CELLS + (size_t)e * LANES + t;
                if (c >= g->n) break;
                p[c] = p[c] + alpha * d[c];
                double rn = r[c] - alpha * q[c];
                r[c] = rn;
                m = fmax(m, fabs(rn));
            }
            v[t] = m;
        }
        part[b] = tree(v, 1);
    }
}

static void dot_blocks(const Grid *g, const double *z, const double *x, double *part)
{
#pragma omp parallel for schedule(static)
    for (int b = 0; b < g->nparts; b++) {
        double v[LANES];
        for (int t = 0; t < LANES; t++) {
            double s = 0.0;
            for (int e = 0; e < 8; e++) {
                size_t c = (size_t)b * CELLS + (size_t)e * LANES + t;
                if (c >= g->n) break;
                s = s + z[c] * x[c];
            }
            v[t] = s;
        }
        part[b] = tree(v, 0);
    }
}

/* mgcg_pcg_coarse (bq_mgcg.hip) through the oracle: levels 1 .. levelnum-1 */
static void coarse_cycle(const SCoarseLevelInfo *L, int levelnum, double *temp, int down, int up, int bottom)
{
    const int c = levelnum - 1;
    for (int l = 1; l < c; l++) {
        memset(temp, 0, (size_t)L[l].number * sizeof(double));
        memset(L[l].x, 0, (size_t)L[l].number * sizeof(double));
        orc_mg_smooth(L[l].x, L[l].b, temp, L[l].alpha, L[l].beta, L[l].ni, L[l].nj, L[l].nk, down);
        orc_mg_residual(L[l].r, L[l].b, L[l].x, L[l].ni, L[l].nj, L[l].nk);
        orc_mg_restrict(L[l].r, L[l + 1].b, L[l].ni, L[l].nj, L[l].nk, L[l + 1].ni, L[l + 1].nj, L[l + 1].nk);
        for (int q = 0; q < L[l + 1].number; q++) L[l + 1].b[q] = L[l + 1].b[q] * 4.0;
    }
    memset(temp, 0, (size_t)L[c].number * sizeof(double));
    memset(L[c].x, 0, (size_t)L[c].number * sizeof(double));
    orc_mg_smooth(L[c].x, L[c].b, temp, L[c].alpha, L[c].beta, L[c].ni, L[c].nj, L[c].nk, bottom);
    for (int l = c - 1; l >= 1; --l) {
        orc_mg_prolong(L[l].x, L[l + 1].x, L[l].ni, L[l].nj, L[l].nk, L[l + 1].ni, L[l + 1].nj, L[l + 1].nk);
        memset(temp, 0, (size_t)L[l].number * sizeof(double));
        orc_mg_smooth(L[l].x, L[l].b, temp, L[l].alpha, L[l].beta, L[l].ni, L[l].nj, L[l].nk, up);
    }
}

static void precondition(const Grid *g, const double *r, double *z, double *t, const SCoarseLevelInfo *L, int levelnum)
{
    smooth(g, NULL, r, t, 1);
    smooth(g, t, r, z, 0);
    if (levelnum >= 2) {
#pragma omp parallel for schedule(static)
        for (size_t c = 0; c < g->n; c++) {
            unsigned code = g->code[c];
            t[c] = (code & UNKNOWN) ? 4.0 * (a_times(g, z, c, code) - r[c]) : 0.0;
        }
        orc_mg_restrict(t, L[1].b, g->ni, g->nj, g->nk, L[1].ni, L[1].nj, L[1].nk);
        coarse_cycle(L, levelnum, t, 4, 4, 32);
        orc_mg_prolong(z, L[1].x, g->ni, g->nj, g->nk, L[1].ni, L[1].nj, L[1].nk);
    }
    smooth(g, z, r, t, 0);
    smooth(g, t, r, z, 0);
}

static int pos_finite(double v) { return v > 0.0 && v <= DMAX; }

void gpu_pcg_solve(const double *div, double *p, const unsigned char *solid, double *r, double *d, double *q, double *z,
                   double *t, double *work, struct SCoarseLevelInfo *levels, int levelNum, int iters, double tol, double *stats)
{
    if (stats) { stats[0] = 0; stats[1] = 0; stats[2] = 0; stats[3] = BQ_PCG_BREAKDOWN; }
    if (!div || !p || !r || !d || !q || !z || !t || !work || !levels || !stats || levelNum < 1 || levelNum > LEVEL_COUNT ||
        iters < 0 || !(tol > 0.0 && tol < 1.0)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_pcg_solve");
        return;
    }
    Grid g;
    g.ni = levels[0].ni; g.nj = levels[0].nj; g.nk = levels[0].nk;
    if (g.ni < 3 || g.nj < 3 || g.nk < 3 || (long long)g.ni * g.nj * g.nk != (long long)levels[0].number) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_pcg_solve");
        return;
    }
    g.n = (size_t)levels[0].number;
    g.nparts = (int)((g.n + CELLS - 1) / CELLS);
    uint16_t *code = (uint16_t *)work;
    g.code = code;
    const double omega = 6.0 / 7.0;
    for (int s = 0; s < 6; s++) g.w[s] = omega / (double)(6 - s);
    g.w[6] = 0.0;
    g.omw = 1.0 - omega;
    double *part = malloc((size_t)g.nparts * 2 * sizeof(double));
    for (int l = 1; l < levelNum; l++) {
        size_t bytes = (size_t)levels[l].number * sizeof(double);
        memset(levels[l].b, 0, bytes); memset(levels[l].x, 0, bytes); memset(levels[l].r, 0, bytes);
    }
    make_codes(&g, solid, code);
    init_blocks(&g, div, r, p, part);
    const double maxb = final_reduce(part, g.nparts, 1);
    stats[1] = stats[2] = maxb;
    if (maxb == 0.0) { stats[3] = BQ_PCG_CONVERGED; free(part); return; }
    if (!(maxb <= DMAX)) { free(part); return; }
    precondition(&g, r, z, t, levels, levelNum);
    dot_blocks(&g, z, r, part);
    double rho = final_reduce(part, g.nparts, 0);
    int okb = pos_finite(rho);
    memcpy(d, z, g.n * sizeof(double));
    int it = 0;
    double reason = BQ_PCG_ITER_LIMIT, maxr = maxb, alpha = 0.0;
    for (; it < iters; it++) {
        apply_blocks(&g, d, q, part);
        double dq = final_reduce(part, g.nparts, 0);
        int oka = pos_finite(rho) && pos_finite(dq);
        alpha = oka ? rho / dq : 0.0;
        if (!okb || !oka) { reason = BQ_PCG_BREAKDOWN; break; }
        update_blocks(&g, p, r, d, q, alpha, part);
        maxr = final_reduce(part, g.nparts, 1);
        if (maxr <= tol * maxb) { reason = BQ_PCG_CONVERGED; it++; break; }
        if (it + 1 == iters) { it++; break; }
        precondition(&g, r, z, t, levels, levelNum);
        dot_blocks(&g, z, r, part);
        dot_blocks(&g, z, q, part + g.nparts);
        double rho_new = final_reduce(part, g.nparts, 0), zq = final_reduce(part + g.nparts, g.nparts, 0);
        okb = pos_finite(rho_new) && zq - zq == 0.0;
        double beta = okb ? -(alpha * zq) / rho : 0.0;
        rho = rho_new;
        if (okb)
            for (size_t c = 0; c < g.n; c++) d[c] = z[c] + beta * d[c];
    }
    if (iters == 0 && !okb) reason = BQ_PCG_BREAKDOWN;
    stats[0] = it;
    stats[1] = maxr;
    stats[3] = reason;
    free(part);
}
