/*
 * walls_slab_abi.c -- TEST-ONLY C restatement of the wall operators of include/bimocq_gpu.h as a z-slab rank sees them
 * (DESIGN.md section 18): gpu_wall_flags, gpu_wall_faces, the walled sweeps and gpu_gradient_masked_walls under the slab
 * context of fl_set_slab, and the two sweeps on plane ranges.  It takes the place of walls_abi.c in
 * tests/_build/libbimocq_host_cpu_walls_slab.so (tests/build_cpu_walls_slab.py): the stand-in on which the host solver's
 * walled slab projection runs without a GPU, and against which the GPU tests compare the HIP kernels bit for bit.
 *
 * Written loop by loop from the contract, not from the kernels: a sweep is gpu_jacobi_sweep_masked's loop on solidw over
 * the planes that are interior planes of the GLOBAL grid, and never looks at `rows` or `walls`.
 *
 * The slab context and the log of a slab projection's schedule are file-static in oracle_abi.c, so that file is part of
 * this translation unit (the build script leaves it out of the link).
 */
#include "oracle_abi.c"

#define WIDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

/* local plane k is global plane k + w_koff() of w_nkg(nk) */
static int w_koff(void) { return s_on ? s_koff : 0; }
static int w_nkg(int nk) { return s_on ? s_nkg : nk; }

/* tests: 0 makes gpu_jacobi_sweep_masked_walls_triple_ranges refuse every shape, as the HIP library refuses wide rows */
static int w_triples = 1;
void abi_walled_triples(int on) { w_triples = on; }

/* :938-948 in global coordinates; the planes of the array outside the global grid hold no cell */
void gpu_wall_flags(unsigned char *solidw, const unsigned char *solid, int walls, int ni, int nj, int nk)
{
    const int koff = w_koff(), nkg = w_nkg(nk);
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                const int kg = k + koff;
                int border = ((walls & BQ_WALL_XLO) && i == 0) || ((walls & BQ_WALL_XHI) && i == ni - 1) ||
                             ((walls & BQ_WALL_YLO) && j == 0) || ((walls & BQ_WALL_YHI) && j == nj - 1) ||
                             ((walls & BQ_WALL_ZLO) && kg == 0) || ((walls & BQ_WALL_ZHI) && kg == nkg - 1);
                if (kg < 0 || kg >= nkg) border = 0;
                unsigned char f = solid ? solid[WIDX(i, j, k, ni, nj)] : 0;
                solidw[WIDX(i, j, k, ni, nj)] = f ? f : (unsigned char)(border ? BQ_FLAG_WALL : 0);
            }
}

/* the flag of cell (i, j, k): 0 outside the global grid; a cell of the grid below or above the window carries the flag of
 * its neighbour inside the window (the header's rule for the w faces of the window's first and last plane) */
static int w_flag(const unsigned char *s, int i, int j, int k, int ni, int nj, int nk)
{
    if (i < 0 || j < 0 || i >= ni || j >= nj) return 0;
    const int kg = k + w_koff();
    if (kg < 0 || kg >= w_nkg(nk)) return 0;
    if (k < 0) k = 0;
    if (k >= nk) k = nk - 1;
    return s[WIDX(i, j, k, ni, nj)];
}

/* the flag as the gradient reads it: 0 outside the array */
static int w_in(const unsigned char *s, int i, int j, int k, int ni, int nj, int nk)
{
    if (i < 0 || j < 0 || k < 0 || i >= ni || j >= nj || k >= nk) return 0;
    return s[WIDX(i, j, k, ni, nj)];
}

static int w_wall_face(int a, int b)
{
    int obstacle = (a != 0 && a != BQ_FLAG_WALL) || (b != 0 && b != BQ_FLAG_WALL);
    return !obstacle && (a == BQ_FLAG_WALL || b == BQ_FLAG_WALL);
}

/* :1157-1164 with velocity 0 */
void gpu_wall_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solidw,
                    int ni, int nj, int nk)
{
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                if (!w_wall_face(w_flag(solidw, i - 1, j, k, ni, nj, nk), w_flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = WIDX(i, j, k, ni + 1, nj);
                if (du) du[id] = 0.f - u[id];
                u[id] = 0.f;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                if (!w_wall_face(w_flag(solidw, i, j - 1, k, ni, nj, nk), w_flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = WIDX(i, j, k, ni, nj + 1);
                if (dv) dv[id] = 0.f - v[id];
                v[id] = 0.f;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                if (!w_wall_face(w_flag(solidw, i, j, k - 1, ni, nj, nk), w_flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = WIDX(i, j, k, ni, nj);
                if (dw) dw[id] = 0.f - w[id];
                w[id] = 0.f;
            }
}

/* one masked sweep on solidw over the local planes [k0, k1) that are interior planes of the array and of the global grid */
static void w_sweep(const float *in, const float *div, float *out, const unsigned char *solidw, int ni, int nj, int nk,
                    int k0, int k1, float alpha, float beta)
{
    float bs[7];
    bs[0] = beta;
    for (int s = 1; s < 6; s++) bs[s] = (float)(1.0 / (1.0 / (double)beta - (double)s));
    const int koff = w_koff(), nkg = w_nkg(nk);
    const size_t sj = (size_t)ni, sk = (size_t)ni * nj;
    if (k0 < 1) k0 = 1;
    if (k1 > nk - 1) k1 = nk - 1;
    for (int k = k0; k < k1; k++) {
        if (k + koff < 1 || k + koff > nkg - 2) continue;
        for (int j = 1; j < nj - 1; j++)
            for (int i = 1; i < ni - 1; i++) {
                size_t id = WIDX(i, j, k, ni, nj);
                if (solidw[id]) continue;
                int s = !!solidw[id - 1] + !!solidw[id + 1] + !!solidw[id - sj] + !!solidw[id + sj] + !!solidw[id - sk] + !!solidw[id + sk];
                float sum = in[id - 1] + in[id + 1] + in[id - sj] + in[id + sj] + in[id - sk] + in[id + sk] + alpha * div[id];
                out[id] = s == 6 ? 0.f : sum * bs[s];
            }
    }
}

static int w_args(const void *a, const void *b, const void *c, const void *d, const void *e, int walls, const char *op)
{
    if (a && b && c && d && e && a != c && walls > 0 && walls < 63) return 1;
    latch(FL_ERR_BAD_ARGUMENT, op);
    return 0;
}

void gpu_jacobi_sweep_masked_walls(const float *in, const float *div, float *out, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, float alpha, float beta)
{
    (void)rows; (void)walls;
    w_sweep(in, div, out, solidw, ni, nj, nk, 0, nk, alpha, beta);
}

int gpu_jacobi_sweeps_masked_walls(float *p, const float *div, float *p_temp, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, int sweeps,
                                   float alpha, float beta)
{
    (void)rows; (void)walls;
    float *in = p, *out = p_temp;
    if (j_open) { const char a = j_name(p); fprintf(j_log, "wsweeps %c->%c %d\n", a, j_name(p_temp), sweeps); }
    for (int s = 0; s < sweeps; s++) {
        w_sweep(in, div, out, solidw, ni, nj, nk, 0, nk, alpha, beta);
        float *t = in; in = out; out = t;
    }
    return in == p ? 0 : 1;
}

int gpu_jacobi_sweep_masked_walls_range(const float *in, const float *div, float *out, const unsigned char *solidw,
                                        const unsigned char *rows, int walls, int ni, int nj, int nk, int k_begin, int k_end,
                                        float alpha, float beta)
{
    if (!w_args(in, div, out, solidw, rows, walls, "gpu_jacobi_sweep_masked_walls_range")) return 0;
    if (j_open) { const char a = j_name(in); fprintf(j_log, "wrange %c->%c %d %d\n", a, j_name(out), k_begin, k_end); }
    w_sweep(in, div, out, solidw, ni, nj, nk, k_begin, k_end, alpha, beta);
    return 1;
}

/* three sweeps, output on two plane ranges: level 1 on the planes two beyond them, level 2 one beyond, level 3 on the ranges */
int gpu_jacobi_sweep_masked_walls_triple_ranges(const float *in, const float *div, float *out, const unsigned char *solidw,
                                                const unsigned char *rows, int walls, int ni, int nj, int nk,
                                                int k0a, int k1a, int k0b, int k1b, float alpha, float beta)
{
    if (!w_args(in, div, out, solidw, rows, walls, "gpu_jacobi_sweep_masked_walls_triple_ranges")) return 0;
    size_t n = (size_t)ni * nj * nk;
    if (!w_triples || g_opt[FL_OPT_JACOBI_FUSE] == 0 || g_opt[FL_OPT_JACOBI_FUSE] == 4)
        return j_ranges("wtriple", in, out, k0a, k1a, k0b, k1b, 0);
    float *l1 = (float *)malloc(n * sizeof(float)), *l2 = (float *)malloc(n * sizeof(float));
    if (!l1 || !l2) { free(l1); free(l2); return 0; }
    memcpy(l1, in, n * sizeof(float));
    memcpy(l2, in, n * sizeof(float));
    const int r[2][2] = { { k0a, k1a }, { k0b, k1b } };
    for (int lev = 0; lev < 3; lev++)
        for (int a = 0; a < 2; a++) {
            int k0 = r[a][0] < 0 ? 0 : r[a][0], k1 = r[a][1] > nk ? nk : r[a][1];
            if (k0 >= k1) continue;
            const int ext = 2 - lev;
            const float *src = lev == 0 ? in : lev == 1 ? l1 : l2;
            float *dst = lev == 0 ? l1 : lev == 1 ? l2 : out;
            w_sweep(src, div, dst, solidw, ni, nj, nk, k0 - ext, k1 + ext, alpha, beta);
        }
    free(l1); free(l2);
    return j_ranges("wtriple", in, out, k0a, k1a, k0b, k1b, 1);
}

/* the gradient on the faces whose two cells are fluid (:1288-1335), in the window that starts at cell 1 behind a closed low
 * side and at cell 2 behind an open one -- along z the window of the GLOBAL planes; w on the array's first plane has no
 * plane below it and stays (dw: 0).  du/dv/dw (when given): new - old in the window, 0 on the other fluid faces, solid faces
 * untouched */
void gpu_gradient_masked_walls(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                               const unsigned char *solidw, int walls, int ni, int nj, int nk, float halfrdx)
{
    const int i0 = (walls & BQ_WALL_XLO) ? 1 : 2, j0 = (walls & BQ_WALL_YLO) ? 1 : 2, k0 = (walls & BQ_WALL_ZLO) ? 1 : 2;
    const int koff = w_koff(), nkg = w_nkg(nk);
    j_end();
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                if (w_in(solidw, i - 1, j, k, ni, nj, nk) || w_in(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = WIDX(i, j, k, ni + 1, nj);
                if (i >= i0 && i < ni && j >= j0 && k + koff >= k0 && k + koff < nkg) {
                    float old = u[id];
                    u[id] = old - halfrdx * (p[WIDX(i, j, k, ni, nj)] - p[WIDX(i - 1, j, k, ni, nj)]);
                    if (du) du[id] = u[id] - old;
                } else if (du) du[id] = 0.f;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                if (w_in(solidw, i, j - 1, k, ni, nj, nk) || w_in(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = WIDX(i, j, k, ni, nj + 1);
                if (i >= i0 && j >= j0 && j < nj && k + koff >= k0 && k + koff < nkg) {
                    float old = v[id];
                    v[id] = old - halfrdx * (p[WIDX(i, j, k, ni, nj)] - p[WIDX(i, j - 1, k, ni, nj)]);
                    if (dv) dv[id] = v[id] - old;
                } else if (dv) dv[id] = 0.f;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                if (w_in(solidw, i, j, k - 1, ni, nj, nk) || w_in(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = WIDX(i, j, k, ni, nj);
                if (i >= i0 && j >= j0 && k >= 1 && k + koff >= k0 && k + koff < nkg && k < nk) {
                    float old = w[id];
                    w[id] = old - halfrdx * (p[WIDX(i, j, k, ni, nj)] - p[WIDX(i, j, k - 1, ni, nj)]);
                    if (dw) dw[id] = w[id] - old;
                } else if (dw) dw[id] = 0.f;
            }
}

/* the same window for the fp64 pressure of the PCG projection: one domain only */
void gpu_pcg_gradient_walls(float *u, float *v, float *w, const double *p, const unsigned char *solidw, int walls,
                            int ni, int nj, int nk, double halfrdx)
{
    const int i0 = (walls & BQ_WALL_XLO) ? 1 : 2, j0 = (walls & BQ_WALL_YLO) ? 1 : 2, k0 = (walls & BQ_WALL_ZLO) ? 1 : 2;
    for (int k = k0; k < nk; k++)
        for (int j = j0; j < nj; j++)
            for (int i = i0; i < ni; i++) {
                size_t c = WIDX(i, j, k, ni, nj);
                if (solidw[c]) continue;
                if (!solidw[WIDX(i - 1, j, k, ni, nj)]) u[WIDX(i, j, k, ni + 1, nj)] -= (float)(halfrdx * (p[c] - p[WIDX(i - 1, j, k, ni, nj)]));
                if (!solidw[WIDX(i, j - 1, k, ni, nj)]) v[WIDX(i, j, k, ni, nj + 1)] -= (float)(halfrdx * (p[c] - p[WIDX(i, j - 1, k, ni, nj)]));
                if (!solidw[WIDX(i, j, k - 1, ni, nj)]) w[WIDX(i, j, k, ni, nj)] -= (float)(halfrdx * (p[c] - p[WIDX(i, j, k - 1, ni, nj)]));
            }
}
