/*
 * walls_abi.c -- TEST-ONLY C restatement of the wall operators of include/bimocq_gpu.h.
 *
 * Linked on top of the obstacle, level-set and PCG restatements into tests/_build/libbimocq_host_cpu_walls.so
 * (tests/build_cpu_walls.py): the stand-in on which the host solver's walled projection runs without a GPU, and against
 * which the GPU tests compare the HIP kernels bit for bit.  Written loop by loop from the contract, not from the kernels:
 * the sweeps are gpu_jacobi_sweep_masked's loop on solidw and never look at `rows` or `walls`.  Reference
 * (src/bimocq3D/BimocqSolver.cpp): the flag-2 border of updateBoundary :938-948, its faces :1157-1164, the masked
 * projection :1184-1356.
 */
#include <stddef.h>

#include "../../include/bimocq_gpu.h"

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

void gpu_jacobi_sweep_masked(const float *in, const float *div, float *out, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, float alpha, float beta);   /* obstacle_abi.c */

/* :938-948: the border layer of every closed side is solid unless an obstacle already owns the cell */
void gpu_wall_flags(unsigned char *solidw, const unsigned char *solid, int walls, int ni, int nj, int nk)
{
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int border = ((walls & BQ_WALL_XLO) && i == 0) || ((walls & BQ_WALL_XHI) && i == ni - 1) ||
                             ((walls & BQ_WALL_YLO) && j == 0) || ((walls & BQ_WALL_YHI) && j == nj - 1) ||
                             ((walls & BQ_WALL_ZLO) && k == 0) || ((walls & BQ_WALL_ZHI) && k == nk - 1);
                unsigned char f = solid ? solid[IDX(i, j, k, ni, nj)] : 0;
                solidw[IDX(i, j, k, ni, nj)] = f ? f : (unsigned char)(border ? BQ_FLAG_WALL : 0);
            }
}

static int flag(const unsigned char *s, int i, int j, int k, int ni, int nj, int nk)
{
    if (i < 0 || j < 0 || k < 0 || i >= ni || j >= nj || k >= nk) return 0;
    return s[IDX(i, j, k, ni, nj)];
}

/* a face between a wall cell and a wall or fluid (or outside) cell */
static int wall_face(int a, int b)
{
    int obstacle = (a != 0 && a != BQ_FLAG_WALL) || (b != 0 && b != BQ_FLAG_WALL);
    return !obstacle && (a == BQ_FLAG_WALL || b == BQ_FLAG_WALL);
}

/* :1157-1164 with velocity 0: all six faces of a wall cell, but for those an obstacle cell shares */
void gpu_wall_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solidw,
                    int ni, int nj, int nk)
{
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                if (!wall_face(flag(solidw, i - 1, j, k, ni, nj, nk), flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = IDX(i, j, k, ni + 1, nj);
                if (du) du[id] = 0.f - u[id];
                u[id] = 0.f;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                if (!wall_face(flag(solidw, i, j - 1, k, ni, nj, nk), flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = IDX(i, j, k, ni, nj + 1);
                if (dv) dv[id] = 0.f - v[id];
                v[id] = 0.f;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                if (!wall_face(flag(solidw, i, j, k - 1, ni, nj, nk), flag(solidw, i, j, k, ni, nj, nk))) continue;
                size_t id = IDX(i, j, k, ni, nj);
                if (dw) dw[id] = 0.f - w[id];
                w[id] = 0.f;
            }
}

void gpu_jacobi_sweep_masked_walls(const float *in, const float *div, float *out, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, float alpha, float beta)
{
    (void)walls;
    gpu_jacobi_sweep_masked(in, div, out, solidw, rows, ni, nj, nk, alpha, beta);
}

int gpu_jacobi_sweeps_masked_walls(float *p, const float *div, float *p_temp, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, int sweeps,
                                   float alpha, float beta)
{
    (void)walls;
    float *in = p, *out = p_temp;
    for (int s = 0; s < sweeps; s++) {
        gpu_jacobi_sweep_masked(in, div, out, solidw, rows, ni, nj, nk, alpha, beta);
        float *t = in; in = out; out = t;
    }
    return in == p ? 0 : 1;
}

/* the gradient on the faces whose two cells are fluid (:1288-1335), in the window that starts at cell 1 behind a closed
 * low side and at cell 2 behind an open one; du/dv/dw (when given): new - old there, 0 on the other fluid faces, solid
 * faces (those of wall cells included) untouched */
void gpu_gradient_masked_walls(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                               const unsigned char *solidw, int walls, int ni, int nj, int nk, float halfrdx)
{
    const int i0 = (walls & BQ_WALL_XLO) ? 1 : 2, j0 = (walls & BQ_WALL_YLO) ? 1 : 2, k0 = (walls & BQ_WALL_ZLO) ? 1 : 2;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                if (flag(solidw, i - 1, j, k, ni, nj, nk) || flag(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni + 1, nj);
                if (i >= i0 && i < ni && j >= j0 && k >= k0) {
                    float old = u[id];
                    u[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i - 1, j, k, ni, nj)]);
                    if (du) du[id] = u[id] - old;
                } else if (du) du[id] = 0.f;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                if (flag(solidw, i, j - 1, k, ni, nj, nk) || flag(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni, nj + 1);
                if (i >= i0 && j >= j0 && j < nj && k >= k0) {
                    float old = v[id];
                    v[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i, j - 1, k, ni, nj)]);
                    if (dv) dv[id] = v[id] - old;
                } else if (dv) dv[id] = 0.f;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                if (flag(solidw, i, j, k - 1, ni, nj, nk) || flag(solidw, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni, nj);
                if (i >= i0 && j >= j0 && k >= k0 && k < nk) {
                    float old = w[id];
                    w[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i, j, k - 1, ni, nj)]);
                    if (dw) dw[id] = w[id] - old;
                } else if (dw) dw[id] = 0.f;
            }
}

/* the same window for the fp64 pressure of the PCG projection */
void gpu_pcg_gradient_walls(float *u, float *v, float *w, const double *p, const unsigned char *solidw, int walls,
                            int ni, int nj, int nk, double halfrdx)
{
    const int i0 = (walls & BQ_WALL_XLO) ? 1 : 2, j0 = (walls & BQ_WALL_YLO) ? 1 : 2, k0 = (walls & BQ_WALL_ZLO) ? 1 : 2;
    for (int k = k0; k < nk; k++)
        for (int j = j0; j < nj; j++)
            for (int i = i0; i < ni; i++) {
                size_t c = IDX(i, j, k, ni, nj);
                if (solidw[c]) continue;
                if (!solidw[IDX(i - 1, j, k, ni, nj)]) u[IDX(i, j, k, ni + 1, nj)] -= (float)(halfrdx * (p[c] - p[IDX(i - 1, j, k, ni, nj)]));
                if (!solidw[IDX(i, j - 1, k, ni, nj)]) v[IDX(i, j, k, ni, nj + 1)] -= (float)(halfrdx * (p[c] - p[IDX(i, j - 1, k, ni, nj)]));
                if (!solidw[IDX(i, j, k - 1, ni, nj)]) w[c] -= (float)(halfrdx * (p[c] - p[IDX(i, j, k - 1, ni, nj)]));
            }
}
