/*
 * obstacle_abi.c -- TEST-ONLY C restatement of the obstacle operators of include/bimocq_gpu.h.
 *
 * Linked, together with oracle_abi.c and the oracle, into tests/_build/libbimocq_host_cpu_obstacles.so
 * (tests/build_cpu_host_obstacles.py): the second CPU stand-in, on which the host solver's obstacle path runs without a
 * GPU, and against which the GPU tests compare the HIP kernels bit for bit.  Written loop by loop from the contract,
 * not from the kernels.  Reference (src/bimocq3D/BimocqSolver.cpp): updateBoundary :936-1064 (flags, solid face
 * velocities), the masked projection :1120-1413, blendBoundary :879-912, clearBoundary :914-934.
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

void fl_report_error(int code, const char *text);

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

/* o + 1: the last obstacle covering the point; -1: in some obstacle's 3h band and inside none; 0: elsewhere */
static int classify(const bq_boundary *b, int n, float h, float x, float y, float z)
{
    int solid = 0, band = 0;
    const float h3 = 3.0f * h;
    for (int o = 0; o < n; o++) {
        float dx = x - b[o].cx, dy = y - b[o].cy, dz = z - b[o].cz;
        if (b[o].shape == BQ_SHAPE_SPHERE) {
            float d2 = dx * dx + dy * dy + dz * dz;
            float R = b[o].rx + h3;
            if (d2 <= b[o].rx * b[o].rx) solid = o + 1;
            else if (d2 < R * R) band = 1;
        } else {
            float ax = fabsf(dx) - b[o].rx, ay = fabsf(dy) - b[o].ry, az = fabsf(dz) - b[o].rz;
            if (ax <= 0.f && ay <= 0.f && az <= 0.f) { solid = o + 1; continue; }
            float qx = ax > 0.f ? ax : 0.f, qy = ay > 0.f ? ay : 0.f, qz = az > 0.f ? az : 0.f;
            float d2 = qx * qx + qy * qy + qz * qz;
            if (d2 > 0.f && d2 < h3 * h3) band = 1;
        }
    }
    return solid ? solid : (band ? -1 : 0);
}

/* (i - o) h with the buffer origins o = 0 (cells) and 1/2 (the staggered axis), BimocqSolver.cpp:32-46, :891-902 */
static float pos(int i, int staggered, float h) { return ((float)i - (staggered ? 0.5f : 0.f)) * h; }

static int cell(const unsigned char *solid, int i, int j, int k, int ni, int nj, int nk)
{
    if (i < 0 || j < 0 || k < 0 || i >= ni || j >= nj || k >= nk) return 0;
    return solid[IDX(i, j, k, ni, nj)];
}

void gpu_obstacle_flags(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, float h, int ni, int nj, int nk)
{
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int c = classify(b, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h));
                solid[IDX(i, j, k, ni, nj)] = (unsigned char)(c > 0 ? c : 0);
            }
    /* rows summary: (j, k) is marked when a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1 */
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++) {
            int any = 0;
            for (int kk = k - 1; kk <= k + 1; kk++)
                for (int jj = j - 1; jj <= j + 1; jj++)
                    for (int i = 0; i < ni; i++) any |= cell(solid, i, jj, kk, ni, nj, nk);
            rows[(size_t)j + (size_t)nj * k] = (unsigned char)(any != 0);
        }
}

/* :1149-1165: the faces of a solid cell take the obstacle's velocity (later obstacle wins on a shared face) */
void gpu_obstacle_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                        const bq_boundary *b, int n, int ni, int nj, int nk)
{
    (void)n;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                int a = cell(solid, i - 1, j, k, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni + 1, nj);
                if (du) du[id] = b[o - 1].vx - u[id];
                u[id] = b[o - 1].vx;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                int a = cell(solid, i, j - 1, k, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni, nj + 1);
                if (dv) dv[id] = b[o - 1].vy - v[id];
                v[id] = b[o - 1].vy;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int a = cell(solid, i, j, k - 1, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni, nj);
                if (dw) dw[id] = b[o - 1].vz - w[id];
                w[id] = b[o - 1].vz;
            }
}

/* the Jacobi sweep of GPU_kernel.cu:1819-1837 with the solid neighbours dropped from the stencil (Neumann) */
void gpu_jacobi_sweep_masked(const float *in, const float *div, float *out, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, float alpha, float beta)
{
    (void)rows;
    float bs[7];
    bs[0] = beta;
    for (int s = 1; s < 6; s++) bs[s] = (float)(1.0 / (1.0 / (double)beta - (double)s));
    const size_t sj = (size_t)ni, sk = (size_t)ni * nj;
    for (int k = 1; k < nk - 1; k++)
        for (int j = 1; j < nj - 1; j++)
            for (int i = 1; i < ni - 1; i++) {
                size_t id = IDX(i, j, k, ni, nj);
                if (solid[id]) continue;
                int s = !!solid[id - 1] + !!solid[id + 1] + !!solid[id - sj] + !!solid[id + sj] + !!solid[id - sk] + !!solid[id + sk];
                float sum = in[id - 1] + in[id + 1] + in[id - sj] + in[id + sj] + in[id - sk] + in[id + sk] + alpha * div[id];
                out[id] = s == 6 ? 0.f : sum * bs[s];
            }
}

int gpu_jacobi_sweeps_masked(float *p, const float *div, float *p_temp, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, int sweeps, float alpha, float beta)
{
    float *in = p, *out = p_temp;
    for (int s = 0; s < sweeps; s++) {
        gpu_jacobi_sweep_masked(in, div, out, solid, rows, ni, nj, nk, alpha, beta);
        float *t = in; in = out; out = t;
    }
    return in == p ? 0 : 1;
}

/* GPU_kernel.cu:1024-1041 on the faces whose two cells are fluid; du/dv/dw (when given): new - old there, 0 on the other
 * fluid faces, solid faces untouched */
void gpu_gradient_masked(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                         const unsigned char *solid, int ni, int nj, int nk, float halfrdx)
{
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                if (cell(solid, i - 1, j, k, ni, nj, nk) || cell(solid, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni + 1, nj);
                if (i >= 2 && i < ni && j >= 2 && k >= 2) {
                    float old = u[id];
                    u[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i - 1, j, k, ni, nj)]);
                    if (du) du[id] = u[id] - old;
                } else if (du) du[id] = 0.f;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                if (cell(solid, i, j - 1, k, ni, nj, nk) || cell(solid, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni, nj + 1);
                if (i >= 2 && j >= 2 && j < nj && k >= 2) {
                    float old = v[id];
                    v[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i, j - 1, k, ni, nj)]);
                    if (dv) dv[id] = v[id] - old;
                } else if (dv) dv[id] = 0.f;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                if (cell(solid, i, j, k - 1, ni, nj, nk) || cell(solid, i, j, k, ni, nj, nk)) continue;
                size_t id = IDX(i, j, k, ni, nj);
                if (i >= 2 && j >= 2 && k >= 2 && k < nk) {
                    float old = w[id];
                    w[id] = old - halfrdx * (p[IDX(i, j, k, ni, nj)] - p[IDX(i, j, k - 1, ni, nj)]);
                    if (dw) dw[id] = w[id] - old;
                } else if (dw) dw[id] = 0.f;
            }
}

/* the oracle's semilag over the whole buffer into a scratch copy, kept at the band nodes only */
void gpu_semilag_band(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                      float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n)
{
    if (n == 0) return;
    const int bi = ni + dim_x, bj = nj + dim_y, bk = nk + dim_z;
    const size_t cnt = (size_t)bi * bj * bk;
    float *tmp = (float *)calloc(cnt, sizeof(float));
    if (!tmp) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_semilag_band: out of memory"); return; }
    orc_semilag(tmp, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt);
    for (int k = 0; k < bk; k++)
        for (int j = 0; j < bj; j++)
            for (int i = 0; i < bi; i++)
                if (classify(b, n, h, pos(i, dim_x, h), pos(j, dim_y, h), pos(k, dim_z, h)) == -1)
                    field[IDX(i, j, k, bi, bj)] = tmp[IDX(i, j, k, bi, bj)];
    free(tmp);
}

/* blendBoundary (:879-912) at band nodes, then clearBoundary (:914-934) of rho */
void gpu_obstacle_blend(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                        const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                        const bq_boundary *b, int n, float h, int ni, int nj, int nk)
{
    if (us) {
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i <= ni; i++)
                    if (classify(b, n, h, pos(i, 1, h), pos(j, 0, h), pos(k, 0, h)) == -1) u[IDX(i, j, k, ni + 1, nj)] = us[IDX(i, j, k, ni + 1, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j <= nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, n, h, pos(i, 0, h), pos(j, 1, h), pos(k, 0, h)) == -1) v[IDX(i, j, k, ni, nj + 1)] = vs[IDX(i, j, k, ni, nj + 1)];
        for (int k = 0; k <= nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 1, h)) == -1) w[IDX(i, j, k, ni, nj)] = ws[IDX(i, j, k, ni, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h)) == -1) {
                        rho[IDX(i, j, k, ni, nj)] = rhos[IDX(i, j, k, ni, nj)];
                        T[IDX(i, j, k, ni, nj)] = Ts[IDX(i, j, k, ni, nj)];
                    }
    }
    for (size_t c = 0; c < (size_t)ni * nj * nk; c++)
        if (solid[c]) rho[c] = 0.f;
}
