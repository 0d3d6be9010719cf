/*
 * levelset_abi.c -- TEST-ONLY C restatement of the level-set obstacle operators of include/bimocq_gpu.h
 * (gpu_obstacle_flags_ls, gpu_semilag_band_ls, gpu_obstacle_blend_ls; DESIGN.md section 14, "Level sets").
 *
 * Linked, together with oracle_abi.c, obstacle_abi.c and the oracle, into tests/_build/libbimocq_host_cpu_levelsets.so
 * (tests/build_cpu_host_levelsets.py): the third CPU stand-in, on which the host solver's level-set path runs without a
 * GPU, and against which the GPU tests compare the HIP kernels bit for bit.  Written from the contract, not from the
 * kernels, and self-contained: the analytic classification is restated here too.  Built with -ffp-contract=off.
 * Reference (src/bimocq3D/BimocqSolver.cpp): updateBoundary :936-1064, blendBoundary :879-912 -- a trilinear BoxSampler
 * look-up of the boundary's FloatGrid at the node position minus b_pos.
 */
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

void fl_report_error(int code, const char *text);

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

/* p + (q - p) t: difference and sum in float, product in double */
static float lerp_ls(float p, float q, double t)
{
    float d = q - p;
    return p + (float)((double)d * t);
}

/* phi at stored node (i, j, k) (0-based in the array), background outside */
static float node(const bq_levelset *l, int i, int j, int k)
{
    if (i < 0 || j < 0 || k < 0 || i >= l->nx || j >= l->ny || k >= l->nz) return l->background;
    return l->phi[IDX(i, j, k, l->nx, l->ny)];
}

/* the level set's value at world point (x, y, z) with its index origin at (cx, cy, cz) */
static float sample(const bq_levelset *l, float cx, float cy, float cz, float x, float y, float z)
{
    double g[3], t[3];
    int a[3];
    const double p[3] = { (double)x - (double)cx, (double)y - (double)cy, (double)z - (double)cz };
    const int lo[3] = { l->i0, l->j0, l->k0 }, n[3] = { l->nx, l->ny, l->nz };
    for (int d = 0; d < 3; d++) {
        g[d] = p[d] / (double)l->voxel;
        if (g[d] < (double)lo[d] - 1.0 || g[d] >= (double)lo[d] + (double)n[d]) return l->background;   /* every corner outside */
    }
    for (int d = 0; d < 3; d++) {
        double f = floor(g[d]);
        t[d] = g[d] - f;
        a[d] = (int)f - lo[d];
    }
    /* z first, then y, then x */
    float zl[2][2];
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            zl[di][dj] = lerp_ls(node(l, a[0] + di, a[1] + dj, a[2]), node(l, a[0] + di, a[1] + dj, a[2] + 1), t[2]);
    float y0 = lerp_ls(zl[0][0], zl[0][1], t[1]);
    float y1 = lerp_ls(zl[1][0], zl[1][1], t[1]);
    return lerp_ls(y0, y1, t[0]);
}

/* o + 1: the last entry covering the point; -1: in some entry's band and covered by none; 0: elsewhere */
static int classify(const bq_boundary *b, const bq_levelset *ls, int n, float h, float x, float y, float z)
{
    int solid = 0, band = 0;
    const float h3 = 3.0f * h;
    for (int o = 0; o < n; o++) {
        if (b[o].shape == BQ_SHAPE_LEVELSET) {
            float s = sample(&ls[o], b[o].cx, b[o].cy, b[o].cz, x, y, z);
            if (s <= 0.f) solid = o + 1;
            else if (s < ls[o].background) band = 1;
            continue;
        }
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

static float pos(int i, int staggered, float h) { return ((float)i - (staggered ? 0.5f : 0.f)) * h; }

/* the descriptor checks every _ls operator makes; 0 (and FL_ERR_BAD_ARGUMENT latched) when one fails */
static int descriptors_ok(const bq_boundary *b, const bq_levelset *ls, int n, const char *op)
{
    if (n < 0 || n > BQ_MAX_BOUNDARIES || (n > 0 && !b)) { fl_report_error(FL_ERR_BAD_ARGUMENT, op); return 0; }
    for (int o = 0; o < n; o++) {
        if (b[o].shape != BQ_SHAPE_LEVELSET) continue;
        const bq_levelset *l = ls ? &ls[o] : NULL;
        if (!l || !l->phi || l->nx < 2 || l->ny < 2 || l->nz < 2 ||
            (double)l->nx * (double)l->ny * (double)l->nz >= 2147483648.0 ||
            (long long)l->i0 - 1 < INT_MIN || (long long)l->j0 - 1 < INT_MIN || (long long)l->k0 - 1 < INT_MIN ||
            (long long)l->i0 + l->nx > INT_MAX || (long long)l->j0 + l->ny > INT_MAX || (long long)l->k0 + l->nz > INT_MAX ||
            !(l->voxel > 0.f) || !(l->background > 0.f) || !isfinite(l->voxel) || !isfinite(l->background)) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, op);
            return 0;
        }
    }
    return 1;
}

void gpu_obstacle_flags_ls(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                           float h, int ni, int nj, int nk)
{
    if (!descriptors_ok(b, ls, n, "gpu_obstacle_flags_ls")) return;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int c = classify(b, ls, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h));
                solid[IDX(i, j, k, ni, nj)] = (unsigned char)(c > 0 ? c : 0);
            }
    /* rows summary: (j, k) is marked when a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1 */
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++) {
            int any = 0;
            for (int kk = k - 1; kk <= k + 1; kk++)
                for (int jj = j - 1; jj <= j + 1; jj++) {
                    if (jj < 0 || kk < 0 || jj >= nj || kk >= nk) continue;
                    for (int i = 0; i < ni; i++) any |= solid[IDX(i, jj, kk, ni, nj)];
                }
            rows[(size_t)j + (size_t)nj * k] = (unsigned char)(any != 0);
        }
}

void gpu_semilag_band_ls(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                         float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n,
                         const bq_levelset *ls)
{
    if (!descriptors_ok(b, ls, n, "gpu_semilag_band_ls")) return;
    if (n == 0) return;
    const int bi = ni + dim_x, bj = nj + dim_y, bk = nk + dim_z;
    const size_t cnt = (size_t)bi * bj * bk;
    float *tmp = (float *)calloc(cnt, sizeof(float));
    if (!tmp) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_semilag_band_ls: out of memory"); return; }
    orc_semilag(tmp, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt);
    for (int k = 0; k < bk; k++)
        for (int j = 0; j < bj; j++)
            for (int i = 0; i < bi; i++)
                if (classify(b, ls, n, h, pos(i, dim_x, h), pos(j, dim_y, h), pos(k, dim_z, h)) == -1)
                    field[IDX(i, j, k, bi, bj)] = tmp[IDX(i, j, k, bi, bj)];
    free(tmp);
}

void gpu_obstacle_blend_ls(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                           const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                           const bq_boundary *b, int n, const bq_levelset *ls, float h, int ni, int nj, int nk)
{
    if (!descriptors_ok(b, ls, n, "gpu_obstacle_blend_ls")) return;
    if (us) {
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i <= ni; i++)
                    if (classify(b, ls, n, h, pos(i, 1, h), pos(j, 0, h), pos(k, 0, h)) == -1) u[IDX(i, j, k, ni + 1, nj)] = us[IDX(i, j, k, ni + 1, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j <= nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, n, h, pos(i, 0, h), pos(j, 1, h), pos(k, 0, h)) == -1) v[IDX(i, j, k, ni, nj + 1)] = vs[IDX(i, j, k, ni, nj + 1)];
        for (int k = 0; k <= nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 1, h)) == -1) w[IDX(i, j, k, ni, nj)] = ws[IDX(i, j, k, ni, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h)) == -1) {
                        rho[IDX(i, j, k, ni, nj)] = rhos[IDX(i, j, k, ni, nj)];
                        T[IDX(i, j, k, ni, nj)] = Ts[IDX(i, j, k, ni, nj)];
                    }
    }
    for (size_t c = 0; c < (size_t)ni * nj * nk; c++)
        if (solid[c]) rho[c] = 0.f;
}
