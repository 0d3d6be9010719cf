/*
 * source_abi.c -- TEST-ONLY C restatement of gpu_emit_sources of include/bimocq_gpu.h.
 *
 * Linked, together with oracle_abi.c, obstacle_abi.c, levelset_abi.c and the oracle, into
 * tests/_build/libbimocq_host_cpu_sources.so (tests/build_cpu_sources.py): the fourth CPU stand-in, on which the host
 * solver's source path runs without a GPU, and against which the GPU tests compare the HIP kernel bit for bit.  Written
 * from the contract, not from the kernel, and self-contained: the inside tests and the sampler are restated here.  Every
 * source gets a pass of its own over EVERY node of the four buffers (no boxes).  Built with -ffp-contract=off.
 * Reference (src/bimocq3D/BimocqSolver.cpp): emitSmoke :696-813.  Single domain only (no z-slab context).
 */
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "../../include/bimocq_gpu.h"

void fl_report_error(int code, const char *text);

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

/* p + (q - p) t: difference and sum in float, product in double */
static float lerp_src(float p, float q, double t)
{
    float d = q - p;
    return p + (float)((double)d * t);
}

static float node(const bq_levelset *l, int i, int j, int k)
{
    if (i < 0 || j < 0 || k < 0 || i >= l->nx || j >= l->ny || k >= l->nz) return l->background;
    return l->phi[IDX(i, j, k, l->nx, l->ny)];
}

/* the level set's value at (x, y, z), its index origin at (cx, cy, cz); `background` when every corner lies outside */
static float sample(const bq_levelset *l, float cx, float cy, float cz, float x, float y, float z)
{
    double g[3], t[3];
    int a[3];
    const double p[3] = { (double)x - (double)cx, (double)y - (double)cy, (double)z - (double)cz };
    const int lo[3] = { l->i0, l->j0, l->k0 }, n[3] = { l->nx, l->ny, l->nz };
    for (int d = 0; d < 3; d++) {
        g[d] = p[d] / (double)l->voxel;
        if (g[d] < (double)lo[d] - 1.0 || g[d] >= (double)lo[d] + (double)n[d]) return l->background;
    }
    for (int d = 0; d < 3; d++) {
        double f = floor(g[d]);
        t[d] = g[d] - f;
        a[d] = (int)f - lo[d];
    }
    float zl[2][2];
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            zl[di][dj] = lerp_src(node(l, a[0] + di, a[1] + dj, a[2]), node(l, a[0] + di, a[1] + dj, a[2] + 1), t[2]);
    float y0 = lerp_src(zl[0][0], zl[0][1], t[1]);
    float y1 = lerp_src(zl[1][0], zl[1][1], t[1]);
    return lerp_src(y0, y1, t[0]);
}

/* 1 when (x, y, z) belongs to source s: the solid test of the obstacle classification, no band */
static int inside(const bq_source *s, const bq_levelset *l, float x, float y, float z)
{
    const bq_boundary *b = &s->shape;
    if (b->shape == BQ_SHAPE_LEVELSET) return sample(l, b->cx, b->cy, b->cz, x, y, z) <= 0.f;   /* (background > 0 outside) */
    float dx = x - b->cx, dy = y - b->cy, dz = z - b->cz;
    if (b->shape == BQ_SHAPE_SPHERE) {
        float d2 = dx * dx + dy * dy + dz * dz;
        return d2 <= b->rx * b->rx;
    }
    float ax = fabsf(dx) - b->rx, ay = fabsf(dy) - b->ry, az = fabsf(dz) - b->rz;
    return ax <= 0.f && ay <= 0.f && az <= 0.f;
}

static float pos(int i, int staggered, float h) { return ((float)i - (staggered ? 0.5f : 0.f)) * h; }

static int descriptor_ok(const bq_levelset *l)
{
    return l && l->phi && l->nx >= 2 && l->ny >= 2 && l->nz >= 2 &&
           (double)l->nx * (double)l->ny * (double)l->nz < 2147483648.0 &&
           (long long)l->i0 - 1 >= INT_MIN && (long long)l->j0 - 1 >= INT_MIN && (long long)l->k0 - 1 >= INT_MIN &&
           (long long)l->i0 + l->nx <= INT_MAX && (long long)l->j0 + l->ny <= INT_MAX && (long long)l->k0 + l->nz <= INT_MAX &&
           l->voxel > 0.f && l->background > 0.f && isfinite(l->voxel) && isfinite(l->background);
}

/* one buffer of dims (bi, bj, bk) staggered along axis `axis` (-1: cells), window 1 < index < n - 2 on its own dims */
static void pass(float *f, float *g, const bq_source *s, const bq_levelset *l, int axis, float h, int bi, int bj, int bk)
{
    const bq_boundary *b = &s->shape;
    for (int k = 2; k < bk - 2; k++)
        for (int j = 2; j < bj - 2; j++)
            for (int i = 2; i < bi - 2; i++) {
                float x = pos(i, axis == 0, h), y = pos(j, axis == 1, h), z = pos(k, axis == 2, h);
                if (!inside(s, l, x, y, z)) continue;
                float dx = x - b->cx, dy = y - b->cy, dz = z - b->cz;
                size_t id = IDX(i, j, k, bi, bj);
                if (axis < 0) { f[id] = s->density; g[id] = s->temperature; }
                else if (axis == 0) f[id] = s->ex + (s->oy * dz - s->oz * dy);
                else if (axis == 1) f[id] = s->ey + (s->oz * dx - s->ox * dz);
                else f[id] = s->ez + (s->ox * dy - s->oy * dx);
            }
}

void gpu_emit_sources(float *u, float *v, float *w, float *rho, float *T, const bq_source *src, const bq_levelset *ls,
                      int n, float h, int ni, int nj, int nk)
{
    if (n < 0 || n > BQ_MAX_SOURCES || (n > 0 && !src) || !u || !v || !w || !rho || !T) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_emit_sources: bad argument");
        return;
    }
    for (int o = 0; o < n; o++) {
        int sh = src[o].shape.shape;
        if ((sh != BQ_SHAPE_SPHERE && sh != BQ_SHAPE_BOX && sh != BQ_SHAPE_LEVELSET) || (src[o].flags & ~BQ_SOURCE_VELOCITY) ||
            (sh == BQ_SHAPE_LEVELSET && !descriptor_ok(ls ? &ls[o] : NULL))) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_emit_sources: unknown shape or flag, or a bad level-set descriptor");
            return;
        }
    }
    for (int o = 0; o < n; o++) {
        const bq_source *s = &src[o];
        const bq_levelset *l = s->shape.shape == BQ_SHAPE_LEVELSET ? &ls[o] : NULL;
        pass(rho, T, s, l, -1, h, ni, nj, nk);
        if (!(s->flags & BQ_SOURCE_VELOCITY)) continue;
        pass(u, NULL, s, l, 0, h, ni + 1, nj, nk);
        pass(v, NULL, s, l, 1, h, ni, nj + 1, nk);
        pass(w, NULL, s, l, 2, h, ni, nj, nk + 1);
    }
}
