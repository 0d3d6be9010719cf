/*
 * pose_abi.c -- TEST-ONLY C restatement of the pose operators of include/bimocq_gpu.h (gpu_obstacle_flags_pose,
 * gpu_semilag_band_pose, gpu_obstacle_blend_pose, gpu_obstacle_faces_pose).
 *
 * Linked on top of the obstacle, level-set, PCG and walls restatements into tests/_build/libbimocq_host_cpu_pose.so
 * (tests/build_cpu_pose.py): the stand-in on which the host solver's rotating obstacles run without a GPU, and against
 * which the GPU tests compare the HIP kernels bit for bit.  Written from the contract, not from the kernels, and
 * self-contained: the whole classification is restated here.  Built with -ffp-contract=off.  The reference has no
 * rotation (Boundary::update only translates, BimocqSolver.h:71-79): the contract is this project's own.
 */
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

void fl_report_error(int code, const char *text);

#define IDX(i, j, k, nx, ny) ((size_t)(i) + (size_t)(nx) * ((size_t)(j) + (size_t)(ny) * (size_t)(k)))

typedef struct { int oriented; float R[3][3]; } rot_t;

/* R (body -> world) from the four floats promoted to double, scale-free, each entry rounded to float */
static void rotation(const bq_boundary *b, const bq_pose *p, rot_t *r)
{
    r->oriented = b->shape != BQ_SHAPE_SPHERE && (p->qx != 0.f || p->qy != 0.f || p->qz != 0.f);
    if (!r->oriented) return;
    const double w = p->qw, x = p->qx, y = p->qy, z = p->qz;
    const double s = w * w + x * x + y * y + z * z;
    r->R[0][0] = (float)(1.0 - 2.0 * (y * y + z * z) / s);
    r->R[0][1] = (float)(2.0 * (x * y - w * z) / s);
    r->R[0][2] = (float)(2.0 * (x * z + w * y) / s);
    r->R[1][0] = (float)(2.0 * (x * y + w * z) / s);
    r->R[1][1] = (float)(1.0 - 2.0 * (x * x + z * z) / s);
    r->R[1][2] = (float)(2.0 * (y * z - w * x) / s);
    r->R[2][0] = (float)(2.0 * (x * z - w * y) / s);
    r->R[2][1] = (float)(2.0 * (y * z + w * x) / s);
    r->R[2][2] = (float)(1.0 - 2.0 * (x * x + y * y) / s);
}

/* p + (q - p) t: difference and sum in float, product in double */
static float lerp_ls(float p, float q, double t)
{
    float d = q - p;
    return p + (float)((double)d * t);
}

static float node(const bq_levelset *l, int i, int j, int k)
{
    if (i < 0 || j < 0 || k < 0 || i >= l->nx || j >= l->ny || k >= l->nz) return l->background;
    return l->phi[IDX(i, j, k, l->nx, l->ny)];
}

/* the level set's value at index-space position g */
static float sample_index(const bq_levelset *l, const double g[3])
{
    double t[3];
    int a[3];
    const int lo[3] = { l->i0, l->j0, l->k0 }, n[3] = { l->nx, l->ny, l->nz };
    for (int d = 0; d < 3; d++)
        if (g[d] < (double)lo[d] - 1.0 || g[d] >= (double)lo[d] + (double)n[d]) return l->background;
    for (int d = 0; d < 3; d++) {
        double f = floor(g[d]);
        t[d] = g[d] - f;
        a[d] = (int)f - lo[d];
    }
    float zl[2][2];
    for (int di = 0; di < 2; di++)
        for (int dj = 0; dj < 2; dj++)
            zl[di][dj] = lerp_ls(node(l, a[0] + di, a[1] + dj, a[2]), node(l, a[0] + di, a[1] + dj, a[2] + 1), t[2]);
    float y0 = lerp_ls(zl[0][0], zl[0][1], t[1]);
    float y1 = lerp_ls(zl[1][0], zl[1][1], t[1]);
    return lerp_ls(y0, y1, t[0]);
}

/* box test on the per-axis offsets (world for an unoriented entry, body for an oriented one): 1 solid, -1 band, 0 */
static int box(const bq_boundary *b, float h3, float dx, float dy, float dz)
{
    float ax = fabsf(dx) - b->rx, ay = fabsf(dy) - b->ry, az = fabsf(dz) - b->rz;
    if (ax <= 0.f && ay <= 0.f && az <= 0.f) return 1;
    float qx = ax > 0.f ? ax : 0.f, qy = ay > 0.f ? ay : 0.f, qz = az > 0.f ? az : 0.f;
    float d2 = qx * qx + qy * qy + qz * qz;
    return (d2 > 0.f && d2 < h3 * h3) ? -1 : 0;
}

/* o + 1: the last entry covering the point; -1: in some entry's band and covered by none; 0: elsewhere */
static int classify(const bq_boundary *b, const bq_levelset *ls, const rot_t *rot, int n, float h, float x, float y, float z)
{
    int solid = 0, band = 0;
    const float h3 = 3.0f * h;
    for (int o = 0; o < n; o++) {
        float dx = x - b[o].cx, dy = y - b[o].cy, dz = z - b[o].cz;
        int c;
        if (rot[o].oriented) {                         /* body coordinates R^T d */
            const float (*R)[3] = rot[o].R;
            float bx = R[0][0] * dx + R[1][0] * dy + R[2][0] * dz;
            float by = R[0][1] * dx + R[1][1] * dy + R[2][1] * dz;
            float bz = R[0][2] * dx + R[1][2] * dy + R[2][2] * dz;
            if (b[o].shape == BQ_SHAPE_LEVELSET) {
                const double g[3] = { (double)bx / (double)ls[o].voxel, (double)by / (double)ls[o].voxel, (double)bz / (double)ls[o].voxel };
                float s = sample_index(&ls[o], g);
                c = s <= 0.f ? 1 : (s < ls[o].background ? -1 : 0);
            } else {
                c = box(&b[o], h3, bx, by, bz);
            }
        } else if (b[o].shape == BQ_SHAPE_LEVELSET) {
            const double v = (double)ls[o].voxel;
            const double g[3] = { ((double)x - (double)b[o].cx) / v, ((double)y - (double)b[o].cy) / v, ((double)z - (double)b[o].cz) / v };
            float s = sample_index(&ls[o], g);
            c = s <= 0.f ? 1 : (s < ls[o].background ? -1 : 0);
        } else if (b[o].shape == BQ_SHAPE_SPHERE) {
            float d2 = dx * dx + dy * dy + dz * dz;
            float R = b[o].rx + h3;
            c = d2 <= b[o].rx * b[o].rx ? 1 : (d2 < R * R ? -1 : 0);
        } else {
            c = box(&b[o], h3, dx, dy, dz);
        }
        if (c > 0) solid = o + 1;
        else if (c < 0) band = 1;
    }
    return solid ? solid : (band ? -1 : 0);
}

static float pos(int i, int staggered, float h) { return ((float)i - (staggered ? 0.5f : 0.f)) * h; }

/* every component finite, the quaternion's squared norm positive and finite */
static int poses_ok(const bq_pose *pose, int n, const char *op)
{
    for (int o = 0; pose && o < n; o++) {
        const bq_pose *p = &pose[o];
        const double s = (double)p->qw * p->qw + (double)p->qx * p->qx + (double)p->qy * p->qy + (double)p->qz * p->qz;
        if (!isfinite(p->qw) || !isfinite(p->qx) || !isfinite(p->qy) || !isfinite(p->qz) || !isfinite(p->ox) ||
            !isfinite(p->oy) || !isfinite(p->oz) || !(s > 0.0) || !isfinite(s)) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, op);
            return 0;
        }
    }
    return 1;
}

/* the checks of the _ls operators plus the poses'; 0 (and FL_ERR_BAD_ARGUMENT latched) when one fails */
static int arguments_ok(const bq_boundary *b, const bq_levelset *ls, const bq_pose *pose, int n, const char *op)
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
    return poses_ok(pose, n, op);
}

static void rotations(const bq_boundary *b, const bq_pose *pose, int n, rot_t rot[BQ_MAX_BOUNDARIES])
{
    for (int o = 0; o < n; o++) {
        rot[o].oriented = 0;
        if (pose) rotation(&b[o], &pose[o], &rot[o]);
    }
}

void gpu_obstacle_flags_pose(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                             const bq_pose *pose, float h, int ni, int nj, int nk)
{
    rot_t rot[BQ_MAX_BOUNDARIES];
    if (!arguments_ok(b, ls, pose, n, "gpu_obstacle_flags_pose")) return;
    rotations(b, pose, n, rot);
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int c = classify(b, ls, rot, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h));
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

void gpu_semilag_band_pose(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                           float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n,
                           const bq_levelset *ls, const bq_pose *pose)
{
    rot_t rot[BQ_MAX_BOUNDARIES];
    if (!arguments_ok(b, ls, pose, n, "gpu_semilag_band_pose")) return;
    if (n == 0) return;
    rotations(b, pose, n, rot);
    const int bi = ni + dim_x, bj = nj + dim_y, bk = nk + dim_z;
    const size_t cnt = (size_t)bi * bj * bk;
    float *tmp = (float *)calloc(cnt, sizeof(float));
    if (!tmp) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_semilag_band_pose: out of memory"); return; }
    orc_semilag(tmp, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt);
    for (int k = 0; k < bk; k++)
        for (int j = 0; j < bj; j++)
            for (int i = 0; i < bi; i++)
                if (classify(b, ls, rot, n, h, pos(i, dim_x, h), pos(j, dim_y, h), pos(k, dim_z, h)) == -1)
                    field[IDX(i, j, k, bi, bj)] = tmp[IDX(i, j, k, bi, bj)];
    free(tmp);
}

void gpu_obstacle_blend_pose(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                             const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                             const bq_boundary *b, int n, const bq_levelset *ls, const bq_pose *pose, float h,
                             int ni, int nj, int nk)
{
    rot_t rot[BQ_MAX_BOUNDARIES];
    if (!arguments_ok(b, ls, pose, n, "gpu_obstacle_blend_pose")) return;
    rotations(b, pose, n, rot);
    if (us) {
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i <= ni; i++)
                    if (classify(b, ls, rot, n, h, pos(i, 1, h), pos(j, 0, h), pos(k, 0, h)) == -1) u[IDX(i, j, k, ni + 1, nj)] = us[IDX(i, j, k, ni + 1, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j <= nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, rot, n, h, pos(i, 0, h), pos(j, 1, h), pos(k, 0, h)) == -1) v[IDX(i, j, k, ni, nj + 1)] = vs[IDX(i, j, k, ni, nj + 1)];
        for (int k = 0; k <= nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, rot, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 1, h)) == -1) w[IDX(i, j, k, ni, nj)] = ws[IDX(i, j, k, ni, nj)];
        for (int k = 0; k < nk; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++)
                    if (classify(b, ls, rot, n, h, pos(i, 0, h), pos(j, 0, h), pos(k, 0, h)) == -1) {
                        rho[IDX(i, j, k, ni, nj)] = rhos[IDX(i, j, k, ni, nj)];
                        T[IDX(i, j, k, ni, nj)] = Ts[IDX(i, j, k, ni, nj)];
                    }
    }
    for (size_t c = 0; c < (size_t)ni * nj * nk; c++)
        if (solid[c]) rho[c] = 0.f;
}

static int cell(const unsigned char *solid, int i, int j, int k, int ni, int nj, int nk)
{
    if (i < 0 || j < 0 || k < 0 || i >= ni || j >= nj || k >= nk) return 0;
    return solid[IDX(i, j, k, ni, nj)];
}

/* the velocity of entry o at (x, y, z), component `axis`: v + omega x (p - c), the cross product term by term */
static float rigid(const bq_boundary *b, const bq_pose *pose, int o, int axis, float x, float y, float z)
{
    const float lin = axis == 0 ? b[o].vx : (axis == 1 ? b[o].vy : b[o].vz);
    if (!pose || (pose[o].ox == 0.f && pose[o].oy == 0.f && pose[o].oz == 0.f)) return lin;
    const float dx = x - b[o].cx, dy = y - b[o].cy, dz = z - b[o].cz;
    const float ox = pose[o].ox, oy = pose[o].oy, oz = pose[o].oz;
    if (axis == 0) return lin + (oy * dz - oz * dy);
    if (axis == 1) return lin + (oz * dx - ox * dz);
    return lin + (ox * dy - oy * dx);
}

void gpu_obstacle_faces_pose(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                             const bq_boundary *b, const bq_pose *pose, int n, float h, int ni, int nj, int nk)
{
    if (n < 0 || n > BQ_MAX_BOUNDARIES || (n > 0 && !b)) { fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_obstacle_faces_pose"); return; }
    if (!poses_ok(pose, n, "gpu_obstacle_faces_pose")) return;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                int a = cell(solid, i - 1, j, k, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni + 1, nj);
                float vo = rigid(b, pose, o - 1, 0, pos(i, 1, h), pos(j, 0, h), pos(k, 0, h));
                if (du) du[id] = vo - u[id];
                u[id] = vo;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                int a = cell(solid, i, j - 1, k, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni, nj + 1);
                float vo = rigid(b, pose, o - 1, 1, pos(i, 0, h), pos(j, 1, h), pos(k, 0, h));
                if (dv) dv[id] = vo - v[id];
                v[id] = vo;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                int a = cell(solid, i, j, k - 1, ni, nj, nk), c = cell(solid, i, j, k, ni, nj, nk), o = a > c ? a : c;
                if (!o) continue;
                size_t id = IDX(i, j, k, ni, nj);
                float vo = rigid(b, pose, o - 1, 2, pos(i, 0, h), pos(j, 0, h), pos(k, 1, h));
                if (dw) dw[id] = vo - w[id];
                w[id] = vo;
            }
}
