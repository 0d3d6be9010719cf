/*
 * obstacle_loads_abi.c -- TEST-ONLY C restatement of gpu_obstacle_loads of include/bimocq_gpu.h.
 *
 * Linked on top of the diagnostics stand-in's list into tests/_build/libbimocq_host_cpu_loads.so (tests/build_cpu_loads.py): the
 * CPU stand-in on which the host solver's load sampling runs without a GPU, and against which the GPU tests compare the HIP
 * kernel.  Written from the header's definitions, one statement per IEEE operation: straight loops over the cells in k, j, i
 * order, the six neighbours of an obstacle cell in the order -x, +x, -y, +y, -z, +z, the sums taken in that order (the
 * kernel sums in another one: the tests bound the difference).
 *
 *   obstacle_loads_abi_terms  per wetted face, in the order above: the owner o, the axis, and the eight values the face adds
 *                             to row o (BQ_LOAD_* order; 0 where it adds nothing) -- what a test sums exactly
 *   obstacle_loads_abi_calls  how many calls have been made (reset != 0: back to 0) -- a test's proof that a step with
 *                             BQ_OPT_OBSTACLE_LOADS = 0 launches nothing
 *   obstacle_loads_abi_log    the last LOG_DEPTH successful calls: the pressure pointer, copies of the pressure (as double),
 *                             of the flags and of the 128 outputs, the centres and n -- the reflection scheme's first
 *                             projection overwrites nothing a test could download afterwards, so it is kept here
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bimocq_gpu.h"

#define NOUT (BQ_MAX_BOUNDARIES * BQ_LOAD_COUNT)
#define LOG_DEPTH 4

static long g_calls = 0;

typedef struct {
    const void *ptr;
    int is64, n, ni, nj, nk;
    double *p;
    unsigned char *solid;
    double out[NOUT];
    double centres[BQ_MAX_BOUNDARIES * 3];
} log_entry;
static log_entry g_log[LOG_DEPTH];
static long g_logged = 0;

long obstacle_loads_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

#define IC(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)nj * (size_t)(k)))

/* the wetted face between the obstacle cell S = (i, j, k) of o and its neighbour one step d along axis a, when there is one:
 * its eight values into t, and 1; else 0 */
static int face_terms(const float *p, const double *p64, const unsigned char *solid, const bq_boundary *b, double h,
                      int ni, int nj, int nk, int i, int j, int k, int o, int a, int d, double t[BQ_LOAD_COUNT])
{
    const int fi = i + (a == 0 ? d : 0), fj = j + (a == 1 ? d : 0), fk = k + (a == 2 ? d : 0);
    if (fi < 0 || fi >= ni || fj < 0 || fj >= nj || fk < 0 || fk >= nk) return 0;
    if (solid[IC(fi, fj, fk)] != 0) return 0;
    const double pf = p ? (double)p[IC(fi, fj, fk)] : p64[IC(fi, fj, fk)];
    const double s = d > 0 ? -1.0 : 1.0;                /* +1 when S has the higher index */
    const double f = s * pf;
    double x[3];
    const int idx[3] = { i, j, k }, fidx[3] = { fi, fj, fk };
    for (int c = 0; c < 3; c++) {
        if (c == a) {
            const double m = (double)(idx[c] + fidx[c]) * 0.5;
            x[c] = m * h;
        } else {
            x[c] = (double)idx[c] * h;
        }
    }
    const double rx = x[0] - (double)b[o].cx, ry = x[1] - (double)b[o].cy, rz = x[2] - (double)b[o].cz;
    for (int c = 0; c < BQ_LOAD_COUNT; c++) t[c] = 0.0;
    t[BQ_LOAD_PX + a] = f;
    if (a == 0) { const double q1 = rz * f, q2 = ry * f; t[BQ_LOAD_MY] = q1; t[BQ_LOAD_MZ] = -q2; }
    if (a == 1) { const double q1 = rx * f, q2 = rz * f; t[BQ_LOAD_MZ] = q1; t[BQ_LOAD_MX] = -q2; }
    if (a == 2) { const double q1 = ry * f, q2 = rx * f; t[BQ_LOAD_MX] = q1; t[BQ_LOAD_MY] = -q2; }
    t[BQ_LOAD_FACES] = 1.0;
    t[BQ_LOAD_PSUM] = pf;
    return 1;
}

/* every wetted face in the restatement's order; returns their number and fills the first `capacity` entries of owner, axis
 * and terms (BQ_LOAD_COUNT doubles per face); NULL arrays: only the count */
long obstacle_loads_abi_terms(const float *p, const double *p64, const unsigned char *solid, const bq_boundary *b, int n, float h,
                              int ni, int nj, int nk, long capacity, int *owner, int *axis, double *terms)
{
    long m = 0;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                const int own = solid[IC(i, j, k)] & 0x7f;
                if (own < 1 || own > n) continue;
                for (int a = 0; a < 3; a++)
                    for (int d = -1; d <= 1; d += 2) {
                        double t[BQ_LOAD_COUNT];
                        if (!face_terms(p, p64, solid, b, (double)h, ni, nj, nk, i, j, k, own - 1, a, d, t)) continue;
                        if (m < capacity && owner && axis && terms) {
                            owner[m] = own - 1; axis[m] = a;
                            memcpy(terms + (size_t)m * BQ_LOAD_COUNT, t, sizeof t);
                        }
                        m++;
                    }
            }
    return m;
}

static int ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return 0;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

static int refuse(const char *why)
{
    fl_report_error(FL_ERR_BAD_ARGUMENT, why);
    return FL_ERR_BAD_ARGUMENT;
}

int gpu_obstacle_loads(const float *p, const double *p64, const unsigned char *solid, const unsigned char *rows,
                       const bq_boundary *b, int n, float h, int ni, int nj, int nk, double *d_out)
{
    if ((p != NULL) == (p64 != NULL)) return refuse("gpu_obstacle_loads: exactly one of p and p64");
    if (!solid || !d_out) return refuse("gpu_obstacle_loads: null solid or d_out");
    if (n < 0 || n > BQ_MAX_BOUNDARIES) return refuse("gpu_obstacle_loads: 0 .. 16 obstacles");
    if (n > 0 && !b) return refuse("gpu_obstacle_loads: obstacles without a list");
    for (int o = 0; o < n; o++)
        if (!isfinite(b[o].cx) || !isfinite(b[o].cy) || !isfinite(b[o].cz)) return refuse("gpu_obstacle_loads: non-finite centre");
    if (!isfinite(h) || !(h > 0.f)) return refuse("gpu_obstacle_loads: h not finite or not positive");
    if (ni < 3 || nj < 3 || nk < 3) return refuse("gpu_obstacle_loads: dims below 3");
    const size_t nc = (size_t)ni * nj * nk;
    if (ranges_overlap(d_out, NOUT * sizeof(double), p, nc * sizeof(float)) || ranges_overlap(d_out, NOUT * sizeof(double), p64, nc * sizeof(double)) ||
        ranges_overlap(d_out, NOUT * sizeof(double), solid, nc) || ranges_overlap(d_out, NOUT * sizeof(double), rows, (size_t)nj * nk))
        return refuse("gpu_obstacle_loads: d_out overlaps an input");
    g_calls++;
    double S[NOUT];
    for (int a = 0; a < NOUT; a++) S[a] = 0.0;
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++) {
            if (rows && !rows[(size_t)j + (size_t)nj * k]) continue;       /* no solid cell in this row: nothing is read */
            for (int i = 0; i < ni; i++) {
                const int own = solid[IC(i, j, k)] & 0x7f;
                if (own < 1 || own > n) continue;
                for (int a = 0; a < 3; a++)
                    for (int d = -1; d <= 1; d += 2) {
                        double t[BQ_LOAD_COUNT];
                        if (!face_terms(p, p64, solid, b, (double)h, ni, nj, nk, i, j, k, own - 1, a, d, t)) continue;
                        double *row = S + (own - 1) * BQ_LOAD_COUNT;
                        row[BQ_LOAD_PX + a] += t[BQ_LOAD_PX + a];
                        const int m1 = BQ_LOAD_MX + (a + 1) % 3, m2 = BQ_LOAD_MX + (a + 2) % 3;
                        row[m1] += t[m1];
                        row[m2] += t[m2];
                        row[BQ_LOAD_FACES] += 1.0;
                        row[BQ_LOAD_PSUM] += t[BQ_LOAD_PSUM];
                    }
            }
        }
    for (int a = 0; a < NOUT; a++) d_out[a] = S[a];
    /* the log */
    log_entry *e = &g_log[g_logged % LOG_DEPTH];
    free(e->p); free(e->solid);
    e->ptr = p ? (const void *)p : (const void *)p64;
    e->is64 = p64 != NULL; e->n = n; e->ni = ni; e->nj = nj; e->nk = nk;
    e->p = (double *)malloc(nc * sizeof(double));
    e->solid = (unsigned char *)malloc(nc);
    if (e->p && e->solid) {
        for (size_t c = 0; c < nc; c++) e->p[c] = p ? (double)p[c] : p64[c];
        memcpy(e->solid, solid, nc);
    }
    memcpy(e->out, S, sizeof S);
    for (int o = 0; o < BQ_MAX_BOUNDARIES; o++) {
        e->centres[3 * o] = o < n ? (double)b[o].cx : 0.0;
        e->centres[3 * o + 1] = o < n ? (double)b[o].cy : 0.0;
        e->centres[3 * o + 2] = o < n ? (double)b[o].cz : 0.0;
    }
    g_logged++;
    return FL_OK;
}

/* the call `back` calls before the newest: meta = {is64, n, ni, nj, nk}, and where non-NULL the copies (p: ni nj nk doubles,
 * solid: ni nj nk bytes, out: 128 doubles, centres: 48 doubles).  Returns the pressure pointer of that call as an integer,
 * or 0 when the log does not hold it. */
uintptr_t obstacle_loads_abi_log(int back, int meta[5], double *p, unsigned char *solid, double *out, double *centres)
{
    if (back < 0 || back >= LOG_DEPTH || back >= g_logged) return 0;
    const log_entry *e = &g_log[(g_logged - 1 - back) % LOG_DEPTH];
    if (!e->p || !e->solid) return 0;
    const size_t nc = (size_t)e->ni * e->nj * e->nk;
    if (meta) { meta[0] = e->is64; meta[1] = e->n; meta[2] = e->ni; meta[3] = e->nj; meta[4] = e->nk; }
    if (p) memcpy(p, e->p, nc * sizeof(double));
    if (solid) memcpy(solid, e->solid, nc);
    if (out) memcpy(out, e->out, sizeof e->out);
    if (centres) memcpy(centres, e->centres, sizeof e->centres);
    return (uintptr_t)e->ptr;
}
