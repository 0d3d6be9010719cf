/*
 * confinement_abi.c -- TEST-ONLY C restatement of gpu_vorticity_confinement of include/bimocq_gpu.h.
 *
 * Linked on top of the diagnostics stand-in's list into tests/_build/libbimocq_host_cpu_confinement.so
 * (tests/build_cpu_confinement.py): the CPU stand-in on which the host solver's confinement runs without a GPU, and against
 * which the GPU tests compare the HIP kernels bit for bit.  Written from the header's text, one statement per IEEE operation,
 * as four plain passes over scratch arrays: omega and m per cell, f per cell, the faces.
 *
 *   confinement_abi_calls   how many calls have been made (reset != 0: back to 0) -- a test's proof that a step with the
 *                           coefficient at 0 launches nothing
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/bimocq_gpu.h"

static long g_calls = 0;

long confinement_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

#define IU(i, j, k) ((size_t)(i) + (size_t)(ni + 1) * ((size_t)(j) + (size_t)nj * (size_t)(k)))
#define IV(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)(nj + 1) * (size_t)(k)))
#define IC(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)nj * (size_t)(k)))

static float cen_u(const float *u, int ni, int nj, int i, int j, int k) { float s = u[IU(i, j, k)] + u[IU(i + 1, j, k)]; return 0.5f * s; }
static float cen_v(const float *v, int ni, int nj, int i, int j, int k) { float s = v[IV(i, j, k)] + v[IV(i, j + 1, k)]; return 0.5f * s; }
static float cen_w(const float *w, int ni, int nj, int i, int j, int k) { float s = w[IC(i, j, k)] + w[IC(i, j, k + 1)]; return 0.5f * s; }

static int ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

static int refuse(const char *why)
{
    fl_report_error(FL_ERR_BAD_ARGUMENT, why);
    return FL_ERR_BAD_ARGUMENT;
}

int gpu_vorticity_confinement(float *uo, float *vo, float *wo, const float *u, const float *v, const float *w,
                              float h, int ni, int nj, int nk, float eps, float dt)
{
    if (!uo || !vo || !wo || !u || !v || !w) return refuse("gpu_vorticity_confinement: null pointer");
    if (ni < 3 || nj < 3 || nk < 3) return refuse("gpu_vorticity_confinement: dims below 3");
    if (!(eps >= 0.f) || !isfinite(eps)) return refuse("gpu_vorticity_confinement: eps negative or not finite");
    const size_t nb[3] = { (size_t)(ni + 1) * nj * nk * sizeof(float), (size_t)ni * (nj + 1) * nk * sizeof(float),
                           (size_t)ni * nj * (nk + 1) * sizeof(float) };
    const void *out[3] = { uo, vo, wo }, *in[3] = { u, v, w };
    for (int a = 0; a < 3; a++) {
        for (int c = 0; c < 3; c++)
            if (ranges_overlap(out[a], nb[a], in[c], nb[c])) return refuse("gpu_vorticity_confinement: an output overlaps an input");
        for (int c = a + 1; c < 3; c++)
            if (ranges_overlap(out[a], nb[a], out[c], nb[c])) return refuse("gpu_vorticity_confinement: two outputs overlap");
    }
    g_calls++;
    const size_t n = (size_t)ni * nj * nk;
    /* omega (3 n), m (n), f (3 n): zero wherever the contract says 0 */
    float *om = (float *)calloc(7 * n, sizeof(float));
    if (!om) { fl_report_error(FL_ERR_HIP, "gpu_vorticity_confinement: out of host memory"); return FL_ERR_HIP; }
    float *wxs = om, *wys = om + n, *wzs = om + 2 * n, *ms = om + 3 * n, *fxs = om + 4 * n, *fys = om + 5 * n, *fzs = om + 6 * n;
    const float q = 2.0f * h;
    for (int k = 1; k <= nk - 2; k++)
        for (int j = 1; j <= nj - 2; j++)
            for (int i = 1; i <= ni - 2; i++) {
                const float a1 = cen_w(w, ni, nj, i, j + 1, k) - cen_w(w, ni, nj, i, j - 1, k);
                const float b1 = cen_v(v, ni, nj, i, j, k + 1) - cen_v(v, ni, nj, i, j, k - 1);
                const float c1 = a1 - b1;
                const float wx = c1 / q;
                const float a2 = cen_u(u, ni, nj, i, j, k + 1) - cen_u(u, ni, nj, i, j, k - 1);
                const float b2 = cen_w(w, ni, nj, i + 1, j, k) - cen_w(w, ni, nj, i - 1, j, k);
                const float c2 = a2 - b2;
                const float wy = c2 / q;
                const float a3 = cen_v(v, ni, nj, i + 1, j, k) - cen_v(v, ni, nj, i - 1, j, k);
                const float b3 = cen_u(u, ni, nj, i, j + 1, k) - cen_u(u, ni, nj, i, j - 1, k);
                const float c3 = a3 - b3;
                const float wz = c3 / q;
                double t = (double)wx * (double)wx;
                t = t + (double)wy * (double)wy;
                t = t + (double)wz * (double)wz;
                const size_t ic = IC(i, j, k);
                wxs[ic] = wx; wys[ic] = wy; wzs[ic] = wz;
                ms[ic] = (float)sqrt(t);
            }
    const float eh = eps * h;
    for (int k = 2; k <= nk - 3; k++)
        for (int j = 2; j <= nj - 3; j++)
            for (int i = 2; i <= ni - 3; i++) {
                const float dx = ms[IC(i + 1, j, k)] - ms[IC(i - 1, j, k)];
                const float dy = ms[IC(i, j + 1, k)] - ms[IC(i, j - 1, k)];
                const float dz = ms[IC(i, j, k + 1)] - ms[IC(i, j, k - 1)];
                const float gx = dx / q;
                const float gy = dy / q;
                const float gz = dz / q;
                double g2 = (double)gx * (double)gx;
                g2 = g2 + (double)gy * (double)gy;
                g2 = g2 + (double)gz * (double)gz;
                const float len = (float)sqrt(g2);
                if (!(len > 0.f)) continue;
                const float nx = gx / len;
                const float ny = gy / len;
                const float nz = gz / len;
                const size_t ic = IC(i, j, k);
                const float wx = wxs[ic], wy = wys[ic], wz = wzs[ic];
                const float p1 = ny * wz, p2 = nz * wy, d1 = p1 - p2;
                const float p3 = nz * wx, p4 = nx * wz, d2 = p3 - p4;
                const float p5 = nx * wy, p6 = ny * wx, d3 = p5 - p6;
                fxs[ic] = eh * d1;
                fys[ic] = eh * d2;
                fzs[ic] = eh * d3;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i <= ni; i++) {
                const size_t a = IU(i, j, k);
                if (i < 1 || i > ni - 1) { uo[a] = u[a]; continue; }
                const float s = fxs[IC(i - 1, j, k)] + fxs[IC(i, j, k)];
                const float mean = 0.5f * s;
                const float add = dt * mean;
                uo[a] = u[a] + add;
            }
    for (int k = 0; k < nk; k++)
        for (int j = 0; j <= nj; j++)
            for (int i = 0; i < ni; i++) {
                const size_t a = IV(i, j, k);
                if (j < 1 || j > nj - 1) { vo[a] = v[a]; continue; }
                const float s = fys[IC(i, j - 1, k)] + fys[IC(i, j, k)];
                const float mean = 0.5f * s;
                const float add = dt * mean;
                vo[a] = v[a] + add;
            }
    for (int k = 0; k <= nk; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                const size_t a = IC(i, j, k);
                if (k < 1 || k > nk - 1) { wo[a] = w[a]; continue; }
                const float s = fzs[IC(i, j, k - 1)] + fzs[IC(i, j, k)];
                const float mean = 0.5f * s;
                const float add = dt * mean;
                wo[a] = w[a] + add;
            }
    free(om);
    return FL_OK;
}
