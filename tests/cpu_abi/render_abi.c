/*
 * render_abi.c -- TEST-ONLY C restatement of gpu_render_density of include/bimocq_gpu.h.
 *
 * Linked on top of the diagnostics stand-in's list into tests/_build/libbimocq_host_cpu_render.so (tests/build_cpu_render.py):
 * the CPU stand-in on which the host solver's render calls run without a GPU, and against which the GPU tests compare the HIP
 * kernels bit for bit.  Written from the header's contract as plain triple loops: one statement per IEEE operation, orc_expf
 * for the exponential, int64 sums.
 *
 *   render_abi_set_slab       the z-slab context gpu_render_density evaluates under (nkg <= 0: off).  oracle_abi.c keeps the
 *                             one the host solver sets (fl_set_slab) to itself, so a slab worker hands the same numbers over
 *   render_abi_set_allreduce  likewise the transport's all-reduce, the rank count and this rank's index (ranks are ordered
 *                             along z)
 *   render_abi_calls          how many calls have been made (reset != 0: back to 0) -- a test's proof that a refused call and
 *                             a step launch nothing
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

static long g_calls = 0;
static int s_on = 0, s_koff = 0, s_nkg = 0, s_own0 = 0, s_own1 = 0;
static fl_allreduce_cb s_allreduce = NULL;
static int s_nranks = 1, s_rank = 0;

long render_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

void render_abi_set_slab(int koff, int nk_global, int own0, int own1)
{
    s_on = nk_global > 0; s_koff = koff; s_nkg = nk_global; s_own0 = own0; s_own1 = own1;
}

void render_abi_set_allreduce(fl_allreduce_cb cb, int nranks, int rank)
{
    s_allreduce = cb; s_nranks = nranks; s_rank = rank;
}

#define IC(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)nj * (size_t)(k)))
#define TWO32 4294967296.0

/* the cell's optical depth d, its fixed-point form D and its opacity a */
static int64_t cell_depth(float rho, float sh, float *a)
{
    const float r = fmaxf(rho, 0.0f);
    const float t = sh * r;
    const float d = fminf(t, 32.0f);
    const double D = trunc((double)d * TWO32);
    const float e = orc_expf(-d);
    *a = 1.0f - e;
    return (int64_t)D;
}

static float att(int64_t A)
{
    if (A >= (int64_t)128 * ((int64_t)1 << 32)) return 0.0f;
    const double x = (double)A * (1.0 / TWO32);
    const float xf = (float)x;
    return orc_expf(-xf);
}

/* exclusive prefix sums of D in the travel order of direction `dir` over the local planes [p0, p1); start: NULL or what
 * every column (i, j) starts at (dir along z on a slab rank) */
static void prefix(const float *rho, float sh, int ni, int nj, int p0, int p1, int dir, const int64_t *start, int64_t *A)
{
    const int axis = dir / 2, back = dir & 1;
    const int n[3] = { ni, nj, p1 - p0 };
    const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
    int c[3];
    for (c[a2] = 0; c[a2] < n[a2]; c[a2]++)
        for (c[a1] = 0; c[a1] < n[a1]; c[a1]++) {
            int64_t run = 0;
            for (int t = 0; t < n[axis]; t++) {
                c[axis] = back ? n[axis] - 1 - t : t;
                const size_t ic = IC(c[0], c[1], c[2] + p0);
                if (t == 0 && start) run = start[(size_t)c[0] + (size_t)ni * c[1]];
                float a;
                A[ic] = run;
                run += cell_depth(rho[ic], sh, &a);
            }
        }
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

int gpu_render_density(const float *rho, float *shadow, float h, int ni, int nj, int nk, int view, int light,
                       const fl_render_params *p, double *d_image)
{
    if (!rho || !p || !d_image) return refuse("gpu_render_density: null rho, p or d_image");
    if (view < 0 || view > 5) return refuse("gpu_render_density: view outside 0..5");
    if (light < -1 || light > 5) return refuse("gpu_render_density: light outside -1..5");
    if (light >= 0 && !shadow) return refuse("gpu_render_density: a light needs the shadow field");
    if (ni < 1 || nj < 1 || nk < 1 || ni > 65534 || nj > 65534 || nk > 65534) return refuse("gpu_render_density: dims outside 1..65534");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("gpu_render_density: field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("gpu_render_density: plane of 2^23 elements or more");
    if (!(h > 0.0f) || isinf(h)) return refuse("gpu_render_density: h must be positive and finite");
    if (!(p->sigma >= 0.0f) || isinf(p->sigma) || !(p->albedo >= 0.0f) || isinf(p->albedo) || !(p->ambient >= 0.0f) || isinf(p->ambient))
        return refuse("gpu_render_density: sigma, albedo and ambient must be finite and >= 0");
    if (p->albedo + p->ambient > 4.0f) return refuse("gpu_render_density: albedo + ambient > 4");
    const int koff = s_on ? s_koff : 0, nkg = s_on ? s_nkg : nk;
    const int vaxis = view / 2;
    const int W = vaxis == 0 ? nj : ni, H = vaxis == 2 ? nj : nkg;
    const size_t nc = (size_t)ni * nj * nk, npix = (size_t)W * H;
    if (ranges_overlap(d_image, 2 * npix * sizeof(double), rho, nc * sizeof(float)) ||
        ranges_overlap(shadow, nc * sizeof(float), rho, nc * sizeof(float)) ||
        ranges_overlap(shadow, nc * sizeof(float), d_image, 2 * npix * sizeof(double)))
        return refuse("gpu_render_density: d_image or shadow overlaps rho");
    g_calls++;
    int p0 = s_on ? s_own0 - koff : 0, p1 = s_on ? s_own1 - koff : nk;
    if (p0 < 0) p0 = 0;
    if (p1 > nk) p1 = nk;
    if (p1 < p0) p1 = p0;
    const int ranks = (s_on && s_allreduce) ? s_nranks : 1;
    const float sh = p->sigma * h;
    const size_t ncol = (size_t)ni * nj;

    /* the starting offsets of the columns along z: the totals of the ranks before (+z) and after (-z) this one */
    int64_t *before = NULL, *after = NULL;
    const int zneeded = vaxis == 2 || (light >= 0 && light / 2 == 2);
    if (ranks > 1 && zneeded) {
        double *gath = (double *)calloc((size_t)ranks * ncol, sizeof(double));
        before = (int64_t *)calloc(ncol, sizeof(int64_t));
        after = (int64_t *)calloc(ncol, sizeof(int64_t));
        for (int k = p0; k < p1; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++) {
                    float a;
                    gath[(size_t)s_rank * ncol + i + (size_t)ni * j] += (double)cell_depth(rho[IC(i, j, k)], sh, &a);
                }
        s_allreduce(gath, (int)((size_t)ranks * ncol), 1, 0);
        for (int r = 0; r < ranks; r++)
            for (size_t c = 0; c < ncol; c++) {
                if (r < s_rank) before[c] += (int64_t)gath[(size_t)r * ncol + c];
                if (r > s_rank) after[c] += (int64_t)gath[(size_t)r * ncol + c];
            }
        free(gath);
    }

    int64_t *A = (int64_t *)malloc((nc ? nc : 1) * sizeof(int64_t));
    if (light >= 0) {
        prefix(rho, sh, ni, nj, p0, p1, light, light / 2 == 2 ? (light & 1 ? after : before) : NULL, A);
        for (int k = p0; k < p1; k++)
            for (int j = 0; j < nj; j++)
                for (int i = 0; i < ni; i++) shadow[IC(i, j, k)] = att(A[IC(i, j, k)]);
    }
    prefix(rho, sh, ni, nj, p0, p1, view, vaxis == 2 ? (view & 1 ? after : before) : NULL, A);
    int64_t *C = (int64_t *)calloc(npix ? npix : 1, sizeof(int64_t)), *Asum = (int64_t *)calloc(npix ? npix : 1, sizeof(int64_t));
    for (int k = p0; k < p1; k++)
        for (int j = 0; j < nj; j++)
            for (int i = 0; i < ni; i++) {
                const size_t ic = IC(i, j, k);
                const int kg = k + koff;
                const size_t pix = vaxis == 2 ? (size_t)i + (size_t)ni * j : vaxis == 1 ? (size_t)i + (size_t)ni * kg : (size_t)j + (size_t)nj * kg;
                float a;
                const int64_t D = cell_depth(rho[ic], sh, &a);
                const float s = light >= 0 ? shadow[ic] : 1.0f;
                const float t1 = p->albedo * s;
                const float t2 = t1 + p->ambient;
                const float q = a * t2;
                const float Tv = att(A[ic]);
                const double prod = (double)Tv * (double)q;
                const double term = trunc(prod * TWO32);
                C[pix] += (int64_t)term;
                Asum[pix] += D;
            }
    for (size_t x = 0; x < npix; x++) { d_image[x] = (double)C[x]; d_image[npix + x] = (double)Asum[x]; }
    if (ranks > 1) s_allreduce(d_image, (int)(2 * npix), 1, 0);
    free(A); free(C); free(Asum); free(before); free(after);
    return FL_OK;
}
