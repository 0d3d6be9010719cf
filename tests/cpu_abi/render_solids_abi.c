/*
 * render_solids_abi.c -- TEST-ONLY C restatement of gpu_render_density_solids of include/bimocq_gpu.h.
 *
 * Linked on top of the preview stand-in's list into tests/_build/libbimocq_host_cpu_render_solids.so
 * (tests/build_cpu_render_solids.py): the CPU stand-in on which the host solver's render_solids calls run without a GPU, and
 * against which the GPU tests compare the HIP kernels bit for bit.  Written from the header's contract as plain triple loops:
 * one statement per IEEE operation, orc_expf for the exponential, int64 sums.  `rows` is checked for overlap and otherwise
 * not read.
 *
 *   render_solids_abi_set_slab  the z-slab context the operator refuses under (nk_global <= 0: off); oracle_abi.c keeps the
 *                               one the host solver sets to itself, so a test hands it over
 *   render_solids_abi_calls     how many calls got past the refusals (reset != 0: back to 0)
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

static long g_calls = 0;
static int s_on = 0;

long render_solids_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

void render_solids_abi_set_slab(int nk_global) { s_on = nk_global > 0; }

#define IC(i, j, k) ((size_t)(i) + (size_t)ni * ((size_t)(j) + (size_t)nj * (size_t)(k)))
#define TWO32 4294967296.0

static int is_solid(const unsigned char *solid, size_t ic) { return (solid[ic] & 0x7f) != 0; }

/* the fluid cell's optical depth d, its fixed-point form D and its opacity a */
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

/* T[cell] = att'(A, B) with the exclusive prefixes A (of D) and B (of "solid") in the travel order of direction `dir` */
static void transmit(const float *rho, const unsigned char *solid, float sh, int ni, int nj, int nk, int dir, float *T)
{
    const int axis = dir / 2, back = dir & 1;
    const int n[3] = { ni, nj, nk };
    const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
    int c[3];
    for (c[a2] = 0; c[a2] < n[a2]; c[a2]++)
        for (c[a1] = 0; c[a1] < n[a1]; c[a1]++) {
            int64_t A = 0;
            int B = 0;
            for (int t = 0; t < n[axis]; t++) {
                c[axis] = back ? n[axis] - 1 - t : t;
                const size_t ic = IC(c[0], c[1], c[2]);
                float a;
                T[ic] = B ? 0.0f : att(A);
                if (is_solid(solid, ic)) B = 1;
                else A += cell_depth(rho[ic], sh, &a);
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

int gpu_render_density_solids(const float *rho, const unsigned char *solid, const unsigned char *rows, float *shadow, float h,
                              int ni, int nj, int nk, int view, int light, const fl_render_params *p,
                              const fl_render_solid_params *sp, double *d_image)
{
    if (!rho || !p || !d_image) return refuse("gpu_render_density_solids: null rho, p or d_image");
    if (!solid || !sp) return refuse("gpu_render_density_solids: null solid or sp");
    if (view < 0 || view > 5) return refuse("gpu_render_density_solids: view outside 0..5");
    if (light < -1 || light > 5) return refuse("gpu_render_density_solids: light outside -1..5");
    if (light >= 0 && !shadow) return refuse("gpu_render_density_solids: a light needs the shadow field");
    if (ni < 1 || nj < 1 || nk < 1 || ni > 65534 || nj > 65534 || nk > 65534) return refuse("gpu_render_density_solids: dims outside 1..65534");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("gpu_render_density_solids: field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("gpu_render_density_solids: plane of 2^23 elements or more");
    if (!(h > 0.0f) || isinf(h)) return refuse("gpu_render_density_solids: h must be positive and finite");
    if (!(p->sigma >= 0.0f) || isinf(p->sigma) || !(p->albedo >= 0.0f) || isinf(p->albedo) || !(p->ambient >= 0.0f) || isinf(p->ambient))
        return refuse("gpu_render_density_solids: sigma, albedo and ambient must be finite and >= 0");
    if (p->albedo + p->ambient > 4.0f) return refuse("gpu_render_density_solids: albedo + ambient > 4");
    if (!(sp->albedo >= 0.0f) || isinf(sp->albedo) || !(sp->ambient >= 0.0f) || isinf(sp->ambient))
        return refuse("gpu_render_density_solids: the solids' albedo and ambient must be finite and >= 0");
    if (sp->albedo + sp->ambient > 4.0f) return refuse("gpu_render_density_solids: the solids' albedo + ambient > 4");
    const int vaxis = view / 2;
    const int W = vaxis == 0 ? nj : ni, H = vaxis == 2 ? nj : nk;
    const size_t nc = (size_t)ni * nj * nk, npix = (size_t)W * H, nimg = 3 * npix * sizeof(double), nrows = (size_t)nj * nk;
    if (ranges_overlap(d_image, nimg, rho, nc * sizeof(float)) || ranges_overlap(shadow, nc * sizeof(float), rho, nc * sizeof(float)) ||
        ranges_overlap(shadow, nc * sizeof(float), d_image, nimg))
        return refuse("gpu_render_density_solids: d_image or shadow overlaps rho");
    if (ranges_overlap(solid, nc, shadow, nc * sizeof(float)) || ranges_overlap(solid, nc, d_image, nimg) ||
        ranges_overlap(rows, nrows, shadow, nc * sizeof(float)) || ranges_overlap(rows, nrows, d_image, nimg))
        return refuse("gpu_render_density_solids: solid or rows overlaps shadow or d_image");
    if (s_on) {
        fl_report_error(FL_ERR_UNSUPPORTED, "gpu_render_density_solids: not supported under a z-slab context");
        return FL_ERR_UNSUPPORTED;
    }
    g_calls++;
    const float sh = p->sigma * h;

    float *T = (float *)malloc(nc * sizeof(float));
    if (light >= 0) {
        transmit(rho, solid, sh, ni, nj, nk, light, T);
        for (size_t ic = 0; ic < nc; ic++) shadow[ic] = T[ic];
    }
    transmit(rho, solid, sh, ni, nj, nk, view, T);
    int64_t *C = (int64_t *)calloc(npix, sizeof(int64_t)), *Asum = (int64_t *)calloc(npix, sizeof(int64_t));
    int64_t *Hit = (int64_t *)calloc(npix, sizeof(int64_t));
    /* the first solid cell of a view ray: in travel order, so the loops below run the view axis in travel order */
    const int back = view & 1;
    const int n[3] = { ni, nj, nk };
    const int a1 = (vaxis + 1) % 3, a2 = (vaxis + 2) % 3;
    int c[3];
    for (c[a2] = 0; c[a2] < n[a2]; c[a2]++)
        for (c[a1] = 0; c[a1] < n[a1]; c[a1]++)
            for (int t = 0; t < n[vaxis]; t++) {
                c[vaxis] = back ? n[vaxis] - 1 - t : t;
                const int i = c[0], j = c[1], k = c[2];
                const size_t ic = IC(i, j, k);
                const size_t pix = vaxis == 2 ? (size_t)i + (size_t)ni * j : vaxis == 1 ? (size_t)i + (size_t)ni * k : (size_t)j + (size_t)nj * k;
                const float s = light >= 0 ? shadow[ic] : 1.0f;
                const float Tv = T[ic];
                if (is_solid(solid, ic)) {
                    const float t1 = sp->albedo * s;
                    const float qs = t1 + sp->ambient;
                    const double prod = (double)Tv * (double)qs;
                    const double term = trunc(prod * TWO32);
                    C[pix] += (int64_t)term;
                    if (!Hit[pix]) Hit[pix] = solid[ic] & 0x7f;
                } else {
                    float a;
                    const int64_t D = cell_depth(rho[ic], sh, &a);
                    const float t1 = p->albedo * s;
                    const float t2 = t1 + p->ambient;
                    const float q = a * t2;
                    const double prod = (double)Tv * (double)q;
                    const double term = trunc(prod * TWO32);
                    C[pix] += (int64_t)term;
                    Asum[pix] += D;
                }
            }
    for (size_t x = 0; x < npix; x++) {
        d_image[x] = (double)C[x];
        d_image[npix + x] = (double)Asum[x];
        d_image[2 * npix + x] = (double)Hit[x];
    }
    free(T); free(C); free(Asum); free(Hit);
    return FL_OK;
}
