/*
 * tracers_abi.c -- TEST-ONLY C stand-in of the tracer operators of include/bimocq_gpu.h.
 *
 * Linked on top of the render stand-in's list into tests/_build/libbimocq_host_cpu_tracers.so (tests/build_cpu_tracers.py):
 * the CPU stand-in on which the host solver's tracers run without a GPU, and against which the GPU tests compare the HIP
 * kernels.
 *
 *   gpu_trace_particles   packs the particles, chunk by chunk, into the interior entries (2 <= index < n - 2) of three
 *                         map-shaped scratch arrays and lets the oracle's orc_solve_forward trace them: the oracle's own
 *                         arithmetic, not a restatement (tests/test_tracers_cpu.py checks the packing against the oracle)
 *   gpu_sample_particles  orc_sample per particle
 *   gpu_seed_particles    the header's hash and formula, restated
 *   gpu_sort_particles    a STABLE counting sort by the header's brick key (the kernels' order inside a brick is arbitrary)
 *   tracers_abi_calls     calls of the four operators so far (reset != 0: back to 0) -- a test's proof that a step without
 *                         tracers launches nothing
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

static long g_calls = 0;

long tracers_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

static int ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return 0;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

static int refuse(const char *text)
{
    fl_report_error(FL_ERR_BAD_ARGUMENT, text);
    return FL_ERR_BAD_ARGUMENT;
}

int gpu_trace_particles(const float *u, const float *v, const float *w, float *px, float *py, float *pz, long n,
                        float h, int ni, int nj, int nk, float cfldt, float dt)
{
    if (!u || !v || !w || !px || !py || !pz) return refuse("gpu_trace_particles: null pointer");
    if (n < 0) return refuse("gpu_trace_particles: n < 0");
    if (ni < 5 || nj < 5 || nk < 5) return refuse("gpu_trace_particles: dims below 5");
    if (!isfinite(h) || !(h > 0.f) || !isfinite(cfldt) || !isfinite(dt)) return refuse("gpu_trace_particles: h, cfldt and dt must be finite");
    if (!(cfldt > 0.f) && dt != 0.f) return refuse("gpu_trace_particles: cfldt <= 0 with dt != 0");
    const size_t pb = (size_t)n * sizeof(float);
    const size_t ub = (size_t)(ni + 1) * nj * nk * 4, vb = (size_t)ni * (nj + 1) * nk * 4, wb = (size_t)ni * nj * (nk + 1) * 4;
    float *pos[3] = { px, py, pz };
    for (int a = 0; a < 3; a++)
        if (ranges_overlap(pos[a], pb, u, ub) || ranges_overlap(pos[a], pb, v, vb) || ranges_overlap(pos[a], pb, w, wb))
            return refuse("gpu_trace_particles: a position array aliases a velocity array");
    if (ranges_overlap(px, pb, py, pb) || ranges_overlap(px, pb, pz, pb) || ranges_overlap(py, pb, pz, pb))
        return refuse("gpu_trace_particles: position arrays overlap");
    g_calls++;
    if (n == 0) return FL_OK;
    const size_t cells = (size_t)ni * nj * nk;
    float *mx = (float *)calloc(cells, sizeof(float)), *my = (float *)calloc(cells, sizeof(float)), *mz = (float *)calloc(cells, sizeof(float));
    if (!mx || !my || !mz) { free(mx); free(my); free(mz); fl_report_error(FL_ERR_HIP, "gpu_trace_particles: out of memory"); return FL_ERR_HIP; }
    const long per = (long)(ni - 4) * (nj - 4) * (nk - 4);
    for (long at = 0; at < n; at += per) {
        const long m = n - at < per ? n - at : per;
        long a = 0;
        for (int k = 2; k < nk - 2; k++)
            for (int j = 2; j < nj - 2; j++)
                for (int i = 2; i < ni - 2; i++, a++) {
                    const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * (size_t)k);
                    /* entries beyond the chunk hold a harmless point of the clamp box */
                    mx[id] = a < m ? px[at + a] : h; my[id] = a < m ? py[at + a] : h; mz[id] = a < m ? pz[at + a] : h;
                }
        orc_solve_forward(u, v, w, mx, my, mz, h, ni, nj, nk, cfldt, dt);
        a = 0;
        for (int k = 2; k < nk - 2 && a < m; k++)
            for (int j = 2; j < nj - 2 && a < m; j++)
                for (int i = 2; i < ni - 2 && a < m; i++, a++) {
                    const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * (size_t)k);
                    px[at + a] = mx[id]; py[at + a] = my[id]; pz[at + a] = mz[id];
                }
    }
    free(mx); free(my); free(mz);
    return FL_OK;
}

int gpu_sample_particles(const float *field, int nx, int ny, int nz, float h, float ox, float oy, float oz,
                         const float *px, const float *py, const float *pz, float *out, long n)
{
    if (!field || !px || !py || !pz || !out) return refuse("gpu_sample_particles: null pointer");
    if (n < 0) return refuse("gpu_sample_particles: n < 0");
    if (nx < 1 || ny < 1 || nz < 1) return refuse("gpu_sample_particles: non-positive dims");
    if (!isfinite(h) || !(h > 0.f)) return refuse("gpu_sample_particles: h must be finite and positive");
    const size_t pb = (size_t)n * sizeof(float);
    if (ranges_overlap(out, pb, field, (size_t)nx * ny * nz * 4) || ranges_overlap(out, pb, px, pb) ||
        ranges_overlap(out, pb, py, pb) || ranges_overlap(out, pb, pz, pb)) return refuse("gpu_sample_particles: out aliases an input");
    g_calls++;
    for (long a = 0; a < n; a++) out[a] = orc_sample(field, nx, ny, nz, h, ox, oy, oz, px[a], py[a], pz[a]);
    return FL_OK;
}

static uint32_t seed_mix(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

int gpu_seed_particles(float *px, float *py, float *pz, int i0, int i1, int j0, int j1, int k0, int k1, int per_cell,
                       unsigned seed, float h, int ni, int nj, int nk)
{
    if (per_cell < 1) return refuse("gpu_seed_particles: per_cell < 1");
    if (ni < 5 || nj < 5 || nk < 5) return refuse("gpu_seed_particles: dims below 5");
    if (!isfinite(h) || !(h > 0.f)) return refuse("gpu_seed_particles: h must be finite and positive");
    const int a0 = imax(i0, 1), b0 = imax(j0, 1), c0 = imax(k0, 1);
    const int bx = imax(imin(i1, ni - 1) - a0, 0), by = imax(imin(j1, nj - 1) - b0, 0), bz = imax(imin(k1, nk - 1) - c0, 0);
    const double count = (double)bx * (double)by * (double)bz * (double)per_cell;
    if (count > 2147483647.0) return refuse("gpu_seed_particles: more than 2^31 - 1 particles");
    g_calls++;
    if (count == 0.0) return FL_OK;
    if (!px || !py || !pz) return refuse("gpu_seed_particles: null pointer");
    const int dims[3] = { ni, nj, nk };
    float *out[3] = { px, py, pz };
    long p = 0;
    for (int z = 0; z < bz; z++)
        for (int y = 0; y < by; y++)
            for (int x = 0; x < bx; x++)
                for (int s = 0; s < per_cell; s++, p++) {
                    const int C[3] = { a0 + x, b0 + y, c0 + z };
                    const uint64_t G = (uint64_t)C[0] + (uint64_t)ni * ((uint64_t)C[1] + (uint64_t)nj * (uint64_t)C[2]);
                    const uint64_t c = G * (uint64_t)per_cell + (uint64_t)s;
                    const uint32_t base = seed_mix(seed_mix((uint32_t)c ^ seed) + (uint32_t)(c >> 32));
                    for (int a = 0; a < 3; a++) {
                        const uint32_t r = seed_mix(base + (uint32_t)a * 0x9e3779b9u) >> 8;
                        const float f = (float)r * 5.9604644775390625e-8f;
                        const float q = (float)C[a] + f;
                        const float v = q * h;
                        const float top = (float)dims[a] * h;
                        const float hi = top - h;
                        out[a][p] = fminf(fmaxf(h, v), hi);
                    }
                }
    return FL_OK;
}

static int brick_of(float p, float h, int n)
{
    const float q = p / h;
    int c = q != q ? 0 : (q <= 0.f ? 0 : (q >= (float)n ? n - 1 : (int)floorf(q)));
    if (c > n - 1) c = n - 1;
    return c >> 2;
}

int gpu_sort_particles(const float *px, const float *py, const float *pz, const unsigned *id,
                       float *qx, float *qy, float *qz, unsigned *qid, long n, float h, int ni, int nj, int nk)
{
    if (!px || !py || !pz || !qx || !qy || !qz || !qid) return refuse("gpu_sort_particles: null pointer");
    if (n < 0 || n > 2147483647L) return refuse("gpu_sort_particles: n outside [0, 2^31)");
    if (ni < 1 || nj < 1 || nk < 1) return refuse("gpu_sort_particles: non-positive dims");
    if (!isfinite(h) || !(h > 0.f)) return refuse("gpu_sort_particles: h must be finite and positive");
    const size_t pb = (size_t)n * sizeof(float);
    const void *ins[4] = { px, py, pz, id }, *outs[4] = { qx, qy, qz, qid };
    for (int a = 0; a < 4; a++) {
        for (int b = 0; b < 4; b++)
            if (ranges_overlap(outs[a], pb, ins[b], pb)) return refuse("gpu_sort_particles: an output aliases an input");
        for (int b = a + 1; b < 4; b++)
            if (ranges_overlap(outs[a], pb, outs[b], pb)) return refuse("gpu_sort_particles: outputs overlap");
    }
    g_calls++;
    if (n == 0) return FL_OK;
    const int nbx = (ni + 3) / 4, nby = (nj + 3) / 4, nbz = (nk + 3) / 4;
    const size_t nb = (size_t)nbx * nby * nbz;
    unsigned *table = (unsigned *)calloc(nb + 1, sizeof(unsigned));
    unsigned *key = (unsigned *)malloc((size_t)n * sizeof(unsigned));
    if (!table || !key) { free(table); free(key); fl_report_error(FL_ERR_HIP, "gpu_sort_particles: out of memory"); return FL_ERR_HIP; }
    for (long a = 0; a < n; a++) {
        key[a] = (unsigned)(brick_of(px[a], h, ni) + nbx * (brick_of(py[a], h, nj) + nby * brick_of(pz[a], h, nk)));
        table[key[a] + 1]++;
    }
    for (size_t b = 0; b < nb; b++) table[b + 1] += table[b];
    for (long a = 0; a < n; a++) {
        const unsigned slot = table[key[a]]++;
        qx[slot] = px[a]; qy[slot] = py[a]; qz[slot] = pz[a];
        qid[slot] = id ? id[a] : (unsigned)a;
    }
    free(table); free(key);
    return FL_OK;
}
