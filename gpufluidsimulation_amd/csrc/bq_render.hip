// bq_render.hip -- shadowed density preview on the device: gpu_render_density draws an orthographic
// emission-absorption image of the density along a grid axis, self-shadowed by one directional light along a grid axis.  The
// contract is in include/bimocq_gpu.h, every line one IEEE operation (-ffp-contract=off); tests/cpu_abi/render_abi.c restates
// it as plain triple loops.  Every accumulated quantity -- the prefix sums of the fixed-point depth D, the pixel sums of the
// fixed-point terms -- is an INTEGER below 2^53 held in a double: additions are exact in any order or grouping, so chunked
// marches, wave-level scans and slab ranks all return the bits of the sequential loop, without atomics and without a tolerance.
//
// Two passes, each a prefix sum of D along an axis:
//   shadow pass  the exclusive prefix along the light -> s = att(prefix) into the shadow field
//   view pass    the exclusive prefix along the view  -> Tv = att(prefix), the terms, the two pixel sums; reads rho and shadow
// and two kernel forms for either:
//   *_march_kernel  axes y and z (the same kernel, the axis is a pair of strides): one thread per column, a wave reads 64
//                   consecutive x; blocks of 64 x 4 columns, chunks of the march along grid.z.  A chunk starts at the totals
//                   of the chunks before it (ray_totals_kernel ran first), and, where the march crosses slab ranks, at the
//                   totals of the ranks before it (gathered by one all-reduce).
//   *_x_kernel      axis x: a wave takes 64 consecutive x of one (j, k) row -- coalesced whatever the direction --, forms the
//                   exclusive prefix with a wave-level scan of doubles and carries the running total to the next 64.
// att() is one exp_portable, a chain of fp64 operations: it is evaluated only where the prefix is neither 0 (att = 1) nor
// opaque (att = 0), and the march keeps it in a register until the prefix changes.
// Everything is queued on the compute stream; nothing synchronises.
#include "bq_device.hip.h"
#include "bq_host.h"
#include "bq_launch_geom.h"
#include <algorithm>

namespace bq {

static constexpr double kTwo32 = 4294967296.0, kInvTwo32 = 1.0 / 4294967296.0, kOpaque = 128.0 * 4294967296.0;

// A family of rays along y or z as strides into the field.  Column (i, m), m < nm, has its cell t (in increasing coordinate)
// at base + i + m * sm + t * st; nt cells per ray.  x rows: row (j, kk), kk < nm, at base + ni * (j + nj * kk).
struct RayGeom {
    int ni, nm, nt;
    long long base, sm, st;
    int back;                   // the ray travels towards decreasing coordinates
    float sh, albedo, ambient;
};

__device__ __forceinline__ float render_depth(float rho, float sh)
{
    const float r = fmaxf(rho, 0.0f);
    return fminf(sh * r, 32.0f);
}
__device__ __forceinline__ double render_fix(float d) { return trunc((double)d * kTwo32); }
__device__ __forceinline__ float render_att(double A)
{
    if (A == 0.0) return 1.0f;                      // exp_portable(-0.0f) is 1.0f
    if (A >= kOpaque) return 0.0f;
    return exp_portable(-(float)(A * kInvTwo32));
}
// the fixed-point term of a cell with depth d != 0 behind the view transmittance Tv, lit by s
__device__ __forceinline__ double render_term(float d, float s, float Tv, float albedo, float ambient)
{
    const float a = 1.0f - exp_portable(-d);
    const float lit = albedo * s + ambient;
    const float q = a * lit;
    return trunc((double)Tv * (double)q * kTwo32);
}

// what the column starts chunk `b` at: the totals of the ranks [r0, r1) (gath: slots of gstride doubles; NULL: none) and of
// the chunks before b
__device__ __forceinline__ double ray_start(const double *__restrict__ tot, const double *__restrict__ gath, int r0, int r1,
                                            size_t gstride, size_t ncol, size_t col, int b)
{
    double A = 0.0;
    if (gath) for (int r = r0; r < r1; r++) A += gath[(size_t)r * gstride + col];
    for (int c = 0; c < b; c++) A += tot[(size_t)c * ncol + col];
    return A;
}

// ---- marches along y and z ---------------------------------------------------------------------------------------------
// tot[b ncol + col] = the sum of D over chunk b (cells [b kc, (b + 1) kc) in travel order) of column col = i + ni m
__global__ __launch_bounds__(256) void ray_totals_kernel(const float *__restrict__ rho, RayGeom g, int kc, double *__restrict__ tot)
{
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const long long step = g.back ? -g.st : g.st;
    const float *p = rho + g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    double sum = 0.0;
    int t = t0;
    for (; t + 4 <= t1; t += 4, p += 4 * step) {
        const float r0 = p[0], r1 = p[step], r2 = p[2 * step], r3 = p[3 * step];
        sum += (render_fix(render_depth(r0, g.sh)) + render_fix(render_depth(r1, g.sh))) +
               (render_fix(render_depth(r2, g.sh)) + render_fix(render_depth(r3, g.sh)));
    }
    for (; t < t1; t++, p += step) sum += render_fix(render_depth(*p, g.sh));
    tot[(size_t)blockIdx.z * ((size_t)g.ni * g.nm) + (size_t)i + (size_t)g.ni * m] = sum;
}

__global__ __launch_bounds__(256) void shadow_march_kernel(const float *__restrict__ rho, float *__restrict__ shadow, RayGeom g, int kc,
                                                           const double *__restrict__ tot, const double *__restrict__ gath,
                                                           int r0, int r1, size_t gstride)
{
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const size_t col = (size_t)i + (size_t)g.ni * m;
    double A = ray_start(tot, gath, r0, r1, gstride, (size_t)g.ni * g.nm, col, blockIdx.z);
    float s = render_att(A);
    const long long step = g.back ? -g.st : g.st;
    long long at = g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    int t = t0;
    for (; t + 4 <= t1; t += 4, at += 4 * step) {
        float r[4];
#pragma unroll
        for (int u = 0; u < 4; u++) r[u] = rho[at + u * step];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            shadow[at + u * step] = s;
            const double D = render_fix(render_depth(r[u], g.sh));
            if (D != 0.0) { A += D; s = render_att(A); }
        }
    }
    for (; t < t1; t++, at += step) {
        shadow[at] = s;
        const double D = render_fix(render_depth(rho[at], g.sh));
        if (D != 0.0) { A += D; s = render_att(A); }
    }
}

// One chunk per ray (gridDim.z == 1): the pixel sums go straight into img (npix doubles per plane, the column's pixel is
// pix0 + col).  Chunked: the chunk's sum of terms goes to cpart[b ncol + col], view_finish_kernel adds the chunks.
template <bool LIGHT>
__global__ __launch_bounds__(256) void view_march_kernel(const float *__restrict__ rho, const float *__restrict__ shadow, RayGeom g, int kc,
                                                         const double *__restrict__ tot, const double *__restrict__ gath,
                                                         int r0, int r1, size_t gstride, double *__restrict__ cpart,
                                                         double *__restrict__ img, size_t npix, size_t pix0)
{
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const size_t ncol = (size_t)g.ni * g.nm, col = (size_t)i + (size_t)g.ni * m;
    const double A0 = ray_start(tot, gath, r0, r1, gstride, ncol, col, blockIdx.z);
    double A = A0, C = 0.0;
    float Tv = render_att(A);
    const long long step = g.back ? -g.st : g.st;
    long long at = g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    int t = t0;
    for (; t + 4 <= t1; t += 4, at += 4 * step) {
        float r[4], s[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { r[u] = rho[at + u * step]; s[u] = LIGHT ? shadow[at + u * step] : 1.0f; }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const float d = render_depth(r[u], g.sh);
            const double D = render_fix(d);
            if (D != 0.0) {
                C += render_term(d, s[u], Tv, g.albedo, g.ambient);
                A += D;
                Tv = render_att(A);
            }
        }
    }
    for (; t < t1; t++, at += step) {
        const float d = render_depth(rho[at], g.sh);
        const double D = render_fix(d);
        if (D != 0.0) {
            C += render_term(d, LIGHT ? shadow[at] : 1.0f, Tv, g.albedo, g.ambient);
            A += D;
            Tv = render_att(A);
        }
    }
    if (gridDim.z == 1) { img[pix0 + col] = C; img[npix + pix0 + col] = A - A0; }
    else cpart[(size_t)blockIdx.z * ncol + col] = C;
}

// pixel of column col: Cfix = the chunks' sums of terms, Afix = the chunks' totals of D
__global__ __launch_bounds__(256) void view_finish_kernel(const double *__restrict__ cpart, const double *__restrict__ tot, int nch, size_t ncol,
                                                          double *__restrict__ img, size_t npix, size_t pix0)
{
    const size_t col = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    double C = 0.0, A = 0.0;
    for (int b = 0; b < nch; b++) { C += cpart[(size_t)b * ncol + col]; A += tot[(size_t)b * ncol + col]; }
    img[pix0 + col] = C;
    img[npix + pix0 + col] = A;
}

// ---- marches along x ---------------------------------------------------------------------------------------------------
// the inclusive prefix of v over the wave's 64 lanes (integers below 2^53: exact in any grouping)
__device__ __forceinline__ double wave_scan(double v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double n = __shfl_up(v, o, 64);
        if (lane >= o) v += n;
    }
    return v;
}

// a wave = threadIdx.y: row (j, kk) = (4 blockIdx.y + threadIdx.y, blockIdx.z).  A wave whose row lies outside the grid
// leaves as a whole; lanes beyond the row's end stay for the shuffles and bring D = 0.
__global__ __launch_bounds__(256) void shadow_x_kernel(const float *__restrict__ rho, float *__restrict__ shadow, RayGeom g, int nj)
{
    const int lane = threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (j >= nj) return;
    const long long row = g.base + (long long)g.ni * (j + (long long)nj * blockIdx.z);
    double carry = 0.0;
    for (int t = lane; t - lane < g.ni; t += 64) {
        const bool in = t < g.ni;
        const long long at = row + (g.back ? g.ni - 1 - t : t);
        const double D = in ? render_fix(render_depth(rho[at], g.sh)) : 0.0;
        double A = carry;
        if (__any(D != 0.0)) {
            const double inc = wave_scan(D, lane);
            A = carry + (inc - D);
            carry += __shfl(inc, 63, 64);
        }
        if (in) shadow[at] = render_att(A);
    }
}

// pixel pix0 + j + nj kk of the row (j, kk): lane 0 leaves both sums
template <bool LIGHT>
__global__ __launch_bounds__(256) void view_x_kernel(const float *__restrict__ rho, const float *__restrict__ shadow, RayGeom g, int nj,
                                                     double *__restrict__ img, size_t npix, size_t pix0)
{
    const int lane = threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (j >= nj) return;
    const long long row = g.base + (long long)g.ni * (j + (long long)nj * blockIdx.z);
    double carry = 0.0, C = 0.0;
    for (int t = lane; t - lane < g.ni; t += 64) {
        const bool in = t < g.ni;
        const long long at = row + (g.back ? g.ni - 1 - t : t);
        const float d = in ? render_depth(rho[at], g.sh) : 0.0f;
        const double D = render_fix(d);
        if (__any(D != 0.0)) {
            const double inc = wave_scan(D, lane);
            if (D != 0.0) C += render_term(d, LIGHT ? shadow[at] : 1.0f, render_att(carry + (inc - D)), g.albedo, g.ambient);
            carry += __shfl(inc, 63, 64);
        }
    }
    C = wave_sum(C);
    if (lane == 0) {
        const size_t pix = pix0 + (size_t)j + (size_t)nj * blockIdx.z;
        img[pix] = C;
        img[npix + pix] = carry;
    }
}

// [a, a + na) and [b, b + nb) bytes share a byte
static bool render_overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// chunk length of a march of nt cells by row_blocks blocks of columns: the forced one; one chunk when asked for (forced < 0),
// or when the rule's chunk would be the whole ray; else whole rounds of two blocks per CU with about 32 cells per chunk
// (bq_launch_geom.h) and no chunk below 8 cells
static int render_chunk(int row_blocks, int nt, int forced)
{
    if (nt <= 1 || forced < 0) return std::max(nt, 1);
    if (forced > 0) return std::min(forced, nt);
    const int nchunks = geom::whole_round_chunks(row_blocks, nt, 32, 512);
    return std::min(nt, std::max((nt + nchunks - 1) / nchunks, 8));
}

// one pass (shadow: img == NULL; view: shadow_out == NULL) along direction dir
struct RenderPass {
    bool x;                     // the wave-scan form
    RayGeom g;
    int kc, nch, gx, gy;        // march: chunk length and count, blocks of columns
    size_t ncol;
    double *tot = nullptr;      // chunk totals (nch > 1)
};

} // namespace bq

using namespace bq;

extern "C" int gpu_render_density(const float *rho, float *shadow, float h, int ni, int nj, int nk, int view, int light,
                                  const fl_render_params *p, double *d_image)
{
    static const char *op = "gpu_render_density";
    if (!ensure_ready(op)) return fl_last_error();
    const int before = fl_last_error();
    auto refuse = [&](const char *why) { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; };
    if (!rho || !p || !d_image) return refuse("null rho, p or d_image");
    if (view < 0 || view > 5) return refuse("view outside 0..5");
    if (light < -1 || light > 5) return refuse("light outside -1..5");
    if (light >= 0 && !shadow) return refuse("a light needs the shadow field");
    if (ni < 1 || nj < 1 || nk < 1 || ni > 65534 || nj > 65534 || nk > 65534) return refuse("dims outside 1..65534");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("plane of 2^23 elements or more");
    if (!(h > 0.0f) || std::isinf(h)) return refuse("h must be positive and finite");
    if (!(p->sigma >= 0.0f) || std::isinf(p->sigma) || !(p->albedo >= 0.0f) || std::isinf(p->albedo) ||
        !(p->ambient >= 0.0f) || std::isinf(p->ambient))
        return refuse("sigma, albedo and ambient must be finite and >= 0");
    if (p->albedo + p->ambient > 4.0f) return refuse("albedo + ambient > 4");
    const Runtime &r = rt();
    int koff, nkg;
    slab_ctx(nk, koff, nkg);
    const int vaxis = view / 2, laxis = light >= 0 ? light / 2 : -1;
    const int W = vaxis == 0 ? nj : ni, H = vaxis == 2 ? nj : nkg;
    const size_t nc = (size_t)ni * nj * nk, npix = (size_t)W * H, plane = (size_t)ni * nj;
    if (render_overlaps(d_image, 2 * npix * sizeof(double), rho, nc * sizeof(float)) ||
        render_overlaps(shadow, nc * sizeof(float), rho, nc * sizeof(float)) ||
        render_overlaps(shadow, nc * sizeof(float), d_image, 2 * npix * sizeof(double)))
        return refuse("d_image or shadow overlaps rho");
    // the local planes that count: the ones this rank owns
    int p0 = r.slab_on ? std::max(0, r.slab_own0 - r.slab_koff) : 0;
    int p1 = r.slab_on ? std::min(nk, r.slab_own1 - r.slab_koff) : nk;
    if (p1 < p0) p1 = p0;
    const int np = p1 - p0;
    const int ranks = r.slab_on ? comm_ranks() : 1, rank = ranks > 1 ? fl_comm_rank() : 0;
    const bool gather = ranks > 1 && (vaxis == 2 || laxis == 2);
    const int forced = r.opt_render_kchunk;
    hipStream_t st = r.compute;

    auto plan = [&](int dir) {
        RenderPass ps;
        const int axis = dir / 2;
        ps.x = axis == 0;
        RayGeom &g = ps.g;
        g.ni = ni; g.back = dir & 1; g.sh = p->sigma * h; g.albedo = p->albedo; g.ambient = p->ambient;
        g.base = (long long)plane * p0;
        if (axis == 2)      { g.nm = nj; g.nt = np; g.sm = ni; g.st = (long long)plane; }
        else if (axis == 1) { g.nm = np; g.nt = nj; g.sm = (long long)plane; g.st = ni; }
        else                { g.nm = np; g.nt = ni; g.sm = 0; g.st = 1; }
        ps.gx = (ni + 63) / 64; ps.gy = (g.nm + 3) / 4;
        ps.ncol = (size_t)ni * g.nm;
        ps.kc = ps.x ? ni : render_chunk(ps.gx * ps.gy, g.nt, forced);
        ps.nch = ps.x ? 1 : std::max(1, (g.nt + ps.kc - 1) / ps.kc);
        return ps;
    };
    RenderPass L = plan(light >= 0 ? light : 0), V = plan(view);
    const bool lit = light >= 0;
    // one workspace: the gather slots, the chunk totals of either pass, the view pass's chunk sums
    const size_t n_gath = gather ? (size_t)ranks * plane : 0;
    const size_t n_totL = lit && L.nch > 1 ? (size_t)L.nch * L.ncol : 0, n_totV = V.nch > 1 ? (size_t)V.nch * V.ncol : 0;
    double *ws = nullptr;
    if (n_gath + n_totL + 2 * n_totV) {
        ws = (double *)scratch((n_gath + n_totL + 2 * n_totV) * sizeof(double));
        if (!ws) return fl_last_error();
    }
    double *gath = gather ? ws : nullptr;
    L.tot = n_totL ? ws + n_gath : nullptr;
    V.tot = n_totV ? ws + n_gath + n_totL : nullptr;
    double *cpart = n_totV ? ws + n_gath + n_totL + n_totV : nullptr;

    if (gather) {               // every rank's column totals of D over its owned planes, in every rank's hands
        if (!BQ_HIP(hipMemsetAsync(gath, 0, n_gath * sizeof(double), st))) return fl_last_error();
        if (np > 0) {
            RenderPass Z = plan(4);
            ray_totals_kernel<<<dim3(Z.gx, Z.gy, 1), kBlock, 0, st>>>(rho, Z.g, np, gath + (size_t)rank * plane);
            BQ_LAUNCH_CHECK("ray_totals_kernel");
        }
        if (!comm_allreduce(gath, n_gath, true, false, st)) return fl_last_error();
    }
    // the ranks whose totals a march along z starts at: the ones before this rank, after it for -z
    auto ranks_before = [&](int dir, int &r0, int &r1, const double *&gp) {
        gp = (gather && dir / 2 == 2) ? gath : nullptr;
        r0 = (dir & 1) ? rank + 1 : 0;
        r1 = (dir & 1) ? ranks : rank;
    };
    auto totals = [&](const RenderPass &ps) {
        if (ps.nch <= 1 || ps.ncol == 0) return;
        ray_totals_kernel<<<dim3(ps.gx, ps.gy, ps.nch), kBlock, 0, st>>>(rho, ps.g, ps.kc, ps.tot);
        BQ_LAUNCH_CHECK("ray_totals_kernel");
    };

    if (lit && np > 0) {        // ---- shadow pass
        if (L.x) {
            shadow_x_kernel<<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, L.g, nj);
            BQ_LAUNCH_CHECK("shadow_x_kernel");
        } else {
            int r0, r1; const double *gp;
            ranks_before(light, r0, r1, gp);
            totals(L);
            shadow_march_kernel<<<dim3(L.gx, L.gy, L.nch), kBlock, 0, st>>>(rho, shadow, L.g, L.kc, L.tot, gp, r0, r1, plane);
            BQ_LAUNCH_CHECK("shadow_march_kernel");
        }
    }
    // ---- view pass: a rank writes the pixels of its owned planes -- all of them when the view runs along z
    const size_t pix0 = vaxis == 2 ? 0 : (size_t)W * (size_t)(p0 + koff);
    if (vaxis == 2 ? np == 0 : np != nkg)
        if (!BQ_HIP(hipMemsetAsync(d_image, 0, 2 * npix * sizeof(double), st))) return fl_last_error();
    if (np > 0) {
        if (V.x) {
            if (lit) view_x_kernel<true><<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, pix0);
            else     view_x_kernel<false><<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, pix0);
            BQ_LAUNCH_CHECK("view_x_kernel");
        } else {
            int r0, r1; const double *gp;
            ranks_before(view, r0, r1, gp);
            totals(V);
            const dim3 grid(V.gx, V.gy, V.nch);
            if (lit) view_march_kernel<true><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, gp, r0, r1, plane, cpart, d_image, npix, pix0);
            else     view_march_kernel<false><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, gp, r0, r1, plane, cpart, d_image, npix, pix0);
            BQ_LAUNCH_CHECK("view_march_kernel");
            if (V.nch > 1) {
                view_finish_kernel<<<(unsigned)((V.ncol + 255) / 256), 256, 0, st>>>(cpart, V.tot, V.nch, V.ncol, d_image, npix, pix0);
                BQ_LAUNCH_CHECK("view_finish_kernel");
            }
        }
    }
    if (ranks > 1) comm_allreduce(d_image, 2 * npix, true, false, st);      // owned pixels and partial sums -> the whole image
    return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
}
