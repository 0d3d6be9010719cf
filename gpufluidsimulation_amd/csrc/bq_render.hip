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

// ---- solid obstacles (gpu_render_density_solids) ---------------------------------------------------
// Every kernel below is a template on SOLID; the kernels of gpu_render_density are its SOLID = false instantiations with
// their own argument lists, the SOLID = true ones take one SolidIn more.  A solid cell (tag = flag & 0x7f != 0) has D = 0
// whatever rho holds, blocks everything behind it on its ray (B, the exclusive OR-prefix of "solid") and, on a view ray, is
// drawn once: the first solid's term and tag.  Both B and the first tag combine associatively, so the totals pass leaves
// each chunk's first tag next to its sum of D and a later chunk starts at the OR of the chunks before it.
struct SolidIn {
    const unsigned char *flag;  // the cell flags
    unsigned char *ctag;        // ctag[b ncol + col]: the first non-zero tag of chunk b in travel order, 0: none (nch > 1)
    float albedo, ambient;      // of the solids
    const unsigned char *rows;  // the rows summary or NULL: byte j + nj k == 0, row (j, k) holds no solid (the x kernels skip its flag loads)
};
// the kernels' optional last argument: none (gpu_render_density's instantiations keep their argument lists) or one SolidIn
__device__ __forceinline__ SolidIn solid_in() { return SolidIn{ nullptr, nullptr, 0.0f, 0.0f, nullptr }; }
__device__ __forceinline__ SolidIn solid_in(SolidIn si) { return si; }

template <bool SOLID> __device__ __forceinline__ unsigned solid_tag(const unsigned char *flag, long long at)
{
    if constexpr (SOLID) return flag[at] & 0x7fu;
    else return 0u;
}
// D of a cell with tag f
template <bool SOLID> __device__ __forceinline__ double cell_fix(float rho, unsigned f, float sh)
{
    if constexpr (SOLID) { if (f) return 0.0; }
    return render_fix(render_depth(rho, sh));
}
// the fixed-point term of the first solid cell of a view ray behind the view transmittance Tv, lit by s
__device__ __forceinline__ double render_solid_term(float s, float Tv, float albedo, float ambient)
{
    const float lit = albedo * s;
    const float qs = lit + ambient;
    return trunc((double)Tv * (double)qs * kTwo32);
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
// and whether a chunk before b holds a solid cell
__device__ __forceinline__ bool ray_blocked(const unsigned char *__restrict__ ctag, size_t ncol, size_t col, int b)
{
    unsigned any = 0;
    for (int c = 0; c < b; c++) any |= ctag[(size_t)c * ncol + col];
    return any != 0;
}

// ---- marches along y and z ---------------------------------------------------------------------------------------------
// tot[b ncol + col] = the sum of D over chunk b (cells [b kc, (b + 1) kc) in travel order) of column col = i + ni m
template <bool SOLID, class... S>
__global__ __launch_bounds__(256) void ray_totals_kernel(const float *__restrict__ rho, RayGeom g, int kc, double *__restrict__ tot, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const long long step = g.back ? -g.st : g.st;
    const float *p = rho + g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    const unsigned char *q = SOLID ? si.flag + (p - rho) : nullptr;
    double sum = 0.0;
    unsigned tag = 0;
    int t = t0;
    for (; t + 4 <= t1; t += 4, p += 4 * step) {
        const float r0 = p[0], r1 = p[step], r2 = p[2 * step], r3 = p[3 * step];
        const unsigned f0 = solid_tag<SOLID>(q, 0), f1 = solid_tag<SOLID>(q, step), f2 = solid_tag<SOLID>(q, 2 * step),
                       f3 = solid_tag<SOLID>(q, 3 * step);
        sum += (cell_fix<SOLID>(r0, f0, g.sh) + cell_fix<SOLID>(r1, f1, g.sh)) +
               (cell_fix<SOLID>(r2, f2, g.sh) + cell_fix<SOLID>(r3, f3, g.sh));
        if constexpr (SOLID) {
            if (!tag) tag = f0 ? f0 : f1 ? f1 : f2 ? f2 : f3;
            q += 4 * step;
        }
    }
    for (; t < t1; t++, p += step) {
        const unsigned f = solid_tag<SOLID>(q, 0);
        sum += cell_fix<SOLID>(*p, f, g.sh);
        if constexpr (SOLID) {
            if (!tag) tag = f;
            q += step;
        }
    }
    const size_t slot = (size_t)blockIdx.z * ((size_t)g.ni * g.nm) + (size_t)i + (size_t)g.ni * m;
    tot[slot] = sum;
    if constexpr (SOLID) si.ctag[slot] = (unsigned char)tag;
}

template <bool SOLID, class... S>
__global__ __launch_bounds__(256) void shadow_march_kernel(const float *__restrict__ rho, float *__restrict__ shadow, RayGeom g, int kc,
                                                           const double *__restrict__ tot, const double *__restrict__ gath,
                                                           int r0, int r1, size_t gstride, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const size_t col = (size_t)i + (size_t)g.ni * m;
    double A = ray_start(tot, gath, r0, r1, gstride, (size_t)g.ni * g.nm, col, blockIdx.z);
    float s = render_att(A);
    bool B = false;             // a solid cell lies before this one
    if constexpr (SOLID) {
        B = ray_blocked(si.ctag, (size_t)g.ni * g.nm, col, blockIdx.z);
        if (B) s = 0.0f;
    }
    const long long step = g.back ? -g.st : g.st;
    long long at = g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    int t = t0;
    for (; t + 4 <= t1; t += 4, at += 4 * step) {
        float r[4];
        unsigned f[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { r[u] = rho[at + u * step]; f[u] = solid_tag<SOLID>(si.flag, at + u * step); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            shadow[at + u * step] = s;
            if constexpr (SOLID) { if (f[u]) { B = true; s = 0.0f; continue; } }
            const double D = render_fix(render_depth(r[u], g.sh));
            if (D != 0.0) { A += D; if (!SOLID || !B) s = render_att(A); }
        }
    }
    for (; t < t1; t++, at += step) {
        shadow[at] = s;
        if constexpr (SOLID) { if (solid_tag<SOLID>(si.flag, at)) { B = true; s = 0.0f; continue; } }
        const double D = render_fix(render_depth(rho[at], g.sh));
        if (D != 0.0) { A += D; if (!SOLID || !B) s = render_att(A); }
    }
}

// One chunk per ray (gridDim.z == 1): the pixel sums go straight into img (npix doubles per plane, the column's pixel is
// pix0 + col).  Chunked: the chunk's sum of terms goes to cpart[b ncol + col], view_finish_kernel adds the chunks.
template <bool LIGHT, bool SOLID, class... S>
__global__ __launch_bounds__(256) void view_march_kernel(const float *__restrict__ rho, const float *__restrict__ shadow, RayGeom g, int kc,
                                                         const double *__restrict__ tot, const double *__restrict__ gath,
                                                         int r0, int r1, size_t gstride, double *__restrict__ cpart,
                                                         double *__restrict__ img, size_t npix, size_t pix0, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const int i = blockIdx.x * 64 + threadIdx.x, m = blockIdx.y * 4 + threadIdx.y;
    if (i >= g.ni || m >= g.nm) return;
    const int t0 = blockIdx.z * kc, t1 = min(t0 + kc, g.nt);
    const size_t ncol = (size_t)g.ni * g.nm, col = (size_t)i + (size_t)g.ni * m;
    const double A0 = ray_start(tot, gath, r0, r1, gstride, ncol, col, blockIdx.z);
    double A = A0, C = 0.0;
    float Tv = render_att(A);
    bool B = false;             // a solid cell lies before this one: nothing behind it is seen
    unsigned hit = 0;
    if constexpr (SOLID) {
        B = ray_blocked(si.ctag, ncol, col, blockIdx.z);
        if (B) Tv = 0.0f;
    }
    const long long step = g.back ? -g.st : g.st;
    long long at = g.base + i + m * g.sm + (long long)(g.back ? g.nt - 1 - t0 : t0) * g.st;
    int t = t0;
    for (; t + 4 <= t1; t += 4, at += 4 * step) {
        float r[4], s[4];
        unsigned f[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            r[u] = rho[at + u * step]; s[u] = LIGHT ? shadow[at + u * step] : 1.0f;
            f[u] = solid_tag<SOLID>(si.flag, at + u * step);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if constexpr (SOLID) {
                if (f[u]) {
                    if (!B) { C += render_solid_term(s[u], Tv, si.albedo, si.ambient); hit = f[u]; B = true; Tv = 0.0f; }
                    continue;
                }
            }
            const float d = render_depth(r[u], g.sh);
            const double D = render_fix(d);
            if (D != 0.0) {
                if (!SOLID || !B) C += render_term(d, s[u], Tv, g.albedo, g.ambient);
                A += D;
                if (!SOLID || !B) Tv = render_att(A);
            }
        }
    }
    for (; t < t1; t++, at += step) {
        if constexpr (SOLID) {
            const unsigned f = solid_tag<SOLID>(si.flag, at);
            if (f) {
                if (!B) { C += render_solid_term(LIGHT ? shadow[at] : 1.0f, Tv, si.albedo, si.ambient); hit = f; B = true; Tv = 0.0f; }
                continue;
            }
        }
        const float d = render_depth(rho[at], g.sh);
        const double D = render_fix(d);
        if (D != 0.0) {
            if (!SOLID || !B) C += render_term(d, LIGHT ? shadow[at] : 1.0f, Tv, g.albedo, g.ambient);
            A += D;
            if (!SOLID || !B) Tv = render_att(A);
        }
    }
    if (gridDim.z == 1) {
        img[pix0 + col] = C; img[npix + pix0 + col] = A - A0;
        if constexpr (SOLID) img[2 * npix + pix0 + col] = (double)hit;
    }
    else cpart[(size_t)blockIdx.z * ncol + col] = C;
}

// pixel of column col: Cfix = the chunks' sums of terms, Afix = the chunks' totals of D, Hfix = the chunks' first tag
template <bool SOLID, class... S>
__global__ __launch_bounds__(256) void view_finish_kernel(const double *__restrict__ cpart, const double *__restrict__ tot, int nch, size_t ncol,
                                                          double *__restrict__ img, size_t npix, size_t pix0, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const size_t col = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    double C = 0.0, A = 0.0;
    for (int b = 0; b < nch; b++) { C += cpart[(size_t)b * ncol + col]; A += tot[(size_t)b * ncol + col]; }
    img[pix0 + col] = C;
    img[npix + pix0 + col] = A;
    if constexpr (SOLID) {
        unsigned hit = 0;
        for (int b = 0; b < nch; b++) {
            const unsigned f = si.ctag[(size_t)b * ncol + col];
            if (!hit) hit = f;
        }
        img[2 * npix + pix0 + col] = (double)hit;
    }
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
// SOLID: B of a lane = a solid among the lanes before it in this segment (a ballot masked to them) or in an earlier segment
// (the carried flag).
template <bool SOLID, class... S>
__global__ __launch_bounds__(256) void shadow_x_kernel(const float *__restrict__ rho, float *__restrict__ shadow, RayGeom g, int nj, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const int lane = threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (j >= nj) return;
    const long long row = g.base + (long long)g.ni * (j + (long long)nj * blockIdx.z);
    double carry = 0.0;
    bool cB = false;
    bool flagged = SOLID;       // wave-uniform: the row may hold a solid cell, its flags are read
    if constexpr (SOLID) { if (si.rows) flagged = si.rows[(size_t)j + (size_t)nj * blockIdx.z] != 0; }
    for (int t = lane; t - lane < g.ni; t += 64) {
        const bool in = t < g.ni;
        const long long at = row + (g.back ? g.ni - 1 - t : t);
        unsigned f = 0;
        if constexpr (SOLID) f = (flagged && in) ? solid_tag<SOLID>(si.flag, at) : 0u;         // issued next to the rho load
        const double D = in ? cell_fix<SOLID>(rho[at], f, g.sh) : 0.0;
        double A = carry;
        if (__any(D != 0.0)) {
            const double inc = wave_scan(D, lane);
            A = carry + (inc - D);
            carry += __shfl(inc, 63, 64);
        }
        if constexpr (SOLID) {
            const unsigned long long sm = __ballot(f != 0);
            const bool B = cB || (sm & ((1ull << lane) - 1ull)) != 0;
            if (in) shadow[at] = B ? 0.0f : render_att(A);
            cB = cB || sm != 0;
        } else {
            if (in) shadow[at] = render_att(A);
        }
    }
}

// pixel pix0 + j + nj kk of the row (j, kk): lane 0 leaves the sums
template <bool LIGHT, bool SOLID, class... S>
__global__ __launch_bounds__(256) void view_x_kernel(const float *__restrict__ rho, const float *__restrict__ shadow, RayGeom g, int nj,
                                                     double *__restrict__ img, size_t npix, size_t pix0, S... sx)
{
    const SolidIn si = solid_in(sx...);
    const int lane = threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (j >= nj) return;
    const long long row = g.base + (long long)g.ni * (j + (long long)nj * blockIdx.z);
    double carry = 0.0, C = 0.0;
    bool cB = false;
    int hit = 0;                // wave-uniform: the tag of the ray's first solid cell
    bool flagged = SOLID;       // wave-uniform: the row may hold a solid cell, its flags are read
    if constexpr (SOLID) { if (si.rows) flagged = si.rows[(size_t)j + (size_t)nj * blockIdx.z] != 0; }
    for (int t = lane; t - lane < g.ni; t += 64) {
        const bool in = t < g.ni;
        const long long at = row + (g.back ? g.ni - 1 - t : t);
        unsigned f = 0;
        if constexpr (SOLID) f = (flagged && in) ? solid_tag<SOLID>(si.flag, at) : 0u;         // issued next to the rho load
        float d = in ? render_depth(rho[at], g.sh) : 0.0f;
        if constexpr (SOLID) { if (f) d = 0.0f; }
        const double D = render_fix(d);
        if constexpr (!SOLID) {
            if (__any(D != 0.0)) {
                const double inc = wave_scan(D, lane);
                if (D != 0.0) C += render_term(d, LIGHT ? shadow[at] : 1.0f, render_att(carry + (inc - D)), g.albedo, g.ambient);
                carry += __shfl(inc, 63, 64);
            }
        } else {
            // a segment of solid cells alone has D == 0 everywhere and is still drawn
            const unsigned long long sm = __ballot(f != 0);
            const bool any = __any(D != 0.0);
            if (any || (sm != 0 && !cB)) {
                const double inc = any ? wave_scan(D, lane) : 0.0;
                const bool B = cB || (sm & ((1ull << lane) - 1ull)) != 0;
                if (!B && (D != 0.0 || f)) {
                    const float Tv = render_att(carry + (inc - D)), s = LIGHT ? shadow[at] : 1.0f;
                    C += f ? render_solid_term(s, Tv, si.albedo, si.ambient) : render_term(d, s, Tv, g.albedo, g.ambient);
                }
                if (any) carry += __shfl(inc, 63, 64);
                if (!cB && sm != 0) { hit = __shfl((int)f, __ffsll((unsigned long long)sm) - 1, 64); cB = true; }
            }
        }
    }
    C = wave_sum(C);
    if (lane == 0) {
        const size_t pix = pix0 + (size_t)j + (size_t)nj * blockIdx.z;
        img[pix] = C;
        img[npix + pix] = carry;
        if constexpr (SOLID) img[2 * npix + pix] = (double)hit;
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
    unsigned char *ctag = nullptr;  // chunk tags (nch > 1, with solids)
};

} // namespace bq

using namespace bq;

// gpu_render_density (solid == NULL: its launches, as they were) and gpu_render_density_solids
static int render_run(const char *op, const float *rho, const unsigned char *solid, const unsigned char *rows, float *shadow, float h,
                      int ni, int nj, int nk, int view, int light, const fl_render_params *p, const fl_render_solid_params *sp,
                      bool solids, double *d_image)
{
    if (!ensure_ready(op)) return fl_last_error();
    const int before = fl_last_error();
    auto refuse = [&](const char *why) { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; };
    if (!rho || !p || !d_image) return refuse("null rho, p or d_image");
    if (solids && (!solid || !sp)) return refuse("null solid or sp");
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
    if (solids) {
        if (!(sp->albedo >= 0.0f) || std::isinf(sp->albedo) || !(sp->ambient >= 0.0f) || std::isinf(sp->ambient))
            return refuse("the solids' albedo and ambient must be finite and >= 0");
        if (sp->albedo + sp->ambient > 4.0f) return refuse("the solids' albedo + ambient > 4");
    }
    const Runtime &r = rt();
    int koff, nkg;
    slab_ctx(nk, koff, nkg);
    const int vaxis = view / 2, laxis = light >= 0 ? light / 2 : -1;
    const int W = vaxis == 0 ? nj : ni, H = vaxis == 2 ? nj : nkg;
    const size_t nc = (size_t)ni * nj * nk, npix = (size_t)W * H, plane = (size_t)ni * nj;
    const size_t nimg = (solids ? 3 : 2) * npix * sizeof(double);
    if (render_overlaps(d_image, nimg, rho, nc * sizeof(float)) ||
        render_overlaps(shadow, nc * sizeof(float), rho, nc * sizeof(float)) ||
        render_overlaps(shadow, nc * sizeof(float), d_image, nimg))
        return refuse("d_image or shadow overlaps rho");
    if (solids) {
        if (render_overlaps(solid, nc, shadow, nc * sizeof(float)) || render_overlaps(solid, nc, d_image, nimg) ||
            render_overlaps(rows, (size_t)nj * nk, shadow, nc * sizeof(float)) || render_overlaps(rows, (size_t)nj * nk, d_image, nimg))
            return refuse("solid or rows overlaps shadow or d_image");
        if (r.slab_on) {
            latch(FL_ERR_UNSUPPORTED, op, "not supported under a z-slab context");
            return (int)FL_ERR_UNSUPPORTED;
        }
    }
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
    // one workspace: the gather slots, the chunk totals of either pass, the view pass's chunk sums; solids: the chunk tags of
    // either pass (bytes) behind the doubles
    const size_t n_gath = gather ? (size_t)ranks * plane : 0;
    const size_t n_totL = lit && L.nch > 1 ? (size_t)L.nch * L.ncol : 0, n_totV = V.nch > 1 ? (size_t)V.nch * V.ncol : 0;
    const size_t n_dbl = n_gath + n_totL + 2 * n_totV, n_tag = solids ? n_totL + n_totV : 0;
    double *ws = nullptr;
    if (n_dbl) {
        ws = (double *)scratch(n_dbl * sizeof(double) + n_tag);
        if (!ws) return fl_last_error();
    }
    double *gath = gather ? ws : nullptr;
    L.tot = n_totL ? ws + n_gath : nullptr;
    V.tot = n_totV ? ws + n_gath + n_totL : nullptr;
    double *cpart = n_totV ? ws + n_gath + n_totL + n_totV : nullptr;
    if (n_tag) {
        unsigned char *tags = (unsigned char *)(ws + n_dbl);
        L.ctag = n_totL ? tags : nullptr;
        V.ctag = n_totV ? tags + n_totL : nullptr;
    }

    if (gather) {               // every rank's column totals of D over its owned planes, in every rank's hands
        if (!BQ_HIP(hipMemsetAsync(gath, 0, n_gath * sizeof(double), st))) return fl_last_error();
        if (np > 0) {
            RenderPass Z = plan(4);
            ray_totals_kernel<false><<<dim3(Z.gx, Z.gy, 1), kBlock, 0, st>>>(rho, Z.g, np, gath + (size_t)rank * plane);
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
        if (solids) ray_totals_kernel<true><<<dim3(ps.gx, ps.gy, ps.nch), kBlock, 0, st>>>(rho, ps.g, ps.kc, ps.tot, SolidIn{ solid, ps.ctag, 0.0f, 0.0f, nullptr });
        else        ray_totals_kernel<false><<<dim3(ps.gx, ps.gy, ps.nch), kBlock, 0, st>>>(rho, ps.g, ps.kc, ps.tot);
        BQ_LAUNCH_CHECK("ray_totals_kernel");
    };

    if (solids) {               // ---- with solid obstacles: one rank, every plane, three image planes
        const SolidIn si = { solid, V.ctag, sp->albedo, sp->ambient, rows }, sl = { solid, L.ctag, 0.0f, 0.0f, rows };
        const dim3 xgrid(1, (nj + 3) / 4, np);
        if (lit) {
            if (L.x) {
                shadow_x_kernel<true><<<xgrid, kBlock, 0, st>>>(rho, shadow, L.g, nj, sl);
                BQ_LAUNCH_CHECK("shadow_x_kernel");
            } else {
                totals(L);
                shadow_march_kernel<true><<<dim3(L.gx, L.gy, L.nch), kBlock, 0, st>>>(rho, shadow, L.g, L.kc, L.tot, nullptr, 0, 0, (size_t)0, sl);
                BQ_LAUNCH_CHECK("shadow_march_kernel");
            }
        }
        if (V.x) {
            if (lit) view_x_kernel<true, true><<<xgrid, kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, (size_t)0, si);
            else     view_x_kernel<false, true><<<xgrid, kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, (size_t)0, si);
            BQ_LAUNCH_CHECK("view_x_kernel");
        } else {
            totals(V);
            const dim3 grid(V.gx, V.gy, V.nch);
            if (lit) view_march_kernel<true, true><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, nullptr, 0, 0, (size_t)0, cpart, d_image, npix, (size_t)0, si);
            else     view_march_kernel<false, true><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, nullptr, 0, 0, (size_t)0, cpart, d_image, npix, (size_t)0, si);
            BQ_LAUNCH_CHECK("view_march_kernel");
            if (V.nch > 1) {
                view_finish_kernel<true><<<(unsigned)((V.ncol + 255) / 256), 256, 0, st>>>(cpart, V.tot, V.nch, V.ncol, d_image, npix, (size_t)0, si);
                BQ_LAUNCH_CHECK("view_finish_kernel");
            }
        }
        return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
    }

    if (lit && np > 0) {        // ---- shadow pass
        if (L.x) {
            shadow_x_kernel<false><<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, L.g, nj);
            BQ_LAUNCH_CHECK("shadow_x_kernel");
        } else {
            int r0, r1; const double *gp;
            ranks_before(light, r0, r1, gp);
            totals(L);
            shadow_march_kernel<false><<<dim3(L.gx, L.gy, L.nch), kBlock, 0, st>>>(rho, shadow, L.g, L.kc, L.tot, gp, r0, r1, plane);
            BQ_LAUNCH_CHECK("shadow_march_kernel");
        }
    }
    // ---- view pass: a rank writes the pixels of its owned planes -- all of them when the view runs along z
    const size_t pix0 = vaxis == 2 ? 0 : (size_t)W * (size_t)(p0 + koff);
    if (vaxis == 2 ? np == 0 : np != nkg)
        if (!BQ_HIP(hipMemsetAsync(d_image, 0, 2 * npix * sizeof(double), st))) return fl_last_error();
    if (np > 0) {
        if (V.x) {
            if (lit) view_x_kernel<true, false><<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, pix0);
            else     view_x_kernel<false, false><<<dim3(1, (nj + 3) / 4, np), kBlock, 0, st>>>(rho, shadow, V.g, nj, d_image, npix, pix0);
            BQ_LAUNCH_CHECK("view_x_kernel");
        } else {
            int r0, r1; const double *gp;
            ranks_before(view, r0, r1, gp);
            totals(V);
            const dim3 grid(V.gx, V.gy, V.nch);
            if (lit) view_march_kernel<true, false><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, gp, r0, r1, plane, cpart, d_image, npix, pix0);
            else     view_march_kernel<false, false><<<grid, kBlock, 0, st>>>(rho, shadow, V.g, V.kc, V.tot, gp, r0, r1, plane, cpart, d_image, npix, pix0);
            BQ_LAUNCH_CHECK("view_march_kernel");
            if (V.nch > 1) {
                view_finish_kernel<false><<<(unsigned)((V.ncol + 255) / 256), 256, 0, st>>>(cpart, V.tot, V.nch, V.ncol, d_image, npix, pix0);
                BQ_LAUNCH_CHECK("view_finish_kernel");
            }
        }
    }
    if (ranks > 1) comm_allreduce(d_image, 2 * npix, true, false, st);      // owned pixels and partial sums -> the whole image
    return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
}

extern "C" int gpu_render_density(const float *rho, float *shadow, float h, int ni, int nj, int nk, int view, int light,
                                  const fl_render_params *p, double *d_image)
{
    return render_run("gpu_render_density", rho, nullptr, nullptr, shadow, h, ni, nj, nk, view, light, p, nullptr, false, d_image);
}

extern "C" int gpu_render_density_solids(const float *rho, const unsigned char *solid, const unsigned char *rows, float *shadow, float h,
                                         int ni, int nj, int nk, int view, int light, const fl_render_params *p,
                                         const fl_render_solid_params *sp, double *d_image)
{
    return render_run("gpu_render_density_solids", rho, solid, rows, shadow, h, ni, nj, nk, view, light, p, sp, true, d_image);
}
