// bq_tracers.hip -- passive tracer particles (the contract is in include/bimocq_gpu.h).
//
//   gpu_trace_particles   trace() of bq_device.hip.h per particle: one lane per particle, blocks of 256.  It is the body of
//                         forward_kernel (bq_advect.hip) over a list instead of a node lattice, so a tracer that starts on a
//                         grid node stays, bit for bit, where the forward map says that node went.
//   gpu_sample_particles  sample() of a field at every particle
//   gpu_seed_particles    jittered positions from a counter-based integer hash (written out in the header); no state
//   gpu_sort_particles    counting sort by 4 x 4 x 4-cell brick: once the flow has mixed the particles, neighbouring lanes of
//                         the trace touch unrelated cache lines; sorted, a wave's 24 taps per stage fall into a few bricks again
//
// The two kernels that interpolate exist twice, like the gather kernels of bq_advect.hip: this file is compiled once as
// is (exact arithmetic, the entry points) and once with -DBQ_FAST_LERP (only the launchers of namespace bq::fast); the
// entry points pick by FL_OPT_FAST_LERP.
#include "bq_device.hip.h"
#include "bq_host.h"
#include <algorithm>

namespace bq {
inline namespace BQ_VARIANT {

// Tail lanes return before trace(): the per-wave votes of get_velocity_auto count active lanes only.  The sub-step loop
// of trace() depends on cfldt and dt alone, so a wave never diverges in it.
template <bool P2>
__global__ __launch_bounds__(256) void trace_particles_kernel(const float *__restrict__ u, const float *__restrict__ v,
                                                              const float *__restrict__ w, float *px, float *py, float *pz,
                                                              long n, Spacing sp, int ni, int nj, int nk, float cfldt, float dt)
{
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    Vel3 vel{make_field(u, ni + 1, nj, nk), make_field(v, ni, nj + 1, nk), make_field(w, ni, nj, nk + 1)};
    const f3 hi = mk3((float)ni * sp.h - sp.h, (float)nj * sp.h - sp.h, (float)nk * sp.h - sp.h);
    const f3 q = trace<P2>(vel, sp, hi, cfldt, dt, mk3(px[a], py[a], pz[a]));
    px[a] = q.x; py[a] = q.y; pz[a] = q.z;
}

template <bool P2>
__global__ __launch_bounds__(256) void sample_particles_kernel(const float *__restrict__ field, int nx, int ny, int nz, Spacing sp,
                                                               float ox, float oy, float oz, const float *__restrict__ px, const float *__restrict__ py,
                                                               const float *__restrict__ pz, float *__restrict__ out, long n)
{
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    out[a] = sample<P2>(make_field(field, nx, ny, nz), sp, mk3(ox, oy, oz), mk3(px[a], py[a], pz[a]));
}

static inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

void launch_trace_particles(const float *u, const float *v, const float *w, float *px, float *py, float *pz, long n,
                            float h, int ni, int nj, int nk, float cfldt, float dt)
{
    const Spacing sp = make_spacing(h);
    hipStream_t st = rt().compute;
    if (sp.pow2) trace_particles_kernel<true><<<blocks_for(n), 256, 0, st>>>(u, v, w, px, py, pz, n, sp, ni, nj, nk, cfldt, dt);
    else         trace_particles_kernel<false><<<blocks_for(n), 256, 0, st>>>(u, v, w, px, py, pz, n, sp, ni, nj, nk, cfldt, dt);
    BQ_LAUNCH_CHECK("trace_particles_kernel");
}

void launch_sample_particles(const float *field, int nx, int ny, int nz, float h, float ox, float oy, float oz,
                             const float *px, const float *py, const float *pz, float *out, long n)
{
    const Spacing sp = make_spacing(h);
    hipStream_t st = rt().compute;
    if (sp.pow2) sample_particles_kernel<true><<<blocks_for(n), 256, 0, st>>>(field, nx, ny, nz, sp, ox, oy, oz, px, py, pz, out, n);
    else         sample_particles_kernel<false><<<blocks_for(n), 256, 0, st>>>(field, nx, ny, nz, sp, ox, oy, oz, px, py, pz, out, n);
    BQ_LAUNCH_CHECK("sample_particles_kernel");
}

} // inline namespace BQ_VARIANT

#ifndef BQ_FAST_LERP
namespace fast {        // the -DBQ_FAST_LERP build of this file
void launch_trace_particles(const float *u, const float *v, const float *w, float *px, float *py, float *pz, long n,
                            float h, int ni, int nj, int nk, float cfldt, float dt);
void launch_sample_particles(const float *field, int nx, int ny, int nz, float h, float ox, float oy, float oz,
                             const float *px, const float *py, const float *pz, float *out, long n);
}

// ---- seeding ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned seed_mix(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

struct SeedBox { int i0, j0, k0, bx, by, bz; };

__global__ __launch_bounds__(256) void seed_particles_kernel(float *__restrict__ px, float *__restrict__ py, float *__restrict__ pz,
                                                             long n, SeedBox b, int per_cell, unsigned seed, float h,
                                                             int ni, int nj, int nk)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const unsigned s = (unsigned)(p % per_cell);
    long cell = p / per_cell;
    const int x = (int)(cell % b.bx); cell /= b.bx;
    const int y = (int)(cell % b.by);
    const int z = (int)(cell / b.by);
    const int C[3] = { b.i0 + x, b.j0 + y, b.k0 + z };
    const int dims[3] = { ni, nj, nk };
    const unsigned long long G = (unsigned long long)C[0] + (unsigned long long)ni * ((unsigned long long)C[1] + (unsigned long long)nj * (unsigned long long)C[2]);
    const unsigned long long c = G * (unsigned long long)per_cell + s;
    const unsigned base = seed_mix(seed_mix((unsigned)c ^ seed) + (unsigned)(c >> 32));
    float out[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const unsigned r = seed_mix(base + (unsigned)a * 0x9e3779b9u) >> 8;
        const float q = (float)C[a] + (float)r * 5.9604644775390625e-8f;       // 2^-24
        out[a] = clampf(q * h, h, (float)dims[a] * h - h);
    }
    px[p] = out[0]; py[p] = out[1]; pz[p] = out[2];
}

// ---- sorting by brick ------------------------------------------------------------------------------------------------
struct BrickGeom { int ni, nj, nk, nbx, nby; float h; };

__device__ __forceinline__ unsigned brick_key(const BrickGeom &g, float x, float y, float z)
{
    // v_cvt_flr_i32_f32 saturates and sends a NaN to 0: the clamp below keeps every key inside the table
    const int i = min(max(floor_to_int(x / g.h), 0), g.ni - 1) >> 2;
    const int j = min(max(floor_to_int(y / g.h), 0), g.nj - 1) >> 2;
    const int k = min(max(floor_to_int(z / g.h), 0), g.nk - 1) >> 2;
    return (unsigned)(i + g.nbx * (j + g.nby * k));
}

__global__ __launch_bounds__(256) void sort_histogram_kernel(const float *__restrict__ px, const float *__restrict__ py,
                                                             const float *__restrict__ pz, long n, BrickGeom g, unsigned *count)
{
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    atomicAdd(&count[brick_key(g, px[a], py[a], pz[a])], 1u);
}

// exclusive scan of count[0 .. nb) in place, one block of 1024 threads: each thread owns a contiguous run
__global__ __launch_bounds__(1024) void sort_scan_kernel(unsigned *count, int nb)
{
    __shared__ unsigned part[1024];
    const int t = threadIdx.x;
    const int run = (nb + 1023) / 1024;
    const int lo = min(t * run, nb), hi = min(lo + run, nb);
    unsigned s = 0;
    for (int a = lo; a < hi; a++) s += count[a];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {            // Hillis-Steele inclusive scan of the run sums
        const unsigned add = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    unsigned at = part[t] - s;                      // exclusive prefix of this thread's run
    for (int a = lo; a < hi; a++) { const unsigned c = count[a]; count[a] = at; at += c; }
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(const float *__restrict__ px, const float *__restrict__ py,
                                                           const float *__restrict__ pz, const unsigned *__restrict__ id,
                                                           float *__restrict__ qx, float *__restrict__ qy, float *__restrict__ qz,
                                                           unsigned *__restrict__ qid, long n, BrickGeom g, unsigned *offset)
{
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const float x = px[a], y = py[a], z = pz[a];
    const unsigned slot = atomicAdd(&offset[brick_key(g, x, y, z)], 1u);
    if (slot >= (unsigned long)n) return;           // cannot happen while the inputs are what the histogram read
    qx[slot] = x; qy[slot] = y; qz[slot] = z;
    qid[slot] = id ? id[a] : (unsigned)a;
}
#endif // !BQ_FAST_LERP

} // namespace bq

#ifndef BQ_FAST_LERP
using namespace bq;

static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// the size limits of the gather operators (bq_advect.hip: dims_ok) for a buffer of nx x ny x nz floats
static bool field_dims_ok(int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return false;
    if (4.0 * (double)nx * (double)ny * (double)nz >= 2147483648.0) return false;
    return (double)nx * (double)ny < 8388608.0;
}

namespace {
struct Refusal {
    const char *op; int before;
    int bad(const char *why) const { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; }
    int slab() const { latch(FL_ERR_UNSUPPORTED, op, "tracer particles are not built for z-slab ranks"); return (int)FL_ERR_UNSUPPORTED; }
    int done() const { return fl_last_error() != before ? fl_last_error() : (int)FL_OK; }
};
}

extern "C" int gpu_trace_particles(const float *u, const float *v, const float *w, float *px, float *py, float *pz, long n,
                                   float h, int ni, int nj, int nk, float cfldt, float dt)
{
    static const char *op = "gpu_trace_particles";
    if (!ensure_ready(op)) return fl_last_error();
    const Refusal r{op, fl_last_error()};
    if (!u || !v || !w || !px || !py || !pz) return r.bad("null pointer");
    if (n < 0) return r.bad("n < 0");
    if (ni < 5 || nj < 5 || nk < 5) return r.bad("dims below 5");
    if (!field_dims_ok(ni + 1, nj + 1, nk + 1)) return r.bad("grid beyond the operators' size limits");
    if (!std::isfinite(h) || !(h > 0.f) || !std::isfinite(cfldt) || !std::isfinite(dt)) return r.bad("h, cfldt and dt must be finite, h > 0");
    if (!(cfldt > 0.f) && dt != 0.f) return r.bad("cfldt <= 0 with dt != 0 would never terminate");
    const size_t pb = (size_t)n * sizeof(float);
    const size_t ub = (size_t)(ni + 1) * nj * nk * 4, vb = (size_t)ni * (nj + 1) * nk * 4, wb = (size_t)ni * nj * (nk + 1) * 4;
    for (const float *p : { px, py, pz })
        if (overlaps(p, pb, u, ub) || overlaps(p, pb, v, vb) || overlaps(p, pb, w, wb)) return r.bad("a position array aliases a velocity array");
    if (overlaps(px, pb, py, pb) || overlaps(px, pb, pz, pb) || overlaps(py, pb, pz, pb)) return r.bad("position arrays overlap");
    if (rt().slab_on) return r.slab();
    if (n == 0) return FL_OK;
    if (rt().opt_fast_lerp) bq::fast::launch_trace_particles(u, v, w, px, py, pz, n, h, ni, nj, nk, cfldt, dt);
    else                    bq::exact::launch_trace_particles(u, v, w, px, py, pz, n, h, ni, nj, nk, cfldt, dt);
    return r.done();
}

extern "C" int gpu_sample_particles(const float *field, int nx, int ny, int nz, float h, float ox, float oy, float oz,
                                    const float *px, const float *py, const float *pz, float *out, long n)
{
    static const char *op = "gpu_sample_particles";
    if (!ensure_ready(op)) return fl_last_error();
    const Refusal r{op, fl_last_error()};
    if (!field || !px || !py || !pz || !out) return r.bad("null pointer");
    if (n < 0) return r.bad("n < 0");
    if (!field_dims_ok(nx, ny, nz)) return r.bad("field dims outside the operators' size limits");
    if (!std::isfinite(h) || !(h > 0.f)) return r.bad("h must be finite and positive");
    const size_t pb = (size_t)n * sizeof(float);
    if (overlaps(out, pb, field, (size_t)nx * ny * nz * 4) || overlaps(out, pb, px, pb) || overlaps(out, pb, py, pb) ||
        overlaps(out, pb, pz, pb)) return r.bad("out aliases an input");
    if (rt().slab_on) return r.slab();
    if (n == 0) return FL_OK;
    if (rt().opt_fast_lerp) bq::fast::launch_sample_particles(field, nx, ny, nz, h, ox, oy, oz, px, py, pz, out, n);
    else                    bq::exact::launch_sample_particles(field, nx, ny, nz, h, ox, oy, oz, px, py, pz, out, n);
    return r.done();
}

extern "C" int gpu_seed_particles(float *px, float *py, float *pz, int i0, int i1, int j0, int j1, int k0, int k1, int per_cell,
                                  unsigned seed, float h, int ni, int nj, int nk)
{
    static const char *op = "gpu_seed_particles";
    if (!ensure_ready(op)) return fl_last_error();
    const Refusal r{op, fl_last_error()};
    if (per_cell < 1) return r.bad("per_cell < 1");
    if (ni < 5 || nj < 5 || nk < 5) return r.bad("dims below 5");
    if (!field_dims_ok(ni + 1, nj + 1, nk + 1)) return r.bad("grid beyond the operators' size limits");
    if (!std::isfinite(h) || !(h > 0.f)) return r.bad("h must be finite and positive");
    SeedBox b;
    b.i0 = std::max(i0, 1); b.j0 = std::max(j0, 1); b.k0 = std::max(k0, 1);
    b.bx = std::max(std::min(i1, ni - 1) - b.i0, 0);
    b.by = std::max(std::min(j1, nj - 1) - b.j0, 0);
    b.bz = std::max(std::min(k1, nk - 1) - b.k0, 0);
    const double count = (double)b.bx * (double)b.by * (double)b.bz * (double)per_cell;
    if (count > 2147483647.0) return r.bad("more than 2^31 - 1 particles");
    if (rt().slab_on) return r.slab();
    const long n = (long)count;
    if (n == 0) return FL_OK;
    if (!px || !py || !pz) return r.bad("null pointer");
    seed_particles_kernel<<<blocks_for(n), 256, 0, rt().compute>>>(px, py, pz, n, b, per_cell, seed, h, ni, nj, nk);
    BQ_LAUNCH_CHECK("seed_particles_kernel");
    return r.done();
}

extern "C" int gpu_sort_particles(const float *px, const float *py, const float *pz, const unsigned *id,
                                  float *qx, float *qy, float *qz, unsigned *qid, long n, float h, int ni, int nj, int nk)
{
    static const char *op = "gpu_sort_particles";
    if (!ensure_ready(op)) return fl_last_error();
    const Refusal r{op, fl_last_error()};
    if (!px || !py || !pz || !qx || !qy || !qz || !qid) return r.bad("null pointer");
    if (n < 0 || n > 2147483647L) return r.bad("n outside [0, 2^31)");
    if (!field_dims_ok(ni + 1, nj + 1, nk + 1)) return r.bad("grid outside the operators' size limits");
    if (!std::isfinite(h) || !(h > 0.f)) return r.bad("h must be finite and positive");
    const size_t pb = (size_t)n * sizeof(float);
    const void *ins[] = { px, py, pz, id }, *outs[] = { qx, qy, qz, qid };
    for (int a = 0; a < 4; a++) {
        for (int b = 0; b < 4; b++)
            if (overlaps(outs[a], pb, ins[b], pb)) return r.bad("an output aliases an input");
        for (int b = a + 1; b < 4; b++)
            if (overlaps(outs[a], pb, outs[b], pb)) return r.bad("outputs overlap");
    }
    if (rt().slab_on) return r.slab();
    if (n == 0) return FL_OK;
    BrickGeom g;
    g.ni = ni; g.nj = nj; g.nk = nk; g.h = h;
    g.nbx = (ni + 3) / 4; g.nby = (nj + 3) / 4;
    const int nb = g.nbx * g.nby * ((nk + 3) / 4);
    unsigned *table = (unsigned *)scratch((size_t)(nb + 1) * sizeof(unsigned));
    if (!table) return r.done();
    hipStream_t st = rt().compute;
    if (!BQ_HIP(hipMemsetAsync(table, 0, (size_t)(nb + 1) * sizeof(unsigned), st))) return r.done();
    sort_histogram_kernel<<<blocks_for(n), 256, 0, st>>>(px, py, pz, n, g, table);
    BQ_LAUNCH_CHECK("sort_histogram_kernel");
    sort_scan_kernel<<<1, 1024, 0, st>>>(table, nb);
    BQ_LAUNCH_CHECK("sort_scan_kernel");
    sort_scatter_kernel<<<blocks_for(n), 256, 0, st>>>(px, py, pz, id, qx, qy, qz, qid, n, g, table);
    BQ_LAUNCH_CHECK("sort_scatter_kernel");
    return r.done();
}
#endif // !BQ_FAST_LERP
