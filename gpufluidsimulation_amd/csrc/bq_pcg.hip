// bq_pcg.hip -- BQ_PROJECTION_PCG: the masked Neumann pressure system of section 14 solved in fp64
// by flexible preconditioned CG to a relative tolerance, the CPU solver's semantics (BimocqSolver.cpp:1269, AMGPCGSolve).
//
//   unknowns     interior cells that are fluid with s < 6 solid neighbours; diagonal 6 - s, -1 per interior fluid neighbour
//   b            -div at the unknowns (alpha = -1), border cells held at p = 0
//   CG           x0 = 0, r0 = b; alpha = rho / d.Ad; flexible (Polak-Ribiere) beta = -alpha z'.Ad / rho, i.e. z'.(r' - r) / rho
//   stop         after the update with max|r| <= tol max|b|, at `iters` updates, or on a breakdown (the update is skipped)
//   M^-1         2 weighted-Jacobi sweeps (omega = 6/7) on level 0 from zero, the level-0 residual restricted to level 1, one
//                unmasked V-cycle of bq_mgcg.hip's coarse machinery there (mgcg_pcg_coarse: 4 sweeps down, 32 at the bottom, 4
//                up), prolongation into z, 2 more sweeps; the level-0 sweeps write 0 at every cell that is not an unknown
//   reductions   fp64, fixed order: a block of 256 threads owns 2048 consecutive cells (thread t: cells t, t + 256, ...), its
//                threads' sums meet in a fixed LDS tree; one block sums the partials (thread t: partials t, t + 256, ...)
//                and runs the same tree.  max|r| is order-free.  tests/cpu_abi/pcg_abi.c restates all of it bit for bit.
//
// Every level-0 array is written in full before it is read, and the coarse arrays are cleared once per solve, so nothing
// depends on what the work arrays hold on entry.  Bounds: the level-0 kernels stream fp64 arrays (one thread per cell, the
// six neighbour loads from the caches).
#include "bq_device.hip.h"
#include "bq_host.h"

#include <cstdint>
#include <cstring>

namespace bq {

namespace {

constexpr int kPcgBlock = 256, kPcgCpt = 8, kPcgCells = kPcgBlock * kPcgCpt;     // cells per reduction block
// scalars in the work array
enum { S_RHO = 0, S_DQ, S_ALPHA, S_OKA, S_ZQ, S_BETA, S_OKB, S_MAXR, S_MAXB, S_COUNT };
enum { MODE_MAXB = 0, MODE_RHO0, MODE_ALPHA, MODE_MAXR, MODE_BETA };
// code of a cell: bit 15 unknown, bits 8..10 solid neighbours s, bit q < 6 neighbour q (-x, +x, -y, +y, -z, +z) is an unknown
constexpr unsigned kUnknown = 0x8000u;

struct PcgWeights { double w[7]; double omw; };      // w[s] = omega / (6 - s), omw = 1 - omega

__global__ __launch_bounds__(256) void pcg_code_kernel(const unsigned char *__restrict__ solid, uint16_t *__restrict__ code,
                                                       int ni, int nj, int nk)
{
    const size_t n = (size_t)ni * nj * nk;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int i = (int)(id % ni), j = (int)((id / ni) % nj), k = (int)(id / ((size_t)ni * nj));
    auto interior = [&](int a, int b, int c) { return a > 0 && a < ni - 1 && b > 0 && b < nj - 1 && c > 0 && c < nk - 1; };
    auto is_solid = [&](size_t q) { return solid && solid[q] != 0; };
    if (!interior(i, j, k) || is_solid(id)) { code[id] = 0; return; }
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t nb[6] = { id - 1, id + 1, id - sj, id + sj, id - sk, id + sk };
    const int ii[6] = { i - 1, i + 1, i, i, i, i }, jj[6] = { j, j, j - 1, j + 1, j, j }, kk[6] = { k, k, k, k, k - 1, k + 1 };
    unsigned s = 0, bits = 0;
    for (int q = 0; q < 6; q++) {
        if (is_solid(nb[q])) s++;
        else if (interior(ii[q], jj[q], kk[q])) bits |= 1u << q;
    }
    code[id] = (uint16_t)(s == 6 ? 0u : (kUnknown | (s << 8) | bits));
}

// sum of the unknown neighbours of cell id in the fixed order -x, +x, -y, +y, -z, +z
__device__ __forceinline__ double nb_sum(const double *__restrict__ x, size_t id, unsigned c, size_t sj, size_t sk)
{
    double acc = 0.0;
    acc = acc + ((c & 1u) ? x[id - 1] : 0.0);
    acc = acc + ((c & 2u) ? x[id + 1] : 0.0);
    acc = acc + ((c & 4u) ? x[id - sj] : 0.0);
    acc = acc + ((c & 8u) ? x[id + sj] : 0.0);
    acc = acc + ((c & 16u) ? x[id - sk] : 0.0);
    acc = acc + ((c & 32u) ? x[id + sk] : 0.0);
    return acc;
}

// one weighted-Jacobi sweep of A z = rhs, every cell written (0 where no unknown); FIRST: from z = 0 (in is not read)
template <bool FIRST>
__global__ __launch_bounds__(256) void pcg_smooth_kernel(const double *__restrict__ in, const double *__restrict__ rhs,
                                                         double *__restrict__ out, const uint16_t *__restrict__ code,
                                                         PcgWeights W, size_t n, int ni, int nj)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const unsigned c = code[id];
    if (!(c & kUnknown)) { out[id] = 0.0; return; }
    const double w = W.w[(c >> 8) & 7u];
    if (FIRST) { out[id] = rhs[id] * w; return; }
    const double acc = nb_sum(in, id, c, (size_t)ni, (size_t)ni * nj);
    out[id] = W.omw * in[id] + (acc + rhs[id]) * w;
}

// out = 4 (A z - rhs) at the unknowns, 0 elsewhere: the level-0 residual in the sign of bq_mgcg.hip's L (= -A), scaled for
// level 1 (mgcg_pcg_coarse)
__global__ __launch_bounds__(256) void pcg_resid4_kernel(const double *__restrict__ z, const double *__restrict__ rhs,
                                                         double *__restrict__ out, const uint16_t *__restrict__ code,
                                                         size_t n, int ni, int nj)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const unsigned c = code[id];
    if (!(c & kUnknown)) { out[id] = 0.0; return; }
    const double acc = nb_sum(z, id, c, (size_t)ni, (size_t)ni * nj);
    const double az = (double)(6 - (int)((c >> 8) & 7u)) * z[id] - acc;
    out[id] = 4.0 * (az - rhs[id]);
}

// the block's LDS tree over its 256 thread values (sum or max); thread 0 returns the result
template <bool MAX>
__device__ __forceinline__ double block_tree(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = kPcgBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = MAX ? fmax(sh[threadIdx.x], sh[threadIdx.x + s]) : sh[threadIdx.x] + sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// r = b at the unknowns (0 elsewhere), p = 0, partial max|b|
__global__ __launch_bounds__(256) void pcg_init_kernel(const double *__restrict__ div, const uint16_t *__restrict__ code,
                                                       double *__restrict__ r, double *__restrict__ p, double *__restrict__ part,
                                                       size_t n)
{
    __shared__ double sh[kPcgBlock];
    double m = 0.0;
    for (int e = 0; e < kPcgCpt; e++) {
        const size_t id = (size_t)blockIdx.x * kPcgCells + (size_t)e * kPcgBlock + threadIdx.x;
        if (id >= n) break;
        const double b = (code[id] & kUnknown) ? -div[id] : 0.0;
        r[id] = b;
        p[id] = 0.0;
        m = fmax(m, fabs(b));
    }
    const double t = block_tree<true>(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// q = A d (0 where no unknown), partial d.q
__global__ __launch_bounds__(256) void pcg_apply_kernel(const double *__restrict__ d, double *__restrict__ q,
                                                        const uint16_t *__restrict__ code, double *__restrict__ part,
                                                        size_t n, int ni, int nj)
{
    __shared__ double sh[kPcgBlock];
    double s = 0.0;
    for (int e = 0; e < kPcgCpt; e++) {
        const size_t id = (size_t)blockIdx.x * kPcgCells + (size_t)e * kPcgBlock + threadIdx.x;
        if (id >= n) break;
        const unsigned c = code[id];
        double v = 0.0;
        if (c & kUnknown) {
            const double acc = nb_sum(d, id, c, (size_t)ni, (size_t)ni * nj);
            v = (double)(6 - (int)((c >> 8) & 7u)) * d[id] - acc;
        }
        q[id] = v;
        s = s + d[id] * v;
    }
    const double t = block_tree<false>(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// p += alpha d, r -= alpha q, partial max|r|; nothing is written when the step broke down
__global__ __launch_bounds__(256) void pcg_update_kernel(double *__restrict__ p, double *__restrict__ r, const double *__restrict__ d,
                                                         const double *__restrict__ q, const double *__restrict__ S,
                                                         double *__restrict__ part, size_t n)
{
    __shared__ double sh[kPcgBlock];
    if (S[S_OKA] == 0.0) return;
    const double alpha = S[S_ALPHA];
    double m = 0.0;
    for (int e = 0; e < kPcgCpt; e++) {
        const size_t id = (size_t)blockIdx.x * kPcgCells + (size_t)e * kPcgBlock + threadIdx.x;
        if (id >= n) break;
        p[id] = p[id] + alpha * d[id];
        const double rn = r[id] - alpha * q[id];
        r[id] = rn;
        m = fmax(m, fabs(rn));
    }
    const double t = block_tree<true>(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// partials of z.r (set 0) and, TWO, z.q (set 1)
template <bool TWO>
__global__ __launch_bounds__(256) void pcg_dots_kernel(const double *__restrict__ z, const double *__restrict__ r,
                                                       const double *__restrict__ q, double *__restrict__ part, int nparts, size_t n)
{
    __shared__ double sh[kPcgBlock];
    double a = 0.0, b = 0.0;
    for (int e = 0; e < kPcgCpt; e++) {
        const size_t id = (size_t)blockIdx.x * kPcgCells + (size_t)e * kPcgBlock + threadIdx.x;
        if (id >= n) break;
        const double zz = z[id];
        a = a + zz * r[id];
        if (TWO) b = b + zz * q[id];
    }
    const double ta = block_tree<false>(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = ta;
    if (TWO) {
        __syncthreads();
        const double tb = block_tree<false>(b, sh);
        if (threadIdx.x == 0) part[nparts + blockIdx.x] = tb;
    }
}

// d = z + beta d (skipped after a breakdown)
__global__ __launch_bounds__(256) void pcg_dir_kernel(double *__restrict__ d, const double *__restrict__ z, const double *__restrict__ S, size_t n)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n || S[S_OKB] == 0.0) return;
    d[id] = z[id] + S[S_BETA] * d[id];
}

__device__ __forceinline__ bool pos_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// one block: the partials of `sets` sets summed (or maxed) in the fixed order, then the scalar step of `mode`
template <bool MAX>
__device__ double final_sum(const double *part, int nparts, double *sh)
{
    double s = 0.0;
    for (int q = threadIdx.x; q < nparts; q += kPcgBlock) s = MAX ? fmax(s, part[q]) : s + part[q];
    const double t = block_tree<MAX>(s, sh);
    __syncthreads();
    return t;
}
__global__ __launch_bounds__(256) void pcg_reduce_kernel(const double *__restrict__ part, int nparts, double *__restrict__ S, int mode)
{
    __shared__ double sh[kPcgBlock];
    if (mode == MODE_MAXB || mode == MODE_MAXR) {
        const double m = final_sum<true>(part, nparts, sh);
        if (threadIdx.x == 0) S[mode == MODE_MAXB ? S_MAXB : S_MAXR] = m;
        return;
    }
    const double a = final_sum<false>(part, nparts, sh);
    const double b = mode == MODE_BETA ? final_sum<false>(part + nparts, nparts, sh) : 0.0;
    if (threadIdx.x != 0) return;
    if (mode == MODE_RHO0) {
        S[S_RHO] = a;
        S[S_OKB] = pos_finite(a) ? 1.0 : 0.0;
    } else if (mode == MODE_ALPHA) {
        const double rho = S[S_RHO];
        const bool ok = S[S_OKB] != 0.0 && pos_finite(rho) && pos_finite(a);     // (OKB: the direction was updated)
        S[S_DQ] = a;
        S[S_ALPHA] = ok ? rho / a : 0.0;
        S[S_OKA] = ok ? 1.0 : 0.0;
    } else {                                                    // MODE_BETA: a = z'.r', b = z'.q
        const double rho = S[S_RHO];
        const bool ok = pos_finite(a) && b - b == 0.0;
        S[S_ZQ] = b;
        S[S_BETA] = ok ? -(S[S_ALPHA] * b) / rho : 0.0;
        S[S_RHO] = a;
        S[S_OKB] = ok ? 1.0 : 0.0;
    }
}

// fp64 divergence of mg_divergence_kernel, every cell
__global__ __launch_bounds__(256) void pcg_divergence_kernel(const float *__restrict__ u, const float *__restrict__ v,
                                                             const float *__restrict__ w, double *__restrict__ div,
                                                             int ni, int nj, int nk, double halfrdx)
{
    const size_t n = (size_t)ni * nj * nk;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int i = (int)(id % ni), j = (int)((id / ni) % nj), k = (int)(id / ((size_t)ni * nj));
    const double ul = u[(size_t)i + (size_t)(ni + 1) * (j + (size_t)nj * k)], ur = u[(size_t)i + 1 + (size_t)(ni + 1) * (j + (size_t)nj * k)];
    const double vf = v[(size_t)i + (size_t)ni * (j + (size_t)(nj + 1) * k)], vb = v[(size_t)i + (size_t)ni * (j + 1 + (size_t)(nj + 1) * k)];
    const double wd = w[id], wu = w[id + (size_t)ni * nj];
    div[id] = halfrdx * ((ur - ul) + (vb - vf) + (wu - wd));
}

// mg_gradient_kernel's window and expression on the faces whose two cells are fluid
// i0, j0, k0: the first cell index of the window on each axis (2, or 1 behind a closed wall: DESIGN.md section 18)
__device__ __forceinline__ void pcg_gradient_body(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                  const double *__restrict__ p, const unsigned char *__restrict__ solid,
                                                  int ni, int nj, int nk, double halfrdx, int i0, int j0, int k0)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (!(i >= i0 && i < ni && j >= j0 && j < nj && k >= k0 && k < nk)) return;
    const size_t sj = ni, sk = (size_t)ni * nj, id = (size_t)i + sj * j + sk * k;
    const double p0 = p[id];
    const bool fc = !solid || solid[id] == 0;
    if (fc && (!solid || solid[id - 1] == 0))  u[(size_t)i + (size_t)(ni + 1) * (j + (size_t)nj * k)] -= (float)(halfrdx * (p0 - p[id - 1]));
    if (fc && (!solid || solid[id - sj] == 0)) v[(size_t)i + (size_t)ni * (j + (size_t)(nj + 1) * k)] -= (float)(halfrdx * (p0 - p[id - sj]));
    if (fc && (!solid || solid[id - sk] == 0)) w[id] -= (float)(halfrdx * (p0 - p[id - sk]));
}
__global__ __launch_bounds__(256) void pcg_gradient_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                           const double *__restrict__ p, const unsigned char *__restrict__ solid,
                                                           int ni, int nj, int nk, double halfrdx)
{
    pcg_gradient_body(u, v, w, p, solid, ni, nj, nk, halfrdx, 2, 2, 2);
}
__global__ __launch_bounds__(256) void pcg_gradient_walls_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                                 const double *__restrict__ p, const unsigned char *__restrict__ solidw,
                                                                 int walls, int ni, int nj, int nk, double halfrdx)
{
    pcg_gradient_body(u, v, w, p, solidw, ni, nj, nk, halfrdx, (walls & BQ_WALL_XLO) ? 1 : 2, (walls & BQ_WALL_YLO) ? 1 : 2,
                      (walls & BQ_WALL_ZLO) ? 1 : 2);
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

} // namespace

// byte layout of the work array: codes (2 bytes per cell), then 3 partial sets and the scalars (doubles)
size_t pcg_work_offset(size_t n) { return (2 * n + 255) / 256 * 256; }
int pcg_nparts(size_t n) { return (int)((n + kPcgCells - 1) / kPcgCells); }

} // namespace bq

using namespace bq;

extern "C" {

void gpu_divergence_double(const float *u, const float *v, const float *w, double *div, int ni, int nj, int nk, double halfrdx)
{
    const char *op = "gpu_divergence_double";
    if (!ensure_ready(op)) return;
    BQ_REQUIRE(u && v && w && div && ni >= 1 && nj >= 1 && nk >= 1, op);
    pcg_divergence_kernel<<<blocks_of((size_t)ni * nj * nk), 256, 0, rt().compute>>>(u, v, w, div, ni, nj, nk, halfrdx);
    BQ_LAUNCH_CHECK(op);
}

void gpu_pcg_gradient(float *u, float *v, float *w, const double *p, const unsigned char *solid, int ni, int nj, int nk, double halfrdx)
{
    const char *op = "gpu_pcg_gradient";
    if (!ensure_ready(op)) return;
    BQ_REQUIRE(u && v && w && p && ni >= 1 && nj >= 1 && nk >= 1 && nk < 65535, op);
    pcg_gradient_kernel<<<dim3((ni + 1 + 63) / 64, (nj + 1 + 3) / 4, nk + 1), dim3(64, 4, 1), 0, rt().compute>>>(u, v, w, p, solid, ni, nj, nk, halfrdx);
    BQ_LAUNCH_CHECK(op);
}

void gpu_pcg_gradient_walls(float *u, float *v, float *w, const double *p, const unsigned char *solidw, int walls,
                            int ni, int nj, int nk, double halfrdx)
{
    const char *op = "gpu_pcg_gradient_walls";
    if (walls == 0) { gpu_pcg_gradient(u, v, w, p, solidw, ni, nj, nk, halfrdx); return; }
    if (!ensure_ready(op)) return;
    BQ_REQUIRE(u && v && w && p && solidw && walls > 0 && walls < 63 && ni >= 3 && nj >= 3 && nk >= 3 && nk < 65535, op);
    pcg_gradient_walls_kernel<<<dim3((ni + 1 + 63) / 64, (nj + 1 + 3) / 4, nk + 1), dim3(64, 4, 1), 0, rt().compute>>>(u, v, w, p, solidw, walls, ni, nj, nk, halfrdx);
    BQ_LAUNCH_CHECK(op);
}

void gpu_pcg_solve(const double *div, double *p, const unsigned char *solid, double *r, double *d, double *q, double *z,
                   double *t, double *work, struct SCoarseLevelInfo *levels, int levelNum, int iters, double tol, double *stats)
{
    const char *op = "gpu_pcg_solve";
    if (stats) { stats[0] = 0; stats[1] = 0; stats[2] = 0; stats[3] = BQ_PCG_BREAKDOWN; }
    if (!ensure_ready(op)) return;
    BQ_REQUIRE(div && p && r && d && q && z && t && work && levels && stats, op);
    BQ_REQUIRE(levelNum >= 1 && levelNum <= LEVEL_COUNT && iters >= 0 && tol > 0.0 && tol < 1.0, op);
    if (rt().slab_on) { latch(FL_ERR_UNSUPPORTED, op, "not built for z-slab ranks"); return; }
    for (int l = 0; l < levelNum; l++) {
        const SCoarseLevelInfo &L = levels[l];
        BQ_REQUIRE(L.ni >= 1 && L.nj >= 1 && L.nk >= 1 && L.nk < 65535 && (long long)L.ni * L.nj * L.nk == (long long)L.number, op);
        BQ_REQUIRE(l == 0 || (L.b && L.x && L.r && L.ni == (levels[l - 1].ni - 1) / 2 && L.nj == (levels[l - 1].nj - 1) / 2 &&
                              L.nk == (levels[l - 1].nk - 1) / 2), op);
    }
    const int ni = levels[0].ni, nj = levels[0].nj, nk = levels[0].nk;
    BQ_REQUIRE(ni >= 3 && nj >= 3 && nk >= 3, op);
    const size_t n = (size_t)levels[0].number;
    const int nparts = pcg_nparts(n);
    BQ_REQUIRE(pcg_work_offset(n) + (size_t)(3 * nparts + S_COUNT) * sizeof(double) <= n * sizeof(double), op);
    hipStream_t st = rt().compute;
    uint16_t *code = reinterpret_cast<uint16_t *>(work);
    double *part = reinterpret_cast<double *>(reinterpret_cast<char *>(work) + pcg_work_offset(n));
    double *S = part + 3 * nparts;
    double *host = static_cast<double *>(pinned(S_COUNT * sizeof(double)));
    if (!host) return;
    const bool coarse = levelNum >= 2;
    // M5 / M4: the coarse kernels read boundary entries they never write; they start from zeros in every solve
    for (int l = 1; l < levelNum; l++) {
        const size_t bytes = (size_t)levels[l].number * sizeof(double);
        BQ_HIP(hipMemsetAsync(levels[l].b, 0, bytes, st));
        BQ_HIP(hipMemsetAsync(levels[l].x, 0, bytes, st));
        BQ_HIP(hipMemsetAsync(levels[l].r, 0, bytes, st));
    }
    BQ_HIP(hipMemsetAsync(S, 0, S_COUNT * sizeof(double), st));
    pcg_code_kernel<<<blocks_of(n), 256, 0, st>>>(solid, code, ni, nj, nk);
    pcg_init_kernel<<<nparts, kPcgBlock, 0, st>>>(div, code, r, p, part, n);
    pcg_reduce_kernel<<<1, kPcgBlock, 0, st>>>(part, nparts, S, MODE_MAXB);
    if (!BQ_LAUNCH_CHECK(op)) return;

    const double omega = 6.0 / 7.0;
    PcgWeights W;
    for (int s = 0; s < 6; s++) W.w[s] = omega / (double)(6 - s);
    W.w[6] = 0.0;
    W.omw = 1.0 - omega;
    auto readback = [&]() -> bool {
        if (!BQ_HIP(hipMemcpyAsync(host, S, S_COUNT * sizeof(double), hipMemcpyDeviceToHost, st))) return false;
        return BQ_HIP(hipStreamSynchronize(st));
    };
    // z = M^-1 r (t: scratch, also the coarse levels' ping-pong partner)
    auto precondition = [&]() {
        pcg_smooth_kernel<true><<<blocks_of(n), 256, 0, st>>>(nullptr, r, t, code, W, n, ni, nj);
        pcg_smooth_kernel<false><<<blocks_of(n), 256, 0, st>>>(t, r, z, code, W, n, ni, nj);
        if (coarse) {
            pcg_resid4_kernel<<<blocks_of(n), 256, 0, st>>>(z, r, t, code, n, ni, nj);
            mgcg_restrict(t, levels[1].b, levels[0], levels[1]);
            mgcg_pcg_coarse(levels, levelNum, t, 4, 4, 32);
            mgcg_prolong(z, levels[1].x, levels[0], levels[1]);
        }
        pcg_smooth_kernel<false><<<blocks_of(n), 256, 0, st>>>(z, r, t, code, W, n, ni, nj);
        pcg_smooth_kernel<false><<<blocks_of(n), 256, 0, st>>>(t, r, z, code, W, n, ni, nj);
        BQ_LAUNCH_CHECK("pcg_smooth_kernel");
    };

    if (!readback()) return;
    const double maxb = host[S_MAXB];
    stats[2] = maxb;
    stats[1] = maxb;
    if (maxb == 0.0) { stats[3] = BQ_PCG_CONVERGED; return; }            // p = 0
    if (!(maxb <= 1.7976931348623157e308)) return;                       // not finite: breakdown, p = 0
    precondition();
    pcg_dots_kernel<false><<<nparts, kPcgBlock, 0, st>>>(z, r, nullptr, part, nparts, n);
    pcg_reduce_kernel<<<1, kPcgBlock, 0, st>>>(part, nparts, S, MODE_RHO0);
    BQ_HIP(hipMemcpyAsync(d, z, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    int it = 0;
    double reason = BQ_PCG_ITER_LIMIT, maxr = maxb;
    for (; it < iters; it++) {
        pcg_apply_kernel<<<nparts, kPcgBlock, 0, st>>>(d, q, code, part, n, ni, nj);
        pcg_reduce_kernel<<<1, kPcgBlock, 0, st>>>(part, nparts, S, MODE_ALPHA);
        pcg_update_kernel<<<nparts, kPcgBlock, 0, st>>>(p, r, d, q, S, part + 2 * nparts, n);
        pcg_reduce_kernel<<<1, kPcgBlock, 0, st>>>(part + 2 * nparts, nparts, S, MODE_MAXR);
        if (!BQ_LAUNCH_CHECK(op) || !readback()) return;
        if (host[S_OKB] == 0.0 || host[S_OKA] == 0.0) { reason = BQ_PCG_BREAKDOWN; break; }
        maxr = host[S_MAXR];
        if (maxr <= tol * maxb) { reason = BQ_PCG_CONVERGED; it++; break; }
        if (it + 1 == iters) { it++; break; }
        precondition();
        pcg_dots_kernel<true><<<nparts, kPcgBlock, 0, st>>>(z, r, q, part, nparts, n);
        pcg_reduce_kernel<<<1, kPcgBlock, 0, st>>>(part, nparts, S, MODE_BETA);
        pcg_dir_kernel<<<blocks_of(n), 256, 0, st>>>(d, z, S, n);
    }
    if (iters == 0 && !readback()) return;
    if (iters == 0 && host[S_OKB] == 0.0) reason = BQ_PCG_BREAKDOWN;
    stats[0] = it;
    stats[1] = maxr;
    stats[3] = reason;
}

} // extern "C"
