// bq_project.hip -- pressure projection: divergence, Jacobi
// sweeps, gradient subtraction, residual norms, viscous diffusion sweeps.
//
// The Jacobi sweep is THE roofline kernel of this path: 12 algorithmic bytes per voxel per
// sweep (read p, read div, write p').  jacobi_tile_kernel stages each p plane once through
// LDS (tile + one-deep halo), marches along k with the k-1 / k / k+1 centre values in
// registers, and moves everything as 16-byte vectors; see DESIGN.md "Jacobi kernel".
// Summation order is the reference's (GPU_kernel.cu:1834), so results are bit-identical.
#include "bq_device.hip.h"
#include "bq_sweep_pack.hip.h"
#include "bq_host.h"
#include "bq_jacobi_plan.h"
#include <algorithm>
#include <vector>

namespace bq {

// z-slab context of a launch: local plane k is global plane k + koff; nkg = global cell planes;
// [klo, khi): optional restriction of a stencil launch to a range of LOCAL planes (used to sweep the
// slab interior while the ghost planes are still in flight).
struct Slab { int koff, nkg, klo, khi; };
// Output planes of a fused two-sweep launch: chunks bz < nchA march [k0a, k1a), the others [k0b, k1b) (used to
// split a launch into the part that needs no ghost planes and the two parts next to them); L1 is evaluated
// wherever those outputs need it.  Whole array: {0, nz, 0, 0, nbz}.
struct PairRanges { int k0a, k1a, k0b, k1b, nchA; };

// ---- divergence_kernel (GPU_kernel.cu:967-985) --------------------------------------------
__global__ __launch_bounds__(256) void divergence_kernel(const float *__restrict__ u, const float *__restrict__ v,
                                                         const float *__restrict__ w, float *__restrict__ div,
                                                         int ni, int nj, int nk, float halfrdx, Slab sl)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    const int kg = k + sl.koff;
    if (i >= ni || j >= nj || kg < 0 || kg >= sl.nkg) return;
    const size_t iu = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
    const size_t iv = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
    const size_t ic = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
    float ul = u[iu], ur = u[iu + 1];
    float vf = v[iv], vb = v[iv + ni];
    float wd = w[ic], wu = w[ic + (size_t)ni * nj];
    div[ic] = halfrdx * ((ur - ul) + (vb - vf) + (wu - wd));
}

// ---- gradient_kernel x3 fused (GPU_kernel.cu:1024-1041, launches :1881-1891) -------------
// All three components update the same cell window 2..n-1, so one pass reads p once.
__global__ __launch_bounds__(256) void gradient_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                       const float *__restrict__ p, int ni, int nj, int nk, float halfrdx, Slab sl)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    const int kg = k + sl.koff;
    if (i < 2 || i >= ni || j < 2 || j >= nj || kg < 2 || kg >= sl.nkg) return;
    const size_t ic = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
    const float p0 = p[ic];
    const size_t iu = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
    const size_t iv = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
    u[iu] -= halfrdx * (p0 - p[ic - 1]);
    v[iv] -= halfrdx * (p0 - p[ic - ni]);
    // a slab rank's first local plane can lie inside the global window (kg >= 2): u and v need no plane below it, w does
    if (k >= 1) w[ic] -= halfrdx * (p0 - p[ic - (size_t)ni * nj]);
}

// The same update that also hands out what it changed: d = u_new - u_old on the window, 0 elsewhere -- exactly
// the d*Proj = U - UTemp that BimocqGPUSolver.cpp:188-193 forms from a snapshot taken before the projection
// (u_new and u_old are the very floats that subtraction sees), without the three snapshot copies and the three
// subtraction passes.  One thread per node of the (ni+1, nj+1, nk+1) super-grid.
__global__ __launch_bounds__(256) void gradient_delta_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                             const float *__restrict__ p,
                                                             float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                             int ni, int nj, int nk, float halfrdx, Slab sl)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    const int kg = k + sl.koff;
    const bool win = !(i < 2 || i >= ni || j < 2 || j >= nj || kg < 2 || kg >= sl.nkg || k >= nk);
    const size_t iu = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
    const size_t iv = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
    const size_t ic = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
    if (win) {
        const float p0 = p[ic];
        const float uo = u[iu], vo = v[iv];
        const float un = uo - halfrdx * (p0 - p[ic - 1]);
        const float vn = vo - halfrdx * (p0 - p[ic - ni]);
        u[iu] = un; v[iv] = vn;
        du[iu] = un - uo; dv[iv] = vn - vo;
        if (k >= 1) {       // as in gradient_kernel: w alone needs the plane below
            const float wo = w[ic], wn = wo - halfrdx * (p0 - p[ic - (size_t)ni * nj]);
            w[ic] = wn; dw[ic] = wn - wo;
        } else dw[ic] = 0.f;
    } else {
        if (j < nj && k < nk) du[iu] = 0.f;                  // the u buffer has ni+1 columns
        if (i < ni && k < nk) dv[iv] = 0.f;                  // the v buffer has nj+1 rows
        if (i < ni && j < nj) dw[ic] = 0.f;                  // the w buffer has nk+1 planes
    }
}

// ---- generic Jacobi sweep: any dims, one thread per cell (GPU_kernel.cu:1819-1837) --------
__global__ __launch_bounds__(256) void jacobi_generic_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                             float *__restrict__ out, int ni, int nj, int nk,
                                                             float alpha, float beta, Slab sl)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    const int kg = k + sl.koff;
    if (!(i > 0 && i < ni - 1 && j > 0 && j < nj - 1 && k > 0 && k < nk - 1 && kg > 0 && kg < sl.nkg - 1 && k >= sl.klo && k < sl.khi)) return;
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t id = (size_t)i + sj * j + sk * k;
    out[id] = (p[id - 1] + p[id + 1] + p[id - sj] + p[id + sj] + p[id - sk] + p[id + sk] + alpha * div[id]) * beta;
}

// ---- LDS-tiled, k-marching Jacobi sweep -----------------------------------------------------
// Block = 256 threads.  Tile = TX (= 4*TXV) floats in x by TY (= R*256/TXV) rows in y; the block
// marches over `kchunk` planes.  Per plane each thread owns R float4 of the tile: it loads them
// once from HBM (as plane k+1), keeps them in registers while they serve as k+1, k and k-1, and
// publishes them to LDS when they are plane k so that neighbours can read x+-1 / y+-1.
// LDS rows carry a 4-float pad on each side: the x halo column sits at pad[3] / pad'[0] and the
// 16-byte alignment of the interior is kept.
template <int TXV, int R>
struct JTile {
    static constexpr int RP = 256 / TXV;        // rows per pass
    static constexpr int TY = RP * R;
    static constexpr int TX = TXV * 4;
    static constexpr int LW = TX + 8;           // LDS row pitch (floats)
    static constexpr int PLANE = (TY + 2) * LW; // floats per LDS plane
};

template <int TXV, int R>
__global__ __launch_bounds__(256) void jacobi_tile_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                          float *__restrict__ out, int nx, int ny, int nz,
                                                          int kchunk, float alpha, float beta, Slab sl)
{
    using T = JTile<TXV, R>;
    __shared__ __attribute__((aligned(16))) float lds[2][T::PLANE];

    const int tid = threadIdx.x;
    const int lx = tid % TXV, rp = tid / TXV;
    const int x0 = blockIdx.x * T::TX, j0 = blockIdx.y * T::TY;
    // local planes 1..nz-2 that are interior planes of the GLOBAL grid
    const int kbeg = max(max(max(1, 1 - sl.koff), sl.klo), (int)blockIdx.z * kchunk);
    const int kend = min(min(min(nz - 1, sl.nkg - 1 - sl.koff), sl.khi), (int)blockIdx.z * kchunk + kchunk);
    if (kbeg >= kend) return;

    const int x = x0 + 4 * lx;                  // first column of this thread's float4 (nx % 4 == 0)
    const bool xin = x < nx;
    const size_t sj = nx, sk = (size_t)nx * ny;

    // halo assignments: two extra rows (j0-1, j0+TY) as float4, two extra columns as scalars
    const bool hrow_thread = tid < 2 * TXV;
    const int hr_row = (tid / TXV) ? T::TY : -1;
    const int hr_j = j0 + hr_row;
    const int hr_x = x0 + 4 * (tid % TXV);
    const bool hr_ok = hrow_thread && hr_j >= 0 && hr_j < ny && hr_x < nx;
    const int hc_id = tid - (256 - 2 * (T::TY + 2));           // >= 0 for the column-halo threads
    const bool hcol_thread = hc_id >= 0;
    const int hc_side = hcol_thread ? hc_id / (T::TY + 2) : 0;  // 0 = left, 1 = right
    const int hc_row = hcol_thread ? hc_id % (T::TY + 2) - 1 : 0;
    const int hc_j = j0 + hc_row;
    const int hc_x = hc_side ? x0 + T::TX : x0 - 1;
    const bool hc_ok = hcol_thread && hc_j >= 0 && hc_j < ny && hc_x >= 0 && hc_x < nx;

    float4 pm[R], pc[R], pn[R];
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: plane kbeg-1 -> pm (own only), plane kbeg -> pc + LDS[0] (own + halos)
#pragma unroll
    for (int m = 0; m < R; m++) {
        const int j = j0 + rp + m * T::RP;
        const bool ok = xin && j < ny;
        const size_t g = (size_t)x + sj * j;
        pm[m] = ok ? *reinterpret_cast<const float4 *>(p + g + sk * (kbeg - 1)) : zero4;
        pc[m] = ok ? *reinterpret_cast<const float4 *>(p + g + sk * kbeg) : zero4;
    }
    {
        float4 hr = hr_ok ? *reinterpret_cast<const float4 *>(p + (size_t)hr_x + sj * hr_j + sk * kbeg) : zero4;
        float hc = hc_ok ? p[(size_t)hc_x + sj * hc_j + sk * kbeg] : 0.f;
        float *L = lds[0];
#pragma unroll
        for (int m = 0; m < R; m++)
            *reinterpret_cast<float4 *>(L + (rp + m * T::RP + 1) * T::LW + 4 + 4 * lx) = pc[m];
        if (hrow_thread) *reinterpret_cast<float4 *>(L + (hr_row + 1) * T::LW + 4 + 4 * (tid % TXV)) = hr;
        if (hcol_thread) L[(hc_row + 1) * T::LW + (hc_side ? 4 + T::TX : 3)] = hc;
    }

    int cur = 0;
    for (int k = kbeg; k < kend; k++) {
        // (1) issue the loads of plane k+1 (own + halos) and div(k)
        float4 dv[R];
        const bool last = (k + 1 >= nz);       // never true (kend <= nz-1) but keeps loads in range
#pragma unroll
        for (int m = 0; m < R; m++) {
            const int j = j0 + rp + m * T::RP;
            const bool ok = xin && j < ny;
            const size_t g = (size_t)x + sj * j;
            pn[m] = (ok && !last) ? *reinterpret_cast<const float4 *>(p + g + sk * (k + 1)) : zero4;
            dv[m] = ok ? *reinterpret_cast<const float4 *>(div + g + sk * k) : zero4;
        }
        float4 hr = (hr_ok && !last) ? *reinterpret_cast<const float4 *>(p + (size_t)hr_x + sj * hr_j + sk * (k + 1)) : zero4;
        float hc = (hc_ok && !last) ? p[(size_t)hc_x + sj * hc_j + sk * (k + 1)] : 0.f;

        // (2) plane k is complete in LDS[cur]
        __syncthreads();
        const float *L = lds[cur];
#pragma unroll
        for (int m = 0; m < R; m++) {
            const int row = rp + m * T::RP;
            const int j = j0 + row;
            const float *c = L + (row + 1) * T::LW + 4 + 4 * lx;
            const float left = c[-1], right = c[4];
            const float4 fr = *reinterpret_cast<const float4 *>(c - T::LW);   // j-1
            const float4 bk = *reinterpret_cast<const float4 *>(c + T::LW);   // j+1
            const float4 q = pc[m];
            float4 o;
            // ((((((l + r) + f) + b) + d) + u) + alpha*div) * beta   -- GPU_kernel.cu:1834
            o.x = (left + q.y + fr.x + bk.x + pm[m].x + pn[m].x + alpha * dv[m].x) * beta;
            o.y = (q.x + q.z + fr.y + bk.y + pm[m].y + pn[m].y + alpha * dv[m].y) * beta;
            o.z = (q.y + q.w + fr.z + bk.z + pm[m].z + pn[m].z + alpha * dv[m].z) * beta;
            o.w = (q.z + right + fr.w + bk.w + pm[m].w + pn[m].w + alpha * dv[m].w) * beta;
            if (xin && j >= 1 && j < ny - 1) {
                float *dst = out + (size_t)x + sj * j + sk * k;
                if (x >= 4 && x + 4 < nx) {
                    *reinterpret_cast<float4 *>(dst) = o;
                } else {                        // the float4 touches the x boundary: interior lanes only
                    if (x >= 1) dst[0] = o.x;
                    dst[1] = o.y;
                    dst[2] = o.z;
                    if (x + 3 < nx - 1) dst[3] = o.w;
                }
            }
        }

        // (3) publish plane k+1 to the other LDS buffer, rotate registers
        float *Ln = lds[cur ^ 1];
#pragma unroll
        for (int m = 0; m < R; m++) {
            *reinterpret_cast<float4 *>(Ln + (rp + m * T::RP + 1) * T::LW + 4 + 4 * lx) = pn[m];
            pm[m] = pc[m];
            pc[m] = pn[m];
        }
        if (hrow_thread) *reinterpret_cast<float4 *>(Ln + (hr_row + 1) * T::LW + 4 + 4 * (tid % TXV)) = hr;
        if (hcol_thread) Ln[(hc_row + 1) * T::LW + (hc_side ? 4 + T::TX : 3)] = hc;
        cur ^= 1;
    }
}

// ---- register-marching Jacobi sweep (no LDS, no barrier) -----------------------------------------
// At 256^3 the three arrays (201 MB) live in the 256 MiB Infinity Cache, where a plain triad streams
// the same 12 B/voxel in ~25 us (tools/membw.hip): the sweep is then bound by how many independent
// 16-byte loads a CU keeps in flight, and a barrier per plane (the LDS kernel above) throttles that.
// Here a thread owns one float4 column of one row and marches along k with the k-1/k/k+1 centre
// values in registers; the j-1/j+1 rows are re-read as float4 (L1/L2 hits: the neighbouring waves of
// the block load them as their own centres), x-1/x+4 come from the neighbouring lanes by shuffle.
// The loads of plane k+1 are issued before plane k is computed, so each wave always has 4 vector
// loads in flight and never waits on another wave.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void jacobi_march_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                  float *__restrict__ out, int nx, int ny, int nz,
                                                                  int cw, int nbx, int nby, int kchunk, float alpha, float beta, Slab sl)
{
    // XCD-aware block order: blocks b and b+8 share an XCD (its L2); give each XCD a contiguous run
    // of (k-chunk, row-block) pairs so halo rows/planes are re-read from the same L2.
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);
    const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);

    const int rows = (WAVES * 64) / cw;             // rows of the tile (cw float4 columns each)
    const int c = threadIdx.x % cw, r = threadIdx.x / cw;
    const int xraw = (bx * cw + c) * 4, j = by * rows + r;
    const int kbeg = max(max(max(1, 1 - sl.koff), sl.klo), bz * kchunk);
    const int kend = min(min(min(nz - 1, sl.nkg - 1 - sl.koff), sl.khi), bz * kchunk + kchunk);
    if (kbeg >= kend) return;
    const bool active = xraw < nx && j >= 1 && j <= ny - 2;
    const int x = xraw < nx ? xraw : nx - 4;                    // lanes past the row read its last float4, never store
    const size_t sj = nx, sk = (size_t)nx * ny;
    const size_t g = (size_t)x + sj * (active ? j : 1);         // inactive lanes read a valid row, never store
    const int lane = threadIdx.x & 63;
    // a lane at a wave edge whose x-neighbour lives in another wave (rows longer than one wave)
    const bool fix_l = lane == 0 && c > 0, fix_r = lane == 63 && c < cw - 1;
    const bool tile_l = c == 0 && x > 0, tile_r = c == cw - 1 && x + 4 < nx;   // neighbour in another block

    // no branch or select per load: out-of-range lanes and the plane past the chunk's end are clamped into the
    // array, what they load is never used for a stored cell
#define BQ_LD4(ptr, off) (*reinterpret_cast<const float4 *>((ptr) + (off)))
    float4 pm = BQ_LD4(p, g + sk * (kbeg - 1));
    float4 pc = BQ_LD4(p, g + sk * kbeg);
    float4 pn = BQ_LD4(p, g + sk * (kbeg + 1));
    float4 fr = BQ_LD4(p, g - sj + sk * kbeg);
    float4 bk = BQ_LD4(p, g + sj + sk * kbeg);
    float4 dv = BQ_LD4(div, g + sk * kbeg);

    for (int k = kbeg; k < kend; k++) {
        // prefetch everything plane k+1 needs (its k+2 centre, its j+-1 rows, its div)
        const size_t k2 = (size_t)min(k + 2, nz - 1);       // k + 1 <= kend <= nz - 1 needs no clamp
        const float4 pn2 = BQ_LD4(p, g + sk * k2);
        const float4 fr2 = BQ_LD4(p, g - sj + sk * (k + 1));
        const float4 bk2 = BQ_LD4(p, g + sj + sk * (k + 1));
        const float4 dv2 = BQ_LD4(div, g + sk * (k + 1));
        float left = lane_up(pc.w), right = lane_down(pc.x);
        if (fix_l || tile_l) left = p[g - 1 + sk * k];
        if (fix_r || tile_r) right = p[g + 4 + sk * k];
        float4 o;
        // ((((((l + r) + f) + b) + d) + u) + alpha*div) * beta   -- GPU_kernel.cu:1834
        o.x = (left + pc.y + fr.x + bk.x + pm.x + pn.x + alpha * dv.x) * beta;
        o.y = (pc.x + pc.z + fr.y + bk.y + pm.y + pn.y + alpha * dv.y) * beta;
        o.z = (pc.y + pc.w + fr.z + bk.z + pm.z + pn.z + alpha * dv.z) * beta;
        o.w = (pc.z + right + fr.w + bk.w + pm.w + pn.w + alpha * dv.w) * beta;
        if (active) {
            float *dst = out + g + sk * k;
            if (x >= 4 && x + 4 < nx) {
                *reinterpret_cast<float4 *>(dst) = o;
            } else {                            // the float4 touches the x boundary: interior cells only
                if (x >= 1) dst[0] = o.x;
                dst[1] = o.y;
                dst[2] = o.z;
                if (x + 3 < nx - 1) dst[3] = o.w;
            }
        }
        pm = pc; pc = pn; pn = pn2; fr = fr2; bk = bk2; dv = dv2;
    }
#undef BQ_LD4
}

// ---- two Jacobi sweeps per launch (temporal fusion, register marching) ---------------------------
// The single-sweep kernel moves 12 B/voxel/sweep through the fabric.  Two consecutive sweeps
//     L1 = J(L0),  L2 = J(L1)        (J = jacobi_kernel, GPU_kernel.cu:1819-1837)
// are fused so that L1 never leaves the registers: a thread marches along k for one float4 column of
// row j, keeps L0 of the rows j-1, j, j+1 for three planes in registers, evaluates L1 on those three
// rows (the two outer ones redundantly: they are what the neighbouring waves compute as their centre)
// and from them L2 on row j, one plane behind.  Per plane: 8 float4 loads (5 of them L1/L2 hits),
// one store, for TWO sweeps -- the fabric traffic per sweep halves.  Each value is produced by exactly
// the reference's expression, so the result is bit-identical to two single sweeps.
// Preconditions (checked by the launcher): nx <= 256 (a row fits one wave; x-neighbours by shuffle)
// and both ping-pong buffers carry the same boundary layer (gpu_projection_jacobi's contract: the
// caller zeroes both), because boundary cells are never written and L1's boundary is taken from L0.
// WIDE: a row spans several waves (nx > 256 floats).  x-neighbours across a wave boundary cannot be shuffled:
// lane 0 / lane 63 fetch the L0 values of the cell just outside the wave from memory and evaluate the single L1
// value there themselves (a few one-lane loads per plane; no LDS, no barrier) -- the same scheme as the fp64
// smoother mg_smooth2_kernel (bq_mgcg.hip).
template <int WAVES, bool WIDE>
__global__ __launch_bounds__(WAVES * 64) void jacobi_march2_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                   float *__restrict__ out, int nx, int ny, int nz,
                                                                   int cw, int nby, int kchunk, float alpha, float beta, Slab sl, PairRanges rg)
{
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);      // XCD-contiguous block order
    const int by = b % nby, bz = b / nby;
    const int rows = (WAVES * 64) / cw;
    const int c = threadIdx.x % cw, r = threadIdx.x / cw;
    const int xraw = 4 * c, j = by * rows + r;
    // local planes a sweep may update: inside the array AND inside the global domain (z-slab ranks);
    // everything else counts as boundary and keeps its input value in L1
    const int kA = max(1, 1 - sl.koff), kB = min(nz - 1, sl.nkg - 1 - sl.koff);
    const int r0 = bz < rg.nchA ? rg.k0a + bz * kchunk : rg.k0b + (bz - rg.nchA) * kchunk, r1 = bz < rg.nchA ? rg.k1a : rg.k1b;
    const int kbeg = max(kA, r0), kend = min(min(kB, r1), r0 + kchunk);
    if (kbeg >= kend) return;
    const bool xok = xraw < nx;
    const bool active = xok && j >= 1 && j <= ny - 2;
    // Out-of-range rows, planes and lanes are CLAMPED into the array instead of being zero-filled: whatever
    // they load only ever feeds cells that are boundary (kept from L0) or not stored at all.  No branch per load.
    const int x = xok ? xraw : nx - 4;
    const size_t sj = nx, sk = (size_t)nx * ny;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool xlo = x == 0, xhi = x + 3 == nx - 1;
    auto rowoff = [&](int row) -> size_t { return (size_t)x + sj * (size_t)min(max(row, 0), ny - 1); };
    const size_t o_m2 = rowoff(j - 2), o_m1 = rowoff(j - 1), o_0 = rowoff(j), o_p1 = rowoff(j + 1), o_p2 = rowoff(j + 2);
    auto plane = [&](int pl) -> size_t { return sk * (size_t)min(max(pl, 0), nz - 1); };
    auto ld4 = [&](const float *ptr, size_t off) -> float4 { return *reinterpret_cast<const float4 *>(ptr + off); };
    const bool rowb_m1 = j - 1 <= 0 || j - 1 >= ny - 1, rowb_0 = j <= 0 || j >= ny - 1, rowb_p1 = j + 1 <= 0 || j + 1 >= ny - 1;
    // edge lanes (WIDE): lane 0 looks after the cell just left of the wave, lane 63 after the cell just right of it
    const int lane = threadIdx.x & 63;
    const bool edgeL = WIDE && lane == 0 && xok && xraw > 0, edgeR = WIDE && lane == 63 && xraw + 4 < nx;
    const bool edge = edgeL || edgeR;
    const int xe = edgeL ? xraw - 1 : xraw + 4;                        // the outside cell
    const int xo = edgeL ? xe - 1 : xe + 1;                            // its own outer x-neighbour
    const size_t e_m1 = (size_t)min(max(xe, 0), nx - 1) + sj * (size_t)min(max(j - 1, 0), ny - 1),
                 e_0 = (size_t)min(max(xe, 0), nx - 1) + sj * (size_t)min(max(j, 0), ny - 1),
                 e_p1 = (size_t)min(max(xe, 0), nx - 1) + sj * (size_t)min(max(j + 1, 0), ny - 1),
                 e_o = (size_t)min(max(xo, 0), nx - 1) + sj * (size_t)min(max(j, 0), ny - 1);
    const bool xe_boundary = xe <= 0 || xe >= nx - 1;

    // one Jacobi evaluation on a float4; ce = centre row (x-neighbours from the neighbouring lanes, or `outside`
    // at a wave edge), fr/bk = rows -+1, dn/up = planes -+1.  Boundary cells keep the input value.
    auto jac = [&](float4 ce, float4 fr, float4 bk, float4 dn, float4 up, float4 dv, float outside, bool boundary) -> float4 {
        float left = lane_up(ce.w), right = lane_down(ce.x);
        if (WIDE) {
            if (lane == 0) left = outside;
            if (lane == 63) right = outside;
        }
        float4 o;
        o.x = (left + ce.y + fr.x + bk.x + dn.x + up.x + alpha * dv.x) * beta;
        o.y = (ce.x + ce.z + fr.y + bk.y + dn.y + up.y + alpha * dv.y) * beta;
        o.z = (ce.y + ce.w + fr.z + bk.z + dn.z + up.z + alpha * dv.z) * beta;
        o.w = (ce.z + right + fr.w + bk.w + dn.w + up.w + alpha * dv.w) * beta;
        if (boundary) return ce;
        if (xlo) o.x = ce.x;
        if (xhi) o.w = ce.w;
        return o;
    };

    // L0 of rows j-1, j, j+1 on three consecutive planes; q = plane whose L1 is being built.  The loads of plane
    // q+2 are issued before plane q is computed.  The three plane sets rotate roles (below, centre, above) from
    // one plane to the next: the loop body is written once as `phase` and instantiated three times with the
    // sets permuted, so that no register moves are needed to rotate them.
    float4 A[3], B[3], C[3], Dv[3], Hf, Hb;
    int q = kbeg - 1;
    {
        const size_t pm = plane(q - 1), pc = plane(q), pn = plane(q + 1);
        A[0] = ld4(p, pm + o_m1); A[1] = ld4(p, pm + o_0); A[2] = ld4(p, pm + o_p1);
        B[0] = ld4(p, pc + o_m1); B[1] = ld4(p, pc + o_0); B[2] = ld4(p, pc + o_p1);
        C[0] = ld4(p, pn + o_m1); C[1] = ld4(p, pn + o_0); C[2] = ld4(p, pn + o_p1);
        Dv[0] = ld4(div, pc + o_m1); Dv[1] = ld4(div, pc + o_0); Dv[2] = ld4(div, pc + o_p1);
        Hf = ld4(p, pc + o_m2); Hb = ld4(p, pc + o_p2);
    }
    float4 Mc[3] = { zero4, zero4, zero4 };     // L1 on plane q-1
    float4 Mm = zero4;                          // L1 of row j on plane q-2
    float4 Dprev = zero4;                       // div of row j on plane q-1
    // the outside cell (edge lanes, WIDE only): L0 on rows j-1..j+1 at plane q (Ec), on row j at planes q-1 (Em) and
    // q+1 (En), its outer x-neighbour at plane q (Eo), its div (Eb); Xp: its L1 on row j, plane q-1
    float Ec[3] = { 0.f, 0.f, 0.f }, Em = 0.f, En = 0.f, Eo = 0.f, Eb = 0.f, Xp = 0.f;
    if (edge) {
        const size_t pm = plane(q - 1), pc = plane(q), pn = plane(q + 1);
        Ec[0] = p[pc + e_m1]; Ec[1] = p[pc + e_0]; Ec[2] = p[pc + e_p1];
        Em = p[pm + e_0]; En = p[pn + e_0]; Eo = p[pc + e_o]; Eb = div[pc + e_0];
    }

    // one plane: Lm/Lc/Ln = L0 on planes q-1/q/q+1; on return Lm holds plane q+2 (it becomes the next "above")
    auto phase = [&](float4 (&Lm)[3], float4 (&Lc)[3], float4 (&Ln)[3]) {
        const size_t pa = plane(q + 2), pb = plane(q + 1);
        float4 La[3], Da[3];
        La[0] = ld4(p, pa + o_m1); La[1] = ld4(p, pa + o_0); La[2] = ld4(p, pa + o_p1);
        Da[0] = ld4(div, pb + o_m1); Da[1] = ld4(div, pb + o_0); Da[2] = ld4(div, pb + o_p1);
        const float4 Hfa = ld4(p, pb + o_m2), Hba = ld4(p, pb + o_p2);
        float E2[3] = { 0.f, En, 0.f }, En2 = 0.f, Eo2 = 0.f, Eb2 = 0.f;
        if (edge) {
            E2[0] = p[pb + e_m1]; E2[2] = p[pb + e_p1];
            En2 = p[pa + e_0]; Eo2 = p[pb + e_o]; Eb2 = div[pb + e_0];
        }
        // L1 on plane q for rows j-1, j, j+1
        const bool qb = q < kA || q >= kB;
        float4 M[3];
        M[0] = jac(Lc[0], Hf, Lc[1], Lm[0], Ln[0], Dv[0], Ec[0], qb || rowb_m1);
        M[1] = jac(Lc[1], Lc[0], Lc[2], Lm[1], Ln[1], Dv[1], Ec[1], qb || rowb_0);
        M[2] = jac(Lc[2], Lc[1], Hb, Lm[2], Ln[2], Dv[2], Ec[2], qb || rowb_p1);
        // L1 of the outside cell on row j, plane q (edge lanes; a boundary cell keeps L0)
        float X = Ec[1];
        if (edge && !(qb || rowb_0 || xe_boundary)) {
            const float l = edgeL ? Eo : Lc[1].w, rr = edgeL ? Lc[1].x : Eo;
            X = (l + rr + Ec[0] + Ec[2] + Em + En + alpha * Eb) * beta;
        }
        // L2 on plane q-1 for row j
        const int k = q - 1;
        const float4 o = jac(Mc[1], Mc[0], Mc[2], Mm, M[1], Dprev, Xp, false);
        if (active && k >= kbeg && k < kend) {
            float *dst = out + (size_t)x + sj * j + sk * k;
            if (x >= 4 && x + 4 < nx) {
                *reinterpret_cast<float4 *>(dst) = o;
            } else {
                if (x >= 1) dst[0] = o.x;
                dst[1] = o.y;
                dst[2] = o.z;
                if (x + 3 < nx - 1) dst[3] = o.w;
            }
        }
        Mm = Mc[1];
        Dprev = Dv[1];
        Xp = X;
        Em = Ec[1]; En = En2; Eo = Eo2; Eb = Eb2;
#pragma unroll
        for (int a = 0; a < 3; a++) { Mc[a] = M[a]; Lm[a] = La[a]; Dv[a] = Da[a]; Ec[a] = E2[a]; }
        Hf = Hfa; Hb = Hba;
        q++;
    };
    while (q <= kend) {
        phase(A, B, C);
        if (q > kend) break;
        phase(B, C, A);
        if (q > kend) break;
        phase(C, A, B);
    }
}

// ---- the same fusion with TWO rows per thread ----------------------------------------------------
// jacobi_march2_kernel evaluates L1 on three rows to produce L2 on one: the two outer rows are what the
// neighbouring waves compute as their own centre.  Here a thread owns the float4 columns of rows j and j + 1: L0
// of the rows j-1 .. j+2 on three planes in registers, L1 on those four rows, L2 on the two inner ones -- four L1
// evaluations for two outputs instead of three for one, and 10 float4 loads (rows j-2 .. j+3 of p, j-1 .. j+2 of
// div) for two outputs instead of 8 for one.  Same expression per value, so bit-identical to the other sweep
// kernels.  One wave per row (nx <= 256).  Preconditions as for jacobi_march2_kernel.
template <int WAVES, bool WIDE>
__global__ __launch_bounds__(WAVES * 64) void jacobi_march2r_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                    float *__restrict__ out, int nx, int ny, int nz,
                                                                    int cw, int nby, int kchunk, float alpha, float beta, Slab sl, PairRanges rg)
{
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);      // XCD-contiguous block order
    const int by = b % nby, bz = b / nby;
    const int rows = (WAVES * 64) / cw;
    const int c = threadIdx.x % cw, r = threadIdx.x / cw;
    const int xraw = 4 * c, j = 2 * (by * rows + r);
    const int kA = max(1, 1 - sl.koff), kB = min(nz - 1, sl.nkg - 1 - sl.koff);
    const int r0 = bz < rg.nchA ? rg.k0a + bz * kchunk : rg.k0b + (bz - rg.nchA) * kchunk, r1 = bz < rg.nchA ? rg.k1a : rg.k1b;
    const int kbeg = max(kA, r0), kend = min(min(kB, r1), r0 + kchunk);
    if (kbeg >= kend) return;
    const bool xok = xraw < nx;
    const bool active0 = xok && j >= 1 && j <= ny - 2, active1 = xok && j + 1 >= 1 && j + 1 <= ny - 2;
    // out-of-range rows, planes and lanes are clamped into the array (see jacobi_march2_kernel)
    const int x = xok ? xraw : nx - 4;
    const size_t sj = nx, sk = (size_t)nx * ny;
    const bool xlo = x == 0, xhi = x + 3 == nx - 1;
    auto rowat = [&](int col, int row) -> size_t { return (size_t)min(max(col, 0), nx - 1) + sj * (size_t)min(max(row, 0), ny - 1); };
    const size_t o_m2 = rowat(x, j - 2), o_p3 = rowat(x, j + 3);
    size_t o[4];
    bool rowb[4];
#pragma unroll
    for (int a = 0; a < 4; a++) { o[a] = rowat(x, j - 1 + a); rowb[a] = j - 1 + a <= 0 || j - 1 + a >= ny - 1; }
    // WIDE (a row spans several waves): the edge lanes look after the cell just outside their wave, on both rows --
    // the scheme of jacobi_march2_kernel, twice
    const int lane = threadIdx.x & 63;
    const bool edgeL = WIDE && lane == 0 && xok && xraw > 0, edgeR = WIDE && lane == 63 && xraw + 4 < nx;
    const bool edge = edgeL || edgeR;
    const int xe = edgeL ? xraw - 1 : xraw + 4, xo = edgeL ? xe - 1 : xe + 1;
    size_t e[4], eo[2];
#pragma unroll
    for (int a = 0; a < 4; a++) e[a] = rowat(xe, j - 1 + a);
    eo[0] = rowat(xo, j); eo[1] = rowat(xo, j + 1);
    const bool xe_boundary = xe <= 0 || xe >= nx - 1;
    auto plane = [&](int pl) -> size_t { return sk * (size_t)min(max(pl, 0), nz - 1); };
    auto ld4 = [&](const float *ptr, size_t off) -> float4 { return *reinterpret_cast<const float4 *>(ptr + off); };
    auto jac = [&](float4 ce, float4 fr, float4 bk, float4 dn, float4 up, float4 dv, float outside, bool boundary) -> float4 {
        float left = lane_up(ce.w), right = lane_down(ce.x);
        if (WIDE) {
            if (lane == 0) left = outside;
            if (lane == 63) right = outside;
        }
        float4 v;
        v.x = (left + ce.y + fr.x + bk.x + dn.x + up.x + alpha * dv.x) * beta;
        v.y = (ce.x + ce.z + fr.y + bk.y + dn.y + up.y + alpha * dv.y) * beta;
        v.z = (ce.y + ce.w + fr.z + bk.z + dn.z + up.z + alpha * dv.z) * beta;
        v.w = (ce.z + right + fr.w + bk.w + dn.w + up.w + alpha * dv.w) * beta;
        if (boundary) return ce;
        if (xlo) v.x = ce.x;
        if (xhi) v.w = ce.w;
        return v;
    };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 A[4], B[4], C[4], Dv[4], Hf, Hb;
    int q = kbeg - 1;
    // the outside cell: L0 on rows j-1 .. j+2 at plane q (Ec), on rows j, j+1 at planes q-1 / q+1 (Em / En), its outer
    // x-neighbour (Eo) and its div (Eb) on rows j, j+1 at plane q; Xp: its L1 on rows j, j+1 at plane q-1
    float Ec[4] = { 0.f, 0.f, 0.f, 0.f }, Em[2] = { 0.f, 0.f }, En[2] = { 0.f, 0.f }, Eo[2] = { 0.f, 0.f }, Eb[2] = { 0.f, 0.f }, Xp[2] = { 0.f, 0.f };
    {
        const size_t pm = plane(q - 1), pc = plane(q), pn = plane(q + 1);
#pragma unroll
        for (int a = 0; a < 4; a++) { A[a] = ld4(p, pm + o[a]); B[a] = ld4(p, pc + o[a]); C[a] = ld4(p, pn + o[a]); Dv[a] = ld4(div, pc + o[a]); }
        Hf = ld4(p, pc + o_m2); Hb = ld4(p, pc + o_p3);
        if (edge) {
#pragma unroll
            for (int a = 0; a < 4; a++) Ec[a] = p[pc + e[a]];
#pragma unroll
            for (int rr = 0; rr < 2; rr++) { Em[rr] = p[pm + e[rr + 1]]; En[rr] = p[pn + e[rr + 1]]; Eo[rr] = p[pc + eo[rr]]; Eb[rr] = div[pc + e[rr + 1]]; }
        }
    }
    float4 Mc[4] = { zero4, zero4, zero4, zero4 };      // L1 on plane q-1, rows j-1 .. j+2
    float4 Mm[2] = { zero4, zero4 };                    // L1 of rows j, j+1 on plane q-2
    float4 Dprev[2] = { zero4, zero4 };                 // div of rows j, j+1 on plane q-1
    auto phase = [&](float4 (&Lm)[4], float4 (&Lc)[4], float4 (&Ln)[4]) {
        const size_t pa = plane(q + 2), pb = plane(q + 1);
        float4 La[4], Da[4];
#pragma unroll
        for (int a = 0; a < 4; a++) { La[a] = ld4(p, pa + o[a]); Da[a] = ld4(div, pb + o[a]); }
        const float4 Hfa = ld4(p, pb + o_m2), Hba = ld4(p, pb + o_p3);
        float E2[4] = { 0.f, En[0], En[1], 0.f }, En2[2] = { 0.f, 0.f }, Eo2[2] = { 0.f, 0.f }, Eb2[2] = { 0.f, 0.f };
        if (edge) {
            E2[0] = p[pb + e[0]]; E2[3] = p[pb + e[3]];
#pragma unroll
            for (int rr = 0; rr < 2; rr++) { En2[rr] = p[pa + e[rr + 1]]; Eo2[rr] = p[pb + eo[rr]]; Eb2[rr] = div[pb + e[rr + 1]]; }
        }
        const bool qb = q < kA || q >= kB;
        float4 M[4];
        M[0] = jac(Lc[0], Hf, Lc[1], Lm[0], Ln[0], Dv[0], Ec[0], qb || rowb[0]);
        M[1] = jac(Lc[1], Lc[0], Lc[2], Lm[1], Ln[1], Dv[1], Ec[1], qb || rowb[1]);
        M[2] = jac(Lc[2], Lc[1], Lc[3], Lm[2], Ln[2], Dv[2], Ec[2], qb || rowb[2]);
        M[3] = jac(Lc[3], Lc[2], Hb, Lm[3], Ln[3], Dv[3], Ec[3], qb || rowb[3]);
        // L1 of the outside cell on rows j, j+1 at plane q (edge lanes; a boundary cell keeps L0)
        float X[2] = { Ec[1], Ec[2] };
        if (edge) {
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                if (qb || rowb[rr + 1] || xe_boundary) continue;
                const float l = edgeL ? Eo[rr] : Lc[rr + 1].w, rg2 = edgeL ? Lc[rr + 1].x : Eo[rr];
                X[rr] = (l + rg2 + Ec[rr] + Ec[rr + 2] + Em[rr] + En[rr] + alpha * Eb[rr]) * beta;
            }
        }
        const int k = q - 1;
        const float4 o0 = jac(Mc[1], Mc[0], Mc[2], Mm[0], M[1], Dprev[0], Xp[0], false);
        const float4 o1 = jac(Mc[2], Mc[1], Mc[3], Mm[1], M[2], Dprev[1], Xp[1], false);
        if (k >= kbeg && k < kend) {
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                if (!(rr ? active1 : active0)) continue;
                const float4 v = rr ? o1 : o0;
                float *dst = out + (size_t)x + sj * (j + rr) + sk * k;
                if (x >= 4 && x + 4 < nx) {
                    *reinterpret_cast<float4 *>(dst) = v;
                } else {
                    if (x >= 1) dst[0] = v.x;
                    dst[1] = v.y;
                    dst[2] = v.z;
                    if (x + 3 < nx - 1) dst[3] = v.w;
                }
            }
        }
        Mm[0] = Mc[1]; Mm[1] = Mc[2];
        Dprev[0] = Dv[1]; Dprev[1] = Dv[2];
#pragma unroll
        for (int rr = 0; rr < 2; rr++) { Xp[rr] = X[rr]; Em[rr] = Ec[rr + 1]; En[rr] = En2[rr]; Eo[rr] = Eo2[rr]; Eb[rr] = Eb2[rr]; }
#pragma unroll
        for (int a = 0; a < 4; a++) { Mc[a] = M[a]; Lm[a] = La[a]; Dv[a] = Da[a]; Ec[a] = E2[a]; }
        Hf = Hfa; Hb = Hba;
        q++;
    };
    while (q <= kend) {
        phase(A, B, C);
        if (q > kend) break;
        phase(B, C, A);
        if (q > kend) break;
        phase(C, A, B);
    }
}

// ---- the two-row fused kernel again, written for the instruction count --------------------------------------------
// jacobi_lean2r_kernel is sweep_lean2r_kernel<PackF4, WIDE, PF> (bq_sweep_pack.hip.h, shared with the fp64 smoother) on the
// plane ranges of a z-slab launch.  Rows of one wave (nx <= 256) or, WIDE, of 2-4 waves.
struct SlabPairs {
    Slab sl;
    PairRanges rg;
    __device__ __forceinline__ int kA() const { return max(1, 1 - sl.koff); }
    __device__ __forceinline__ int kB(int nz) const { return min(nz - 1, sl.nkg - 1 - sl.koff); }
    __device__ __forceinline__ int r0(int bz, int kchunk) const { return bz < rg.nchA ? rg.k0a + bz * kchunk : rg.k0b + (bz - rg.nchA) * kchunk; }
    __device__ __forceinline__ int r1(int bz) const { return bz < rg.nchA ? rg.k1a : rg.k1b; }
};

// ---- THREE sweeps per launch (rows of one wave, whole array) ---------------------------------------------------------
// With the lean plumbing the two-sweep kernel is bound by the fabric again (6.9 TB/s of real traffic at 256^3); what is
// left is to move fewer bytes per sweep.  Same scheme, one level deeper: a thread owns the float4 columns of rows j, j+1
// and keeps, in rings of four planes with compile-time indices,
//     L0 on rows j-2 .. j+3 (+ rows j-3, j+4 of the centre plane),  L1 on rows j-2 .. j+3,  L2 on rows j-1 .. j+2,
//     div on rows j-2 .. j+3;
// per plane q it makes L1(q) on six rows, L2(q-1) on four, L3(q-2) on its two -- 12 evaluations and 14 float4 loads for
// two outputs of three sweeps (two sweeps: 6 and 10 for two).  ~400 registers: one wave per SIMD.  Every value is
// jacobi_kernel's expression, planes and rows outside the interior keep their input through all three levels, so the
// result is bit-identical to three single sweeps.  Preconditions as for the two-sweep kernels.
template <int PF>
__global__ __launch_bounds__(256) void jacobi_lean3r_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                            float *__restrict__ out, int nx, int ny, int nz,
                                                            int cw, int nby, int kchunk, float alpha, float beta, Slab sl)
{
    constexpr int P = 3 + PF;                                       // ring period; loads run PF planes ahead
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);      // XCD-contiguous block order
    const int by = b % nby, bz = b / nby;
    const int rows = 256 / cw;
    const int c = threadIdx.x % cw;
    const int r = cw >= 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / cw) : (int)threadIdx.x / cw;   // (see the two-sweep kernel)
    const int xraw = 4 * c, j = 2 * (by * rows + r);
    const int kA = max(1, 1 - sl.koff), kB = min(nz - 1, sl.nkg - 1 - sl.koff);
    const int kbeg = max(kA, bz * kchunk), kend = min(kB, bz * kchunk + kchunk);
    if (kbeg >= kend) return;
    const bool xok = xraw < nx;
    const bool active0 = xok && j >= 1 && j <= ny - 2, active1 = xok && j + 1 >= 1 && j + 1 <= ny - 2;
    const int x = xok ? xraw : nx - 4;
    const bool xlo = x == 0, xhi = x + 3 == nx - 1;
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * 4u;
    const v4i rp = make_rsrc4(p, bytes), rd = make_rsrc4(div, bytes), ro = make_rsrc4(out, bytes);
    unsigned vo[8];                                                 // rows j-3 .. j+4
    bool rowb[6];                                                   // rows j-2 .. j+3 are boundary rows
#pragma unroll
    for (int a = 0; a < 8; a++) vo[a] = ((unsigned)x + (unsigned)nx * (unsigned)min(max(j - 3 + a, 0), ny - 1)) * 4u;
#pragma unroll
    for (int a = 0; a < 6; a++) rowb[a] = j - 2 + a <= 0 || j - 2 + a >= ny - 1;
    const bool edge_block = 2 * by * rows - 2 <= 0 || 2 * (by * rows + rows - 1) + 3 >= ny - 1;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * 4u;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    auto run = [&](auto EDGE_T) {
    constexpr bool EDGE = decltype(EDGE_T)::value;
    // rings indexed by (iteration + distance) mod P, all compile-time inside the unrolled loop:
    //   L0: planes q-1, q, q+1 .. q+PF live, q+1+PF arriving;  H (rows j-3, j+4) and D: q .. q+PF-1 (D also q-1, q-2), q+PF arriving;
    //   L1: q (being made), q-1, q-2;  L2: q-1 (being made), q-2, q-3
    R4 L0[P][6], H[P][2], L1[P][6], L2[P][4], D[P][6];
    const R4 zero = R4{v2f{0.f, 0.f}, v2f{0.f, 0.f}};
#pragma unroll
    for (int a = 0; a < P; a++) {
#pragma unroll
        for (int bb = 0; bb < 6; bb++) { L1[a][bb] = zero; D[a][bb] = zero; }
#pragma unroll
        for (int bb = 0; bb < 4; bb++) L2[a][bb] = zero;
    }
    int q = kbeg - 2;
#pragma unroll
    for (int d = -1; d <= PF; d++) {                                // prologue: planes q-1 .. q+PF
        const int sl_ = ring_slot(0, d, P);
        const unsigned pp = po(q + d);
#pragma unroll
        for (int a = 0; a < 6; a++) L0[sl_][a] = ld_r4(rp, vo[a + 1], pp);
        if (d >= 0 && d < PF) {
#pragma unroll
            for (int a = 0; a < 6; a++) D[sl_][a] = ld_r4(rd, vo[a + 1], pp);
            H[sl_][0] = ld_r4(rp, vo[0], pp); H[sl_][1] = ld_r4(rp, vo[7], pp);
        }
    }
#define BQ_LEAN3_PHASE(T)                                                                                           \
    {                                                                                                               \
        constexpr int im = ring_slot(T, -1, P), ic = ring_slot(T, 0, P), in_ = ring_slot(T, 1, P), ia = ring_slot(T, 1 + PF, P);  /* L0 */    \
        constexpr int hc = ring_slot(T, 0, P), ha = ring_slot(T, PF, P);                                                        \
        constexpr int a0 = ring_slot(T, 0, P), a1 = ring_slot(T, -1, P), a2 = ring_slot(T, -2, P);             /* L1: q, q-1, q-2 */    \
        constexpr int b1 = ring_slot(T, -1, P), b2 = ring_slot(T, -2, P), b3 = ring_slot(T, -3, P);            /* L2: q-1, q-2, q-3 */  \
        constexpr int d0 = ring_slot(T, 0, P), d1 = ring_slot(T, -1, P), d2 = ring_slot(T, -2, P);                                    \
        const unsigned pa = po(q + 1 + PF), pb = po(q + PF);                                                        \
        _Pragma("unroll") for (int a = 0; a < 6; a++) { L0[ia][a] = ld_r4(rp, vo[a + 1], pa); D[ha][a] = ld_r4(rd, vo[a + 1], pb); } \
        H[ha][0] = ld_r4(rp, vo[0], pb); H[ha][1] = ld_r4(rp, vo[7], pb);                                           \
        if (q < kA || q >= kB) {                                /* first sweep on plane q, rows j-2 .. j+3 */        \
            _Pragma("unroll") for (int a = 0; a < 6; a++) L1[a0][a] = L0[ic][a];                                      \
        } else {                                                                                                    \
            /* alpha * div once per value: this plane's first sweep and the later sweeps on it reuse the product */   \
            _Pragma("unroll") for (int a = 0; a < 6; a++) { D[d0][a].a = alpha * D[d0][a].a; D[d0][a].b = alpha * D[d0][a].b; } \
            _Pragma("unroll") for (int a = 0; a < 6; a++) {                                                          \
                const R4 fr = a == 0 ? H[hc][0] : L0[ic][a == 0 ? 0 : a - 1], bk = a == 5 ? H[hc][1] : L0[ic][a == 5 ? 5 : a + 1]; \
                L1[a0][a] = jac_r4<false, true>(L0[ic][a], fr, bk, L0[im][a], L0[in_][a], D[d0][a], alpha, beta, xlo, xhi); \
                if (EDGE && rowb[a]) L1[a0][a] = L0[ic][a];                                                         \
            }                                                                                                       \
        }                                                                                                           \
        if (q - 1 < kA || q - 1 >= kB) {                        /* second sweep on plane q-1, rows j-1 .. j+2 */     \
            _Pragma("unroll") for (int a = 0; a < 4; a++) L2[b1][a] = L1[a1][a + 1];                                  \
        } else {                                                                                                    \
            _Pragma("unroll") for (int a = 0; a < 4; a++) {                                                          \
                L2[b1][a] = jac_r4<false, true>(L1[a1][a + 1], L1[a1][a], L1[a1][a + 2], L1[a2][a + 1], L1[a0][a + 1], D[d1][a + 1], alpha, beta, xlo, xhi); \
                if (EDGE && rowb[a + 1]) L2[b1][a] = L1[a1][a + 1];                                                 \
            }                                                                                                       \
        }                                                                                                           \
        const int k = q - 2;                                                                                        \
        if (k >= kbeg && k < kend) {                            /* third sweep on plane q-2, rows j, j+1: stored */  \
            const R4 o0 = jac_r4<false, true>(L2[b2][1], L2[b2][0], L2[b2][2], L2[b3][1], L2[b1][1], D[d2][2], alpha, beta, xlo, xhi); \
            const R4 o1 = jac_r4<false, true>(L2[b2][2], L2[b2][1], L2[b2][3], L2[b3][2], L2[b1][2], D[d2][3], alpha, beta, xlo, xhi); \
            const unsigned pk = pstride * (unsigned)k;                                                              \
            if (active0) st_r4(o0, ro, vo[3], pk);                                                                  \
            if (active1) st_r4(o1, ro, vo[4], pk);                                                                  \
        }                                                                                                           \
        q++;                                                                                                        \
    }
    while (true) {
        BQ_LEAN3_PHASE(0)
        if (q > kend + 1) break;
        BQ_LEAN3_PHASE(1)
        if (q > kend + 1) break;
        BQ_LEAN3_PHASE(2)
        if (q > kend + 1) break;
        BQ_LEAN3_PHASE(3)
        if (q > kend + 1) break;
        if constexpr (P > 4) {
            BQ_LEAN3_PHASE(4)
            if (q > kend + 1) break;
        }
    }
    };
    if (edge_block) run(std::true_type{}); else run(std::false_type{});
#undef BQ_LEAN3_PHASE
}

// Obstacles (MASK = true; bq_obstacle.hip).  solid: one byte per cell, 0 = fluid; rows: one byte per
// (row, plane), 1 when a solid cell lies in rows j-1 .. j+1 of planes k-1 .. k+1; b0 .. b6: beta_s for s solid neighbours.
struct SweepMask { const unsigned char *solid = nullptr, *rows = nullptr; float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, b4 = 0.f, b5 = 0.f, b6 = 0.f; };
// Closed domain walls (WALLS = true).  solid: the obstacle flags plus BQ_FLAG_WALL in the wall cells; rows:
// still the summary of the OBSTACLE flags; walls: the closed sides (BQ_WALL_* bits).
struct SweepMaskWalls : SweepMask { int walls = 0; };
// ... on a z-slab rank (SLABZ = true).  wzl, wzh: the LOCAL plane with a closed z side below / above it -- global plane 1 /
// nkg - 2 -- or -8 where that side is open or the plane lies in another rank's array (walls_z_planes: formed on the host)
struct SweepMaskWallsZ : SweepMaskWalls { int wzl = -8, wzh = -8; };
template <bool WALLS, typename M> __device__ __forceinline__ int walls_of(const M &m) { if constexpr (WALLS) return m.walls; else return 0; }

// Per cell of a float4 column a code byte: 7 = solid, else s = the number of solid neighbours.  own / lw / rw: the flag words
// (one byte per cell) of the column, of the column to the left (lane - 1) and to the right (lane + 1); yl, yh, zl, zh: of
// the same column in the neighbouring rows and planes.  Computed once per (row, plane), when the plane's level 1 is formed.
__device__ __forceinline__ unsigned mask_code(unsigned own, unsigned lw, unsigned rw, unsigned yl, unsigned yh, unsigned zl, unsigned zh)
{
    unsigned code = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const unsigned lb = c == 0 ? lw >> 24 : own >> (8 * (c - 1));
        const unsigned rb = c == 3 ? rw : own >> (8 * (c + 1));
        const unsigned n = ((lb & 255u) != 0) + ((rb & 255u) != 0) + (((yl >> (8 * c)) & 255u) != 0) + (((yh >> (8 * c)) & 255u) != 0)
                         + (((zl >> (8 * c)) & 255u) != 0) + (((zh >> (8 * c)) & 255u) != 0);
        code |= (((own >> (8 * c)) & 255u) ? 7u : n) << (8 * c);
    }
    return code;
}
// the masked sweep's value from the UNSCALED sum (jac_r4 with beta = 1: the same float as the sum): solid cells keep `ce`, a
// cell with s solid neighbours takes sum * beta_s (s = 6: 0), x-boundary cells keep `ce`
__device__ __forceinline__ float mask_one(float sum, float ce, unsigned k, const SweepMask &mk)
{
    const float bs = k == 0 ? mk.b0 : k == 1 ? mk.b1 : k == 2 ? mk.b2 : k == 3 ? mk.b3 : k == 4 ? mk.b4 : mk.b5;
    return k == 7 ? ce : (k == 6 ? 0.f : sum * bs);
}
__device__ __forceinline__ R4 mask_finish(R4 sum, R4 ce, unsigned code, const SweepMask &mk, bool xlo, bool xhi)
{
    R4 o;
    o.a.x = xlo ? ce.a.x : mask_one(sum.a.x, ce.a.x, code & 255u, mk);
    o.a.y = mask_one(sum.a.y, ce.a.y, (code >> 8) & 255u, mk);
    o.b.x = mask_one(sum.b.x, ce.b.x, (code >> 16) & 255u, mk);
    o.b.y = xhi ? ce.b.y : mask_one(sum.b.y, ce.b.y, code >> 24, mk);
    return o;
}

// ---- THREE sweeps per launch, the intermediate levels' neighbour rows exchanged through LDS (round 3) ------------------
// jacobi_lean3r_kernel is bound by instruction ISSUE: a thread that owns rows j, j+1 evaluates the first sweep on six rows and
// the second on four to produce the third on two -- 12 evaluations for 6 useful ones -- and its ~400 registers leave one wave
// per SIMD, where an instruction costs ~5 cycles instead of ~2.5.  Here every wave evaluates each level on ITS OWN two rows
// only and fetches the two neighbouring rows of the level below from LDS, where the waves that own them have put them:
//   block = W + 2 waves: W row pairs that produce output + one HALO wave at either end, which evaluates the first two levels
//           on the two rows outside the block (the block's edge pairs need them) and stores nothing;
//   per plane step q, per wave: L1(q) on its rows -> LDS A[q & 1]; L2(q-1) on its rows from L1(q-1) (own rows: registers,
//           rows j-1, j+2: A[(q-1) & 1]) -> LDS B[(q-1) & 1]; L3(q-2) from L2(q-2) (own: registers, neighbours: B[q & 1]) ->
//           global; ONE barrier.  Each buffer written in step q was last read in step q-1, before that step's barrier.
// 6 evaluations and 6 float4 loads per plane and wave instead of 12 and 14, ~190 registers: two waves per SIMD.  Every value
// is jacobi_kernel's expression on the same operands, boundary rows / planes / columns keep their input through all three
// levels: bit-identical to three single sweeps (and to the other fused kernels).  Rows of one wave, whole arrays; same
// precondition as the other fused kernels (both buffers carry the same boundary layer).
// R: rows per wave (2: a wave owns a row pair and has one neighbour row of each level in its own registers; 1: one row per
// wave, both neighbour rows come from LDS -- twice the waves for the same work).  S: sweeps per launch (3 or 4): level s is
// needed S - s rows outside the block, so a block carries H = ceil((S - 1) / R) halo waves at either end; a chunk marches
// 2 (S - 1) warm-up planes.  All rings have period 4 (planes q-1, q, q+1 of the input live, q+2 arriving; three planes of every
// intermediate level; div of the S planes the levels are working on -- with S = 4 the slot of the oldest one is refilled at
// the END of the step, after the last level has used it).
// A halo wave whose nearest row lies dn rows outside the block owes the block levels 1 .. S - dn only: the march is instantiated
// once per level count and a block's waves run different code between the same barriers (S = 4 in row pairs: 11.4 -> 10.0 us
// per sweep at 256^3; S = 3 unchanged, 10.7 -- its waves wait for each other, not for the VALU).
// WALLS (with MASK): a block the rows summary finds clean still has wall cells next to its first and last
// interior column, row and plane.  Their number is a function of the position alone: such a block reads no flag and scales the
// unscaled sum by beta_s with s = [x wall] + [y wall] (per row: wave-uniform) + [z wall] (per plane) -- the floats mask_finish
// gives for the same s.  A dirty block takes the flag words (of solid + walls) as before.
// SLABZ (with WALLS): the z term by the GLOBAL plane, for z-slab ranks -- an instantiation of its own, so that the kernel of one
// domain stays the code it was (the same source with the two planes as kernel arguments measured 3 % slower there).
template <int W, int R, int S, bool MASK = false, bool WALLS = false, bool SLABZ = false>
__global__ __launch_bounds__((W + 2 * ((S - 1 + R - 1) / R)) * 64) void jacobi_lds_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                  float *__restrict__ out, int nx, int ny, int nz,
                                                                  int nby, int nblk, int kchunk, float alpha, float beta, Slab sl, PairRanges rg,
                                                                  std::conditional_t<SLABZ, SweepMaskWallsZ, std::conditional_t<WALLS, SweepMaskWalls, SweepMask>> mk)
{
    static_assert(WALLS || !SLABZ, "the slab form is a state of the walled kernel");
    static_assert((R == 1 || R == 2) && (S == 3 || S == 4), "one or two rows per wave, three or four sweeps per launch");
    static_assert(MASK || !WALLS, "walls are a state of the masked kernel");
    constexpr int H = (S - 1 + R - 1) / R, NW = W + 2 * H, NS = NW * R, P = 4, A = P - 2;   // A: the plane loaded in step q is q + A
    __shared__ v4f lds[S - 1][2][NS][64];                           // [level - 1][plane parity][row slot][lane]
    // XCD-contiguous block order: the grid is padded to a multiple of 8 blocks (nblk real ones), XCD x = blockIdx % 8 works
    // through its own run of consecutive (row block, chunk) pairs -- neighbouring row blocks share their halo rows in one L2
    const int per = (int)gridDim.x >> 3;
    const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
    if (b >= nblk) return;                                          // padding (block-uniform, before any barrier)
    const int by = b % nby, bz = b / nby;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int jb = by * (W * R);                                    // first output row of the block
    const int j = jb + R * (wv - H);                                // this wave's rows: j .. j + R - 1 (halo waves: outside the block)
    const bool halo = wv < H || wv >= NW - H;
    // a halo wave whose nearest row lies dn rows outside the block owes the block levels 1 .. S - dn only (wave-uniform)
    const int dn = wv < H ? R * (H - wv) - (R - 1) : (wv >= NW - H ? R * (wv - (NW - H)) + 1 : 0);
    const int smax = S - dn;
    const int kA = max(1, 1 - sl.koff), kB = min(nz - 1, sl.nkg - 1 - sl.koff);
    // output planes: chunk bz of plane range A or B (whole arrays: A = [0, nz), B empty)
    const int c0 = bz < rg.nchA ? rg.k0a + bz * kchunk : rg.k0b + (bz - rg.nchA) * kchunk, c1 = bz < rg.nchA ? rg.k1a : rg.k1b;
    const int kbeg = max(kA, c0), kend = min(min(kB, c1), c0 + kchunk);
    if (kbeg >= kend) return;                                       // (block-uniform: no barrier is skipped by part of a block)
    const int xraw = 4 * lane;
    const bool xok = xraw < nx;
    const int x = xok ? xraw : nx - 4;                              // out-of-range lanes, rows, planes: clamped into the array
    const bool xlo = x == 0, xhi = x + 3 == nx - 1;
    bool active[R], rowb[R];                                        // rowb: boundary (or outside) rows keep L0
#pragma unroll
    for (int a = 0; a < R; a++) {
        active[a] = xok && !halo && j + a >= 1 && j + a <= ny - 2;
        rowb[a] = j + a <= 0 || j + a >= ny - 1;
    }
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * 4u;
    const v4i rp = make_rsrc4(p, bytes), rd = make_rsrc4(div, bytes), ro = make_rsrc4(out, bytes);
    unsigned vo[R + 2];                                             // byte offsets of this thread's column in rows j-1 .. j+R
#pragma unroll
    for (int a = 0; a < R + 2; a++) vo[a] = ((unsigned)x + (unsigned)nx * (unsigned)min(max(j - 1 + a, 0), ny - 1)) * 4u;
    // only blocks that touch the first or last row of the grid (their halo rows included) pay the boundary-row selects
    const bool edge_block = jb - H * R <= 0 || jb + W * R + H * R - 1 >= ny - 1;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * 4u;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    // LDS rows: slot R wv + a holds row j + a; the neighbours j - 1 and j + R are the slots below and above (the outermost halo
    // row has no neighbour on its far side: it reads a clamped slot, and what it computes from that is never used)
    const int r0 = R * wv, rlo = max(r0 - 1, 0), rhi = min(r0 + R, NS - 1);
    auto put = [&](v4f (*buf)[64], int a, R4 v) { buf[r0 + a][lane] = v4f{v.a.x, v.a.y, v.b.x, v.b.y}; };
    auto get = [&](v4f (*buf)[64], int r) -> R4 { const v4f v = buf[r][lane]; return R4{v2f{v.x, v.y}, v2f{v.z, v.w}}; };

    // masked blocks: the flag words of this thread's column in row `row` of plane `pl` and the masked value of a level there
    // (rows and planes clamped into the array: what a clamped neighbour contributes is never used -- boundary rows and
    // planes keep their input)
    const size_t fplane = (size_t)nx * (size_t)ny;
    auto fword = [&](int row, int pl) -> unsigned {
        return *(const unsigned *)(mk.solid + (size_t)x + (size_t)nx * (size_t)min(max(row, 0), ny - 1) + fplane * (size_t)min(max(pl, 0), nz - 1));
    };
    auto code_of = [&](unsigned own, unsigned yl, unsigned yh, unsigned zl, unsigned zh) -> unsigned {
        return mask_code(own, __shfl_up(own, 1), __shfl_down(own, 1), yl, yh, zl, zh);
    };
    auto run = [&](auto EDGE_T, auto SM_T, auto MASK_T) __attribute__((always_inline)) {
    constexpr bool EDGE = decltype(EDGE_T)::value;
    constexpr bool MK = decltype(MASK_T)::value == 1;               // this block lies near a solid cell
    constexpr bool PW = decltype(MASK_T)::value == 2;               // clean, walls on: solid neighbours by position
    constexpr int SM = decltype(SM_T)::value;                       // the levels this wave evaluates (halo waves: fewer than S)
    R4 L0[P][R + 2], D[P][R], Lv[S][P][R];                          // Lv[s]: level s (1 .. S-1) on the wave's own rows
    // masked blocks: flag words of rows j-1 .. j+R in the same ring as L0 (loaded with it, A planes ahead), and the code
    // words (mask_code) of the own rows per plane, formed with level 1 and reused by the later levels of that plane
    unsigned Fw[P][R + 2], Cd[P][R];
    const R4 zero = R4{v2f{0.f, 0.f}, v2f{0.f, 0.f}};
    // PW: the y term of the own rows (wave-uniform), the z term of a plane, and the finish of a level from its unscaled sum --
    // component .y of the xlo lane is cell 1, component .z of the xhi lane cell nx - 2; s <= 3 (nj >= 8, nk >= 12)
    int wy[R];
    bool wxl = false, wxh = false;
    int wzl = 0, wzh = 0;
    if constexpr (PW) {
        const int wl = walls_of<WALLS>(mk);
#pragma unroll
        for (int a = 0; a < R; a++) wy[a] = (int)((wl & 4) != 0 && j + a == 1) + (int)((wl & 8) != 0 && j + a == ny - 2);
        wxl = xlo && (wl & 1) != 0; wxh = xhi && (wl & 2) != 0;
        wzl = (wl & 16) != 0 ? 1 : -8; wzh = (wl & 32) != 0 ? nz - 2 : -8;      // the plane with a closed z side below / above it
        if constexpr (SLABZ) { wzl = mk.wzl; wzh = mk.wzh; }
    }
    auto pw_finish = [&](R4 sum, R4 ce, int a, int pl) -> R4 {
        const int n = wy[a] + (int)(pl == wzl) + (int)(pl == wzh);
        const float bu = n == 0 ? mk.b0 : n == 1 ? mk.b1 : mk.b2, bx = n == 0 ? mk.b1 : n == 1 ? mk.b2 : mk.b3;
        R4 o;
        o.a.x = xlo ? ce.a.x : sum.a.x * bu;
        o.a.y = sum.a.y * (wxl ? bx : bu);
        o.b.x = sum.b.x * (wxh ? bx : bu);
        o.b.y = xhi ? ce.b.y : sum.b.y * bu;
        return o;
    };
    if (MK) {
#pragma unroll
        for (int a = 0; a < P; a++)
#pragma unroll
            for (int c = 0; c < R; c++) Cd[a][c] = 0u;
    }
#pragma unroll
    for (int a = 0; a < P; a++)
#pragma unroll
        for (int c = 0; c < R; c++) {
            D[a][c] = zero;
#pragma unroll
            for (int l = 0; l < S; l++) Lv[l][a][c] = zero;
        }
    int q = kbeg - (S - 1);
#pragma unroll
    for (int d = -1; d <= A - 1; d++) {                             // prologue: planes q-1 .. q+A-1 of p; div of planes q .. q+A-2
        const int sl_ = ring_slot(0, d, P);
        const unsigned pp = po(q + d);
#pragma unroll
        for (int a = 0; a < R + 2; a++) L0[sl_][a] = ld_r4(rp, vo[a], pp);
        if (MK) {
#pragma unroll
            for (int a = 0; a < R + 2; a++) Fw[sl_][a] = fword(j - 1 + a, q + d);
        }
        if (d >= 0 && d <= A - 2) {
#pragma unroll
            for (int a = 0; a < R; a++) D[sl_][a] = ld_r4(rd, vo[a + 1], pp);
        }
    }
#define BQ_LDS_PHASE(T)                                                                                             \
    {                                                                                                               \
        constexpr int im = ring_slot(T, -1, P), ic = ring_slot(T, 0, P), in_ = ring_slot(T, 1, P), ia = ring_slot(T, A, P), id_ = ring_slot(T, A - 1, P); \
        const unsigned pa = po(q + A), pb = po(q + A - 1);                                                          \
        _Pragma("unroll") for (int a = 0; a < R + 2; a++) L0[ia][a] = ld_r4(rp, vo[a], pa);                           \
        if (MK) { _Pragma("unroll") for (int a = 0; a < R + 2; a++) Fw[ia][a] = fword(j - 1 + a, q + A); }               \
        if (MK) { _Pragma("unroll") for (int a = 0; a < R; a++) Cd[ic][a] = code_of(Fw[ic][a + 1], Fw[ic][a], Fw[ic][a + 2], Fw[im][a + 1], Fw[in_][a + 1]); } \
        if (S == 3) { _Pragma("unroll") for (int a = 0; a < R; a++) D[id_][a] = ld_r4(rd, vo[a + 1], pb); }           \
        /* the neighbour rows every later level of this step needs were put into LDS before the last barrier: fetch them   \
           all now, ahead of the first level's arithmetic (the compiler cannot hoist them over this step's own puts) */     \
        R4 nlo[S + 1], nhi[S + 1];                                                                                  \
        _Pragma("unroll") for (int s = 2; s <= SM; s++) {                                                            \
            nlo[s] = get(lds[s - 2][(q - (s - 1)) & 1], rlo); nhi[s] = get(lds[s - 2][(q - (s - 1)) & 1], rhi);     \
        }                                                                                                           \
        /* first sweep on plane q, own rows */                                                                       \
        if (q < kA || q >= kB) {                                                                                    \
            _Pragma("unroll") for (int a = 0; a < R; a++) Lv[1][ic][a] = L0[ic][a + 1];                               \
        } else {                                                                                                    \
            _Pragma("unroll") for (int a = 0; a < R; a++) {                                                          \
                D[ic][a].a = alpha * D[ic][a].a; D[ic][a].b = alpha * D[ic][a].b;                                   \
                if (MK) Lv[1][ic][a] = mask_finish(jac_r4<false, true, true>(L0[ic][a + 1], L0[ic][a], L0[ic][a + 2], L0[im][a + 1], L0[in_][a + 1], D[ic][a], alpha, 1.0f, false, false), L0[ic][a + 1], Cd[ic][a], mk, xlo, xhi); \
                else if (PW) Lv[1][ic][a] = pw_finish(jac_r4<false, true, true>(L0[ic][a + 1], L0[ic][a], L0[ic][a + 2], L0[im][a + 1], L0[in_][a + 1], D[ic][a], alpha, 1.0f, false, false), L0[ic][a + 1], a, q); \
                else Lv[1][ic][a] = jac_r4<false, true, true>(L0[ic][a + 1], L0[ic][a], L0[ic][a + 2], L0[im][a + 1], L0[in_][a + 1], D[ic][a], alpha, beta, xlo, xhi); \
                if (EDGE && rowb[a]) Lv[1][ic][a] = L0[ic][a + 1];                                                  \
            }                                                                                                       \
        }                                                                                                           \
        _Pragma("unroll") for (int a = 0; a < R; a++) put(lds[0][q & 1], a, Lv[1][ic][a]);                            \
        /* sweep s on plane q - (s - 1): rows j-1, j+R of level s-1 on that plane were put into LDS before the last barrier */ \
        _Pragma("unroll") for (int s = 2; s <= S; s++) {                                                             \
            const int ps = q - (s - 1);                                                                             \
            const int cs = ring_slot(T, -(s - 1), P), us = ring_slot(T, -(s - 2), P), ds = ring_slot(T, -s, P);                       \
            if (s <= SM && (s < S || (ps >= kbeg && ps < kend))) {   /* (a step without the two wave-uniform plane tests measured slower) */ \
                const bool keep = ps < kA || ps >= kB;                                                              \
                _Pragma("unroll") for (int a = 0; a < R; a++) {                                                      \
                    const R4 ce = Lv[s - 1][cs][a];                                                                 \
                    const R4 fr = a == 0 ? nlo[s] : Lv[s - 1][cs][a == 0 ? 0 : a - 1], bk = a == R - 1 ? nhi[s] : Lv[s - 1][cs][a == R - 1 ? a : a + 1]; \
                    R4 v = MK ? mask_finish(jac_r4<false, true, true>(ce, fr, bk, Lv[s - 1][ds][a], Lv[s - 1][us][a], D[cs][a], alpha, 1.0f, false, false), ce, Cd[cs][a], mk, xlo, xhi) \
                         : PW ? pw_finish(jac_r4<false, true, true>(ce, fr, bk, Lv[s - 1][ds][a], Lv[s - 1][us][a], D[cs][a], alpha, 1.0f, false, false), ce, a, ps) \
                              : jac_r4<false, true, true>(ce, fr, bk, Lv[s - 1][ds][a], Lv[s - 1][us][a], D[cs][a], alpha, beta, xlo, xhi); \
                    if (keep || (EDGE && rowb[a])) v = ce;                                                          \
                    if (s < S) { Lv[s][cs][a] = v; put(lds[s - 1][ps & 1], a, v); }                                 \
                    else if (active[a]) st_r4(v, ro, vo[a + 1], pstride * (unsigned)ps);                            \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        if (S == 4) { _Pragma("unroll") for (int a = 0; a < R; a++) D[id_][a] = ld_r4(rd, vo[a + 1], pb); }           \
        __syncthreads();                                                                                            \
        q++;                                                                                                        \
    }
    while (true) {
        BQ_LDS_PHASE(0)
        if (q > kend + S - 2) break;
        BQ_LDS_PHASE(1)
        if (q > kend + S - 2) break;
        BQ_LDS_PHASE(2)
        if (q > kend + S - 2) break;
        BQ_LDS_PHASE(3)
        if (q > kend + S - 2) break;
    }
    };
    // one instance of the march per number of levels: the waves of a block run different code between the same barriers
    auto go = [&](auto E, auto M) __attribute__((always_inline)) {
        if (smax >= S) run(E, std::integral_constant<int, S>{}, M);
        else if (smax == 1) run(E, std::integral_constant<int, 1>{}, M);
        else if (smax == 2) run(E, std::integral_constant<int, 2>{}, M);
        else run(E, std::integral_constant<int, 3>{}, M);
    };
    if constexpr (MASK) {
        // a block is clean when no solid cell lies within S cells of its output rows and planes (rows summary: already one
        // cell wide): then every value it computes equals the unmasked one, and it runs the unmasked stream
        const int r0 = max(jb - S, 0), r1 = min(jb + W * R + S, ny), k0 = max(kbeg - S, 0), k1 = min(kend + S, nz);
        const int nr = max(r1 - r0, 0), cnt = nr * max(k1 - k0, 0);
        int any = 0;
        for (int t = (int)threadIdx.x; t < cnt; t += (int)blockDim.x)
            any |= mk.rows[(size_t)(r0 + t % nr) + (size_t)ny * (size_t)(k0 + t / nr)];
        if (__syncthreads_or(any)) {
            if (edge_block) go(std::true_type{}, std::integral_constant<int, 1>{}); else go(std::false_type{}, std::integral_constant<int, 1>{});
            return;
        }
        if constexpr (WALLS) {                                      // clean, but never wall-free: the positional state
            if (edge_block) go(std::true_type{}, std::integral_constant<int, 2>{}); else go(std::false_type{}, std::integral_constant<int, 2>{});
            return;
        }
    }
    if (edge_block) go(std::true_type{}, std::integral_constant<int, 0>{}); else go(std::false_type{}, std::integral_constant<int, 0>{});
#undef BQ_LDS_PHASE
}

// ---- THREE sweeps per launch for rows of 260 .. 512 floats: two float4 segments per lane -----------------------------------
// jacobi_lds_kernel needs a row to fit one wave.  Here lane l holds the cells 4l .. 4l+3 (segment A) AND 256 + 4l .. 256 + 4l + 3
// (segment B) of its wave's row, so a 512-float row still belongs to ONE wave and every access is a coalesced 16-byte column;
// the x-neighbours across the seam travel through the adds' DPP operand with a wave rotation (lane 63 receives lane 0's cell
// 256, lane 0 lane 63's cell 255).  Twice the registers per row, so the neighbour rows of ALL levels come out of LDS -- the
// input too: a wave loads its own row only (the outermost halo waves also the one row beyond them) -- and twelve waves of 8
// output rows + two halo rows at either end fit three to a SIMD.  Same arithmetic, same boundary handling, same precondition
// as jacobi_lds_kernel; the fp64 smoother mg_lds3_kernel (bq_mgcg.hip) is this kernel's twin.
struct R8 { R4 a, b; };
__device__ __forceinline__ float add_rol(float from, float own)      // own + `from` of lane + 1 (lane 63: of lane 0)
{
    float r;
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 wave_rol:1 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(from), "v"(own));
    return r;
}
__device__ __forceinline__ float add_ror(float from, float own)      // own + `from` of lane - 1 (lane 0: of lane 63)
{
    float r;
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 wave_ror:1 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(from), "v"(own));
    return r;
}
// jacobi_kernel's expression on the eight cells of a lane; adv = alpha * div
__device__ __forceinline__ R8 jac_r8(R8 ce, R8 fr, R8 bk, R8 dn, R8 up, R8 adv, float beta, bool xlo, bool xhi, bool first, bool last)
{
    const float uR = first ? ce.b.a.x : ce.a.a.x;                   // lane 63's right neighbour: cell 256, lane 0's segment B
    const float uL = last ? ce.a.b.y : ce.b.b.y;                    // lane 0's left neighbour in segment B: cell 255, lane 63's segment A
    v2f s0 = v2f{add_from_left_lane(ce.a.b.y, ce.a.a.y), ce.a.a.x + ce.a.b.x};
    v2f s1 = v2f{ce.a.a.y + ce.a.b.y, add_rol(uR, ce.a.b.x)};
    v2f t0 = v2f{add_ror(uL, ce.b.a.y), ce.b.a.x + ce.b.b.x};
    v2f t1 = v2f{ce.b.a.y + ce.b.b.y, add_from_right_lane(ce.b.a.x, ce.b.b.x)};
    s0 = s0 + fr.a.a; s1 = s1 + fr.a.b; t0 = t0 + fr.b.a; t1 = t1 + fr.b.b;
    s0 = s0 + bk.a.a; s1 = s1 + bk.a.b; t0 = t0 + bk.b.a; t1 = t1 + bk.b.b;
    s0 = s0 + dn.a.a; s1 = s1 + dn.a.b; t0 = t0 + dn.b.a; t1 = t1 + dn.b.b;
    s0 = s0 + up.a.a; s1 = s1 + up.a.b; t0 = t0 + up.b.a; t1 = t1 + up.b.b;
    s0 = s0 + adv.a.a; s1 = s1 + adv.a.b; t0 = t0 + adv.b.a; t1 = t1 + adv.b.b;
    s0 = s0 * beta; s1 = s1 * beta; t0 = t0 * beta; t1 = t1 * beta;
    if (xlo) s0.x = ce.a.a.x;
    if (xhi) t1.y = ce.b.b.y;
    return R8{R4{s0, s1}, R4{t0, t1}};
}

template <int W>
__global__ __launch_bounds__((W + 4) * 64) void jacobi_lds2seg_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                      float *__restrict__ out, int nx, int ny, int nz,
                                                                      int nby, int nblk, int kchunk, float alpha, float beta, Slab sl, PairRanges rg)
{
    constexpr int S = 3, H = 2, NW = W + 2 * H, P = 4;
    __shared__ v4f lds[S][2][NW][2][64];                            // [level][plane parity][row slot][segment][lane]; level 0: the input
    const int per = (int)gridDim.x >> 3;                            // XCD-contiguous block order (grid padded to 8 k blocks)
    const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
    if (b >= nblk) return;
    const int by = b % nby, bz = b / nby;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int jb = by * W;
    const int j = jb + (wv - H);                                    // this wave's row (halo waves: outside the block)
    const bool halo = wv < H || wv >= NW - H;
    const int dn_rows = wv < H ? H - wv : (wv >= NW - H ? wv - (NW - H) + 1 : 0);
    const int smax = S - dn_rows;                                   // a halo wave dn rows outside owes levels 1 .. S - dn
    const bool low_end = wv == 0;
    const int kA = max(1, 1 - sl.koff), kB = min(nz - 1, sl.nkg - 1 - sl.koff);
    const int r0 = bz < rg.nchA ? rg.k0a + bz * kchunk : rg.k0b + (bz - rg.nchA) * kchunk, r1 = bz < rg.nchA ? rg.k1a : rg.k1b;
    const int kbeg = max(kA, r0), kend = min(min(kB, r1), r0 + kchunk);
    if (kbeg >= kend) return;                                       // (block-uniform)
    const int xA = 4 * lane, xBraw = 256 + 4 * lane;
    const bool okB = xBraw < nx;
    const int xB = okB ? xBraw : nx - 4;                            // out-of-range lanes, rows, planes: clamped into the array
    const bool xlo = lane == 0, xhi = okB && xBraw + 3 == nx - 1;
    const bool first = lane == 0, last = lane == 63;
    const bool row_in = !halo && j >= 1 && j <= ny - 2;
    const bool rowb = j <= 0 || j >= ny - 1;
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * 4u;
    const v4i rp = make_rsrc4(p, bytes), rd = make_rsrc4(div, bytes), ro = make_rsrc4(out, bytes);
    const unsigned row_own = (unsigned)nx * (unsigned)min(max(j, 0), ny - 1);
    const unsigned row_far = (unsigned)nx * (unsigned)min(max(low_end ? j - 1 : j + 1, 0), ny - 1);
    const unsigned voA = ((unsigned)xA + row_own) * 4u, voB = ((unsigned)xB + row_own) * 4u;
    const unsigned vfA = ((unsigned)xA + row_far) * 4u, vfB = ((unsigned)xB + row_far) * 4u;
    const bool edge_block = jb - H <= 0 || jb + W + H - 1 >= ny - 1;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * 4u;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    const int rlo = max(wv - 1, 0), rhi = min(wv + 1, NW - 1);
    auto put = [&](v4f (*buf)[2][64], R8 v) {
        buf[wv][0][lane] = v4f{v.a.a.x, v.a.a.y, v.a.b.x, v.a.b.y}; buf[wv][1][lane] = v4f{v.b.a.x, v.b.a.y, v.b.b.x, v.b.b.y};
    };
    auto get = [&](v4f (*buf)[2][64], int r) -> R8 {
        const v4f u = buf[r][0][lane], w = buf[r][1][lane];
        return R8{R4{v2f{u.x, u.y}, v2f{u.z, u.w}}, R4{v2f{w.x, w.y}, v2f{w.z, w.w}}};
    };
    const R4 z4 = R4{v2f{0.f, 0.f}, v2f{0.f, 0.f}};
    const R8 zero = R8{z4, z4};
    auto ld_own = [&](v4i rs, unsigned pp) -> R8 { return R8{ld_r4(rs, voA, pp), ld_r4(rs, voB, pp)}; };
    auto ld_far = [&](unsigned pp) -> R8 { return R8{ld_r4(rp, vfA, pp), ld_r4(rp, vfB, pp)}; };

    auto run = [&](auto EDGE_T, auto SM_T) __attribute__((always_inline)) {
    constexpr bool EDGE = decltype(EDGE_T)::value;
    constexpr int SM = decltype(SM_T)::value;                       // the levels this wave evaluates
    constexpr bool OUTER = SM == 1;                                 // an outermost halo wave
    R8 L0[P], Lx[P], D[P], L1[P], L2[P];
#pragma unroll
    for (int a = 0; a < P; a++) { D[a] = zero; L1[a] = zero; L2[a] = zero; Lx[a] = zero; }
    int q = kbeg - (S - 1);
#pragma unroll
    for (int d = -1; d <= 1; d++) {                                 // prologue: planes q-1, q, q+1 of p; div of plane q
        const int sl_ = ring_slot(0, d, P);
        const unsigned pp = po(q + d);
        L0[sl_] = ld_own(rp, pp);
        if (OUTER && d >= 0) Lx[sl_] = ld_far(pp);
        if (d == 0) D[sl_] = ld_own(rd, pp);
    }
    put(lds[0][q & 1], L0[ring_slot(0, 0, P)]);                           // the first step's centre plane for the neighbours
    __syncthreads();
#define BQ_L2S_PHASE(T)                                                                                             \
    {                                                                                                               \
        constexpr int im = ring_slot(T, -1, P), ic = ring_slot(T, 0, P), in_ = ring_slot(T, 1, P), ia = ring_slot(T, 2, P);                   \
        const unsigned pa = po(q + 2), pb = po(q + 1);                                                              \
        L0[ia] = ld_own(rp, pa);                                                                                    \
        if (OUTER) Lx[ia] = ld_far(pa);                                                                             \
        D[in_] = ld_own(rd, pb);                                                                                    \
        R8 fr0 = zero, bk0 = zero, nlo2 = zero, nhi2 = zero, nlo3 = zero, nhi3 = zero;                              \
        if (!OUTER || !low_end) fr0 = get(lds[0][q & 1], rlo);                                                      \
        if (!OUTER || low_end) bk0 = get(lds[0][q & 1], rhi);                                                       \
        if (OUTER) { if (low_end) fr0 = Lx[ic]; else bk0 = Lx[ic]; }                                                \
        put(lds[0][(q + 1) & 1], L0[in_]);                      /* the next step's centre plane */                   \
        /* first sweep on plane q */                                                                                \
        if (q < kA || q >= kB) {                                                                                    \
            L1[ic] = L0[ic];                                                                                        \
        } else {                                                                                                    \
            D[ic].a.a = alpha * D[ic].a.a; D[ic].a.b = alpha * D[ic].a.b;                                           \
            D[ic].b.a = alpha * D[ic].b.a; D[ic].b.b = alpha * D[ic].b.b;                                           \
            L1[ic] = jac_r8(L0[ic], fr0, bk0, L0[im], L0[in_], D[ic], beta, xlo, xhi, first, last);                 \
            if (EDGE && rowb) L1[ic] = L0[ic];                                                                      \
        }                                                                                                           \
        /* (the later levels' neighbour rows are fetched level by level: six rows in flight at once cost too many registers) */ \
        if (SM >= 2) { nlo2 = get(lds[1][(q - 1) & 1], rlo); nhi2 = get(lds[1][(q - 1) & 1], rhi); }                \
        put(lds[1][q & 1], L1[ic]);                                                                                 \
        if (SM >= 2) {      /* second sweep on plane q - 1 */                                                       \
            constexpr int cs = ring_slot(T, -1, P), us = ring_slot(T, 0, P), ds = ring_slot(T, -2, P);                                 \
            const int ps = q - 1;                                                                                   \
            R8 v = jac_r8(L1[cs], nlo2, nhi2, L1[ds], L1[us], D[cs], beta, xlo, xhi, first, last);                  \
            if (ps < kA || ps >= kB || (EDGE && rowb)) v = L1[cs];                                                  \
            L2[cs] = v;                                                                                             \
            if (SM >= 3) { nlo3 = get(lds[2][(q - 2) & 1], rlo); nhi3 = get(lds[2][(q - 2) & 1], rhi); }            \
            put(lds[2][ps & 1], v);                                                                                 \
        }                                                                                                           \
        if (SM >= 3) {      /* third sweep on plane q - 2 */                                                        \
            constexpr int cs = ring_slot(T, -2, P), us = ring_slot(T, -1, P), ds = ring_slot(T, -3, P);                                \
            const int ps = q - 2;                                                                                   \
            if (ps >= kbeg && ps < kend) {                                                                          \
                R8 v = jac_r8(L2[cs], nlo3, nhi3, L2[ds], L2[us], D[cs], beta, xlo, xhi, first, last);              \
                if (EDGE && rowb) v = L2[cs];                                                                       \
                if (row_in) {                                                                                       \
                    const unsigned pk = pstride * (unsigned)ps;                                                     \
                    st_r4<2>(v.a, ro, voA, pk);                                                                     \
                    if (okB) st_r4<2>(v.b, ro, voB, pk);                                                            \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        q++;                                                                                                        \
    }
    while (true) {
        BQ_L2S_PHASE(0)
        if (q > kend + S - 2) break;
        BQ_L2S_PHASE(1)
        if (q > kend + S - 2) break;
        BQ_L2S_PHASE(2)
        if (q > kend + S - 2) break;
        BQ_L2S_PHASE(3)
        if (q > kend + S - 2) break;
    }
    };
    auto go = [&](auto E) __attribute__((always_inline)) {
        if (smax >= S) run(E, std::integral_constant<int, S>{});
        else if (smax == 1) run(E, std::integral_constant<int, 1>{});
        else run(E, std::integral_constant<int, 2>{});
    };
    if (edge_block) go(std::true_type{}); else go(std::false_type{});
#undef BQ_L2S_PHASE
}

// ---- residual norms (A15 re-specified): r = div - (sum6 p - 6p), sum r^2 and max|r| --------
// update_residual_kernel / calc_poisson_value arithmetic (GPU_kernel.cu:1048-1060,1239-1249);
// the reduction is ours: wave64 shuffles -> one partial per block -> fixed-order final pass.
__global__ __launch_bounds__(256) void residual_partial_kernel(const float *__restrict__ div, const float *__restrict__ p,
                                                               int ni, int nj, int nk,
                                                               double *__restrict__ part_sum, float *__restrict__ part_max,
                                                               Slab sl, int own0, int own1)
{
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t total = sk * nk;
    double s = 0.0;
    float mx = 0.f;
    for (size_t id = (size_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (size_t)gridDim.x * 256) {
        const int i = (int)(id % sj), j = (int)((id / sj) % nj), k = (int)(id / sk);
        const int kg = k + sl.koff;
        if (i > 0 && i < ni - 1 && j > 0 && j < nj - 1 && kg > 0 && kg < sl.nkg - 1 && kg >= own0 && kg < own1 && k > 0 && k < nk - 1) {
            float ax = (p[id - 1] + p[id + 1] + p[id - sj] + p[id + sj] + p[id - sk] + p[id + sk]) - p[id] * 6;
            float r = div[id] - ax;
            s += (double)r * (double)r;
            mx = fmaxf(mx, fabsf(r));
        }
    }
    __shared__ double ssum[4];
    __shared__ float smax[4];
    s = wave_sum(s);
    mx = wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ssum[wave] = s; smax[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
        part_max[blockIdx.x] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

__global__ __launch_bounds__(256) void residual_final_kernel(const double *__restrict__ part_sum, const float *__restrict__ part_max,
                                                             int nparts, double *out_sum, float *out_max,
                                                             float *dbg_sum, float *dbg_max)
{
    double s = 0.0;
    float mx = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) { s += part_sum[i]; mx = fmaxf(mx, part_max[i]); }
    __shared__ double ssum[4];
    __shared__ float smax[4];
    s = wave_sum(s);
    mx = wave_max(mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { ssum[wave] = s; smax[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = ((ssum[0] + ssum[1]) + ssum[2]) + ssum[3];
        float m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        if (out_sum) *out_sum = tot;
        if (out_max) *out_max = m;
        if (dbg_sum) *dbg_sum = (float)tot;
        if (dbg_max) *dbg_max = m;
    }
}

// ---- diffuse_field_kernel (GPU_kernel.cu:834-853) ------------------------------------------
__global__ __launch_bounds__(256) void diffuse_kernel(const float *__restrict__ field, const float *__restrict__ in,
                                                      float *__restrict__ out, int ni, int nj, int nk, float coef,
                                                      int koff, int nkg)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    const int kg = k + koff;                    // nkg: GLOBAL plane count of this buffer
    if (!(i > 0 && i < ni - 1 && j > 0 && j < nj - 1 && k > 0 && k < nk - 1 && kg > 0 && kg < nkg - 1)) return;
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t id = (size_t)i + sj * j + sk * k;
    float s = in[id - 1] + in[id + 1] + in[id - sj] + in[id + sj] + in[id - sk] + in[id + sk];
    out[id] = (field[id] + coef * s) / (1.0f + 6.0f * coef);
}

static bool dims_ok(int ni, int nj, int nk, const char *op)
{
    if (ni < 1 || nj < 1 || nk < 1) { latch(FL_ERR_BAD_ARGUMENT, op, "non-positive grid dims"); return false; }
    double bytes = 4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1);
    if (bytes >= 4294967296.0) { latch(FL_ERR_BAD_ARGUMENT, op, "field larger than 4 GiB"); return false; }
    if (nk + 1 > 65535) { latch(FL_ERR_BAD_ARGUMENT, op, "nk too large for grid.z"); return false; }
    return true;
}

// the same limits for ONE BUFFER of ni x nj x nk floats: the diffusion sweeps run on a component's own dims, and the w component
// of the tallest grid has nk + 1 = 65535 planes, which dims_ok on buffer dims would turn away as a grid of 65536
static bool buffer_dims_ok(int ni, int nj, int nk, const char *op)
{
    if (ni < 1 || nj < 1 || nk < 1) { latch(FL_ERR_BAD_ARGUMENT, op, "non-positive buffer dims"); return false; }
    if (4.0 * (double)ni * (double)nj * (double)nk >= 4294967296.0) { latch(FL_ERR_BAD_ARGUMENT, op, "field larger than 4 GiB"); return false; }
    if (nk > 65535) { latch(FL_ERR_BAD_ARGUMENT, op, "nk too large for grid.z"); return false; }
    return true;
}

// per-context state of this file (bq_host.h: Runtime::project_state), behind the names it always had
struct SweepSpan { hipEvent_t a, b; long long launches, sweeps; };
struct ProjectState {
    const char *last_pair_kernel = "";      // name of the fused sweep kernel launched last; gpu_jacobi_sweeps: of the one it launched most (fl_jacobi_kernel_name)
    std::vector<SweepSpan> spans;           // FL_OPT_PROFILE_JACOBI
};
static ProjectState &ps()
{
    Runtime &r = rt();
    if (!r.project_state) r.project_state = new ProjectState();
    return *static_cast<ProjectState *>(r.project_state);
}
void project_release_state(Runtime &r)
{
    ProjectState *st = static_cast<ProjectState *>(r.project_state);
    if (!st) return;
    for (const SweepSpan &sp : st->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    delete st;
    r.project_state = nullptr;
}

// [klo, khi): the local planes a stencil launch is restricted to; default: the whole array
static inline Slab slab_of(int nk, int klo = 0, int khi = 1 << 30)
{
    const Runtime &r = rt();
    if (r.slab_on) return Slab{r.slab_koff, r.slab_nkg, klo, khi};
    return Slab{0, nk, klo, khi};
}
// the kernel argument and the chunk count of a launch that marches the ranges `pr` in chunks of kc planes
struct RangeLaunch { PairRanges rg; int nbz; };
static inline RangeLaunch range_launch(const geom::PlaneRanges &pr, int kc)
{
    const geom::PlaneRanges::Chunks c = pr.chunks(kc);
    return RangeLaunch{PairRanges{c.k0a, c.k1a, c.k0b, c.k1b, c.nchA}, c.nbz};
}

// The Jacobi tuning options of the current context, decoded (bq_jacobi_plan.h).  Once per entry-point call: the options are per
// context and may change between two calls.
plan::JacobiTuning jacobi_tuning()
{
    const Runtime &r = rt();
    return plan::decode_jacobi_tuning(r.opt_jacobi_variant, r.opt_jacobi_rows, r.opt_jacobi_kchunk, r.opt_jacobi_kchunk2, r.opt_jacobi_fuse);
}

// The launchers below ask bq_jacobi_plan.h which kernel, template arguments and geometry apply, switch on the answer and launch on
// the compute stream; every rule and the measurements behind it live with the planners.

// One Jacobi sweep in -> out, on the local planes [klo, khi) (default: the whole array).
static void jacobi_sweep(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                         float beta, int klo = 0, int khi = 1 << 30)
{
    const plan::LaunchPlan pl = plan::plan_single(ni, nj, nk, aligned16(in, div, out), tun);
    hipStream_t st = rt().compute;
    const Slab sl = slab_of(nk, klo, khi);
    switch (pl.kernel) {
    case plan::Kernel::kGeneric:
        jacobi_generic_kernel<<<grid_for(ni, nj, nk), kBlock, 0, st>>>(in, div, out, ni, nj, nk, alpha, beta, sl);
        BQ_LAUNCH_CHECK("jacobi_generic_kernel");
        return;
    case plan::Kernel::kMarch:
#define BQ_JM(W) jacobi_march_kernel<W><<<pl.grid, W * 64, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.col_blocks, pl.row_blocks, pl.kc, alpha, beta, sl)
        if (pl.W == 4) BQ_JM(4); else if (pl.W == 8) BQ_JM(8); else BQ_JM(16);
#undef BQ_JM
        BQ_LAUNCH_CHECK("jacobi_march_kernel");
        return;
    case plan::Kernel::kTile: {
        const dim3 grid(pl.col_blocks, pl.row_blocks, pl.nbz);
#define BQ_JT(TXV, RR) jacobi_tile_kernel<TXV, RR><<<grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.kc, alpha, beta, sl)
        if (pl.wide) { if (pl.R == 4) BQ_JT(64, 4); else if (pl.R == 2) BQ_JT(64, 2); else BQ_JT(64, 1); }
        else         { if (pl.R == 4) BQ_JT(32, 4); else if (pl.R == 2) BQ_JT(32, 2); else BQ_JT(32, 1); }
#undef BQ_JT
        BQ_LAUNCH_CHECK("jacobi_tile_kernel");
        return;
    }
    default: return;                                // no interior
    }
}

// The fused launch that `pl` describes: in -> out holds iterate + pl.S on the output planes `pr`.  false: the plan does not apply,
// nothing launched.  Records the kernel's name for fl_jacobi_kernel_name.  The caller guarantees that both buffers carry the same
// boundary layer.
static bool launch_fused(const plan::LaunchPlan &pl, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                         float beta, const geom::PlaneRanges &pr, const SweepMaskWallsZ *mask = nullptr)
{
    using plan::Kernel;
    if (pl.kernel == Kernel::kNone) return false;
    if (pl.kernel == Kernel::kEmpty) return true;
    hipStream_t st = rt().compute;
    const Slab sl = slab_of(nk);
    const PairRanges rg = range_launch(pr, pl.kc).rg;
    const char *name = "", *what = nullptr;             // the name reported, and the one an error message carries where it differs
    switch (pl.kernel) {
    case Kernel::kLean2r:
#define BQ_LEAN2R(W, F) sweep_lean2r_kernel<PackF4, W, F, false><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, SlabPairs{sl, rg})
        if (pl.wide) { if (pl.pf == 1) BQ_LEAN2R(true, 1); else BQ_LEAN2R(true, 2); }
        else         { if (pl.pf == 1) BQ_LEAN2R(false, 1); else BQ_LEAN2R(false, 2); }
#undef BQ_LEAN2R
        name = "jacobi_lean2r_kernel";
        break;
    case Kernel::kMarch2r:
        if (pl.wide) jacobi_march2r_kernel<4, true><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl, rg);
        else         jacobi_march2r_kernel<4, false><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl, rg);
        name = "jacobi_march2r_kernel";
        break;
    case Kernel::kMarch2:
        if (pl.wide) jacobi_march2_kernel<4, true><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl, rg);
        else         jacobi_march2_kernel<4, false><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl, rg);
        name = "jacobi_march2_kernel";
        break;
    case Kernel::kLds2seg:
        jacobi_lds2seg_kernel<8><<<pl.grid, pl.block, 0, st>>>(in, div, out, ni, nj, nk, pl.row_blocks, pl.nblk, pl.kc, alpha, beta, sl, rg);
        name = "jacobi_lds2seg_kernel";
        break;
    case Kernel::kLds:
        if (mask && mask->walls) {
            if (rt().slab_on)
                jacobi_lds_kernel<8, 1, 3, true, true, true><<<pl.grid, pl.block, 0, st>>>(in, div, out, ni, nj, nk, pl.row_blocks, pl.nblk, pl.kc, alpha, beta, sl, rg, *mask);
            else
                jacobi_lds_kernel<8, 1, 3, true, true><<<pl.grid, pl.block, 0, st>>>(in, div, out, ni, nj, nk, pl.row_blocks, pl.nblk, pl.kc, alpha, beta, sl, rg, SweepMaskWalls(*mask));
            name = "jacobi_lds3_walls_kernel"; what = "jacobi_lds_kernel<walls>";
            break;
        }
        if (mask) {
            jacobi_lds_kernel<8, 1, 3, true><<<pl.grid, pl.block, 0, st>>>(in, div, out, ni, nj, nk, pl.row_blocks, pl.nblk, pl.kc, alpha, beta, sl, rg, SweepMask(*mask));
            name = "jacobi_lds3_masked_kernel"; what = "jacobi_lds_kernel<masked>";
            break;
        }
#define BQ_LDS(WV, RV, SV) jacobi_lds_kernel<WV, RV, SV><<<pl.grid, pl.block, 0, st>>>(in, div, out, ni, nj, nk, pl.row_blocks, pl.nblk, pl.kc, alpha, beta, sl, rg, SweepMask{})
        if (pl.S == 4) {
            if (pl.R == 2) BQ_LDS(4, 2, 4); else BQ_LDS(6, 1, 4);
        } else if (pl.R == 2) {
            if (pl.W == 4) BQ_LDS(4, 2, 3); else if (pl.W == 5) BQ_LDS(5, 2, 3); else BQ_LDS(6, 2, 3);
        } else {
            if (pl.W == 12) BQ_LDS(12, 1, 3); else BQ_LDS(8, 1, 3);
        }
#undef BQ_LDS
        name = pl.S == 4 ? "jacobi_lds_kernel<4 sweeps>" : "jacobi_lds3_kernel"; what = "jacobi_lds_kernel";
        break;
    case Kernel::kLean3r:
        if (pl.pf == 2) jacobi_lean3r_kernel<2><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl);
        else            jacobi_lean3r_kernel<1><<<pl.grid, 256, 0, st>>>(in, div, out, ni, nj, nk, pl.cw, pl.row_blocks, pl.kc, alpha, beta, sl);
        name = "jacobi_lean3r_kernel";
        break;
    default: return false;                          // (a one-sweep plan: jacobi_sweep's)
    }
    BQ_LAUNCH_CHECK(what ? what : name);
    ps().last_pair_kernel = name;
    return true;
}

static inline geom::PlaneRanges whole_array(int nk) { return geom::PlaneRanges(0, 1 << 30, 0, 0, nk); }

// Two, three (LDS kernels, else the lean triple) or four sweeps in one launch on the whole array; false = not applicable
static bool jacobi_sweep_pair(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha, float beta)
{
    const geom::PlaneRanges pr = whole_array(nk);
    return launch_fused(plan::plan_pair(ni, nj, nk, aligned16(in, div, out), pr, tun, rt().num_cus), in, div, out, ni, nj, nk, alpha, beta, pr);
}
static bool jacobi_sweep_triple(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha, float beta)
{
    return launch_fused(plan::plan_triple(ni, nj, nk, aligned16(in, div, out), tun, rt().num_cus), in, div, out, ni, nj, nk, alpha, beta, whole_array(nk));
}
static bool jacobi_sweep_quad(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha, float beta)
{
    return launch_fused(plan::plan_quad(ni, nj, nk, aligned16(in, div, out), tun, rt().num_cus, rt().slab_on), in, div, out, ni, nj, nk, alpha, beta,
                        whole_array(nk));
}

// The mask argument of the masked LDS kernel.  The z term of the positional state: a swept plane lies in [1, nk - 1), so a plane
// of another rank's array (an index <= 0 or >= nk - 1 here) never matches, like -8.  One domain: planes 1 and nk - 2.
static SweepMaskWallsZ make_sweep_mask(const unsigned char *solid, const unsigned char *rows, const float betas[7], int walls, int nk)
{
    const Slab sl = slab_of(nk);
    SweepMaskWallsZ mk;
    mk.solid = solid; mk.rows = rows; mk.walls = walls;
    mk.wzl = (walls & BQ_WALL_ZLO) ? 1 - sl.koff : -8;
    mk.wzh = (walls & BQ_WALL_ZHI) ? sl.nkg - 2 - sl.koff : -8;
    mk.b0 = betas[0]; mk.b1 = betas[1]; mk.b2 = betas[2]; mk.b3 = betas[3]; mk.b4 = betas[4]; mk.b5 = betas[5]; mk.b6 = betas[6];
    return mk;
}

// What the masked LDS kernel asks of its arrays: float4 columns of in, div and out, and the four flag bytes of a column as one
// word (fword) -- a flag array off a 4-byte boundary takes the one-sweep masked kernels, which read bytes.  `rows` is read bytewise.
static inline bool masked_vectors_ok(const float *in, const float *div, const float *out, const unsigned char *solid)
{
    return aligned16(in, div, out) && ((uintptr_t)solid & 3u) == 0;
}

// Three MASKED sweeps in one launch (bq_obstacle.hip: gpu_jacobi_sweeps_masked; walls != 0: gpu_jacobi_sweeps_masked_walls, solid then
// being solid + walls); false = not applicable, nothing launched
bool jacobi_sweep_triple_masked(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                                const unsigned char *solid, const unsigned char *rows, const float betas[7], int walls)
{
    const SweepMaskWallsZ mk = make_sweep_mask(solid, rows, betas, walls, nk);
    return launch_fused(plan::plan_triple_masked(ni, nj, nk, masked_vectors_ok(in, div, out, solid), tun, rt().num_cus, rt().slab_on, walls != 0), in, div, out, ni, nj, nk,
                        alpha, betas[0], whole_array(nk), &mk);
}
// The walled triple on the output planes `pr` (gpu_jacobi_sweep_masked_walls_triple_ranges), z-slab ranks included: the kernel takes
// its z term from the global plane.  walls != 0.
bool jacobi_sweep_triple_masked_ranges(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                                       const unsigned char *solid, const unsigned char *rows, const float betas[7], int walls,
                                       const geom::PlaneRanges &pr)
{
    const SweepMaskWallsZ mk = make_sweep_mask(solid, rows, betas, walls, nk);
    return launch_fused(plan::plan_triple_masked_ranges(ni, nj, nk, masked_vectors_ok(in, div, out, solid), pr, tun, rt().num_cus), in, div, out, ni, nj, nk,
                        alpha, betas[0], pr, &mk);
}

static const int kResidualBlocks = 1024;

static void residual_norms_async(const float *div, const float *p, int ni, int nj, int nk,
                                 double *d_sum, float *d_max, float *dbg_sum, float *dbg_max)
{
    char *ws = (char *)scratch(kResidualBlocks * (sizeof(double) + sizeof(float)) + 64);
    if (!ws) return;
    double *ps = (double *)ws;
    float *pm = (float *)(ws + kResidualBlocks * sizeof(double));
    hipStream_t st = rt().compute;
    {
        const Runtime &r = rt();
        const int own0 = r.slab_on ? r.slab_own0 : 0, own1 = r.slab_on ? r.slab_own1 : nk;
        residual_partial_kernel<<<kResidualBlocks, 256, 0, st>>>(div, p, ni, nj, nk, ps, pm, slab_of(nk), own0, own1);
    }
    BQ_LAUNCH_CHECK("residual_partial_kernel");
    residual_final_kernel<<<1, 256, 0, st>>>(ps, pm, kResidualBlocks, d_sum, d_max, dbg_sum, dbg_max);
    BQ_LAUNCH_CHECK("residual_final_kernel");
    if (comm_ranks() > 1) {                     // owned-plane partials -> global norms
        if (d_sum) comm_allreduce(d_sum, 1, true, false, st);
        if (d_max) comm_allreduce(d_max, 1, false, true, st);
        if (dbg_sum) comm_allreduce(dbg_sum, 1, false, false, st);
        if (dbg_max) comm_allreduce(dbg_max, 1, false, true, st);
    }
}

// hipEvent pairs around the sweep loops of gpu_projection_jacobi (FL_OPT_PROFILE_JACOBI):
// lets bench.py price the dominant kernel inside the timed region, on the launch stream.

bool profile_begin(ProfileSpan &sp)
{
    if (!rt().opt_profile_jacobi) return false;
    if (!BQ_HIP(hipEventCreate(&sp.a)) || !BQ_HIP(hipEventCreate(&sp.b))) return false;
    return BQ_HIP(hipEventRecord(sp.a, rt().compute));
}
void profile_end(ProfileSpan &sp, long long launches, long long sweeps)
{
    if (!sp.a || !sp.b) return;
    BQ_HIP(hipEventRecord(sp.b, rt().compute));
    ps().spans.push_back(SweepSpan{sp.a, sp.b, launches, sweeps});
}

// bq_host.h.  Owns the profile span, the swaps, the launch count and fl_jacobi_kernel_name: the fused kernel this call launched most
// often (more sweeps per launch first on a tie).  launch_fused records every launch's name, so with one stage (the masked and walled
// loops) that is the name the stage recorded last, which those loops have always reported; with no fused launch the name stays.
int run_sweeps(float *p, float *p_temp, int sweeps, std::initializer_list<SweepStage> stages, const SweepLaunch &single)
{
    float *in = p, *out = p_temp;
    int s = 0;
    long long launches = 0;
    ProfileSpan span;
    const bool prof = sweeps > 0 && profile_begin(span);      // FL_OPT_PROFILE_JACOBI (the z-slab projection runs through here)
    const char *most_name = nullptr;
    long long most = 0;
    for (const SweepStage &stage : stages) {
        long long n_here = 0;
        while (stage.on && s + stage.sweeps <= sweeps && stage.launch(in, out)) {
            std::swap(in, out);                        // the newest iterate sits in the former `out`
            s += stage.sweeps; launches++;
            if (++n_here > most) { most = n_here; most_name = ps().last_pair_kernel; }
        }
    }
    if (most_name) ps().last_pair_kernel = most_name;
    for (; s < sweeps && single(in, out); s++) {
        std::swap(in, out);
        launches++;
    }
    if (prof) profile_end(span, launches, sweeps);
    return in == p ? 0 : 1;
}

} // namespace bq

using namespace bq;

#define BQ_ENTER(op, ...) BQ_ENTER_IF(dims_ok(ni, nj, nk, op), op, __VA_ARGS__)
#define BQ_ENTER_IF(dims_fit, op, ...)                                     \
    if (!ensure_ready(op)) return;                                         \
    if (!(dims_fit)) return;                                               \
    {                                                                      \
        const void *ptrs_[] = { __VA_ARGS__ };                             \
        for (const void *p_ : ptrs_)                                       \
            if (!p_) { latch(FL_ERR_BAD_ARGUMENT, op, "null device pointer"); return; } \
    }

extern "C" {

void gpu_divergence(const float *u, const float *v, const float *w, float *div, int ni, int nj, int nk, float halfrdx)
{
    BQ_ENTER("gpu_divergence", u, v, w, div)
    divergence_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(u, v, w, div, ni, nj, nk, halfrdx, slab_of(nk));
    BQ_LAUNCH_CHECK("divergence_kernel");
}

int gpu_jacobi_sweeps(float *p, const float *div, float *p_temp, int ni, int nj, int nk, int sweeps, float alpha, float beta)
{
    if (!ensure_ready("gpu_jacobi_sweeps")) return 0;
    if (!dims_ok(ni, nj, nk, "gpu_jacobi_sweeps")) return 0;
    if (!p || !div || !p_temp || p == p_temp) { latch(FL_ERR_BAD_ARGUMENT, "gpu_jacobi_sweeps", "null or aliased buffers"); return 0; }
    const plan::JacobiTuning tun = jacobi_tuning();
    // FL_OPT_JACOBI_FUSE >= 2: the caller vouches that p and p_temp carry the same boundary layer, so sweeps may share a launch:
    // four where plan_quad admits them, then three, then two (FL_OPT_JACOBI_FUSE = 4: two only), the rest one by one
    const bool all = tun.sweeps_fuse == plan::SweepsFuse::kAll;
    const auto fused = [&](auto launcher) {
        return [&, launcher](const float *in, float *out) { return launcher(tun, in, div, out, ni, nj, nk, alpha, beta); };
    };
    return run_sweeps(p, p_temp, sweeps,
                      {{4, all, fused(jacobi_sweep_quad)}, {3, all, fused(jacobi_sweep_triple)},
                       {2, tun.sweeps_fuse != plan::SweepsFuse::kNone, fused(jacobi_sweep_pair)}},
                      [&](const float *in, float *out) { jacobi_sweep(tun, in, div, out, ni, nj, nk, alpha, beta); return true; });
}

// one sweep in -> out restricted to the local planes [k_begin, k_end) (clipped to the interior)
void gpu_jacobi_sweep_range(const float *in, const float *div, float *out, int ni, int nj, int nk,
                            int k_begin, int k_end, float alpha, float beta)
{
    BQ_ENTER("gpu_jacobi_sweep_range", in, div, out)
    BQ_REQUIRE(in != out, "gpu_jacobi_sweep_range");
    if (k_begin >= k_end) return;
    jacobi_sweep(jacobi_tuning(), in, div, out, ni, nj, nk, alpha, beta, k_begin, k_end);
}

// Two sweeps in one launch, `out` written on the planes [k0a, k1a) and [k0b, k1b) only (either may be empty): the
// pieces of a chunk's first two sweeps on a z-slab rank -- planes whose two-sweep stencil stays inside the owned
// planes while the ghost planes are in flight, then the rest.  Returns 1 when the fused kernel ran, 0 when it does
// not apply to this grid (nothing launched: the caller sweeps plane ranges one sweep at a time instead).
int gpu_jacobi_sweep_pair_ranges(const float *in, const float *div, float *out, int ni, int nj, int nk,
                                 int k0a, int k1a, int k0b, int k1b, float alpha, float beta)
{
    if (!ensure_ready("gpu_jacobi_sweep_pair_ranges") || !dims_ok(ni, nj, nk, "gpu_jacobi_sweep_pair_ranges")) return 0;
    if (!in || !div || !out || in == out) { latch(FL_ERR_BAD_ARGUMENT, "gpu_jacobi_sweep_pair_ranges", "null or aliased buffers"); return 0; }
    const plan::JacobiTuning tun = jacobi_tuning();
    if (!tun.pair_ranges) return 0;
    const geom::PlaneRanges pr(k0a, k1a, k0b, k1b, nk);
    return launch_fused(plan::plan_pair(ni, nj, nk, aligned16(in, div, out), pr, tun, rt().num_cus), in, div, out, ni, nj, nk, alpha, beta, pr) ? 1 : 0;
}

// Three sweeps in -> out on the output planes [k0a, k1a) and [k0b, k1b) (either may be empty) through the LDS-exchanged
// kernels: the triple counterpart of gpu_jacobi_sweep_pair_ranges for the chunks of a z-slab rank.  The input must be
// valid three planes beyond each range.  Returns 1 when it ran, 0 when it does not apply (nothing launched).
int gpu_jacobi_sweep_triple_ranges(const float *in, const float *div, float *out, int ni, int nj, int nk,
                                   int k0a, int k1a, int k0b, int k1b, float alpha, float beta)
{
    if (!ensure_ready("gpu_jacobi_sweep_triple_ranges") || !dims_ok(ni, nj, nk, "gpu_jacobi_sweep_triple_ranges")) return 0;
    if (!in || !div || !out || in == out) { latch(FL_ERR_BAD_ARGUMENT, "gpu_jacobi_sweep_triple_ranges", "null or aliased buffers"); return 0; }
    const geom::PlaneRanges pr(k0a, k1a, k0b, k1b, nk);
    const plan::LaunchPlan pl = plan::plan_triple_ranges(ni, nj, nk, aligned16(in, div, out), pr, jacobi_tuning(), rt().num_cus);
    return launch_fused(pl, in, div, out, ni, nj, nk, alpha, beta, pr) ? 1 : 0;
}

void gpu_gradient(float *u, float *v, float *w, const float *p, int ni, int nj, int nk, float halfrdx)
{
    BQ_ENTER("gpu_gradient", u, v, w, p)
    gradient_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(u, v, w, p, ni, nj, nk, halfrdx, slab_of(nk));
    BQ_LAUNCH_CHECK("gradient_kernel");
}

void gpu_gradient_delta(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                        int ni, int nj, int nk, float halfrdx)
{
    BQ_ENTER("gpu_gradient_delta", u, v, w, p, du, dv, dw)
    gradient_delta_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, p, du, dv, dw, ni, nj, nk, halfrdx, slab_of(nk));
    BQ_LAUNCH_CHECK("gradient_delta_kernel");
}

void gpu_residual_norms(const float *div, const float *p, int ni, int nj, int nk, double *sum_sq, float *max_abs)
{
    BQ_ENTER("gpu_residual_norms", div, p)
    char *host = (char *)pinned(64);
    char *dev = (char *)scratch(kResidualBlocks * 12 + 64 + 64);
    if (!host || !dev) return;
    double *d_sum = (double *)(dev + kResidualBlocks * 12 + 64);
    float *d_max = (float *)(d_sum + 1);
    residual_norms_async(div, p, ni, nj, nk, d_sum, d_max, nullptr, nullptr);
    BQ_HIP(hipMemcpyAsync(host, d_sum, 16, hipMemcpyDeviceToHost, rt().compute));
    BQ_HIP(hipStreamSynchronize(rt().compute));
    if (sum_sq) *sum_sq = *(double *)host;
    if (max_abs) *max_abs = *(float *)(host + 8);
}

} // extern "C"

// The boundary shell (outermost cell layer) of a pressure buffer is never written by a sweep; the reference
// ping-pongs, so odd iterates carry p_temp's shell and even ones p's (GPU_kernel.cu:1819-1837: interior only).
// A fused two-sweep launch reads the intermediate iterate's shell from its INPUT buffer, which is the same thing
// only when both shells hold the same values.  One compare of the two shells, one flag.
__global__ void __launch_bounds__(256) shell_differs_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                           int ni, int nj, int nk, int *__restrict__ flag)
{
    const long n = (long)ni * nj * nk;
    bool bad = false;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < n; id += (long)gridDim.x * blockDim.x) {
        const int i = (int)(id % ni), j = (int)((id / ni) % nj), k = (int)(id / ((long)ni * nj));
        const bool shell = i == 0 || j == 0 || k == 0 || i == ni - 1 || j == nj - 1 || k == nk - 1;
        // value equality, with NaN == NaN (a NaN shell propagates identically from either buffer)
        if (shell && !(a[id] == b[id] || (a[id] != a[id] && b[id] != b[id]))) bad = true;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// true when p and p_temp carry the same boundary shell (blocking: one 4-byte read-back)
static bool shells_match(const float *p, const float *p_temp, int ni, int nj, int nk)
{
    int *dflag = (int *)scratch(64);
    int *hflag = (int *)pinned(64);
    if (!dflag || !hflag) return false;
    hipStream_t st = rt().compute;
    if (!BQ_HIP(hipMemsetAsync(dflag, 0, 4, st))) return false;
    // the shell is 6 faces of a box: walk the whole index space only when it is small, else face by face would be
    // cheaper -- but a single pass at HBM rate costs 20 us at 256^3 against a 3.5 ms projection
    const long n = (long)ni * nj * nk;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    shell_differs_kernel<<<blocks, 256, 0, st>>>(p, p_temp, ni, nj, nk, dflag);
    if (!BQ_LAUNCH_CHECK("shell_differs_kernel")) return false;
    if (!BQ_HIP(hipMemcpyAsync(hflag, dflag, 4, hipMemcpyDeviceToHost, st)) || !BQ_HIP(hipStreamSynchronize(st))) return false;
    return *hflag == 0;
}

extern "C" {

// GPU_kernel.cu:1839-1895.  iter sweeps are specified, iterate iter-1 is what the reference
// applies and leaves in p -> run iter-1 sweeps and make sure the result is in p.
// Two sweeps share a launch (FL_OPT_JACOBI_FUSE) only when that cannot change a value: with the option at 1 (default)
// after checking that p and p_temp carry the same boundary shell -- true for the reference's own caller, which clears
// both (gpuMapper::projectionJacobi, GPU_Advection.h:604-606), not guaranteed for any other caller of this symbol
// (a warm-started p, a p_temp with stale contents) --, at 2 on the caller's word, at 0 never.
void gpu_projection_jacobi(float *u, float *v, float *w, float *div, float *p, float *p_temp, float *debugParam,
                           int ni, int nj, int nk, int iter, float halfrdx, float alpha, float beta)
{
    BQ_ENTER("gpu_projection_jacobi", u, v, w, div, p, p_temp)
    BQ_REQUIRE(p != p_temp && iter >= 0, "gpu_projection_jacobi");
    hipStream_t st = rt().compute;
    divergence_kernel<<<grid_for(ni, nj, nk), kBlock, 0, st>>>(u, v, w, div, ni, nj, nk, halfrdx, slab_of(nk));
    BQ_LAUNCH_CHECK("divergence_kernel");
    const int stride = rt().opt_residual_stride;
    const bool dbg = debugParam != nullptr && stride > 0;
    float *in = p, *out = p_temp;
    ProfileSpan span;
    const bool prof = !dbg && iter > 1 && profile_begin(span);
    long long launches = 0;
    const plan::JacobiTuning tun = jacobi_tuning();
    const bool may_fuse = iter > 2 && (tun.trust == plan::Trust::kVouched ||
                                      (tun.trust == plan::Trust::kChecked && !rt().slab_on && shells_match(p, p_temp, ni, nj, nk)));
    if (iter == 0) {
        // the reference's swap loop does not run: p_out is still p_temp, which is copied over p (:1876-1879) and used
        // by the gradient (:1883-1891)
        fl_memcpy_d2d(p, p_temp, (size_t)ni * nj * nk * sizeof(float));
    }
    for (int it = 0; it + 1 < iter; ) {
        if (dbg && it % stride == 0 && it < 2000)
            residual_norms_async(div, in, ni, nj, nk, nullptr, nullptr, debugParam + it, debugParam + 2000 + it);
        // equal boundary shells (checked above): two sweeps may share a launch -- unless residual norms are wanted
        // for the iterate in between
        const bool pair_ok = may_fuse && it + 2 < iter && !(dbg && (it + 1) % stride == 0);
        const bool triple_ok = pair_ok && it + 3 < iter && !(dbg && (it + 2) % stride == 0) && tun.beyond_pairs;
        if (triple_ok && jacobi_sweep_triple(tun, in, div, out, ni, nj, nk, alpha, beta)) {
            it += 3;
        } else if (pair_ok && jacobi_sweep_pair(tun, in, div, out, ni, nj, nk, alpha, beta)) {
            it += 2;
        } else {
            jacobi_sweep(tun, in, div, out, ni, nj, nk, alpha, beta);
            it += 1;
        }
        launches++;
        float *t = in; in = out; out = t;
    }
    if (prof) profile_end(span, launches, iter - 1);
    if (dbg && iter > 0 && (iter - 1) % stride == 0 && iter - 1 < 2000)
        residual_norms_async(div, in, ni, nj, nk, nullptr, nullptr, debugParam + iter - 1, debugParam + 2000 + iter - 1);
    if (in != p) fl_memcpy_d2d(p, in, (size_t)ni * nj * nk * sizeof(float));
    gradient_kernel<<<grid_for(ni, nj, nk), kBlock, 0, st>>>(u, v, w, p, ni, nj, nk, halfrdx, slab_of(nk));
    BQ_LAUNCH_CHECK("gradient_kernel");
}

// Sum of the recorded sweep-loop spans since the last call (blocking); clears the list.
void fl_jacobi_profile(double *total_ms, long long *launches, long long *sweeps)
{
    double ms = 0.0;
    long long n = 0, sw = 0;
    std::vector<SweepSpan> &spans = ps().spans;
    for (SweepSpan &sp : spans) {
        float t = 0.f;
        if (BQ_HIP(hipEventSynchronize(sp.b)) && BQ_HIP(hipEventElapsedTime(&t, sp.a, sp.b))) { ms += t; n += sp.launches; sw += sp.sweeps; }
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    spans.clear();
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    if (sweeps) *sweeps = sw;
}

const char *fl_jacobi_kernel_name(void) { return ps().last_pair_kernel; }

// GPU_kernel.cu:855-876
void gpu_diffuse_field(float *field, float *fieldTemp0, float *filedTemp1, int ni, int nj, int nk, int iter, float coef)
{
    BQ_ENTER_IF(buffer_dims_ok(ni, nj, nk, "gpu_diffuse_field"), "gpu_diffuse_field", field, fieldTemp0, filedTemp1)
    BQ_REQUIRE(field != fieldTemp0 && field != filedTemp1 && fieldTemp0 != filedTemp1 && iter >= 0, "gpu_diffuse_field");
    const size_t bytes = (size_t)ni * nj * nk * sizeof(float);
    float *in = fieldTemp0, *out = filedTemp1;
    // nk is a BUFFER dim here (nk+1 for w); the slab context carries cell planes: keep the difference
    Slab dsl = slab_of(nk);
    if (rt().slab_on) dsl.nkg += nk - rt().slab_nkl;
    fl_memcpy_d2d(in, field, bytes);
    for (int it = 0; it < iter; it++) {
        diffuse_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(field, in, out, ni, nj, nk, coef, dsl.koff, dsl.nkg);
        BQ_LAUNCH_CHECK("diffuse_kernel");
        float *t = out; out = in; in = t;
    }
    fl_memcpy_d2d(field, out, bytes);
}

// `sweeps` sweeps of diffuse_field_kernel ping-ponging in -> out -> in ...; returns 0 when the newest iterate
// sits in `in`, 1 when it sits in `out` (the other buffer holds the iterate before it).  No copies: the pieces
// of gpu_diffuse_field a z-slab host needs to refresh ghost planes between chunks of sweeps.
int gpu_diffuse_sweeps(const float *field, float *in, float *out, int ni, int nj, int nk, int sweeps, float coef)
{
    if (!ensure_ready("gpu_diffuse_sweeps") || !buffer_dims_ok(ni, nj, nk, "gpu_diffuse_sweeps")) return 0;
    if (!field || !in || !out || in == out || field == in || field == out || sweeps < 0) {
        latch(FL_ERR_BAD_ARGUMENT, "gpu_diffuse_sweeps", "null or aliased buffers"); return 0;
    }
    Slab dsl = slab_of(nk);
    if (rt().slab_on) dsl.nkg += nk - rt().slab_nkl;        // nk is a BUFFER dim (nk+1 for w)
    float *a = in, *b = out;
    for (int it = 0; it < sweeps; it++) {
        diffuse_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(field, a, b, ni, nj, nk, coef, dsl.koff, dsl.nkg);
        float *t = a; a = b; b = t;
    }
    BQ_LAUNCH_CHECK("diffuse_kernel");
    return a == in ? 0 : 1;
}

void gpu_conjugate_gradient(float *, float *, float *, float *, float *, float *, float *, float *, int, int, int, int, float)
{
    latch(FL_ERR_UNSUPPORTED, "gpu_conjugate_gradient", "out of scope: alternative solver compiled out in the reference");
}

// gpu_multi_grid_conjugate_gradient: bq_mgcg.hip

} // extern "C"
