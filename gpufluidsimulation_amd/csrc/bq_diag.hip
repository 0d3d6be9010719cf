// bq_diag.hip -- flow diagnostics on the device: gpu_flow_stats makes ONE pass over the velocity and
// returns kinetic energy, enstrophy, divergence norms, the density moments and the largest vorticity magnitude as
// BQ_STAT_COUNT doubles in device memory; it can also write the cell-centred vorticity magnitude.  The definitions are the
// contract of include/bimocq_gpu.h, every line one IEEE operation (-ffp-contract=off); tests/cpu_abi/flow_stats_abi.c
// restates them in plain C.
//
// Two forms of the pass:
//   flow_stats_march_kernel  blocks of 64 x 4 columns march a chunk of planes.  The centred velocity (uc, vc) of the planes
//                            k-1, k, k+1 of the thread's own column sits in a register ring, plane k's centred triples go
//                            into a 66 x 6 LDS tile (double-buffered by plane parity, one barrier per step) from which the
//                            +-1 neighbours in x and y are read, w(k+1) is carried into the next step: five loads per cell
//                            and step plus the tile's rim instead of 30.  The fp64 partial sums stay in registers across
//                            the whole march, so a block leaves ONE partial row.
//   flow_stats_cell_kernel   one thread per cell, every operand loaded where it is used (the caches serve the re-reads);
//                            one partial row per block and plane.  FL_OPT_DIAG_KCHUNK = -1; the A/B partner.
// Reduction: wave_sum / wave_max -> LDS -> one row of BQ_STAT_COUNT doubles per block in the workspace -> stats_reduce_kernel
// (fixed order; a folding launch first when there are many rows) -> d_out.  No floating-point atomics: two calls on the same
// data return the same bits.  Everything is queued on the compute stream; nothing synchronises.
#include "bq_device.hip.h"
#include "bq_host.h"
#include "bq_launch_geom.h"
#include <algorithm>

namespace bq {

// dims, slab context and the local planes [p0, p1) whose cells count (the planes this rank owns)
struct DiagGeom { int ni, nj, nk, koff, nkg, p0, p1; float h, q; };

// a thread's share of the ten results: rows of the workspace hold them in the order of BQ_STAT_*
struct DiagAcc {
    double e2 = 0.0, m2 = 0.0, d2 = 0.0, rho = 0.0, rx = 0.0, ry = 0.0, rz = 0.0, T = 0.0;
    float dmax = 0.f, mmax = 0.f;
};

__device__ __forceinline__ size_t diag_iu(const DiagGeom &g, int i, int j, int k) { return (size_t)i + (size_t)(g.ni + 1) * ((size_t)j + (size_t)g.nj * k); }
__device__ __forceinline__ size_t diag_iv(const DiagGeom &g, int i, int j, int k) { return (size_t)i + (size_t)g.ni * ((size_t)j + (size_t)(g.nj + 1) * k); }
__device__ __forceinline__ size_t diag_ic(const DiagGeom &g, int i, int j, int k) { return (size_t)i + (size_t)g.ni * ((size_t)j + (size_t)g.nj * k); }

// cell (i, j, k) with centred velocity (uc, vc, wc), divergence d and vorticity (wx, wy, wz): what it adds to the sums
// (counted cells only) and its vorticity magnitude
template <bool SCAL>
__device__ __forceinline__ float diag_cell(DiagAcc &a, bool counted, float uc, float vc, float wc, float d, float wx, float wy, float wz,
                                           const float *__restrict__ rho, const float *__restrict__ T, size_t ic, int i, int j, int kg)
{
    const double m2 = (double)wx * (double)wx + (double)wy * (double)wy + (double)wz * (double)wz;
    const float mag = (float)sqrt(m2);
    if (counted) {
        a.e2 += (double)uc * (double)uc + (double)vc * (double)vc + (double)wc * (double)wc;
        a.m2 += m2;
        a.d2 += (double)d * (double)d;
        a.dmax = fmaxf(a.dmax, fabsf(d));
        a.mmax = fmaxf(a.mmax, mag);
        if (SCAL) {
            if (rho) {
                const double r = (double)rho[ic];
                a.rho += r; a.rx += r * (double)i; a.ry += r * (double)j; a.rz += r * (double)kg;
            }
            if (T) a.T += (double)T[ic];
        }
    }
    return mag;
}

// every thread of a 256-thread block brings its share; thread 0 leaves the block's row.  Fixed order throughout.
__device__ __forceinline__ void diag_block_row(const DiagAcc &a, double *__restrict__ row)
{
    __shared__ double ssum[4][8];
    __shared__ float smax[4][2];
    const int tid = threadIdx.x + blockDim.x * threadIdx.y, wave = tid >> 6;
    const double s0 = wave_sum(a.e2), s1 = wave_sum(a.m2), s2 = wave_sum(a.d2), s3 = wave_sum(a.rho);
    const double s4 = wave_sum(a.rx), s5 = wave_sum(a.ry), s6 = wave_sum(a.rz), s7 = wave_sum(a.T);
    const float m0 = wave_max(a.dmax), m1 = wave_max(a.mmax);
    if ((tid & 63) == 0) {
        ssum[wave][0] = s0; ssum[wave][1] = s1; ssum[wave][2] = s2; ssum[wave][3] = s3;
        ssum[wave][4] = s4; ssum[wave][5] = s5; ssum[wave][6] = s6; ssum[wave][7] = s7;
        smax[wave][0] = m0; smax[wave][1] = m1;
    }
    __syncthreads();
    if (tid == 0) {
        double t[8];
        for (int c = 0; c < 8; c++) t[c] = ((ssum[0][c] + ssum[1][c]) + ssum[2][c]) + ssum[3][c];
        row[0] = t[0]; row[1] = t[1]; row[2] = t[2];
        row[3] = (double)fmaxf(fmaxf(smax[0][0], smax[1][0]), fmaxf(smax[2][0], smax[3][0]));
        row[4] = t[3]; row[5] = t[4]; row[6] = t[5]; row[7] = t[6]; row[8] = t[7];
        row[9] = (double)fmaxf(fmaxf(smax[0][1], smax[1][1]), fmaxf(smax[2][1], smax[3][1]));
    }
}

// ---- one thread per cell ----------------------------------------------------------------------------------------------
template <bool VORT, bool SCAL>
__global__ __launch_bounds__(256) void flow_stats_cell_kernel(const float *__restrict__ u, const float *__restrict__ v, const float *__restrict__ w,
                                                              const float *__restrict__ rho, const float *__restrict__ T,
                                                              float *__restrict__ vort, DiagGeom g, int ka, double *__restrict__ part)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z + ka, kg = k + g.koff;
    DiagAcc a;
    if (i < g.ni && j < g.nj) {
        const size_t ic = diag_ic(g, i, j, k);
        float mag = 0.f;
        if (kg >= 0 && kg < g.nkg) {
            auto ucf = [&](int ii, int jj, int kk) { return 0.5f * (u[diag_iu(g, ii, jj, kk)] + u[diag_iu(g, ii + 1, jj, kk)]); };
            auto vcf = [&](int ii, int jj, int kk) { return 0.5f * (v[diag_iv(g, ii, jj, kk)] + v[diag_iv(g, ii, jj + 1, kk)]); };
            auto wcf = [&](int ii, int jj, int kk) { return 0.5f * (w[diag_ic(g, ii, jj, kk)] + w[diag_ic(g, ii, jj, kk + 1)]); };
            const float ul = u[diag_iu(g, i, j, k)], ur = u[diag_iu(g, i + 1, j, k)];
            const float vf = v[diag_iv(g, i, j, k)], vb = v[diag_iv(g, i, j + 1, k)];
            const float wd = w[ic], wu = w[diag_ic(g, i, j, k + 1)];
            const float uc = 0.5f * (ul + ur), vc = 0.5f * (vf + vb), wc = 0.5f * (wd + wu);
            const float d = ((ur - ul) + (vb - vf) + (wu - wd)) / g.h;
            float wx = 0.f, wy = 0.f, wz = 0.f;
            // an owned plane always has stored neighbours; a stored plane without one counts as border
            if (i >= 1 && i <= g.ni - 2 && j >= 1 && j <= g.nj - 2 && kg >= 1 && kg <= g.nkg - 2 && k >= 1 && k <= g.nk - 2) {
                wx = ((wcf(i, j + 1, k) - wcf(i, j - 1, k)) - (vcf(i, j, k + 1) - vcf(i, j, k - 1))) / g.q;
                wy = ((ucf(i, j, k + 1) - ucf(i, j, k - 1)) - (wcf(i + 1, j, k) - wcf(i - 1, j, k))) / g.q;
                wz = ((vcf(i + 1, j, k) - vcf(i - 1, j, k)) - (ucf(i, j + 1, k) - ucf(i, j - 1, k))) / g.q;
            }
            mag = diag_cell<SCAL>(a, k >= g.p0 && k < g.p1, uc, vc, wc, d, wx, wy, wz, rho, T, ic, i, j, kg);
        }
        if (VORT) vort[ic] = mag;
    }
    diag_block_row(a, part + (size_t)BQ_STAT_COUNT * (blockIdx.x + gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z)));
}

// ---- marching form ----------------------------------------------------------------------------------------------------
// Chunk blockIdx.z marches the local planes [ka + bz kc, min(ka + (bz + 1) kc, kb)).  Every thread of the block takes every
// barrier: a thread whose column lies outside the grid only skips its loads and stores.
template <bool VORT, bool SCAL>
__global__ __launch_bounds__(256) void flow_stats_march_kernel(const float *__restrict__ u, const float *__restrict__ v, const float *__restrict__ w,
                                                               const float *__restrict__ rho, const float *__restrict__ T,
                                                               float *__restrict__ vort, DiagGeom g, int ka, int kb, int kc,
                                                               double *__restrict__ part)
{
    __shared__ float tu[2][6][66], tv[2][6][66], tw[2][6][66];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.x * 64, j0 = blockIdx.y * 4, i = i0 + tx, j = j0 + ty;
    const int k0 = ka + blockIdx.z * kc, k1 = min(k0 + kc, kb);
    const bool col = i < g.ni && j < g.nj;
    // the tile's rim: rows j0 - 1 and j0 + 4 (uc and wc are read there) by the first and the last wave, columns i0 - 1 and
    // i0 + 64 (vc and wc) by four lanes each of the two others; the corners are never read
    const bool rim_y = ty == 0 || ty == 3;
    int ri, rj, rr, rc;
    if (rim_y) { ri = i; rj = ty == 0 ? j0 - 1 : j0 + 4; rr = ty == 0 ? 0 : 5; rc = tx + 1; }
    else       { ri = ty == 1 ? i0 - 1 : i0 + 64; rj = j0 + tx; rr = tx + 1; rc = ty == 1 ? 0 : 65; }
    const bool rim = (rim_y || tx < 4) && ri >= 0 && ri < g.ni && rj >= 0 && rj < g.nj;

    // centred (uc, vc) and the differences (du, dv) of the own column at plane kk; zeros where the plane is not stored
    auto load_uv = [&](int kk, float &uc, float &vc, float &du, float &dv) {
        uc = vc = du = dv = 0.f;
        if (col && kk >= 0 && kk < g.nk) {
            const float ul = u[diag_iu(g, i, j, kk)], ur = u[diag_iu(g, i + 1, j, kk)];
            const float vf = v[diag_iv(g, i, j, kk)], vb = v[diag_iv(g, i, j + 1, kk)];
            uc = 0.5f * (ul + ur); vc = 0.5f * (vf + vb); du = ur - ul; dv = vb - vf;
        }
    };
    float um, vm, u0, v0, du0, dv0, up, vp, dup, dvp, unused0, unused1;
    load_uv(k0 - 1, um, vm, unused0, unused1);
    load_uv(k0, u0, v0, du0, dv0);
    float wcur = (col && k0 < k1) ? w[diag_ic(g, i, j, k0)] : 0.f;
    float rwcur = (rim && k0 < k1) ? w[diag_ic(g, ri, rj, k0)] : 0.f;
    DiagAcc a;
    for (int k = k0; k < k1; k++) {
        const int b = k & 1, kg = k + g.koff;
        load_uv(k + 1, up, vp, dup, dvp);
        const float wnext = col ? w[diag_ic(g, i, j, k + 1)] : 0.f;     // w holds nk + 1 planes
        const float wc = 0.5f * (wcur + wnext);
        if (col) { tu[b][ty + 1][tx + 1] = u0; tv[b][ty + 1][tx + 1] = v0; tw[b][ty + 1][tx + 1] = wc; }
        if (rim) {
            const float rwnext = w[diag_ic(g, ri, rj, k + 1)];
            tw[b][rr][rc] = 0.5f * (rwcur + rwnext);
            rwcur = rwnext;
            if (rim_y) tu[b][rr][rc] = 0.5f * (u[diag_iu(g, ri, rj, k)] + u[diag_iu(g, ri + 1, rj, k)]);
            else       tv[b][rr][rc] = 0.5f * (v[diag_iv(g, ri, rj, k)] + v[diag_iv(g, ri, rj + 1, k)]);
        }
        // the only barrier of the step: the next step writes the other buffer, and nobody writes this one again before
        // every thread has passed the next barrier, i.e. has finished reading it
        __syncthreads();
        if (col) {
            const size_t ic = diag_ic(g, i, j, k);
            float mag = 0.f;
            if (kg >= 0 && kg < g.nkg) {
                const float d = (du0 + dv0 + (wnext - wcur)) / g.h;
                float wx = 0.f, wy = 0.f, wz = 0.f;
                if (i >= 1 && i <= g.ni - 2 && j >= 1 && j <= g.nj - 2 && kg >= 1 && kg <= g.nkg - 2 && k >= 1 && k <= g.nk - 2) {
                    wx = ((tw[b][ty + 2][tx + 1] - tw[b][ty][tx + 1]) - (vp - vm)) / g.q;
                    wy = ((up - um) - (tw[b][ty + 1][tx + 2] - tw[b][ty + 1][tx])) / g.q;
                    wz = ((tv[b][ty + 1][tx + 2] - tv[b][ty + 1][tx]) - (tu[b][ty + 2][tx + 1] - tu[b][ty][tx + 1])) / g.q;
                }
                mag = diag_cell<SCAL>(a, k >= g.p0 && k < g.p1, u0, v0, wc, d, wx, wy, wz, rho, T, ic, i, j, kg);
            }
            if (VORT) vort[ic] = mag;
        }
        um = u0; vm = v0; u0 = up; v0 = vp; du0 = dup; dv0 = dvp; wcur = wnext;
    }
    diag_block_row(a, part + (size_t)BQ_STAT_COUNT * (blockIdx.x + gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z)));
}

// Rows [b rpb, min(nin, (b + 1) rpb)) of `in` -> row b of `out`, rpb = ceil(nin / gridDim.x): thread t adds the rows t, t + 256,
// ... of its block's range in that order, then the block reduction above.  One block: the final pass, straight into d_out.
__global__ __launch_bounds__(256) void stats_reduce_kernel(const double *__restrict__ in, int nin, double *__restrict__ out)
{
    const int rpb = (nin + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rpb, r1 = min(nin, r0 + rpb);
    DiagAcc a;
    for (int r = r0 + threadIdx.x; r < r1; r += 256) {
        const double *row = in + (size_t)BQ_STAT_COUNT * r;
        a.e2 += row[0]; a.m2 += row[1]; a.d2 += row[2]; a.dmax = fmaxf(a.dmax, (float)row[3]);
        a.rho += row[4]; a.rx += row[5]; a.ry += row[6]; a.rz += row[7]; a.T += row[8]; a.mmax = fmaxf(a.mmax, (float)row[9]);
    }
    diag_block_row(a, out + (size_t)BQ_STAT_COUNT * blockIdx.x);
}

// [a, a + na) and [b, b + nb) bytes share a byte
static bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// chunk length of the march over `planes` planes: the forced one, else whole rounds of two blocks per CU with about 16
// planes per chunk (bq_launch_geom.h), and no chunk shorter than 8 planes, whose three primed planes would outweigh it
static int diag_chunk(int row_blocks, int planes, int forced)
{
    if (forced > 0) return std::min(forced, planes);
    const int nchunks = geom::whole_round_chunks(row_blocks, planes, 16, 512);
    return std::min(planes, std::max((planes + nchunks - 1) / nchunks, 8));
}

template <bool VORT, bool SCAL>
static void launch_flow_stats(const float *u, const float *v, const float *w, const float *rho, const float *T, float *vort,
                              const DiagGeom &g, int ka, int kb, int forced, double *d_out)
{
    hipStream_t st = rt().compute;
    const int gx = (g.ni + 63) / 64, gy = (g.nj + 3) / 4, planes = kb - ka;
    const bool march = forced >= 0;
    const int kc = march ? diag_chunk(gx * gy, planes, forced) : 1;
    const int gz = (planes + kc - 1) / kc;
    const size_t rows = (size_t)gx * gy * gz;
    // up to 4096 rows go straight into the final pass; more are folded 256 to one first
    const size_t folded = rows > 4096 ? (rows + 255) / 256 : 0;
    double *part = (double *)scratch((rows + folded) * BQ_STAT_COUNT * sizeof(double));
    if (!part) return;
    if (march) {
        flow_stats_march_kernel<VORT, SCAL><<<dim3(gx, gy, gz), kBlock, 0, st>>>(u, v, w, rho, T, vort, g, ka, kb, kc, part);
        BQ_LAUNCH_CHECK("flow_stats_march_kernel");
    } else {
        flow_stats_cell_kernel<VORT, SCAL><<<dim3(gx, gy, gz), kBlock, 0, st>>>(u, v, w, rho, T, vort, g, ka, part);
        BQ_LAUNCH_CHECK("flow_stats_cell_kernel");
    }
    const double *rows_in = part;
    size_t nin = rows;
    if (folded) {
        double *fold = part + rows * BQ_STAT_COUNT;
        stats_reduce_kernel<<<(unsigned)folded, 256, 0, st>>>(part, (int)rows, fold);
        BQ_LAUNCH_CHECK("stats_reduce_kernel");
        rows_in = fold; nin = folded;
    }
    stats_reduce_kernel<<<1, 256, 0, st>>>(rows_in, (int)nin, d_out);
    BQ_LAUNCH_CHECK("stats_reduce_kernel");
    if (comm_ranks() > 1) {                     // owned-plane results -> the grid's: sums and maxima lie interleaved in d_out
        comm_allreduce(d_out + 0, 3, true, false, st);
        comm_allreduce(d_out + 3, 1, true, true, st);
        comm_allreduce(d_out + 4, 5, true, false, st);
        comm_allreduce(d_out + 9, 1, true, true, st);
    }
}

} // namespace bq

using namespace bq;

extern "C" int gpu_flow_stats(const float *u, const float *v, const float *w, const float *rho, const float *T, float *vort_mag,
                              float h, int ni, int nj, int nk, double *d_out)
{
    static const char *op = "gpu_flow_stats";
    if (!ensure_ready(op)) return fl_last_error();
    const int before = fl_last_error();
    auto refuse = [&](const char *why) { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; };
    if (!u || !v || !w || !d_out) return refuse("null velocity or d_out");
    if (ni < 3 || nj < 3 || nk < 3) return refuse("dims below 3");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("plane of 2^23 elements or more");
    if (nk + 1 > 65535) return refuse("nk too large for grid.z");
    const size_t nc = (size_t)ni * nj * nk * sizeof(float);
    if (vort_mag && (overlaps(vort_mag, nc, u, (size_t)(ni + 1) * nj * nk * sizeof(float)) ||
                     overlaps(vort_mag, nc, v, (size_t)ni * (nj + 1) * nk * sizeof(float)) ||
                     overlaps(vort_mag, nc, w, (size_t)ni * nj * (nk + 1) * sizeof(float)) ||
                     overlaps(vort_mag, nc, rho, nc) || overlaps(vort_mag, nc, T, nc) ||
                     overlaps(vort_mag, nc, d_out, BQ_STAT_COUNT * sizeof(double))))
        return refuse("vort_mag aliases an input");
    const Runtime &r = rt();
    DiagGeom g;
    g.ni = ni; g.nj = nj; g.nk = nk; g.h = h; g.q = 2.0f * h;
    slab_ctx(nk, g.koff, g.nkg);
    g.p0 = r.slab_on ? std::max(0, r.slab_own0 - r.slab_koff) : 0;
    g.p1 = r.slab_on ? std::min(nk, r.slab_own1 - r.slab_koff) : nk;
    if (g.p1 < g.p0) g.p1 = g.p0;
    // with vort_mag every stored plane is visited (every cell of the buffer is written); without it only the counted ones
    int ka = vort_mag ? 0 : g.p0, kb = vort_mag ? nk : g.p1;
    if (kb <= ka) { ka = 0; kb = 1; }           // nothing owned: one plane, none of it counted, leaves the zeros
    const int forced = r.opt_diag_kchunk;
    const bool scal = rho || T;
    if (vort_mag) { if (scal) launch_flow_stats<true, true>(u, v, w, rho, T, vort_mag, g, ka, kb, forced, d_out);
                    else      launch_flow_stats<true, false>(u, v, w, rho, T, vort_mag, g, ka, kb, forced, d_out); }
    else          { if (scal) launch_flow_stats<false, true>(u, v, w, rho, T, vort_mag, g, ka, kb, forced, d_out);
                    else      launch_flow_stats<false, false>(u, v, w, rho, T, vort_mag, g, ka, kb, forced, d_out); }
    return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
}
