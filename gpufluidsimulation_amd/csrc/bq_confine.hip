// bq_confine.hip -- vorticity confinement as one fused force: gpu_vorticity_confinement reads the MAC
// velocity and writes u + dt f, f = eps h (N x omega), N the normalised gradient of |omega|, omega and |omega| exactly those of
// gpu_flow_stats (section 20).  The definitions are the contract of include/bimocq_gpu.h, every line one IEEE operation
// (-ffp-contract=off); tests/cpu_abi/confinement_abi.c restates them in plain C.
//
// Two forms:
//   confine_march_kernel  blocks of 32 x 16 threads march a chunk of planes, one thread per cell column of an OVERLAPPED
//                         tile: the block's columns include the stencil's halo (3 cells on the low side, 2 on the high
//                         side), every thread carries its own column through every stage, and the 27 x 11 columns in the
//                         middle store.  Per step one plane of faces is loaded, and four stages advance, each one plane
//                         behind the one before:  centred velocity of plane q -> LDS | barrier | omega, m of plane q (own
//                         column's uc, vc of q-1 and q+1 from a register ring) -> LDS;  f of plane q-1 (m of q-1 of the
//                         neighbours from the tile the PREVIOUS step left, m of q and q-2 from the ring) -> LDS;  wo of plane
//                         q-1 (fz of q-2 and q-1 from the ring), uo and vo of plane q-2 (f of the left / front neighbour from
//                         the previous step's tile).  All tiles are double-buffered by plane parity, so ONE barrier per step
//                         orders everything.  The faces themselves ride a register ring from their load to their store:
//                         every face is loaded once per block that covers it and nothing is read twice along the march.
//   confine_node_kernel   one thread per output node, everything recomputed from global memory, no scratch fields.
//                         FL_OPT_CONFINE_KCHUNK = -1; the A/B partner.
// Every value is computed by the same expression in both forms and for every chunk length: same bits.  No atomics.
#include "bq_host.h"
#include "bq_launch_geom.h"
#include <algorithm>

namespace bq {

struct ConfGeom { int ni, nj, nk; float h, q, eh, dt; };        // q = 2.0f * h, eh = eps * h

__device__ __forceinline__ size_t cf_iu(const ConfGeom &g, int i, int j, int k) { return (size_t)i + (size_t)(g.ni + 1) * ((size_t)j + (size_t)g.nj * k); }
__device__ __forceinline__ size_t cf_iv(const ConfGeom &g, int i, int j, int k) { return (size_t)i + (size_t)g.ni * ((size_t)j + (size_t)(g.nj + 1) * k); }
__device__ __forceinline__ size_t cf_ic(const ConfGeom &g, int i, int j, int k) { return (size_t)i + (size_t)g.ni * ((size_t)j + (size_t)g.nj * k); }

__device__ __forceinline__ float cf_mag(float wx, float wy, float wz)
{
    const double m2 = (double)wx * (double)wx + (double)wy * (double)wy + (double)wz * (double)wz;
    return (float)sqrt(m2);
}

// the force of a confined cell from m at its six neighbours and its own vorticity
__device__ __forceinline__ void cf_force(const ConfGeom &g, float mxp, float mxm, float myp, float mym, float mzp, float mzm,
                                         float wx, float wy, float wz, float &fx, float &fy, float &fz)
{
    const float gx = (mxp - mxm) / g.q, gy = (myp - mym) / g.q, gz = (mzp - mzm) / g.q;
    const double g2 = (double)gx * (double)gx + (double)gy * (double)gy + (double)gz * (double)gz;
    const float len = (float)sqrt(g2);
    fx = fy = fz = 0.f;
    if (!(len > 0.f)) return;
    const float nx = gx / len, ny = gy / len, nz = gz / len;
    fx = g.eh * (ny * wz - nz * wy);
    fy = g.eh * (nz * wx - nx * wz);
    fz = g.eh * (nx * wy - ny * wx);
}

// a face between two cells: its value plus dt times the mean of their forces
__device__ __forceinline__ float cf_face(const ConfGeom &g, float val, float fm, float f0) { return val + g.dt * (0.5f * (fm + f0)); }

// ---- one thread per output node ---------------------------------------------------------------------------------------
// section 20's vorticity of cell (i, j, k), zeros on border cells and outside the grid
__device__ __forceinline__ void cf_omega(const ConfGeom &g, const float *__restrict__ u, const float *__restrict__ v,
                                         const float *__restrict__ w, int i, int j, int k, float &wx, float &wy, float &wz)
{
    wx = wy = wz = 0.f;
    if (i < 1 || i > g.ni - 2 || j < 1 || j > g.nj - 2 || k < 1 || k > g.nk - 2) return;
    auto ucf = [&](int ii, int jj, int kk) { return 0.5f * (u[cf_iu(g, ii, jj, kk)] + u[cf_iu(g, ii + 1, jj, kk)]); };
    auto vcf = [&](int ii, int jj, int kk) { return 0.5f * (v[cf_iv(g, ii, jj, kk)] + v[cf_iv(g, ii, jj + 1, kk)]); };
    auto wcf = [&](int ii, int jj, int kk) { return 0.5f * (w[cf_ic(g, ii, jj, kk)] + w[cf_ic(g, ii, jj, kk + 1)]); };
    wx = ((wcf(i, j + 1, k) - wcf(i, j - 1, k)) - (vcf(i, j, k + 1) - vcf(i, j, k - 1))) / g.q;
    wy = ((ucf(i, j, k + 1) - ucf(i, j, k - 1)) - (wcf(i + 1, j, k) - wcf(i - 1, j, k))) / g.q;
    wz = ((vcf(i + 1, j, k) - vcf(i - 1, j, k)) - (ucf(i, j + 1, k) - ucf(i, j - 1, k))) / g.q;
}

__device__ __forceinline__ float cf_m(const ConfGeom &g, const float *__restrict__ u, const float *__restrict__ v,
                                      const float *__restrict__ w, int i, int j, int k)
{
    float wx, wy, wz;
    cf_omega(g, u, v, w, i, j, k, wx, wy, wz);
    return cf_mag(wx, wy, wz);
}

// the force of cell (i, j, k): zeros unless the cell is confined
__device__ __forceinline__ void cf_cell_force(const ConfGeom &g, const float *__restrict__ u, const float *__restrict__ v,
                                              const float *__restrict__ w, int i, int j, int k, float &fx, float &fy, float &fz)
{
    fx = fy = fz = 0.f;
    if (i < 2 || i > g.ni - 3 || j < 2 || j > g.nj - 3 || k < 2 || k > g.nk - 3) return;
    float wx, wy, wz;
    cf_omega(g, u, v, w, i, j, k, wx, wy, wz);
    cf_force(g, cf_m(g, u, v, w, i + 1, j, k), cf_m(g, u, v, w, i - 1, j, k), cf_m(g, u, v, w, i, j + 1, k), cf_m(g, u, v, w, i, j - 1, k),
             cf_m(g, u, v, w, i, j, k + 1), cf_m(g, u, v, w, i, j, k - 1), wx, wy, wz, fx, fy, fz);
}

// node (i, j, k) of the (ni + 1) x (nj + 1) x (nk + 1) node box: the u, v and w face with these indices, where they exist
__global__ __launch_bounds__(256) void confine_node_kernel(float *__restrict__ uo, float *__restrict__ vo, float *__restrict__ wo,
                                                           const float *__restrict__ u, const float *__restrict__ v,
                                                           const float *__restrict__ w, ConfGeom g)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > g.ni || j > g.nj) return;
    float fx, fy, fz, ax, ay, az;
    cf_cell_force(g, u, v, w, i, j, k, fx, fy, fz);
    if (j < g.nj && k < g.nk) {
        const size_t a = cf_iu(g, i, j, k);
        float val = u[a];
        if (i >= 1 && i <= g.ni - 1) { cf_cell_force(g, u, v, w, i - 1, j, k, ax, ay, az); val = cf_face(g, val, ax, fx); }
        uo[a] = val;
    }
    if (i < g.ni && k < g.nk) {
        const size_t a = cf_iv(g, i, j, k);
        float val = v[a];
        if (j >= 1 && j <= g.nj - 1) { cf_cell_force(g, u, v, w, i, j - 1, k, ax, ay, az); val = cf_face(g, val, ay, fy); }
        vo[a] = val;
    }
    if (i < g.ni && j < g.nj) {
        const size_t a = cf_ic(g, i, j, k);
        float val = w[a];
        if (k >= 1 && k <= g.nk - 1) { cf_cell_force(g, u, v, w, i, j, k - 1, ax, ay, az); val = cf_face(g, val, az, fz); }
        wo[a] = val;
    }
}

// ---- marching form ----------------------------------------------------------------------------------------------------
// The tile: CF_TX x CF_TY columns per block, of which the CF_SX x CF_SY from (3, 3) on store.  What a column's stages can
// trust shrinks by one column per LDS hand-over: centred velocity everywhere, omega and m inside 1 column of the tile's
// edge, f inside 2, a face (which reads f of its LOW neighbour only) from 3 on the low side and 2 on the high side.
constexpr int CF_TX = 32, CF_TY = 16, CF_SX = CF_TX - 5, CF_SY = CF_TY - 5;
constexpr int CF_WARM = 4;              // steps a chunk marches before its first complete store

// Chunk blockIdx.z stores the planes [k0, k1) of uo and vo and the planes [k0, k1) of wo (the last chunk also plane nk).  Step q
// loads the faces of plane q + 2.  Every thread of the block takes every barrier: a thread whose column lies outside the
// grid carries zeros and skips its loads and stores.
__global__ __launch_bounds__(CF_TX * CF_TY) __attribute__((amdgpu_waves_per_eu(6, 6))) void confine_march_kernel(float *__restrict__ uo, float *__restrict__ vo, float *__restrict__ wo,
                                                                      const float *__restrict__ u, const float *__restrict__ v,
                                                                      const float *__restrict__ w, ConfGeom g, int kc)
{
    __shared__ float tu[2][CF_TY][CF_TX], tv[2][CF_TY][CF_TX], tw[2][CF_TY][CF_TX];
    __shared__ float tm[2][CF_TY][CF_TX], tfx[2][CF_TY][CF_TX], tfy[2][CF_TY][CF_TX];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i = (int)blockIdx.x * CF_SX - 3 + tx, j = (int)blockIdx.y * CF_SY - 3 + ty;
    const int k0 = (int)blockIdx.z * kc, k1 = min(k0 + kc, g.nk);
    const bool col = i >= 0 && i < g.ni && j >= 0 && j < g.nj;
    const bool own = col && tx >= 3 && tx < CF_TX - 2 && ty >= 3 && ty < CF_TY - 2;
    // neighbours inside the tile; a column on the tile's edge reads itself and computes values nobody trusts
    const int txm = max(tx - 1, 0), txp = min(tx + 1, CF_TX - 1), tym = max(ty - 1, 0), typ = min(ty + 1, CF_TY - 1);
    const bool vort_ij = i >= 1 && i <= g.ni - 2 && j >= 1 && j <= g.nj - 2;
    // (f of the two outermost columns of the tile is never read: the first and the last wave of the block skip it whole)
    const bool conf_ij = i >= 2 && i <= g.ni - 3 && j >= 2 && j <= g.nj - 3 && tx >= 2 && tx < CF_TX - 2 && ty >= 2 && ty < CF_TY - 2;

    // the own column's faces u(i), v(j) and centred (uc, vc) at plane kk; zeros where nothing is stored
    auto load_uv = [&](int kk, float &fu, float &fv, float &uc, float &vc) {
        fu = fv = uc = vc = 0.f;
        if (col && kk >= 0 && kk < g.nk) {
            fu = u[cf_iu(g, i, j, kk)];
            fv = v[cf_iv(g, i, j, kk)];
            uc = 0.5f * (fu + u[cf_iu(g, i + 1, j, kk)]);
            vc = 0.5f * (fv + v[cf_iv(g, i, j + 1, kk)]);
        }
    };
    auto load_w = [&](int kk) { return (col && kk >= 0 && kk <= g.nk) ? w[cf_ic(g, i, j, kk)] : 0.f; };

    // rings, named by their plane relative to the step's q:  faces u, v at q+2 .. q-2, w at q+2 .. q-1;  centred (uc, vc) at
    // q+2 .. q-1;  omega at q-1;  m at q-1, q-2;  f at q-2.  Plane q+2 is only in flight: a step issues its loads first and
    // nothing reads them before the next step, so their latency hides behind the step's arithmetic.
    float fu2, fv2, uc2, vc2, fu1, fv1, ucp, vcp, fu0, fv0, uc0, vc0, fum1, fvm1, ucm, vcm, fum2 = 0.f, fvm2 = 0.f;
    load_uv(k0 - 3, fum1, fvm1, ucm, vcm);
    load_uv(k0 - 2, fu0, fv0, uc0, vc0);
    load_uv(k0 - 1, fu1, fv1, ucp, vcp);
    float fw2, fw1 = load_w(k0 - 1), fw0 = load_w(k0 - 2), fwm1 = 0.f;
    float wxm = 0.f, wym = 0.f, wzm = 0.f, mm1 = 0.f, mm2 = 0.f, fxm = 0.f, fym = 0.f, fzm = 0.f;
    for (int q = k0 - 2; q <= k1 + 1; q++) {
        const int b = q & 1, r = q - 1, p = q - 2;
        load_uv(q + 2, fu2, fv2, uc2, vc2);
        fw2 = load_w(q + 2);
        tu[b][ty][tx] = uc0; tv[b][ty][tx] = vc0; tw[b][ty][tx] = 0.5f * (fw0 + fw1);
        // the only barrier of the step.  It publishes this step's centred velocity AND what the previous step wrote after
        // its barrier (m and f into the other buffers); a buffer is rewritten two barriers after it was filled.
        __syncthreads();
        float wx = 0.f, wy = 0.f, wz = 0.f;
        if (vort_ij && q >= 1 && q <= g.nk - 2) {
            wx = ((tw[b][typ][tx] - tw[b][tym][tx]) - (vcp - vcm)) / g.q;
            wy = ((ucp - ucm) - (tw[b][ty][txp] - tw[b][ty][txm])) / g.q;
            wz = ((tv[b][ty][txp] - tv[b][ty][txm]) - (tu[b][typ][tx] - tu[b][tym][tx])) / g.q;
        }
        const float m0 = cf_mag(wx, wy, wz);
        tm[b][ty][tx] = m0;
        // f of plane r: the first plane this chunk needs is k0 - 1 (for wo of plane k0); before that the other buffers hold nothing
        float fx = 0.f, fy = 0.f, fz = 0.f;
        if (conf_ij && r >= 2 && r <= g.nk - 3 && r >= k0 - 1)
            cf_force(g, tm[b ^ 1][ty][txp], tm[b ^ 1][ty][txm], tm[b ^ 1][typ][tx], tm[b ^ 1][tym][tx], m0, mm2, wxm, wym, wzm, fx, fy, fz);
        if (own) {
            if (r >= k0 && (r < k1 || (r == g.nk && k1 == g.nk)))
                wo[cf_ic(g, i, j, r)] = (r >= 1 && r <= g.nk - 1) ? cf_face(g, fwm1, fzm, fz) : fwm1;
            if (p >= k0 && p < k1) {
                uo[cf_iu(g, i, j, p)] = i >= 1 ? cf_face(g, fum2, tfx[b ^ 1][ty][tx - 1], fxm) : fum2;
                vo[cf_iv(g, i, j, p)] = j >= 1 ? cf_face(g, fvm2, tfy[b ^ 1][ty - 1][tx], fym) : fvm2;
                if (i == g.ni - 1) uo[cf_iu(g, g.ni, j, p)] = u[cf_iu(g, g.ni, j, p)];       // the boundary faces are copied
                if (j == g.nj - 1) vo[cf_iv(g, i, g.nj, p)] = v[cf_iv(g, i, g.nj, p)];
            }
        }
        tfx[b][ty][tx] = fx; tfy[b][ty][tx] = fy;
        ucm = uc0; vcm = vc0; uc0 = ucp; vc0 = vcp; ucp = uc2; vcp = vc2;
        fum2 = fum1; fum1 = fu0; fu0 = fu1; fu1 = fu2; fvm2 = fvm1; fvm1 = fv0; fv0 = fv1; fv1 = fv2; fwm1 = fw0; fw0 = fw1; fw1 = fw2;
        wxm = wx; wym = wy; wzm = wz; mm2 = mm1; mm1 = m0; fxm = fx; fym = fy; fzm = fz;
    }
}

// [a, a + na) and [b, b + nb) bytes share a byte
static bool cf_overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// chunk length of the march: the forced one, else the count that costs the fewest rounds x (chunk + warm-up) steps with
// three blocks per CU (76 VGPRs, 24 KB of LDS) and about 32 planes per chunk (bq_launch_geom.h: chunks_for_cus -- the tile's
// 27 x 11 stride gives row-block counts that no chunk count turns into whole rounds, 240 at 256^3)
static int confine_chunk(int row_blocks, int nk, int forced, int ncus)
{
    if (forced > 0) return std::min(forced, nk);
    const int nchunks = geom::chunks_for_cus(nk, row_blocks, 32, CF_WARM, std::max(ncus, 1), 3);
    return (nk + nchunks - 1) / nchunks;
}

} // namespace bq

using namespace bq;

extern "C" int gpu_vorticity_confinement(float *uo, float *vo, float *wo, const float *u, const float *v, const float *w,
                                         float h, int ni, int nj, int nk, float eps, float dt)
{
    static const char *op = "gpu_vorticity_confinement";
    if (!ensure_ready(op)) return fl_last_error();
    const int before = fl_last_error();
    auto refuse = [&](const char *why) { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; };
    if (!uo || !vo || !wo || !u || !v || !w) return refuse("null pointer");
    if (ni < 3 || nj < 3 || nk < 3) return refuse("dims below 3");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return refuse("eps negative or not finite");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("plane of 2^23 elements or more");
    if (nk + 1 > 65535) return refuse("nk too large for grid.z");
    if ((nj + 4) / 4 > 65535) return refuse("nj too large for grid.y");
    const size_t nb[3] = { (size_t)(ni + 1) * nj * nk * sizeof(float), (size_t)ni * (nj + 1) * nk * sizeof(float),
                           (size_t)ni * nj * (nk + 1) * sizeof(float) };
    const void *out[3] = { uo, vo, wo }, *in[3] = { u, v, w };
    for (int a = 0; a < 3; a++) {
        for (int c = 0; c < 3; c++)
            if (cf_overlaps(out[a], nb[a], in[c], nb[c])) return refuse("an output overlaps an input");
        for (int c = a + 1; c < 3; c++)
            if (cf_overlaps(out[a], nb[a], out[c], nb[c])) return refuse("two outputs overlap");
    }
    const Runtime &r = rt();
    if (r.slab_on) {
        latch(FL_ERR_UNSUPPORTED, op, "not supported under a z-slab context");
        return (int)FL_ERR_UNSUPPORTED;
    }
    ConfGeom g;
    g.ni = ni; g.nj = nj; g.nk = nk; g.h = h; g.q = 2.0f * h; g.eh = eps * h; g.dt = dt;
    const int forced = r.opt_confine_kchunk;
    if (forced < 0) {
        confine_node_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, r.compute>>>(uo, vo, wo, u, v, w, g);
        BQ_LAUNCH_CHECK("confine_node_kernel");
    } else {
        const int gx = (ni + CF_SX - 1) / CF_SX, gy = (nj + CF_SY - 1) / CF_SY;
        const int kc = confine_chunk(gx * gy, nk, forced, r.num_cus);
        confine_march_kernel<<<dim3(gx, gy, (nk + kc - 1) / kc), dim3(CF_TX, CF_TY, 1), 0, r.compute>>>(uo, vo, wo, u, v, w, g, kc);
        BQ_LAUNCH_CHECK("confine_march_kernel");
    }
    return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
}
