// bq_source.hip -- shaped, moving smoke sources (reference: Emitter and BimocqSolver::emitSmoke of
// the CPU solver, BimocqSolver.h:31-59, BimocqSolver.cpp:696-813).  A source is an obstacle shape of section 14 -- sphere,
// box or level set -- and a node belongs to it when the obstacle classification calls the node solid: the list travels as
// the obstacle kernels' ObsSet / LsSet and is tested by obs_solid (bq_obstacle.hip.h).  One launch covers the node boxes
// the entries can reach; the window and the inside tests are evaluated per node, so the boxes never change a value.
#include "bq_device.hip.h"
#include "bq_host.h"
#include "bq_obstacle.hip.h"

#include <algorithm>
#include <vector>

namespace bq {

static_assert(BQ_MAX_SOURCES == BQ_MAX_BOUNDARIES, "sources travel in the obstacle list's ObsSet / LsSet");

// what the entries write
struct SrcVal {
    float density[BQ_MAX_SOURCES], temperature[BQ_MAX_SOURCES];
    float ex[BQ_MAX_SOURCES], ey[BQ_MAX_SOURCES], ez[BQ_MAX_SOURCES];
    float ox[BQ_MAX_SOURCES], oy[BQ_MAX_SOURCES], oz[BQ_MAX_SOURCES];
    int flags[BQ_MAX_SOURCES];
};

// the launch: box b covers the super-grid nodes [x0, x0 + 64 gridDim.x) x [y0, y0 + 4 gridDim.y) x [z0, ...) (GLOBAL
// planes); its planes are the blocks zbeg[b] <= blockIdx.z < zbeg[b + 1].  x1, y1: last node of the box.
struct SrcBoxes {
    int n;
    int x0[BQ_MAX_SOURCES], x1[BQ_MAX_SOURCES], y0[BQ_MAX_SOURCES], y1[BQ_MAX_SOURCES], z0[BQ_MAX_SOURCES];
    int zbeg[BQ_MAX_SOURCES + 1];
};

// o + 1 for the last entry that contains (x, y, z) -- with `velocity`: and has BQ_SOURCE_VELOCITY --, 0 when none does
template <typename... Ls>
__device__ __forceinline__ int src_last(float x, float y, float z, bool velocity, const ObsSet &s, const SrcVal &sv, const Ls &...ls)
{
    int last = 0;
    for (int o = 0; o < s.n; o++) {
        if (velocity && !(sv.flags[o] & BQ_SOURCE_VELOCITY)) continue;
        if (obs_solid(x, y, z, o, s, ls...)) last = o + 1;
    }
    return last;
}

// one thread per node (i, j, k) of the (ni + 1, nj + 1, nkg + 1) super-grid inside a box: its cell node and its u, v, w
// face nodes, each inside the legacy emitter's window of its own buffer (1 < index < n - 2) and the stored planes
template <typename... Ls>
__global__ __launch_bounds__(256) void emit_sources_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                           float *__restrict__ rho, float *__restrict__ T,
                                                           ObsSet ob, Ls... ls, SrcVal sv, SrcBoxes bx, float h,
                                                           int ni, int nj, int nk, int koff, int nkg)
{
    int b = 0;
    while (b + 1 < bx.n && (int)blockIdx.z >= bx.zbeg[b + 1]) b++;        // uniform over the block
    const int i = bx.x0[b] + (int)(blockIdx.x * 64 + threadIdx.x), j = bx.y0[b] + (int)(blockIdx.y * 4 + threadIdx.y);
    const int k = bx.z0[b] + ((int)blockIdx.z - bx.zbeg[b]), kl = k - koff;
    if (i > bx.x1[b] || j > bx.y1[b]) return;
    // (the host clipped the boxes to these ranges; evaluated again so that no box can reach outside a buffer)
    const bool ic = i > 1 && i < ni - 2, jc = j > 1 && j < nj - 2, kc = k > 1 && k < nkg - 2 && kl >= 0 && kl < nk;
    const bool iu = i > 1 && i < ni - 1, jv = j > 1 && j < nj - 1, kw = k > 1 && k < nkg - 1 && kl >= 0 && kl <= nk;
    const float x0 = obs_pos(i, 0, h), y0 = obs_pos(j, 0, h), z0 = obs_pos(k, 0, h);
    const float x1 = obs_pos(i, 1, h), y1 = obs_pos(j, 1, h), z1 = obs_pos(k, 1, h);
    if (ic && jc && kc) {
        const int o = src_last(x0, y0, z0, false, ob, sv, ls...);
        if (o) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * kl);
            rho[id] = sv.density[o - 1];
            T[id] = sv.temperature[o - 1];
        }
    }
    if (iu && jc && kc) {
        const int o = src_last(x1, y0, z0, true, ob, sv, ls...);
        if (o) {
            const float dy = y0 - ob.cy[o - 1], dz = z0 - ob.cz[o - 1];
            u[(size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * kl)] = sv.ex[o - 1] + (sv.oy[o - 1] * dz - sv.oz[o - 1] * dy);
        }
    }
    if (ic && jv && kc) {
        const int o = src_last(x0, y1, z0, true, ob, sv, ls...);
        if (o) {
            const float dx = x0 - ob.cx[o - 1], dz = z0 - ob.cz[o - 1];
            v[(size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * kl)] = sv.ey[o - 1] + (sv.oz[o - 1] * dx - sv.ox[o - 1] * dz);
        }
    }
    if (ic && jc && kw) {
        const int o = src_last(x0, y0, z1, true, ob, sv, ls...);
        if (o) {
            const float dx = x0 - ob.cx[o - 1], dy = y0 - ob.cy[o - 1];
            w[(size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * kl)] = sv.ez[o - 1] + (sv.ox[o - 1] * dy - sv.oy[o - 1] * dx);
        }
    }
}

// the super-grid nodes [lo, hi] of one axis that positions in [a, b] (world units, double) can belong to, one node wider
// on either side, clipped to [wlo, whi]; an interval that is not finite keeps the whole range
static void node_range(double a, double b, double h, int wlo, int whi, int &lo, int &hi)
{
    const double l = std::floor(a / h) - 1.0, r = std::ceil(b / h + 0.5) + 1.0;      // faces sit at (i - 1/2) h
    lo = l > (double)wlo ? (l < (double)whi + 1.0 ? (int)l : whi + 1) : wlo;
    hi = r < (double)whi ? (r > (double)wlo - 1.0 ? (int)r : wlo - 1) : whi;
}

} // namespace bq

using namespace bq;

extern "C" void gpu_emit_sources(float *u, float *v, float *w, float *rho, float *T, const bq_source *src, const bq_levelset *ls,
                                 int n, float h, int ni, int nj, int nk)
{
    const char *op = "gpu_emit_sources";
    if (!ensure_ready(op)) return;
    if (!obstacle_dims_ok(ni, nj, nk, op)) return;
    if (n < 0 || n > BQ_MAX_SOURCES || (n > 0 && !src)) { latch(FL_ERR_BAD_ARGUMENT, op, "0 .. 16 sources"); return; }
    if (!u || !v || !w || !rho || !T || !(h > 0.f)) { latch(FL_ERR_BAD_ARGUMENT, op, "null device pointer or spacing"); return; }
    bq_boundary shapes[BQ_MAX_SOURCES];
    bool any_ls = false;
    for (int o = 0; o < n; o++) {
        shapes[o] = src[o].shape;
        const int sh = shapes[o].shape;
        if ((sh != BQ_SHAPE_SPHERE && sh != BQ_SHAPE_BOX && sh != BQ_SHAPE_LEVELSET) || (src[o].flags & ~BQ_SOURCE_VELOCITY)) {
            latch(FL_ERR_BAD_ARGUMENT, op, "unknown shape or flag");
            return;
        }
        any_ls = any_ls || sh == BQ_SHAPE_LEVELSET;
    }
    if (const char *why = ls_check(shapes, ls, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    if (n == 0) return;

    int koff, nkg;
    slab_ctx(nk, koff, nkg);
    // the union of the four node windows, and the stored planes (w has one more)
    const int wx0 = 2, wx1 = ni - 2, wy0 = 2, wy1 = nj - 2;
    const int wz0 = std::max(2, koff), wz1 = std::min(nkg - 2, koff + nk);
    SrcBoxes bx{};
    SrcVal sv{};
    int gx = 0, gy = 0, planes = 0;
    for (int o = 0; o < n; o++) {
        const bq_boundary &s = shapes[o];
        sv.density[o] = src[o].density; sv.temperature[o] = src[o].temperature;
        sv.ex[o] = src[o].ex; sv.ey[o] = src[o].ey; sv.ez[o] = src[o].ez;
        sv.ox[o] = src[o].ox; sv.oy[o] = src[o].oy; sv.oz[o] = src[o].oz;
        sv.flags[o] = src[o].flags;
        double lo[3], hi[3];
        if (s.shape == BQ_SHAPE_LEVELSET) {
            const bq_levelset &l = ls[o];
            const int i0[3] = { l.i0, l.j0, l.k0 }, nn[3] = { l.nx, l.ny, l.nz };
            const float c[3] = { s.cx, s.cy, s.cz };
            for (int d = 0; d < 3; d++) {
                lo[d] = (double)c[d] + ((double)i0[d] - 1.0) * (double)l.voxel;
                hi[d] = (double)c[d] + ((double)i0[d] + (double)nn[d]) * (double)l.voxel;
            }
        } else {
            const float c[3] = { s.cx, s.cy, s.cz }, r[3] = { s.rx, s.shape == BQ_SHAPE_SPHERE ? s.rx : s.ry, s.shape == BQ_SHAPE_SPHERE ? s.rx : s.rz };
            for (int d = 0; d < 3; d++) { lo[d] = (double)c[d] - std::fabs((double)r[d]); hi[d] = (double)c[d] + std::fabs((double)r[d]); }
        }
        int x0, x1, y0, y1, z0, z1;
        node_range(lo[0], hi[0], (double)h, wx0, wx1, x0, x1);
        node_range(lo[1], hi[1], (double)h, wy0, wy1, y0, y1);
        node_range(lo[2], hi[2], (double)h, wz0, wz1, z0, z1);
        if (x1 < x0 || y1 < y0 || z1 < z0) continue;                // nothing of this entry inside the window
        const int b = bx.n++;
        bx.x0[b] = x0; bx.x1[b] = x1; bx.y0[b] = y0; bx.y1[b] = y1; bx.z0[b] = z0;
        bx.zbeg[b] = planes;
        planes += z1 - z0 + 1;
        bx.zbeg[b + 1] = planes;
        gx = std::max(gx, (x1 - x0 + 64) / 64);
        gy = std::max(gy, (y1 - y0 + 4) / 4);
    }
    if (!bx.n) return;
    if (planes > 65535) { latch(FL_ERR_BAD_ARGUMENT, op, "source boxes hold more than 65535 planes"); return; }
    const dim3 grid(gx, gy, planes);
    if (any_ls)
        emit_sources_kernel<LsSet><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, make_obs(shapes, n, h), make_ls(shapes, ls, n), sv, bx, h, ni, nj, nk, koff, nkg);
    else
        emit_sources_kernel<><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, make_obs(shapes, n, h), sv, bx, h, ni, nj, nk, koff, nkg);
    BQ_LAUNCH_CHECK("emit_sources_kernel");
}
