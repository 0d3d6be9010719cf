// bq_obstacle.hip -- solid obstacles (reference: setBoundary / updateBoundary, blendBoundary,
// clearBoundary and the masked projection of BimocqSolver.cpp:879-1413): cell flags + tile summary, the solid face
// write, the masked Jacobi sweep, the masked gradient, and the band blend fused with the density clear.
// The band semi-Lagrangian pass lives beside semilag_kernel in bq_advect.hip.
#include "bq_device.hip.h"
#include "bq_host.h"
#include "bq_jacobi_plan.h"
#include "bq_obstacle.hip.h"

namespace bq {

// ---- flags: one thread per cell; a solid cell marks the rows summary of its own row and plane and the neighbouring ones --
template <typename... Ls>
__global__ __launch_bounds__(256) void obstacle_flags_kernel(unsigned char *__restrict__ solid, unsigned char *__restrict__ rows,
                                                             ObsSet ob, Ls... ls, float h, int ni, int nj, int nk)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i >= ni || j >= nj) return;
    const int c = obs_classify(obs_pos(i, 0, h), obs_pos(j, 0, h), obs_pos(k, 0, h), ob, ls...);
    const unsigned char f = c > 0 ? (unsigned char)c : 0;
    solid[(size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k)] = f;
    if (!f) return;
    for (int kk = max(k - 1, 0); kk <= min(k + 1, nk - 1); kk++)
        for (int jj = max(j - 1, 0); jj <= min(j + 1, nj - 1); jj++)
            rows[(size_t)jj + (size_t)nj * kk] = 1;                 // same value from every writer
}

__device__ __forceinline__ int flag_at(const unsigned char *solid, int i, int j, int k, int ni, int nj, int nk)
{
    return (i >= 0 && i < ni && j >= 0 && j < nj && k >= 0 && k < nk) ? solid[(size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k)] : 0;
}

// ---- solid faces: one thread per node of the (ni+1, nj+1, nk+1) super-grid ------------------------------------------
__global__ __launch_bounds__(256) void obstacle_faces_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                             float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                             const unsigned char *__restrict__ solid, ObsVel ov, int ni, int nj, int nk)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    if (j < nj && k < nk) {                                         // u face between cells i-1 and i
        const int o = max(flag_at(solid, i - 1, j, k, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
            const float vo = ov.vx[o - 1];
            if (du) du[id] = vo - u[id];
            u[id] = vo;
        }
    }
    if (i < ni && k < nk) {                                         // v face between cells j-1 and j
        const int o = max(flag_at(solid, i, j - 1, k, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
            const float vo = ov.vy[o - 1];
            if (dv) dv[id] = vo - v[id];
            v[id] = vo;
        }
    }
    if (i < ni && j < nj) {                                         // w face between cells k-1 and k
        const int o = max(flag_at(solid, i, j, k - 1, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
            const float vo = ov.vz[o - 1];
            if (dw) dw[id] = vo - w[id];
            w[id] = vo;
        }
    }
}

// obstacle_faces_kernel for lists with spinning entries: a face owned by entry o with bit o of
// `spin` set takes the rigid velocity v + omega x (p - c) at its own sample position p, in gpu_emit_sources' operation order
struct ObsSpin {
    unsigned spin;
    float cx[BQ_MAX_BOUNDARIES], cy[BQ_MAX_BOUNDARIES], cz[BQ_MAX_BOUNDARIES];
    float ox[BQ_MAX_BOUNDARIES], oy[BQ_MAX_BOUNDARIES], oz[BQ_MAX_BOUNDARIES];
};
__global__ __launch_bounds__(256) void obstacle_faces_pose_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                                  float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                                  const unsigned char *__restrict__ solid, ObsVel ov, ObsSpin os,
                                                                  float h, int ni, int nj, int nk)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    const float x0 = obs_pos(i, 0, h), y0 = obs_pos(j, 0, h), z0 = obs_pos(k, 0, h);
    if (j < nj && k < nk) {                                         // u face between cells i-1 and i
        const int o = max(flag_at(solid, i - 1, j, k, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
            float vo = ov.vx[o - 1];
            if ((os.spin >> (o - 1)) & 1u) {
                const float dy = y0 - os.cy[o - 1], dz = z0 - os.cz[o - 1];
                vo = vo + (os.oy[o - 1] * dz - os.oz[o - 1] * dy);
            }
            if (du) du[id] = vo - u[id];
            u[id] = vo;
        }
    }
    if (i < ni && k < nk) {                                         // v face between cells j-1 and j
        const int o = max(flag_at(solid, i, j - 1, k, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
            float vo = ov.vy[o - 1];
            if ((os.spin >> (o - 1)) & 1u) {
                const float dx = x0 - os.cx[o - 1], dz = z0 - os.cz[o - 1];
                vo = vo + (os.oz[o - 1] * dx - os.ox[o - 1] * dz);
            }
            if (dv) dv[id] = vo - v[id];
            v[id] = vo;
        }
    }
    if (i < ni && j < nj) {                                         // w face between cells k-1 and k
        const int o = max(flag_at(solid, i, j, k - 1, ni, nj, nk), flag_at(solid, i, j, k, ni, nj, nk));
        if (o) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
            float vo = ov.vz[o - 1];
            if ((os.spin >> (o - 1)) & 1u) {
                const float dx = x0 - os.cx[o - 1], dy = y0 - os.cy[o - 1];
                vo = vo + (os.ox[o - 1] * dy - os.oy[o - 1] * dx);
            }
            if (dw) dw[id] = vo - w[id];
            w[id] = vo;
        }
    }
}

// ---- masked Jacobi sweep, one per launch ------------------------------------------------------------------------------
// Odd sweep counts and the test baseline of the fused masked sweeps (jacobi_lds_kernel<8, 1, 3, true>, bq_project.hip).  A
// cell whose rows summary is clean (no solid cell in its row or the neighbouring rows and planes) evaluates
// jacobi_generic_kernel's expression without reading a flag; the others skip solid cells and scale the same sum by beta_s.
// Solid cells hold +0 in both buffers, so their terms add +0: the sum is the Neumann sum over the fluid neighbours.
struct BetaTab { float b[7]; };
__global__ __launch_bounds__(256) void jacobi_masked_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                            float *__restrict__ out, const unsigned char *__restrict__ solid,
                                                            const unsigned char *__restrict__ rows,
                                                            int ni, int nj, int nk, float alpha, BetaTab bt)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (!(i > 0 && i < ni - 1 && j > 0 && j < nj - 1 && k > 0 && k < nk - 1)) return;
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t id = (size_t)i + sj * j + sk * k;
    if (!rows[(size_t)j + (size_t)nj * k]) {
        out[id] = (p[id - 1] + p[id + 1] + p[id - sj] + p[id + sj] + p[id - sk] + p[id + sk] + alpha * div[id]) * bt.b[0];
        return;
    }
    if (solid[id]) return;
    const int s = (solid[id - 1] != 0) + (solid[id + 1] != 0) + (solid[id - sj] != 0) + (solid[id + sj] != 0)
                + (solid[id - sk] != 0) + (solid[id + sk] != 0);
    const float sum = p[id - 1] + p[id + 1] + p[id - sj] + p[id + sj] + p[id - sk] + p[id + sk] + alpha * div[id];
    out[id] = s == 6 ? 0.f : sum * bt.b[s];
}

// ---- closed domain walls (BimocqSolver.cpp:938-948) --------------------------------------------------
// On a z-slab rank (fl_set_slab) every position below is GLOBAL: the kernels pass plane k + koff for k and the global plane count
// nkg for nk, so BQ_WALL_ZLO is global plane 0 and BQ_WALL_ZHI global plane nkg - 1 on whichever rank holds them, and a rank in
// the middle has x and y walls only.  One domain: koff = 0, nkg = nk -- the same expressions on the same operands.
struct SlabZ { int koff, nkg; };
// a border cell of a closed side
__device__ __forceinline__ bool wall_cell(int walls, int i, int j, int k, int ni, int nj, int nk)
{
    return ((walls & BQ_WALL_XLO) && i == 0) || ((walls & BQ_WALL_XHI) && i == ni - 1) || ((walls & BQ_WALL_YLO) && j == 0) ||
           ((walls & BQ_WALL_YHI) && j == nj - 1) || ((walls & BQ_WALL_ZLO) && k == 0) || ((walls & BQ_WALL_ZHI) && k == nk - 1);
}
// the solid neighbours of the interior cell (i, j, k) of a grid without obstacles nearby: the closed sides it touches
__device__ __forceinline__ int wall_neighbours(int walls, int i, int j, int k, int ni, int nj, int nk)
{
    return (int)((walls & BQ_WALL_XLO) && i == 1) + (int)((walls & BQ_WALL_XHI) && i == ni - 2) + (int)((walls & BQ_WALL_YLO) && j == 1) +
           (int)((walls & BQ_WALL_YHI) && j == nj - 2) + (int)((walls & BQ_WALL_ZLO) && k == 1) + (int)((walls & BQ_WALL_ZHI) && k == nk - 2);
}

// solidw = solid (or 0) with BQ_FLAG_WALL in the wall cells no obstacle covers: one thread per cell
// (a slab rank's planes outside the global grid hold no cell: flag 0)
__global__ __launch_bounds__(256) void wall_flags_kernel(unsigned char *__restrict__ solidw, const unsigned char *__restrict__ solid,
                                                         int walls, int ni, int nj, int nk, SlabZ sz)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i >= ni || j >= nj) return;
    const int kg = k + sz.koff;
    const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
    const unsigned char f = solid ? solid[id] : (unsigned char)0;
    const bool wall = kg >= 0 && kg < sz.nkg && wall_cell(walls, i, j, kg, ni, nj, sz.nkg);
    solidw[id] = f ? f : (wall ? (unsigned char)BQ_FLAG_WALL : (unsigned char)0);
}

// wall faces: one thread per node of the (ni+1, nj+1, nk+1) super-grid; a face takes 0 when one of its cells is a wall cell
// and neither is an obstacle cell (those faces are gpu_obstacle_faces')
__device__ __forceinline__ bool wall_face(int a, int b)
{
    return (a == BQ_FLAG_WALL || b == BQ_FLAG_WALL) && (a == 0 || a == BQ_FLAG_WALL) && (b == 0 || b == BQ_FLAG_WALL);
}
// z-slab ranks: the flags are those of the rank's window.  The cell below the window's first plane (above its last one) is not in
// it; where it lies inside the global grid it is taken to carry the flag of its neighbour inside the window -- exact for the x and
// y walls, which do not depend on the plane, and wrong only for the w face between the window and a closed z plane just outside it
// (window from global plane 1, or up to nkg - 2): that face is the outermost ghost face of w, and the host counts w's ghost
// planes one short after this pass.
__global__ __launch_bounds__(256) void wall_faces_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                         float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                         const unsigned char *__restrict__ solidw, int ni, int nj, int nk, SlabZ sz)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    const int kg = k + sz.koff;
    // the flag of cell (i, j, k): beyond the window but inside the grid, that of the nearest plane of the window
    const int kc = k == nk && kg < sz.nkg ? nk - 1 : k;
    const int c = flag_at(solidw, i, j, kc, ni, nj, nk);
    if (j < nj && k < nk && wall_face(flag_at(solidw, i - 1, j, k, ni, nj, nk), c)) {
        const size_t id = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
        if (du) du[id] = 0.f - u[id];
        u[id] = 0.f;
    }
    if (i < ni && k < nk && wall_face(flag_at(solidw, i, j - 1, k, ni, nj, nk), c)) {
        const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
        if (dv) dv[id] = 0.f - v[id];
        v[id] = 0.f;
    }
    if (i < ni && j < nj && wall_face(flag_at(solidw, i, j, k == 0 && kg > 0 ? 0 : k - 1, ni, nj, nk), c)) {
        const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
        if (dw) dw[id] = 0.f - w[id];
        w[id] = 0.f;
    }
}

// jacobi_masked_kernel with walls: a cell whose (obstacle) rows summary is clean counts its solid neighbours by position and
// reads no flag; the others read the flags of solid + walls.  [klo, khi): the local planes of the launch, one per blockIdx.z
// (gpu_jacobi_sweep_masked_walls_range; whole arrays: [0, nk)); planes outside the interior of the global grid keep their value, as in the unmasked sweeps
__global__ __launch_bounds__(256) void jacobi_masked_walls_kernel(const float *__restrict__ p, const float *__restrict__ div,
                                                                  float *__restrict__ out, const unsigned char *__restrict__ solidw,
                                                                  const unsigned char *__restrict__ rows, int walls,
                                                                  int ni, int nj, int nk, float alpha, BetaTab bt, SlabZ sz, int klo, int khi)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = klo + blockIdx.z;
    const int kg = k + sz.koff;
    if (!(i > 0 && i < ni - 1 && j > 0 && j < nj - 1 && k > 0 && k < nk - 1 && kg > 0 && kg < sz.nkg - 1 && k < khi)) return;
    const size_t sj = ni, sk = (size_t)ni * nj;
    const size_t id = (size_t)i + sj * j + sk * k;
    int s;
    if (!rows[(size_t)j + (size_t)nj * k]) {
        s = wall_neighbours(walls, i, j, kg, ni, nj, sz.nkg);
    } else {
        if (solidw[id]) return;
        s = (solidw[id - 1] != 0) + (solidw[id + 1] != 0) + (solidw[id - sj] != 0) + (solidw[id + sj] != 0)
          + (solidw[id - sk] != 0) + (solidw[id + sk] != 0);
    }
    const float sum = p[id - 1] + p[id + 1] + p[id - sj] + p[id + sj] + p[id - sk] + p[id + sk] + alpha * div[id];
    out[id] = s == 6 ? 0.f : sum * bt.b[s];
}

// ---- masked gradient (gradient_delta_kernel / gradient_kernel with solid faces left alone) ----------------------------
// i0, j0, k0: the first cell index of the window on each axis -- 2 (the open-boundary window of gradient_kernel), or 1 behind a
// closed wall (gradient_masked_walls_kernel), where the faces between the cells of the first interior layer are projected too;
// along z the window is that of the GLOBAL planes (sz)
__device__ __forceinline__ void gradient_masked_body(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                     const float *__restrict__ p,
                                                     float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                     const unsigned char *__restrict__ solid, int ni, int nj, int nk, float halfrdx,
                                                     int i0, int j0, int k0, SlabZ sz)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    const int kg = k + sz.koff;
    const bool win = !(i < i0 || i >= ni || j < j0 || j >= nj || kg < k0 || kg >= sz.nkg || k >= nk);
    const size_t iu = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
    const size_t iv = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
    const size_t ic = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
    const bool hu = j < nj && k < nk, hv = i < ni && k < nk, hw = i < ni && j < nj;
    const bool su = hu && (flag_at(solid, i - 1, j, k, ni, nj, nk) | flag_at(solid, i, j, k, ni, nj, nk));
    const bool sv = hv && (flag_at(solid, i, j - 1, k, ni, nj, nk) | flag_at(solid, i, j, k, ni, nj, nk));
    const bool sw = hw && (flag_at(solid, i, j, k - 1, ni, nj, nk) | flag_at(solid, i, j, k, ni, nj, nk));
    if (win) {
        const float p0 = p[ic];
        if (!su) {
            const float uo = u[iu], un = uo - halfrdx * (p0 - p[ic - 1]);
            u[iu] = un;
            if (du) du[iu] = un - uo;
        }
        if (!sv) {
            const float vo = v[iv], vn = vo - halfrdx * (p0 - p[ic - ni]);
            v[iv] = vn;
            if (dv) dv[iv] = vn - vo;
        }
        if (!sw && k >= 1) {
            const float wo = w[ic], wn = wo - halfrdx * (p0 - p[ic - (size_t)ni * nj]);
            w[ic] = wn;
            if (dw) dw[ic] = wn - wo;
        } else if (!sw && dw) dw[ic] = 0.f;      // a slab rank's first plane inside the window: w needs the plane below (gradient_kernel)
    } else if (du) {
        if (hu && !su) du[iu] = 0.f;
        if (hv && !sv) dv[iv] = 0.f;
        if (hw && !sw) dw[ic] = 0.f;
    }
}
__global__ __launch_bounds__(256) void gradient_masked_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                              const float *__restrict__ p,
                                                              float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                              const unsigned char *__restrict__ solid, int ni, int nj, int nk, float halfrdx)
{
    gradient_masked_body(u, v, w, p, du, dv, dw, solid, ni, nj, nk, halfrdx, 2, 2, 2, SlabZ{0, nk});
}
// closed domain walls: the window starts at cell 1 behind a closed low side (BimocqSolver.cpp:1288-1335
// updates every face between two fluid cells); the faces of the wall cells themselves are solid faces and stay alone
__global__ __launch_bounds__(256) void gradient_masked_walls_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                                    const float *__restrict__ p,
                                                                    float *__restrict__ du, float *__restrict__ dv, float *__restrict__ dw,
                                                                    const unsigned char *__restrict__ solidw, int walls,
                                                                    int ni, int nj, int nk, float halfrdx, SlabZ sz)
{
    gradient_masked_body(u, v, w, p, du, dv, dw, solidw, ni, nj, nk, halfrdx, (walls & BQ_WALL_XLO) ? 1 : 2, (walls & BQ_WALL_YLO) ? 1 : 2,
                         (walls & BQ_WALL_ZLO) ? 1 : 2, sz);
}

// ---- band blend + density clear: one thread per super-grid node -------------------------------------------------------
template <typename... Ls>
__global__ __launch_bounds__(256) void obstacle_blend_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                             float *__restrict__ rho, float *__restrict__ T,
                                                             const float *__restrict__ us, const float *__restrict__ vs,
                                                             const float *__restrict__ ws, const float *__restrict__ rhos,
                                                             const float *__restrict__ Ts, const unsigned char *__restrict__ solid,
                                                             ObsSet ob, Ls... ls, float h, int ni, int nj, int nk)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = blockIdx.z;
    if (i > ni || j > nj || k > nk) return;
    const float x0 = obs_pos(i, 0, h), y0 = obs_pos(j, 0, h), z0 = obs_pos(k, 0, h);
    const float x1 = obs_pos(i, 1, h), y1 = obs_pos(j, 1, h), z1 = obs_pos(k, 1, h);
    if (us) {
        if (j < nj && k < nk && obs_classify(x1, y0, z0, ob, ls...) == -1) {
            const size_t id = (size_t)i + (size_t)(ni + 1) * ((size_t)j + (size_t)nj * k);
            u[id] = us[id];
        }
        if (i < ni && k < nk && obs_classify(x0, y1, z0, ob, ls...) == -1) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)(nj + 1) * k);
            v[id] = vs[id];
        }
        if (i < ni && j < nj && obs_classify(x0, y0, z1, ob, ls...) == -1) {
            const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
            w[id] = ws[id];
        }
    }
    if (i < ni && j < nj && k < nk) {
        const size_t id = (size_t)i + (size_t)ni * ((size_t)j + (size_t)nj * k);
        if (us && obs_classify(x0, y0, z0, ob, ls...) == -1) { rho[id] = rhos[id]; T[id] = Ts[id]; }
        if (solid[id]) rho[id] = 0.f;
    }
}

// slab_ok: the operator honours the z-slab context (the wall operators); every other one refuses a slab rank
static bool obs_args_ok(const bq_boundary *b, int n, int ni, int nj, int nk, const char *op, bool slab_ok = false)
{
    if (!ensure_ready(op)) return false;
    if (!obstacle_dims_ok(ni, nj, nk, op)) return false;
    if (n < 0 || n > BQ_MAX_BOUNDARIES || (n > 0 && !b)) { latch(FL_ERR_BAD_ARGUMENT, op, "1 .. 16 obstacles"); return false; }
    if (rt().slab_on && !slab_ok) { latch(FL_ERR_UNSUPPORTED, op, "obstacles on z-slab ranks"); return false; }
    return true;
}

// gpu_obstacle_flags and gpu_obstacle_blend with (ls non-NULL) and without level sets, with (pose non-NULL) and without
// poses: one set of checks, and the analytic kernels whenever there are no descriptors
static void obstacle_flags(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                           const bq_pose *pose, float h, int ni, int nj, int nk, const char *op)
{
    if (!obs_args_ok(b, n, ni, nj, nk, op)) return;
    if (const char *why = ls_check(b, ls, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    if (const char *why = pose_check(pose, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    if (!solid || !rows) { latch(FL_ERR_BAD_ARGUMENT, op, "null device pointer"); return; }
    if (!BQ_HIP(hipMemsetAsync(rows, 0, (size_t)nj * (size_t)nk, rt().compute))) return;
    if (pose && ls)
        obstacle_flags_kernel<LsSet, PoseSet><<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(solid, rows, make_obs(b, n, h), make_ls(b, ls, n), make_pose(b, pose, n), h, ni, nj, nk);
    else if (pose)
        obstacle_flags_kernel<PoseSet><<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(solid, rows, make_obs(b, n, h), make_pose(b, pose, n), h, ni, nj, nk);
    else if (ls)
        obstacle_flags_kernel<LsSet><<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(solid, rows, make_obs(b, n, h), make_ls(b, ls, n), h, ni, nj, nk);
    else
        obstacle_flags_kernel<><<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(solid, rows, make_obs(b, n, h), h, ni, nj, nk);
    BQ_LAUNCH_CHECK("obstacle_flags_kernel");
}

static void obstacle_blend(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                           const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                           const bq_boundary *b, int n, const bq_levelset *ls, const bq_pose *pose, float h, int ni, int nj, int nk,
                           const char *op)
{
    if (!obs_args_ok(b, n, ni, nj, nk, op)) return;
    if (const char *why = ls_check(b, ls, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    if (const char *why = pose_check(pose, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    if (!rho || !solid || (us && (!u || !v || !w || !T || !vs || !ws || !rhos || !Ts))) { latch(FL_ERR_BAD_ARGUMENT, op, "null device pointer"); return; }
    const dim3 grid = grid_for(ni + 1, nj + 1, nk + 1);
    if (pose && ls)
        obstacle_blend_kernel<LsSet, PoseSet><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, make_obs(b, n, h), make_ls(b, ls, n), make_pose(b, pose, n), h, ni, nj, nk);
    else if (pose)
        obstacle_blend_kernel<PoseSet><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, make_obs(b, n, h), make_pose(b, pose, n), h, ni, nj, nk);
    else if (ls)
        obstacle_blend_kernel<LsSet><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, make_obs(b, n, h), make_ls(b, ls, n), h, ni, nj, nk);
    else
        obstacle_blend_kernel<><<<grid, kBlock, 0, rt().compute>>>(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, make_obs(b, n, h), h, ni, nj, nk);
    BQ_LAUNCH_CHECK("obstacle_blend_kernel");
}

bool jacobi_sweep_triple_masked(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                                const unsigned char *solid, const unsigned char *rows, const float betas[7], int walls = 0);   // bq_project.hip
bool jacobi_sweep_triple_masked_ranges(const plan::JacobiTuning &tun, const float *in, const float *div, float *out, int ni, int nj, int nk, float alpha,
                                       const unsigned char *solid, const unsigned char *rows, const float betas[7], int walls,
                                       const geom::PlaneRanges &pr);                                                          // bq_project.hip

// the z-slab context of the wall operators (slab_ctx): the global plane of local plane 0 and the global plane count
static inline SlabZ slab_z(int nk) { SlabZ z; slab_ctx(nk, z.koff, z.nkg); return z; }

} // namespace bq

using namespace bq;

extern "C" {

void gpu_obstacle_flags(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, float h, int ni, int nj, int nk)
{
    obstacle_flags(solid, rows, b, n, nullptr, nullptr, h, ni, nj, nk, "gpu_obstacle_flags");
}

// the velocities of a list, by entry, as the faces kernels take them
static ObsVel make_obs_vel(const bq_boundary *b, int n)
{
    ObsVel ov{};
    for (int o = 0; o < n; o++) { ov.vx[o] = b[o].vx; ov.vy[o] = b[o].vy; ov.vz[o] = b[o].vz; }
    return ov;
}

// the pointers of a faces pass: three components, the flags, and all three deltas or none
static bool faces_ptrs_ok(const float *u, const float *v, const float *w, const float *du, const float *dv, const float *dw,
                          const unsigned char *solid, const char *op)
{
    if (u && v && w && solid && (!du) == (!dv) && (!du) == (!dw)) return true;
    latch(FL_ERR_BAD_ARGUMENT, op, "null device pointer");
    return false;
}

void gpu_obstacle_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                        const bq_boundary *b, int n, int ni, int nj, int nk)
{
    if (!obs_args_ok(b, n, ni, nj, nk, "gpu_obstacle_faces") || !faces_ptrs_ok(u, v, w, du, dv, dw, solid, "gpu_obstacle_faces")) return;
    obstacle_faces_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, du, dv, dw, solid, make_obs_vel(b, n), ni, nj, nk);
    BQ_LAUNCH_CHECK("obstacle_faces_kernel");
}

static BetaTab beta_table(float beta)
{
    BetaTab t;
    t.b[0] = beta;
    for (int s = 1; s < 6; s++) t.b[s] = (float)(1.0 / (1.0 / (double)beta - (double)s));
    t.b[6] = 0.f;
    return t;
}

static bool walls_ok(int walls, const char *op)
{
    if (walls >= 0 && walls < 63) return true;
    latch(FL_ERR_BAD_ARGUMENT, op, "walls: BQ_WALL_* bits, at least one side open");
    return false;
}

// The argument check of the masked sweep entry points.  kNone: the family without walls, which refuses a slab rank; kAny: a walled entry
// point (walls = 0 is forwarded to the family without walls before it gets here); kClosed: the walled sweeps on plane ranges of a z-slab
// rank's schedule, which refuse walls = 0 -- the masked family without walls has no sweep on plane ranges.
enum class Walls { kNone, kAny, kClosed };
static bool masked_sweep_args(const float *in, const float *div, const float *out, const unsigned char *solid, const unsigned char *rows,
                              int ni, int nj, int nk, const char *op, Walls kind = Walls::kNone, int walls = 0)
{
    if (!obs_args_ok(nullptr, 0, ni, nj, nk, op, kind != Walls::kNone)) return false;
    if (kind == Walls::kAny && !walls_ok(walls, op)) return false;
    if (kind == Walls::kClosed && (walls <= 0 || walls >= 63)) { latch(FL_ERR_BAD_ARGUMENT, op, "walls: BQ_WALL_* bits, at least one side closed and one open"); return false; }
    if (!in || !div || !out || !solid || !rows || in == out) { latch(FL_ERR_BAD_ARGUMENT, op, "null or aliased buffers"); return false; }
    return true;
}

// One masked sweep in -> out: jacobi_masked_kernel, or with walls (solid then being solid + walls) jacobi_masked_walls_kernel on
// the local planes [klo, khi).  false: the launch check failed (latched).
static bool masked_sweep(const float *in, const float *div, float *out, const unsigned char *solid, const unsigned char *rows, int walls,
                         int ni, int nj, int nk, float alpha, const BetaTab &bt, int klo, int khi)
{
    if (walls == 0) {
        jacobi_masked_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(in, div, out, solid, rows, ni, nj, nk, alpha, bt);
        return BQ_LAUNCH_CHECK("jacobi_masked_kernel");
    }
    jacobi_masked_walls_kernel<<<grid_for(ni, nj, khi - klo), kBlock, 0, rt().compute>>>(in, div, out, solid, rows, walls, ni, nj, nk, alpha, bt,
                                                                                        slab_z(nk), klo, khi);
    return BQ_LAUNCH_CHECK("jacobi_masked_walls_kernel");
}

// `sweeps` checked masked sweeps.  FL_OPT_JACOBI_FUSE >= 2 (the caller vouches that p and p_temp carry the same boundary layer and the same
// values in solid cells): three sweeps per launch through the masked LDS kernel where plan_triple_masked admits the shape
static int masked_sweeps(float *p, const float *div, float *p_temp, const unsigned char *solid, const unsigned char *rows, int walls,
                         int ni, int nj, int nk, int sweeps, float alpha, float beta)
{
    const BetaTab bt = beta_table(beta);
    const plan::JacobiTuning tun = jacobi_tuning();
    return run_sweeps(p, p_temp, sweeps,
                      {{3, tun.sweeps_fuse == plan::SweepsFuse::kAll, [&](const float *in, float *out) {
                            return jacobi_sweep_triple_masked(tun, in, div, out, ni, nj, nk, alpha, solid, rows, bt.b, walls); }}},
                      [&](const float *in, float *out) { return masked_sweep(in, div, out, solid, rows, walls, ni, nj, nk, alpha, bt, 0, nk); });
}

void gpu_jacobi_sweep_masked(const float *in, const float *div, float *out, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, float alpha, float beta)
{
    if (!masked_sweep_args(in, div, out, solid, rows, ni, nj, nk, "gpu_jacobi_sweep_masked")) return;
    masked_sweep(in, div, out, solid, rows, 0, ni, nj, nk, alpha, beta_table(beta), 0, nk);
}

int gpu_jacobi_sweeps_masked(float *p, const float *div, float *p_temp, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, int sweeps, float alpha, float beta)
{
    if (!masked_sweep_args(p, div, p_temp, solid, rows, ni, nj, nk, "gpu_jacobi_sweeps_masked")) return 0;
    return masked_sweeps(p, div, p_temp, solid, rows, 0, ni, nj, nk, sweeps, alpha, beta);
}

void gpu_wall_flags(unsigned char *solidw, const unsigned char *solid, int walls, int ni, int nj, int nk)
{
    if (!obs_args_ok(nullptr, 0, ni, nj, nk, "gpu_wall_flags", true) || !walls_ok(walls, "gpu_wall_flags")) return;
    if (!solidw || solidw == solid) { latch(FL_ERR_BAD_ARGUMENT, "gpu_wall_flags", "null or aliased buffers"); return; }
    wall_flags_kernel<<<grid_for(ni, nj, nk), kBlock, 0, rt().compute>>>(solidw, solid, walls, ni, nj, nk, slab_z(nk));
    BQ_LAUNCH_CHECK("wall_flags_kernel");
}

void gpu_wall_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solidw, int ni, int nj, int nk)
{
    if (!obs_args_ok(nullptr, 0, ni, nj, nk, "gpu_wall_faces", true) || !faces_ptrs_ok(u, v, w, du, dv, dw, solidw, "gpu_wall_faces")) return;
    wall_faces_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, du, dv, dw, solidw, ni, nj, nk, slab_z(nk));
    BQ_LAUNCH_CHECK("wall_faces_kernel");
}

void gpu_jacobi_sweep_masked_walls(const float *in, const float *div, float *out, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, float alpha, float beta)
{
    if (walls == 0) { gpu_jacobi_sweep_masked(in, div, out, solidw, rows, ni, nj, nk, alpha, beta); return; }
    if (!masked_sweep_args(in, div, out, solidw, rows, ni, nj, nk, "gpu_jacobi_sweep_masked_walls", Walls::kAny, walls)) return;
    masked_sweep(in, div, out, solidw, rows, walls, ni, nj, nk, alpha, beta_table(beta), 0, nk);
}

// one walled sweep in -> out on the local planes [k_begin, k_end), clipped to the interior: returns 1 (0: refused arguments)
int gpu_jacobi_sweep_masked_walls_range(const float *in, const float *div, float *out, const unsigned char *solidw,
                                        const unsigned char *rows, int walls, int ni, int nj, int nk, int k_begin, int k_end,
                                        float alpha, float beta)
{
    if (!masked_sweep_args(in, div, out, solidw, rows, ni, nj, nk, "gpu_jacobi_sweep_masked_walls_range", Walls::kClosed, walls)) return 0;
    const int k0 = std::max(k_begin, 1), k1 = std::min(k_end, nk - 1);
    if (k0 < k1) masked_sweep(in, div, out, solidw, rows, walls, ni, nj, nk, alpha, beta_table(beta), k0, k1);
    return 1;
}

// three walled sweeps in one launch, `out` written on the planes [k0a, k1a) and [k0b, k1b) (either may be empty): the input must
// be valid three planes beyond each range, and both buffers carry the same boundary layer.  Returns 1 when the kernel ran, 0 when
// it does not apply (nothing launched): the shapes the whole-array walled triple refuses, and FL_OPT_JACOBI_FUSE = 0 or 4.
int gpu_jacobi_sweep_masked_walls_triple_ranges(const float *in, const float *div, float *out, const unsigned char *solidw,
                                                const unsigned char *rows, int walls, int ni, int nj, int nk,
                                                int k0a, int k1a, int k0b, int k1b, float alpha, float beta)
{
    if (!masked_sweep_args(in, div, out, solidw, rows, ni, nj, nk, "gpu_jacobi_sweep_masked_walls_triple_ranges", Walls::kClosed, walls)) return 0;
    const BetaTab bt = beta_table(beta);
    return jacobi_sweep_triple_masked_ranges(jacobi_tuning(), in, div, out, ni, nj, nk, alpha, solidw, rows, bt.b, walls,
                                             geom::PlaneRanges(k0a, k1a, k0b, k1b, nk)) ? 1 : 0;
}

int gpu_jacobi_sweeps_masked_walls(float *p, const float *div, float *p_temp, const unsigned char *solidw, const unsigned char *rows,
                                   int walls, int ni, int nj, int nk, int sweeps, float alpha, float beta)
{
    if (walls == 0) return gpu_jacobi_sweeps_masked(p, div, p_temp, solidw, rows, ni, nj, nk, sweeps, alpha, beta);
    if (!masked_sweep_args(p, div, p_temp, solidw, rows, ni, nj, nk, "gpu_jacobi_sweeps_masked_walls", Walls::kAny, walls)) return 0;
    return masked_sweeps(p, div, p_temp, solidw, rows, walls, ni, nj, nk, sweeps, alpha, beta);
}

void gpu_gradient_masked(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                         const unsigned char *solid, int ni, int nj, int nk, float halfrdx)
{
    if (!obs_args_ok(nullptr, 0, ni, nj, nk, "gpu_gradient_masked")) return;
    if (!u || !v || !w || !p || !solid || (!du) != (!dv) || (!du) != (!dw)) { latch(FL_ERR_BAD_ARGUMENT, "gpu_gradient_masked", "null device pointer"); return; }
    gradient_masked_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, p, du, dv, dw, solid, ni, nj, nk, halfrdx);
    BQ_LAUNCH_CHECK("gradient_masked_kernel");
}

void gpu_gradient_masked_walls(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                               const unsigned char *solidw, int walls, int ni, int nj, int nk, float halfrdx)
{
    if (walls == 0) { gpu_gradient_masked(u, v, w, p, du, dv, dw, solidw, ni, nj, nk, halfrdx); return; }
    if (!obs_args_ok(nullptr, 0, ni, nj, nk, "gpu_gradient_masked_walls", true) || !walls_ok(walls, "gpu_gradient_masked_walls")) return;
    if (!u || !v || !w || !p || !solidw || (!du) != (!dv) || (!du) != (!dw)) { latch(FL_ERR_BAD_ARGUMENT, "gpu_gradient_masked_walls", "null device pointer"); return; }
    gradient_masked_walls_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, p, du, dv, dw, solidw, walls, ni, nj, nk, halfrdx, slab_z(nk));
    BQ_LAUNCH_CHECK("gradient_masked_walls_kernel");
}

void gpu_obstacle_blend(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                        const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                        const bq_boundary *b, int n, float h, int ni, int nj, int nk)
{
    obstacle_blend(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, nullptr, nullptr, h, ni, nj, nk, "gpu_obstacle_blend");
}

void gpu_obstacle_flags_ls(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                           float h, int ni, int nj, int nk)
{
    obstacle_flags(solid, rows, b, n, ls, nullptr, h, ni, nj, nk, "gpu_obstacle_flags_ls");
}

void gpu_obstacle_blend_ls(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                           const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                           const bq_boundary *b, int n, const bq_levelset *ls, float h, int ni, int nj, int nk)
{
    obstacle_blend(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, ls, nullptr, h, ni, nj, nk, "gpu_obstacle_blend_ls");
}

void gpu_obstacle_flags_pose(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                             const bq_pose *pose, float h, int ni, int nj, int nk)
{
    obstacle_flags(solid, rows, b, n, ls, pose, h, ni, nj, nk, pose ? "gpu_obstacle_flags_pose" : "gpu_obstacle_flags_ls");
}

void gpu_obstacle_blend_pose(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                             const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                             const bq_boundary *b, int n, const bq_levelset *ls, const bq_pose *pose, float h, int ni, int nj, int nk)
{
    obstacle_blend(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, ls, pose, h, ni, nj, nk,
                   pose ? "gpu_obstacle_blend_pose" : "gpu_obstacle_blend_ls");
}

void gpu_obstacle_faces_pose(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                             const bq_boundary *b, const bq_pose *pose, int n, float h, int ni, int nj, int nk)
{
    const char *op = "gpu_obstacle_faces_pose";
    if (!obs_args_ok(b, n, ni, nj, nk, op)) return;
    if (const char *why = pose_check(pose, n)) { latch(FL_ERR_BAD_ARGUMENT, op, why); return; }
    ObsSpin os{};
    for (int o = 0; pose && o < n; o++) {
        if (!pose_spins(pose[o])) continue;
        os.spin |= 1u << o;
        os.cx[o] = b[o].cx; os.cy[o] = b[o].cy; os.cz[o] = b[o].cz;
        os.ox[o] = pose[o].ox; os.oy[o] = pose[o].oy; os.oz[o] = pose[o].oz;
    }
    if (!os.spin) { gpu_obstacle_faces(u, v, w, du, dv, dw, solid, b, n, ni, nj, nk); return; }
    if (!faces_ptrs_ok(u, v, w, du, dv, dw, solid, op)) return;
    obstacle_faces_pose_kernel<<<grid_for(ni + 1, nj + 1, nk + 1), kBlock, 0, rt().compute>>>(u, v, w, du, dv, dw, solid, make_obs_vel(b, n), os, h, ni, nj, nk);
    BQ_LAUNCH_CHECK("obstacle_faces_pose_kernel");
}

} // extern "C"
