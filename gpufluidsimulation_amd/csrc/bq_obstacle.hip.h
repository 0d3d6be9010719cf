// bq_obstacle.hip.h -- the obstacle list as a kernel argument and the one classification every obstacle kernel uses
// (squared distances, no sqrt, so that flags are the same bits on the CPU stand-in and the GPU).
#pragma once
#include <hip/hip_runtime.h>
#include "bimocq_gpu.h"
#include "bq_levelset.h"
#include "bq_pose.h"

#include <cmath>
#include <type_traits>

namespace bq {

struct ObsSet {
    int n;
    float h3;                                   // band width 3 h
    int shape[BQ_MAX_BOUNDARIES];
    float cx[BQ_MAX_BOUNDARIES], cy[BQ_MAX_BOUNDARIES], cz[BQ_MAX_BOUNDARIES];
    float rx[BQ_MAX_BOUNDARIES], ry[BQ_MAX_BOUNDARIES], rz[BQ_MAX_BOUNDARIES];
};

struct ObsVel { float vx[BQ_MAX_BOUNDARIES], vy[BQ_MAX_BOUNDARIES], vz[BQ_MAX_BOUNDARIES]; };

static inline ObsSet make_obs(const bq_boundary *b, int n, float h)
{
    ObsSet s{};
    s.n = n;
    s.h3 = 3.0f * h;
    for (int o = 0; o < n; o++) {
        s.shape[o] = b[o].shape;
        s.cx[o] = b[o].cx; s.cy[o] = b[o].cy; s.cz[o] = b[o].cz;
        s.rx[o] = b[o].rx; s.ry[o] = b[o].ry; s.rz[o] = b[o].rz;
    }
    return s;
}

// the level sets of a list (entries whose shape is BQ_SHAPE_LEVELSET; the others are left empty).  A kernel takes the
// list as `ObsSet ob, Ls... ls`: the pack Ls is empty for lists without level sets and LsSet for the others.  (As one
// aggregate kernel argument, the level-set band semi-Lagrangian kernel's trace is scheduled for fewer waves.)
struct LsSet {
    const float *phi[BQ_MAX_BOUNDARIES];
    int nx[BQ_MAX_BOUNDARIES], ny[BQ_MAX_BOUNDARIES], nz[BQ_MAX_BOUNDARIES];
    int i0[BQ_MAX_BOUNDARIES], j0[BQ_MAX_BOUNDARIES], k0[BQ_MAX_BOUNDARIES];
    float voxel[BQ_MAX_BOUNDARIES], bg[BQ_MAX_BOUNDARIES];
};

static inline LsSet make_ls(const bq_boundary *b, const bq_levelset *ls, int n)
{
    LsSet s{};
    for (int o = 0; o < n; o++) {
        if (b[o].shape != BQ_SHAPE_LEVELSET) continue;
        const bq_levelset &l = ls[o];
        s.phi[o] = l.phi;
        s.nx[o] = l.nx; s.ny[o] = l.ny; s.nz[o] = l.nz;
        s.i0[o] = l.i0; s.j0[o] = l.j0; s.k0[o] = l.k0;
        s.voxel[o] = l.voxel; s.bg[o] = l.background;
    }
    return s;
}

// p + (q - p) t with the difference and the sum in float and the product in double (BoxSampler's lerp)
__device__ __forceinline__ float ls_lerp(float p, float q, double t) { return p + (float)((double)(q - p) * t); }

// trilinear sample of level set o at the position (gx, gy, gz) of its own index space ("Level sets").
// false when all eight corners lie outside the stored nodes (the sample is exactly the background there): the exact
// early-out, taken before any load.  Otherwise corners outside the stored nodes read the background.
__device__ __forceinline__ bool ls_sample_index(const LsSet &l, int o, double gx, double gy, double gz, float &sdf)
{
    const int nx = l.nx[o], ny = l.ny[o], nz = l.nz[o], i0 = l.i0[o], j0 = l.j0[o], k0 = l.k0[o];
    if (gx < (double)(i0 - 1) || gx >= (double)(i0 + nx) || gy < (double)(j0 - 1) || gy >= (double)(j0 + ny) ||
        gz < (double)(k0 - 1) || gz >= (double)(k0 + nz))
        return false;
    const double fx = floor(gx), fy = floor(gy), fz = floor(gz);
    const double tx = gx - fx, ty = gy - fy, tz = gz - fz;
    const int ia = (int)fx - i0, ja = (int)fy - j0, ka = (int)fz - k0;     // corners a = -1 .. n-1 and a + 1
    const float bg = l.bg[o];
    const float *phi = l.phi[o];
    const bool xa = ia >= 0, xb = ia + 1 < nx, ya = ja >= 0, yb = ja + 1 < ny, za = ka >= 0, zb = ka + 1 < nz;
    const size_t sy = (size_t)nx, sz = (size_t)nx * (size_t)ny;
    const float *c = phi + (ptrdiff_t)ia + (ptrdiff_t)ja * (ptrdiff_t)sy + (ptrdiff_t)ka * (ptrdiff_t)sz;   // corner (a, a, a)
    const float v000 = xa && ya && za ? c[0] : bg,           v001 = xa && ya && zb ? c[sz] : bg;
    const float v010 = xa && yb && za ? c[sy] : bg,          v011 = xa && yb && zb ? c[sy + sz] : bg;
    const float v100 = xb && ya && za ? c[1] : bg,           v101 = xb && ya && zb ? c[1 + sz] : bg;
    const float v110 = xb && yb && za ? c[1 + sy] : bg,      v111 = xb && yb && zb ? c[1 + sy + sz] : bg;
    const float a0 = ls_lerp(ls_lerp(v000, v001, tz), ls_lerp(v010, v011, tz), ty);
    const float a1 = ls_lerp(ls_lerp(v100, v101, tz), ls_lerp(v110, v111, tz), ty);
    sdf = ls_lerp(a0, a1, tx);
    return true;
}
// ... at the world point (x, y, z), the index origin at (cx, cy, cz): index = (point - origin) / voxel in double
__device__ __forceinline__ bool ls_sample(const LsSet &l, int o, float x, float y, float z, float cx, float cy, float cz,
                                          float &sdf)
{
    const double vox = (double)l.voxel[o];
    const double gx = ((double)x - (double)cx) / vox, gy = ((double)y - (double)cy) / vox, gz = ((double)z - (double)cz) / vox;
    return ls_sample_index(l, o, gx, gy, gz, sdf);
}

// the rotations of a list with poses, one more optional element of the pack after LsSet: bit o of
// `oriented` marks the entries classified in body coordinates, r[3 a + c][o] is R_ac (body -> world) of entry o.
struct PoseSet {
    unsigned oriented;
    float r[9][BQ_MAX_BOUNDARIES];
};

static inline PoseSet make_pose(const bq_boundary *b, const bq_pose *pose, int n)
{
    PoseSet s{};
    for (int o = 0; o < n; o++) {
        if (!pose_oriented(b[o], pose[o])) continue;
        float R[9];
        pose_matrix(pose[o], R);
        s.oriented |= 1u << o;
        for (int m = 0; m < 9; m++) s.r[m][o] = R[m];
    }
    return s;
}

// the pack of a kernel: <>, <LsSet>, <PoseSet> or <LsSet, PoseSet>
template <typename T, typename... A> inline constexpr bool pack_has = (std::is_same_v<T, A> || ...);
template <typename... A> inline constexpr bool pack_ok = (sizeof...(A) == 0) || (sizeof...(A) == 1 && (pack_has<LsSet, A...> || pack_has<PoseSet, A...>)) ||
                                                         (sizeof...(A) == 2 && pack_has<LsSet, A...> && pack_has<PoseSet, A...>);
template <typename T, typename A0, typename... A>
__device__ __forceinline__ const T &pack_get(const A0 &a0, const A &...a)
{
    if constexpr (std::is_same_v<T, A0>) return a0;
    else return pack_get<T>(a...);
}

// o + 1 when obstacle o is the last one covering (x, y, z); -1 when the point lies in the band of some obstacle and
// inside none; 0 otherwise.  Without ls: analytic entries only; with an LsSet in ls: level-set entries are sampled, solid
// when the sample is <= 0, band when 0 < sample < background; with a PoseSet in ls: its oriented entries are classified
// in body coordinates.
template <typename... Ls>
__device__ __forceinline__ int obs_classify(float x, float y, float z, const ObsSet &s, const Ls &...ls)
{
    static_assert(pack_ok<Ls...>, "one LsSet and one PoseSet at most");
    int solid = 0;
    bool band = false;
    for (int o = 0; o < s.n; o++) {
        if constexpr (pack_has<PoseSet, Ls...>) {
            const PoseSet &ps = pack_get<PoseSet>(ls...);
            if ((ps.oriented >> o) & 1u) {                  // body coordinates R^T d, each product and sum one float operation
                const float dx = x - s.cx[o], dy = y - s.cy[o], dz = z - s.cz[o];
                const float bx = ps.r[0][o] * dx + ps.r[3][o] * dy + ps.r[6][o] * dz;
                const float by = ps.r[1][o] * dx + ps.r[4][o] * dy + ps.r[7][o] * dz;
                const float bz = ps.r[2][o] * dx + ps.r[5][o] * dy + ps.r[8][o] * dz;
                if (s.shape[o] == BQ_SHAPE_LEVELSET) {
                    if constexpr (pack_has<LsSet, Ls...>) {
                        const LsSet &l = pack_get<LsSet>(ls...);
                        const double vox = (double)l.voxel[o];
                        float sdf;
                        if (ls_sample_index(l, o, (double)bx / vox, (double)by / vox, (double)bz / vox, sdf)) {
                            if (sdf <= 0.f) solid = o + 1;
                            else if (sdf < l.bg[o]) band = true;
                        }
                    }
                } else {
                    const float ax = fabsf(bx) - s.rx[o], ay = fabsf(by) - s.ry[o], az = fabsf(bz) - s.rz[o];
                    if (ax <= 0.f && ay <= 0.f && az <= 0.f) {
                        solid = o + 1;
                    } else {
                        const float qx = fmaxf(ax, 0.f), qy = fmaxf(ay, 0.f), qz = fmaxf(az, 0.f);
                        const float d2 = qx * qx + qy * qy + qz * qz;
                        if (d2 > 0.f && d2 < s.h3 * s.h3) band = true;
                    }
                }
                continue;
            }
        }
        if constexpr (pack_has<LsSet, Ls...>) {
            if (s.shape[o] == BQ_SHAPE_LEVELSET) {
                const LsSet &l = pack_get<LsSet>(ls...);
                float sdf;
                if (ls_sample(l, o, x, y, z, s.cx[o], s.cy[o], s.cz[o], sdf)) {
                    if (sdf <= 0.f) solid = o + 1;
                    else if (sdf < l.bg[o]) band = true;
                }
                continue;
            }
        }
        const float dx = x - s.cx[o], dy = y - s.cy[o], dz = z - s.cz[o];
        if (s.shape[o] == BQ_SHAPE_SPHERE) {
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float R = s.rx[o] + s.h3;
            if (d2 <= s.rx[o] * s.rx[o]) solid = o + 1;
            else if (d2 < R * R) band = true;
        } else {
            const float ax = fabsf(dx) - s.rx[o], ay = fabsf(dy) - s.ry[o], az = fabsf(dz) - s.rz[o];
            if (ax <= 0.f && ay <= 0.f && az <= 0.f) {
                solid = o + 1;
            } else {
                const float qx = fmaxf(ax, 0.f), qy = fmaxf(ay, 0.f), qz = fmaxf(az, 0.f);
                const float d2 = qx * qx + qy * qy + qz * qz;
                if (d2 > 0.f && d2 < s.h3 * s.h3) band = true;
            }
        }
    }
    return solid ? solid : (band ? -1 : 0);
}

// the solid test of obs_classify for ONE entry o, without the band: what makes a node part of a source (DESIGN.md
// section 16).  Same expressions, same operation order.
template <typename... Ls>
__device__ __forceinline__ bool obs_solid(float x, float y, float z, int o, const ObsSet &s, const Ls &...ls)
{
    static_assert(sizeof...(Ls) <= 1, "one LsSet at most");
    if constexpr (sizeof...(Ls) == 1) {
        if (s.shape[o] == BQ_SHAPE_LEVELSET) {
            const LsSet &l = (ls, ...);
            float sdf;
            return ls_sample(l, o, x, y, z, s.cx[o], s.cy[o], s.cz[o], sdf) && sdf <= 0.f;
        }
    }
    const float dx = x - s.cx[o], dy = y - s.cy[o], dz = z - s.cz[o];
    if (s.shape[o] == BQ_SHAPE_SPHERE) {
        const float d2 = dx * dx + dy * dy + dz * dz;
        return d2 <= s.rx[o] * s.rx[o];
    }
    const float ax = fabsf(dx) - s.rx[o], ay = fabsf(dy) - s.ry[o], az = fabsf(dz) - s.rz[o];
    return ax <= 0.f && ay <= 0.f && az <= 0.f;
}

// sample position of node i on an axis with stagger d (0: cell centre, 1: face): (i - d/2) h
__device__ __forceinline__ float obs_pos(int i, int d, float h) { return ((float)i - (d ? 0.5f : 0.f)) * h; }

} // namespace bq
