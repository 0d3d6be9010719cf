// bq_pose.h -- the host arithmetic of rigid obstacle poses: when a pose list is usable, which
// entries are oriented or spin, and the rotation matrix of a quaternion.  Plain C++: the obstacle operators
// (bq_obstacle.hip.h) and the host solver (host/fluid_solver.cpp) share it.
#pragma once
#include "bimocq_gpu.h"

#include <cmath>

namespace bq {

// NULL when every pose of pose[0 .. n) is usable, else what is wrong (pose == NULL: no poses, nothing to check)
static inline const char *pose_check(const bq_pose *pose, int n)
{
    if (!pose) return nullptr;
    for (int o = 0; o < n; o++) {
        const bq_pose &p = pose[o];
        if (!std::isfinite(p.qw) || !std::isfinite(p.qx) || !std::isfinite(p.qy) || !std::isfinite(p.qz) ||
            !std::isfinite(p.ox) || !std::isfinite(p.oy) || !std::isfinite(p.oz))
            return "pose with a non-finite component";
        const double w = p.qw, x = p.qx, y = p.qy, z = p.qz, s = w * w + x * x + y * y + z * z;
        if (!(s > 0.0) || !std::isfinite(s)) return "pose with a zero or non-finite quaternion";
    }
    return nullptr;
}

// an oriented entry is classified in body coordinates; a sphere ignores its orientation
static inline bool pose_oriented(const bq_boundary &b, const bq_pose &p)
{
    return b.shape != BQ_SHAPE_SPHERE && (p.qx != 0.f || p.qy != 0.f || p.qz != 0.f);
}

static inline bool pose_spins(const bq_pose &p) { return p.ox != 0.f || p.oy != 0.f || p.oz != 0.f; }

static inline bool pose_any(const bq_boundary *b, const bq_pose *pose, int n)
{
    if (!pose) return false;
    for (int o = 0; o < n; o++)
        if (pose_oriented(b[o], pose[o]) || pose_spins(pose[o])) return true;
    return false;
}

// R (row-major, body -> world) of the quaternion of p: the scale-free formula in double from the four floats, every entry
// rounded to float.  Only + - * /, one rounding each (no contraction: numpy's float64 gives the same bits), so that
// q = (1, 0, 0, 1) is exactly the quarter turn about +z and (0, 0, 0, 1) the half turn.
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static inline void pose_matrix(const bq_pose &p, float R[9])
{
    const double w = p.qw, x = p.qx, y = p.qy, z = p.qz;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double s = ((ww + xx) + yy) + zz;
    const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    R[0] = (float)(1.0 - (2.0 * (yy + zz)) / s);
    R[1] = (float)((2.0 * (xy - wz)) / s);
    R[2] = (float)((2.0 * (xz + wy)) / s);
    R[3] = (float)((2.0 * (xy + wz)) / s);
    R[4] = (float)(1.0 - (2.0 * (xx + zz)) / s);
    R[5] = (float)((2.0 * (yz - wx)) / s);
    R[6] = (float)((2.0 * (xz - wy)) / s);
    R[7] = (float)((2.0 * (yz + wx)) / s);
    R[8] = (float)(1.0 - (2.0 * (xx + yy)) / s);
}

} // namespace bq
