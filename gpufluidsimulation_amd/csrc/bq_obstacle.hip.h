// bq_obstacle.hip.h -- the obstacle list as a kernel argument and the one classification every obstacle kernel uses
// (squared distances, no sqrt, so that flags are the same bits on the CPU stand-in and the GPU).
#pragma once
#include <hip/hip_runtime.h>
#include "bimocq_gpu.h"

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

// o + 1 when obstacle o is the last one covering (x, y, z); -1 when the point lies in the band of some obstacle and
// inside none; 0 otherwise
__device__ __forceinline__ int obs_classify(const ObsSet &s, float x, float y, float z)
{
    int solid = 0;
    bool band = false;
    for (int o = 0; o < s.n; o++) {
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

// sample position of node i on an axis with stagger d (0: cell centre, 1: face): (i - d/2) h
__device__ __forceinline__ float obs_pos(int i, int d, float h) { return ((float)i - (d ? 0.5f : 0.f)) * h; }

} // namespace bq
