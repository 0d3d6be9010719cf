// bq_levelset.h -- when a level-set descriptor is usable ("Level sets").  Plain C++: the obstacle
// operators (bq_obstacle.hip.h) and the host solver's setBoundary (host/fluid_solver.cpp) both refuse with it.
#pragma once
#include "bimocq_gpu.h"

#include <climits>
#include <cmath>

namespace bq {

// NULL when every level-set entry of b[0 .. n) has a usable descriptor in ls[], else what is wrong
static inline const char *ls_check(const bq_boundary *b, const bq_levelset *ls, int n)
{
    for (int o = 0; o < n; o++) {
        if (b[o].shape != BQ_SHAPE_LEVELSET) continue;
        if (!ls) return "level-set entry without descriptors";
        const bq_levelset &l = ls[o];
        if (!l.phi) return "level set with a null grid";
        if (l.nx < 2 || l.ny < 2 || l.nz < 2 || (double)l.nx * (double)l.ny * (double)l.nz >= 2147483648.0)
            return "level-set dimensions below 2 or 2^31 nodes and more";
        if ((long long)l.i0 - 1 < INT_MIN || (long long)l.j0 - 1 < INT_MIN || (long long)l.k0 - 1 < INT_MIN ||
            (long long)l.i0 + l.nx > INT_MAX || (long long)l.j0 + l.ny > INT_MAX || (long long)l.k0 + l.nz > INT_MAX)
            return "level-set index range beyond int";
        if (!(l.voxel > 0.f) || !(l.background > 0.f) || !std::isfinite(l.voxel) || !std::isfinite(l.background))
            return "level-set voxel or background not finite and positive";
    }
    return nullptr;
}

} // namespace bq
