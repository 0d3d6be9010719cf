// bq_gather_op.hip.h -- what each of the three nine-point gather operators IS (GPU_kernel.cu:312-499): index window,
// clamp box, tap weight, lerp form, the housekeeping fused into it and the value a node gets.  The one-plane kernels and
// the wall fix-up of bq_advect.hip, the marching kernel of bq_gather_march.hip.h and the host launcher read it from here;
// a change to an operator is a change to this file.
#pragma once
#include "bq_device.hip.h"

namespace bq {
inline namespace BQ_VARIANT {

enum { kOpAdvect = 0, kOpCumulate = 1, kOpCompensate = 2 };

// NF fields that live on the same nodes share one map look-up (density + temperature; the two velocity-change fields
// accumulated back to back).  Results per field are what NF single launches in the same order produce.
//                 src (sampled)      out               aux        coeff
//   advect        init               field             -          -
//   cumulate      src                dst (added to)    -          coeff
//   compensate    src                err               init       -
template <int NF> struct GatherArgs { const float *src[NF]; float *out[NF]; float *aux[NF]; float coeff[NF]; };

template <int KIND> struct GatherOp {
    // the operator works on nodes with margin < index < n - margin - 1 (GPU_kernel.cu:353, :414, :476)
    static constexpr int margin = KIND == kOpAdvect ? 2 : 1;
    // advect clamps its positions to >= h: every lerp may take its one-fma form (lerp_w<true>).  The others may where a
    // whole wave happens to have all positions >= h (wave_all_ge)
    static constexpr bool always_ge1 = KIND == kOpAdvect;
    static constexpr bool has_housekeeping = KIND != kOpCumulate;
    // whose counters of fl_sparse_stats_kind a launch feeds, and the name a failed launch is reported under
    static constexpr int counter_slot = KIND == kOpAdvect ? 0 : KIND == kOpCompensate ? 1 : 2;
    static constexpr const char *kernel_name = KIND == kOpAdvect ? "advect_kernel" : KIND == kOpCumulate ? "cumulate_kernel" : "compensate_kernel";

    // clamp box of the mapped positions, in GLOBAL coordinates (z over the nkg planes of the whole grid)
    static __device__ __forceinline__ f3 lo(float h) { return KIND == kOpAdvect ? mk3(h, h, h) : mk3(0.f, 0.f, 0.f); }
    static __device__ __forceinline__ f3 hi(float h, int ni, int nj, int nkg)
    {
        return KIND == kOpAdvect ? mk3(h * (float)ni - h, h * (float)nj - h, h * (float)nkg - h)
                                 : mk3(h * (float)ni, h * (float)nj, h * (float)nkg);
    }
    // weight of a tap: (0.125f * coeff) * sample is the reference's left-to-right product; point mode has the one tap
    static __device__ __forceinline__ float weight(bool pt, float coeff)
    {
        return KIND == kOpCumulate ? (pt ? 1.0f : 0.125f) * coeff : (pt ? 1.0f : 0.125f);
    }
    // FL_OPT_FUSED_HOUSEKEEPING at node id0 + off of the buffer (offset inside its plane + offset of the plane: handed over
    // apart so that a march along z keeps base + id0 out of its loop), inside the index window (active) or not.
    // advect, bit 1: out = the zero the caller's clear would have left outside the window.
    // compensate, bit 2: init <- the uncompensated field on EVERY node (stage 2 of gpu_compensate_*, GPU_kernel.cu:656-658).
    // A thread reads init only at its own node, before it stores there, and no thread reads init anywhere else or
    // writes src, so doing it here is race-free.  Bit 1: err = 0 outside the window.  init_own: init as the caller left it.
    template <int NF>
    static __device__ __forceinline__ void housekeeping(const GatherArgs<NF> &a, size_t id0, size_t off, int fused, bool active, float (&init_own)[NF])
    {
        if constexpr (KIND == kOpAdvect) {
            if ((fused & 1) && !active) {
#pragma unroll
                for (int f = 0; f < NF; f++) a.out[f][id0 + off] = 0.f;
            }
        } else if constexpr (KIND == kOpCompensate) {
#pragma unroll
            for (int f = 0; f < NF; f++) {
                init_own[f] = a.aux[f][id0 + off];
                if (fused & 2) a.aux[f][id0 + off] = a.src[f][id0 + off];
                if ((fused & 1) && !active) a.out[f][id0 + off] = 0.f;
            }
        }
    }
    // what a node gets from sum = sum of w * tap and value = the centre sample (init_own is read by compensate only)
    static __device__ __forceinline__ float result(float sum, float value, float coeff, const float &init_own)
    {
        if constexpr (KIND == kOpAdvect) return 0.5f * sum + 0.5f * value;
        else if constexpr (KIND == kOpCumulate) return (float)(0.5 * (double)sum + 0.5 * (double)(coeff * value));
        else return (float)(0.5 * (double)sum + 0.5 * (double)value) - init_own;
    }
    // ... and its store.  cumulate adds to the destination; out[0] == out[1] is allowed and applied in order: the second
    // field starts from what the first stored.
    template <int NF>
    static __device__ __forceinline__ void store(const GatherArgs<NF> &a, int f, size_t id, float r)
    {
        if constexpr (KIND == kOpCumulate) a.out[f][id] += r;
        else a.out[f][id] = r;
    }
};

} // inline namespace BQ_VARIANT
} // namespace bq
