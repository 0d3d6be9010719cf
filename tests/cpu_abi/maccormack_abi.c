/*
 * maccormack_abi.c -- TEST-ONLY C restatement of gpu_maccormack of include/bimocq_gpu.h.
 *
 * Linked, together with oracle_abi.c, the obstacle, level-set, PCG and source restatements and the oracle, into
 * tests/_build/libbimocq_host_cpu_maccormack.so (tests/build_cpu_maccormack.py): the CPU stand-in on which the host
 * solver's fused MacCormack body runs without a GPU, and against which the GPU tests compare the HIP kernel value for
 * value.  Written from the contract: the literal composition of the header's definition on the oracle's operators, with
 * buffers of its own for the two intermediate fields.  The oracle's operators carry the z-slab context of the stand-in
 * (oracle_abi.c: fl_set_slab -> orc_set_slab), so this restatement honours it as they do.
 * maccormack_abi_calls(reset): how many calls have been made (and back to 0 when reset != 0) -- a test's proof that the
 * host solver took the fused body.
 */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/bimocq_gpu.h"
#include "../../oracle/bimocq_oracle.h"

void fl_report_error(int code, const char *text);

static long g_calls = 0;

long maccormack_abi_calls(int reset)
{
    long c = g_calls;
    if (reset) g_calls = 0;
    return c;
}

void gpu_maccormack(float *out, const float *f1, const float *f_adv, const float *f_lim, float *u, float *v, float *w,
                    int dim_x, int dim_y, int dim_z, float h, int ni, int nj, int nk, float cfldt, float dt, float dt_clamp)
{
    if (!out || !f1 || !f_adv || !f_lim || !u || !v || !w || ni < 1 || nj < 1 || nk < 1) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_maccormack: null pointer or non-positive dims");
        return;
    }
    if (out == f1 || out == f_adv || out == f_lim || out == u || out == v || out == w) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_maccormack: out aliases an input");
        return;
    }
    if (!(cfldt > 0.f || dt == 0.f)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_maccormack: cfldt <= 0 with dt != 0");
        return;
    }
    if (dim_x < 0 || dim_x > 1 || dim_y < 0 || dim_y > 1 || dim_z < 0 || dim_z > 1 || dim_x + dim_y + dim_z > 1) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "gpu_maccormack: bad stagger triple");
        return;
    }
    const size_t n = (size_t)(ni + dim_x) * (size_t)(nj + dim_y) * (size_t)(nk + dim_z);
    float *back = (float *)calloc(n, sizeof(float));
    if (!back) {
        fl_report_error(FL_ERR_HIP, "gpu_maccormack: out of host memory");
        return;
    }
    g_calls++;
    orc_semilag(back, f1, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt);
    memcpy(out, f1, n * sizeof(float));
    orc_add(out, back, -0.5f, (int)n);
    orc_add(out, f_adv, 0.5f, (int)n);
    orc_clamp_extrema(f_lim, out, u, v, w, ni + dim_x, nj + dim_y, nk + dim_z, dim_x, dim_y, dim_z,
                      0.5f * dim_x, 0.5f * dim_y, 0.5f * dim_z, h, dt_clamp);
    free(back);
}
