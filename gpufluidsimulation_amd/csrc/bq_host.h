// bq_host.h -- host-side state shared by the C-ABI translation units (runtime, launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include "../../include/bimocq_gpu.h"

namespace bq {

struct Runtime {
    bool        ready = false;
    int         device = -1;
    hipStream_t compute = nullptr;      // every operator launches here
    hipStream_t halo = nullptr;         // ghost-plane exchange (multi-GPU), overlapped with interior work
    hipStream_t copy = nullptr;         // device -> host downloads of the dump path, overlapped with the next step
    // fl_aux_*: a second compute stream for an operator that is independent of the ones that follow it (the forward-map
    // update beside the backward one): while a section is open `compute` IS the auxiliary stream
    hipStream_t aux = nullptr, compute_main = nullptr;
    hipEvent_t  aux_fork = nullptr, aux_done = nullptr;
    bool        aux_pending = false;
    int         err = FL_OK;
    char        err_text[256] = {0};
    int         opt_residual_stride = 0;
    int         opt_skip_unit_blend = 1;
    int         opt_jacobi_variant = 0;
    int         opt_profile_jacobi = 0;
    int         opt_structured_maps = 1;
    int         opt_jacobi_fuse = 1;        // 0 never, 1 inside gpu_projection_jacobi, 2 also in gpu_jacobi_sweeps
    int         opt_jacobi_kchunk2 = 0;     // FL_OPT_JACOBI_KCHUNK2 (option table in include/bimocq_gpu.h)
    int         opt_jacobi_kchunk = 0;      // 0 = auto
    int         opt_fused_housekeeping = 0; // FL_OPT_FUSED_HOUSEKEEPING bit mask
    int         opt_fast_lerp = 0;          // gather kernels: one fp32 fma per lerp instead of the double-evaluated one
    int         opt_map_quarter_fp32 = 0;   // FL_OPT_MAP_QUARTER_FP32: the caller vouches for the maps (gpu_maps_quarter_safe)
    // map-value guard (fl_map_guard_*): gpu_solve_backwardDMC ORs word 0, gpu_solve_forward word 1 of this device array
    // when a map value they store fails tile_value_ok; nullptr while the guard is off
    int        *map_guard = nullptr;
    bool        map_guard_on = false;
    int         opt_mgcg_graph = 1;         // replay the multigrid V-cycle from a captured hipGraph
    int         opt_mgcg_tile = 1;          // FL_OPT_MGCG_TILE: LDS tile smoother on the coarse levels of the V-cycle
    int         opt_profile_comm = 0;       // FL_OPT_PROFILE_COMM: time the compute stream's waits on the halo stream
    int         opt_mgcg_bottom = 1;        // FL_OPT_MGCG_BOTTOM: the two coarsest V-cycle levels in one launch
    int         opt_mgcg_fuse = -1;         // FL_OPT_MGCG_FUSE: level-0 vector updates inside the stencil passes (bq_mgcg_fused.hip.inc); -1 = not vouched for: off
    int         opt_comm_check = 0;         // FL_OPT_COMM_CHECK: ledger of communicator calls (bq_halo.hip)
    int         opt_field_window = -1;      // FL_OPT_FIELD_WINDOW: -1 auto (on with FL_OPT_FAST_LERP), 0 off, 1 on, k > 1 planes per block
    int         opt_reserve_cus = 0;        // FL_OPT_RESERVE_CUS: CUs the compute stream leaves to the halo stream's RCCL kernels
    int         device_cus = 0;             // CUs of the device (hipDeviceProp_t::multiProcessorCount), set by fl_init
    int         num_cus = 256;              // CUs the compute stream may use (device CUs - opt_reserve_cus)
    int         opt_diag_kchunk = 0;        // FL_OPT_DIAG_KCHUNK: planes per block of gpu_flow_stats' march (0 = its rule, -1 = one thread per cell)
    int         opt_render_kchunk = 0;      // FL_OPT_RENDER_KCHUNK: cells per chunk of gpu_render_density's marches along y and z (0 = its rule, -1 = one march per ray)
    int         opt_confine_kchunk = 0;     // FL_OPT_CONFINE_KCHUNK: planes per block of gpu_vorticity_confinement's march (0 = its rule, -1 = one thread per output node)
    int         opt_jacobi_rows = 0;        // FL_OPT_JACOBI_ROWS: one code per kernel choice (option table in include/bimocq_gpu.h)
    // z-slab context (fl_set_slab): local plane k is global plane k + slab_koff of slab_nkg planes;
    // this rank owns global planes [slab_own0, slab_own1) (reductions count only those)
    // plane window (fl_set_plane_window): the map operators that honour it produce the local planes [win_k0, win_k1) only
    bool        win_on = false;
    int         win_k0 = 0, win_k1 = 0;
    bool        slab_on = false;
    int         slab_koff = 0, slab_nkg = 0, slab_own0 = 0, slab_own1 = 0, slab_nkl = 0;  // nkl: local cell planes
    // persistent workspace (replaces the cudaMalloc/cudaFree pair inside the reference's
    // gpu_projection_jacobi, GPU_kernel.cu:1847-1850,1893-1894)
    void  *scratch = nullptr;           // device: reduction partials
    size_t scratch_bytes = 0;
    void  *pinned = nullptr;            // host-pinned mirror for blocking reductions
    size_t pinned_bytes = 0;
    // state the other translation units keep PER CONTEXT (fl_context_*): the communicator and its event ring (bq_halo.hip),
    // the sweep-profile spans (bq_project.hip), the cached V-cycle graphs (bq_mgcg.hip).  Allocated on first
    // use, released by fl_shutdown through the *_release hooks below.
    void  *halo_state = nullptr, *project_state = nullptr, *mgcg_state = nullptr;
    // tables of the structured map look-up on spacings that are not a power of two (bq_advect.hip: map_tabs): device
    // arrays frac / rel, what they were built for, and which (axis, stagger) pairs conform (bit 2 * axis + S)
    float *map_tab_dev = nullptr;
    float  map_tab_h = 0.f;
    int    map_tab_dims[3] = {0, 0, 0}, map_tab_stride = 0, map_tab_ok = 0;
    // FL_OPT_SKIP_EMPTY_BRICKS (bq_advect.hip: brick_flags): one flag per 8^3 brick of the arrays the last flag pass read, and a
    // header -- word 0: number of the last pass that found an empty brick; bytes 8..55: three pairs of 64-bit block counters (option value 2);
    // bytes 64..79: the pair of wave counters of FL_OPT_SKIP_EMPTY_TAPS.  Behind the brick flags and the block list, sparse_flags
    // holds that option's CELL flags: one byte per brick of base nodes, (n >> 3) + 1 bricks per axis, 0 only if every word a
    // cell based there can deliver to corners() is zero (bq_sparse.hip.h: cell_flags_kernel).
    unsigned char *sparse_flags = nullptr;
    size_t sparse_cap = 0;
    int   *sparse_hdr = nullptr;
    int    sparse_epoch = 0;            // passes issued so far
    int    opt_skip_empty_bricks = 1;   // 0 off, 1 on (advection, error stage), 2 = 1 and counting, 3 = 1 plus the accumulation, 4 = 3 and counting
    // FL_OPT_SKIP_EMPTY_TAPS: with opt_skip_empty_bricks 1 or 2 the unstaggered accumulation runs as a launch that tests the
    // taps it has computed against the cell flags, wave by wave, followed by the unchanged kernel on an empty block list, which
    // does the work where the flag pass found no empty brick (no classifying launch: the backward map's zeroed border makes the
    // tile range of half the blocks useless, while the nine taps of a border lane land at nine definite, usually empty points).
    // A skipped wave may read no corner word of any tap -- the flags vouch that all of them are 0x00000000 -- and its stores are
    // the full path's statements with +0.0f for every gather result.
    int    opt_skip_empty_taps = 1;
    int    nonfinite_seen = 0;          // sticky: a gpu_max_abs3 met a NaN or an Inf (fl_nonfinite_seen)
    const char *map_kernel_name[2] = { "", "" };    // the DMC / forward instance launched last (fl_map_kernel_name)
    int    map_kernels_seen = 0;        // instances launched since the last reset, as bits (fl_map_kernels_seen)
    long long   mg_fused_launches = 0;  // fl_mg_fused_launches
    long long   mg_residual_launches = 0;   // fl_mg_residual_launches
    const char *mg_smooth_kernel = ""; // the fused kernel the last fp64 smoothing call launched first (fl_mg_smooth_kernel_name)
};

Runtime &rt();
// slab context of the library: (koff, nkg); single GPU: (0, nk)
inline void slab_ctx(int nk, int &koff, int &nkg)
{
    const Runtime &r = rt();
    koff = r.slab_on ? r.slab_koff : 0;
    nkg = r.slab_on ? r.slab_nkg : nk;
}
void latch(int code, const char *what, const char *detail);
bool ensure_ready(const char *op);      // lazily fl_init(current device); false -> latched
void *scratch(size_t bytes);            // device scratch of at least `bytes` (grows, never shrinks)
void *pinned(size_t bytes);
// bq_halo.hip: in-stream all-reduce of device values across slab ranks (no-op on one rank)
bool comm_allreduce(void *dev, size_t count, bool is_double, bool is_max, hipStream_t st);
int  comm_ranks();
void mgcg_release_graph();              // bq_mgcg.hip: drop the cached V-cycle graphs of the current context (fl_free / fl_shutdown)
void mgcg_release_state(Runtime &r);    // ... and free the per-context state itself (fl_shutdown)
// bq_mgcg.hip: the coarse machinery of the V-cycle for the PCG projection (bq_pcg.hip)
void mgcg_restrict(const double *fine, double *coarse, const SCoarseLevelInfo &F, const SCoarseLevelInfo &Cl);
void mgcg_prolong(double *x, const double *coarse, const SCoarseLevelInfo &F, const SCoarseLevelInfo &Cl);
void mgcg_pcg_coarse(const SCoarseLevelInfo *L, int levelnum, double *temp, int down, int up, int bottom);
void halo_release_state(Runtime &r);    // bq_halo.hip
void halo_abandon_comm(Runtime &r);     // bq_halo.hip: forget the communicator without destroying it (process exit)
void project_release_state(Runtime &r); // bq_project.hip
// bq_project.hip: FL_OPT_JACOBI_VARIANT / _ROWS / _KCHUNK / _KCHUNK2 / _FUSE of the current context, decoded (bq_jacobi_plan.h); the
// launchers call it once per entry-point call and read the named fields, never the raw integers
namespace plan { struct JacobiTuning; }
plan::JacobiTuning jacobi_tuning();
// bq_project.hip: FL_OPT_PROFILE_JACOBI spans -- an event pair around a loop of sweep launches on the compute
// stream, summed by fl_jacobi_profile().  profile_begin returns false when profiling is off.
struct ProfileSpan { hipEvent_t a = nullptr, b = nullptr; };
bool profile_begin(ProfileSpan &sp);
void profile_end(ProfileSpan &sp, long long launches, long long sweeps);
// bq_project.hip: the loop of the gpu_jacobi_sweeps* entry points -- `sweeps` sweeps ping-ponging from p to p_temp.  Each stage in turn
// launches its `sweeps` per launch in -> out while that many are left and it returns true (false: not applicable, nothing launched);
// `single` takes the rest one by one (false: a failed launch check ends the loop).  Returns 0: the newest iterate is in p, 1: in p_temp.
using SweepLaunch = std::function<bool(const float *in, float *out)>;
struct SweepStage { int sweeps; bool on; SweepLaunch launch; };
int run_sweeps(float *p, float *p_temp, int sweeps, std::initializer_list<SweepStage> stages, const SweepLaunch &single);

// one thread per element: blocks of 64 (x) x 4 (y), planes along grid.z
static const dim3 kBlock(64, 4, 1);
inline dim3 grid_for(int nbi, int nbj, int nbk) { return dim3((nbi + 63) / 64, (nbj + 3) / 4, nbk); }
// grid.z takes at most 65535 planes and the w component has nk + 1.  grid.y has no rule here: the runtime takes more than
// 65535 blocks on it, so nj is bounded by the plane limit where a launcher has one and not at all where this is its only
// check (include/bimocq_gpu.h, "Limits").  False: latched under the text every launcher uses for this limit.
inline bool planes_ok(int nk, const char *op)
{
    if (nk + 1 <= 65535) return true;
    latch(FL_ERR_BAD_ARGUMENT, op, "nk too large for grid.z");
    return false;
}
// the size rules of the obstacle and source operators (size_t indices: 4 GiB, no plane limit), each refusal under its own text
inline bool obstacle_dims_ok(int ni, int nj, int nk, const char *op)
{
    if (ni < 3 || nj < 3 || nk < 3) { latch(FL_ERR_BAD_ARGUMENT, op, "dims below 3"); return false; }
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 4294967296.0) {
        latch(FL_ERR_BAD_ARGUMENT, op, "field larger than 4 GiB");
        return false;
    }
    return planes_ok(nk, op);
}
// true when every pointer is 16-byte aligned (float4 / double2 accesses)
template <typename... P>
inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15u) == 0; }

inline bool hip_ok(hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    latch(FL_ERR_HIP, what, hipGetErrorString(e));
    return false;
}

} // namespace bq

#define BQ_HIP(call) ::bq::hip_ok((call), #call)
#define BQ_LAUNCH_CHECK(name) ::bq::hip_ok(hipGetLastError(), name)

// argument validation shared by the launchers: positive dims, non-null pointers
#define BQ_REQUIRE(cond, op)                                                        \
    do {                                                                            \
        if (!(cond)) { ::bq::latch(FL_ERR_BAD_ARGUMENT, op, #cond); return; }       \
    } while (0)
