/*
 * bimocq_gpu.h -- C-ABI of the MI355X (gfx950) bimocq3D hot path.
 *
 * Drop-in boundary: the 22 `extern "C" gpu_*` operators below carry exactly the
 * signatures of the reference's CUDA launchers (reference: src/bimocq3D/GPU_Advection.h:26-108,
 * implemented in src/bimocq3D/GPU_kernel.cu), so the reference's gpuMapper / MapperBaseGPU /
 * BimocqGPUSolver link against libbimocq_hip.so unchanged.  All pointers are DEVICE pointers
 * (hipMalloc / fl_malloc); fields are dense fp32, x fastest: index = i + nx*j + nx*ny*k.
 * Staggered sizes: u (ni+1,nj,nk), v (ni,nj+1,nk), w (ni,nj,nk+1); scalars and maps (ni,nj,nk).
 *
 * The fl_* group replaces the raw CUDA runtime calls gpuMapper makes
 * (GPU_Advection.h:214-326: findCudaDevice, cudaMalloc/Memset/Memcpy, cudaEvent*).
 * The last group is additive (no reference counterpart).
 *
 * Error convention: the reference's operators return void and check nothing
 * (SURVEY 8b).  Kept: every operator returns void, is asynchronous on the library's
 * compute stream, and latches the first failure (bad argument, HIP error, unsupported
 * operator) for fl_last_error().
 */
#ifndef BIMOCQ_GPU_H
#define BIMOCQ_GPU_H

#include <stddef.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* GPU_Advection.h:14-24 */
#define LEVEL_COUNT 6
struct SCoarseLevelInfo {
    int ni, nj, nk;
    int number;
    double alpha;
    double beta;
    double *b;
    double *x;
    double *r;
};
#ifndef __cplusplus
typedef struct SCoarseLevelInfo SCoarseLevelInfo;
#endif

/* ------------------------------------------------------------------------------------------
 * 1. Reference operators (same names, argument order and meaning)
 * ---------------------------------------------------------------------------------------- */

/* GPU_Advection.h:26-28 / GPU_kernel.cu:567-574.  In-place RK3 trace of the forward map,
 * sub-stepped by cfldt, interior nodes 2..n-3. */
void gpu_solve_forward(float *u, float *v, float *w,
                       float *x_fwd, float *y_fwd, float *z_fwd,
                       float h, int ni, int nj, int nk, float cfldt, float dt);

/* GPU_Advection.h:30-33 / GPU_kernel.cu:576-584.  One DMC backward sub-step in -> out.
 * out must not alias in; nodes outside 2..n-3 of out are left untouched. */
void gpu_solve_backwardDMC(float *u, float *v, float *w,
                           float *x_in, float *y_in, float *z_in,
                           float *x_out, float *y_out, float *z_out,
                           float h, int ni, int nj, int nk, float substep);

/* GPU_Advection.h:35-38 / GPU_kernel.cu:586-598.  Caller zeroes u,v,w first
 * (GPU_Advection.h:477-479): only the window 3+dim..nbuf-4 is written. */
void gpu_advect_velocity(float *u, float *v, float *w,
                         float *u_init, float *v_init, float *w_init,
                         float *backward_x, float *backward_y, float *backward_z,
                         float h, int ni, int nj, int nk, bool is_point);

/* GPU_Advection.h:40-44 / GPU_kernel.cu:600-618.  u = u*b + (1-b)*prev(psi_prev(psi_back)). */
void gpu_advect_vel_double(float *u, float *v, float *w,
                           float *utemp, float *vtemp, float *wtemp,
                           float *backward_x, float *backward_y, float *backward_z,
                           float *backward_xprev, float *backward_yprev, float *backward_zprev,
                           float h, int ni, int nj, int nk, bool is_point, float blend_coeff);

/* GPU_Advection.h:46-48 / GPU_kernel.cu:620-627 */
void gpu_advect_field(float *field, float *field_init,
                      float *backward_x, float *backward_y, float *backward_z,
                      float h, int ni, int nj, int nk, bool is_point);

/* GPU_Advection.h:50-53 / GPU_kernel.cu:629-638 */
void gpu_advect_field_double(float *field, float *field_init,
                             float *backward_x, float *backward_y, float *backward_z,
                             float *backward_xprev, float *backward_yprev, float *backward_zprev,
                             float h, int ni, int nj, int nk, bool is_point, float blend_coeff);

/* GPU_Advection.h:55-58 / GPU_kernel.cu:684-696.  d*_init += coeff * blend9(change(psi_fwd(x))). */
void gpu_accumulate_velocity(float *u_change, float *v_change, float *w_change,
                             float *du_init, float *dv_init, float *dw_init,
                             float *forward_x, float *forward_y, float *forward_z,
                             float h, int ni, int nj, int nk, bool is_point, float coeff);

/* GPU_Advection.h:60-62 / GPU_kernel.cu:698-705 */
void gpu_accumulate_field(float *field_change, float *dfield_init,
                          float *forward_x, float *forward_y, float *forward_z,
                          float h, int ni, int nj, int nk, bool is_point, float coeff);

/* GPU_Advection.h:64-67 / GPU_kernel.cu:707-716.  du (ni*nj*nk floats) receives the squared
 * round-trip distortion on nodes 2..n-3; caller zeroes it first (GPU_Advection.h:583). */
void gpu_estimate_distortion(float *du,
                             float *x_init, float *y_init, float *z_init,
                             float *x_fwd, float *y_fwd, float *z_fwd,
                             float h, int ni, int nj, int nk);

/* GPU_Advection.h:69 / GPU_kernel.cu:729-734.  field1 += coeff*field2 over exactly `number`
 * elements (the reference's grid overruns to the next multiple of 256; not replicated). */
void gpu_add(float *field1, float *field2, float coeff, int number);

/* GPU_Advection.h:71-76 / GPU_kernel.cu:640-666.  u,v,w: field in/out.  du,dv,dw: `init`, read,
 * then OVERWRITTEN with the uncompensated field.  u_src..: scratch, zeroed by the caller
 * (GPU_Advection.h:499-501). */
void gpu_compensate_velocity(float *u, float *v, float *w,
                             float *du, float *dv, float *dw,
                             float *u_src, float *v_src, float *w_src,
                             float *forward_x, float *forward_y, float *forward_z,
                             float *backward_x, float *backward_y, float *backward_z,
                             float h, int ni, int nj, int nk, bool is_point);

/* GPU_Advection.h:78-81 / GPU_kernel.cu:668-682.  All three buffers hold ni*nj*nk floats
 * (the reference's (ni+1)*nj*nk copy size is an overrun, not replicated). */
void gpu_compensate_field(float *u, float *du, float *u_src,
                          float *forward_x, float *forward_y, float *forward_z,
                          float *backward_x, float *backward_y, float *backward_z,
                          float h, int ni, int nj, int nk, bool is_point);

/* GPU_Advection.h:83-86 / GPU_kernel.cu:718-727 */
void gpu_semilag(float *field, float *field_src,
                 float *u, float *v, float *w,
                 int dim_x, int dim_y, int dim_z,
                 float h, int ni, int nj, int nk, float cfldt, float dt);

/* GPU_Advection.h:88-90 / GPU_kernel.cu:782-802.  ni,nj,nk are CELL dims. */
void gpu_emit_smoke(float *u, float *v, float *w, float *rho, float *T,
                    float h, int ni, int nj, int nk,
                    float centerX, float centerY, float centerZ, float radius,
                    float density, float temperature, float emiter);

/* GPU_Advection.h:92-93 / GPU_kernel.cu:825-832.  field = v component; ni,nj,nk CELL dims.
 * Implements the intended indexing (the reference mis-indexes rho/T for k>0):
 * v(i,j,k) += 0.5*dt*(beta*(T(j)+T(j-1)) - alpha*(rho(j)+rho(j-1))), 1 <= j <= nj-1. */
void gpu_add_buoyancy(float *field, float *density, float *temperature,
                      int ni, int nj, int nk, float alpha, float beta, float dt);

/* GPU_Advection.h:95 / GPU_kernel.cu:855-876.  ni,nj,nk are BUFFER dims.  fieldTemp0 receives a
 * copy of field and is the first sweep's input; on return field holds iterate iter-1. */
void gpu_diffuse_field(float *field, float *fieldTemp0, float *filedTemp1,
                       int ni, int nj, int nk, int iter, float coef);

/* GPU_Advection.h:97 / GPU_kernel.cu:885-890.  out = field1 + coeff*field2. */
void gpu_add_field(float *out, float *field1, float *field2, float coeff, int number);

/* GPU_Advection.h:99 / GPU_kernel.cu:1839-1895.  Caller zeroes div, p, p_temp
 * (GPU_Advection.h:604-606).  On return u,v,w are projected with iterate iter-1, which is
 * also what p holds (the reference's off-by-one, SURVEY Q1, kept).  debugParam may be NULL;
 * otherwise it needs >= 2000+iter floats and receives, for it = 0..iter-1,
 * debugParam[it] = sum r^2 and debugParam[2000+it] = max|r| of iterate `it`
 * (exact norms; the reference's buggy reductions are re-specified),
 * evaluated every fl_set_option(FL_OPT_RESIDUAL_STRIDE) iterates (0 = never).
 * A caller that does NOT clear p / p_temp (warm start) gets the reference's values too: sweeps ping-pong, odd
 * iterates carry p_temp's boundary shell, iter == 0 copies p_temp over p (:1876-1879).  Two sweeps share a launch only
 * where that cannot change a value: FL_OPT_JACOBI_FUSE = 1 (default) compares the two boundary shells first (one small
 * kernel and a 4-byte read-back per call), 2 skips the check on the caller's word, 0 never fuses.  p_temp is scratch:
 * its contents on return differ from the reference's (which performs one sweep more and discards it). */
void gpu_projection_jacobi(float *u, float *v, float *w, float *div, float *p, float *p_temp,
                           float *debugParam, int ni, int nj, int nk, int iter,
                           float halfrdx, float alpha, float beta);

/* GPU_Advection.h:101 / GPU_kernel.cu:892-950 -- MacCormack limiter of the reflection scheme, CORRECTED
 * (SURVEY 8f N3).  The reference kernel adds the stagger offset with the wrong sign, uses the departure
 * point's world coordinates as grid indices (:913-915) and tests/overwrites fieldTemp there from every
 * thread, so its output is undefined; this entry does what it evidently means:
 *   node x = (i - o) h, o = (ox, oy, oz) (0.5 along the staggered axis); x_d = x - dt u(x - dt/2 u(x)),
 *   clamped to [h, (n-1)h]; if fieldTemp at this node lies outside the min/max of the 8 values of `field`
 *   around x_d, it becomes the trilinear value of `field` at x_d.
 * ni, nj, nk: BUFFER dims (cells + dim).  field is read only; fieldTemp must not alias it. */
void gpu_clamp_extrema(float *field, float *fieldTemp, float *u, float *v, float *w,
                       int ni, int nj, int nk, int dimx, int dimy, int dimz,
                       float ox, float oy, float oz, float h, float dt);

/* (ours) The MacCormack correction and its limiter in one launch: what the reflection scheme issues after its first
 * semi-Lagrangian pass (BimocqGPUSolver.cpp:240-262), for one field.  `out` receives, value for value, what
 *     back = 0;  gpu_semilag(back, f1, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt);
 *     out = f1;  gpu_add(out, back, -0.5f, n);  gpu_add(out, f_adv, 0.5f, n);
 *     gpu_clamp_extrema(f_lim, out, u, v, w, ni + dim_x, nj + dim_y, nk + dim_z, dim_x, dim_y, dim_z,
 *                       0.5f * dim_x, 0.5f * dim_y, 0.5f * dim_z, h, dt_clamp);
 * leaves there (n = the buffer's element count): two separately rounded products and sums, back = 0 at the nodes
 * outside gpu_semilag's window.  f1: the caller's first pass, gpu_semilag(..., -dt) of f_adv into a cleared buffer;
 * f_adv: the field that was advected; f_lim: the field the limiter looks at (f_adv itself, except in the reflection
 * scheme's second half).  ni, nj, nk: CELL dims as in gpu_semilag; every buffer holds (ni + dim_x)(nj + dim_y)(nk + dim_z)
 * floats and EVERY node of `out` is written: it needs no clear.  The inputs are read only.  Honours the z-slab context.
 * FL_ERR_BAD_ARGUMENT, nothing launched: `out` aliasing f1, f_adv, f_lim, u, v or w; cfldt <= 0 with dt != 0; a stagger
 * triple other than (0,0,0), (1,0,0), (0,1,0), (0,0,1). */
void gpu_maccormack(float *out, const float *f1, const float *f_adv, const float *f_lim,
                    float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                    float h, int ni, int nj, int nk, float cfldt, float dt, float dt_clamp);

/* GPU_Advection.h:103 / GPU_kernel.cu:959-964.  field = c1*field1 + c2*field2. */
void gpu_mad(float *field, float *field1, float *field2, float coeff1, float coeff2, int number);

/* GPU_Advection.h:105 -- OUT OF SCOPE (alternative solver, compiled out in the reference,
 * BimocqGPUSolver.cpp:419).  Latches FL_ERR_UNSUPPORTED. */
void gpu_conjugate_gradient(float *u, float *v, float *w, float *div, float *p,
                            float *residual, float *dir, float *dotR,
                            int ni, int nj, int nk, int iter, float halfrdx);

/* GPU_Advection.h:107-108 / GPU_kernel.cu:1764-1815 -- fp64 multigrid-corrected CG projection (what the
 * reference's shipped binary runs, BimocqGPUSolver.cpp:443-446: iter = 50, LEVEL_COUNT levels, halfrdx 0.5).
 * `levels` is a HOST array of levelNum entries holding DEVICE pointers (level l has dims (n-1)/2 of level
 * l-1, BimocqGPUSolver.cpp:68-90); div, p, dir, residual, temp0, temp1: levels[0].number doubles each;
 * tempResult: 4096 doubles -- [2i], [2i+1], [2i+2] the CG sums of outer iteration i, [2000+i] the largest
 * positive residual before iteration i.  p is cleared here; the caller owns and zero-allocates the rest
 * (boundary entries are never written).  Single GPU only: latches FL_ERR_UNSUPPORTED on a z-slab rank. */
void gpu_multi_grid_conjugate_gradient(float *u, float *v, float *w, double *div, double *p,
                                       double *dir, double *residual, double *temp0, double *temp1,
                                       double *tempResult, struct SCoarseLevelInfo *levels,
                                       int levelNum, int iter, double halfrdx);

/* ---- Limits of the operators (part of the ABI contract; each violation latches FL_ERR_BAD_ARGUMENT under the text in quotes,
 * nothing is launched, no buffer is touched).  What the launchers enforce, family by family -- F = 4 (ni+1)(nj+1)(nk+1) bytes,
 * the bound of every buffer of the grid; P = (ni+1)(nj+1) elements, the bound of every plane:
 *
 *   family (where the check is)                                     field            plane        planes
 *   ------------------------------------------------------------------------------------------------------------------
 *   descriptor-addressed gathers (bq_advect.hip: dims_ok):          F < 2 GiB        P < 2^23     nk + 1 <= 65535
 *     gpu_solve_*, gpu_advect_*, gpu_compensate_*, gpu_accumulate_*, gpu_estimate_distortion, gpu_semilag*, gpu_maccormack,
 *     gpu_clamp_extrema (from the component's dims back to its grid's), gpu_brick_flags, gpu_maps_quarter_safe;
 *     gpu_clamp_extrema_box / _box_w (buffer_dims_ok: the same three for the ONE buffer nx x ny x nz they are given:
 *     4 nx ny nz < 2 GiB, nx ny < 2^23, nz <= 65535)
 *   gpu_flow_stats, gpu_vorticity_confinement, gpu_obstacle_loads,  F < 2 GiB        P < 2^23     nk + 1 <= 65535
 *     gpu_render_density (each its own check; dims >= 3, render: 1..65534); the tracer entry points (bq_tracers.hip)
 *   projection (bq_project.hip: dims_ok): gpu_divergence,           F < 4 GiB        --           nk + 1 <= 65535
 *     gpu_jacobi_sweep*, gpu_gradient*, gpu_residual_norms, gpu_projection_jacobi; gpu_diffuse_field / gpu_diffuse_sweeps
 *     (buffer_dims_ok: 4 ni nj nk < 4 GiB and nk <= 65535 of the one buffer they are given)
 *   obstacles and walls (bq_obstacle.hip: obs_args_ok),             F < 4 GiB        --           nk + 1 <= 65535
 *     gpu_emit_sources (bq_source.hip); dims >= 3
 *   streaming: gpu_emit_smoke, gpu_add_buoyancy, gpu_init_maps,     --               --           nk + 1 <= 65535
 *     gpu_map_travel_z (bq_host.h: planes_ok; 64-bit indices); the fp64 projection entry points (nk < 65535 per level)
 *
 *   "field larger than 2 GiB": the gather kernels address a field through a buffer resource descriptor with 32-bit byte offsets,
 *     and the offset 2 GiB is where a cell whose base index is negative is parked so that the descriptor's range check zeroes its
 *     corners.  512^3 is 0.5 GiB; BASELINE config 5 (1024 x 1024 x 512 = 2.0 GiB per field) needs >= 2 z-slab ranks --
 *     bq_solver_create / gpuMapper refuse it on one rank with FL_ERR_UNSUPPORTED and name the rank count.
 *   "plane larger than 2^23 elements" ("plane of 2^23 elements or more"): flat indices are formed with 24-bit multiplies.
 *   "nk too large for grid.z": planes are launched along grid.z, and the w component has nk + 1 of them.  An entry point that
 *     takes a component's own dims accepts that buffer: 65535 planes of w on a grid of nk = 65534.
 *   nj has no limit of its own: where a family has the plane limit, that bounds it; in the rows marked "--" under "plane"
 *     only the field size does (projection, obstacles, sources), and in the streaming row nothing does.  Rows go along grid.y
 *     four to a block, so a grid of few columns puts more than 65535 blocks there; the HIP runtime on gfx950 takes such a launch,
 *     and at grid.y = 65540 and 65541 (nj = 262160, the v component) the gather, projection, streaming, obstacle, wall and fp64
 *     operators, gpu_flow_stats and gpu_emit_sources (a source box along the whole grid) equal their references bit for bit
 *     (tests/test_gpu_needle_grids.py).  Two operators keep a rule of their own, "nj too large for grid.y" when
 *     (nj + 4) / 4 > 65535: gpu_vorticity_confinement and gpu_obstacle_loads, whose marching kernels tile nj + 1 rows and have
 *     not been run beyond it.  gpu_render_density takes no dimension above 65534 ("dims outside 1..65534"): a ray's optical
 *     depth, at most 32 * 2^32 per cell, must stay an integer below 2^53.
 *   The entry points that take ONE buffer's dims (buffer_dims_ok, both files) bound that buffer, not the grid around it: the
 *     u, v and w buffers of a grid are each smaller than F, so a buffer passes whenever its grid would, and a buffer just below
 *     2 (4) GiB also passes whose grid, one node larger per axis, would not.  That is deliberate: these kernels index the one
 *     buffer they are given (with 64-bit indices), and the w buffer of the tallest grid, 65535 planes, must pass.
 *   "dims below 3": the obstacle, wall and source operators (bq_host.h: obstacle_dims_ok), gpu_flow_stats,
 *     gpu_vorticity_confinement and gpu_obstacle_loads need three cells per axis.
 *   A field between 2 and 4 GiB is accepted by the projection, obstacle and source families and covered by no test: the
 *     oracle needs minutes for one.  Everything a test covers lies below 2 GiB.
 *   The fused Jacobi kernels take rows of 32..1024 floats with ni % 4 == 0 and 16-byte aligned pointers; any other row runs
 *     the one-sweep kernels (same values).
 *
 * ---- Alignment (part of the ABI contract; the table per family is in DESIGN.md section 2).  The caller owns every buffer and
 * may carve u, v, w, p, ... out of one pool: ELEMENT-SIZE ALIGNMENT IS ENOUGH FOR EVERY ARRAY -- 4 bytes for float (and the
 * tracers' unsigned ids), 8 for double, 1 for the flag arrays solid / solidw / rows.  The values are those on 16-byte aligned
 * arrays, nothing outside an array is written, and no entry point refuses an array for its alignment.  Alignment only selects
 * the kernel form, per call, from that call's pointers:
 *   fp32 Jacobi sweeps (gpu_jacobi_sweeps, _sweep_range, _pair_ranges, _triple_ranges, gpu_projection_jacobi): the float4 and
 *     fused kernels need ni % 4 == 0, ni >= 32 and in, div, out all on 16-byte boundaries; otherwise one generic sweep per
 *     launch, and the range entry points return 0 ("does not apply") with nothing written.
 *   masked and walled sweeps (gpu_jacobi_sweeps_masked[_walls], _walls_triple_ranges): the fused kernel reads the four flag
 *     bytes of a float4 column as one word, so it needs solid / solidw on a 4-byte boundary as well; otherwise one masked
 *     sweep per launch (byte reads).  rows is read bytewise everywhere.  gpu_obstacle_loads has a word and a byte form likewise.
 *   gpu_clamp_extrema_box[_w] and the limiter inside gpu_maccormack / gpu_clamp_extrema: the float4 kernel on rows of 4 m floats
 *     needs both arrays on 16-byte boundaries; otherwise the scalar kernel.
 *   fp64 (gpu_smoothing_jacobi, gpu_multi_grid_conjugate_gradient): the double2 kernels need even ni and x, temp, b on 16-byte
 *     boundaries (the launch that also stores a level's residual: that array too), the fused level-0 passes (FL_OPT_MGCG_FUSE)
 *     every array; otherwise one cell per lane and the single passes.
 *   gpu_max_field*, gpu_max_abs3: a scalar head up to the first 16-byte boundary, float4 bulk, scalar tail.
 *   everything else (gathers, map updates, streaming operators, flags, faces, diagnostics, render, sources, tracers, box
 *     copies, the PCG operators: gpu_pcg_solve's work array holds 2-byte codes and then doubles at a multiple of 256 bytes) has one
 *     form, made of accesses no wider than it may assume.
 *   Three kernels issue accesses wider than their alignment BY DESIGN, because their row length makes it unavoidable, and rely on
 *     gfx950 serving global and buffer accesses at dword alignment: the float4 limiter on rows of 4 m + 1 floats, the double2
 *     smoother and stencil on rows of an odd number of doubles, and the two-dword corner loads of the gathers.
 * tests/test_gpu_alignment.py holds every family to this on arrays 1, 2 and 3 elements off a 16-byte boundary between guard bytes.
 */

/* ------------------------------------------------------------------------------------------
 * 2. Runtime mini-ABI (replaces gpuMapper's direct CUDA runtime calls)
 * ---------------------------------------------------------------------------------------- */
enum {
    FL_OK = 0,
    FL_ERR_NO_DEVICE = 1,       /* no HIP device / wrong architecture                         */
    FL_ERR_HIP = 2,             /* a HIP runtime call failed (text in fl_last_error_string)   */
    FL_ERR_BAD_ARGUMENT = 3,
    FL_ERR_UNSUPPORTED = 4,
    FL_ERR_COMM = 5             /* RCCL failure                                               */
};

/* ---- contexts (round 3) ----
 * All state of this library -- device, the three streams, the option table, the error latch, the z-slab context and plane
 * window, the communicator, profiles, cached graphs -- belongs to a CONTEXT.  A program that never creates one uses the
 * default context and notices nothing.  fl_context_create(device) makes another (its own streams on `device`; NULL on
 * failure, the error latched on the caller's context), fl_context_make_current switches the calling THREAD to it (NULL: back
 * to the default context; thread-local, like hipSetDevice -- which it also calls), and every fl_* / gpu_* call of that thread
 * then acts on it.  One process can so drive several devices (SURVEY section 5's "single process, 8 devices": one context
 * and communicator per device, one thread each or one thread switching) or several solvers on one device side by side.
 * The host solver's C API (bimocq_solver.h) remembers the context a solver was created under and switches to it in every
 * call.  Buffers belong to the device, not to a context; a context must be current when its resources are used or freed. */
typedef struct fl_context fl_context;
fl_context *fl_context_create(int device);
void        fl_context_make_current(fl_context *ctx);
fl_context *fl_context_current(void);
void        fl_context_destroy(fl_context *ctx);       /* synchronises, destroys its communicator and streams */

/* Select device `device` (findCudaDevice, GPU_Advection.h:214-226), create the compute and
 * halo streams.  Returns FL_OK or an error code (the reference exit()s; we report). */
int   fl_init(int device);
void  fl_shutdown(void);
/* fl_shutdown for EVERY live context of the process (the default one and those of fl_context_create).  The first
 * successful fl_init registers it with atexit(), so a program that simply returns from main -- or a Python process that
 * ends -- releases the library's streams while the HIP runtime is still whole; callable directly, idempotent.  A
 * communicator that is still alive is abandoned, not destroyed (fl_comm_destroy is the orderly way). */
void  fl_shutdown_all(void);
/* cudaMalloc + cudaMemset(0) (allocGPUBuffer, GPU_Advection.h:322-326).  NULL on failure. */
void *fl_malloc(size_t bytes);
void  fl_free(void *p);
void  fl_memset(void *dst, int value, size_t bytes);                    /* async on the compute stream */
void  fl_memcpy_h2d(void *dst, const void *src, size_t bytes);          /* blocking */
void  fl_memcpy_d2h(void *dst, const void *src, size_t bytes);          /* blocking, after queued work */
void  fl_memcpy_d2d(void *dst, const void *src, size_t bytes);          /* async on the compute stream */
void  fl_sync(void);
/* An auxiliary compute stream for ONE operator that is independent of the ones that follow it (round 4): between
 * fl_aux_begin() and fl_aux_end() operators are launched on a second stream that first waits for everything queued on the
 * compute stream; after fl_aux_end() launches go to the compute stream again while the auxiliary work keeps running;
 * fl_aux_join() makes the compute stream wait for it.  The caller vouches for the independence.  The host solver runs the
 * forward-map update (gpu_solve_forward: reads the velocity, updates its own three arrays) beside the backward map's DMC
 * sub-steps this way on one GPU (BQ_OPT_CONCURRENT_MAPS). */
void  fl_aux_begin(void);
void  fl_aux_end(void);
void  fl_aux_join(void);
/* Asynchronous download for the dump path (replaces the blocking cudaMemcpy of copyDeviceToHost,
 * GPU_Advection.h:276-299): pinned host memory, a copy on the library's third stream ordered after the
 * compute work queued so far, and a ticket any host thread can wait on while the next step runs. */
void *fl_malloc_host(size_t bytes);
void  fl_free_host(void *p);
void *fl_download_begin(void *host_dst, const void *dev_src, size_t bytes);
int   fl_download_wait(void *ticket);
/* startEventRecord / endEventRecord (GPU_Advection.h:228-247) */
void *fl_event_create(void);
void  fl_event_record(void *ev);
float fl_event_elapsed_ms(void *start, void *stop);                     /* synchronises on `stop` */
void  fl_event_destroy(void *ev);
int         fl_last_error(void);
const char *fl_last_error_string(void);
void        fl_clear_error(void);
/* latch an error on behalf of host code that sits on top of this ABI (first error wins) */
void        fl_report_error(int code, const char *text);
/* the hipStream_t the operators launch on (for timing / interop with other runtimes) */
void *fl_compute_stream(void);

enum {
    FL_OPT_RESIDUAL_STRIDE = 1, /* evaluate Jacobi residual norms every k-th iterate (default 0)  */
    FL_OPT_SKIP_UNIT_BLEND = 2, /* gpu_advect_*_double with blend==1 (field*1 + 0*prev): 1 (default) = no launch, the
                                   values cannot change for finite prev; 2 = one-pass field+0 kernel (turns -0
                                   into +0 like the reference); 0 = the full two-level kernel               */
    /* The five Jacobi tuning options below are decoded in one place, csrc/bq_jacobi_plan.h (JacobiTuning); one line per code,
     * saying what it does to each reader.  "fused" = the kernels that run two to four sweeps per launch. */
    FL_OPT_JACOBI_VARIANT  = 3, /* 0 (default): one sweep = jacobi_march_kernel on 16-byte aligned rows of 4 k >= 32 floats, else the generic kernel; fused kernels allowed
                                 * 1: one sweep = jacobi_generic_kernel; no fused kernel; gpu_clamp_extrema_box*: the one-thread-per-cell kernel instead of the marching one
                                 * 3: one sweep = jacobi_march_kernel (generic where float4 rows do not apply); fused kernels allowed, as with 0
                                 * any other value (2): one sweep = jacobi_tile_kernel (generic where float4 rows do not apply); no fused kernel */
    FL_OPT_PROFILE_JACOBI  = 4, /* record a hipEvent pair around each projection's sweep loop      */
    FL_OPT_JACOBI_KCHUNK   = 5, /* 0 (default, negative values count as 0): every reader's own rule
                                 * k > 0, every code below included: jacobi_march_kernel and jacobi_tile_kernel march chunks of k planes (24 is also a 24-plane chunk)
                                 * 1 / 2: the loads of jacobi_lean2r_kernel, jacobi_lean3r_kernel and mg_lean2r_kernel (fp64) run one / two planes ahead
                                 *        (auto: one while the arrays fit the Infinity Cache, else two; jacobi_lean3r_kernel: one)
                                 * 14: mg_lds3_kernel (fp64) in blocks of 4 output rows (8 waves) instead of 8 (12 waves)
                                 * 18 / 19: jacobi_lds_kernel, three sweeps, in blocks of 8 / 12 single rows (18 is the default); four sweeps: 18 = 6 single rows, 19 = default
                                 * 24 / 25 / 26: jacobi_lds_kernel, three sweeps, in blocks of 4 / 5 / 6 row pairs; four sweeps: always 4 row pairs (the default)
                                 * 19 / 24 / 25 / 26: gpu_jacobi_sweeps_masked launches no three-sweep kernel (it has the default shape only) */
    FL_OPT_JACOBI_ROWS     = 6, /* 0 (default): every reader's own rule -- two-row pair kernel where it pays; triples through the LDS kernels, else jacobi_lean3r_kernel;
                                 *    four sweeps per launch (jacobi_lds_kernel<.., 4>) on whole unmasked arrays with chunks of >= 24 planes, not on a z-slab
                                 *    rank -- 256^3: 49 launches of four sweeps + 1 of three for 199 sweeps, 10.1 instead of 11.0 us per sweep inside whole
                                 *    steps, 11.40 instead of 11.56 ms per step
                                 * 1: tile kernel 1 row per thread; never the two-row pair kernel (jacobi_march2_kernel); no three- or four-sweep launch
                                 * 2: tile kernel 2 rows per thread; always the two-row pair kernel; no LDS triple, no four-sweep launch; jacobi_lean3r_kernel also with chunks below 16 planes
                                 * 3: jacobi_march2r_kernel instead of jacobi_lean2r_kernel; no three- or four-sweep launch; fp64: mg_smooth2_kernel instead of mg_lean2r_kernel (A/B timing)
                                 * 4: tile kernel 4 rows per thread and jacobi_march_kernel 4 waves per block (both the default); LDS triple wherever it applies, no four-sweep launch
                                 * 5: never the LDS triple (jacobi_lean3r_kernel instead), no four-sweep launch, gpu_jacobi_sweep_triple_ranges returns 0; fp64: never mg_lds3_kernel (A/B timing)
                                 * 6: the four-sweep kernel wherever it applies (a z-slab rank and forced chunks below 24 planes included)
                                 * 7: 0 without the four-sweep kernel: the launch sequence from before it became the default (A/B timing)
                                 * 8 / 16: jacobi_march_kernel 8 / 16 waves per block; fused kernels: as any other value, below; 8 on fp64: mg_smooth2_kernel, in blocks of 512 threads
                                 * the masked triple ignores this option; gpu_jacobi_sweep_triple_ranges honours 5 only; any other value: as 0 without the LDS triple and the four-sweep kernel */
    FL_OPT_STRUCTURED_MAPS = 7, /* 9-point kernels: compile-time taps when h is a power of two (1)  */
    FL_OPT_JACOBI_FUSE     = 8, /* 0: one sweep per launch everywhere; gpu_jacobi_sweep_pair_ranges / _triple_ranges return 0; fp64: one sweep per launch
                                 * 1 (default): gpu_projection_jacobi fuses after it has checked that p and p_temp carry the same boundary shell (never on a z-slab rank);
                                 *    gpu_jacobi_sweeps and gpu_jacobi_sweeps_masked do not fuse; the *_ranges entry points launch; fp64: fused smoothers from 2^20 cells
                                 *    (mg_smooth2_kernel from 2^21)
                                 * 2 and above (but 4): gpu_projection_jacobi fuses without the check, gpu_jacobi_sweeps and gpu_jacobi_sweeps_masked fuse too (the caller
                                 *    vouches for equal boundary shells); fp64: fused smoothers at every size
                                 * 4: as 2 with at most two sweeps per launch; gpu_jacobi_sweep_triple_ranges returns 0
                                 * negative: as 0, except that the *_ranges entry points launch */
    FL_OPT_JACOBI_KCHUNK2  = 9, /* 0 (default, negative values count as 0): every fused kernel's own chunk rule
                                 * k > 0: planes marched per block of every fused kernel, fp64 smoothers included (pair kernels at least 2, jacobi_lean3r_kernel and
                                 *    mg_lean2r_kernel at least 4, the fused mgcg passes at least 4); the LDS kernels then take whole arrays from 8 planes per chunk
                                 *    instead of 24, and the four-sweep auto rule still wants 24 */
    FL_OPT_MGCG_GRAPH      = 10,/* 1 (default): the multigrid V-cycle is captured into a hipGraph once and
                                 * replayed in every outer iteration; 0: plain launches                */
    FL_OPT_FUSED_HOUSEKEEPING = 12, /* bit mask, default 0 (the reference's operator semantics).  Lets a caller drop the clears
                                 * and copies it issues around the map operators; what each bit makes the kernels do:
                                 *   1: gpu_advect_velocity/_field/_field2 and gpu_compensate_error_* write zeros outside their
                                 *      index window -- the outputs need not be cleared first (GPU_Advection.h:472-526);
                                 *   2: gpu_compensate_error_* store the uncompensated field into `init` (du/dv/dw) after
                                 *      reading it -- stage 2 of gpu_compensate_* (GPU_kernel.cu:656-658) needs no copy;
                                 *   4: gpu_solve_backwardDMC writes zeros to the border nodes of x/y/z_out (what the
                                 *      reference's cleared scratch holds there, GPU_Advection.h:464-468);
                                 *   8: gpu_solve_backwardDMC copies the border nodes of x/y/z_in to x/y/z_out instead.  */
    FL_OPT_FAST_LERP       = 11,/* 0 (default): the reference's double-evaluated lerp, results bit-identical to the
                                 * oracle.  1: every lerp of the gather kernels is one fp32 fma, fmaf(c, b-a, a) -- NOT the
                                 * reference arithmetic; deviation measured per grid size   */
    FL_OPT_MGCG_TILE       = 14,/* multigrid V-cycle, levels below 2^19 cells (63^3 and coarser; 2: below 2^21): 1 (default) smooths them with
                                 * the LDS tile kernel -- 4 (the 32-sweep calls) or 2 (the 4-sweep calls) sweeps per launch on a
                                 * 16^3 region per workgroup, and the clears of x / temp0 folded into the first two launches;
                                 * 0: one launch per sweep (mg_smooth_kernel).  Same values either way.          */
    FL_OPT_PROFILE_COMM    = 15,/* 1: every wait of the compute stream on the halo stream (fl_halo_exchange with wait != 0, fl_halo_wait,
                                 * fl_p2p_exchange) is bracketed by two timing events, and every in-stream all-reduce too; the
                                 * sums are read with fl_comm_profile().  Default 0.                                 */
    FL_OPT_RESERVE_CUS     = 16,/* k > 0: the compute stream is (re)created with a CU mask that leaves k compute units (k / 8 per
                                 * XCD) to the halo stream, so that RCCL's send/recv kernels start the moment an exchange is
                                 * issued instead of waiting for compute workgroups to drain; the Jacobi launchers size their
                                 * grids for the remaining CUs.  Setting it synchronises.  Default 0 (all CUs).       */
    FL_OPT_MGCG_BOTTOM     = 17,/* 1 (default): the two coarsest levels of the multigrid V-cycle -- when both fit one workgroup's
                                 * LDS (4096 and 512 cells: 15^3 and 7^3 of a 256^3 pyramid) -- run as ONE launch
                                 * (mg_vbottom_kernel: 32 sweeps, residual, restriction, 32 sweeps, prolongation, 4 sweeps)
                                 * instead of ~22, and the last launch of level 0's 32 sweeps also writes the residual that
                                 * follows.  0: one launch per operator.  Same values either way.                   */
    FL_OPT_FIELD_WINDOW    = 18,/* nine-point operators (gpu_advect_*, gpu_compensate_*, gpu_accumulate_*) on power-of-two
                                 * spacing: k > 0 runs them as z-marching blocks that read the sampled field out of a rolling
                                 * LDS window (bq_gather_march.hip.h) instead of gathering every corner from memory; a tap
                                 * outside the window takes the direct path, so values never change.  k = planes marched per
                                 * block (1 = chosen by the launcher).  0: the one-plane kernels.  Negative (default): on
                                 * with FL_OPT_FAST_LERP, whose kernels it speeds up, off in the exact arithmetic, which is
                                 * bound by its double-rounded lerps either way.  BQ_FIELD_WINDOW in the environment sets
                                 * the initial value.                                                                 */
    FL_OPT_COMM_CHECK      = 19,/* 1: every RCCL call of the z-slab path (ncclSend / ncclRecv of the exchanges, the scalar
                                 * all-reduces) is entered into a per-rank ledger that fl_comm_check() compares across the
                                 * ranks; the host solver calls it at the end of every step while the option is on.  A
                                 * debugging aid for the first runs on real links: a mismatch latches FL_ERR_COMM instead of
                                 * hanging or silently pairing the wrong messages.  Default 0.                        */
    FL_OPT_MGCG_FUSE       = 20,/* gpu_multi_grid_conjugate_gradient on rows of 256 or 512 cells: 1 runs the level-0 vector updates of
                                 * an outer iteration inside the stencil pass that follows each of them (update_x + residual;
                                 * add + residual + max + dot; update_dir + A dir + dot -- three launches for nine passes over
                                 * the arrays, bq_mgcg_fused.hip.inc) on grids of 2^20 cells and more, 2 on any grid of that row
                                 * length, 0 never (3: as 2 with the wave-per-row form of the kernels on rows of 256 -- the same
                                 * time, kept for A/B).  Same values.  The fused form keeps its intermediate vectors in temp1
                                 * and levels[0].b, i.e. it needs BOTH to be full-size arrays (ni nj nk doubles) -- as the
                                 * reference's caller allocates them (BimocqGPUSolver.cpp:65-66) but more than the reference's
                                 * kernels themselves touch of temp1; what temp0 / temp1 hold after the call differs (both are
                                 * scratch).  Hence the default is -1 = off until a caller says so: setting 1 is the caller's
                                 * word that its arrays have that size.  The host solver of this package (csrc/host), which
                                 * allocates them, sets 1 unless the option has been set before.                      */
    FL_OPT_SKIP_EMPTY_BRICKS = 21,/* nine-point operators on UNSTAGGERED fields, one GPU, whole arrays, the staged structured
                                 * kernels: 1 (default) puts a streaming pass in front of each advection (gpu_advect_field/_field2)
                                 * and error-stage launch (gpu_compensate_error_field/_field2, the first stage of
                                 * gpu_compensate_field) that flags the 8 x 8 x 8 bricks of the sampled fields holding anything but
                                 * the word 0x00000000, and a block whose taps can only land in empty bricks runs its stores with
                                 * every gather result taken as +0.0f -- no map look-up, no gathers.  Same bits in every output.
                                 * 0: the launches without the pass.  2: as 1, and every tested block is counted
                                 * (fl_sparse_stats).  3: as 1, and the accumulation (gpu_accumulate_field/_field2, the second
                                 * stage of gpu_compensate_field) takes part too -- not the default: through a backward map with
                                 * its zeroed border half of that operator's blocks cannot be skipped at 256^3 and it comes out
                                 * slower.  4: as 3, counting.  Staggered launches, z-slab ranks, plane windows, point mode, the
                                 * generic path, the identity accumulate and the kernels of FL_OPT_FIELD_WINDOW never take part. */
    FL_OPT_DIAG_KCHUNK     = 22,/* gpu_flow_stats: 0 (default) = the marching kernel with its own chunk rule (whole rounds of about
                                 * 16 planes per block, bq_launch_geom.h); k > 0 = chunks of k planes (tests and tuning);
                                 * negative = the one-thread-per-cell kernel (the A/B partner).  vort_mag and the maxima are
                                 * the same bits whatever the value; the sums differ in summation order only.        */
    FL_OPT_RENDER_KCHUNK   = 23,/* gpu_render_density, marches along y and z: 0 (default) = the kernels' own rule (bq_render.hip:
                                 * chunks of about 32 cells in whole rounds of blocks, one chunk where that covers the ray);
                                 * k > 0 = chunks of k cells along the march (tests and tuning); negative = one sequential march
                                 * per ray.  Marches along x are a wave-level scan and take no chunks.  Same bits whatever the value. */
    FL_OPT_CONFINE_KCHUNK = 24,/* gpu_vorticity_confinement: 0 (default) = the marching kernel with its own chunk rule (the chunk
                                 * count that costs the fewest rounds of blocks, about 32 planes per block, bq_launch_geom.h);
                                 * k > 0 = chunks of k planes (tests and tuning); negative = the one-thread-per-output-node
                                 * kernel (the A/B partner).  Same bits in every output whatever the value.           */
    FL_OPT_SKIP_EMPTY_TAPS = 25,/* the unstaggered accumulation (gpu_accumulate_field/_field2, the second stage of
                                 * gpu_compensate_field) on power-of-two spacing while FL_OPT_SKIP_EMPTY_BRICKS is 1 or 2: 1 (default)
                                 * runs it behind the flag pass and a small cell-flag pass (one byte per brick of base nodes: 0
                                 * only if every word a cell based there can hand to the gather is 0x00000000, the +1 neighbours
                                 * and the flat-index wrap at the upper ends included) as a launch that tests its own taps: after
                                 * the map look-up and the clamp every lane looks up the flag of the cell of each of its nine
                                 * taps; a wave in which no lane finds a set flag loads no corner at all and runs the operator's
                                 * stores with every gather result taken as +0.0f -- the statements of the full path, so dst +=
                                 * ..., the products with the coefficient and the dst[0] == dst[1] order stay.  Every other wave
                                 * runs the same gather in another schedule (about a fifth more instructions for two fields).
                                 * Same bits in every output.  A flag pass that finds no empty brick makes that launch return at
                                 * once; the unchanged kernel, launched behind it on an empty block list, then does the work (and
                                 * returns at once otherwise): a dense pair pays the two passes and one empty launch.  The block
                                 * classification of option 21 is not used here: the map is a backward map, whose zeroed border
                                 * widens the tile range of half the blocks to the whole grid, while the taps of a border node
                                 * land at nine definite points.  0: the accumulation as option 21 alone runs it.  With option
                                 * 21 = 2 the waves are counted (fl_sparse_wave_stats).                                */
    FL_OPT_MAP_QUARTER_FP32 = 13 /* 0 (default): every lerp of the structured map look-up follows the double-rounding
                                 * contract.  1: the caller vouches that every value of the map arrays it passes to the
                                 * 9-point operators is 0 or lies in [h/256, 1024 h] (gpu_maps_quarter_safe checks a map
                                 * set); the weight-1/4 lerps of the look-up then run as one fp32 fma, which is provably
                                 * the same value under that bound (bq_device.hip.h: lerp_q) -- same results, ~15 % fewer
                                 * issue cycles per launch.  The host solver checks its maps after every update.     */
};
void fl_set_option(int option, int value);
int  fl_get_option(int option);
/* FL_OPT_PROFILE_JACOBI: total milliseconds, sweep-kernel launches and Jacobi sweeps (a fused launch
 * performs two) of the sweep loops recorded since the previous call (blocking; resets the record) */
void fl_jacobi_profile(double *total_ms, long long *launches, long long *sweeps);
/* name of the fused sweep kernel launched last; after gpu_jacobi_sweeps: of the one that call launched most often
 * ("" before the first; for reports) */
const char *fl_jacobi_kernel_name(void);
/* name of the fused kernel the last fp64 smoothing call (gpu_smoothing_jacobi, V_Cycle) launched first ("" if none; for
 * reports and tests) */
const char *fl_mg_smooth_kernel_name(void);
/* launches of the fused level-0 kernels (FL_OPT_MGCG_FUSE) since the previous call (resets the count; for reports and tests) */
long long fl_mg_fused_launches(void);
/* smoothing launches that also stored the level's residual r = b - A x (mg_lds3_kernel's pair form: rows of 130 .. 256 doubles,
 * x, temp, b AND r on 16-byte boundaries) since the previous call (resets the count; for reports and tests) */
long long fl_mg_residual_launches(void);
/* FL_OPT_SKIP_EMPTY_BRICKS = 2 or 4: out[0] = blocks tested against the brick flags, out[1] = blocks skipped, since the last reset
 * (blocking; reset != 0 clears the counters) */
void fl_sparse_stats(long long out[2], int reset);
/* the same for one operator: kind 0 = the advection, 1 = the error stage, 2 = the accumulation */
void fl_sparse_stats_kind(int kind, long long out[2], int reset);
/* FL_OPT_SKIP_EMPTY_TAPS with FL_OPT_SKIP_EMPTY_BRICKS = 2: out[0] = waves that tested their taps against the cell flags, out[1] =
 * waves skipped, since the last reset (blocking; reset != 0 clears the counters) */
void fl_sparse_wave_stats(long long out[2], int reset);
/* the flag pass of FL_OPT_SKIP_EMPTY_BRICKS on its own (for tests and tools): one byte per 8 x 8 x 8 brick of f1 -- of f1 and
 * f2 taken together when f2 is not NULL -- into flags_host (HOST memory, ceil(ni/8) ceil(nj/8) ceil(nk/8) bytes, x fastest):
 * 1 = some word of the brick is not 0x00000000.  *any_empty (may be NULL): 1 when a brick is empty.  Blocking.  Returns the
 * number of bricks, -1 on an error. */
int gpu_brick_flags(const float *f1, const float *f2, int ni, int nj, int nk, unsigned char *flags_host, int *any_empty);

/* ------------------------------------------------------------------------------------------
 * 3. Additive entry points (no reference counterpart)
 * ---------------------------------------------------------------------------------------- */
/* precondition check of FL_OPT_MAP_QUARTER_FP32: 1 when every value of x, y, z is 0 or in [h/256, 1024 h]; blocking;
 * z-slab ranks get one common answer */
/* 1 when a gpu_max_abs3 since the last reset met a NaN or an Inf in the velocity (on any slab rank; reset != 0 clears).  The
 * CFL maximum skips NaNs like the reference's host scan (BimocqGPUSolver.cpp:348-373), so a run that has gone NaN -- e.g. a
 * source whose axis passes through grid nodes, SURVEY Q14 -- would otherwise look perfectly calm to its driver. */
int  fl_nonfinite_seen(int reset);
int  gpu_maps_quarter_safe(const float *x, const float *y, const float *z, float h, int ni, int nj, int nk);
/* the same check without a pass over the maps: while armed, gpu_solve_backwardDMC (word 0) and gpu_solve_forward (word 1)
 * flag every value they store that fails the test.  _reset(which) arms the guard and clears a word (which < 0: off);
 * _read fills ok[0], ok[1] (1 = nothing flagged since the reset); blocking, z-slab ranks get common answers */
void fl_map_guard_reset(int which);
void fl_map_guard_read(int ok[2]);
/* maps <- (i*h, j*h, k*h): the host loop + H2D of MapperBaseGPU::init (Mapping.cpp:306-328) */
void gpu_init_maps(float *x, float *y, float *z, float h, int ni, int nj, int nk);
/* gpu_solve_backwardDMC / gpu_solve_forward with promises of the caller (`hints`, FL_MAP_HINT_* or-ed) that let the
 * kernels skip work the result does not need.  Results are bit-identical to the plain entry points whenever the promises
 * are true; a false promise gives wrong maps.  A promise the library cannot use (spacing not a power of two, a plane
 * window, a slab context) is ignored: the plain kernel runs.
 *   FL_MAP_HINT_FINITE    every value of u, v, w is finite (and below 2^126 in magnitude): both velocity look-ups of a DMC
 *                         sub-step are at grid nodes, where the trilinear sample is the mean of two values -- but only in
 *                         value, and only while the six discarded corners are finite.  gpu_max_abs3 tells (fl_nonfinite_seen).
 *   FL_MAP_HINT_IDENTITY  (with _FINITE) x/y/z_in resp. x/y/z_fwd hold what gpu_init_maps wrote for these dims: the DMC
 *                         sub-step computes the map corners it would load, the forward trace its start, whose first velocity
 *                         look-up is then a node look-up too. */
enum { FL_MAP_HINT_FINITE = 1, FL_MAP_HINT_IDENTITY = 2 };
void gpu_solve_forward_hint(float *u, float *v, float *w, float *x_fwd, float *y_fwd, float *z_fwd,
                            float h, int ni, int nj, int nk, float cfldt, float dt, unsigned hints);
void gpu_solve_backwardDMC_hint(float *u, float *v, float *w, float *x_in, float *y_in, float *z_in,
                                float *x_out, float *y_out, float *z_out,
                                float h, int ni, int nj, int nk, float substep, unsigned hints);
/* which map-update kernel ran last (which: 0 DMC sub-step, 1 forward update; "" before the first): "dmc_kernel",
 * "dmc_node_kernel", "dmc_node_identity_kernel", "forward_kernel", "forward_identity_kernel" -- and which have run since
 * the last reset, as bits 1, 2, 4, 8, 16 in that order (reset != 0 clears).  For reports and tests. */
const char *fl_map_kernel_name(int which);
int  fl_map_kernels_seen(int reset);
/* device getCFL (BimocqGPUSolver.cpp:348-373): max(1e-4, max|u|,|v|,|w|); blocking */
float gpu_max_abs3(const float *u, const float *v, const float *w, int ni, int nj, int nk);
/* the three stages of gpu_projection_jacobi, separately launchable */
void gpu_divergence(const float *u, const float *v, const float *w, float *div,
                    int ni, int nj, int nk, float halfrdx);
/* `sweeps` Jacobi sweeps ping-ponging p <-> p_temp starting from p; returns 0 if the newest
 * iterate ends in p, 1 if it ends in p_temp.  Boundary cells are never written. */
int  gpu_jacobi_sweeps(float *p, const float *div, float *p_temp,
                       int ni, int nj, int nk, int sweeps, float alpha, float beta);
/* window: cells 2 <= i < ni, 2 <= j < nj, 2 <= kg < nk_global (kg the GLOBAL plane on a z-slab rank).  A slab rank's first
 * local plane may lie inside it: u and v are updated there too, w -- which reads the plane below -- is not.  The rule of
 * gpu_gradient, gpu_gradient_delta and the gradient stage of gpu_projection_jacobi alike (the oracle's orc_gradient).
 * gpu_multi_grid_conjugate_gradient_slab differs on purpose: it keeps its pressure on its own plane range and promises the
 * projected velocity on the owned planes and 7 ghost planes only, so it leaves the whole first stored plane alone. */
void gpu_gradient(float *u, float *v, float *w, const float *p,
                  int ni, int nj, int nk, float halfrdx);
/* gpu_gradient that also returns what it changed: (du, dv, dw) = new - old on the update window, 0 elsewhere --
 * the d*Proj = U - UTemp of BimocqGPUSolver.cpp:188-193 without the snapshot copies and the subtraction passes */
void gpu_gradient_delta(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                        int ni, int nj, int nk, float halfrdx);
/* one Jacobi sweep in -> out over the local planes [k_begin, k_end) only: lets a z-slab host sweep the
 * planes that do not depend on ghost planes while those are still being exchanged */
void gpu_jacobi_sweep_range(const float *in, const float *div, float *out, int ni, int nj, int nk,
                            int k_begin, int k_end, float alpha, float beta);
/* TWO Jacobi sweeps in -> out in one launch, `out` written on the local planes [k0a, k1a) and [k0b, k1b) only (either
 * range may be empty): a z-slab host issues the first two sweeps after an exchange as the planes whose two-sweep stencil
 * stays inside the owned planes (while the ghost planes are in flight) and then the rest.  Both buffers must carry the
 * same boundary layer (as for FL_OPT_JACOBI_FUSE = 2).  Returns 1 when the fused kernel ran, 0 when it does not apply
 * to this grid -- nothing was launched and the caller falls back to gpu_jacobi_sweep_range. */
int gpu_jacobi_sweep_pair_ranges(const float *in, const float *div, float *out, int ni, int nj, int nk,
                                 int k0a, int k1a, int k0b, int k1b, float alpha, float beta);
/* THREE sweeps in -> out in one launch on the local planes [k0a, k1a) and [k0b, k1b) (either may be empty), through the
 * LDS-exchanged kernels (rows of 32 .. 512 floats): the pieces of a z-slab rank's pressure chunk.  `in` must be valid three
 * planes beyond each range; same precondition as above.  Returns 1 when it ran, 0 when it does not apply (nothing launched). */
int gpu_jacobi_sweep_triple_ranges(const float *in, const float *div, float *out, int ni, int nj, int nk,
                                   int k0a, int k1a, int k0b, int k1b, float alpha, float beta);
/* exact sum r^2 (double) and max|r| of r = div - (sum6 p - 6p) over interior cells; blocking */
void gpu_residual_norms(const float *div, const float *p, int ni, int nj, int nk,
                        double *sum_sq, float *max_abs);
/* stage 1 of gpu_compensate_velocity / _field on its own (compensate_kernel, GPU_kernel.cu:438-499,
 * launches :652-654 / :676): u_src = blend9(u(psi_fwd(x))) - du.  The full operator is then
 * [this] ; du <- u ; gpu_accumulate_*(u_src -> u, backward map, -0.5) ; gpu_clamp_extrema_box(du, u),
 * which lets a z-slab host refresh ghost planes between the stages. */
void gpu_compensate_error_velocity(float *u, float *v, float *w, float *du, float *dv, float *dw,
                                   float *u_src, float *v_src, float *w_src,
                                   float *forward_x, float *forward_y, float *forward_z,
                                   float h, int ni, int nj, int nk, bool is_point);
void gpu_compensate_error_field(float *u, float *du, float *u_src,
                                float *forward_x, float *forward_y, float *forward_z,
                                float h, int ni, int nj, int nk, bool is_point);
/* Batched forms: fields that live on the same nodes share ONE map look-up (the look-up is ~70 % of a
 * gather kernel's arithmetic).  Each is, result for result, the two single calls it names, in order.
 *   gpu_advect_field2            = gpu_advect_field(field1..) ; gpu_advect_field(field2..)
 *   gpu_compensate_error_field2  = gpu_compensate_error_field(u1..) ; (u2..)
 *   gpu_accumulate_field2        = gpu_accumulate_field(change1, dinit1, coeff1) ; (change2, dinit2, coeff2)
 *   gpu_accumulate_velocity2     = gpu_accumulate_velocity(change1 -> d*_init, coeff1) ; (change2 -> d*_init, coeff2)
 * (BimocqGPUSolver.cpp:144-145 advects rho and T back to back; :213-214 accumulates the force and the
 * projection change back to back.) */
void gpu_advect_field2(float *field1, float *field1_init, float *field2, float *field2_init,
                       float *backward_x, float *backward_y, float *backward_z,
                       float h, int ni, int nj, int nk, bool is_point);
void gpu_compensate_error_field2(float *u1, float *du1, float *u1_src, float *u2, float *du2, float *u2_src,
                                 float *forward_x, float *forward_y, float *forward_z,
                                 float h, int ni, int nj, int nk, bool is_point);
void gpu_accumulate_field2(float *change1, float *dinit1, float coeff1, float *change2, float *dinit2, float coeff2,
                           float *forward_x, float *forward_y, float *forward_z,
                           float h, int ni, int nj, int nk, bool is_point);
void gpu_accumulate_velocity2(float *u_change1, float *v_change1, float *w_change1, float coeff1,
                              float *u_change2, float *v_change2, float *w_change2, float coeff2,
                              float *du_init, float *dv_init, float *dw_init,
                              float *forward_x, float *forward_y, float *forward_z,
                              float h, int ni, int nj, int nk, bool is_point);
/* one component (axis 0/1/2 = u/v/w) of gpu_accumulate_velocity with one or two sources (change2 may be NULL):
 * d_init += blend9(coeff1*change1(psi(x))) [then += blend9(coeff2*change2(psi(x)))].  For hosts that know a
 * component's source to be identically zero (no force acts on u and w when only buoyancy is on). */
void gpu_accumulate_component(float *change1, float coeff1, float *change2, float coeff2, float *d_init,
                              float *forward_x, float *forward_y, float *forward_z,
                              float h, int ni, int nj, int nk, int axis, bool is_point);
/* gpu_accumulate_velocity when the caller KNOWS the forward map is the identity map gpu_init_maps wrote
 * (BimocqGPUSolver.cpp:222-223: accumulate right after reinitializeMapping): with power-of-two spacing
 * the mapped positions follow from the node indices alone, by the same lerps, and the map is not read.
 * Same results as gpu_accumulate_velocity on that map. */
void gpu_accumulate_velocity_identity(float *u_change, float *v_change, float *w_change,
                                      float *du_init, float *dv_init, float *dw_init,
                                      float *forward_x, float *forward_y, float *forward_z,
                                      float h, int ni, int nj, int nk, bool is_point, float coeff);
/* the sweeps of gpu_diffuse_field without its two copies: `sweeps` times out = (field + coef*sum6(in))/(1+6coef)
 * on interior cells, ping-ponging in <-> out; returns 0 if the newest iterate ends in `in`, 1 if in `out`.
 * Lets a z-slab host refresh ghost planes between chunks of sweeps. */
int gpu_diffuse_sweeps(const float *field, float *in, float *out, int ni, int nj, int nk, int sweeps, float coef);
/* smoothing_jacobi<double> (GPU_kernel.cu:1464-1483) on its own: `iter` (rounded up to even) sweeps of
 * x' = ((sum6 x) + alpha*b) * beta on interior cells, ping-ponging x <-> temp; the newest iterate ends in x.
 * x and temp must carry the same boundary layer (V_Cycle clears both): sweeps are fused pairwise. */
/* gpu_multi_grid_conjugate_gradient on a z-slab rank with the grid's fine levels SHARED between the ranks (round 4;
 * csrc/bq_mgcg_slab.hip.inc): every level the ranks share is stored as owned planes + ghost planes, the single-GPU launchers run
 * on those plane ranges with the ghost planes computed redundantly and refreshed by the neighbour exchange (fl_halo_exchange),
 * the float-narrowed block dot products are computed per rank and all-gathered for the reference's final sum, thin levels are
 * gathered and solved replicated.  Bit-identical to the single-domain solver.
 *   u, v, w      the rank's LOCAL velocity buffers, planes [own0 - ghost, own1 + ghost) (w one more), ghost planes correct
 *   tempResult   device, 4096 doubles: the reference's residual history (identical on every rank)
 * Collective (every rank of the communicator calls it with its own planes).  gpu_mgcg_slab_supported says whether a
 * decomposition can run this way: planes of a multiple of 256 cells, equal slabs of a multiple of 8 planes that hold at least
 * 17, ghost >= 8 (csrc/bq_mgcg_slab_plan.h); the host solver keeps the replicated solve otherwise.  The answer depends on the
 * grid, the ghost depth and the number of ranks only, so every rank of a communicator gets the same one -- callers choose
 * between two collectives by it; rank, own0 and own1 must describe those equal slabs (pass fl_comm_rank / fl_comm_size).  On
 * return the velocity is projected on the owned planes and on 7 ghost planes of either side. */
int  gpu_mgcg_slab_supported(int ni, int nj, int nkg, int own0, int own1, int ghost, int rank, int nranks);
void gpu_multi_grid_conjugate_gradient_slab(float *u, float *v, float *w, double *tempResult,
                                            int ni, int nj, int nkg, int own0, int own1, int ghost, int iter, double halfrdx);
void gpu_smoothing_jacobi(double *x, double *b, double *temp, double alpha, double beta,
                          int ni, int nj, int nk, int iter);
/* max(0, max of field[0..count)) with NaNs skipped -- the host scan of MapperBaseGPU::estimateDistortion
 * (Mapping.cpp:500-516) over the buffer gpu_estimate_distortion filled, as a device reduction; blocking.
 * Intended for non-negative data (it reduces |x|).  Not slab-aware. */
float gpu_max_field(const float *field, size_t count);
/* the same over the planes this rank OWNS of a scalar-sized field of nk local planes, all-reduced over the slab ranks
 * (single GPU: the whole field): estimateDistortion on z-slab ranks */
float gpu_max_field_owned(const float *field, int ni, int nj, int nk);
/* out[0] / out[1]: how many cells along z the backward / forward map (their z components bz, fz) carries a node at most --
 * max |map_z - z| / h over the nodes the map updates write (2 <= i, j, k <= n - 3), owned planes, all-reduced over the slab
 * ranks; a NaN counts as infinity.  Tells a z-slab host whether maps that live for more than one step still fit its ghost
 * zone (csrc/host/fluid_solver.cpp: BQ_OPT_REINIT_MAX_TRAVEL).  Blocking. */
void  gpu_map_travel_z(const float *bz, const float *fz, float h, int ni, int nj, int nk, float out[2]);
/* clamp_extrema_box for a staggered buffer: dz = 1 for the w component (nk+1 planes) */
void gpu_clamp_extrema_box_w(const float *before, float *after, int ni, int nj, int nk_buffer);
/* clampExtrema_kernel (GPU_kernel.cu:146-167) on its own: after = clamp(after, min/max27(before)) */
void gpu_clamp_extrema_box(const float *before, float *after, int ni, int nj, int nk);

/* ------------------------------------------------------------------------------------------
 * 4. Multi-GPU: z-slab context and ghost-plane exchange (one process per GPU, RCCL over xGMI)
 * ---------------------------------------------------------------------------------------- */
/* Tell the operators that the buffers they are given hold the global cell planes
 * [koff, koff + nk_local) of a grid with nk_global planes, of which this rank owns [own0, own1).
 * Index windows, positions and clamps are then evaluated in global coordinates; reductions
 * (gpu_max_abs3, residual norms) count owned planes and are all-reduced.  nk_global <= 0 resets. */
void fl_set_slab(int koff, int nk_global, int own0, int own1, int nk_local);
/* Restrict the map operators (gpu_solve_forward, gpu_solve_backwardDMC, gpu_advect_velocity/_field/_field2,
 * gpu_compensate_error_*, gpu_accumulate_*) to the local cell planes [k0, k1): they produce exactly the nodes of those
 * planes (the w component's extra plane belongs to the window that reaches the last cell plane).  k0 < 0 switches it
 * off.  A z-slab host runs an operator on the planes that need no ghost data while the ghost planes are in flight
 * (fl_halo_exchange with wait = 0), then on the rest after fl_halo_wait.  Returns 1 if supported, 0 if not. */
int fl_set_plane_window(int k0, int k1);
/* rank 0 obtains a 128-byte ncclUniqueId, the host program distributes it, every rank calls init */
int  fl_comm_unique_id(void *id128);
int  fl_comm_init(const void *id128, int rank, int nranks);
void fl_comm_destroy(void);
/* runs every RCCL call of this library on a temporary one-rank communicator (single-GPU check of the
 * dlopen'ed binding); FL_OK or an error code with fl_last_error_string() set */
int  fl_comm_selftest(void);
/* How many RCCL communicators the current context holds: 2 = the ghost-plane exchanges (halo stream) and the in-stream
 * scalar all-reduces (compute stream) each have their own, so that neither waits for the other inside RCCL's per-communicator
 * launch order; 1 = one serves both (a RCCL without ncclCommSplit, or BQ_SINGLE_COMM=1 in the environment); 0 = none. */
int  fl_comm_count(void);
/* FL_OPT_COMM_CHECK: compare the ranks' ledgers of communicator calls since the last check (collective: every rank calls
 * it at the same point; two 8-to-24-byte all-reduces + one read-back).  FL_OK, or FL_ERR_COMM (latched) when a send has no
 * receive of the same size at the same position of its pair's sequence, or the all-reduce sequences differ.  perturb != 0
 * falsifies this rank's ledger first (tests). */
int  fl_comm_check(int perturb);
int  fl_comm_rank(void);
int  fl_comm_size(void);
/* refresh `depth` (<= G) ghost planes per side of n fields with the z-neighbours, one RCCL group on
 * the halo stream.  extra[f] = 1 for a w-type buffer (nk+1 planes).  wait != 0: the compute stream
 * waits for the exchange; else call fl_halo_wait() before touching the exchanged planes. */
void fl_halo_exchange(int n, float *const *fields, const size_t *plane_elems, const int *extra,
                      int nk_local, int G, int depth, int wait);
void fl_halo_wait(void);
/* traffic of this rank since the last reset: out[0] ghost-plane exchanges issued, out[1] bytes sent in them, out[2] point-to-point
 * message groups (wall sheets), out[3] bytes sent in them (counted also when the transport is the null or a host-side one) */
void fl_comm_stats(long long out[4], int reset);
/* FL_OPT_PROFILE_COMM: ms[0] / n[0] = milliseconds the compute stream spent blocked on the halo stream (communication that
 * no kernel hid; with a host-side transport: the wall time of its blocking calls) and the number of such waits,
 * ms[1] / n[1] = the in-stream scalar all-reduces (CFL maximum, map guard, norms), since the last reset.  Blocking. */
void fl_comm_profile(double ms[2], long long n[2], int reset);
/* ncclGetVersion() of the RCCL this process loaded (e.g. 22105), 0 when none is loaded */
int  fl_comm_rccl_version(void);
/* Host-side transport hook: replaces RCCL by two callbacks (blocking, called with the compute stream
 * idle).  `exchange` receives fl_halo_exchange's arguments and must move the planes itself
 * (fl_memcpy_d2h / its own wire / fl_memcpy_h2d; plane ranges as documented in bq_halo.hip);
 * `allreduce` reduces `count` host values in place.  Used to run slab ranks over gloo / shared
 * memory, e.g. several ranks on one GPU in the tests. */
typedef void (*fl_exchange_cb)(int n, float *const *fields, const size_t *plane_elems, const int *extra,
                               int nk_local, int G, int depth);
typedef void (*fl_allreduce_cb)(void *host_values, int count, int is_double, int is_max);
void fl_comm_set_custom(int rank, int nranks, fl_exchange_cb exchange, fl_allreduce_cb allreduce);
/* timing aid: play rank `rank` of `nranks` with a transport that moves nothing and never waits (the compute-side cost
 * of the z-slab path on one GPU; results near the slab boundary are meaningless) */
void fl_comm_set_null(int rank, int nranks);

/* ---- wall sheets: what makes z-slab ranks reproduce ONE GPU bit for bit in the reference-faithful mode -------------
 * The reference zeroes the border nodes of the backward map in every DMC update (GPU_Advection.h:464-468, the protecting
 * pre-copy is commented out at :335-337).  Stage 3 of gpu_compensate_* (cumulate_kernel with the backward map,
 * GPU_kernel.cu:659-661) interpolates towards those zeros on the first and last node layer of its index window: such a
 * tap lands at 1/4, 1/2 or 3/4 (or a product of those) of its position -- near the wall on one GPU, arbitrarily far
 * along z for a slab rank.  The cells those taps can touch form a few thin sheets; a slab rank collects them from the
 * ranks that own them into a copy of the sampled field that spans the needed global planes, and re-evaluates the wall
 * layers from that copy.  Pieces (host computes WHICH boxes; csrc/host/wall_sheets.*): */
typedef struct fl_box { int x0, x1, y0, y1, z0, z1; } fl_box;   /* half-open, GLOBAL indices of the field's buffer */
/* All three box calls: a box that leaves the field (fl_box_copy: the source's or the destination's planes) or is inverted
 * (x1 < x0, ...) latches FL_ERR_BAD_ARGUMENT for the whole list before anything is written; zero-volume boxes are legal and
 * take no room in `packed`; nboxes == 0 is a no-op. */
/* packed <- the boxes of `field`, one after the other, x fastest.  `field` holds the global planes [koff, koff + nk_field)
 * of a buffer with rows of nbi and planes of nbi*nbj floats; every box must lie inside them.  `boxes` is a HOST array. */
void fl_box_pack(const float *field, int nbi, int nbj, int nk_field, int koff, const fl_box *boxes, int nboxes, float *packed);
/* the inverse, into `field`; packed == NULL fills the boxes with NaN (a cell the plan missed must not pass for data) */
void fl_box_unpack(float *field, int nbi, int nbj, int nk_field, int koff, const fl_box *boxes, int nboxes, const float *packed);
/* the boxes straight from one field to another with the same rows that holds other global planes: dst(cell) <- src(cell) */
void fl_box_copy(const float *src, int nbi, int nbj, int nk_src, int koff_src, float *dst, int nk_dst, int koff_dst,
                 const fl_box *boxes, int nboxes);
/* n point-to-point messages in one RCCL group on the halo stream: send[m] (send_count[m] floats) goes to rank peers[m],
 * recv[m] (recv_count[m] floats) comes from it; a count may be 0.  Ordered after the compute work queued so far; the
 * compute stream waits for the transfers.  Peers need not be z-neighbours (xGMI is a full mesh: one link per pair). */
void fl_p2p_exchange(int n, const int *peers, float *const *send, const size_t *send_count,
                     float *const *recv, const size_t *recv_count);
/* the same without the compute stream waiting: the messages travel while the compute stream goes on; fl_halo_wait()
 * before the received data are read or the send buffers rewritten (a later fl_halo_exchange / fl_halo_wait pair covers it
 * too: the halo stream runs its exchanges in order).  A host-side transport completes inside the call. */
void fl_p2p_exchange_begin(int n, const int *peers, float *const *send, const size_t *send_count,
                           float *const *recv, const size_t *recv_count);
/* host-side transport for fl_p2p_exchange (see fl_comm_set_custom; called with the compute stream idle) */
typedef void (*fl_p2p_cb)(int n, const int *peers, float *const *send, const size_t *send_count,
                          float *const *recv, const size_t *recv_count);
void fl_comm_set_custom_p2p(fl_p2p_cb p2p);
/* cumulate_kernel's expression (GPU_kernel.cu:376-436) on the nodes of its index window with i in xlist, j in ylist or
 * GLOBAL plane in zlist (host arrays, at most 8 entries each), the source read from `src`, which holds the global
 * planes [src_koff, src_koff + src_nk) of the sampled field:  dst = before + blend9(coeff * src(map(x))), `before`
 * being dst's value ahead of the stage (gpu_compensate_*'s stage-2 copy).  axis: -1 scalar, 0/1/2 = u/v/w buffers.
 * The maps and before/dst are local slab buffers (slab context, plane window honoured).  A node of a slab's FIRST local plane
 * looks its map up in cells that start one plane below the buffer: where that plane lies inside the global window its listed
 * nodes are written, but with unspecified ghost data (as with every nine-point operator there; no host reads that plane). */
void gpu_accumulate_wall_fixup(const float *src, int src_koff, int src_nk, const float *before, float *dst,
                               const float *mx, const float *my, const float *mz,
                               float h, int ni, int nj, int nk, int axis, float coeff,
                               const int *xlist, int nxl, const int *ylist, int nyl, const int *zlist, int nzl);
/* gpu_advect_vel_double / gpu_advect_field_double (GPU_kernel.cu:236-310, 600-638) for a z-slab rank with blend_coeff != 1 in the
 * reference-faithful mode (zeroed map border).  The kernel's second look-up reads the PREVIOUS backward map at the
 * position the current one returns; where that lands in a cell with zeroed border nodes (more than 3/4 of a cell towards a wall
 * from the outermost nodes of the window) all three components come back scaled by the live nodes' weight s in [0, 1], and the
 * *_prev field is sampled at s * q -- anywhere on the segment from the origin to the node, on any rank's planes, with a
 * data-dependent s.  No sheet bounds that: these entry points take the *_prev fields of the WHOLE grid (nk_global planes, + 1
 * for w; plane 0 = global plane 0), which the host solver assembles once per re-initialisation -- the only time they change
 * (BimocqGPUSolver.cpp:503-527).  Everything else (fields, maps, windows, clamps) as in the local forms; global arrays below
 * 2 GiB.  Ref: Mapping.cpp:383-390. */
void gpu_advect_vel_double_global(float *u, float *v, float *w,
                                  float *uprev_global, float *vprev_global, float *wprev_global,
                                  float *backward_x, float *backward_y, float *backward_z,
                                  float *backward_xprev, float *backward_yprev, float *backward_zprev,
                                  float h, int ni, int nj, int nk, bool is_point, float blend_coeff);
void gpu_advect_field_double_global(float *field, float *field_prev_global,
                                    float *backward_x, float *backward_y, float *backward_z,
                                    float *backward_xprev, float *backward_yprev, float *backward_zprev,
                                    float h, int ni, int nj, int nk, bool is_point, float blend_coeff);

/* ---- solid obstacles ------------------------------------------------------------------------
 * Analytic obstacles, classified by squared distances at the reference CPU solver's sample positions: cell (i,j,k) at
 * (i h, j h, k h), the u face at ((i - 1/2) h, j h, k h), v and w likewise.  `solid`: one byte per cell, 0 = fluid,
 * o + 1 = solid, made so by obstacle o (the last obstacle in the list that covers the cell).  `rows`: the rows summary of
 * the masked sweeps, one byte per (row j, plane k) (nj * nk bytes, j fastest), 1 when a solid cell lies in rows j-1 .. j+1
 * of planes k-1 .. k+1.  At most BQ_MAX_BOUNDARIES obstacles; the list is passed by host pointer.  Single GPU. */
#ifndef BQ_BOUNDARY_DEFINED
#define BQ_BOUNDARY_DEFINED
enum { BQ_SHAPE_SPHERE = 0, BQ_SHAPE_BOX = 1, BQ_SHAPE_LEVELSET = 2 };
enum { BQ_MAX_BOUNDARIES = 16 };
typedef struct bq_boundary {
    int   shape;
    float cx, cy, cz;        /* centre, world units                                          */
    float rx, ry, rz;        /* sphere: radius in rx; box: half extents                      */
    float vx, vy, vz;        /* velocity: the solid face velocity, and the motion per update */
} bq_boundary;
/* A level set (shape BQ_SHAPE_LEVELSET; DESIGN.md section 14, "Level sets"): a dense float32 signed-distance grid,
 * phi[k][j][i] (x fastest, nx, ny, nz >= 2, nx * ny * nz < 2^31), negative inside.  phi[k][j][i] is the value at index
 * (i0 + i, j0 + j, k0 + k) of the level set's own index space, whose index (0, 0, 0) sits at the obstacle's centre
 * (cx, cy, cz) of its bq_boundary entry (rx, ry, rz unused); `voxel` > 0 is its spacing, `background` > 0 the value it
 * takes outside the stored nodes (OpenVDB's half_width * voxel).  A node is solid when the trilinear sample is <= 0 and
 * band when 0 < sample < background.  Outside the stored nodes the sample is `background`, i.e. fluid: the stored nodes
 * must enclose the solid and its band. */
typedef struct bq_levelset {
    const float *phi;        /* nz * ny * nx floats (device pointer for the gpu_*_ls operators)  */
    int   nx, ny, nz;
    int   i0, j0, k0;        /* index of phi[0][0][0]                                         */
    float voxel, background;
} bq_levelset;
#endif
/* cell flags and rows summary of the obstacles at their current centres (one launch after a clear of `rows`) */
void gpu_obstacle_flags(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, float h,
                        int ni, int nj, int nk);
/* every face of a solid cell takes the velocity of the obstacle that owns it (the later of the two cells' owners);
 * where du/dv/dw are non-NULL they receive obstacle velocity - previous value on those faces (the d*Proj share of the
 * face write) and are left alone elsewhere */
void gpu_obstacle_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                        const bq_boundary *b, int n, int ni, int nj, int nk);
/* one masked Jacobi sweep in -> out: interior fluid cells with s solid neighbours take today's sum times
 * beta_s = (float)(1 / (1/(double)beta - s)) (beta_0 = beta; s = 6: 0); solid and boundary cells are not written.
 * Cells whose rows summary is 0 run today's expression without reading the flags. */
void gpu_jacobi_sweep_masked(const float *in, const float *div, float *out, const unsigned char *solid,
                             const unsigned char *rows, int ni, int nj, int nk, float alpha, float beta);
/* `sweeps` masked sweeps ping-ponging p <-> p_temp from p; returns 0 when the newest iterate ends in p, 1 in p_temp.
 * With FL_OPT_JACOBI_FUSE = 2 (the caller vouches that p and p_temp carry the same boundary layer and the same values in
 * solid cells) three sweeps per launch through the masked form of the LDS three-sweep kernel (rows of 32 .. 256 floats,
 * ni % 4 == 0): a block with no solid cell within three cells of its outputs runs the unmasked instruction stream. */
int  gpu_jacobi_sweeps_masked(float *p, const float *div, float *p_temp, const unsigned char *solid,
                              const unsigned char *rows, int ni, int nj, int nk, int sweeps, float alpha, float beta);
/* gpu_gradient_delta (du != NULL) or gpu_gradient (du == NULL) that leaves every face with a solid cell on either side
 * alone: velocity and delta keep what gpu_obstacle_faces wrote */
void gpu_gradient_masked(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                         const unsigned char *solid, int ni, int nj, int nk, float halfrdx);
/* gpu_semilag at the band nodes of the obstacles only (0 < distance outside the surface < 3 h, no obstacle covering the
 * node): there the same value gpu_semilag writes into a cleared field; every other node is left alone */
void gpu_semilag_band(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                      float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n);
/* blendBoundary + clearBoundary in one launch: at band nodes u, v, w, rho, T take the values of us, vs, ws, rhos, Ts
 * (skipped when us == NULL), then rho = 0 in solid cells */
void gpu_obstacle_blend(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                        const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                        const bq_boundary *b, int n, float h, int ni, int nj, int nk);
/* gpu_obstacle_flags, gpu_semilag_band and gpu_obstacle_blend for lists that may hold level sets: `ls` is a host array
 * of n descriptors whose phi are device pointers; entry o is read only when b[o].shape == BQ_SHAPE_LEVELSET (ls may be
 * NULL when no entry is one).  Analytic entries are classified exactly as above.  A bad descriptor (null phi, a
 * dimension below 2, nx * ny * nz >= 2^31, an index range beyond int, a non-finite or non-positive voxel or background)
 * latches FL_ERR_BAD_ARGUMENT. */
void gpu_obstacle_flags_ls(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n,
                           const bq_levelset *ls, float h, int ni, int nj, int nk);
void gpu_semilag_band_ls(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                         float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n,
                         const bq_levelset *ls);
void gpu_obstacle_blend_ls(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                           const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                           const bq_boundary *b, int n, const bq_levelset *ls, float h, int ni, int nj, int nk);
/* Rigid poses (an extension, the reference's obstacles only translate): entry o of a list may carry
 * an orientation and an angular velocity about its centre.  The nine entries of the body -> world rotation R are formed
 * on the host in double from the four floats by the scale-free formula (s = w^2 + x^2 + y^2 + z^2, R00 = 1 - 2 (y^2 +
 * z^2) / s, R01 = 2 (x y - w z) / s, ...) and rounded to float; the kernels see R only.  An entry is ORIENTED when it is
 * not a sphere and (qx, qy, qz) != (0, 0, 0): it is classified at the body coordinates R^T (x - c), a box by the
 * analytic test, a level set sampled at index (double)b / (double)voxel.  Every other entry is classified as above, bit
 * for bit.  An entry SPINS when (ox, oy, oz) != (0, 0, 0): its faces take v + omega x (p - c) at the face's own sample
 * position p. */
#ifndef BQ_POSE_DEFINED
#define BQ_POSE_DEFINED
typedef struct bq_pose {
    float qw, qx, qy, qz;    /* orientation, body -> world; any non-zero quaternion, need not be unit */
    float ox, oy, oz;        /* angular velocity about the centre (cx, cy, cz), world frame, rad / time unit */
} bq_pose;
#endif
/* gpu_obstacle_flags_ls, gpu_semilag_band_ls and gpu_obstacle_blend_ls for lists with poses: `pose` is a host array of n
 * entries; NULL: the _ls operator itself.  The _ls refusals apply; a non-finite component of a pose, or a quaternion whose
 * s is 0 or not finite, latches FL_ERR_BAD_ARGUMENT and launches nothing. */
void gpu_obstacle_flags_pose(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n,
                             const bq_levelset *ls, const bq_pose *pose, float h, int ni, int nj, int nk);
void gpu_semilag_band_pose(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z,
                           float h, int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n,
                           const bq_levelset *ls, const bq_pose *pose);
void gpu_obstacle_blend_pose(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs,
                             const float *ws, const float *rhos, const float *Ts, const unsigned char *solid,
                             const bq_boundary *b, int n, const bq_levelset *ls, const bq_pose *pose, float h,
                             int ni, int nj, int nk);
/* gpu_obstacle_faces where a face owned by a spinning entry takes the rigid velocity at its own sample position
 * (u = vx + (oy dz - oz dy), v = vy + (oz dx - ox dz), w = vz + (ox dy - oy dx), d = p - c in float); pose == NULL or no
 * spinning entry: the values of gpu_obstacle_faces.  The same pose refusals. */
void gpu_obstacle_faces_pose(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solid,
                             const bq_boundary *b, const bq_pose *pose, int n, float h, int ni, int nj, int nk);

/* ---- closed domain walls (reference: updateBoundary's flag-2 border, BimocqSolver.cpp:938-948, which the
 * projection treats as obstacle cells with velocity 0, :1157-1164, :1184-1256, :1288-1356) -------------------------------
 * `walls`: the closed sides, a sum of BQ_WALL_* bits.  A border cell of a closed side that no obstacle covers is a wall
 * cell: solid, velocity 0.  Open sides keep p = 0 in the border cell.  `solidw`: the obstacle flags plus BQ_FLAG_WALL in
 * the wall cells; `rows` stays the summary of the OBSTACLE flags (all zero without obstacles).  One domain, or z-slab ranks
 * without obstacles (below). */
#ifndef BQ_WALLS_DEFINED
#define BQ_WALLS_DEFINED
enum { BQ_WALL_XLO = 1, BQ_WALL_XHI = 2, BQ_WALL_YLO = 4, BQ_WALL_YHI = 8, BQ_WALL_ZLO = 16, BQ_WALL_ZHI = 32 };
enum { BQ_WALLS_NONE = 0, BQ_WALLS_REFERENCE_BOX = 1 | 2 | 4 | 16 | 32 };   /* every side but +y (:938-948) */
enum { BQ_FLAG_WALL = 0x80 };
#endif
/* solidw = solid (NULL: no obstacles) with BQ_FLAG_WALL in the wall cells (:938-948; an obstacle in the border layer
 * keeps its own flag, as flag 3 is written over flag 2) */
void gpu_wall_flags(unsigned char *solidw, const unsigned char *solid, int walls, int ni, int nj, int nk);
/* a face with a wall cell on at least one side and an obstacle cell on neither takes 0 (:1157-1164: all six faces of a
 * wall cell); where du/dv/dw are non-NULL they receive 0 - previous value there.  Writes no face gpu_obstacle_faces
 * writes. */
void gpu_wall_faces(float *u, float *v, float *w, float *du, float *dv, float *dw, const unsigned char *solidw,
                    int ni, int nj, int nk);
/* gpu_jacobi_sweep_masked / gpu_jacobi_sweeps_masked on solidw, value for value (:1184-1256): where the obstacle rows
 * summary is clean the number of solid neighbours comes from the position alone (a closed side at i = 1, i = ni-2,
 * j = 1, ...) and no flag is read; elsewhere from the flags of solidw.  walls = 0: the masked operators themselves. */
void gpu_jacobi_sweep_masked_walls(const float *in, const float *div, float *out, const unsigned char *solidw,
                                   const unsigned char *rows, int walls, int ni, int nj, int nk, float alpha, float beta);
int  gpu_jacobi_sweeps_masked_walls(float *p, const float *div, float *p_temp, const unsigned char *solidw,
                                    const unsigned char *rows, int walls, int ni, int nj, int nk, int sweeps,
                                    float alpha, float beta);
/* gpu_gradient_masked / gpu_pcg_gradient on solidw with the window starting at cell 1 instead of 2 on every axis whose
 * low side is closed (:1288-1335 update every face between two fluid cells): the faces between the cells of the first
 * interior layer behind a closed wall are projected too, so that those cells end divergence-free; behind an open side
 * the window is the unchanged one.  The faces of wall cells are solid faces and stay alone.  walls = 0: the operators
 * without walls. */
void gpu_gradient_masked_walls(float *u, float *v, float *w, const float *p, float *du, float *dv, float *dw,
                               const unsigned char *solidw, int walls, int ni, int nj, int nk, float halfrdx);
void gpu_pcg_gradient_walls(float *u, float *v, float *w, const double *p, const unsigned char *solidw, int walls,
                            int ni, int nj, int nk, double halfrdx);
/* Z-SLAB RANKS (fl_set_slab).  A library that exports the two range operators below promises that gpu_wall_flags,
 * gpu_wall_faces, gpu_jacobi_sweep_masked_walls / gpu_jacobi_sweeps_masked_walls and gpu_gradient_masked_walls honour the
 * slab context, and the host relies on it (a library without them runs walls on one domain only):
 *   - every position along z is GLOBAL: local plane k is global plane k + koff of nkg, BQ_WALL_ZLO is global plane 0 and
 *     BQ_WALL_ZHI global plane nkg - 1, so a rank in the middle has x and y walls only; the wall cells, the wall-neighbour
 *     count of the sweeps and the gradient's window (cell 1 instead of 2 behind a closed low side) follow from that;
 *   - planes of the rank's array outside the global grid hold no cell: flag 0, nothing written; the sweeps leave global
 *     planes 0 and nkg - 1 alone;
 *   - gpu_wall_faces decides a w face on the first or last plane of the window from the cell inside the window where the
 *     other one lies outside the window but inside the grid (exact for x and y walls; the face next to a closed z plane
 *     just outside the window belongs to a ghost plane the caller must count as stale); gpu_gradient_masked_walls leaves w
 *     on the window's first plane alone where the plane below it is not in the window (dw: 0), as gpu_gradient does.
 * With the context off every operator computes what it computed before.  gpu_pcg_gradient_walls stays single-domain.
 *
 * One walled sweep in -> out on the local planes [k_begin, k_end) (clipped to the interior), and three walled sweeps in one
 * launch with `out` written on [k0a, k1a) and [k0b, k1b) (either may be empty; the input valid three planes beyond each
 * range, both buffers with the same boundary layer): the walled counterparts of gpu_jacobi_sweep_range and
 * gpu_jacobi_sweep_triple_ranges, value for value gpu_jacobi_sweep_masked_walls on the same operands.  Each returns 1 when
 * it ran and 0 when it refuses, having launched nothing: bad arguments (latched), walls = 0 (latched: the masked family has
 * no range sweeps), and for the triple the shapes the whole-array walled triple refuses and FL_OPT_JACOBI_FUSE 0 / 4.  Where
 * `rows` is clean neither loads a flag. */
int  gpu_jacobi_sweep_masked_walls_range(const float *in, const float *div, float *out, const unsigned char *solidw,
                                         const unsigned char *rows, int walls, int ni, int nj, int nk, int k_begin, int k_end,
                                         float alpha, float beta);
int  gpu_jacobi_sweep_masked_walls_triple_ranges(const float *in, const float *div, float *out, const unsigned char *solidw,
                                                 const unsigned char *rows, int walls, int ni, int nj, int nk,
                                                 int k0a, int k1a, int k0b, int k1b, float alpha, float beta);

/* ---- shaped, moving smoke sources (reference: Emitter and BimocqSolver::emitSmoke of the CPU
 * solver, BimocqSolver.h:31-59, BimocqSolver.cpp:696-813) ----------------------------------------------------------------
 * A source is a shape of section 14 (sphere, box or level set) at a position.  A node belongs to it when the obstacle
 * classification calls the node solid (no band).  Cell nodes inside take the source's density and temperature; u, v and
 * w nodes inside, each sampled at its own face position, take the emitted velocity when the source has
 * BQ_SOURCE_VELOCITY: with d = node position - source position, u = ex + (oy dz - oz dy), v = ey + (oz dx - ox dz),
 * w = ez + (ox dy - oy dx), every operation one float operation in that order.  Sources act in list order, values are
 * overwritten: the last source that contains a node (for faces: and has the flag) wins. */
#ifndef BQ_SOURCE_DEFINED
#define BQ_SOURCE_DEFINED
enum { BQ_SOURCE_VELOCITY = 1 };        /* flags: the source also imposes its velocity field */
enum { BQ_MAX_SOURCES = 16 };
typedef struct bq_source {
    bq_boundary shape;                  /* shape code, position cx..cz, extents rx..rz (unused for level sets),
                                           vx..vz = the velocity the SOURCE ITSELF moves with */
    float density, temperature;
    float ex, ey, ez;                   /* emitted velocity at the position */
    float ox, oy, oz;                   /* angular velocity of the emitted field about the position */
    int   emit_frames;                  /* active while framenum < emit_frames (read by the host solver only) */
    int   flags;
} bq_source;
#endif
/* every entry of src[0 .. n) applied to the nodes of the legacy emitter's window (1 < i < n - 2 on every axis of each
 * buffer's own dimensions, the global plane index on z-slab ranks; pointwise, ghost planes included).  ni, nj, nk: CELL
 * dims.  `ls`: host array of n descriptors whose phi are device pointers, ls[o] read only when src[o].shape.shape ==
 * BQ_SHAPE_LEVELSET (NULL allowed when no entry is one).  One launch over the node boxes the entries can reach; nothing
 * is launched when no box meets the window.  n > BQ_MAX_SOURCES, an unknown shape or flag bit, a level-set entry without
 * descriptors or with a bad one latch FL_ERR_BAD_ARGUMENT and launch nothing.  So does a list whose boxes hold more than
 * 65 535 planes in all (planes are launched along grid.z: 16 sources that each span 4096 planes and more). */
void gpu_emit_sources(float *u, float *v, float *w, float *rho, float *T, const bq_source *src, const bq_levelset *ls,
                      int n, float h, int ni, int nj, int nk);

/* ---- converged fp64 projection, BQ_PROJECTION_PCG -------------------------------------------
 * The masked Neumann system of section 14 on the interior cells that are fluid with s < 6 solid neighbours (diagonal
 * 6 - s, -1 per interior fluid neighbour, border cells held at 0, b = -div), solved by flexible preconditioned CG from
 * p = 0 until max|r| <= tol * max|b| (a geometric V-cycle preconditioner on the levels of gpu_multi_grid_conjugate_gradient).
 * Single GPU. */
enum { BQ_PCG_CONVERGED = 0, BQ_PCG_ITER_LIMIT = 1, BQ_PCG_BREAKDOWN = 2 };
/* div = halfrdx ((u_r - u_l) + (v_b - v_f) + (w_u - w_d)) in fp64 at every cell (mg_divergence_kernel's expression) */
void gpu_divergence_double(const float *u, const float *v, const float *w, double *div, int ni, int nj, int nk,
                           double halfrdx);
/* solve on `div` and `solid` (NULL: no obstacles) into p (every cell written: 0 where no unknown).  r, d, q, z, t, work:
 * N-double device arrays (N = levels[0].number; their content on entry does not matter); levels[1 .. levelNum-1]: the
 * coarse levels (dims (n - 1) / 2 per axis, alpha -1, beta 1/6), cleared and used as work arrays; levels[0] gives the
 * dims only.  At most `iters` CG updates, 0 < tol < 1.  stats (host, 4 doubles): iterations, final max|r| (of the
 * recursive residual), max|b|, stop reason (BQ_PCG_*).  Blocking: reads a few doubles back per iteration. */
void gpu_pcg_solve(const double *div, double *p, const unsigned char *solid, double *r, double *d, double *q, double *z,
                   double *t, double *work, struct SCoarseLevelInfo *levels, int levelNum, int iters, double tol,
                   double *stats);
/* u -= (float)(halfrdx (p_c - p_left)) (v, w likewise) on the faces of gpu_multi_grid_conjugate_gradient's gradient
 * window [2, n) whose two cells are fluid (solid == NULL: every face of the window); other faces are left alone */
void gpu_pcg_gradient(float *u, float *v, float *w, const double *p, const unsigned char *solid, int ni, int nj, int nk,
                      double halfrdx);

/* ---- flow diagnostics -------------------------------------------------------------------------
 * One pass over the velocity that returns every scalar diagnostic and, on request, the cell-centred vorticity magnitude.
 * Arrays as everywhere: u (ni+1, nj, nk), v (ni, nj+1, nk), w (ni, nj, nk+1), rho, T and vort_mag (ni, nj, nk), x fastest; on a
 * z-slab rank kg = k + koff is the global plane and nkg the global plane count.  Per cell (i, j, k), in float, every line one
 * IEEE operation:
 *   uc = 0.5f * (u(i,j,k) + u(i+1,j,k));  vc, wc likewise along y and z
 *   d  = ((u(i+1) - u(i)) + (v(j+1) - v(j)) + (w(k+1) - w(k))) / h          (divergence_kernel's sum order, / h for halfrdx)
 *   interior cells 1 <= i <= ni-2, 1 <= j <= nj-2, 1 <= kg <= nkg-2, with q = 2.0f * h:
 *     wx = ((wc(j+1) - wc(j-1)) - (vc(k+1) - vc(k-1))) / q
 *     wy = ((uc(k+1) - uc(k-1)) - (wc(i+1) - wc(i-1))) / q
 *     wz = ((vc(i+1) - vc(i-1)) - (uc(j+1) - uc(j-1))) / q              (the mean of the four MAC edge vorticities round the cell)
 *   border cells: wx = wy = wz = 0 (so does a stored plane whose neighbour plane is not stored; owned planes always have one)
 *   in double, left to right: m2 = (double)wx*wx + (double)wy*wy + (double)wz*wz,  e2 = (double)uc*uc + (double)vc*vc + (double)wc*wc
 *   mag = (float)sqrt(m2)                                                   (the double square root: norm3df as restated here)
 * d_out (DEVICE, BQ_STAT_COUNT doubles) receives, over all cells -- on a slab rank over the owned planes, all-reduced:
 *   [0] sum e2   [1] sum m2   [2] sum (double)d*d   [3] max |d|   [4] sum rho   [5..7] sum rho*i, rho*j, rho*kg (products in
 *   double)   [8] sum T   [9] max mag.  Maxima skip NaNs as fmaxf does, sums propagate non-finite values; [4..7] are 0 when rho
 * is NULL, [8] when T is.  No floating-point atomics: two calls on the same data return the same bits.
 * vort_mag (may be NULL): every cell of the local buffer is written -- mag, 0 in border cells (no clear needed); cells of ghost
 * planes take 0 or their computed value.  Asynchronous on the compute stream, nothing synchronises; honours the slab context.
 * FL_ERR_BAD_ARGUMENT, nothing launched: NULL u, v, w or d_out, a dimension below 3, the size limits above, vort_mag overlapping
 * an input or d_out.  Returns FL_OK or the error it latched.  Solid cells count as fluid.  FL_OPT_DIAG_KCHUNK picks the kernel. */
enum { BQ_STAT_E2 = 0, BQ_STAT_M2, BQ_STAT_D2, BQ_STAT_DIV_MAX, BQ_STAT_RHO, BQ_STAT_RHO_I, BQ_STAT_RHO_J, BQ_STAT_RHO_K,
       BQ_STAT_T, BQ_STAT_VORT_MAX, BQ_STAT_COUNT };
int gpu_flow_stats(const float *u, const float *v, const float *w, const float *rho, const float *T, float *vort_mag,
                   float h, int ni, int nj, int nk, double *d_out);

/* ---- vorticity confinement ----------------------------------------------------------------------
 * uo, vo, wo = u, v, w + dt f on the faces, f = eps h (N x omega) on the cells: the confinement force of Fedkiw, Stam and Jensen
 * (Visual Simulation of Smoke, 2001) as ONE fused operator.  An extension: the reference has no such force.  Arrays as
 * everywhere: u (ni+1, nj, nk), v (ni, nj+1, nk), w (ni, nj, nk+1), x fastest.  Out of place: EVERY element of uo, vo, wo is
 * written.  Every line is one IEEE fp32 operation unless it says double (no contraction):
 *   cells 1 <= i <= ni-2, 1 <= j <= nj-2, 1 <= k <= nk-2:  uc, vc, wc and (wx, wy, wz) exactly as in gpu_flow_stats above;
 *     border cells: wx = wy = wz = 0.  m = (float)sqrt(m2) with that operator's double m2: the bits of its vort_mag.
 *   confined cells 2 <= i <= ni-3, 2 <= j <= nj-3, 2 <= k <= nk-3 (all six neighbours carry a computed omega); every other
 *   cell has f = 0:
 *     gx = (m(i+1) - m(i-1)) / (2.0f * h);  gy, gz likewise along y and z
 *     g2 = (double)gx*gx + (double)gy*gy + (double)gz*gz          (double, left to right)
 *     len = (float)sqrt(g2);   !(len > 0.f): f = 0 for this cell, else
 *     nx = gx / len;  ny = gy / len;  nz = gz / len
 *     eh = eps * h
 *     fx = eh * (ny * wz - nz * wy);  fy = eh * (nz * wx - nx * wz);  fz = eh * (nx * wy - ny * wx)
 *                                                                  (two products, one subtraction, one product each)
 *   faces:  1 <= i <= ni-1:  uo(i,j,k) = u(i,j,k) + dt * (0.5f * (fx(i-1,j,k) + fx(i,j,k)));  i = 0 and i = ni: copied.
 *           vo along j and wo along k likewise.
 * The operator does not see the obstacle mask or the walls, like gpu_flow_stats: solid cells count as fluid, and the shear at
 * a solid surface or at the domain border counts as vorticity.  (Both projections rewrite solid and wall faces before they
 * take the divergence, so the force on those faces is overwritten.)  A dimension below 5 has no confined cell: the outputs
 * equal the inputs in value.  Non-finite inputs propagate through the arithmetic as written; no special cases.
 * Asynchronous on the compute stream, one launch, nothing allocated, no floating-point atomics: same bits on every call
 * and for every FL_OPT_CONFINE_KCHUNK.  FL_ERR_BAD_ARGUMENT, nothing launched: a NULL pointer, a dimension below 3, the size
 * limits above, a negative or non-finite eps, an output overlapping an input or another output.  FL_ERR_UNSUPPORTED, nothing
 * launched: a z-slab context (fl_set_slab) -- the stencil needs three valid ghost planes and a global-plane border rule, which
 * are not built.  Returns FL_OK or the error it latched. */
int gpu_vorticity_confinement(float *uo, float *vo, float *wo, const float *u, const float *v, const float *w,
                              float h, int ni, int nj, int nk, float eps, float dt);

/* ---- per-obstacle pressure loads --------------------------------------------------------------------
 * One pass over the owner-tagged cell flags that returns, per obstacle, the sums of the pressure over its wetted faces: what a
 * caller scales into the force and the torque the fluid's pressure puts on the body.  Exactly one of p (float, the Jacobi
 * pressure) and p64 (double, the PCG pressure) is non-NULL; each holds ni nj nk values, x fastest.  `solid`: the flags as
 * gpu_obstacle_flags* / gpu_wall_flags write them.  `b`: the HOST list of n obstacles (only the centres are read).
 *   own(c) = solid[c] & 0x7f.  Cell c is an OBSTACLE CELL of o when 1 <= own(c) <= n and o = own(c) - 1, with or without
 *   BQ_FLAG_WALL (an obstacle in the border layer keeps its flag); a FLUID CELL when solid[c] == 0.  A cell with only
 *   BQ_FLAG_WALL is neither, and so is a cell with own(c) > n (the list is shorter than the flags say: the cell is ignored and
 *   never used as an index).
 *   A WETTED FACE of o is a pair of face-adjacent cells (S, F), both inside the array, S an obstacle cell of o and F a fluid
 *   cell.  Each is counted once.  Obstacle-obstacle pairs, obstacle-wall pairs and faces on the outside of the array are not
 *   wetted; a border-layer fluid cell counts like any other (on an open side its p is 0).
 * Per wetted face along axis a, with s = +1 when S has the higher index along a and -1 otherwise (+a s points from the fluid
 * into the solid), every line one IEEE double operation (no contraction):
 *   pf = (double)p[F];   f = s * pf
 *   face centre x: along a ((double)(idx_a(S) + idx_a(F)) * 0.5) * (double)h, on the other two axes (double)idx * (double)h
 *   r = x - ((double)b[o].cx, (double)b[o].cy, (double)b[o].cz)
 *   P[a] += f
 *   M += r x (f e_a):   a = x: My += rz*f, Mz -= ry*f;   a = y: Mz += rx*f, Mx -= rz*f;   a = z: Mx += ry*f, My -= rx*f
 *   FACES += 1;   PSUM += pf
 * d_out (DEVICE, BQ_MAX_BOUNDARIES x BQ_LOAD_COUNT doubles, row o = obstacle o in the order of BQ_LOAD_*): all 128 are written by
 * every successful call, rows o >= n are 0.  Non-finite pressures propagate.  The result depends only on p at the F cells of
 * wetted faces: p in solid cells, wall cells and fluid cells away from every obstacle never enters the arithmetic (a NaN there
 * leaves no trace; no such value is multiplied by 0).
 * `rows` (may be NULL): the rows summary of the obstacle flags as gpu_obstacle_flags writes it; rows with a zero byte are skipped
 * without being read.  It changes what is read, not which terms are added or their order: the 128 doubles are the same bits
 * with and without it.  No floating-point atomics: two calls on the same data return the same bits; the summation order is
 * otherwise the kernel's own.
 * What the sums mean: the masked gradient applies du = -halfrdx (p_c - p_left) on fluid-fluid faces only, so summing by parts
 * over the fluid, halfrdx h^3 P is the momentum the obstacle's surface takes from the fluid (density 1) in that projection and
 * halfrdx h^3 M the angular momentum about its centre.  The scaling is the caller's, in double.
 * Asynchronous on the compute stream: two launches, nothing allocated beyond the library's scratch (the blocks' partials,
 * blocks x n x 8 doubles), nothing synchronises once that scratch is large enough: like every operator that uses it, the
 * first call that needs more than the scratch holds waits for the compute stream and reallocates it.
 * Single GPU.  Nothing is launched and d_out is untouched on a refusal.  FL_ERR_BAD_ARGUMENT: both or neither of p / p64, NULL
 * solid or d_out, n < 0 or n > BQ_MAX_BOUNDARIES, n > 0 with NULL b, a non-finite centre, h not finite or <= 0, a dimension
 * below 3, the size limits above, d_out overlapping an input.  FL_ERR_UNSUPPORTED: a z-slab context (fl_set_slab).  n == 0 is
 * allowed and writes 128 zeros.  Returns FL_OK or the error it latched. */
enum { BQ_LOAD_PX = 0, BQ_LOAD_PY, BQ_LOAD_PZ, BQ_LOAD_MX, BQ_LOAD_MY, BQ_LOAD_MZ, BQ_LOAD_FACES, BQ_LOAD_PSUM, BQ_LOAD_COUNT };
int gpu_obstacle_loads(const float *p, const double *p64, const unsigned char *solid, const unsigned char *rows,
                       const bq_boundary *b, int n, float h, int ni, int nj, int nk, double *d_out);

/* ---- shadowed density preview --------------------------------------------------------------------
 * An emission-absorption image of the density with single-scattering self-shadowing from one directional light; the view is
 * orthographic along a grid axis.  Directions are codes 0..5 = +x, -x, +y, -y, +z, -z: the direction a ray TRAVELS.  `view` is
 * the direction from the eye into the volume, `light` the direction the light travels, light = -1 means no shadowing.
 * Image axes are the two remaining grid axes in increasing order, columns (fastest) the lower one, rows the higher one:
 *   view +-z: W x H = ni x nj (x, y)     view +-y: ni x nk (x, z)     view +-x: nj x nk (y, z)
 * on z-slab ranks nk means the global plane count nkg, and an image row along z is the global plane.
 * Per cell, every line one IEEE operation (no contraction):
 *   sh = sigma * h                      (float)
 *   r  = fmaxf(rho, 0.0f)               (a NaN density is empty, negative undershoots are empty)
 *   d  = fminf(sh * r, 32.0f)
 *   D  = trunc((double)d * 2^32)        (an integer <= 2^37)
 *   a  = 1.0f - exp_portable(-d)        (exp_portable: the oracle's orc_expf, operation for operation)
 * For a ray through the cells c0, c1, ... in travel order A(c_m) = sum of D(c_n), n < m: the exclusive prefix sum.
 *   att(A) = 0 when A >= 128 * 2^32, else exp_portable(-(float)((double)A * 2^-32))
 *   s    = att(A_light(cell))           (light = -1: s = 1.0f)
 *   q    = a * (albedo * s + ambient)   (three separately rounded float operations)
 *   Tv   = att(A_view(cell))
 *   term = trunc((double)Tv * (double)q * 2^32)
 * d_image (DEVICE, 2 W H doubles) receives per pixel: plane 0 Cfix = sum of term over the pixel's ray, plane 1 Afix = sum of D
 * over it.  Every pixel is written.  A caller derives radiance = Cfix * 2^-32 and transmittance = att(Afix).
 * Limits: 1 <= ni, nj, nk <= 65534 next to the operators' size limits above, d <= 32, 0 <= albedo, 0 <= ambient,
 * albedo + ambient <= 4 (so term <= 2^34): EVERY ACCUMULATED QUANTITY IS AN INTEGER BELOW 2^53.  It is held in doubles, may be
 * added in any order or grouping and sent through the double-sum all-reduce, and it is the same bits: chunked marches,
 * wave-level scans along x and slab ranks all give exactly the bits of the plain triple loop.  No floating-point atomics.
 * Cells with D == 0 contribute term = 0; solid obstacles are not drawn.
 * shadow: scratch field of ni nj nk floats that receives s per cell (on a z-slab rank: per cell of the OWNED planes; ghost
 * planes are not touched); NULL only with light = -1.
 * z-slab ranks (fl_set_slab): only owned planes contribute.  Views and lights along x or y cross no rank boundary: each rank
 * fills its owned rows of a zero-filled image.  With the view or the light along +-z each rank first leaves its per-column
 * total of D over its owned planes in its slot of a zero-filled world x ni x nj double buffer, one all-reduce fills every slot
 * on every rank, and a rank starts its columns at the totals of the ranks before it (after it for -z); one gather serves
 * view and light.  Last, one all-reduce (double, sum) over the 2 W H doubles gives every rank the whole image.  Both run in
 * stream order on the communicator of the scalar all-reduces, no host sync.  The gather buffer lives in the library's
 * scratch: world x ni x nj x 8 bytes, 64 MB at 1024^2 x 8 ranks.
 * Asynchronous on the compute stream.  FL_ERR_BAD_ARGUMENT, nothing launched: a NULL rho, p or d_image, view outside 0..5,
 * light outside -1..5, shadow == NULL with light >= 0, d_image or shadow overlapping rho (or each other), a non-finite or
 * negative sigma, albedo or ambient, albedo + ambient > 4, a non-finite or non-positive h, sizes outside the limits.
 * Returns FL_OK or the error it latched.  FL_OPT_RENDER_KCHUNK picks the chunking of the marches along y and z. */
typedef struct { float sigma, albedo, ambient; } fl_render_params;
int gpu_render_density(const float *rho, float *shadow, float h, int ni, int nj, int nk, int view, int light,
                       const fl_render_params *p, double *d_image);
/* gpu_render_density_solids: the same image with the solid obstacles drawn as opaque, flat-shaded,
 * shadow-casting bodies.  Everything above holds -- one IEEE operation per line, no contraction, every sum an integer below
 * 2^53 --, and in addition:
 *   solid cells   a cell is solid iff (solid[cell] & 0x7f) != 0: the low bits are the tag o + 1 that gpu_obstacle_flags* wrote.
 *                 Bit 0x80 (BQ_FLAG_WALL of solidw) is ignored: solidw may be passed, domain walls stay undrawn.
 *   density       a solid cell's density is ignored: its D is 0 whatever rho holds, NaN and huge values included.
 *   blocking      along a ray c0, c1, ... in travel order B(c_m) = 1 iff some c_n, n < m, is solid (the exclusive "blocked"
 *                 prefix); A is the exclusive prefix of D as before;  att'(A, B) = B ? 0.0f : att(A).
 *   s    = att'(A_light, B_light), written to `shadow` for every cell, solid cells included (light = -1: s = 1.0f): the first
 *          solid cell along a light ray is lit, everything behind it is in full shadow.
 *   Tv   = att'(A_view, B_view)
 *   fluid cell    today's term with that Tv.
 *   solid cell    qs   = sp->albedo * s + sp->ambient        (two float operations)
 *                 term = trunc((double)Tv * (double)qs * 2^32)
 *                 so only the first solid cell of a view ray can contribute.  Shading is flat, there is no normal term: a
 *                 sphere shows a lit half and an ambient half through s alone.
 * d_image (DEVICE, 3 W H doubles): plane 0 Cfix = sum of term, plane 1 Afix = sum of D over the whole ray (solids add 0),
 * plane 2 Hfix = the tag of the first solid cell on the view ray, 0 when there is none.  A caller derives radiance =
 * Cfix * 2^-32 and transmittance = Hfix ? 0 : att(Afix).  With all flags zero planes 0 and 1 and the shadow field are the bits
 * of gpu_render_density and plane 2 is zero.
 * Limits: sp->albedo and sp->ambient finite and >= 0, sp->albedo + sp->ambient <= 4: a solid term is <= 2^34 and every sum
 * stays below 2^53.
 * rows: the obstacles' rows summary (nj * nk bytes, above) or NULL; a row whose byte is 0 holds no solid cell.  The result is
 * the same bits with it or with NULL.  The kernels along x skip the flag loads of a row whose byte is 0 (measured: DESIGN.md
 * section 27); the marches along y and z read the flags of every cell.
 * FL_OPT_RENDER_KCHUNK applies unchanged.  Asynchronous on the compute stream.  FL_ERR_BAD_ARGUMENT, nothing launched: everything
 * gpu_render_density refuses (d_image counted as 3 W H doubles), a NULL solid or sp, sp values outside the limits, solid or
 * rows overlapping shadow or d_image.  FL_ERR_UNSUPPORTED, nothing launched: a z-slab context (fl_set_slab) -- obstacles do
 * not exist there.  Returns FL_OK or the error it latched. */
typedef struct { float albedo, ambient; } fl_render_solid_params;
int gpu_render_density_solids(const float *rho, const unsigned char *solid, const unsigned char *rows, float *shadow, float h,
                              int ni, int nj, int nk, int view, int light, const fl_render_params *p,
                              const fl_render_solid_params *sp, double *d_image);

/* ---- passive tracer particles ---------------------------------------------------------------------
 * Particles are three device arrays of n floats each (px, py, pz): world positions, cell centre i at i h like everything
 * else here.  All four operators are asynchronous on the compute stream, return FL_OK or the error they latched, launch
 * nothing when they refuse, and treat n = 0 (an empty box) as a no-op.  One GPU: FL_ERR_UNSUPPORTED under a z-slab context
 * (fl_set_slab) -- particles would have to migrate between ranks, which is not built.
 *
 * gpu_trace_particles: the reference's trace() (GPU_kernel.cu:92-125) per particle, in place: RK3 sub-steps of cfldt
 * (the last one shorter) until |dt| is used up, backwards for dt < 0, every sub-step clamped to [h, (n_a - 1) h] (the upper
 * bound evaluated as (float)n_a * h - h).  Same bits as gpu_solve_forward for a map entry that holds the same position,
 * with FL_OPT_FAST_LERP on or off.  The caller promises cfldt * max|u| <= h and positions inside the clamp box, as for the
 * forward map.  FL_ERR_BAD_ARGUMENT: a NULL pointer, n < 0, a dimension below 5 or beyond the operators' size limits,
 * cfldt <= 0 with dt != 0, a non-finite h, cfldt or dt, a position array overlapping a velocity array or another one. */
int gpu_trace_particles(const float *u, const float *v, const float *w, float *px, float *py, float *pz, long n,
                        float h, int ni, int nj, int nk, float cfldt, float dt);
/* gpu_sample_particles: out[a] = sample_buffer (GPU_kernel.cu:43-62) of `field` (nx x ny x nz floats, x fastest, value index
 * (i, j, k) at position (ox + i h, oy + j h, oz + k h)) at particle a: trilinear, a cell whose base corner has a negative
 * flat index reads zeros, a corner outside the allocation is 0.  Positions must be finite with |(p - o) / h| < 2^22.
 * A cell-centred field has o = 0, the u faces ox = (float)(-0.5 * (double)h) (v: oy, w: oz).  FL_ERR_BAD_ARGUMENT: a NULL
 * pointer, n < 0, a non-positive dimension or one beyond the size limits, `out` overlapping an input. */
int gpu_sample_particles(const float *field, int nx, int ny, int nz, float h, float ox, float oy, float oz,
                         const float *px, const float *py, const float *pz, float *out, long n);
/* gpu_seed_particles: per_cell jittered positions in every cell of the half-open cell box [i0, i1) x [j0, j1) x [k0, k1),
 * which is first intersected with the cells 1 .. n_a - 2 of every axis; bx, by, bz the extents left.  Returns nothing but the
 * status: the count bx * by * bz * per_cell is closed-form (the caller sizes the arrays with it; at most 2^31 - 1).
 * Particle p = s + per_cell * (x + bx * (y + by * z)) sits in cell C = (i0' + x, j0' + y, k0' + z): k outermost, then j, then
 * i, then the sample s.  With G = C_x + ni * (C_y + nj * C_z), the 64-bit counter c = G * per_cell + s and, all in unsigned
 * 32-bit arithmetic (wrapping),
 *     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16;  return x
 *     r_a    = mix(mix(mix((uint32)c ^ seed) + (uint32)(c >> 32)) + a * 0x9e3779b9) >> 8        (a = 0, 1, 2: a 24-bit value)
 * component a of the particle is  fminf(fmaxf(((float)C_a + (float)r_a * 2^-24f) * h, h), (float)n_a * h - h)  -- a float sum,
 * a float product (the sum can round up to C_a + 1: a particle may sit ON the upper face of its cell), then the trace's clamp,
 * which can move the last bit on the outermost cells only.  The same cell and sample get the same jitter whatever the box.
 * No state, no library generator.  FL_ERR_BAD_ARGUMENT: a NULL pointer with a non-empty box, per_cell < 1, a count
 * above 2^31 - 1, a dimension below 5. */
int gpu_seed_particles(float *px, float *py, float *pz, int i0, int i1, int j0, int j1, int k0, int k1, int per_cell,
                       unsigned seed, float h, int ni, int nj, int nk);
/* gpu_sort_particles: counting sort of the particles (px, py, pz, id) into (qx, qy, qz, qid) by brick key: bricks of 4 x 4 x 4
 * cells, key = bx + nbx * (by + nby * bz) with b_a = clamp(floor(p_a / h), 0, n_a - 1) >> 2 (IEEE division) and
 * nb_a = (n_a + 3) / 4.  Histogram (integer atomics), exclusive scan, scatter (slots handed out by integer atomics): the
 * order INSIDE a brick is whatever the atomics made it and may differ from run to run; positions and ids travel together.
 * id == NULL stands for the identity (particle a has id a).  The key table (nbx nby nbz + 1 unsigned) lives in the library's
 * scratch.  FL_ERR_BAD_ARGUMENT: a NULL pointer other than id, n < 0 or n >= 2^31, an output overlapping an input or another
 * output, a dimension below 1 or beyond the size limits. */
int gpu_sort_particles(const float *px, const float *py, const float *pz, const unsigned *id,
                       float *qx, float *qy, float *qz, unsigned *qid, long n, float h, int ni, int nj, int nk);

#ifdef __cplusplus
}
#endif
#endif /* BIMOCQ_GPU_H */
