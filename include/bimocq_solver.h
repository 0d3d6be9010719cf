/*
 * bimocq_solver.h -- C view of the C++ host solver (gpufluidsimulation_amd/csrc/host/).
 *
 * The host solver keeps the reference's BimocqGPUSolver surface
 * (reference: src/bimocq3D/BimocqGPUSolver.h:27-56): construct with (nx, ny, nz, L, viscosity,
 * blend, scheme), setSmoke, advance(framenum, dt), outputResult(frame, path).  It is plain C++
 * that calls nothing but the C-ABI of include/bimocq_gpu.h; this header lets non-C++ hosts
 * (the Python tests and bench.py via ctypes) drive the same object.
 */
#ifndef BIMOCQ_SOLVER_H
#define BIMOCQ_SOLVER_H

#include "bimocq_gpu.h"        /* bq_boundary */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bq_solver bq_solver;

/* one spherical smoke source; the reference hard-codes two of these in
 * BimocqGPUSolver::emitSmoke (BimocqGPUSolver.cpp:387-390) */
typedef struct bq_emitter {
    float cx, cy, cz, radius, density, temperature, emiter;
    int   emit_frames;                  /* active while framenum < emit_frames */
} bq_emitter;

/* enum Scheme, BimocqSolver.h:29.  The reference's GPU solver implements BIMOCQ and MAC_REFLECTION
 * (BimocqGPUSolver.cpp:112-122); MACCORMACK is its CPU solver's advanceMacCormack (BimocqSolver.cpp:282-364) on device
 * buffers.  Both MacCormack schemes run with the corrected limiter (gpu_clamp_extrema).  SEMILAG
 * (1) is not built: bq_solver_create returns NULL for it. */
enum { BQ_SCHEME_BIMOCQ = 0, BQ_SCHEME_MACCORMACK = 2, BQ_SCHEME_MAC_REFLECTION = 3 };
enum {
    BQ_PROJECTION_JACOBI = 0,           /* the `#if 0` branch of BimocqGPUSolver::projection (:408-417); iters = sweeps      */
    BQ_PROJECTION_MGCG = 1,             /* the `#else` branch (:443-446): fp64 multigrid-CG; iters = outer iterations (50)  */
    BQ_PROJECTION_PCG = 2               /* fp64 flexible PCG on the masked system to a tolerance, the
                                           CPU solver's semantics (BimocqSolver.cpp:1269); iters = most CG updates (1000).
                                           One GPU: refused (FL_ERR_UNSUPPORTED) on z-slab ranks and when the operator
                                           library has no PCG operators */
};

/* which-ids for bq_solver_download */
enum {
    BQ_F_RHO = 0, BQ_F_T, BQ_F_U, BQ_F_V, BQ_F_W, BQ_F_UINIT, BQ_F_VINIT, BQ_F_WINIT,
    BQ_F_RHOINIT, BQ_F_TINIT, BQ_F_FWDX, BQ_F_FWDY, BQ_F_FWDZ, BQ_F_BACKX, BQ_F_BACKY, BQ_F_BACKZ,
    BQ_F_P, BQ_F_DIV, BQ_F_COUNT
};

/* BimocqGPUSolver::BimocqGPUSolver (BimocqGPUSolver.cpp:3-106).  device: HIP device index.
 * Returns NULL on failure (see fl_last_error_string()). */
bq_solver *bq_solver_create(int device, int nx, int ny, int nz, float L,
                            float viscosity, float blend, int scheme);
/* z-slab rank of a multi-GPU run (one process per GPU): nz is the GLOBAL plane count, rank r of
 * nranks owns planes [r*nz/nranks, (r+1)*nz/nranks) and keeps `ghost` ghost planes per side
 * (>= CFL travel + 3; 8 covers CFL <= 5).  Requires fl_comm_init() first when nranks > 1. */
bq_solver *bq_solver_create_slab(int device, int nx, int ny, int nz, float L, float viscosity, float blend,
                                 int scheme, int rank, int nranks, int ghost);
void  bq_solver_slab_info(const bq_solver *s, int out[8]);
void  bq_solver_destroy(bq_solver *s);
/* setSmoke (BimocqGPUSolver.cpp:529-534): alpha = drop (rho coefficient), beta = rise (T) */
void  bq_solver_set_smoke(bq_solver *s, float drop, float rise, const bq_emitter *emitters, int n);
/* projection variant + parameters (compile-time `#if` in the reference, :408-466) */
void  bq_solver_set_projection(bq_solver *s, int kind, int iters, float halfrdx);
/* solver options: BQ_OPT_KEEP_DMC_BORDER (default 0 = reference behaviour: the backward map's border
 * nodes are zeroed by the DMC update; 1 = they keep their values, see csrc/host/mapping.hpp) */
enum {
    BQ_OPT_KEEP_DMC_BORDER = 1,
    /* 0 (default): both map sets are re-initialised every frame, as the reference's GPU solver does (`if (1)`,
     * BimocqGPUSolver.cpp:218-229).  1: distortion-driven re-initialisation with the CPU solver's rules
     * (BimocqSolver.cpp:165-229): velocity maps when their round-trip error exceeds 1 step-travel or after 10
     * frames, scalar maps above 5 or after 30 frames; the scalar snapshots are taken before the sources act
     * so that emission reaches DensityInit through the accumulation.  Set before the first advance().
     * z-slab ranks (round 3): maps that live for many steps must still fit the ghost zone, see BQ_OPT_REINIT_MAX_TRAVEL. */
    BQ_OPT_REINIT_POLICY = 2,
    /* 0 (default): state that nothing can read is not computed -- with blend == 1 and a re-initialisation every
     * frame the *Prev fields are never sampled, so the pre-reinit accumulation into *Init (which only survives as
     * *Prev) and the force delta feeding it are skipped.  1: execute the reference's full sequence.  Every field
     * reachable through this API, and every dump, is identical either way. */
    BQ_OPT_FULL_STATE = 3,
    /* 1 (default): the clears and copies the reference issues around the map operators (GPU_Advection.h:464-526,
     * GPU_kernel.cu:656-658) are done by the kernels themselves (FL_OPT_FUSED_HOUSEKEEPING of the operator ABI):
     * same values in every buffer, ~25 fewer memset/memcpy launches per step.  0: separate launches. */
    BQ_OPT_FUSED_HOUSEKEEPING = 4,
    /* z-slab ranks, 1 (default): the ghost-plane exchange in front of a map operator runs on the halo stream while the
     * operator works on the planes that cannot reach a ghost plane; the planes at both ends follow the exchange.
     * 0: exchange, then the whole operator.  Same values either way. */
    BQ_OPT_OVERLAP_EXCHANGES = 5,
    /* z-slab ranks, 0 (default): a BLOCKING ghost-plane refresh (the ones no operator hides: the projection's velocity
     * refresh, the limiter's) moves all G ghost planes, whatever depth was asked for -- the deeper validity spares later
     * operators their own exchange.  1: it moves only the planes asked for (3 instead of 24 MB per velocity refresh at
     * 512^2 planes); the operators that need more fetch it in their own, overlapped exchange.  Same values either way;
     * which is faster depends on the links (host-staged transport: 0).  2: the overlapped exchanges in front of the map
     * operators move only the planes the operator can reach as well (reach 4-5 of G = 8 planes at CFL 1-2). */
    BQ_OPT_SHALLOW_BLOCKING_EXCHANGE = 6,
    /* z-slab ranks with at least 2 G + 8 owned planes, 1 (default): the last two fused pairs of every pressure chunk that
     * another chunk follows run on the planes next to the slab ends first, the exchange for the next chunk starts there,
     * and their interiors (and the next chunk's first interior) run while it travels -- three launches hide the 8-plane
     * exchange instead of one, at two more short launches per chunk (+ 2 % compute on a 512 x 512 x 64 rank).  0: the
     * exchange starts when the chunk is complete.  Same values either way.  2: ... and with closed walls too -- the walled
     * chunk of a rank with at least 2 G + 8 + 2 ((G - 1) mod 3) + 2 owned planes and G >= 7 gives up the sweeps behind its last
     * triple (G = 8: 7 sweeps per exchange) and runs its last two triples ends first.  With 1 a walled chunk keeps the
     * plain order: on a rank whose exchange costs nothing the ends-first order is slower there. */
    BQ_OPT_JACOBI_ENDS_FIRST = 7,
    /* 1: advanceBimocq brackets its phases with events on the compute stream (read with bq_solver_phase_ms): where the
     * step's time goes on this rank, the waits for ghost planes included in the phase that needs them.  Default 0. */
    BQ_OPT_PROFILE_PHASES = 8,
    /* policy 1 only.  T > 0: after every map update the z-travel of both maps of a set is measured (gpu_map_travel_z: max
     * |map_z - z| / h, all-reduced over the ranks) and replaces the running sum of CFL travels as the set's displacement
     * bound; a set whose bound + this step's CFL travel + the two cells of the sampling footprint exceeds T is
     * re-initialised at the end of the step even though the CPU solver's thresholds would let it live on.  z-slab ranks:
     * default and maximum T = the ghost depth G (what their ghost planes can serve); single GPU: default 0 (no such rule) --
     * give both the same T and they re-initialise on the same frames and produce the same fields
     * (tests/test_slab_multirank.py).  bq_solver_reinit_counts(s, 2) counts the re-initialisations this rule caused. */
    BQ_OPT_REINIT_MAX_TRAVEL = 9,
    /* z-slab ranks, G = 8, 1 (default): the six sweeps of a pressure chunk that follow its overlapped first pair run as TWO
     * fused triples (gpu_jacobi_sweep_triple_ranges: the LDS-exchanged three-sweep kernels on plane ranges) instead of three
     * pairs -- with BQ_OPT_JACOBI_ENDS_FIRST both triples do the planes next to the slab ends first, the exchange for the next
     * chunk starts there and the two interiors (and the next chunk's first interior) hide it.  Where the kernels do not apply
     * (rows wider than 512 floats, ...) and with 0 the pairs run.  Same values either way. */
    BQ_OPT_JACOBI_TRIPLES = 10,
    /* z-slab ranks with the multigrid-CG projection, 1 (default): the grid's fine levels are SHARED between the ranks
     * (gpu_multi_grid_conjugate_gradient_slab: owned + ghost planes per level, neighbour exchanges, all-gathered block dot
     * products; thin levels gathered and solved replicated) wherever gpu_mgcg_slab_supported says the decomposition allows it
     * -- no global fp64 array on any rank, the solve scales with the rank count.  0, and any decomposition it does not cover:
     * the replicated solve of round 3 (every rank assembles the whole velocity and solves the whole grid).  Same bits.
     * bq_solver_get_option returns 2 once a projection has taken the shared path. */
    BQ_OPT_MGCG_SHARED = 11,
    /* one GPU, 1: updateMapping launches the forward-map update on the library's auxiliary stream beside the backward map's DMC
     * sub-steps (fl_aux_*: disjoint arrays) instead of after them.  Same values.  Default 0: measured at 256^3 and 128^3, the
     * two kernels each fill the chip and gain nothing from running side by side (11.14-11.19 against 11.10-11.15 ms per step). */
    BQ_OPT_CONCURRENT_MAPS = 12,
    /* z-slab ranks, blend coefficient != 1, reference-faithful map border (BQ_OPT_KEEP_DMC_BORDER = 0), 1 (default): at every
     * re-initialisation each rank assembles whole-grid copies of the *Prev fields (the only time they change; one message per
     * peer and field) and the two-level advection samples those (gpu_advect_vel_double_global, include/bimocq_gpu.h): its second
     * look-up lands anywhere between the origin and the node once it meets the zeroed border cells of the previous backward
     * map, which no ghost zone or sheet bounds.  Bit-identical to one GPU.  0: local *Prev fields with ghost planes only --
     * exact as long as no node within a cell of the outermost window nodes is carried more than 3/4 of a cell towards a wall
     * between two re-initialisations (reads outside the slab return 0 otherwise).  get: 2 = copies are in use.  Costs five
     * whole-grid float arrays per rank. */
    BQ_OPT_WHOLE_GRID_PREV = 13,
    /* one GPU, power-of-two spacing, 1 (default): the map updates tell their kernels what the solver knows -- that getCFL()
     * has just found the velocity finite, and that a map still is the identity gpu_init_maps wrote (always at the first DMC
     * sub-step and the forward update after a re-initialisation) -- through gpu_solve_backwardDMC_hint / gpu_solve_forward_hint
     * (include/bimocq_gpu.h).  The kernels then look the velocity up at grid nodes as the mean of two values and compute
     * identity-map corners instead of loading them.  Same bits.  0: the reference entry points, for A/B runs. */
    BQ_OPT_NODE_LOOKUPS = 14,
    /* The MacCormack advection of a field (schemes MACCORMACK and MAC_REFLECTION) after its first semi-Lagrangian pass: 0 =
     * the reference's launches (clear + second pass, two adds, the limiter, a copy); 1 (default) = one gpu_maccormack launch
     * (include/bimocq_gpu.h) in the MACCORMACK scheme, whose result becomes the field by a buffer swap; 2 = in MAC_REFLECTION
     * too.  With 0 and 1 the reflection scheme issues the launches it always did.  Same values in every field either way.
     * An operator library without gpu_maccormack runs the separate launches whatever the value. */
    BQ_OPT_FUSED_MACCORMACK = 15,
    /* N > 0: after every N-th advance() the flow diagnostics (gpu_flow_stats, include/bimocq_gpu.h) of the fields the step
     * left are enqueued into the next row of a device ring of 1024 rows -- in stream order, no host sync; read them with
     * bq_solver_diagnostics_history.  0 (default): nothing is launched or allocated and a step is exactly what it was.
     * Refused with FL_ERR_UNSUPPORTED on an operator library without gpu_flow_stats, FL_ERR_BAD_ARGUMENT for N < 0. */
    BQ_OPT_DIAGNOSTICS_EVERY = 16,
    /* N > 0: after every N-th advance() the tracers are re-sorted by 4 x 4 x 4-cell brick (gpu_sort_particles) so that
     * neighbouring lanes of the trace read neighbouring cells again once the flow has mixed the set; an id array and a second
     * set of position arrays then exist.  0 (default, by measurement: DESIGN.md section 22): never, and neither exists.
     * Everything public is in id order and the same bits either way.  FL_ERR_BAD_ARGUMENT for N < 0, FL_ERR_UNSUPPORTED for
     * N > 0 where tracers are (z-slab ranks, an operator library without the tracer operators). */
    BQ_OPT_TRACER_SORT_EVERY = 17,
    /* N > 0: on every N-th advance() (advance() calls so far % N == 0, as for BQ_OPT_DIAGNOSTICS_EVERY) each projection of the
     * step that ran with a non-empty obstacle list is followed, in stream order and with no host sync, by one
     * gpu_obstacle_loads call (include/bimocq_gpu.h) on the pressure that projection produced, the flags it used and the list
     * at its current centres, into a slot of a device ring of 1024 rows of two slots; read them with
     * bq_solver_obstacle_loads / _history.  A sampled step with an empty list records a row with N = 0 and launches nothing.
     * 0 (default): nothing is launched or allocated and a step is exactly what it was.  Refused, the previous value staying
     * in place: N < 0 with FL_ERR_BAD_ARGUMENT; N > 0 on z-slab ranks or on an operator library without gpu_obstacle_loads
     * with FL_ERR_UNSUPPORTED. */
    BQ_OPT_OBSTACLE_LOADS = 18
};
/* BQ_OPT_PROFILE_PHASES: milliseconds per phase summed over the steps since the last reset -- map update (DMC + RK3,
 * BimocqGPUSolver.cpp:136-139), advection with error compensation (:143-145), sources and forces (:157-177), projection
 * (:179-193), accumulation and re-initialisation (:195-229).  Returns the number of steps summed.  Blocking. */
enum { BQ_PHASE_MAPS = 0, BQ_PHASE_ADVECT, BQ_PHASE_FORCES, BQ_PHASE_PROJECTION, BQ_PHASE_ACCUMULATE, BQ_PHASE_COUNT };
long long bq_solver_phase_ms(bq_solver *s, double ms[BQ_PHASE_COUNT], int reset);
/* after a step: re-initialisation counts (which: 0 velocity maps, 1 scalar maps, 2 those forced by BQ_OPT_REINIT_MAX_TRAVEL) and the distortions the
 * last step measured (policy 1; 0 otherwise) */
int   bq_solver_reinit_counts(const bq_solver *s, int which);
float bq_solver_last_distortion(const bq_solver *s, int which);
void  bq_solver_set_option(bq_solver *s, int option, int value);
/* current value of an option above (-1: unknown option) */
int   bq_solver_get_option(const bq_solver *s, int option);
/* advance (BimocqGPUSolver.cpp:108-127) */
void  bq_solver_advance(bq_solver *s, int framenum, float dt);
/* outputResult (BimocqGPUSolver.cpp:536-543): D2H of rho,u,v,w and a sparse density dump
 * <path>/density_render_%04d.bqd for frame+1 (writeVDB's contract, utils/volumeMeshTools.h:33-60,
 * in a dependency-free container).  path == NULL: only refresh the host copies.  Returns the
 * number of voxels written (|rho| > 1e-4) or -1 on error. */
long  bq_solver_output_result(bq_solver *s, unsigned frame, const char *path);
/* copy one device field to host (blocking).  Returns its element count (0 on bad id); copies
 * min(count, capacity) elements when host != NULL. */
long  bq_solver_download(bq_solver *s, int which, float *host, long capacity);
/* tempResult of the last multigrid-CG projection (4096 doubles: CG sums at [0..2*iters+2], largest positive
 * residual per outer iteration at [2000..2000+iters] -- what the reference prints, BimocqGPUSolver.cpp:447-452).
 * Returns the count (0 before the first MGCG projection); copies min(count, capacity). */
long  bq_solver_mg_history(const bq_solver *s, double *host, long capacity);
/* BQ_PROJECTION_PCG: relative tolerance of the stopping rule max|r| <= tol * max|b| (default 1e-6); a tol that is not
 * finite or lies outside (0, 1) is refused (FL_ERR_BAD_ARGUMENT, the tolerance is kept).  Returns 0 on success. */
int   bq_solver_set_pcg_tolerance(bq_solver *s, double tol);
/* out = {iterations, final max|r|, max|b|, stop reason (BQ_PCG_CONVERGED / _ITER_LIMIT / _BREAKDOWN) of the last PCG
 * projection, PCG projections so far, those of them that did not converge}; returns 0 before the first one, else 1 */
int   bq_solver_pcg_stats(const bq_solver *s, double out[6]);
/* the fp64 pressure of the last PCG projection (nz * ny * nx, x fastest); returns the count (0 before the first one) and
 * copies min(count, capacity) */
long  bq_solver_pcg_pressure(bq_solver *s, double *host, long capacity);
/* The dump without stalling the simulation: asynchronous download on a third stream + a writer thread; the
 * file is the one bq_solver_output_result would write.  At most one dump in flight (a second call waits for
 * the first).  _wait returns the voxel count of the last asynchronous dump, or -1. */
int   bq_solver_output_result_async(bq_solver *s, unsigned frame, const char *path);
long  bq_solver_output_wait(bq_solver *s);
/* Solid obstacles (setBoundary / updateBoundary, BimocqSolver.cpp:936-1064).  set_boundary
 * replaces the whole list (n = 0 removes every obstacle; at most BQ_MAX_BOUNDARIES) and builds the cell flags at the
 * given centres; update_boundary moves every centre by v * dt (Boundary::update) and rebuilds them.  One GPU, with the
 * Jacobi projection or BQ_PROJECTION_PCG (either call order): z-slab ranks and BQ_PROJECTION_MGCG are refused through
 * fl_last_error.  Returns 0 on success.
 * download_solid copies min(cells, capacity) flags (1 = obstacle) and returns the cell count. */
int   bq_solver_set_boundary(bq_solver *s, const bq_boundary *b, int n);
/* set_boundary for lists that may hold level sets (shape BQ_SHAPE_LEVELSET; DESIGN.md section 14, "Level sets"): ls is
 * an array of n descriptors, ls[o] read only where b[o].shape == BQ_SHAPE_LEVELSET, whose phi are HOST arrays.  Every grid
 * is copied into one device allocation (at most 256 MiB in all): the caller may free its arrays after the call.  The
 * level set moves with its entry's centre (update_boundary); the grid is never uploaded again.  The refusals of
 * set_boundary apply, plus bad descriptors and a library without the level-set operators.  Any failure leaves no
 * obstacles.  Returns 0 on success. */
int   bq_solver_set_boundary_levelsets(bq_solver *s, const bq_boundary *b, const bq_levelset *ls, int n);
int   bq_solver_update_boundary(bq_solver *s, int framenum, float dt);
/* set_boundary_levelsets for lists whose entries may carry a rigid pose (an extension, the reference's
 * obstacles only translate): pose is an array of n bq_pose (orientation quaternion, any non-zero scale, and angular velocity
 * about the entry's centre); ls and pose may each be NULL.  A box or level set with (qx, qy, qz) != 0 is ORIENTED: it is
 * classified in its body frame.  An entry with a non-zero angular velocity SPINS: its solid faces take v + omega x (p - c),
 * and update_boundary turns its orientation by |omega| dt about omega (a double quaternion kept by the solver, so nothing
 * drifts).  A list without an oriented or spinning entry issues exactly the launches of set_boundary_levelsets.
 * set_boundary and set_boundary_levelsets keep their meaning: no rotation.  The refusals of set_boundary_levelsets apply,
 * plus: a non-finite component of a pose or a quaternion of squared norm 0 or not finite (FL_ERR_BAD_ARGUMENT), and an
 * oriented or spinning entry on a library without the pose operators (FL_ERR_UNSUPPORTED).  z-slab ranks and
 * BQ_PROJECTION_MGCG are refused as for every obstacle; orientation of sources and a time-varying angular velocity are not
 * supported (callers set the list again, as for v).  Any failure leaves no obstacles.  Returns 0 on success.
 * boundary_pose: centre (3), orientation quaternion w, x, y, z (4), angular velocity (3) of entry i into out; returns 0,
 * or -1 for a bad index. */
int   bq_solver_set_boundary_poses(bq_solver *s, const bq_boundary *b, const bq_levelset *ls, const bq_pose *pose, int n);
int   bq_solver_boundary_pose(const bq_solver *s, int i, double out[10]);
/* Closed domain walls (the reference's container, BimocqSolver.cpp:938-948): `walls` is a sum of
 * BQ_WALL_* bits (include/bimocq_gpu.h), BQ_WALLS_NONE (default: every side open, p = 0 in the border cells) or
 * BQ_WALLS_REFERENCE_BOX (every side closed but +y).  Border cells of a closed side are solid cells with velocity 0 for
 * the projection; no band, no blend, no density clear, and download_solid keeps reporting obstacle cells only.  One GPU
 * with the Jacobi projection or BQ_PROJECTION_PCG, with or without obstacles, or z-slab ranks with the Jacobi projection
 * and no obstacles (every rank sets the same mask; BQ_WALL_ZLO / _ZHI are the first / last GLOBAL plane, a rank in the
 * middle has x and y walls only; every owned plane equals the one-GPU walled run bit for bit); every scheme, in any call
 * order.  Refused through fl_last_error, the previous setting staying in place: BQ_PROJECTION_MGCG (also
 * set_projection(MGCG) while walls are on), an operator library without the wall operators, and on a z-slab rank one
 * without gpu_jacobi_sweep_masked_walls_range / _triple_ranges, with FL_ERR_UNSUPPORTED; bits outside 0 .. 63
 * and all six sides closed (the pressure needs an open side as its reference) with FL_ERR_BAD_ARGUMENT.
 * Returns 0 on success; get_walls returns the setting in force. */
int   bq_solver_set_walls(bq_solver *s, int walls);
int   bq_solver_get_walls(bq_solver *s);
/* Vorticity confinement (an extension: the reference's only forces are buoyancy and viscosity): with a
 * coefficient eps > 0 every step adds dt eps h (N x omega) to the velocity by one gpu_vorticity_confinement call
 * (include/bimocq_gpu.h has the contract) right after the buoyancy, over the same dt and before the viscous diffusion: once
 * per step in BiMocq and MacCormack, in both half steps of the reflection scheme over dt / 2 each.  eps is dimensionless
 * (the force scales with h); useful values lie between 0.05 and 1.  The operator sees neither obstacles nor walls: the shear
 * at a solid surface and at the domain border counts as vorticity, so the force near a solid is not physically filtered (the
 * projections overwrite the solid and wall faces themselves).  Default 0: a step then issues exactly the launches it issues
 * without this feature.  Refused through fl_last_error, the previous coefficient staying in place: a negative or
 * non-finite eps with FL_ERR_BAD_ARGUMENT; eps > 0 on z-slab ranks or on an operator library without
 * gpu_vorticity_confinement with FL_ERR_UNSUPPORTED.  set returns FL_OK or that error; get the coefficient in force. */
int   bq_solver_set_vorticity_confinement(bq_solver *s, float eps);
float bq_solver_get_vorticity_confinement(const bq_solver *s);
/* Shaped, moving smoke sources (Emitter / emitSmoke of the CPU solver, BimocqSolver.h:31-59, BimocqSolver.cpp:696-813;
 * DESIGN.md section 16): a second list next to the emitters of set_smoke, which keep their launches and their bits.
 * set_sources replaces the list (n = 0 releases list and grids; at most BQ_MAX_SOURCES).  ls is an array of n
 * descriptors, ls[o] read only where src[o].shape.shape == BQ_SHAPE_LEVELSET (NULL allowed when no entry is one), whose
 * phi are HOST arrays: every grid is copied into one device allocation of the sources' own (at most 256 MiB in all) and
 * never uploaded again.  At every emission point of a step (once per advance in both schemes, after the emitters) every
 * source, active or not, first moves by shape.v * dt per component in float; then the sources with framenum <
 * emit_frames act in list order (gpu_emit_sources).  Allowed on z-slab ranks, with every projection kind, with and
 * without obstacles.  Refused with FL_ERR_BAD_ARGUMENT: more than 16 entries, an unknown shape or flag, a non-finite
 * field, a non-positive extent of an analytic shape, a negative emit_frames, a level-set entry without descriptors, a
 * bad descriptor, the cap; with FL_ERR_UNSUPPORTED: an operator library without gpu_emit_sources.  Any failure leaves
 * no sources.  Returns 0 on success.
 * source_position: the current position of source i into out; returns 0 on success, -1 for a bad index. */
int   bq_solver_set_sources(bq_solver *s, const bq_source *src, const bq_levelset *ls, int n);
int   bq_solver_source_position(const bq_solver *s, int i, float out[3]);
long  bq_solver_download_solid(bq_solver *s, unsigned char *host, long capacity);
/* Flow diagnostics of the current fields, from the raw sums S0..S9 of gpu_flow_stats (cell-centred
 * velocity, h = L / nx; solid cells count as fluid):
 *   KINETIC = 0.5 h^3 S0   ENSTROPHY = 0.5 h^3 S1   DIV_L2 = sqrt(h^3 S2)   DIV_MAX = S3   RHO_SUM = S4 (raw: the sum of the cell
 *   values)   CENTROID_X/Y/Z = h S5..7 / S4 (0 when S4 is 0)   T_SUM = S8   VORT_MAX = S9   STEP = advance() calls so far.
 * Blocking.  On z-slab ranks collective, and every rank gets the values of the whole grid.  Returns FL_OK, or the error
 * latched (FL_ERR_UNSUPPORTED on an operator library without gpu_flow_stats). */
enum { BQ_DIAG_KINETIC = 0, BQ_DIAG_ENSTROPHY, BQ_DIAG_DIV_L2, BQ_DIAG_DIV_MAX, BQ_DIAG_RHO_SUM, BQ_DIAG_CENTROID_X,
       BQ_DIAG_CENTROID_Y, BQ_DIAG_CENTROID_Z, BQ_DIAG_T_SUM, BQ_DIAG_VORT_MAX, BQ_DIAG_STEP, BQ_DIAG_COUNT };
int   bq_solver_diagnostics(bq_solver *s, double out[BQ_DIAG_COUNT]);
/* BQ_OPT_DIAGNOSTICS_EVERY: the retained samples (at most the last 1024), oldest first, as rows of BQ_DIAG_COUNT doubles in
 * bq_solver_diagnostics' layout with STEP = the step the sample followed.  Blocking.  Returns the number of retained rows
 * and copies min(rows, capacity_rows) of them when host != NULL. */
long  bq_solver_diagnostics_history(bq_solver *s, double *host, long capacity_rows);
/* Per-obstacle pressure loads (BQ_OPT_OBSTACLE_LOADS): the force and the torque about its centre that
 * the pressure of a step's projection(s) puts on every obstacle, from the raw sums P, M, FACES, PSUM of gpu_obstacle_loads.
 * BiMocq and MacCormack project once per step and fill slot 0 of a row; the reflection scheme projects twice and fills slot 0
 * at its first projection and slot 1 at its second.  The slot weights (w0, w1) are (1, 0) for the one-projection schemes and
 * (2, 1) for the reflection scheme: its reflected velocity 2 u_projected - u_unprojected applies the first projection's
 * pressure gradient twice, so the fluid's net pressure momentum change over the step is 2 J1 + J2.
 * A row is BQ_OLOAD_ROW doubles, computed on the host in double at read time: STEP (advance() calls so far when it was
 * sampled), DT, N (obstacles), then per obstacle o < N the BQ_OLOAD_COUNT values
 *   FX, FY, FZ = halfrdx h^3 / dt (w0 P0 + w1 P1)        TX, TY, TZ likewise from M (about the centre the projection used)
 *   AREA = h^2 FACES of the step's last projection        P_MEAN = halfrdx h / dt PSUM / FACES of it (0 without faces)
 * (the six loads and P_MEAN are 0 when dt == 0); the entries of obstacles o >= N are 0.  The values survive a later
 * set_boundary: a row keeps the N, halfrdx and weights it was sampled with.  "Last projection": slot 1 when w1 != 0.
 * Limits: pressure loads only, no viscous traction; halfrdx = 1 is the physical projection strength, the default 0.5
 * reports what that projection actually applied; the Jacobi pressure is as converged as its sweeps make it, BQ_PROJECTION_PCG
 * is the converged one; one GPU.
 * obstacle_loads: the newest sampled row; blocking; 1, 0 when none has been sampled yet, -1 on error.
 * obstacle_loads_history: the retained rows (at most the last 1024), oldest first; blocking; returns their number and copies
 * min(rows, capacity_rows) of them when host != NULL.
 * obstacle_loads_raw (for tests and tools): the two raw slots (BQ_MAX_BOUNDARIES x BQ_LOAD_COUNT doubles each; a slot the
 * step did not fill reads 0) and the weights of the row `back` rows before the newest; returns its STEP, or -1 when there
 * is no such row or on error.  Blocking. */
enum { BQ_OLOAD_STEP = 0, BQ_OLOAD_DT, BQ_OLOAD_N, BQ_OLOAD_HEADER };
enum { BQ_OLOAD_FX = 0, BQ_OLOAD_FY, BQ_OLOAD_FZ, BQ_OLOAD_TX, BQ_OLOAD_TY, BQ_OLOAD_TZ, BQ_OLOAD_AREA, BQ_OLOAD_P_MEAN, BQ_OLOAD_COUNT };
enum { BQ_OLOAD_ROW = 3 + BQ_MAX_BOUNDARIES * BQ_OLOAD_COUNT };
int   bq_solver_obstacle_loads(bq_solver *s, double row[BQ_OLOAD_ROW]);
long  bq_solver_obstacle_loads_history(bq_solver *s, double *host, long capacity_rows);
long  bq_solver_obstacle_loads_raw(bq_solver *s, long back, double slots[2 * 128], double weights[2]);
/* the cell-centred vorticity magnitude |omega| of the LOCAL planes (nk_local * ny * nx, x fastest; border cells 0) through a
 * scratch field that is allocated on the first call.  Returns the element count (host == NULL: only that) and copies
 * min(count, capacity); -1 on error.  Blocking. */
long  bq_solver_vorticity(bq_solver *s, float *host, long capacity);
/* |omega| into <path>/vorticity_render_%04u.bqd for frame + 1 (z-slab ranks: .k%05d.bqd with their owned planes) in the
 * container of bq_solver_output_result: grid "vorticity", voxels whose value exceeds `threshold`.  Returns the number of
 * voxels written or -1. */
long  bq_solver_output_vorticity(bq_solver *s, unsigned frame, const char *path, float threshold);
/* Shadowed density preview (the contract of gpu_render_density in include/bimocq_gpu.h): an orthographic
 * emission-absorption image of the current density along a grid axis, self-shadowed by one directional light.  view and
 * light are direction codes 0..5 = +x, -x, +y, -y, +z, -z (the direction a ray travels: from the eye into the volume, from
 * the light into the volume); light = -1: no shadowing.  The image is W x H, columns fastest: view +-z: nx x ny (x, y),
 * +-y: nx x nz (x, z), +-x: ny x nz (y, z), nz the GLOBAL plane count.  The shadow field and the image buffer are allocated
 * on the first call; advance() launches nothing for this.  On z-slab ranks the calls are collective and every rank gets the
 * whole image.  FL_ERR_UNSUPPORTED on an operator library without gpu_render_density.
 * bq_solver_render_size: W and H of a view; FL_OK or FL_ERR_BAD_ARGUMENT. */
int   bq_solver_render_size(bq_solver *s, int view, int *w, int *h);
/* radiance = (float)(Cfix * 2^-32) and transmittance = att(Afix) per pixel.  Blocking.  Returns W * H and copies
 * min(W * H, capacity) pixels into each non-NULL array; with both NULL it only returns the count; -1 on error. */
long  bq_solver_render(bq_solver *s, int view, int light, float sigma, float albedo, float ambient, float *radiance,
                       float *transmittance, long capacity);
/* the image into <path>/preview_%04u.pgm for frame + 1: binary 8-bit P5, a pixel is clamp(radiance + transmittance *
 * background, 0, 1) (product and sum in double) times 255, rounded to nearest (ties to even); rows are written highest index
 * first, so +y or +z points up.  On z-slab ranks only rank 0 writes (the others return 0).  Returns the bytes written or -1. */
long  bq_solver_output_preview(bq_solver *s, unsigned frame, const char *path, int view, int light, float sigma, float albedo,
                               float ambient, float background);
/* The preview with the solid obstacles drawn (the contract of gpu_render_density_solids): opaque bodies
 * with flat shading solid_albedo * s + solid_ambient that cast full shadows; solid_albedo, solid_ambient finite, >= 0, sum <= 4.
 * hit receives per pixel the tag o + 1 of the first obstacle cell on the view ray (o: index in the boundary list), 0 where
 * there is none; a hit pixel's transmittance is 0, so the background does not shine through a body.  Returns W * H and copies
 * min(W * H, capacity) pixels into each non-NULL array; all three NULL: only the count; -1 on error.  With an empty boundary
 * list and on z-slab ranks (no obstacles there) this is bq_solver_render and hit = 0.  The three-plane image buffer is
 * allocated on the first call that draws obstacles.  FL_ERR_UNSUPPORTED with obstacles on an operator library without
 * gpu_render_density_solids.  Domain walls are not drawn. */
long  bq_solver_render_solids(bq_solver *s, int view, int light, float sigma, float albedo, float ambient, float solid_albedo,
                              float solid_ambient, float *radiance, float *transmittance, unsigned char *hit, long capacity);
/* bq_solver_output_preview with that image: the same file, the same pixel formula */
long  bq_solver_output_preview_solids(bq_solver *s, unsigned frame, const char *path, int view, int light, float sigma, float albedo,
                                      float ambient, float solid_albedo, float solid_ambient, float background);
/* Passive tracer particles (the operators' contracts are in include/bimocq_gpu.h).  The solver owns
 * the positions on the device.  In every scheme, while the count is non-zero, advance() moves each tracer over the whole dt
 * through the velocity the step STARTS with, in sub-steps of that step's getCFL() value, clamped to [h, (n - 1) h]: the
 * trace the forward map's nodes take (gpu_trace_particles / gpu_solve_forward), on the compute stream with no host sync,
 * before anything writes the velocity.  A tracer placed on a grid node therefore equals, bit for bit, the forward map's entry
 * of that node for as long as the map is not re-initialised.  Tracers are passive: they follow the velocity as it is, inside
 * obstacles and walls too.  With no tracers advance() launches and allocates nothing for this.  A tracer's id is its index in
 * the set as given (set_tracers) or appended (seed_tracers); everything below is in id order, whatever
 * BQ_OPT_TRACER_SORT_EVERY has done to the stored order.  FL_ERR_UNSUPPORTED: z-slab ranks (migration of particles between
 * ranks is deliberately not built) and an operator library without gpu_trace_particles.
 * set_tracers: replaces the set with n positions (x, y, z interleaved, float32); n = 0 releases everything.  A non-finite
 * component is refused with FL_ERR_BAD_ARGUMENT before anything is uploaded; finite positions are clamped componentwise into
 * the trace's box; at most BQ_MAX_TRACERS.  Any failure leaves no tracers.  Returns FL_OK or the error. */
#define BQ_MAX_TRACERS (1L << 26)
int   bq_solver_set_tracers(bq_solver *s, const float *xyz, long n);
/* appends per_cell jittered tracers in every cell of the half-open cell box [lo, hi) intersected with the cells 1 .. n - 2
 * (gpu_seed_particles: k outermost, then j, i, the sample; the same cell and sample get the same jitter whatever the box).
 * Ids continue from the current count.  Returns the number added -- (hi' - lo') products times per_cell -- or -1. */
long  bq_solver_seed_tracers(bq_solver *s, const int lo[3], const int hi[3], int per_cell, unsigned seed);
long  bq_solver_tracer_count(const bq_solver *s);
/* positions in id order: copies min(count, capacity) triples when xyz != NULL; returns the count or -1.  Blocking. */
long  bq_solver_tracers(bq_solver *s, float *xyz, long capacity);
/* the CURRENT field `which` (BQ_F_RHO, BQ_F_T, BQ_F_U, BQ_F_V, BQ_F_W; each with its own stagger) sampled at every tracer
 * (gpu_sample_particles), in id order: copies min(count, capacity) values when out != NULL; returns the count or -1. Blocking. */
long  bq_solver_tracer_sample(bq_solver *s, int which, float *out, long capacity);
/* <path>/tracers_%04u.bqp for frame + 1, little endian, packed: char magic[8] = "BQPART01", uint32 version = 1, uint32 frame,
 * uint64 count, int32 nx, ny, nz, float h, int32 attribute (-1: none, else the BQ_F_* id); then count x (x, y, z) float32 in
 * id order; then, when which >= 0, count float32 of bq_solver_tracer_sample(which).  Returns the bytes written or -1. */
long  bq_solver_output_tracers(bq_solver *s, unsigned frame, const char *path, int which);
/* the STORED order, for tests and tools: xyz receives three runs of min(count, capacity) floats (all x, all y, all z), ids
 * the id of every stored slot (either may be NULL).  Returns the count.  Blocking. */
long  bq_solver_tracer_stored(bq_solver *s, float *xyz, unsigned *ids, long capacity);
float bq_solver_last_cfldt(const bq_solver *s);
float bq_solver_last_ms(const bq_solver *s);          /* event time of the last advance()        */
int   bq_solver_reinit_count(const bq_solver *s);

#ifdef __cplusplus
}
#endif
#endif
