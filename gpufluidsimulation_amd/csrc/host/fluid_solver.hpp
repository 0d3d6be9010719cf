// fluid_solver.hpp -- GPU-resident BiMocq smoke solver: the time-step state machine.
//
// Keeps the reference's BimocqGPUSolver surface (src/bimocq3D/BimocqGPUSolver.h:27-56):
//   BimocqGPUSolver(nx, ny, nz, L, vis_coeff, blend_coeff, scheme, gpuMapper*)
//   setSmoke(drop, raise, emitters) / advance(framenum, dt) / outputResult(frame, path)
// so the reference's driver loop (src/bimocq3D/main.cpp:151-159) runs against it unchanged.
// `FluidSolver` (the name BASELINE.json uses) is an alias with step()/dump() spellings.
#pragma once
#include <string>
#include <thread>
#include <array>
#include <vector>
#include "bimocq_solver.h"
#include "mapping.hpp"

namespace bqhost {

enum Scheme { BIMOCQ = 0, SEMILAG, MACCORMACK, MAC_REFLECTION };     // BimocqSolver.h:29

// The legacy emitter: the reference's GPU solver never samples its Emitter's OpenVDB SDF
// (BimocqGPUSolver.cpp:376-392 uses hard-coded spheres); what it does use is kept.  Sources that are
// sampled -- spheres, boxes, level sets -- are bq_source entries (setSources below).
struct Emitter {
    int emitFrame = 0;
    float emit_density = 0.f, emit_temperature = 0.f;
    float e_pos[3] = { 0.f, 0.f, 0.f };
    float radius = 0.f;
    float emiter = 0.f;                 // sign/scale of the x-velocity the source imposes
};

class BimocqGPUSolver {
public:
    BimocqGPUSolver(unsigned nx, unsigned ny, unsigned nz, float L, float vis_coeff, float blend_coeff,
                    Scheme inScheme, gpuMapper *mymapper);
    bool ok() const { return ok_; }

    void advance(int framenum, float dt);
    void advanceBimocq(int framenum, float dt);
    void advanceReflection(int framenum, float dt);
    void advanceMacCormack(int framenum, float dt);
    // MacCormack advection, the building block of both schemes above (fluid_solver.cpp).  adv: what is advected; field: what
    // the limiter looks at and the result replaces (the two differ in the reflection scheme's second half only).
    struct MacCormackFields { int count; DeviceField *adv[3]; DeviceField *field[3]; };   // count 1: a scalar, 3: u, v, w
    void macCormack(const MacCormackFields &f, float t, float dt_clamp);
    // BQ_OPT_FUSED_MACCORMACK: 0 the separate launches everywhere, 1 (default) gpu_maccormack in the MACCORMACK scheme,
    // 2 in MAC_REFLECTION too.  An operator library without gpu_maccormack runs the separate launches.
    int  fused_maccormack = 1;
    bool fusedMacCormack() const;
    bool beginSchemeStep();
    int  reach(float t) const;              // ghost planes a look-up after a trace over t can touch
    int  velValid() const;
    void semilagScalar(DeviceField &dst, DeviceField &src, float t);
    void semilagVelocity(DeviceField &uo, DeviceField &vo, DeviceField &wo, DeviceField &us, DeviceField &vs, DeviceField &ws, float t);
    void limiter(DeviceField &field, DeviceField &temp, int dx, int dy, int dz, float dtc);
    void axpy(DeviceField &f1, DeviceField &f2, float coeff, size_t count);
    void applySources(bool emit, int framenum, float dt_emit, float dt_forces);
    float getCFL();
    void emitSmoke(int framenum, float dt);
    void addBuoyancy(float dt);
    // Vorticity confinement (an extension, the reference has no such force): u += dt eps h (N x omega) by one
    // gpu_vorticity_confinement call right after the buoyancy, over the same dt, in every scheme.  One GPU.  With the
    // coefficient at 0 (default) a step issues exactly the launches it issues without this feature and nothing is allocated.
    float confinement = 0.f;
    static bool confinementOperator();              // the operator library has gpu_vorticity_confinement
    bool setVorticityConfinement(float eps);
    void confine(float dt);
    void diffuseField(float *field, float *t0, float *t1, int ni, int nj, int nk, int iter, float nu, float dt);
    void diffuseFieldSlab(DeviceField &field, DeviceField &t0, DeviceField &t1, int bi, int bj, int bk, int iter, float nu, float dt);
    void diffuseVelocity(float dt);
    bool projection(bool with_delta = false);
    bool projectionJacobi(bool with_delta);         // one GPU: plain, with obstacles, with walls
    bool projectionJacobiSlabs(bool with_delta);    // z-slab ranks: chunks of G sweeps per exchange (slab_jacobi_plan.hpp)
    void velocityReinitialize();
    void scalarReinitialize();
    bool whole_grid_prev = true;            // BQ_OPT_WHOLE_GRID_PREV
    bool wholeGridPrev() const;             // blend != 1 on z-slab ranks with the zeroed map border: *Prev fields need whole-grid copies
    void setSmoke(float drop, float raise, const std::vector<Emitter> &emitters);
    long outputResult(unsigned frame, const std::string &filepath);
    // The same dump without stalling the simulation: the density is downloaded into pinned
    // memory on the copy stream, ordered after the step that produced it, and a worker thread writes the file
    // while the next advance() runs.  At most one dump is in flight: a second call first waits for the
    // previous one.  waitOutput() returns that dump's voxel count (or -1) and leaves nothing in flight.
    bool outputResultAsync(unsigned frame, const std::string &filepath);
    long waitOutput();
    ~BimocqGPUSolver();

    // FluidSolver spellings
    void step(int framenum, float dt) { advance(framenum, dt); }
    long dump(unsigned frame, const std::string &filepath) { return outputResult(frame, filepath); }

    // projection variant (compile-time `#if` in the reference, BimocqGPUSolver.cpp:408-466)
    bool  keep_full_state = false;      // BQ_OPT_FULL_STATE: also compute state nothing reads (see advanceBimocq)
    int   reinit_policy = 0;            // BQ_OPT_REINIT_POLICY
    bool  setReinitPolicy(int policy);
    // BQ_OPT_REINIT_MAX_TRAVEL (policy 1): a map set is also re-initialised when its measured z-travel (cells) + this step's
    // CFL travel + the sampling footprint would no longer fit `travel_limit` planes next step.  0 = no such rule (single GPU
    // default); z-slab ranks: the ghost depth G (default, and the largest value that makes sense there).
    int   travel_limit = 0;
    void  setTravelLimit(int cells);
    int   forced_reinits = 0;           // re-initialisations the travel rule (not the CPU solver's thresholds) caused
    int   vel_reinits = 0, scalar_reinits = 0;
    float last_vel_distortion = 0.f, last_scalar_distortion = 0.f;
    int   steps_taken = 0;
    DeviceField DensityTemp, TemperatureTemp, DensityExtern, TemperatureExtern;   // policy 1 only (:53-58)
    int   projection_kind = 0;          // BQ_PROJECTION_JACOBI / BQ_PROJECTION_MGCG / BQ_PROJECTION_PCG
    int   mg_iters = 50;                // :444
    int   jacobi_iters = 100;           // :409
    float halfrdx = 0.5f;               // :410 (quarter-strength projection; 1.0 is the physical value)
    bool  verbose = false;              // print "[Bimocq GPU Time: ...]" like the reference (:126)
    // BQ_OPT_PROFILE_PHASES: event pairs on the compute stream around the phases of advanceBimocq -- where a step's time
    // goes on THIS rank, exposed communication included (the waits sit inside the phase that needs the data)
    enum Phase { PH_MAPS = 0, PH_ADVECT, PH_FORCES, PH_PROJECTION, PH_ACCUMULATE, PH_COUNT };
    bool  profile_phases = false;
    void  phaseMark(int phase);                     // closes the running phase and opens `phase` (PH_COUNT: just close)
    void  phaseTotals(double ms[PH_COUNT], long long *steps, bool reset);   // blocking

    float _alpha = 0.f, _beta = 0.f;    // smoke parameters (:529-534)
    Scheme myscheme;

    GridDims g;
    float CellSize, MaxVelocity = 0.f, Viscosity;
    float last_cfldt = 0.f, last_ms = 0.f;
    float step_cfldt_ = 0.f, step_vmax_ = 0.f;      // MacCormack / reflection step: getCFL()'s bound, speed bound of the traces

    DeviceField VelocityU, VelocityV, VelocityW;
    DeviceField VelocityUInit, VelocityVInit, VelocityWInit;
    DeviceField VelocityUPrev, VelocityVPrev, VelocityWPrev;
    DeviceField VelocityUPrevAll, VelocityVPrevAll, VelocityWPrevAll, DensityPrevAll, TemperaturePrevAll;   // wholeGridPrev()
    DeviceField VelocityUTemp, VelocityVTemp, VelocityWTemp;
    DeviceField duProj, dvProj, dwProj, duExtern, dvExtern, dwExtern;
    DeviceField TempSrcU, TempSrcV, TempSrcW;
    DeviceField Density, DensityInit, DensityPrev;
    DeviceField Temperature, TemperatureInit, TemperaturePrev;
    DeviceField div, p, p_temp;         // the reference lends DensityTemp/TemperatureTemp/TempSrcV here (:410)
    DeviceField debugParam;             // 4096 floats, residual history (:412-417)
    // fp64 work arrays + level pyramid of the multigrid-CG projection (:60-90), allocated on first use
    struct Mgcg {
        DeviceBytes div, p, dir, residual, temp0, temp1, result;
        std::vector<DeviceBytes> b, x, r;
        std::vector<SCoarseLevelInfo> levels;
        bool ready = false;
        // z-slab ranks: the velocity of the WHOLE grid, assembled on every rank for the replicated solve (projectionMgcgSlabs)
        DeviceField gu, gv, gw;
    } mg;
    bool allocMgcg();
    bool projectionMgcgSlabs();
    bool projectionMgcgShared();                    // the levels shared between the slab ranks; false: not applicable here
    bool mgcg_shared = true;                        // BQ_OPT_MGCG_SHARED
    bool mgcg_shared_ran = false;                   // the last MGCG projection on slabs took the shared path
    std::vector<double> mgHistory() const;          // tempResult (4096 doubles), downloaded
    // BQ_PROJECTION_PCG: the masked system solved to a relative tolerance in the arrays of allocMgcg;
    // with or without obstacles, one GPU only
    int    pcg_iters = 1000;                        // most CG updates per projection (BimocqSolver.cpp:1269)
    double pcg_tol = 1e-6;
    double pcg_stats[4] = { 0, 0, 0, 0 };           // last projection: iterations, final max|r|, max|b|, stop reason (BQ_PCG_*)
    long long pcg_projections = 0, pcg_unconverged = 0;
    static bool pcgOperators();                     // the operator library has the PCG operators
    bool projectionPcg();

    // Solid obstacles (setBoundary / updateBoundary, BimocqSolver.cpp:936-1064).  Jacobi projection on
    // one GPU only.  With an empty list a step issues exactly the launches it issues without this feature.
    std::vector<bq_boundary> boundaries;
    DeviceBytes solid, rows;                        // cell flags (0 fluid, o + 1 solid by obstacle o), rows summary (include/bimocq_gpu.h)
    bool setBoundary(const bq_boundary *b, const bq_levelset *ls, int n, const bq_pose *pose = nullptr);   // ls: NULL when no entry is a level set
    bool updateBoundary(int framenum, float dt);
    // Level sets (shape BQ_SHAPE_LEVELSET): `levelsets` holds one descriptor per entry of `boundaries` (phi into lsgrids)
    // when the list holds a level set, and is empty otherwise -- then every obstacle operator call is the analytic one.
    static constexpr size_t kMaxLevelsetBytes = (size_t)256 << 20;
    std::vector<bq_levelset> levelsets;
    DeviceBytes lsgrids;                            // every level-set grid of the list, one allocation
    const bq_levelset *levelsetList() const { return levelsets.empty() ? nullptr : levelsets.data(); }
    // Rigid poses: one pose per entry of `boundaries`, `orientations` the double master copies of the
    // quaternions that updateBoundary integrates (the floats of `poses` are rounded from them).  posed_list: the list holds an
    // oriented or spinning entry -- only then do the obstacle operator calls become the _pose ones.
    std::vector<bq_pose> poses;
    std::vector<std::array<double, 4>> orientations;
    bool posed_list = false;
    const bq_pose *poseList() const { return posed_list ? poses.data() : nullptr; }
    void dropBoundaries();
    bool buildFlags(const std::vector<bq_boundary> &list, const bq_levelset *ls, const bq_pose *pose);
    // Closed domain walls (the reference's container, BimocqSolver.cpp:938-948): `walls` the closed sides
    // (BQ_WALL_* bits), `solidw` = solid + BQ_FLAG_WALL in the wall cells, allocated only while walls are on and rebuilt when the
    // walls or the obstacle flags change.  solid and rows stay the obstacles' own (rows: all zero while the list is empty).
    // With walls off a step issues exactly the launches it issues without this feature.
    int walls = 0;
    DeviceBytes solidw;
    bool setWalls(int mask);
    bool buildWallFlags();                          // on failure the walls are dropped
    void dropWalls();
    static bool wallOperators();                    // the operator library has the wall operators
    const unsigned char *projectionFlags() { return walls ? solidw.u8() : (boundaries.empty() ? nullptr : solid.u8()); }
    void blendBoundary(bool band);                  // band: blendBoundary + clearBoundary, else clearBoundary only
    void semilagBand(float cfldt, float dt);

    // Shaped, moving smoke sources (Emitter / emitSmoke of the CPU solver, BimocqSolver.h:31-59, BimocqSolver.cpp:696-813;
    // DESIGN.md section 16): a second list next to sim_emitter.  At every emission point each source first moves by its own
    // velocity * dt, then the active ones are applied by one gpu_emit_sources call.  With an empty list a step issues
    // exactly the launches it issues without this feature.
    std::vector<bq_source> sources;
    std::vector<bq_levelset> source_levelsets;      // one descriptor per entry of `sources` (phi into source_grids) when the list holds a level set, else empty
    DeviceBytes source_grids;                       // every level-set grid of the sources, one allocation (counted apart from lsgrids)
    bool setSources(const bq_source *src, const bq_levelset *ls, int n);       // ls: NULL when no entry is a level set
    void dropSources();
    bool velocitySourceActive(int framenum) const;  // some source imposes its velocity this frame

    std::vector<float> host_density, host_u, host_v, host_w;    // outputResult staging (:538-541)

    // Flow diagnostics: kinetic energy, enstrophy, divergence norms, density moments and the vorticity
    // magnitude from one pass of gpu_flow_stats over the current fields.  Solid cells count as fluid.  With
    // diagnostics_every == 0 (default) nothing is allocated and a step issues exactly the launches it issues without this.
    static constexpr int kDiagRing = 1024;          // rows of the device ring of BQ_OPT_DIAGNOSTICS_EVERY
    static bool diagOperator();                     // the operator library has gpu_flow_stats
    int  diagnostics_every = 0;                     // BQ_OPT_DIAGNOSTICS_EVERY
    bool setDiagnosticsEvery(int n);
    bool diagnostics(double out[BQ_DIAG_COUNT]);    // blocking; every slab rank gets the grid's values
    long diagnosticsHistory(double *host, long capacity_rows);     // the retained rows, oldest first; blocking
    long vorticity(float *host, long capacity);     // |omega| of the local planes; blocking
    long outputVorticity(unsigned frame, const std::string &filepath, float threshold);
    bool enqueueStats(float *vort, double *d_out);
    void sampleDiagnostics();
    void diagRow(const double raw[BQ_STAT_COUNT], int step, double out[BQ_DIAG_COUNT]) const;
    DeviceBytes diag_one, diag_ring;                // BQ_STAT_COUNT doubles of the blocking calls; kDiagRing rows of them
    std::vector<int> diag_ring_steps;               // STEP of every ring row
    long long diag_rows = 0;                        // samples enqueued so far
    DeviceField Vorticity;                          // scratch of vorticity(), allocated on first use
    std::vector<float> host_vorticity;

    // Per-obstacle pressure loads: on a sampled step every projection that ran with obstacles is followed
    // by one gpu_obstacle_loads call into a slot of a device ring (row = step, slot = which projection of the step); the host
    // keeps what it needs to scale a row at read time.  With loads_every == 0 (default) nothing is allocated and a step
    // issues exactly the launches it issues without this.
    static constexpr int kLoadRing = 1024;          // rows of the device ring of BQ_OPT_OBSTACLE_LOADS
    static constexpr int kLoadSlot = BQ_MAX_BOUNDARIES * BQ_LOAD_COUNT;    // doubles per slot; two slots per row
    struct LoadRow {
        int    step = 0, n = 0, filled = 0;         // filled: slots a projection of the step wrote (the others read 0)
        double dt = 0.0, halfrdx = 0.0, w[2] = { 1.0, 0.0 };       // w[1] != 0: the scheme projects twice, slot 1 is its last
    };
    static bool loadsOperator();                    // the operator library has gpu_obstacle_loads
    int  loads_every = 0;                           // BQ_OPT_OBSTACLE_LOADS
    bool setObstacleLoads(int n);
    int  obstacleLoads(double row[BQ_OLOAD_ROW]);   // the newest row; blocking; 1, 0 when there is none, -1 on error
    long obstacleLoadsHistory(double *host, long capacity_rows);   // the retained rows, oldest first; blocking
    long obstacleLoadsRaw(long back, double *slots, double weights[2]);    // STEP of that row or -1; blocking
    void beginLoadRow(float dt);                    // advance(): opens the row of a sampled step
    void sampleLoads(const float *p, const double *p64);           // after a projection with obstacles: the next slot
    void endLoadRow();
    void loadRow(const LoadRow &r, const double *slots, double out[BQ_OLOAD_ROW]) const;
    DeviceBytes load_ring;                          // kLoadRing rows of 2 kLoadSlot doubles
    std::vector<LoadRow> load_ring_rows;            // what the host keeps per ring row
    long long load_rows = 0;                        // rows sampled so far
    bool load_open = false;                         // a sampled step is running
    int  load_slot = 0;                             // the slot its next projection fills

    // Shadowed density preview: gpu_render_density on the current density.  The shadow field and the
    // image buffer are allocated on the first call; advance() never touches any of this.
    static bool renderOperator();                   // the operator library has gpu_render_density
    bool renderSize(int view, int &w, int &h) const;
    // radiance and transmittance of the W x H image (both may be NULL: only the count); blocking; every slab rank gets the
    // whole image.  Returns W * H or -1.
    long render(int view, int light, float sigma, float albedo, float ambient, float *radiance, float *transmittance, long capacity);
    long outputPreview(unsigned frame, const std::string &filepath, int view, int light, float sigma, float albedo, float ambient,
                       float background);
    // the same with the solid obstacles drawn: gpu_render_density_solids on `solid` and `rows`; hit:
    // the tag o + 1 of the first obstacle cell of the pixel's ray, 0: none (its transmittance is then 0).  Without obstacles
    // (an empty list, z-slab ranks) it is render() and hit = 0.  The three-plane image is allocated on the first such call.
    static bool renderSolidsOperator();             // the operator library has gpu_render_density_solids
    long renderSolids(int view, int light, float sigma, float albedo, float ambient, float solid_albedo, float solid_ambient,
                      float *radiance, float *transmittance, unsigned char *hit, long capacity);
    long outputPreviewSolids(unsigned frame, const std::string &filepath, int view, int light, float sigma, float albedo, float ambient,
                             float solid_albedo, float solid_ambient, float background);
    DeviceBytes render_image_solids;                // 3 W H doubles: Cfix, Afix, Hfix
    DeviceField Shadow;                             // s per cell, scratch of render()
    DeviceBytes render_image;                       // 2 W H doubles: Cfix, Afix
    std::vector<double> host_image;
    std::vector<float> host_radiance, host_transmittance;

    // Passive tracer particles: positions live on the device as three arrays; advance() moves them
    // over the whole dt through the velocity the step starts with (gpu_trace_particles, the forward map's own trace), on
    // the compute stream, no host sync.  One GPU.  With no tracers a step issues exactly the launches it issues without
    // this feature and nothing is allocated.  Everything public is in id order: id = position in the set as it was given
    // (setTracers) or appended (seedTracers), whatever sorting has happened in between.
    static bool tracerOperators();                  // the operator library has the tracer operators
    long tracer_count = 0;
    int  tracer_sort_every = 0;                     // BQ_OPT_TRACER_SORT_EVERY
    long long tracer_sorts = 0;                     // sorts issued so far
    bool setTracerSortEvery(int n);
    bool tracersAllowed(const char *who);           // latches the refusal
    bool setTracers(const float *xyz, long n);      // replaces the set; any failure leaves none
    long seedTracers(const int lo[3], const int hi[3], int per_cell, unsigned seed);    // appends; the number added or -1
    long tracers(float *xyz, long capacity);        // blocking; the count, min(count, capacity) triples copied
    long tracerSample(int which, float *out, long capacity);    // blocking; the count or -1
    long outputTracers(unsigned frame, const std::string &filepath, int which);        // which < 0: no attribute
    void dropTracers();
    bool growTracers(long total);                   // room for `total` particles, the first tracer_count kept
    void moveTracers(float cfldt, float dt);
    void sortTracers();
    bool downloadTracerIds();                       // host_tracer_ids: the id of every stored slot (empty: identity)
    DeviceField TracerX, TracerY, TracerZ;
    DeviceField TracerX2, TracerY2, TracerZ2, TracerAttr;   // the sort's second buffers; scratch of tracerSample
    DeviceBytes tracer_id, tracer_id2;              // unsigned per stored slot, allocated by the first sort
    bool tracer_ids = false;
    std::vector<float> host_tracers, host_tracer_xyz, host_tracer_attr;
    std::vector<unsigned> host_tracer_ids;

    gpuMapper *GpuSolver;
    MapperBaseGPU VelocityAdvector, ScalarAdvector;
    int vel_lastReinit = -11, scalar_lastReinit = -31;          // BimocqGPUSolver.h:109-110
    std::vector<Emitter> sim_emitter;

private:
    struct PhaseSpan { void *a, *b; int phase; };
    std::vector<PhaseSpan> phase_spans_;
    void *phase_open_ev_ = nullptr;
    int phase_open_ = -1;
    long long phase_steps_ = 0;
    bool ok_ = false;
    float *dump_host_ = nullptr;        // pinned staging buffer of the asynchronous dump
    DeviceField dump_dev_;              // device snapshot of the dumped frame (the next advance() rewrites Density)
    std::thread dump_thread_;
    long dump_result_ = 0;
};

using FluidSolver = BimocqGPUSolver;

// writeVDB's contract (utils/volumeMeshTools.h:33-60) in a dependency-free container; returns the
// number of voxels written or -1.  Defined in density_dump.cpp.
long write_density_dump(unsigned frame, const std::string &filepath, float voxel_size,
                        const float *density, int nx, int ny, int nz, int k_offset, int nz_global);
// the same container for any cell-centred field: grid name, file stem (<path>/<stem>_%04u.bqd) and threshold are the
// caller's; a voxel is kept where (double)|value| > cut, `threshold` is what the header records
long write_field_dump(unsigned frame, const std::string &filepath, float voxel_size, const float *field, int nx, int ny, int nz,
                      int k_offset, int nz_global, const char *grid_name, const char *stem, float threshold, double cut);
// <path>/preview_%04u.pgm, binary 8-bit P5, w x h: a pixel is clamp(radiance + transmittance * background, 0, 1) (the sum in
// double: one rounding) times 255 rounded to nearest; image rows are written highest index first.  Returns the bytes written or -1.
long write_preview_pgm(unsigned frame, const std::string &filepath, const float *radiance, const float *transmittance, int w, int h,
                       float background);
// <path>/tracers_%04u.bqp, little endian, packed: char magic[8] = "BQPART01", uint32 version = 1, uint32 frame, uint64 count,
// int32 nx, ny, nz, float h, int32 attribute (-1: none, else the BQ_F_* id sampled); then count x (x, y, z) float32 in id
// order; then, with an attribute, count float32.  Returns the bytes written or -1.
long write_tracer_dump(unsigned frame, const std::string &filepath, const float *xyz, const float *attribute, long count,
                       int nx, int ny, int nz, float h, int which);
// exp_portable of the operators (the oracle's orc_expf), operation for operation, on the host; att() of gpu_render_density
float portable_expf(float x);
float render_attenuation(double afix);
#ifdef HAVE_OPENVDB
long write_density_vdb(unsigned frame, const std::string &filepath, float voxel_size,
                       const float *density, int nx, int ny, int nz, int k_offset, int nz_global);
#endif

} // namespace bqhost
