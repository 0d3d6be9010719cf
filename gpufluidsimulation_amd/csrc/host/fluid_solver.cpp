// fluid_solver.cpp -- see fluid_solver.hpp.  Reference: src/bimocq3D/BimocqGPUSolver.cpp.
//
// The step restates BimocqGPUSolver::advanceBimocq (:129-230) operator by operator.  Work that the
// reference performs but that provably cannot change any value is dropped, each case documented
// where it happens (shared map sets, the identically-zero scalar "extern" deltas, buffer swaps in
// place of copies whose source is dead).  Everything else -- including the reference's quirks that
// DO change values -- is kept, and tests/ checks the trajectory against
// the CPU oracle bit for bit.
//
// z-slab ranks run the same code: gpuMapper::require()/produced() keep track of how many ghost
// planes of every field are correct and exchange them with the z-neighbours exactly when an operator
// reaches further than that (no-ops on a single GPU).
#include "fluid_solver.hpp"
#include "../bq_levelset.h"
#include "../bq_pose.h"
#include "slab_jacobi_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// The obstacle operators are weak references: the CPU stand-ins of the operator ABI that the host tests link against need
// not provide them (the references resolve to null there), and setBoundary refuses obstacles when they are missing.
#pragma weak gpu_obstacle_flags
#pragma weak gpu_obstacle_faces
#pragma weak gpu_jacobi_sweeps_masked
#pragma weak gpu_gradient_masked
#pragma weak gpu_semilag_band
#pragma weak gpu_obstacle_blend
#pragma weak gpu_obstacle_flags_ls
#pragma weak gpu_semilag_band_ls
#pragma weak gpu_obstacle_blend_ls
#pragma weak gpu_obstacle_flags_pose
#pragma weak gpu_semilag_band_pose
#pragma weak gpu_obstacle_blend_pose
#pragma weak gpu_obstacle_faces_pose
#pragma weak gpu_divergence_double
#pragma weak gpu_pcg_solve
#pragma weak gpu_pcg_gradient
#pragma weak gpu_emit_sources
#pragma weak gpu_maccormack
#pragma weak gpu_wall_flags
#pragma weak gpu_wall_faces
#pragma weak gpu_jacobi_sweeps_masked_walls
#pragma weak gpu_gradient_masked_walls
#pragma weak gpu_pcg_gradient_walls
#pragma weak gpu_jacobi_sweep_masked_walls_range
#pragma weak gpu_jacobi_sweep_masked_walls_triple_ranges
#pragma weak gpu_flow_stats
#pragma weak gpu_render_density
#pragma weak gpu_render_density_solids
#pragma weak gpu_vorticity_confinement
#pragma weak gpu_obstacle_loads

namespace bqhost {
namespace slab = bq::slab;

// While one lives, the caller vouches that the two pressure buffers it hands to the sweep entry points carry the same boundary
// layer (and the same values in every solid cell): FL_OPT_JACOBI_FUSE 1 (fuse after checking the shells) becomes 2 (fuse on the
// caller's word); every other setting is the user's and stays.
class JacobiFuseVouched {
    const int was_ = fl_get_option(FL_OPT_JACOBI_FUSE);
public:
    JacobiFuseVouched() { if (was_ == 1) fl_set_option(FL_OPT_JACOBI_FUSE, 2); }
    ~JacobiFuseVouched() { fl_set_option(FL_OPT_JACOBI_FUSE, was_); }
    JacobiFuseVouched(const JacobiFuseVouched &) = delete;
    JacobiFuseVouched &operator=(const JacobiFuseVouched &) = delete;
};

// The obstacle operators for a list with level-set descriptors ls (non-NULL only when it holds a level set, and then
// setBoundary has found the _ls operators), else the analytic ones: runs without level sets issue the launches they did
// before level sets existed, and the stand-ins without the _ls operators still run analytic lists.  Likewise `pose`
// (DESIGN.md section 23): non-NULL only when the list holds an oriented or spinning entry, and then setBoundary has found the
// _pose operators.
static void obstacle_flags(unsigned char *solid, unsigned char *rows, const bq_boundary *b, int n, const bq_levelset *ls,
                           const bq_pose *pose, float h, int ni, int nj, int nk)
{
    if (pose) gpu_obstacle_flags_pose(solid, rows, b, n, ls, pose, h, ni, nj, nk);
    else if (ls) gpu_obstacle_flags_ls(solid, rows, b, n, ls, h, ni, nj, nk);
    else    gpu_obstacle_flags(solid, rows, b, n, h, ni, nj, nk);
}

static void semilag_band(float *field, float *field_src, float *u, float *v, float *w, int dim_x, int dim_y, int dim_z, float h,
                         int ni, int nj, int nk, float cfldt, float dt, const bq_boundary *b, int n, const bq_levelset *ls,
                         const bq_pose *pose)
{
    if (pose) gpu_semilag_band_pose(field, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt, b, n, ls, pose);
    else if (ls) gpu_semilag_band_ls(field, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt, b, n, ls);
    else    gpu_semilag_band(field, field_src, u, v, w, dim_x, dim_y, dim_z, h, ni, nj, nk, cfldt, dt, b, n);
}

static void obstacle_blend(float *u, float *v, float *w, float *rho, float *T, const float *us, const float *vs, const float *ws,
                           const float *rhos, const float *Ts, const unsigned char *solid, const bq_boundary *b, int n,
                           const bq_levelset *ls, const bq_pose *pose, float h, int ni, int nj, int nk)
{
    if (pose) gpu_obstacle_blend_pose(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, ls, pose, h, ni, nj, nk);
    else if (ls) gpu_obstacle_blend_ls(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, ls, h, ni, nj, nk);
    else    gpu_obstacle_blend(u, v, w, rho, T, us, vs, ws, rhos, Ts, solid, b, n, h, ni, nj, nk);
}

// The operators of one projection, chosen once from the obstacle list and the walls: plain (neither), masked (obstacles), walled
// (closed sides, with or without obstacles).  Every choice between the three families is made in here; a _walls entry point is
// reached only with walls != 0, so an operator library without them is never called through a null reference.  Plane ranges
// exist for the plain and the walled family (the z-slab projection; setBoundary refuses slab ranks).
struct ProjectionOps {
    static constexpr float alpha = -1.f, beta = (float)(1.0 / 6.0);
    enum Kind { kPlain, kMasked, kWalled };
    BimocqGPUSolver &s;
    const Kind kind;
    float *const u, *const v, *const w, *const div;
    const int ni, nj, nk, walls;
    const unsigned char *const flags, *const rows;      // the flags the projection reads (walls on: solid + walls), the rows summary

    explicit ProjectionOps(BimocqGPUSolver &s_)
        : s(s_), kind(s.walls ? kWalled : s.boundaries.empty() ? kPlain : kMasked), u(s.VelocityU), v(s.VelocityV), w(s.VelocityW),
          div(s.div), ni(s.g.ni), nj(s.g.nj), nk(s.g.nk), walls(s.walls), flags(s.projectionFlags()), rows(s.rows.u8()) {}

    // solid faces take the obstacle velocity, wall faces 0 (du: their share of d*Proj); disjoint faces, so the order is free
    void faces(float *du, float *dv, float *dw) const
    {
        const int n = (int)s.boundaries.size();
        if (n && s.poseList()) gpu_obstacle_faces_pose(u, v, w, du, dv, dw, s.solid.u8(), s.boundaries.data(), s.poseList(), n, s.CellSize, ni, nj, nk);
        else if (n) gpu_obstacle_faces(u, v, w, du, dv, dw, s.solid.u8(), s.boundaries.data(), n, ni, nj, nk);
        if (kind == kWalled) gpu_wall_faces(u, v, w, du, dv, dw, flags, ni, nj, nk);
    }
    // `count` sweeps on the whole array, one launch or several as the library sees fit; 1: the newest iterate is in `b`
    int sweeps(float *a, float *b, int count) const
    {
        if (kind == kWalled) return gpu_jacobi_sweeps_masked_walls(a, div, b, flags, rows, walls, ni, nj, nk, count, alpha, beta);
        if (kind == kMasked) return gpu_jacobi_sweeps_masked(a, div, b, flags, rows, ni, nj, nk, count, alpha, beta);
        return gpu_jacobi_sweeps(a, div, b, ni, nj, nk, count, alpha, beta);
    }
    // one sweep on the planes `a`
    void single(const float *in, float *out, slab::Planes a) const
    {
        if (kind == kWalled) gpu_jacobi_sweep_masked_walls_range(in, div, out, flags, rows, walls, ni, nj, nk, a.k0, a.k1, alpha, beta);
        else if (kind == kPlain) gpu_jacobi_sweep_range(in, div, out, ni, nj, nk, a.k0, a.k1, alpha, beta);
        else fl_report_error(FL_ERR_UNSUPPORTED, "projection: the masked sweeps have no plane ranges");
    }
    // S = 2 or 3 sweeps in one launch on up to two plane ranges; false: the library refuses (nothing was launched).  The walled
    // family has no pairs, and its plan names none.
    bool fused(int S, const float *in, float *out, slab::Planes a, slab::Planes b = slab::Planes{0, 0}) const
    {
        if (kind != kPlain)
            return kind == kWalled && S == 3 && gpu_jacobi_sweep_masked_walls_triple_ranges(in, div, out, flags, rows, walls, ni, nj, nk, a.k0, a.k1,
                                                                                            b.k0, b.k1, alpha, beta) != 0;
        return (S == 3 ? gpu_jacobi_sweep_triple_ranges : gpu_jacobi_sweep_pair_ranges)(in, div, out, ni, nj, nk, a.k0, a.k1, b.k0, b.k1,
                                                                                         alpha, beta) != 0;
    }
    // p's gradient off the faces between fluid cells (du: the change handed out, all three or none); p64: the PCG projection's
    void gradient(const float *p, float *du, float *dv, float *dw) const
    {
        if (kind == kWalled) gpu_gradient_masked_walls(u, v, w, p, du, dv, dw, flags, walls, ni, nj, nk, s.halfrdx);
        else if (kind == kMasked) gpu_gradient_masked(u, v, w, p, du, dv, dw, flags, ni, nj, nk, s.halfrdx);
        else if (du) gpu_gradient_delta(u, v, w, p, du, dv, dw, ni, nj, nk, s.halfrdx);
        else gpu_gradient(u, v, w, p, ni, nj, nk, s.halfrdx);
    }
    void gradient(const double *p64) const
    {
        if (kind == kWalled) gpu_pcg_gradient_walls(u, v, w, p64, flags, walls, ni, nj, nk, (double)s.halfrdx);
        else gpu_pcg_gradient(u, v, w, p64, flags, ni, nj, nk, (double)s.halfrdx);
    }
};

// Every level-set grid of a list (entry o is one when is_ls[o]; ls[o].phi a HOST array) copied into ONE device allocation,
// `descs` receiving one descriptor per entry whose phi points into it.  `who` prefixes the refusal (more than `cap` bytes
// in all).  Shared by setBoundary and setSources, whose allocations are counted apart.
static bool upload_levelsets(const std::vector<char> &is_ls, const bq_levelset *ls, size_t cap, const char *who,
                             DeviceBytes &grids, std::vector<bq_levelset> &descs)
{
    const int n = (int)is_ls.size();
    auto grid_bytes = [&](int o) { return (size_t)ls[o].nx * (size_t)ls[o].ny * (size_t)ls[o].nz * sizeof(float); };
    size_t total = 0;                                   // below 16 * 2^33 bytes: no overflow
    for (int o = 0; o < n; o++)
        if (is_ls[o]) total += grid_bytes(o);
    if (total > cap) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, (std::string(who) + ": level-set grids above 256 MiB in all").c_str());
        return false;
    }
    if (!grids.alloc(total)) return false;
    descs.assign((size_t)n, bq_levelset{});
    size_t at = 0;
    for (int o = 0; o < n; o++) {
        if (!is_ls[o]) continue;
        float *dst = reinterpret_cast<float *>(grids.u8() + at);
        fl_memcpy_h2d(dst, ls[o].phi, grid_bytes(o));
        descs[o] = ls[o];
        descs[o].phi = dst;
        at += grid_bytes(o);
    }
    return fl_last_error() == FL_OK;
}

// BQ_TRACE=1 (debug): after each stage print the sum of squares of the planes this rank owns, so a
// slab run can be compared stage by stage with a single-GPU run (sum the ranks' lines).
static void trace_stage(BimocqGPUSolver &s, const char *stage, int frame)
{
    static const bool on = getenv("BQ_TRACE") && atoi(getenv("BQ_TRACE")) != 0;
    if (!on) return;
    const SlabCtx &sl = s.GpuSolver->slab;
    const int G = sl.on ? sl.G : 0, own = sl.on ? sl.own1 - sl.own0 : s.g.nk;
    const bool top = !sl.on || sl.own1 == sl.nkg;
    struct Item { const char *name; DeviceField *f; } items[] = {
        { "U", &s.VelocityU }, { "V", &s.VelocityV }, { "W", &s.VelocityW }, { "Ui", &s.VelocityUInit }, { "Wi", &s.VelocityWInit },
        { "rho", &s.Density }, { "bz", &s.VelocityAdvector.maps->BackwardZ }, { "fz", &s.VelocityAdvector.maps->ForwardZ },
        { "dUp", &s.duProj }, { "dWp", &s.dwProj }, { "p", &s.p }, { "div", &s.div },
        { "bx", &s.VelocityAdvector.maps->BackwardX }, { "by", &s.VelocityAdvector.maps->BackwardY },
        { "fx", &s.VelocityAdvector.maps->ForwardX }, { "usrc", &s.GpuSolver->u_src }, { "vsrc", &s.GpuSolver->v_src }, { "wsrc", &s.GpuSolver->w_src } };
    std::vector<float> host;
    char fname[128];
    snprintf(fname, sizeof fname, "/tmp/bqtrace_%dof%d.txt", sl.rank, sl.nranks);
    FILE *fo = fopen(fname, "a");
    if (!fo) return;
    fprintf(fo, "[trace r%d f%d %-14s]", sl.rank, frame, stage);
    for (const Item &it : items) {
        host.resize(it.f->count());
        it.f->download(host.data());
        const size_t pe = it.f->plane ? it.f->plane : (size_t)s.g.ni * s.g.nj;
        const size_t lo = pe * (size_t)G, hi = pe * (size_t)(G + own + ((it.f->extra && top) ? 1 : 0));
        double acc = 0;
        for (size_t a = lo; a < hi && a < host.size(); a++) acc += (double)host[a] * (double)host[a];
        fprintf(fo, " %s=%.17g", it.name, acc);
    }
    fprintf(fo, "\n");
    fclose(fo);
    const char *dump = getenv("BQ_DUMP");
    if (dump && frame == 1 && strcmp(dump, stage) == 0) {
        for (const Item &it : items) {
            host.resize(it.f->count());
            it.f->download(host.data());
            snprintf(fname, sizeof fname, "/tmp/bqdump_%dof%d_%s.bin", sl.rank, sl.nranks, it.name);
            FILE *fd = fopen(fname, "wb");
            if (fd) { fwrite(host.data(), sizeof(float), host.size(), fd); fclose(fd); }
        }
    }
}

BimocqGPUSolver::BimocqGPUSolver(unsigned nx, unsigned ny, unsigned nz, float L, float vis_coeff, float blend_coeff,
                                 Scheme inScheme, gpuMapper *mymapper)
    : myscheme(inScheme), GpuSolver(mymapper)
{
    CellSize = L / nx;                                   // :10
    Viscosity = vis_coeff;
    (void)ny; (void)nz;
    if (!mymapper || !mymapper->ok()) return;
    g = mymapper->g;                                     // local dims (a slab rank holds owned + ghost planes)
    g.h = CellSize;

    DeviceField *ub[] = { &VelocityU, &VelocityUInit, &VelocityUPrev, &VelocityUTemp, &duProj, &duExtern, &TempSrcU };
    DeviceField *vb[] = { &VelocityV, &VelocityVInit, &VelocityVPrev, &VelocityVTemp, &dvProj, &dvExtern, &TempSrcV };
    DeviceField *wb[] = { &VelocityW, &VelocityWInit, &VelocityWPrev, &VelocityWTemp, &dwProj, &dwExtern, &TempSrcW };
    for (int a = 0; a < 7; a++)
        if (!mymapper->allocField(*ub[a], FIELD_U) || !mymapper->allocField(*vb[a], FIELD_V) || !mymapper->allocField(*wb[a], FIELD_W)) return;
    DeviceField *sb[] = { &Density, &DensityInit, &DensityPrev, &Temperature, &TemperatureInit, &TemperaturePrev,
                          &div, &p, &p_temp };
    for (DeviceField *f : sb)
        if (!mymapper->allocField(*f, FIELD_S)) return;
    if (!debugParam.alloc(4096)) return;

    if (!VelocityAdvector.init(g.ni, g.nj, g.nk, CellSize, blend_coeff, mymapper)) return;      // :92
    if (!ScalarAdvector.init(g.ni, g.nj, g.nk, CellSize, blend_coeff, mymapper)) return;        // :93
    // Both advectors are updated with the same velocity and re-initialised on the same frames
    // (`if (1)`, :218-229), so their map sets are bit-identical: keep one.
    ScalarAdvector.shareMapsOf(VelocityAdvector);

    host_density.assign(g.n(), 0.f);
    host_u.assign(g.nu(), 0.f); host_v.assign(g.nv(), 0.f); host_w.assign(g.nw(), 0.f);
    ok_ = fl_last_error() == FL_OK;
}

void BimocqGPUSolver::setSmoke(float drop, float raise, const std::vector<Emitter> &emitters)
{
    _alpha = drop;                                       // :531
    _beta = raise;                                       // :532
    sim_emitter = emitters;
}

// :108-127
void BimocqGPUSolver::advance(int framenum, float dt)
{
    GpuSolver->startEventRecord();
    if (loads_every > 0 && (steps_taken + 1) % loads_every == 0) beginLoadRow(dt);      // BQ_OPT_OBSTACLE_LOADS
    switch (myscheme) {
    case BIMOCQ: advanceBimocq(framenum, dt); break;
    case MAC_REFLECTION: advanceReflection(framenum, dt); break;
    case MACCORMACK: advanceMacCormack(framenum, dt); break;      // (the CPU solver's scheme, BimocqSolver.cpp:282-364)
    default: break;                                      // SEMILAG: refused by bq_solver_create
    }
    if (load_open) endLoadRow();
    // FL_OPT_COMM_CHECK (debugging aid for the first runs on real links): every rank has issued this step's communicator
    // calls; compare the ledgers (include/bimocq_gpu.h: fl_comm_check)
    if (diagnostics_every > 0 && steps_taken % diagnostics_every == 0) sampleDiagnostics();     // BQ_OPT_DIAGNOSTICS_EVERY
    if (tracer_sort_every > 0 && tracer_count > 0 && steps_taken % tracer_sort_every == 0) sortTracers();   // BQ_OPT_TRACER_SORT_EVERY
    if (fl_comm_size() > 1 && fl_get_option(FL_OPT_COMM_CHECK) > 0) (void)fl_comm_check(0);
    last_ms = GpuSolver->endEventRecord();
    if (verbose) printf("[Bimocq GPU Time: %gms ]\n", last_ms);
}

// ---- the pieces the MacCormack and the reflection scheme are made of -------------------------------------------------
// z-slab ranks (Jacobi projection): every look-up states how far it reaches along z -- the trace travels at most
// |t| * max|u| (getCFL) and the sample adds its cell and the half-cell stagger -- so gpuMapper::require refreshes ghost
// planes exactly when an input's correct depth no longer covers that reach, and produced() records what is left of it.
// step_cfldt_ / step_vmax_: getCFL()'s step bound and the speed bound of the velocity field the traces run through (max|u|
// of getCFL() until a projection has changed the field, a fresh maximum after it; single-GPU runs never look at it).
int BimocqGPUSolver::reach(float t) const
{
    return (int)std::ceil(std::fabs((double)t) * (double)step_vmax_ / (double)CellSize) + 3;
}

int BimocqGPUSolver::velValid() const { return gpuMapper::minValid({ &VelocityU, &VelocityV, &VelocityW }); }

// semilagAdvectField / semilagAdvectVelocity (GPU_Advection.h:530-551) clear their outputs first
void BimocqGPUSolver::semilagScalar(DeviceField &dst, DeviceField &src, float t)
{
    gpuMapper &gs = *GpuSolver;
    const int r = reach(t);
    gs.require({ &src, &VelocityU, &VelocityV, &VelocityW }, r);
    fl_memset(dst, 0, g.n() * sizeof(float));
    gpu_semilag(dst, src, VelocityU, VelocityV, VelocityW, 0, 0, 0, CellSize, g.ni, g.nj, g.nk, step_cfldt_, t);
    gs.produced(dst, std::min(src.valid, velValid()) - r);
}

void BimocqGPUSolver::semilagVelocity(DeviceField &uo, DeviceField &vo, DeviceField &wo, DeviceField &us, DeviceField &vs,
                                      DeviceField &ws, float t)
{
    gpuMapper &gs = *GpuSolver;
    const float h = CellSize;
    const int ni = g.ni, nj = g.nj, nk = g.nk;
    const int r = reach(t);
    gs.require({ &us, &vs, &ws, &VelocityU, &VelocityV, &VelocityW }, r);
    uo.zero(); vo.zero(); wo.zero();
    gpu_semilag(uo, us, VelocityU, VelocityV, VelocityW, 1, 0, 0, h, ni, nj, nk, step_cfldt_, t);
    gpu_semilag(vo, vs, VelocityU, VelocityV, VelocityW, 0, 1, 0, h, ni, nj, nk, step_cfldt_, t);
    gpu_semilag(wo, ws, VelocityU, VelocityV, VelocityW, 0, 0, 1, h, ni, nj, nk, step_cfldt_, t);
    const int vv = velValid();
    gs.produced(uo, std::min(us.valid, vv) - r); gs.produced(vo, std::min(vs.valid, vv) - r); gs.produced(wo, std::min(ws.valid, vv) - r);
}

// the limiter reads `field` around the departure point of a trace over dtc and rewrites `temp` at the node itself
void BimocqGPUSolver::limiter(DeviceField &field, DeviceField &temp, int dx, int dy, int dz, float dtc)
{
    gpuMapper &gs = *GpuSolver;
    const int r = reach(dtc);
    gs.require({ &field, &VelocityU, &VelocityV, &VelocityW }, r);
    gpu_clamp_extrema(field, temp, VelocityU, VelocityV, VelocityW, g.ni + dx, g.nj + dy, g.nk + dz, dx, dy, dz,
                      0.5f * dx, 0.5f * dy, 0.5f * dz, CellSize, dtc);
    gs.produced(temp, std::min(temp.valid, std::min(field.valid, velValid()) - r));
}

// f1 += coeff * f2
void BimocqGPUSolver::axpy(DeviceField &f1, DeviceField &f2, float coeff, size_t count)
{
    GpuSolver->add(f1, f2, coeff, count);
    GpuSolver->produced(f1, std::min(f1.valid, f2.valid));
}

// emission over dt_emit (legacy emitters and the source list), buoyancy and viscous diffusion over dt_forces
void BimocqGPUSolver::applySources(bool emit, int framenum, float dt_emit, float dt_forces)
{
    if (emit) emitSmoke(framenum, dt_emit);
    addBuoyancy(dt_forces);
    confine(dt_forces);
    if (Viscosity) diffuseVelocity(dt_forces);
}

bool BimocqGPUSolver::fusedMacCormack() const
{
    return gpu_maccormack && fused_maccormack >= (myscheme == MACCORMACK ? 1 : 2);
}

// MacCormack advection of one scalar (count 1) or of three velocity-like components (count 3) through the step's
// velocity: f.field <- limit(first + 0.5 (f.adv - semilag(first, +t))), first = semilag(f.adv, -t), the limiter looking at
// f.field over dt_clamp (BimocqSolver.cpp:293-304 / :324-348, BimocqGPUSolver.cpp:237-287).
//   unfused: memset + semilag(-t), memset + semilag(+t), two adds, the limiter and a copy per field;
//   fused (fusedMacCormack()): memset + semilag(-t), then gpu_maccormack into a scratch field that becomes the field by a
//   swap (DeviceField::swap carries the ghost validity along) -- for the velocity after all three components exist, since
//   every trace reads all of them.
// Scratch: the scalars' *Temp fields and TempSrcU, the velocity's *Temp and TempSrc* fields; their contents afterwards
// differ between the two bodies and nothing reads them.
void BimocqGPUSolver::macCormack(const MacCormackFields &f, float t, float dt_clamp)
{
    gpuMapper &gs = *GpuSolver;
    const float h = CellSize;
    const int ni = g.ni, nj = g.nj, nk = g.nk;
    const bool fused = fusedMacCormack();
    // what the fused operator leaves of its inputs' ghost planes: the sample of `first` after a trace over t, the
    // limiter's corners of `lim` after one over dt_clamp, adv at the node itself
    auto fusedCall = [&](DeviceField &out, DeviceField &first, DeviceField &adv, DeviceField &lim, int dx, int dy, int dz) {
        const int rt = reach(t), rc = reach(dt_clamp);
        gs.require({ &first, &VelocityU, &VelocityV, &VelocityW }, rt);
        gs.require({ &lim, &VelocityU, &VelocityV, &VelocityW }, rc);
        gpu_maccormack(out, first, adv, lim, VelocityU, VelocityV, VelocityW, dx, dy, dz, h, ni, nj, nk, step_cfldt_, t, dt_clamp);
        const int vv = velValid();
        gs.produced(out, std::min({ std::min(first.valid, vv) - rt, std::min(lim.valid, vv) - rc, adv.valid }));
    };
    if (f.count == 1) {
        DeviceField &field = *f.field[0], &adv = *f.adv[0];
        if (fused) {
            semilagScalar(DensityTemp, adv, -t);
            fusedCall(TemperatureTemp, DensityTemp, adv, field, 0, 0, 0);
            field.swap(TemperatureTemp);
            return;
        }
        DeviceField &tmp = &field == &Temperature ? TemperatureTemp : DensityTemp;
        semilagScalar(tmp, adv, -t);
        semilagScalar(TempSrcU, tmp, t);
        axpy(tmp, TempSrcU, -0.5f, g.n());
        axpy(tmp, adv, 0.5f, g.n());
        limiter(field, tmp, 0, 0, 0, dt_clamp);
        fl_memcpy_d2d(field, tmp, g.n() * sizeof(float));
        gs.produced(field, tmp.valid);
        return;
    }
    semilagVelocity(VelocityUTemp, VelocityVTemp, VelocityWTemp, *f.adv[0], *f.adv[1], *f.adv[2], -t);
    if (fused) {
        fusedCall(TempSrcU, VelocityUTemp, *f.adv[0], *f.field[0], 1, 0, 0);
        fusedCall(TempSrcV, VelocityVTemp, *f.adv[1], *f.field[1], 0, 1, 0);
        fusedCall(TempSrcW, VelocityWTemp, *f.adv[2], *f.field[2], 0, 0, 1);
        f.field[0]->swap(TempSrcU); f.field[1]->swap(TempSrcV); f.field[2]->swap(TempSrcW);
        return;
    }
    semilagVelocity(TempSrcU, TempSrcV, TempSrcW, VelocityUTemp, VelocityVTemp, VelocityWTemp, t);
    axpy(VelocityUTemp, TempSrcU, -0.5f, g.nu()); axpy(VelocityVTemp, TempSrcV, -0.5f, g.nv()); axpy(VelocityWTemp, TempSrcW, -0.5f, g.nw());
    axpy(VelocityUTemp, *f.adv[0], 0.5f, g.nu()); axpy(VelocityVTemp, *f.adv[1], 0.5f, g.nv()); axpy(VelocityWTemp, *f.adv[2], 0.5f, g.nw());
    limiter(*f.field[0], VelocityUTemp, 1, 0, 0, dt_clamp);
    limiter(*f.field[1], VelocityVTemp, 0, 1, 0, dt_clamp);
    limiter(*f.field[2], VelocityWTemp, 0, 0, 1, dt_clamp);
    f.field[0]->copy_from(VelocityUTemp); f.field[1]->copy_from(VelocityVTemp); f.field[2]->copy_from(VelocityWTemp);
}

// the scratch scalars of both schemes and the step's bounds; false: allocation failed
bool BimocqGPUSolver::beginSchemeStep()
{
    for (DeviceField *f : { &DensityTemp, &TemperatureTemp })
        if (!f->get() && !GpuSolver->allocField(*f, FIELD_S)) return false;
    step_cfldt_ = last_cfldt = getCFL();
    step_vmax_ = MaxVelocity;
    return true;
}

// BimocqSolver.cpp:282-364 advanceMacCormack on device buffers: MacCormack advection of rho, T (:293-320) and of the
// velocity (:324-348) over the whole step through the step's old velocity, one getCFL() (:291), clearBoundary (:351),
// sources and forces (:352-361), projection (:363).  The limiter is the corrected gpu_clamp_extrema, as in the reflection
// scheme; emitters, setSources, the projection kinds and obstacles come with the shared emitSmoke / projection().
void BimocqGPUSolver::advanceMacCormack(int framenum, float dt)
{
    if (!beginSchemeStep()) return;
    moveTracers(step_cfldt_, dt);                         // through the step's old velocity, before anything writes it
    macCormack({ 1, { &Density }, { &Density } }, dt, dt);
    macCormack({ 1, { &Temperature }, { &Temperature } }, dt, dt);
    macCormack({ 3, { &VelocityU, &VelocityV, &VelocityW }, { &VelocityU, &VelocityV, &VelocityW } }, dt, dt);
    if (!boundaries.empty()) blendBoundary(false);        // clearBoundary(_rho) (:351)
    applySources(true, framenum, dt, dt);
    projection();
    steps_taken++;
}

// :232-337 advanceReflection: MacCormack advection of rho, T and of the velocity (half step),
// sources, projection, reflection 2 u_proj - u advected another half step, sources, projection.  The
// limiter is the corrected gpu_clamp_extrema (include/bimocq_gpu.h).
void BimocqGPUSolver::advanceReflection(int framenum, float dt)
{
    gpuMapper &gs = *GpuSolver;
    const bool slabs = gs.slab.on && gs.slab.nranks > 1;
    if (!beginSchemeStep()) return;                      // :234
    moveTracers(step_cfldt_, dt);                         // through the step's old velocity, before anything writes it
    const size_t nu = g.nu(), nv = g.nv(), nw = g.nw();

    macCormack({ 1, { &Density }, { &Density } }, dt, dt);                  // :237-263
    macCormack({ 1, { &Temperature }, { &Temperature } }, dt, dt);
    if (!boundaries.empty()) blendBoundary(false);        // clearBoundary (BimocqSolver.cpp:406)
    // :267-287
    macCormack({ 3, { &VelocityU, &VelocityV, &VelocityW }, { &VelocityU, &VelocityV, &VelocityW } }, 0.5f * dt, 0.5f * dt);

    applySources(true, framenum, dt, 0.5f * dt);              // :289-297
    VelocityUTemp.copy_from(VelocityU); VelocityVTemp.copy_from(VelocityV); VelocityWTemp.copy_from(VelocityW);   // :299-303
    projection();                                        // :305
    if (slabs) step_vmax_ = std::max(step_vmax_, gpu_max_abs3(VelocityU, VelocityV, VelocityW, g.ni, g.nj, g.nk));
    gpu_mad(duProj, VelocityU, VelocityUTemp, 2.f, -1.f, (int)nu);      // :307-309
    gpu_mad(dvProj, VelocityV, VelocityVTemp, 2.f, -1.f, (int)nv);
    gpu_mad(dwProj, VelocityW, VelocityWTemp, 2.f, -1.f, (int)nw);
    gs.produced(duProj, std::min(VelocityU.valid, VelocityUTemp.valid));
    gs.produced(dvProj, std::min(VelocityV.valid, VelocityVTemp.valid));
    gs.produced(dwProj, std::min(VelocityW.valid, VelocityWTemp.valid));
    // :311-325: d*Proj is advected, the limiter looks at Velocity*, which the result replaces
    macCormack({ 3, { &duProj, &dvProj, &dwProj }, { &VelocityU, &VelocityV, &VelocityW } }, 0.5f * dt, 0.5f * dt);
    applySources(false, framenum, dt, 0.5f * dt);             // :330-337
    projection();
    steps_taken++;
}

// :348-373.  The reference scans host copies that outputResult() refreshed after the previous
// frame; the same numbers are on the device at this point, so reduce them there (slab ranks reduce
// their owned planes and all-reduce the maximum).
float BimocqGPUSolver::getCFL()
{
    MaxVelocity = gpu_max_abs3(VelocityU, VelocityV, VelocityW, g.ni, g.nj, g.nk);    // includes the 1e-4 floor
    // what the map updates of this step may promise their kernels (gpuMapper::mapHints): the reduction has just read every
    // value they will read.  The library's flag is sticky, so once a NaN or an Inf has been met the plain kernels stay.
    GpuSolver->velocity_finite = !GpuSolver->slab.on && fl_nonfinite_seen && fl_nonfinite_seen(0) == 0 && MaxVelocity < 1.0e30f;
    return CellSize / MaxVelocity;
}

// :376-392 with the hard-coded scene constants replaced by the emitter list (pointwise in z)
void BimocqGPUSolver::emitSmoke(int framenum, float dt)
{
    for (const Emitter &e : sim_emitter)
        if (framenum < e.emitFrame)
            GpuSolver->emitSmoke(VelocityU, VelocityV, VelocityW, Density, Temperature,
                                 e.e_pos[0], e.e_pos[1], e.e_pos[2], e.radius, e.emit_density, e.emit_temperature, e.emiter);
    if (sources.empty()) return;
    // BimocqSolver.cpp:696-813: Emitter::update moves every source, active or not, before the active test (:698); then
    // the active ones write at the moved position, in list order (pointwise in z: ghost planes are written too)
    std::vector<bq_source> act;
    std::vector<bq_levelset> act_ls;
    for (size_t o = 0; o < sources.size(); o++) {
        bq_boundary &b = sources[o].shape;
        b.cx = b.cx + b.vx * dt;
        b.cy = b.cy + b.vy * dt;
        b.cz = b.cz + b.vz * dt;
        if (framenum >= sources[o].emit_frames) continue;
        act.push_back(sources[o]);
        if (!source_levelsets.empty()) act_ls.push_back(source_levelsets[o]);
    }
    if (!act.empty())
        gpu_emit_sources(VelocityU, VelocityV, VelocityW, Density, Temperature, act.data(), act_ls.empty() ? nullptr : act_ls.data(),
                         (int)act.size(), CellSize, g.ni, g.nj, g.nk);
}

bool BimocqGPUSolver::velocitySourceActive(int framenum) const
{
    return std::any_of(sources.begin(), sources.end(), [&](const bq_source &s) {
        return framenum < s.emit_frames && (s.flags & BQ_SOURCE_VELOCITY); });
}

// The source list replaces the previous one (n = 0: none, list and grids released).  ls[o] is read for the entries whose
// shape is BQ_SHAPE_LEVELSET, its phi a HOST array that is copied into one device allocation with every other grid of the
// list.  Any refusal leaves no sources.
bool BimocqGPUSolver::setSources(const bq_source *src, const bq_levelset *ls, int n)
{
    dropSources();
    if (n < 0 || n > BQ_MAX_SOURCES || (n > 0 && !src)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setSources: 0 .. 16 sources");
        return false;
    }
    if (n == 0) return true;
    if (!gpu_emit_sources) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setSources: the operator library has no gpu_emit_sources");
        return false;
    }
    std::vector<bq_boundary> shapes((size_t)n);
    std::vector<char> is_ls((size_t)n);
    for (int o = 0; o < n; o++) {
        const bq_source &s = src[o];
        const bq_boundary &x = shapes[o] = s.shape;
        const bool sphere = x.shape == BQ_SHAPE_SPHERE, levelset = x.shape == BQ_SHAPE_LEVELSET;
        is_ls[o] = levelset;
        const float fin[] = { x.cx, x.cy, x.cz, x.vx, x.vy, x.vz, s.density, s.temperature, s.ex, s.ey, s.ez, s.ox, s.oy, s.oz };
        const bool finite = std::all_of(std::begin(fin), std::end(fin), [](float f) { return std::isfinite(f); });
        if ((!levelset && ((!sphere && x.shape != BQ_SHAPE_BOX) || !(x.rx > 0.f) || (!sphere && !(x.ry > 0.f && x.rz > 0.f)) ||
                           !std::isfinite(x.rx) || !std::isfinite(x.ry) || !std::isfinite(x.rz))) ||
            !finite || s.emit_frames < 0 || (s.flags & ~BQ_SOURCE_VELOCITY)) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "setSources: unknown shape or flag, non-positive size, negative emit_frames or non-finite value");
            return false;
        }
    }
    const bool any_ls = std::any_of(is_ls.begin(), is_ls.end(), [](char c) { return c != 0; });
    if (any_ls && !ls) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setSources: level-set entries without descriptors");
        return false;
    }
    if (const char *why = bq::ls_check(shapes.data(), ls, n)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, (std::string("setSources: ") + why).c_str());
        return false;
    }
    DeviceBytes grids;
    std::vector<bq_levelset> descs;
    if (any_ls && !upload_levelsets(is_ls, ls, kMaxLevelsetBytes, "setSources", grids, descs)) return false;
    sources.assign(src, src + n);
    source_levelsets.swap(descs);
    source_grids = std::move(grids);
    return true;
}

void BimocqGPUSolver::dropSources()
{
    sources.clear();
    source_levelsets.clear();
    source_grids.release();
}

// :394-397 (reads rho/T at j and j-1 of the same plane: no reach along z)
void BimocqGPUSolver::addBuoyancy(float dt)
{
    GpuSolver->add_buoyancy(VelocityV, Density, Temperature, _alpha, _beta, dt);
    GpuSolver->produced(VelocityV, gpuMapper::minValid({ &VelocityV, &Density, &Temperature }));
}

bool BimocqGPUSolver::confinementOperator() { return gpu_vorticity_confinement != nullptr; }

// A refused coefficient leaves the previous one in place; 0 is accepted everywhere (the step is then exactly the one without
// this feature).
bool BimocqGPUSolver::setVorticityConfinement(float eps)
{
    if (!(eps >= 0.f) || !std::isfinite(eps)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setVorticityConfinement: the coefficient must be finite and not negative");
        return false;
    }
    if (eps != 0.f && GpuSolver->slab.on) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setVorticityConfinement: vorticity confinement is not supported on z-slab ranks");
        return false;
    }
    if (eps != 0.f && !confinementOperator()) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setVorticityConfinement: the operator library has no gpu_vorticity_confinement");
        return false;
    }
    confinement = eps;
    return true;
}

// Vorticity confinement over dt, right after the buoyancy: the operator is out of place, its outputs
// are TempSrcU/V/W, which then become the velocity by a swap, as in the fused MacCormack.  Nothing holds a value in
// TempSrc* here: advanceBimocq used them last in blendBoundary(true), which precedes the forces; macCormack() leaves them
// as scratch (both bodies), and the viscous diffusion that follows only uses them as work arrays.
void BimocqGPUSolver::confine(float dt)
{
    if (confinement == 0.f) return;
    gpu_vorticity_confinement(TempSrcU, TempSrcV, TempSrcW, VelocityU, VelocityV, VelocityW, CellSize, g.ni, g.nj, g.nk, confinement, dt);
    VelocityU.swap(TempSrcU); VelocityV.swap(TempSrcV); VelocityW.swap(TempSrcW);
}

// :399-404
void BimocqGPUSolver::diffuseField(float *field, float *t0, float *t1, int ni, int nj, int nk, int iter, float nu, float dt)
{
    float coef = nu * (dt / (CellSize * CellSize));
    GpuSolver->diffuseField(field, t0, t1, ni, nj, nk, iter, coef);
}

// :167-172: 20 diffusion sweeps per velocity component, with the reference's buffer aliasing
void BimocqGPUSolver::diffuseVelocity(float dt)
{
    const int ni = g.ni, nj = g.nj, nk = g.nk;
    if (GpuSolver->slab.on && GpuSolver->slab.nranks > 1) {
        diffuseFieldSlab(VelocityU, VelocityUTemp, TempSrcU, ni + 1, nj, nk, 20, Viscosity, dt);
        diffuseFieldSlab(VelocityV, VelocityVTemp, TempSrcV, ni, nj + 1, nk, 20, Viscosity, dt);
        diffuseFieldSlab(VelocityW, VelocityWTemp, TempSrcW, ni, nj, nk + 1, 20, Viscosity, dt);
    } else {
        diffuseField(VelocityU, VelocityUTemp, TempSrcU, ni + 1, nj, nk, 20, Viscosity, dt);
        diffuseField(VelocityV, VelocityVTemp, TempSrcV, ni, nj + 1, nk, 20, Viscosity, dt);
        diffuseField(VelocityW, VelocityWTemp, TempSrcW, ni, nj, nk + 1, 20, Viscosity, dt);
    }
}

// gpu_diffuse_field (GPU_kernel.cu:855-876) on a z-slab rank: t0 <- field, `iter` sweeps in chunks of at most G
// (one exchange of the newest iterate's ghost planes buys G sweeps, each sweep reaching one plane), field <-
// the iterate BEFORE the last one.  bk: buffer planes (nk + 1 for w).
void BimocqGPUSolver::diffuseFieldSlab(DeviceField &field, DeviceField &t0, DeviceField &t1, int bi, int bj, int bk,
                                       int iter, float nu, float dt)
{
    gpuMapper &gs = *GpuSolver;
    const int G = gs.slab.G;
    const float coef = nu * (dt / (CellSize * CellSize));
    gs.require({ &field }, G);
    t0.copy_from(field);
    DeviceField *in = &t0, *out = &t1;
    gs.produced(*out, 0);
    int left = iter;
    while (left > 0) {
        const int chunk = std::min(left, G);
        gs.require({ in }, chunk);
        const int v0 = in->valid;
        const int where = gpu_diffuse_sweeps(field, *in, *out, bi, bj, bk, chunk, coef);
        // sweep s of the chunk leaves min(v0 - s, field.valid) correct ghost planes in its output
        const int newest = std::min(v0 - chunk, field.valid), older = std::min(v0 - chunk + 1, field.valid);
        if (where) std::swap(in, out);                     // `in` = newest iterate, `out` = the one before it
        gs.produced(*in, newest);
        gs.produced(*out, chunk == 1 ? v0 : older);
        left -= chunk;
    }
    field.copy_from(*out);
}

// :406-467, the Jacobi branch (:409-410): alpha = -1, beta = 1/6
// Distortion-driven re-initialisation (BQ_OPT_REINIT_POLICY = 1): the two map sets follow different
// schedules, so the scalar advector needs its own; the scalar snapshot/delta buffers the every-frame
// policy never needs are allocated here.
bool BimocqGPUSolver::setReinitPolicy(int policy)
{
    if (policy == reinit_policy) return true;
    if (steps_taken != 0) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_REINIT_POLICY must be set before the first advance()"); return false; }
    if (policy != 0 && policy != 1) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_REINIT_POLICY: 0 or 1"); return false; }
    if (policy == 1) {
        if (!ScalarAdvector.unshareMaps()) return false;
        // z-slab ranks: maps that live for many steps must not outgrow the ghost zone -- their z-travel is measured after
        // every update and a map set is re-initialised before it would (setTravelLimit)
        if (GpuSolver->slab.on && GpuSolver->slab.nranks > 1 && travel_limit == 0) setTravelLimit(GpuSolver->slab.G);
        DeviceField *sb[] = { &DensityTemp, &TemperatureTemp, &DensityExtern, &TemperatureExtern };
        for (DeviceField *f : sb)
            if (!f->get() && !GpuSolver->allocField(*f, FIELD_S)) return false;
    } else {
        ScalarAdvector.shareMapsOf(VelocityAdvector);
    }
    reinit_policy = policy;
    return true;
}

void BimocqGPUSolver::setTravelLimit(int cells)
{
    const SlabCtx &sl = GpuSolver->slab;
    if (cells < 0) cells = 0;
    if (sl.on && sl.nranks > 1 && (cells == 0 || cells > sl.G)) cells = sl.G;      // a slab rank cannot serve more than its ghost planes
    travel_limit = cells;
    VelocityAdvector.measureTravel = ScalarAdvector.measureTravel = cells > 0;
}

// BimocqGPUSolver.cpp:60-90: p, dir, residual, div, temp0, temp1 (N doubles each), tempResult (4096), and
// LEVEL_COUNT levels of b/x/r with dims n -> (n - 1) / 2.  Levels without a single cell are left out (the
// reference launches empty grids for them).
bool BimocqGPUSolver::allocMgcg()
{
    if (mg.ready) return true;
    // temp1 and levels[0].b below are full-size arrays: the operator may keep its fused level-0 vectors in them
    // (include/bimocq_gpu.h, FL_OPT_MGCG_FUSE; -1 = nobody has set the option)
    if (fl_get_option(FL_OPT_MGCG_FUSE) < 0) fl_set_option(FL_OPT_MGCG_FUSE, 1);
    // a z-slab rank solves on the WHOLE grid (projectionMgcgSlabs): global plane count
    const bool slabs = GpuSolver->slab.on && GpuSolver->slab.nranks > 1;
    const int nk_all = slabs ? GpuSolver->slab.nkg : g.nk;
    const size_t n = (size_t)g.ni * g.nj * nk_all;
    DeviceBytes *full[] = { &mg.div, &mg.p, &mg.dir, &mg.residual, &mg.temp0, &mg.temp1 };
    for (DeviceBytes *f : full)
        if (!f->alloc(n * sizeof(double))) return false;
    if (!mg.result.alloc(4096 * sizeof(double))) return false;
    int ni = g.ni, nj = g.nj, nk = nk_all;
    for (int l = 0; l < LEVEL_COUNT; l++) {
        if (l) { ni = (ni - 1) / 2; nj = (nj - 1) / 2; nk = (nk - 1) / 2; }
        if (ni < 1 || nj < 1 || nk < 1) break;
        SCoarseLevelInfo L{};
        L.ni = ni; L.nj = nj; L.nk = nk; L.number = ni * nj * nk;
        L.alpha = -1.0; L.beta = 1.0 / 6.0;
        mg.b.emplace_back(); mg.x.emplace_back(); mg.r.emplace_back();
        const size_t bytes = (size_t)L.number * sizeof(double);
        if (!mg.b.back().alloc(bytes) || !mg.x.back().alloc(bytes) || !mg.r.back().alloc(bytes)) return false;
        L.b = mg.b.back().f64(); L.x = mg.x.back().f64(); L.r = mg.r.back().f64();
        mg.levels.push_back(L);
    }
    if (slabs) {
        if (!mg.gu.alloc((size_t)(g.ni + 1) * g.nj * nk_all) || !mg.gv.alloc((size_t)g.ni * (g.nj + 1) * nk_all) ||
            !mg.gw.alloc((size_t)g.ni * g.nj * (nk_all + 1))) return false;
    }
    mg.ready = true;
    return true;
}

// The multigrid-CG projection on z-slab ranks, REPLICATED: every rank assembles the velocity of the whole grid (its own planes
// + one point-to-point message per peer and component, a single RCCL group: xGMI is a full mesh), runs the very solver a
// single GPU runs on it (slab context off) and takes its own planes, ghost planes included, back.  Bit-identical to one GPU
// by construction -- the reference's float-narrowed dot products, its level pyramid n -> (n - 1) / 2 and its interpolation
// quirks all see the global arrays -- and the first step towards a slab-decomposed V-cycle: the advection
// scales with the rank count, the solve does not (it costs what it costs on one GPU, plus ~1 ms of gather).
bool BimocqGPUSolver::projectionMgcgSlabs()
{
    gpuMapper &gs = *GpuSolver;
    const SlabCtx &sl = gs.slab;
    const int G = sl.G, nkg = sl.nkg, R = sl.nranks;
    const bool last = sl.own1 == nkg;
    struct Comp { DeviceField *loc, *glob; size_t plane; int extra; } comps[3] = {
        { &VelocityU, &mg.gu, (size_t)(g.ni + 1) * g.nj, 0 }, { &VelocityV, &mg.gv, (size_t)g.ni * (g.nj + 1), 0 },
        { &VelocityW, &mg.gw, (size_t)g.ni * g.nj, 1 } };
    // planes rank r owns of a component: its cell planes, the w face on top of the grid goes to the last rank
    const auto own0_of = [&](int r) { return r * (nkg / R); };
    const auto planes_of = [&](int r, int extra) { return nkg / R + ((extra && r == R - 1) ? 1 : 0); };
    std::vector<int> peers; std::vector<float *> send, recv; std::vector<size_t> send_count, recv_count;
    for (const Comp &c : comps) {
        const size_t mine = c.plane * (size_t)planes_of(sl.rank, c.extra);
        fl_memcpy_d2d(c.glob->get() + c.plane * (size_t)sl.own0, c.loc->get() + c.plane * (size_t)G, mine * sizeof(float));
    }
    for (int r = 0; r < R; r++) {
        if (r == sl.rank) continue;
        for (const Comp &c : comps) {
            peers.push_back(r);
            send.push_back(c.loc->get() + c.plane * (size_t)G);
            send_count.push_back(c.plane * (size_t)planes_of(sl.rank, c.extra));
            recv.push_back(c.glob->get() + c.plane * (size_t)own0_of(r));
            recv_count.push_back(c.plane * (size_t)planes_of(r, c.extra));
        }
    }
    fl_p2p_exchange((int)peers.size(), peers.data(), send.data(), send_count.data(), recv.data(), recv_count.data());
    (void)last;
    fl_set_slab(0, 0, 0, 0, 0);                                         // the solve sees one global grid
    gpu_multi_grid_conjugate_gradient(mg.gu, mg.gv, mg.gw, mg.div.f64(), mg.p.f64(), mg.dir.f64(),
                                      mg.residual.f64(), mg.temp0.f64(), mg.temp1.f64(), mg.result.f64(),
                                      mg.levels.data(), (int)mg.levels.size(), mg_iters, (double)halfrdx);
    fl_set_slab(sl.koff(), sl.nkg, sl.own0, sl.own1, sl.nk_local());
    // the projected velocity on this rank's planes, ghost planes included (those outside the grid stay zero)
    const int k0 = std::max(sl.own0 - G, 0), k1 = std::min(sl.own1 + G, nkg);
    for (const Comp &c : comps) {
        const int np = k1 - k0 + ((c.extra && k1 == nkg) ? 1 : 0);
        fl_memcpy_d2d(c.loc->get() + c.plane * (size_t)(k0 - (sl.own0 - G)), c.glob->get() + c.plane * (size_t)k0,
                      c.plane * (size_t)np * sizeof(float));
        gs.produced(*c.loc, G);
    }
    return fl_last_error() == FL_OK;
}

// The multigrid-CG projection on z-slab ranks with the fine levels SHARED (round 4: include/bimocq_gpu.h,
// gpu_multi_grid_conjugate_gradient_slab; csrc/bq_mgcg_slab.hip.inc): nothing global is allocated here -- the operator owns its
// per-level slab arrays -- and the velocity needs its ghost planes only as deep as level 0's (8).  false when the decomposition
// is not covered (planes that are not a multiple of 256 cells, thin slabs or slabs of no multiple of 8 planes, the CPU
// stand-in): the caller falls back to the replicated solve, which is bit-identical.  Both are collectives, so the choice must
// be the same on every rank: the predicate is asked with the communicator's rank and size -- exactly what the operator will
// consult (csrc/bq_mgcg_slab_plan.h: an answer that depends on the grid and the number of ranks alone) -- and an operator that
// refuses all the same (FL_ERR_UNSUPPORTED: the predicate or the plan, computed alike on every rank) is not a projection: the
// error is cleared and the replicated solve runs.  Any other error stays latched, and nothing counts as projected.
bool BimocqGPUSolver::projectionMgcgShared()
{
    gpuMapper &gs = *GpuSolver;
    const SlabCtx &sl = gs.slab;
    mgcg_shared_ran = false;
    if (!mgcg_shared || !gpu_mgcg_slab_supported(g.ni, g.nj, sl.nkg, sl.own0, sl.own1, sl.G, fl_comm_rank(), fl_comm_size())) return false;
    if (mg.result.bytes() < 4096 * sizeof(double) && !mg.result.alloc(4096 * sizeof(double))) return false;
    gs.require({ &VelocityU, &VelocityV, &VelocityW }, sl.G);
    const int before = fl_last_error();                     // (an earlier failure stays what it is: the refusal below cannot be told from it)
    gpu_multi_grid_conjugate_gradient_slab(VelocityU, VelocityV, VelocityW, mg.result.f64(), g.ni, g.nj, sl.nkg, sl.own0, sl.own1, sl.G,
                                           mg_iters, (double)halfrdx);
    if (const int err = before == FL_OK ? fl_last_error() : FL_OK) {
        if (err != FL_ERR_UNSUPPORTED) return true;         // local to this rank (an allocation): latched, nothing projected
        fl_clear_error();
        return false;
    }
    // projected on the owned planes and on the 7 ghost planes next to them (the gradient needs p one plane below)
    const int depth = std::min(sl.G, 8) - 1;
    gs.produced(VelocityU, depth); gs.produced(VelocityV, depth); gs.produced(VelocityW, depth);
    mgcg_shared_ran = true;
    return true;
}

std::vector<double> BimocqGPUSolver::mgHistory() const
{
    std::vector<double> h(4096, 0.0);
    if (mg.result.bytes() >= h.size() * sizeof(double)) fl_memcpy_d2h(h.data(), mg.result.f64(), h.size() * sizeof(double));
    return h;
}

// setBoundary (BimocqSolver.cpp:936-1064 without the domain walls): the list replaces the previous one, the flags are built
// at the given centres.  n = 0 removes every obstacle and the step is exactly the one without this feature.  ls[o] is read
// for the entries of shape BQ_SHAPE_LEVELSET ("Level sets"), its phi a HOST array that is copied into
// one device allocation with every other grid of the list.  pose (NULL: none): one orientation and
// angular velocity per entry; the quaternions become the double master copies that updateBoundary integrates.  A refused
// list leaves the previous one in place.
bool BimocqGPUSolver::setBoundary(const bq_boundary *b, const bq_levelset *ls, int n, const bq_pose *pose)
{
    if (n < 0 || n > BQ_MAX_BOUNDARIES || (n > 0 && !b)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setBoundary: 0 .. 16 obstacles");
        return false;
    }
    if (n == 0) {
        dropBoundaries();
        return buildWallFlags();
    }
    if (GpuSolver->slab.on) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setBoundary: obstacles are not supported on z-slab ranks");
        return false;
    }
    if (projection_kind == BQ_PROJECTION_MGCG) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setBoundary: obstacles need the Jacobi projection (not BQ_PROJECTION_MGCG)");
        return false;
    }
    if (!gpu_obstacle_flags || !gpu_obstacle_faces || !gpu_jacobi_sweeps_masked || !gpu_gradient_masked || !gpu_semilag_band ||
        !gpu_obstacle_blend) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setBoundary: the operator library has no obstacle operators");
        return false;
    }
    const bool any_ls = std::any_of(b, b + n, [](const bq_boundary &x) { return x.shape == BQ_SHAPE_LEVELSET; });
    if (any_ls && !ls) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setBoundary: level-set entries without descriptors");
        return false;
    }
    if (any_ls && (!gpu_obstacle_flags_ls || !gpu_semilag_band_ls || !gpu_obstacle_blend_ls)) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setBoundary: the operator library has no level-set obstacle operators");
        return false;
    }
    for (int o = 0; o < n; o++) {
        const bq_boundary &x = b[o];
        const bool sphere = x.shape == BQ_SHAPE_SPHERE, levelset = x.shape == BQ_SHAPE_LEVELSET;   // a level set has no radii
        if ((!levelset && ((!sphere && x.shape != BQ_SHAPE_BOX) || !(x.rx > 0.f) || (!sphere && !(x.ry > 0.f && x.rz > 0.f)) ||
                           !std::isfinite(x.rx) || !std::isfinite(x.ry) || !std::isfinite(x.rz))) ||
            !std::isfinite(x.cx) || !std::isfinite(x.cy) || !std::isfinite(x.cz) || !std::isfinite(x.vx) ||
            !std::isfinite(x.vy) || !std::isfinite(x.vz)) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "setBoundary: unknown shape, non-positive size or non-finite value");
            return false;
        }
    }
    if (const char *why = bq::ls_check(b, ls, n)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, (std::string("setBoundary: ") + why).c_str());
        return false;
    }
    if (const char *why = bq::pose_check(pose, n)) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, (std::string("setBoundary: ") + why).c_str());
        return false;
    }
    const bool posed = bq::pose_any(b, pose, n);
    if (posed && (!gpu_obstacle_flags_pose || !gpu_semilag_band_pose || !gpu_obstacle_blend_pose || !gpu_obstacle_faces_pose)) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setBoundary: the operator library has no pose operators (rotating obstacles)");
        return false;
    }
    // every grid into one allocation, the descriptors pointing into it
    DeviceBytes grids;
    std::vector<bq_levelset> descs;
    if (any_ls) {
        std::vector<char> is_ls((size_t)n);
        for (int o = 0; o < n; o++) is_ls[o] = b[o].shape == BQ_SHAPE_LEVELSET;
        if (!upload_levelsets(is_ls, ls, kMaxLevelsetBytes, "setBoundary", grids, descs)) return false;
    }
    const size_t nrows = (size_t)g.nj * (size_t)g.nk;
    if (solid.bytes() != g.n() && !solid.alloc(g.n())) return false;
    if (rows.bytes() != nrows && !rows.alloc(nrows)) return false;
    std::vector<bq_boundary> list(b, b + n);
    std::vector<bq_pose> pl((size_t)n, bq_pose{ 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f });
    if (pose) pl.assign(pose, pose + n);
    if (!buildFlags(list, any_ls ? descs.data() : nullptr, posed ? pl.data() : nullptr)) return false;
    boundaries.swap(list);
    levelsets.swap(descs);
    orientations.resize((size_t)n);
    for (int o = 0; o < n; o++) orientations[(size_t)o] = { (double)pl[o].qw, (double)pl[o].qx, (double)pl[o].qy, (double)pl[o].qz };
    poses.swap(pl);
    posed_list = posed;
    lsgrids = std::move(grids);
    return buildWallFlags();
}

// no obstacles: the list, the flags, the rows summary and the level-set grids released
void BimocqGPUSolver::dropBoundaries()
{
    boundaries.clear();
    levelsets.clear();
    poses.clear();
    orientations.clear();
    posed_list = false;
    solid.release();
    rows.release();
    lsgrids.release();
}

// the flags of `list` (ls: its level-set descriptors, or NULL when it holds none); on failure the obstacles are dropped (no
// step may run on flags that were never built)
bool BimocqGPUSolver::buildFlags(const std::vector<bq_boundary> &list, const bq_levelset *ls, const bq_pose *pose)
{
    obstacle_flags(solid.u8(), rows.u8(), list.data(), (int)list.size(), ls, pose, CellSize, g.ni, g.nj, g.nk);
    if (fl_last_error() == FL_OK) return true;
    dropBoundaries();
    dropWalls();                                    // (solidw held the flags of the list that is gone)
    return false;
}

// updateBoundary: Boundary::update (BimocqSolver.h:71-73, b_pos += vel_func(framenum) * dt) with the velocity of the list,
// then the flags at the new centres.  A spinning entry turns by theta = |omega| dt about omega:
// q <- dq (x) q with dq = (cos(theta/2), sin(theta/2) omega/|omega|), renormalised, all in double on the master copy; the
// four floats the operators see are rounded from it, so nothing drifts.  Zero omega leaves q's bits alone.
bool BimocqGPUSolver::updateBoundary(int /*framenum*/, float dt)
{
    if (boundaries.empty()) return true;
    std::vector<bq_boundary> list = boundaries;
    for (bq_boundary &b : list) {
        b.cx += b.vx * dt;
        b.cy += b.vy * dt;
        b.cz += b.vz * dt;
    }
    if (!posed_list) {
        if (!buildFlags(list, levelsetList(), nullptr)) return false;
        boundaries.swap(list);
        return buildWallFlags();
    }
    std::vector<bq_pose> pl = poses;
    std::vector<std::array<double, 4>> ql = orientations;
    for (size_t o = 0; o < pl.size(); o++) {
        if (!bq::pose_spins(pl[o])) continue;
        const double ox = pl[o].ox, oy = pl[o].oy, oz = pl[o].oz, len = std::sqrt(ox * ox + oy * oy + oz * oz);
        const double half = 0.5 * len * (double)dt, sn = std::sin(half) / len;
        const double a = std::cos(half), bx = sn * ox, by = sn * oy, bz = sn * oz;       // dq
        const std::array<double, 4> q = ql[o];
        double w = a * q[0] - bx * q[1] - by * q[2] - bz * q[3];
        double x = a * q[1] + bx * q[0] + by * q[3] - bz * q[2];
        double y = a * q[2] - bx * q[3] + by * q[0] + bz * q[1];
        double z = a * q[3] + bx * q[2] - by * q[1] + bz * q[0];
        const double norm = std::sqrt(w * w + x * x + y * y + z * z);
        ql[o] = { w / norm, x / norm, y / norm, z / norm };
        pl[o].qw = (float)ql[o][0]; pl[o].qx = (float)ql[o][1]; pl[o].qy = (float)ql[o][2]; pl[o].qz = (float)ql[o][3];
    }
    if (!buildFlags(list, levelsetList(), pl.data())) return false;
    boundaries.swap(list);
    poses.swap(pl);
    orientations.swap(ql);
    return buildWallFlags();
}

bool BimocqGPUSolver::wallOperators()
{
    return gpu_wall_flags && gpu_wall_faces && gpu_jacobi_sweeps_masked_walls && gpu_gradient_masked_walls &&
           (!pcgOperators() || gpu_pcg_gradient_walls);
}

// setWalls (BimocqSolver.cpp:938-948 as an opt-in): the closed sides; 0 releases solidw and the step is exactly the one without
// this feature.  A refused mask leaves the previous one in place.  On a z-slab rank solidw covers the rank's local planes, with
// the walls where the GLOBAL grid has them (gpu_wall_flags reads the slab context), and `rows` is all zero: no obstacles there.
bool BimocqGPUSolver::setWalls(int mask)
{
    if (mask < 0 || mask > 63) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setWalls: bits outside BQ_WALL_XLO .. BQ_WALL_ZHI");
        return false;
    }
    if (mask == 63) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "setWalls: all six sides closed (the pressure needs one open side as its reference)");
        return false;
    }
    if (mask == 0) {
        dropWalls();
        return true;
    }
    if (projection_kind == BQ_PROJECTION_MGCG) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setWalls: walls need the Jacobi or the PCG projection (not BQ_PROJECTION_MGCG)");
        return false;
    }
    if (!wallOperators()) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setWalls: the operator library has no wall operators");
        return false;
    }
    // z-slab ranks: a library with the two range operators promises that its wall operators honour the slab context
    // (include/bimocq_gpu.h); any other would put a wall on every rank's first and last local plane
    if (GpuSolver->slab.on && !(gpu_jacobi_sweep_masked_walls_range && gpu_jacobi_sweep_masked_walls_triple_ranges)) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setWalls: the operator library has no wall operators for z-slab ranks");
        return false;
    }
    if (GpuSolver->slab.on && projection_kind != BQ_PROJECTION_JACOBI) {
        fl_report_error(FL_ERR_UNSUPPORTED, "setWalls: walls on z-slab ranks need the Jacobi projection");
        return false;
    }
    const size_t nrows = (size_t)g.nj * (size_t)g.nk;
    DeviceBytes sw, rw;
    if (!sw.alloc(g.n())) return false;
    if (boundaries.empty()) {                       // the obstacles' rows summary of an empty list: all zero
        if (!rw.alloc(nrows)) return false;
        fl_memset(rw.u8(), 0, nrows);
        if (fl_last_error() != FL_OK) return false;
    }
    gpu_wall_flags(sw.u8(), boundaries.empty() ? nullptr : solid.u8(), mask, g.ni, g.nj, g.nk);
    if (fl_last_error() != FL_OK) return false;
    solidw = std::move(sw);
    if (boundaries.empty()) rows = std::move(rw);
    walls = mask;
    return true;
}

void BimocqGPUSolver::dropWalls()
{
    walls = 0;
    solidw.release();
    if (boundaries.empty()) rows.release();
}

// solidw from the current obstacle flags (after setBoundary / updateBoundary); nothing to do with walls off
bool BimocqGPUSolver::buildWallFlags()
{
    if (!walls) return true;
    const size_t nrows = (size_t)g.nj * (size_t)g.nk;
    bool ok = true;
    if (boundaries.empty()) {
        ok = rows.bytes() == nrows || rows.alloc(nrows);
        if (ok) fl_memset(rows.u8(), 0, nrows);
    }
    if (ok) gpu_wall_flags(solidw.u8(), boundaries.empty() ? nullptr : solid.u8(), walls, g.ni, g.nj, g.nk);
    if (ok && fl_last_error() == FL_OK) return true;
    dropWalls();
    return false;
}

// the semi-Lagrangian values of blendBoundary (BimocqSolver.cpp:106): u, v, w, rho, T traced back over dt, at band nodes only,
// into scratch fields the step does not read before the blend consumes them
void BimocqGPUSolver::semilagBand(float cfldt, float dt)
{
    gpuMapper &gs = *GpuSolver;
    for (DeviceField *f : { &DensityTemp, &TemperatureTemp })
        if (!f->get() && !gs.allocField(*f, FIELD_S)) return;
    const bq_boundary *b = boundaries.data();
    const int n = (int)boundaries.size(), ni = g.ni, nj = g.nj, nk = g.nk;
    const bq_levelset *ls = levelsetList();
    const bq_pose *pose = poseList();
    const float h = CellSize;
    semilag_band(TempSrcU, VelocityU, VelocityU, VelocityV, VelocityW, 1, 0, 0, h, ni, nj, nk, cfldt, -dt, b, n, ls, pose);
    semilag_band(TempSrcV, VelocityV, VelocityU, VelocityV, VelocityW, 0, 1, 0, h, ni, nj, nk, cfldt, -dt, b, n, ls, pose);
    semilag_band(TempSrcW, VelocityW, VelocityU, VelocityV, VelocityW, 0, 0, 1, h, ni, nj, nk, cfldt, -dt, b, n, ls, pose);
    semilag_band(DensityTemp, Density, VelocityU, VelocityV, VelocityW, 0, 0, 0, h, ni, nj, nk, cfldt, -dt, b, n, ls, pose);
    semilag_band(TemperatureTemp, Temperature, VelocityU, VelocityV, VelocityW, 0, 0, 0, h, ni, nj, nk, cfldt, -dt, b, n, ls, pose);
}

// blendBoundary (:879-912) of all five fields from semilagBand's values + clearBoundary (:914-934) of rho; band = false:
// the clear only (the reflection scheme has no blend)
void BimocqGPUSolver::blendBoundary(bool band)
{
    const bq_boundary *b = boundaries.data();
    const int n = (int)boundaries.size();
    if (band)
        obstacle_blend(VelocityU, VelocityV, VelocityW, Density, Temperature, TempSrcU, TempSrcV, TempSrcW, DensityTemp,
                       TemperatureTemp, solid.u8(), b, n, levelsetList(), poseList(), CellSize, g.ni, g.nj, g.nk);
    else
        obstacle_blend(nullptr, nullptr, nullptr, Density, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       solid.u8(), b, n, levelsetList(), poseList(), CellSize, g.ni, g.nj, g.nk);
}

bool BimocqGPUSolver::pcgOperators() { return gpu_divergence_double && gpu_pcg_solve && gpu_pcg_gradient; }

// BQ_PROJECTION_PCG: solid faces (obstacles only), fp64 divergence, the solve to pcg_tol, the masked
// gradient.  d*Proj comes from the snapshot the caller takes before this call (as for the MGCG projection).
bool BimocqGPUSolver::projectionPcg()
{
    if (!allocMgcg()) return false;
    const ProjectionOps ops(*this);
    ops.faces(nullptr, nullptr, nullptr);
    gpu_divergence_double(VelocityU, VelocityV, VelocityW, mg.div.f64(), g.ni, g.nj, g.nk, (double)halfrdx);
    SCoarseLevelInfo &L0 = mg.levels[0];
    gpu_pcg_solve(mg.div.f64(), mg.p.f64(), ops.flags, mg.residual.f64(), mg.dir.f64(), mg.temp0.f64(), mg.temp1.f64(), L0.b, L0.r,
                  mg.levels.data(), (int)mg.levels.size(), pcg_iters, pcg_tol, pcg_stats);
    if (fl_last_error() != FL_OK) return false;
    pcg_projections++;
    if (pcg_stats[3] != BQ_PCG_CONVERGED) pcg_unconverged++;
    ops.gradient(mg.p.f64());
    if (load_open && !boundaries.empty()) sampleLoads(nullptr, mg.p.f64());
    return false;
}

// with_delta: d*Proj = (projected - unprojected) velocity comes out of the gradient pass itself
// (gpu_gradient_delta) instead of a snapshot before and a subtraction after; Jacobi branch only (returns
// whether it did).
bool BimocqGPUSolver::projection(bool with_delta)
{
    const gpuMapper &gs = *GpuSolver;
    const bool slabs = gs.slab.on && gs.slab.nranks > 1;
    if (projection_kind == BQ_PROJECTION_PCG) return projectionPcg();   // (refused on slabs by bq_solver_set_projection)
    if (projection_kind == BQ_PROJECTION_MGCG) {            // :443-446
        if (slabs && projectionMgcgShared()) return false;
        if (!allocMgcg()) return false;
        if (slabs) projectionMgcgSlabs();
        else gpu_multi_grid_conjugate_gradient(VelocityU, VelocityV, VelocityW, mg.div.f64(), mg.p.f64(), mg.dir.f64(),
                                               mg.residual.f64(), mg.temp0.f64(), mg.temp1.f64(), mg.result.f64(),
                                               mg.levels.data(), (int)mg.levels.size(), mg_iters, (double)halfrdx);
        return false;
    }
    if (slabs) return projectionJacobiSlabs(with_delta);                 // (walls included; setBoundary refuses slab ranks)
    return projectionJacobi(with_delta);
}

// One GPU, every family (:1120-1413 with obstacles): gpu_projection_jacobi (GPU_kernel.cu:1839-1895) in its pieces -- solid faces
// (with_delta: their share of d*Proj), divergence, iter-1 sweeps, the newest iterate made `p` by a buffer swap instead
// of the copy-back, gradient on the faces between fluid cells with the change handed out
bool BimocqGPUSolver::projectionJacobi(bool with_delta)
{
    const ProjectionOps ops(*this);
    if (ops.kind == ProjectionOps::kPlain && !with_delta) {              // the reference's own entry point
        GpuSolver->projectionJacobi(VelocityU, VelocityV, VelocityW, div, p, p_temp, debugParam, jacobi_iters, halfrdx, ops.alpha, ops.beta);
        return false;
    }
    float *du = with_delta ? duProj.get() : nullptr, *dv = with_delta ? dvProj.get() : nullptr, *dw = with_delta ? dwProj.get() : nullptr;
    div.zero(); p.zero(); p_temp.zero();                                 // GPU_Advection.h:604-606
    ops.faces(du, dv, dw);
    gpu_divergence(VelocityU, VelocityV, VelocityW, div, g.ni, g.nj, g.nk, halfrdx);
    int where = 0;
    if (jacobi_iters > 1) {
        JacobiFuseVouched same_shell;       // p and p_temp carry the same (zero) boundary layer and +0 in every solid cell: sweeps may share a launch
        where = ops.sweeps(p, p_temp, jacobi_iters - 1);
    }
    if (where) p.swap(p_temp);
    ops.gradient(p, du, dv, dw);
    if (load_open && !boundaries.empty()) sampleLoads(p, nullptr);
    return with_delta;
}

// z-slab form of gpu_projection_jacobi (GPU_kernel.cu:1839-1895): same three kernels, with the sweeps issued in chunks of G:
// one exchange of G ghost planes of p buys G sweeps, because each sweep shrinks the correct ghost depth by one plane (the ghost
// planes are swept redundantly, which yields the very values the neighbour computes).  What a chunk consists of is stated in
// slab_jacobi_plan.hpp; this function issues it and keeps the plan's two permissions up to date when the library refuses a launch.
// WALLS ON: the same loop on the plan's walled mode with the walled launches -- the wall faces first
// (with_delta: their share of d*Proj), one sweep or three per launch on the same plane ranges, the walled gradient last.  Every
// wall operator places the walls by the global plane, so the ghost planes are swept to the values their owner computes.
bool BimocqGPUSolver::projectionJacobiSlabs(bool with_delta)
{
    gpuMapper &gs = *GpuSolver;
    const int G = gs.slab.G;
    const ProjectionOps ops(*this);
    const bool walled = ops.kind == ProjectionOps::kWalled;              // (for the schedule and the ghost-plane bookkeeping only)
    float *du = with_delta ? duProj.get() : nullptr, *dv = with_delta ? dvProj.get() : nullptr, *dw = with_delta ? dwProj.get() : nullptr;
    // The redundant ghost sweeps need div on all G ghost planes.  Rather than refreshing three velocity components to
    // depth G and evaluating div there, div is evaluated where the velocities are valid (the owned planes need one ghost
    // plane of w) and its own ghost planes are fetched: one field instead of three, the same values (a neighbour's
    // owned-plane divergence is the very expression this rank would evaluate).
    gs.require({ &VelocityU, &VelocityV, &VelocityW }, 1);
    div.zero(); p.zero(); p_temp.zero();                                 // GPU_Advection.h:604-606
    // a pointwise pass on the faces of the window; the w face between the window and a closed z plane just outside it is the one
    // the wall pass cannot decide (gpu_wall_faces): w's outermost ghost plane no longer counts
    ops.faces(du, dv, dw);
    if (walled) gs.produced(VelocityW, std::min(VelocityW.valid, G - 1));
    gpu_divergence(VelocityU, VelocityV, VelocityW, div, g.ni, g.nj, g.nk, halfrdx);
    gs.produced(div, std::min({ VelocityU.valid, VelocityV.valid, VelocityW.valid - 1 }));
    gs.require({ &div }, G);
    DeviceField *cur = &p, *oth = &p_temp;
    gs.produced(*cur, G);                                                // zeros everywhere
    const int own0 = G, own1 = g.nk - G;                                 // local owned planes [own0, own1)
    // the G ghost planes of `f` start travelling on the halo stream; fl_halo_wait (or the next blocking exchange) joins them
    auto startExchange = [&](DeviceField &f) {
        float *ptr = f.get(); size_t pe = f.plane; int ex = 0;
        fl_halo_exchange(1, &ptr, &pe, &ex, g.nk, G, G, /*wait=*/0);
    };
    // The exchange a chunk starts with is hidden by the interior part of its first pass only -- one launch (40 us at 512 x 512 x 80)
    // against 8 planes per direction (130 us at 64 GB/s).  ENDS FIRST, for the last two passes A and B of a chunk that another
    // chunk follows: both on the planes next to the slab ends (which need nothing beyond what the pass before produced; B's are
    // the planes the neighbours receive), the exchange of those now final planes starts, and the two interiors plus the interior
    // of the next chunk's first pass run while it travels (three launches instead of one).  A's interior reads `in` from plane
    // own0 + G on, which is where B's end stopped writing it.  d: ghost planes correct after A.  The newest iterate is back in `in`.
    // All four launches apply or none: the same kernel on the same rows either takes every one of these ranges or refuses the
    // first; a later refusal would leave `in` half-updated, so it is an error, not a fall-back.
    auto endsFirst = [&](int S, DeviceField &in, DeviceField &out, int d) {
        const slab::Ends ea = slab::ends(own0, own1, G, d), eb = slab::ends(own0, own1, G, d - S);
        if (!ops.fused(S, in, out, ea.a, ea.b)) return false;
        bool later = ops.fused(S, out, in, eb.a, eb.b);
        startExchange(in);
        later &= ops.fused(S, in, out, slab::interior(own0, own1, G, d));
        later &= ops.fused(S, out, in, slab::interior(own0, own1, G, d - S));
        if (!later) fl_report_error(FL_ERR_UNSUPPORTED, "projection on slabs: a follow-up launch of an ends-first group was refused after the first one ran");
        return true;
    };
    JacobiFuseVouched same_shell;                                        // p and p_temp carry the same (zero) boundary layer: gpu_jacobi_sweeps may fuse
    slab::ChunkIn plan{};
    plan.left = jacobi_iters - 1;                                        // iterate iter-1 is applied
    plan.G = G; plan.owned = own1 - own0;
    plan.pairs_ok = G >= 2 && own1 - own0 >= 5;                          // until the operator library says it cannot
    plan.triples_ok = true;                                              // likewise
    plan.overlap_exchanges = gs.overlap_exchanges; plan.triples = gs.jacobi_triples;
    plan.ends_first = walled ? gs.jacobi_ends_first_walled : gs.jacobi_ends_first;
    plan.walled = walled;
    bool in_flight = false;                                              // the exchange of `cur`'s ghost planes has been started
    while (plan.left > 0) {
        int where, chunk;
        if (!in_flight && cur->valid >= std::min(plan.left, G)) {
            chunk = std::min(plan.left, G);
            where = ops.sweeps(*cur, *oth, chunk);
        } else {
            // The ghost planes of `cur` travel on the halo stream while the compute stream sweeps what does not
            // depend on them; the planes next to them follow the exchange.
            if (!in_flight) startExchange(*cur);
            in_flight = false;
            slab::Chunk c = slab::plan_chunk(plan);
            if (c.first == 2 && !ops.fused(2, *cur, *oth, slab::first_interior(own0, own1, 2))) {
                plan.pairs_ok = false;                                   // the fused kernel does not apply to this grid
                c = slab::plan_chunk(plan);
            }
            const slab::Ends fe = slab::first_ends(own0, own1, g.nk, c.first);
            if (c.first == 1) ops.single(*cur, *oth, slab::first_interior(own0, own1, 1));
            fl_halo_wait();
            gs.produced(*cur, G);
            if (c.first == 2) ops.fused(2, *cur, *oth, fe.a, fe.b);          // (one launch for both ends)
            else { ops.single(*cur, *oth, fe.a); ops.single(*cur, *oth, fe.b); }
            // The remaining sweeps of the chunk start from `oth`.  Nothing reads the planes beyond the depth that stays correct:
            // every fused pass is restricted to the planes that will still be correct after it (G = 8 in pairs: 264, 260, 256 of
            // 272 planes).
            DeviceField *in = oth, *out = cur;
            int d = G - c.first;                                         // correct ghost planes of `in`
            for (int i = 0; i < c.fused;) {
                const bool group = c.ends_first && i == c.fused - 2;     // this pass and the next, ends first
                const bool ran = group ? endsFirst(c.S, *in, *out, d - c.S) : ops.fused(c.S, *in, *out, slab::whole(own0, own1, d - c.S));
                if (!ran && c.S == 3 && i == 0) {                        // the kernels do not apply to this grid: pairs from now on
                    plan.triples_ok = false;
                    c = slab::plan_chunk(plan);
                    continue;
                }
                if (!ran && c.S == 3)
                    fl_report_error(FL_ERR_UNSUPPORTED, "projection on slabs: the second three-sweep launch was refused after the first one ran");
                if (!ran) break;                                         // what is left of the chunk goes to gpu_jacobi_sweeps
                if (group) in_flight = true;                             // (two launches per piece: the newest iterate is back in `in`)
                else std::swap(in, out);
                const int passes = group ? 2 : 1;
                i += passes; d -= passes * c.S;
            }
            const int rest = c.sweeps - (G - d);
            const int w2 = rest > 0 ? ops.sweeps(*in, *out, rest) : 0;
            DeviceField *newest = w2 ? out : in;
            where = newest == cur ? 0 : 1;
            chunk = c.sweeps;
        }
        int v = cur->valid;
        for (int s = 0; s < chunk; s++) v = std::min(v - 1, div.valid);     // each sweep reaches one plane
        if (where) std::swap(cur, oth);
        gs.produced(*cur, v);
        gs.produced(*oth, 0);
        plan.left -= chunk;
    }
    if (cur != &p) p.swap(p_temp);                                       // the newest iterate becomes `p` (no copy-back)
    gs.require({ &p }, 1);
    const int vu = std::min(VelocityU.valid, p.valid), vv = std::min(VelocityV.valid, p.valid), vw = std::min(VelocityW.valid, p.valid - 1);
    ops.gradient(p, du, dv, dw);
    if (with_delta) { gs.produced(duProj, vu); gs.produced(dvProj, vv); gs.produced(dwProj, vw); }
    gs.produced(VelocityU, vu);
    gs.produced(VelocityV, vv);
    gs.produced(VelocityW, vw);
    return with_delta;
}

// The two-level advection of blend != 1 (Mapping.cpp:383-390) samples the *Prev fields through the previous backward map.  With
// the reference's zeroed map border a look-up that meets border cells returns s * q, s in [0, 1]: anywhere between
// the origin and the node -- on a z-slab rank, on any other rank's planes.  The *Prev fields change at a re-initialisation and
// nowhere else, so that is when every rank assembles whole-grid copies of them (gpuMapper::assembleGlobal: one message per peer
// and field); the advectors find the copies through gpuMapper::globalTwin.  BQ_OPT_KEEP_DMC_BORDER = 1 has no zeroed cells and
// needs none of this.
bool BimocqGPUSolver::wholeGridPrev() const
{
    const gpuMapper &gs = *GpuSolver;
    return whole_grid_prev && gs.slab.on && gs.slab.nranks > 1 && VelocityAdvector.BlendCoeff != 1.f && !VelocityAdvector.keepDmcBorder;
}

// :503-516.  UPrev <- UInit by swap (UInit is refilled right after), UInit <- U by copy.
void BimocqGPUSolver::velocityReinitialize()
{
    VelocityUPrev.swap(VelocityUInit); VelocityVPrev.swap(VelocityVInit); VelocityWPrev.swap(VelocityWInit);
    VelocityUInit.copy_from(VelocityU); VelocityVInit.copy_from(VelocityV); VelocityWInit.copy_from(VelocityW);
    if (wholeGridPrev())
        GpuSolver->assembleGlobal({ { &VelocityUPrev, &VelocityUPrevAll }, { &VelocityVPrev, &VelocityVPrevAll }, { &VelocityWPrev, &VelocityWPrevAll } });
    else GpuSolver->dropGlobalTwins();
}

// :518-527
void BimocqGPUSolver::scalarReinitialize()
{
    DensityPrev.swap(DensityInit); TemperaturePrev.swap(TemperatureInit);
    DensityInit.copy_from(Density); TemperatureInit.copy_from(Temperature);
    if (wholeGridPrev())
        GpuSolver->assembleGlobal({ { &DensityPrev, &DensityPrevAll }, { &TemperaturePrev, &TemperaturePrevAll } });
    else GpuSolver->dropGlobalTwins();
}

static BimocqGPUSolver *g_trace_solver = nullptr;
static int g_trace_frame = 0;
static void trace_hook_fn(const char *stage) { if (g_trace_solver) trace_stage(*g_trace_solver, stage, g_trace_frame); }

// BQ_OPT_PROFILE_PHASES: one event per phase boundary on the compute stream (it closes the running span and opens the
// next); the spans are summed in phaseTotals()
void BimocqGPUSolver::phaseMark(int phase)
{
    if (!profile_phases && phase_open_ < 0) return;
    void *ev = fl_event_create();
    if (!ev) return;
    fl_event_record(ev);
    bool used = false;
    if (phase_open_ >= 0) { phase_spans_.push_back(PhaseSpan{ phase_open_ev_, ev, phase_open_ }); used = true; }
    if (profile_phases && phase >= 0 && phase < PH_COUNT) { phase_open_ev_ = ev; phase_open_ = phase; used = true; }
    else { phase_open_ev_ = nullptr; phase_open_ = -1; }
    if (!used) fl_event_destroy(ev);
}

void BimocqGPUSolver::phaseTotals(double ms[PH_COUNT], long long *steps, bool reset)
{
    for (int a = 0; a < PH_COUNT; a++) ms[a] = 0.0;
    for (const PhaseSpan &sp : phase_spans_) {
        const float t = fl_event_elapsed_ms(sp.a, sp.b);
        if (t > 0.f) ms[sp.phase] += (double)t;
    }
    if (steps) *steps = phase_steps_;
    if (reset) {
        std::vector<void *> evs;
        for (const PhaseSpan &sp : phase_spans_) { evs.push_back(sp.a); evs.push_back(sp.b); }
        std::sort(evs.begin(), evs.end());
        evs.erase(std::unique(evs.begin(), evs.end()), evs.end());
        for (void *e : evs) if (e != phase_open_ev_) fl_event_destroy(e);
        phase_spans_.clear();
        phase_steps_ = 0;
    }
}

// :129-230
void BimocqGPUSolver::advanceBimocq(int framenum, float dt)
{
    gpuMapper &gs = *GpuSolver;
    g_trace_solver = this; g_trace_frame = framenum; g_trace_hook = trace_hook_fn;
    if (framenum == 0) MaxVelocity = CellSize;           // :131 (overwritten by getCFL, kept for the record)
    float proj_coeff = 2.f;
    phaseMark(PH_MAPS);
    const float cfldt = getCFL();                        // :136
    last_cfldt = cfldt;
    // how many cells anything can travel this step (bounds the reach of the gather kernels on slab ranks)
    const int dcells = (int)std::ceil((double)dt * (double)MaxVelocity / (double)CellSize) + 1;

    // :138-139.  One update serves both advectors (shared map set).
    VelocityAdvector.updateMapping(VelocityU, VelocityV, VelocityW, cfldt, dt, dcells);
    if (!ScalarAdvector.sharesMaps()) ScalarAdvector.updateMapping(VelocityU, VelocityV, VelocityW, cfldt, dt, dcells);
    moveTracers(cfldt, dt);                               // the forward map's own trace, per particle (tracers.cpp)
    trace_stage(*this, "maps", framenum);
    phaseMark(PH_ADVECT);

    // :143-145
    if (!boundaries.empty()) semilagBand(cfldt, dt);      // BimocqSolver.cpp:106 (band nodes only)
    VelocityAdvector.advectVelocity(VelocityU, VelocityV, VelocityW, VelocityUInit, VelocityVInit, VelocityWInit,
                                    VelocityUPrev, VelocityVPrev, VelocityWPrev);
    // density and temperature live on the same nodes and use the same maps: batched (one map look-up)
    ScalarAdvector.advectFields2(Density, DensityInit, DensityPrev, Temperature, TemperatureInit, TemperaturePrev);
    if (!boundaries.empty()) blendBoundary(true);         // BimocqSolver.cpp:121-125 + clearBoundary (:134)
    const bool policy1 = reinit_policy == 1;
    trace_stage(*this, "advect", framenum);
    phaseMark(PH_FORCES);

    // Dead state: what :213-214 accumulates into *Init before a re-initialisation moves to *Prev (:503-511), and *Prev
    // is read by the two-level advection only when blend != 1 (Mapping.cpp:383-390).  With blend == 1 and a
    // re-initialisation every frame (the reference's GPU solver) nothing ever reads it: the force delta, its
    // snapshot and that accumulation are not executed (BQ_OPT_FULL_STATE = 1 executes them; every field a caller
    // can observe is the same either way, tests/test_gpu_solver.py).
    const bool prev_dead = !keep_full_state && reinit_policy == 0 && VelocityAdvector.BlendCoeff == 1.f;
    // Buoyancy acts on v only: unless a source imposes its velocity ring this frame or viscosity smooths all three
    // components, u and w stay what they are until the projection.
    bool forces_touch_uw = Viscosity != 0.f || confinement != 0.f;     // (the confinement force has all three components)
    for (const Emitter &e : sim_emitter) forces_touch_uw = forces_touch_uw || framenum < e.emitFrame;
    forces_touch_uw = forces_touch_uw || velocitySourceActive(framenum);
    // :157-159 snapshots for the force delta (:175-177).  The u and w snapshots are only ever read by that delta
    // (with the Jacobi projection the gradient pass hands out d*Proj, :179-193 needs no snapshot) and by the
    // viscous diffusion, which uses them as work arrays: not taken when nothing will touch u and w.
    if (!prev_dead) {
        if (forces_touch_uw || projection_kind != BQ_PROJECTION_JACOBI) { VelocityUTemp.copy_from(VelocityU); VelocityWTemp.copy_from(VelocityW); }
        VelocityVTemp.copy_from(VelocityV);
    }
    // policy 1 follows the CPU solver (BimocqSolver.cpp:129-133): scalar snapshots BEFORE the sources act
    if (policy1) { DensityTemp.copy_from(Density); TemperatureTemp.copy_from(Temperature); }

    emitSmoke(framenum, dt);                             // :164
    addBuoyancy(dt);                                     // :165
    confine(dt);                                         // (no counterpart in the reference: DESIGN.md section 25)

    if (Viscosity) diffuseVelocity(dt);                  // :167-172

    // :175-177 velocity change due to external forces.  When nothing touched u and w they still equal their
    // snapshots, U - UTemp is identically +0, and accumulating blend9 of a zero field (:213) changes no value --
    // neither the difference nor its look-up is executed for u and w then.
    if (prev_dead) {
        // nothing: d*Extern only feeds the accumulation that is dead
    } else if (forces_touch_uw) {
        gs.addFields(duExtern, VelocityU, VelocityUTemp, -1.f, g.nu());
        gs.addFields(dwExtern, VelocityW, VelocityWTemp, -1.f, g.nw());
        gs.produced(duExtern, std::min(VelocityU.valid, VelocityUTemp.valid));
        gs.produced(dwExtern, std::min(VelocityW.valid, VelocityWTemp.valid));
    }
    if (!prev_dead) {
        gs.addFields(dvExtern, VelocityV, VelocityVTemp, -1.f, g.nv());
        gs.produced(dvExtern, std::min(VelocityV.valid, VelocityVTemp.valid));
    }
    // :179-193: UTemp <- U, projection, dProj = U - UTemp.  With the Jacobi projection the gradient pass hands the
    // change out itself (same floats, same subtraction): no snapshot, no subtraction pass.
    const bool delta_from_gradient = projection_kind == BQ_PROJECTION_JACOBI;
    if (!delta_from_gradient) { VelocityUTemp.copy_from(VelocityU); VelocityVTemp.copy_from(VelocityV); VelocityWTemp.copy_from(VelocityW); }

    trace_stage(*this, "forces", framenum);
    phaseMark(PH_PROJECTION);
    const bool have_delta = projection(delta_from_gradient);             // :183
    trace_stage(*this, "projection", framenum);
    phaseMark(PH_ACCUMULATE);

    if (!have_delta) {
        // :188-193 dProj = U - UTemp.  The reference copies U into dProj and then adds -1*UTemp in
        // place; out = U + (-1)*UTemp is the same expression in one pass.
        gs.addFields(duProj, VelocityU, VelocityUTemp, -1.f, g.nu());
        gs.addFields(dvProj, VelocityV, VelocityVTemp, -1.f, g.nv());
        gs.addFields(dwProj, VelocityW, VelocityWTemp, -1.f, g.nw());
        gs.produced(duProj, std::min(VelocityU.valid, VelocityUTemp.valid));
        gs.produced(dvProj, std::min(VelocityV.valid, VelocityVTemp.valid));
        gs.produced(dwProj, std::min(VelocityW.valid, VelocityWTemp.valid));
    }
    // :185-186,195-198: DensityExtern = Density - DensityTemp right after DensityTemp <- Density is
    // identically zero, and accumulating a zero field (:215-216) adds 0: not executed.

    bool velReinit = true, scalarReinit = true;
    if (policy1) {
        // BimocqSolver.cpp:160-185: what the sources added to the scalars, the distortion of each map set in
        // units of the step's travel, and the CPU solver's thresholds
        gs.addFields(DensityExtern, Density, DensityTemp, -1.f, g.n());
        gs.addFields(TemperatureExtern, Temperature, TemperatureTemp, -1.f, g.n());
        gs.produced(DensityExtern, std::min(Density.valid, DensityTemp.valid));
        gs.produced(TemperatureExtern, std::min(Temperature.valid, TemperatureTemp.valid));
        last_vel_distortion = VelocityAdvector.estimateDistortion() / (MaxVelocity * dt);
        last_scalar_distortion = ScalarAdvector.estimateDistortion() / (MaxVelocity * dt);
        velReinit = scalarReinit = false;
        if (last_vel_distortion > 1.f || framenum - vel_lastReinit > 10) { velReinit = true; vel_lastReinit = framenum; proj_coeff = 1.f; }
        if (last_scalar_distortion > 5.f || framenum - scalar_lastReinit > 30) { scalarReinit = true; scalar_lastReinit = framenum; }
        if (travel_limit > 0) {
            // BQ_OPT_REINIT_MAX_TRAVEL: the next update samples the velocity up to Dfwd + dcells + 2 planes away and the
            // next advection its fields up to Dback + dcells + 2 (mapping.cpp: reachField), dcells taken as this step's.
            // A set that would not fit is re-initialised now -- the same decision on every rank (the travel is all-reduced)
            // and on one GPU given the same limit.  Should the flow speed up beyond that estimate the next step's require()
            // refuses ("ghost zone too shallow") rather than compute from missing planes.
            const auto outgrows = [&](const MapSet &ms) { return std::max(ms.Dback, ms.Dfwd) + dcells + 2 > travel_limit; };
            if (!velReinit && outgrows(*VelocityAdvector.maps)) { velReinit = true; vel_lastReinit = framenum; proj_coeff = 1.f; forced_reinits++; }
            if (!scalarReinit && outgrows(*ScalarAdvector.maps)) { scalarReinit = true; scalar_lastReinit = framenum; forced_reinits++; }
        }
    } else {
        if (framenum - vel_lastReinit > 10) {                // :200-205
            vel_lastReinit = framenum;
            proj_coeff = 1.f;
        }
        if (framenum - scalar_lastReinit > 30) {             // :207-211
            scalar_lastReinit = framenum;
        }
    }

    // :213-214
    if (!prev_dead)
        VelocityAdvector.accumulateVelocity2(VelocityUInit, VelocityVInit, VelocityWInit,
                                             duExtern, dvExtern, dwExtern, 1.f, duProj, dvProj, dwProj, proj_coeff, !forces_touch_uw);
    if (policy1) {                                       // BimocqSolver.cpp:191-192 (:215-216 here adds zeros)
        ScalarAdvector.accumulateField(DensityInit, DensityExtern);
        ScalarAdvector.accumulateField(TemperatureInit, TemperatureExtern);
    }
    trace_stage(*this, "accumulate", framenum);

    // :218-223 `if (1)`: re-initialise every frame; policy 1: when the rules above say so
    if (velReinit) {
        vel_reinits++;
        VelocityAdvector.reinitializeMapping();
        velocityReinitialize();
        VelocityAdvector.accumulateVelocity(VelocityUInit, VelocityVInit, VelocityWInit, duProj, dvProj, dwProj, 1.f);
    }
    // :225-229
    if (scalarReinit) {
        scalar_reinits++;
        if (ScalarAdvector.sharesMaps()) ScalarAdvector.noteSharedReinit();
        else ScalarAdvector.reinitializeMapping();
        scalarReinitialize();
    }
    steps_taken++;
    if (phase_open_ >= 0) phase_steps_++;
    phaseMark(PH_COUNT);
    trace_stage(*this, "reinit", framenum);
}

bool BimocqGPUSolver::outputResultAsync(unsigned frame, const std::string &filepath)
{
    waitOutput();
    if (!dump_host_) dump_host_ = static_cast<float *>(fl_malloc_host(g.n() * sizeof(float)));
    if (!dump_host_) return false;
    // The next advance() rewrites Density in place (and swaps buffers) long before a 67 MB (256^3) or 2 GB download
    // has left the device, and the copy stream's download is ordered only against compute work queued BEFORE it.  So
    // the frame is first snapshot on the compute stream (a device-to-device copy at HBM rate: 25 us at 256^3) and the
    // copy stream downloads the snapshot; the simulation never waits for PCIe.  waitOutput() above has retired the
    // previous download, so the snapshot buffer is free.
    if (dump_dev_.count() != g.n() && !dump_dev_.alloc(g.n())) return false;
    fl_memcpy_d2d(dump_dev_.get(), Density.get(), g.n() * sizeof(float));
    void *ticket = fl_download_begin(dump_host_, dump_dev_.get(), g.n() * sizeof(float));
    if (!ticket) return false;
    const SlabCtx sl = GpuSolver->slab;
    const GridDims gd = g;
    const float h = CellSize;
    float *host = dump_host_;
    dump_thread_ = std::thread([this, ticket, frame, filepath, sl, gd, h, host] {
        if (fl_download_wait(ticket) != FL_OK) { dump_result_ = -1; return; }
        if (filepath.empty()) { dump_result_ = 0; return; }
        if (!sl.on) { dump_result_ = write_density_dump(frame + 1, filepath, h, host, gd.ni, gd.nj, gd.nk, 0, gd.nk); return; }
        const size_t plane = (size_t)gd.ni * gd.nj;
        dump_result_ = write_density_dump(frame + 1, filepath, h, host + plane * sl.G, gd.ni, gd.nj, sl.own1 - sl.own0, sl.own0, sl.nkg);
    });
    return true;
}

long BimocqGPUSolver::waitOutput()
{
    if (dump_thread_.joinable()) dump_thread_.join();
    return dump_result_;
}

BimocqGPUSolver::~BimocqGPUSolver()
{
    waitOutput();
    if (dump_host_) fl_free_host(dump_host_);
}

// :536-543.  A slab rank downloads its local planes and writes the planes it owns.
long BimocqGPUSolver::outputResult(unsigned frame, const std::string &filepath)
{
    Density.download(host_density.data());
    VelocityU.download(host_u.data());
    VelocityV.download(host_v.data());
    VelocityW.download(host_w.data());
    if (fl_last_error() != FL_OK) return -1;
    if (filepath.empty()) return 0;
    const SlabCtx &sl = GpuSolver->slab;
    if (!sl.on)
        return write_density_dump(frame + 1, filepath, CellSize, host_density.data(), g.ni, g.nj, g.nk, 0, g.nk);
    const size_t plane = (size_t)g.ni * g.nj;
    return write_density_dump(frame + 1, filepath, CellSize, host_density.data() + plane * sl.G, g.ni, g.nj,
                              sl.own1 - sl.own0, sl.own0, sl.nkg);
}

// ---- per-obstacle pressure loads ----------------------------------------------------------------
bool BimocqGPUSolver::loadsOperator() { return gpu_obstacle_loads != nullptr; }

// A refused value leaves the previous one in place; 0 is accepted everywhere.
bool BimocqGPUSolver::setObstacleLoads(int n)
{
    if (n < 0) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_OBSTACLE_LOADS: a step count >= 0"); return false; }
    if (n > 0) {
        if (GpuSolver->slab.on) { fl_report_error(FL_ERR_UNSUPPORTED, "BQ_OPT_OBSTACLE_LOADS: obstacle loads are not supported on z-slab ranks"); return false; }
        if (!loadsOperator()) { fl_report_error(FL_ERR_UNSUPPORTED, "BQ_OPT_OBSTACLE_LOADS: the operator library has no gpu_obstacle_loads"); return false; }
        if (!load_ring.f64() && !load_ring.alloc((size_t)kLoadRing * 2 * kLoadSlot * sizeof(double))) return false;
        load_ring_rows.resize(kLoadRing);
    }
    loads_every = n;
    return true;
}

// the row of the step that is about to run: what the projections of this step share.  The reflection scheme's reflected
// velocity 2 u_projected - u_unprojected applies the first projection's pressure gradient twice, so the fluid's net pressure
// momentum change over the step is 2 J1 + J2; the other schemes project once.
void BimocqGPUSolver::beginLoadRow(float dt)
{
    LoadRow r;
    r.dt = (double)dt;
    r.halfrdx = (double)halfrdx;
    r.n = (int)boundaries.size();
    if (myscheme == MAC_REFLECTION) { r.w[0] = 2.0; r.w[1] = 1.0; }
    load_ring_rows[(size_t)(load_rows % kLoadRing)] = r;
    load_open = true;
    load_slot = 0;
}

// gpu_obstacle_loads on the pressure a projection has just produced (p after the ping-pong swap, or mg.p), the flags it used
// and the list at its current centres, in stream order behind it
void BimocqGPUSolver::sampleLoads(const float *pf, const double *pd)
{
    if (load_slot > 1) return;
    const size_t row = (size_t)(load_rows % kLoadRing);
    double *d_out = load_ring.f64() + (row * 2 + (size_t)load_slot) * kLoadSlot;
    if (gpu_obstacle_loads(pf, pd, projectionFlags(), rows.u8(), boundaries.data(), (int)boundaries.size(), CellSize, g.ni, g.nj, g.nk,
                           d_out) == FL_OK)
        load_ring_rows[row].filled |= 1 << load_slot;
    load_slot++;
}

void BimocqGPUSolver::endLoadRow()
{
    load_ring_rows[(size_t)(load_rows % kLoadRing)].step = steps_taken;
    load_rows++;
    load_open = false;
}

// the two raw slots of a row (unfilled ones already zeroed) -> the row a caller sees (include/bimocq_solver.h: BQ_OLOAD_*)
void BimocqGPUSolver::loadRow(const LoadRow &r, const double *slots, double out[BQ_OLOAD_ROW]) const
{
    std::fill(out, out + BQ_OLOAD_ROW, 0.0);
    out[BQ_OLOAD_STEP] = (double)r.step;
    out[BQ_OLOAD_DT] = r.dt;
    out[BQ_OLOAD_N] = (double)r.n;
    const double h = (double)CellSize;
    const double kf = r.dt != 0.0 ? r.halfrdx * (h * h * h) / r.dt : 0.0, kp = r.dt != 0.0 ? r.halfrdx * h / r.dt : 0.0;
    // the step's last projection: slot 1 of a scheme that projects twice (w[1] != 0), whatever was filled -- a sample that was
    // refused latched its error and reads 0 here like it does in the force
    const double *last = slots + (r.w[1] != 0.0 ? kLoadSlot : 0);
    for (int o = 0; o < r.n; o++) {
        const double *s0 = slots + o * BQ_LOAD_COUNT, *s1 = slots + kLoadSlot + o * BQ_LOAD_COUNT, *sl = last + o * BQ_LOAD_COUNT;
        double *q = out + BQ_OLOAD_HEADER + o * BQ_OLOAD_COUNT;
        for (int a = 0; a < 6; a++) q[BQ_OLOAD_FX + a] = r.dt != 0.0 ? kf * (r.w[0] * s0[BQ_LOAD_PX + a] + r.w[1] * s1[BQ_LOAD_PX + a]) : 0.0;
        q[BQ_OLOAD_AREA] = (h * h) * sl[BQ_LOAD_FACES];
        q[BQ_OLOAD_P_MEAN] = (r.dt != 0.0 && sl[BQ_LOAD_FACES] != 0.0) ? kp * sl[BQ_LOAD_PSUM] / sl[BQ_LOAD_FACES] : 0.0;
    }
}

// ring row `row` downloaded into slots (2 kLoadSlot doubles), the slots no projection filled zeroed
static void download_load_row(const DeviceBytes &ring, size_t row, int filled, double *slots)
{
    fl_memcpy_d2h(slots, ring.f64() + row * 2 * BimocqGPUSolver::kLoadSlot, 2 * BimocqGPUSolver::kLoadSlot * sizeof(double));    // blocking, after the queued work
    for (int s = 0; s < 2; s++)
        if (!(filled & (1 << s))) std::fill(slots + s * BimocqGPUSolver::kLoadSlot, slots + (s + 1) * BimocqGPUSolver::kLoadSlot, 0.0);
}

long BimocqGPUSolver::obstacleLoadsRaw(long back, double *slots, double weights[2])
{
    const long kept = (long)std::min<long long>(load_rows, kLoadRing);
    if (back < 0 || back >= kept) return -1;
    const size_t row = (size_t)((load_rows - 1 - back) % kLoadRing);
    const LoadRow &r = load_ring_rows[row];
    download_load_row(load_ring, row, r.filled, slots);
    if (fl_last_error() != FL_OK) return -1;
    weights[0] = r.w[0]; weights[1] = r.w[1];
    return r.step;
}

int BimocqGPUSolver::obstacleLoads(double out[BQ_OLOAD_ROW])
{
    if (load_rows == 0) return 0;
    double slots[2 * kLoadSlot];
    const size_t row = (size_t)((load_rows - 1) % kLoadRing);
    download_load_row(load_ring, row, load_ring_rows[row].filled, slots);
    if (fl_last_error() != FL_OK) return -1;
    loadRow(load_ring_rows[row], slots, out);
    return 1;
}

long BimocqGPUSolver::obstacleLoadsHistory(double *host, long capacity_rows)
{
    const long kept = (long)std::min<long long>(load_rows, kLoadRing);
    if (!host || capacity_rows <= 0 || kept == 0) return kept;
    const long long first = load_rows - kept;                       // oldest retained row
    std::vector<double> raw((size_t)kLoadRing * 2 * kLoadSlot);
    fl_memcpy_d2h(raw.data(), load_ring.f64(), raw.size() * sizeof(double));        // blocking, after the queued work
    if (fl_last_error() != FL_OK) return -1;
    for (long a = 0; a < std::min(kept, capacity_rows); a++) {
        const size_t row = (size_t)((first + a) % kLoadRing);
        double *slots = raw.data() + row * 2 * kLoadSlot;
        for (int s = 0; s < 2; s++)
            if (!(load_ring_rows[row].filled & (1 << s))) std::fill(slots + s * kLoadSlot, slots + (s + 1) * kLoadSlot, 0.0);
        loadRow(load_ring_rows[row], slots, host + (size_t)a * BQ_OLOAD_ROW);
    }
    return kept;
}

// ---- flow diagnostics ---------------------------------------------------------------------------
bool BimocqGPUSolver::diagOperator() { return gpu_flow_stats != nullptr; }

// gpu_flow_stats on the current fields into `d_out` (device, BQ_STAT_COUNT doubles); vort: NULL or the scratch field.  A slab
// rank's centred differences read one ghost plane of the velocity.
bool BimocqGPUSolver::enqueueStats(float *vort, double *d_out)
{
    if (!diagOperator()) { fl_report_error(FL_ERR_UNSUPPORTED, "diagnostics: the operator library has no gpu_flow_stats"); return false; }
    GpuSolver->require({ &VelocityU, &VelocityV, &VelocityW }, 1);
    return gpu_flow_stats(VelocityU, VelocityV, VelocityW, Density, Temperature, vort, CellSize, g.ni, g.nj, g.nk, d_out) == FL_OK;
}

// the raw sums of gpu_flow_stats -> the row a caller sees (include/bimocq_solver.h: BQ_DIAG_*)
void BimocqGPUSolver::diagRow(const double raw[BQ_STAT_COUNT], int step, double out[BQ_DIAG_COUNT]) const
{
    const double h = (double)CellSize, h3 = h * h * h;
    out[BQ_DIAG_KINETIC] = 0.5 * h3 * raw[BQ_STAT_E2];
    out[BQ_DIAG_ENSTROPHY] = 0.5 * h3 * raw[BQ_STAT_M2];
    out[BQ_DIAG_DIV_L2] = std::sqrt(h3 * raw[BQ_STAT_D2]);
    out[BQ_DIAG_DIV_MAX] = raw[BQ_STAT_DIV_MAX];
    out[BQ_DIAG_RHO_SUM] = raw[BQ_STAT_RHO];
    const bool any = raw[BQ_STAT_RHO] != 0.0;
    out[BQ_DIAG_CENTROID_X] = any ? h * raw[BQ_STAT_RHO_I] / raw[BQ_STAT_RHO] : 0.0;
    out[BQ_DIAG_CENTROID_Y] = any ? h * raw[BQ_STAT_RHO_J] / raw[BQ_STAT_RHO] : 0.0;
    out[BQ_DIAG_CENTROID_Z] = any ? h * raw[BQ_STAT_RHO_K] / raw[BQ_STAT_RHO] : 0.0;
    out[BQ_DIAG_T_SUM] = raw[BQ_STAT_T];
    out[BQ_DIAG_VORT_MAX] = raw[BQ_STAT_VORT_MAX];
    out[BQ_DIAG_STEP] = (double)step;
}

bool BimocqGPUSolver::diagnostics(double out[BQ_DIAG_COUNT])
{
    if (!diag_one.f64() && !diag_one.alloc(BQ_STAT_COUNT * sizeof(double))) return false;
    if (!enqueueStats(nullptr, diag_one.f64())) return false;
    double raw[BQ_STAT_COUNT];
    fl_memcpy_d2h(raw, diag_one.f64(), sizeof raw);                 // blocking, after the queued work
    if (fl_last_error() != FL_OK) return false;
    diagRow(raw, steps_taken, out);
    return true;
}

bool BimocqGPUSolver::setDiagnosticsEvery(int n)
{
    if (n < 0) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_DIAGNOSTICS_EVERY: a step count >= 0"); return false; }
    if (n > 0) {
        if (!diagOperator()) { fl_report_error(FL_ERR_UNSUPPORTED, "BQ_OPT_DIAGNOSTICS_EVERY: the operator library has no gpu_flow_stats"); return false; }
        if (!diag_ring.f64() && !diag_ring.alloc((size_t)kDiagRing * BQ_STAT_COUNT * sizeof(double))) return false;
        diag_ring_steps.resize(kDiagRing, 0);
    }
    diagnostics_every = n;
    return true;
}

// after the step: the stats go into the next row of the device ring, in stream order, without a host sync
void BimocqGPUSolver::sampleDiagnostics()
{
    const size_t row = (size_t)(diag_rows % kDiagRing);
    if (!enqueueStats(nullptr, diag_ring.f64() + row * BQ_STAT_COUNT)) return;
    diag_ring_steps[row] = steps_taken;
    diag_rows++;
}

long BimocqGPUSolver::diagnosticsHistory(double *host, long capacity_rows)
{
    const long kept = (long)std::min<long long>(diag_rows, kDiagRing);
    if (!host || capacity_rows <= 0 || kept == 0) return kept;
    std::vector<double> raw((size_t)kDiagRing * BQ_STAT_COUNT);
    fl_memcpy_d2h(raw.data(), diag_ring.f64(), raw.size() * sizeof(double));
    if (fl_last_error() != FL_OK) return -1;
    const long long first = diag_rows - kept;                      // oldest retained sample
    for (long a = 0; a < kept && a < capacity_rows; a++) {
        const size_t row = (size_t)((first + a) % kDiagRing);
        diagRow(raw.data() + row * BQ_STAT_COUNT, diag_ring_steps[row], host + (size_t)a * BQ_DIAG_COUNT);
    }
    return kept;
}

// |omega| at the cell centres of the local planes; the scratch field exists from the first call on
long BimocqGPUSolver::vorticity(float *host, long capacity)
{
    const long count = (long)g.n();
    if (!host || capacity <= 0) return count;
    if (Vorticity.count() != g.n() && !GpuSolver->allocField(Vorticity, FIELD_S)) return -1;
    if (!diag_one.f64() && !diag_one.alloc(BQ_STAT_COUNT * sizeof(double))) return -1;
    if (!enqueueStats(Vorticity, diag_one.f64())) return -1;
    fl_memcpy_d2h(host, Vorticity.get(), (size_t)std::min(count, capacity) * sizeof(float));
    return fl_last_error() == FL_OK ? count : -1;
}

long BimocqGPUSolver::outputVorticity(unsigned frame, const std::string &filepath, float threshold)
{
    host_vorticity.resize(g.n());
    if (vorticity(host_vorticity.data(), (long)host_vorticity.size()) < 0) return -1;
    const SlabCtx &sl = GpuSolver->slab;
    if (!sl.on)
        return write_field_dump(frame + 1, filepath, CellSize, host_vorticity.data(), g.ni, g.nj, g.nk, 0, g.nk,
                                "vorticity", "vorticity_render", threshold, (double)threshold);
    const size_t plane = (size_t)g.ni * g.nj;
    return write_field_dump(frame + 1, filepath, CellSize, host_vorticity.data() + plane * sl.G, g.ni, g.nj, sl.own1 - sl.own0,
                            sl.own0, sl.nkg, "vorticity", "vorticity_render", threshold, (double)threshold);
}

// ---- shadowed density preview -------------------------------------------------------------------
// The oracle's orc_expf / the kernels' exp_portable, operation for operation (no contraction: the products and sums below
// must round one by one).
__attribute__((optimize("fp-contract=off"))) float portable_expf(float xf)
{
    double x = (double)xf;
    if (!(x == x)) return xf;
    if (x > 90.0) x = 90.0;
    if (x < -110.0) x = -110.0;
    const double LOG2E = 1.4426950408889634074;
    const double LN2HI = 6.93147180369123816490e-01;
    const double LN2LO = 1.90821492927058770002e-10;
    const double kd = std::floor(x * LOG2E + 0.5);
    const double r = (x - kd * LN2HI) - kd * LN2LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const uint64_t bits = (uint64_t)((int64_t)kd + 1023) << 52;
    double scale;
    std::memcpy(&scale, &bits, sizeof scale);
    return (float)(p * scale);
}

// att() of include/bimocq_gpu.h: the transmittance behind the fixed-point depth afix
float render_attenuation(double afix)
{
    if (afix >= 128.0 * 4294967296.0) return 0.0f;
    return portable_expf(-(float)(afix * (1.0 / 4294967296.0)));
}

bool BimocqGPUSolver::renderOperator() { return gpu_render_density != nullptr; }

bool BimocqGPUSolver::renderSize(int view, int &w, int &h) const
{
    if (view < 0 || view > 5) { fl_report_error(FL_ERR_BAD_ARGUMENT, "render: view is a direction code 0..5"); return false; }
    const int nkg = GpuSolver->slab.on ? GpuSolver->slab.nkg : g.nk;
    w = view / 2 == 0 ? g.nj : g.ni;
    h = view / 2 == 2 ? g.nj : nkg;
    return true;
}

long BimocqGPUSolver::render(int view, int light, float sigma, float albedo, float ambient, float *radiance, float *transmittance,
                             long capacity)
{
    int w = 0, h = 0;
    if (!renderSize(view, w, h)) return -1;
    const long count = (long)w * h;
    if (!radiance && !transmittance) return count;
    if (!renderOperator()) { fl_report_error(FL_ERR_UNSUPPORTED, "render: the operator library has no gpu_render_density"); return -1; }
    const size_t bytes = 2 * (size_t)count * sizeof(double);
    if (render_image.bytes() != bytes && !render_image.alloc(bytes)) return -1;
    if (light >= 0 && Shadow.count() != g.n() && !GpuSolver->allocField(Shadow, FIELD_S)) return -1;
    GpuSolver->require({ &Density }, 0);            // owned planes only: no ghost plane is read
    const fl_render_params prm = { sigma, albedo, ambient };
    if (gpu_render_density(Density, light >= 0 ? Shadow.get() : nullptr, CellSize, g.ni, g.nj, g.nk, view, light, &prm,
                           render_image.f64()) != FL_OK) return -1;
    host_image.resize(2 * (size_t)count);
    fl_memcpy_d2h(host_image.data(), render_image.f64(), bytes);    // blocking, after the queued work
    if (fl_last_error() != FL_OK) return -1;
    const long n = std::min(count, std::max(capacity, 0L));
    for (long a = 0; a < n; a++) {
        if (radiance) radiance[a] = (float)(host_image[a] * (1.0 / 4294967296.0));
        if (transmittance) transmittance[a] = render_attenuation(host_image[(size_t)count + a]);
    }
    return count;
}

bool BimocqGPUSolver::renderSolidsOperator() { return gpu_render_density_solids != nullptr; }

// render() with the solid obstacles drawn: gpu_render_density_solids on the obstacle flags.  Without
// obstacles (an empty list, z-slab ranks) it is render() and hit = 0.
long BimocqGPUSolver::renderSolids(int view, int light, float sigma, float albedo, float ambient, float solid_albedo, float solid_ambient,
                                   float *radiance, float *transmittance, unsigned char *hit, long capacity)
{
    int w = 0, h = 0;
    if (!renderSize(view, w, h)) return -1;
    const long count = (long)w * h;
    if (!radiance && !transmittance && !hit) return count;
    const long n = std::min(count, std::max(capacity, 0L));
    if (boundaries.empty() || GpuSolver->slab.on) {
        if (!(solid_albedo >= 0.0f) || std::isinf(solid_albedo) || !(solid_ambient >= 0.0f) || std::isinf(solid_ambient) ||
            solid_albedo + solid_ambient > 4.0f) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "render: the solids' albedo and ambient must be finite, >= 0 and sum to at most 4");
            return -1;
        }
        // what the operator would refuse, also when only `hit` is asked for and nothing is drawn
        if (light < -1 || light > 5 || !(sigma >= 0.0f) || std::isinf(sigma) || !(albedo >= 0.0f) || std::isinf(albedo) ||
            !(ambient >= 0.0f) || std::isinf(ambient) || albedo + ambient > 4.0f) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "render: light is -1..5; sigma, albedo and ambient are finite, >= 0, albedo + ambient <= 4");
            return -1;
        }
        if ((radiance || transmittance) && render(view, light, sigma, albedo, ambient, radiance, transmittance, capacity) < 0) return -1;
        if (hit) std::fill(hit, hit + n, (unsigned char)0);
        return count;
    }
    if (!renderSolidsOperator()) {
        fl_report_error(FL_ERR_UNSUPPORTED, "render: the operator library has no gpu_render_density_solids");
        return -1;
    }
    const size_t bytes = 3 * (size_t)count * sizeof(double);
    if (render_image_solids.bytes() != bytes && !render_image_solids.alloc(bytes)) return -1;
    if (light >= 0 && Shadow.count() != g.n() && !GpuSolver->allocField(Shadow, FIELD_S)) return -1;
    GpuSolver->require({ &Density }, 0);
    const fl_render_params prm = { sigma, albedo, ambient };
    const fl_render_solid_params sprm = { solid_albedo, solid_ambient };
    if (gpu_render_density_solids(Density, solid.u8(), rows.u8(), light >= 0 ? Shadow.get() : nullptr, CellSize, g.ni, g.nj, g.nk, view,
                                  light, &prm, &sprm, render_image_solids.f64()) != FL_OK) return -1;
    host_image.resize(3 * (size_t)count);
    fl_memcpy_d2h(host_image.data(), render_image_solids.f64(), bytes);     // blocking, after the queued work
    if (fl_last_error() != FL_OK) return -1;
    for (long a = 0; a < n; a++) {
        const double tag = host_image[2 * (size_t)count + a];
        if (radiance) radiance[a] = (float)(host_image[a] * (1.0 / 4294967296.0));
        if (transmittance) transmittance[a] = tag != 0.0 ? 0.0f : render_attenuation(host_image[(size_t)count + a]);
        if (hit) hit[a] = (unsigned char)tag;
    }
    return count;
}

long BimocqGPUSolver::outputPreviewSolids(unsigned frame, const std::string &filepath, int view, int light, float sigma, float albedo,
                                          float ambient, float solid_albedo, float solid_ambient, float background)
{
    int w = 0, h = 0;
    if (!renderSize(view, w, h)) return -1;
    host_radiance.resize((size_t)w * h);
    host_transmittance.resize((size_t)w * h);
    if (renderSolids(view, light, sigma, albedo, ambient, solid_albedo, solid_ambient, host_radiance.data(), host_transmittance.data(),
                     nullptr, (long)w * h) < 0) return -1;
    if (GpuSolver->slab.on && GpuSolver->slab.rank != 0) return 0;
    return write_preview_pgm(frame + 1, filepath, host_radiance.data(), host_transmittance.data(), w, h, background);
}

long BimocqGPUSolver::outputPreview(unsigned frame, const std::string &filepath, int view, int light, float sigma, float albedo,
                                    float ambient, float background)
{
    int w = 0, h = 0;
    if (!renderSize(view, w, h)) return -1;
    host_radiance.resize((size_t)w * h);
    host_transmittance.resize((size_t)w * h);
    if (render(view, light, sigma, albedo, ambient, host_radiance.data(), host_transmittance.data(), (long)w * h) < 0) return -1;
    if (GpuSolver->slab.on && GpuSolver->slab.rank != 0) return 0;  // every rank holds the whole image; rank 0 writes it
    return write_preview_pgm(frame + 1, filepath, host_radiance.data(), host_transmittance.data(), w, h, background);
}

} // namespace bqhost
