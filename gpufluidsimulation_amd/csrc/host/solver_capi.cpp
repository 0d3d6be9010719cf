// solver_capi.cpp -- C view of the host solver (include/bimocq_solver.h).
#include "fluid_solver.hpp"

#include <algorithm>
#include <memory>

using namespace bqhost;

struct bq_solver {
    std::unique_ptr<gpuMapper> mapper;
    std::unique_ptr<BimocqGPUSolver> solver;
    fl_context *ctx = nullptr;          // the context that was current when the solver was created (NULL: the default one)
};
// every entry point below acts on the solver's own context: several solvers -- on one device or on several -- can be driven
// from one thread in any order
#define BQ_ENTER(s) do { if (s) fl_context_make_current((s)->ctx); } while (0)

extern "C" {

bq_solver *bq_solver_create(int device, int nx, int ny, int nz, float L, float viscosity, float blend, int scheme)
{
    return bq_solver_create_slab(device, nx, ny, nz, L, viscosity, blend, scheme, 0, 1, 0);
}

bq_solver *bq_solver_create_slab(int device, int nx, int ny, int nz, float L, float viscosity, float blend, int scheme,
                                 int rank, int nranks, int ghost)
{
    if (nx < 8 || ny < 8 || nz < 8 || (scheme != BQ_SCHEME_BIMOCQ && scheme != BQ_SCHEME_MACCORMACK && scheme != BQ_SCHEME_MAC_REFLECTION)) return nullptr;
    SlabCtx sl;
    if (nranks > 1 || ghost > 0) {
        // even z-slabs: rank r owns planes [r*nz/nranks, (r+1)*nz/nranks); each must be deeper than the ghost zone
        if (nranks < 1 || rank < 0 || rank >= nranks || ghost < 2 || nz % nranks != 0 || nz / nranks < ghost + 1) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_create_slab: need nz % nranks == 0, ghost >= 2 and nz/nranks > ghost");
            return nullptr;
        }
        sl.on = true; sl.rank = rank; sl.nranks = nranks; sl.nkg = nz; sl.G = ghost;
        sl.own0 = rank * (nz / nranks); sl.own1 = sl.own0 + nz / nranks;
    }
    auto s = std::make_unique<bq_solver>();
    s->ctx = fl_context_current();
    s->mapper = std::make_unique<gpuMapper>(device, nx, ny, nz, L / nx, sl);   // main.cpp:151 / :37 (h = L/ni)
    if (!s->mapper->ok()) return nullptr;
    s->solver = std::make_unique<BimocqGPUSolver>(nx, ny, nz, L, viscosity, blend, scheme == BQ_SCHEME_MAC_REFLECTION ? MAC_REFLECTION : scheme == BQ_SCHEME_MACCORMACK ? MACCORMACK : BIMOCQ,
                                                  s->mapper.get());
    if (!s->solver->ok()) return nullptr;
    return s.release();
}

void bq_solver_destroy(bq_solver *s)
{
    BQ_ENTER(s);
    if (!s) return;
    fl_sync();
    s->solver.reset();
    s->mapper.reset();
    delete s;
}

void bq_solver_set_smoke(bq_solver *s, float drop, float rise, const bq_emitter *emitters, int n)
{
    if (!s) return;
    std::vector<Emitter> list;
    for (int a = 0; a < n; a++) {
        Emitter e;
        e.emitFrame = emitters[a].emit_frames;
        e.emit_density = emitters[a].density;
        e.emit_temperature = emitters[a].temperature;
        e.e_pos[0] = emitters[a].cx; e.e_pos[1] = emitters[a].cy; e.e_pos[2] = emitters[a].cz;
        e.radius = emitters[a].radius;
        e.emiter = emitters[a].emiter;
        list.push_back(e);
    }
    s->solver->setSmoke(drop, rise, list);
}

void bq_solver_set_projection(bq_solver *s, int kind, int iters, float halfrdx)
{
    if (!s) return;
    if (kind == BQ_PROJECTION_MGCG && !s->solver->boundaries.empty()) {
        fl_report_error(FL_ERR_UNSUPPORTED, "bq_solver_set_projection: obstacles need the Jacobi projection");
        return;
    }
    if (kind == BQ_PROJECTION_MGCG && s->solver->walls) {
        fl_report_error(FL_ERR_UNSUPPORTED, "bq_solver_set_projection: walls need the Jacobi or the PCG projection");
        return;
    }
    if (kind == BQ_PROJECTION_MGCG) {
        s->solver->projection_kind = kind;
        s->solver->mg_iters = iters;
    } else if (kind == BQ_PROJECTION_PCG) {
        if (s->mapper->slab.on) {
            fl_report_error(FL_ERR_UNSUPPORTED, "bq_solver_set_projection: BQ_PROJECTION_PCG is not built for z-slab ranks");
            return;
        }
        if (!BimocqGPUSolver::pcgOperators()) {
            fl_report_error(FL_ERR_UNSUPPORTED, "bq_solver_set_projection: the operator library has no PCG operators");
            return;
        }
        if (iters < 0) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_set_projection: BQ_PROJECTION_PCG needs iters >= 0");
            return;
        }
        s->solver->projection_kind = kind;
        s->solver->pcg_iters = iters;
    } else if (kind == BQ_PROJECTION_JACOBI) {
        s->solver->projection_kind = kind;
        s->solver->jacobi_iters = iters;
    } else {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_set_projection: unknown projection kind");
        return;
    }
    s->solver->halfrdx = halfrdx;
}

void bq_solver_set_option(bq_solver *s, int option, int value)
{
    BQ_ENTER(s);
    if (!s) return;
    if (option == BQ_OPT_KEEP_DMC_BORDER) {
        s->solver->VelocityAdvector.keepDmcBorder = value != 0;
        s->solver->ScalarAdvector.keepDmcBorder = value != 0;
    } else if (option == BQ_OPT_FULL_STATE) {
        s->solver->keep_full_state = value != 0;
    } else if (option == BQ_OPT_FUSED_HOUSEKEEPING) {
        bqhost::gpuMapper &gm = *s->solver->GpuSolver;
        gm.fuse_housekeeping = value != 0;
        if (!value) {   // the unfused DMC update relies on scratch sets whose border nodes are zero; swaps may have left map data there
            gm.x_out.zero(); gm.y_out.zero(); gm.z_out.zero(); gm.x_out2.zero(); gm.y_out2.zero(); gm.z_out2.zero();
        }
    } else if (option == BQ_OPT_OVERLAP_EXCHANGES) {
        s->solver->GpuSolver->overlap_exchanges = value != 0;
    } else if (option == BQ_OPT_JACOBI_ENDS_FIRST) {
        s->solver->GpuSolver->jacobi_ends_first = value != 0;
        s->solver->GpuSolver->jacobi_ends_first_walled = value == 2;
    } else if (option == BQ_OPT_JACOBI_TRIPLES) {
        s->solver->GpuSolver->jacobi_triples = value != 0;
    } else if (option == BQ_OPT_MGCG_SHARED) {
        s->solver->mgcg_shared = value != 0;
    } else if (option == BQ_OPT_CONCURRENT_MAPS) {
        s->solver->GpuSolver->concurrent_maps = value != 0;
    } else if (option == BQ_OPT_NODE_LOOKUPS) {
        s->solver->GpuSolver->node_lookups = value != 0;
    } else if (option == BQ_OPT_WHOLE_GRID_PREV) {
        s->solver->whole_grid_prev = value != 0;
        if (!value) s->solver->GpuSolver->dropGlobalTwins();
    } else if (option == BQ_OPT_SHALLOW_BLOCKING_EXCHANGE) {
        s->solver->GpuSolver->shallow_blocking = value < 0 ? 0 : value;
    } else if (option == BQ_OPT_REINIT_MAX_TRAVEL) {
        s->solver->setTravelLimit(value);
    } else if (option == BQ_OPT_PROFILE_PHASES) {
        s->solver->profile_phases = value != 0;
    } else if (option == BQ_OPT_FUSED_MACCORMACK) {
        if (value < 0 || value > 2) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_FUSED_MACCORMACK: 0, 1 or 2"); return; }
        s->solver->fused_maccormack = value;
    } else if (option == BQ_OPT_DIAGNOSTICS_EVERY) {
        s->solver->setDiagnosticsEvery(value);
    } else if (option == BQ_OPT_TRACER_SORT_EVERY) {
        s->solver->setTracerSortEvery(value);
    } else if (option == BQ_OPT_OBSTACLE_LOADS) {
        s->solver->setObstacleLoads(value);
    } else if (option == BQ_OPT_REINIT_POLICY) {
        s->solver->setReinitPolicy(value);
        s->solver->ScalarAdvector.keepDmcBorder = s->solver->VelocityAdvector.keepDmcBorder;
    }
}

int bq_solver_get_option(const bq_solver *s, int option)
{
    if (!s) return -1;
    switch (option) {
    case BQ_OPT_KEEP_DMC_BORDER:     return s->solver->VelocityAdvector.keepDmcBorder ? 1 : 0;
    case BQ_OPT_REINIT_POLICY:       return s->solver->reinit_policy;
    case BQ_OPT_FULL_STATE:          return s->solver->keep_full_state ? 1 : 0;
    case BQ_OPT_FUSED_HOUSEKEEPING:  return s->solver->GpuSolver->fuse_housekeeping ? 1 : 0;
    case BQ_OPT_OVERLAP_EXCHANGES:   return s->solver->GpuSolver->overlap_exchanges ? 1 : 0;
    case BQ_OPT_JACOBI_ENDS_FIRST:   return s->solver->GpuSolver->jacobi_ends_first_walled ? 2 : s->solver->GpuSolver->jacobi_ends_first ? 1 : 0;
    case BQ_OPT_JACOBI_TRIPLES:      return s->solver->GpuSolver->jacobi_triples ? 1 : 0;
    case BQ_OPT_CONCURRENT_MAPS:     return s->solver->GpuSolver->concurrent_maps ? 1 : 0;
    case BQ_OPT_NODE_LOOKUPS:        return s->solver->GpuSolver->node_lookups ? 1 : 0;
    case BQ_OPT_WHOLE_GRID_PREV:     return s->solver->whole_grid_prev ? (s->solver->GpuSolver->globalTwin(&s->solver->VelocityUPrev) ? 2 : 1) : 0;
    case BQ_OPT_MGCG_SHARED:         return s->solver->mgcg_shared ? (s->solver->mgcg_shared_ran ? 2 : 1) : 0;    // 2: the last projection took it
    case BQ_OPT_SHALLOW_BLOCKING_EXCHANGE: return s->solver->GpuSolver->shallow_blocking;
    case BQ_OPT_PROFILE_PHASES:      return s->solver->profile_phases ? 1 : 0;
    case BQ_OPT_REINIT_MAX_TRAVEL:   return s->solver->travel_limit;
    case BQ_OPT_FUSED_MACCORMACK:    return s->solver->fused_maccormack;
    case BQ_OPT_DIAGNOSTICS_EVERY:   return s->solver->diagnostics_every;
    case BQ_OPT_TRACER_SORT_EVERY:   return s->solver->tracer_sort_every;
    case BQ_OPT_OBSTACLE_LOADS:      return s->solver->loads_every;
    default:                         return -1;
    }
}

int bq_solver_reinit_counts(const bq_solver *s, int which)
{
    if (!s) return 0;
    if (which == 2) return s->solver->forced_reinits;
    return which ? s->solver->scalar_reinits : s->solver->vel_reinits;
}

float bq_solver_last_distortion(const bq_solver *s, int which)
{
    if (!s) return 0.f;
    return which ? s->solver->last_scalar_distortion : s->solver->last_vel_distortion;
}

void bq_solver_advance(bq_solver *s, int framenum, float dt)
{
    BQ_ENTER(s);
    if (s) s->solver->advance(framenum, dt);
}

long bq_solver_output_result(bq_solver *s, unsigned frame, const char *path)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->outputResult(frame, path ? std::string(path) : std::string());
}

int bq_solver_output_result_async(bq_solver *s, unsigned frame, const char *path)
{
    BQ_ENTER(s);
    if (!s) return 0;
    return s->solver->outputResultAsync(frame, path ? std::string(path) : std::string()) ? 1 : 0;
}

long bq_solver_output_wait(bq_solver *s)
{
    BQ_ENTER(s);
    return s ? s->solver->waitOutput() : -1;
}

long bq_solver_download(bq_solver *s, int which, float *host, long capacity)
{
    BQ_ENTER(s);
    if (!s) return 0;
    BimocqGPUSolver &b = *s->solver;
    MapSet &m = *b.VelocityAdvector.maps;
    const DeviceField *f[BQ_F_COUNT] = {
        &b.Density, &b.Temperature, &b.VelocityU, &b.VelocityV, &b.VelocityW,
        &b.VelocityUInit, &b.VelocityVInit, &b.VelocityWInit, &b.DensityInit, &b.TemperatureInit,
        &m.ForwardX, &m.ForwardY, &m.ForwardZ, &m.BackwardX, &m.BackwardY, &m.BackwardZ, &b.p, &b.div };
    if (which < 0 || which >= BQ_F_COUNT) return 0;
    long count = (long)f[which]->count();
    if (host && capacity > 0)
        fl_memcpy_d2h(host, f[which]->get(), (size_t)std::min(count, capacity) * sizeof(float));
    return count;
}

int bq_solver_set_boundary(bq_solver *s, const bq_boundary *b, int n)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->setBoundary(b, nullptr, n) ? 0 : -1;
}

int bq_solver_set_boundary_levelsets(bq_solver *s, const bq_boundary *b, const bq_levelset *ls, int n)
{
    BQ_ENTER(s);
    if (!s) return -1;
    if (s->solver->setBoundary(b, ls, n)) return 0;
    s->solver->dropBoundaries();                    // after any failure no obstacles are left
    return -1;
}

int bq_solver_set_boundary_poses(bq_solver *s, const bq_boundary *b, const bq_levelset *ls, const bq_pose *pose, int n)
{
    BQ_ENTER(s);
    if (!s) return -1;
    if (s->solver->setBoundary(b, ls, n, pose)) return 0;
    s->solver->dropBoundaries();                    // after any failure no obstacles are left
    return -1;
}

int bq_solver_boundary_pose(const bq_solver *s, int i, double out[10])
{
    if (!s || !out || i < 0 || i >= (int)s->solver->boundaries.size()) return -1;
    const bq_boundary &b = s->solver->boundaries[(size_t)i];
    const bq_pose &p = s->solver->poses[(size_t)i];
    const std::array<double, 4> &q = s->solver->orientations[(size_t)i];
    out[0] = b.cx; out[1] = b.cy; out[2] = b.cz;
    out[3] = q[0]; out[4] = q[1]; out[5] = q[2]; out[6] = q[3];
    out[7] = p.ox; out[8] = p.oy; out[9] = p.oz;
    return 0;
}

int bq_solver_set_sources(bq_solver *s, const bq_source *src, const bq_levelset *ls, int n)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->setSources(src, ls, n) ? 0 : -1;      // (a refused list leaves no sources)
}

int bq_solver_source_position(const bq_solver *s, int i, float out[3])
{
    if (!s || !out || i < 0 || i >= (int)s->solver->sources.size()) return -1;
    const bq_boundary &b = s->solver->sources[(size_t)i].shape;
    out[0] = b.cx; out[1] = b.cy; out[2] = b.cz;
    return 0;
}

int bq_solver_update_boundary(bq_solver *s, int framenum, float dt)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->updateBoundary(framenum, dt) ? 0 : -1;
}

int bq_solver_set_walls(bq_solver *s, int walls)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->setWalls(walls) ? 0 : -1;
}

int bq_solver_get_walls(bq_solver *s)
{
    return s ? s->solver->walls : 0;
}

int bq_solver_set_vorticity_confinement(bq_solver *s, float eps)
{
    BQ_ENTER(s);
    if (!s) return -1;
    return s->solver->setVorticityConfinement(eps) ? FL_OK : fl_last_error();
}

float bq_solver_get_vorticity_confinement(const bq_solver *s)
{
    return s ? s->solver->confinement : 0.f;
}

long bq_solver_download_solid(bq_solver *s, unsigned char *host, long capacity)
{
    BQ_ENTER(s);
    if (!s) return 0;
    BimocqGPUSolver &b = *s->solver;
    const long count = (long)b.g.n();
    if (!host || capacity <= 0) return count;
    const size_t m = (size_t)std::min(count, capacity);
    if (b.boundaries.empty()) {
        std::fill(host, host + m, (unsigned char)0);
        return count;
    }
    fl_memcpy_d2h(host, b.solid.u8(), m);
    for (size_t a = 0; a < m; a++) host[a] = host[a] ? 1 : 0;
    return count;
}

/* slab geometry of this solver: {on, rank, nranks, nk_global, own0, own1, ghost, nk_local} */
void bq_solver_slab_info(const bq_solver *s, int out[8])
{
    if (!s || !out) return;
    const SlabCtx &sl = s->mapper->slab;
    out[0] = sl.on; out[1] = sl.rank; out[2] = sl.nranks; out[3] = sl.on ? sl.nkg : s->mapper->g.nk;
    out[4] = sl.on ? sl.own0 : 0; out[5] = sl.on ? sl.own1 : s->mapper->g.nk; out[6] = sl.G; out[7] = s->mapper->g.nk;
}

long bq_solver_mg_history(const bq_solver *s, double *host, long capacity)
{
    BQ_ENTER(s);
    // (the shared solve on slab ranks owns its vectors: only tempResult is allocated here, mg.ready stays false)
    if (!s || (!s->solver->mg.ready && s->solver->mg.result.bytes() < 4096 * sizeof(double))) return 0;
    const std::vector<double> h = s->solver->mgHistory();
    if (host)
        for (long a = 0; a < capacity && a < (long)h.size(); a++) host[a] = h[(size_t)a];
    return (long)h.size();
}

int bq_solver_set_pcg_tolerance(bq_solver *s, double tol)
{
    if (!s) return -1;
    if (!(tol > 0.0 && tol < 1.0)) {                   // (NaN fails the test too)
        fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_set_pcg_tolerance: tol must be finite and in (0, 1)");
        return -1;
    }
    s->solver->pcg_tol = tol;
    return 0;
}

int bq_solver_pcg_stats(const bq_solver *s, double out[6])
{
    if (!s || !out) return 0;
    const BimocqGPUSolver &b = *s->solver;
    for (int a = 0; a < 4; a++) out[a] = b.pcg_stats[a];
    out[4] = (double)b.pcg_projections;
    out[5] = (double)b.pcg_unconverged;
    return b.pcg_projections > 0 ? 1 : 0;
}

long bq_solver_pcg_pressure(bq_solver *s, double *host, long capacity)
{
    BQ_ENTER(s);
    if (!s || s->solver->pcg_projections == 0) return 0;
    const BimocqGPUSolver &b = *s->solver;
    const long count = (long)b.g.n();
    if (host && capacity > 0) fl_memcpy_d2h(host, b.mg.p.f64(), (size_t)std::min(count, capacity) * sizeof(double));
    return count;
}

long long bq_solver_phase_ms(bq_solver *s, double ms[BQ_PHASE_COUNT], int reset)
{
    BQ_ENTER(s);
    if (!s || !ms) return 0;
    long long steps = 0;
    s->solver->phaseTotals(ms, &steps, reset != 0);
    return steps;
}

int bq_solver_diagnostics(bq_solver *s, double out[BQ_DIAG_COUNT])
{
    BQ_ENTER(s);
    if (!s || !out) return FL_ERR_BAD_ARGUMENT;
    if (s->solver->diagnostics(out)) return FL_OK;
    const int err = fl_last_error();
    return err != FL_OK ? err : (int)FL_ERR_HIP;
}

long bq_solver_diagnostics_history(bq_solver *s, double *host, long capacity_rows)
{
    BQ_ENTER(s);
    return s ? s->solver->diagnosticsHistory(host, capacity_rows) : 0;
}

int bq_solver_obstacle_loads(bq_solver *s, double row[BQ_OLOAD_ROW])
{
    BQ_ENTER(s);
    if (!s || !row) return -1;
    return s->solver->obstacleLoads(row);
}

long bq_solver_obstacle_loads_history(bq_solver *s, double *host, long capacity_rows)
{
    BQ_ENTER(s);
    return s ? s->solver->obstacleLoadsHistory(host, capacity_rows) : 0;
}

long bq_solver_obstacle_loads_raw(bq_solver *s, long back, double slots[2 * 128], double weights[2])
{
    BQ_ENTER(s);
    if (!s || !slots || !weights) return -1;
    return s->solver->obstacleLoadsRaw(back, slots, weights);
}

long bq_solver_vorticity(bq_solver *s, float *host, long capacity)
{
    BQ_ENTER(s);
    return s ? s->solver->vorticity(host, capacity) : 0;
}

long bq_solver_output_vorticity(bq_solver *s, unsigned frame, const char *path, float threshold)
{
    BQ_ENTER(s);
    if (!s || !path) return -1;
    return s->solver->outputVorticity(frame, std::string(path), threshold);
}

int bq_solver_render_size(bq_solver *s, int view, int *w, int *h)
{
    BQ_ENTER(s);
    if (!s || !w || !h) return FL_ERR_BAD_ARGUMENT;
    return s->solver->renderSize(view, *w, *h) ? (int)FL_OK : (int)FL_ERR_BAD_ARGUMENT;
}

long bq_solver_render(bq_solver *s, int view, int light, float sigma, float albedo, float ambient, float *radiance,
                      float *transmittance, long capacity)
{
    BQ_ENTER(s);
    return s ? s->solver->render(view, light, sigma, albedo, ambient, radiance, transmittance, capacity) : -1;
}

long bq_solver_output_preview(bq_solver *s, unsigned frame, const char *path, int view, int light, float sigma, float albedo,
                              float ambient, float background)
{
    BQ_ENTER(s);
    if (!s || !path) return -1;
    return s->solver->outputPreview(frame, std::string(path), view, light, sigma, albedo, ambient, background);
}

long bq_solver_render_solids(bq_solver *s, int view, int light, float sigma, float albedo, float ambient, float solid_albedo,
                             float solid_ambient, float *radiance, float *transmittance, unsigned char *hit, long capacity)
{
    BQ_ENTER(s);
    return s ? s->solver->renderSolids(view, light, sigma, albedo, ambient, solid_albedo, solid_ambient, radiance, transmittance, hit,
                                       capacity) : -1;
}

long bq_solver_output_preview_solids(bq_solver *s, unsigned frame, const char *path, int view, int light, float sigma, float albedo,
                                     float ambient, float solid_albedo, float solid_ambient, float background)
{
    BQ_ENTER(s);
    if (!s || !path) return -1;
    return s->solver->outputPreviewSolids(frame, std::string(path), view, light, sigma, albedo, ambient, solid_albedo, solid_ambient,
                                          background);
}

int bq_solver_set_tracers(bq_solver *s, const float *xyz, long n)
{
    BQ_ENTER(s);
    if (!s) return FL_ERR_BAD_ARGUMENT;
    if (s->solver->setTracers(xyz, n)) return FL_OK;
    const int err = fl_last_error();
    return err != FL_OK ? err : (int)FL_ERR_HIP;
}

long bq_solver_seed_tracers(bq_solver *s, const int lo[3], const int hi[3], int per_cell, unsigned seed)
{
    BQ_ENTER(s);
    return s ? s->solver->seedTracers(lo, hi, per_cell, seed) : -1;
}

long bq_solver_tracer_count(const bq_solver *s) { return s ? s->solver->tracer_count : 0; }

long bq_solver_tracers(bq_solver *s, float *xyz, long capacity)
{
    BQ_ENTER(s);
    return s ? s->solver->tracers(xyz, capacity) : -1;
}

long bq_solver_tracer_sample(bq_solver *s, int which, float *out, long capacity)
{
    BQ_ENTER(s);
    return s ? s->solver->tracerSample(which, out, capacity) : -1;
}

long bq_solver_output_tracers(bq_solver *s, unsigned frame, const char *path, int which)
{
    BQ_ENTER(s);
    if (!s || !path) return -1;
    return s->solver->outputTracers(frame, std::string(path), which);
}

long bq_solver_tracer_stored(bq_solver *s, float *xyz, unsigned *ids, long capacity)
{
    BQ_ENTER(s);
    if (!s) return -1;
    BimocqGPUSolver &b = *s->solver;
    const long n = std::min(b.tracer_count, std::max(capacity, 0L));
    if (n > 0 && xyz) {
        const DeviceField *f[3] = { &b.TracerX, &b.TracerY, &b.TracerZ };
        for (int c = 0; c < 3; c++) fl_memcpy_d2h(xyz + (size_t)c * n, f[c]->get(), (size_t)n * sizeof(float));
    }
    if (n > 0 && ids) {
        if (b.tracer_ids) fl_memcpy_d2h(ids, b.tracer_id.u8(), (size_t)n * sizeof(unsigned));
        else for (long a = 0; a < n; a++) ids[a] = (unsigned)a;
    }
    return b.tracer_count;
}

float bq_solver_last_cfldt(const bq_solver *s) { return s ? s->solver->last_cfldt : 0.f; }
float bq_solver_last_ms(const bq_solver *s) { return s ? s->solver->last_ms : 0.f; }
int   bq_solver_reinit_count(const bq_solver *s) { return s ? (int)s->solver->VelocityAdvector.TotalReinitCount : 0; }

} // extern "C"
