// tracers.cpp -- passive tracer particles of the host solver (fluid_solver.hpp).
//
// The solver owns three position arrays on the device and, once a sort has run, an id per stored slot.  advance() traces
// every particle over the step's dt through the velocity the step starts with -- the very trace the forward map's nodes
// take (gpu_trace_particles / gpu_solve_forward), so a tracer seeded on a grid node stays, bit for bit, on the forward map's
// entry for that node until the map is re-initialised.  Tracers are passive: they follow the velocity as it is, inside
// solids too.  Everything public is in id order.  One GPU: particles would have to migrate between z-slab ranks.
#include "fluid_solver.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

// weak references, like the obstacle operators in fluid_solver.cpp: a stand-in of the operator ABI need not provide them
#pragma weak gpu_trace_particles
#pragma weak gpu_sample_particles
#pragma weak gpu_seed_particles
#pragma weak gpu_sort_particles

namespace bqhost {

bool BimocqGPUSolver::tracerOperators()
{
    return gpu_trace_particles && gpu_sample_particles && gpu_seed_particles && gpu_sort_particles;
}

bool BimocqGPUSolver::tracersAllowed(const char *who)
{
    if (GpuSolver->slab.on) {
        fl_report_error(FL_ERR_UNSUPPORTED, (std::string(who) + ": tracers are not built for z-slab ranks (no migration between ranks)").c_str());
        return false;
    }
    if (!tracerOperators()) {
        fl_report_error(FL_ERR_UNSUPPORTED, (std::string(who) + ": the operator library has no gpu_trace_particles").c_str());
        return false;
    }
    return true;
}

void BimocqGPUSolver::dropTracers()
{
    for (DeviceField *f : { &TracerX, &TracerY, &TracerZ, &TracerX2, &TracerY2, &TracerZ2, &TracerAttr }) f->release();
    tracer_id.release(); tracer_id2.release();
    tracer_ids = false;
    tracer_count = 0;
}

bool BimocqGPUSolver::setTracerSortEvery(int n)
{
    if (n < 0) { fl_report_error(FL_ERR_BAD_ARGUMENT, "BQ_OPT_TRACER_SORT_EVERY: N >= 0"); return false; }
    if (n > 0 && !tracersAllowed("BQ_OPT_TRACER_SORT_EVERY")) return false;
    tracer_sort_every = n;
    return true;
}

// the first tracer_count particles (and their ids) move into arrays of `total` elements
bool BimocqGPUSolver::growTracers(long total)
{
    DeviceField nx, ny, nz;
    if (!nx.alloc((size_t)total) || !ny.alloc((size_t)total) || !nz.alloc((size_t)total)) return false;
    const size_t keep = (size_t)tracer_count * sizeof(float);
    if (keep) {
        fl_memcpy_d2d(nx, TracerX, keep); fl_memcpy_d2d(ny, TracerY, keep); fl_memcpy_d2d(nz, TracerZ, keep);
    }
    if (tracer_ids) {
        DeviceBytes nid;
        if (!nid.alloc((size_t)total * sizeof(unsigned))) return false;
        if (keep) fl_memcpy_d2d(nid.u8(), tracer_id.u8(), (size_t)tracer_count * sizeof(unsigned));
        std::vector<unsigned> fresh((size_t)(total - tracer_count));            // appended ids continue from the count
        for (size_t a = 0; a < fresh.size(); a++) fresh[a] = (unsigned)((size_t)tracer_count + a);
        if (!fresh.empty())
            fl_memcpy_h2d(nid.u8() + (size_t)tracer_count * sizeof(unsigned), fresh.data(), fresh.size() * sizeof(unsigned));
        tracer_id = std::move(nid);
    }
    TracerX = std::move(nx); TracerY = std::move(ny); TracerZ = std::move(nz);
    return fl_last_error() == FL_OK;
}

bool BimocqGPUSolver::setTracers(const float *xyz, long n)
{
    dropTracers();
    if (n == 0) return true;
    if (!tracersAllowed("bq_solver_set_tracers")) return false;
    if (n < 0 || n > (long)BQ_MAX_TRACERS || !xyz) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_set_tracers: need positions and 0 <= n <= BQ_MAX_TRACERS");
        return false;
    }
    for (long a = 0; a < 3 * n; a++)
        if (!std::isfinite(xyz[a])) {
            fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_set_tracers: a position is not finite");
            return false;
        }
    // into the trace's clamp box, by the trace's own expressions
    const float h = CellSize;
    const float hi[3] = { (float)g.ni * h - h, (float)g.nj * h - h, (float)g.nk * h - h };
    host_tracers.resize((size_t)3 * n);
    for (long a = 0; a < n; a++)
        for (int c = 0; c < 3; c++) host_tracers[(size_t)c * n + a] = std::fmin(std::fmax(h, xyz[3 * a + c]), hi[c]);
    if (!growTracers(n)) { dropTracers(); return false; }
    const size_t bytes = (size_t)n * sizeof(float);
    fl_memcpy_h2d(TracerX, host_tracers.data(), bytes);
    fl_memcpy_h2d(TracerY, host_tracers.data() + n, bytes);
    fl_memcpy_h2d(TracerZ, host_tracers.data() + 2 * n, bytes);
    if (fl_last_error() != FL_OK) { dropTracers(); return false; }
    tracer_count = n;
    return true;
}

long BimocqGPUSolver::seedTracers(const int lo[3], const int hi[3], int per_cell, unsigned seed)
{
    if (!tracersAllowed("bq_solver_seed_tracers")) return -1;
    if (!lo || !hi || per_cell < 1) { fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_seed_tracers: need a box and per_cell >= 1"); return -1; }
    // the operator's own intersection with the cells 1 .. n - 2: the count is closed-form
    const int dims[3] = { g.ni, g.nj, g.nk };
    double count = (double)per_cell;
    for (int c = 0; c < 3; c++) count *= (double)std::max(std::min(hi[c], dims[c] - 1) - std::max(lo[c], 1), 0);
    if ((double)tracer_count + count > (double)BQ_MAX_TRACERS) {
        fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_seed_tracers: more than BQ_MAX_TRACERS tracers");
        return -1;
    }
    const long added = (long)count;
    if (added == 0) return 0;
    if (!growTracers(tracer_count + added)) return -1;
    if (gpu_seed_particles(TracerX.get() + tracer_count, TracerY.get() + tracer_count, TracerZ.get() + tracer_count,
                           lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], per_cell, seed, CellSize, g.ni, g.nj, g.nk) != FL_OK) return -1;
    tracer_count += added;
    return added;
}

// advance(): the whole dt through the velocity the step starts with, sub-steps of this step's getCFL() value
void BimocqGPUSolver::moveTracers(float cfldt, float dt)
{
    if (tracer_count == 0) return;
    gpu_trace_particles(VelocityU, VelocityV, VelocityW, TracerX, TracerY, TracerZ, tracer_count, CellSize, g.ni, g.nj, g.nk, cfldt, dt);
}

void BimocqGPUSolver::sortTracers()
{
    if (tracer_count == 0) return;
    const size_t n = (size_t)tracer_count;
    for (DeviceField *f : { &TracerX2, &TracerY2, &TracerZ2 })
        if (f->count() != TracerX.count() && !f->alloc(TracerX.count())) return;
    if (tracer_id2.bytes() != TracerX.count() * sizeof(unsigned) && !tracer_id2.alloc(TracerX.count() * sizeof(unsigned))) return;
    const unsigned *ids = tracer_ids ? reinterpret_cast<const unsigned *>(tracer_id.u8()) : nullptr;       // none yet: the identity
    if (gpu_sort_particles(TracerX, TracerY, TracerZ, ids, TracerX2, TracerY2, TracerZ2, reinterpret_cast<unsigned *>(tracer_id2.u8()),
                           (long)n, CellSize, g.ni, g.nj, g.nk) != FL_OK) return;
    TracerX.swap(TracerX2); TracerY.swap(TracerY2); TracerZ.swap(TracerZ2);
    std::swap(tracer_id, tracer_id2);
    tracer_ids = true;
    tracer_sorts++;
}

bool BimocqGPUSolver::downloadTracerIds()
{
    host_tracer_ids.clear();
    if (!tracer_ids) return true;
    host_tracer_ids.resize((size_t)tracer_count);
    fl_memcpy_d2h(host_tracer_ids.data(), tracer_id.u8(), (size_t)tracer_count * sizeof(unsigned));
    if (fl_last_error() != FL_OK) return false;
    for (unsigned id : host_tracer_ids)
        if ((long)id >= tracer_count) { fl_report_error(FL_ERR_HIP, "tracers: an id is out of range"); return false; }
    return true;
}

long BimocqGPUSolver::tracers(float *xyz, long capacity)
{
    if (!xyz || capacity <= 0 || tracer_count == 0) return tracer_count;
    const size_t n = (size_t)tracer_count, bytes = n * sizeof(float);
    host_tracers.resize(3 * n);
    fl_memcpy_d2h(host_tracers.data(), TracerX, bytes);             // blocking, after the queued work
    fl_memcpy_d2h(host_tracers.data() + n, TracerY, bytes);
    fl_memcpy_d2h(host_tracers.data() + 2 * n, TracerZ, bytes);
    if (fl_last_error() != FL_OK || !downloadTracerIds()) return -1;
    for (size_t a = 0; a < n; a++) {
        const size_t id = tracer_ids ? host_tracer_ids[a] : a;
        if ((long)id >= capacity) continue;
        for (int c = 0; c < 3; c++) xyz[3 * id + c] = host_tracers[(size_t)c * n + a];
    }
    return tracer_count;
}

long BimocqGPUSolver::tracerSample(int which, float *out, long capacity)
{
    const float mh = (float)(-0.5 * (double)CellSize);              // the stagger of get_velocity (GPU_kernel.cu:64-72)
    struct Item { const DeviceField *f; int nx, ny, nz; float ox, oy, oz; };
    Item it;
    switch (which) {
    case BQ_F_RHO: it = { &Density, g.ni, g.nj, g.nk, 0.f, 0.f, 0.f }; break;
    case BQ_F_T:   it = { &Temperature, g.ni, g.nj, g.nk, 0.f, 0.f, 0.f }; break;
    case BQ_F_U:   it = { &VelocityU, g.ni + 1, g.nj, g.nk, mh, 0.f, 0.f }; break;
    case BQ_F_V:   it = { &VelocityV, g.ni, g.nj + 1, g.nk, 0.f, mh, 0.f }; break;
    case BQ_F_W:   it = { &VelocityW, g.ni, g.nj, g.nk + 1, 0.f, 0.f, mh }; break;
    default:
        fl_report_error(FL_ERR_BAD_ARGUMENT, "bq_solver_tracer_sample: which is BQ_F_RHO, BQ_F_T, BQ_F_U, BQ_F_V or BQ_F_W");
        return -1;
    }
    if (!out || capacity <= 0 || tracer_count == 0) return tracer_count;
    if (!tracersAllowed("bq_solver_tracer_sample")) return -1;
    const size_t n = (size_t)tracer_count;
    if (TracerAttr.count() < n && !TracerAttr.alloc(TracerX.count())) return -1;
    if (gpu_sample_particles(it.f->get(), it.nx, it.ny, it.nz, CellSize, it.ox, it.oy, it.oz, TracerX, TracerY, TracerZ, TracerAttr,
                             tracer_count) != FL_OK) return -1;
    host_tracers.resize(n);
    fl_memcpy_d2h(host_tracers.data(), TracerAttr, n * sizeof(float));
    if (fl_last_error() != FL_OK || !downloadTracerIds()) return -1;
    for (size_t a = 0; a < n; a++) {
        const size_t id = tracer_ids ? host_tracer_ids[a] : a;
        if ((long)id < capacity) out[id] = host_tracers[a];
    }
    return tracer_count;
}

long BimocqGPUSolver::outputTracers(unsigned frame, const std::string &filepath, int which)
{
    const size_t n = (size_t)tracer_count;
    host_tracer_xyz.resize(3 * n);
    if (tracers(host_tracer_xyz.data(), tracer_count) < 0) return -1;
    const float *attr = nullptr;
    if (which >= 0) {
        host_tracer_attr.resize(n);
        if (tracerSample(which, host_tracer_attr.data(), tracer_count) < 0) return -1;
        attr = host_tracer_attr.data();
    }
    return write_tracer_dump(frame + 1, filepath, host_tracer_xyz.data(), attr, tracer_count, g.ni, g.nj, g.nk, CellSize, which);
}

} // namespace bqhost
