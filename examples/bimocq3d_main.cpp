// bimocq3d_main.cpp -- the reference's driver loop (src/bimocq3D/main.cpp:137-159, GPU branch) on this library:
//   gpuMapper + BimocqGPUSolver(ni, nj, nk, L, viscosity, blend, scheme, mapper); setSmoke; advance(i, dt);
//   outputResult(i, path) every frame.
// The scene is the synthetic rising-smoke case of SURVEY 8(d) (one warm sphere near the floor) instead of the
// reference's OpenVDB-SDF emitters, which need OpenVDB.
//
// scene = 1 is BASELINE config 5's shape: an N x N x N/2 box (1024 x 1024 x 512 at N = 1024) with two coaxial vortex
// rings blown along x by the reference's emitter velocity formula (main.cpp:52-73, emiter = +1 for both: the rear
// ring catches up and threads the front one -- leapfrogging), no buoyancy, density dumped every frame.
//
//   make example && build/bimocq3d [N=128] [frames=20] [outdir=out] [scheme=0|2|3] [projection=0|1] [async=1] [scene=0|1] [walls=0] [diag_every=0] [preview_every=0] [tracers_per_cell=0] [paddle_spin=0] [confinement=0] [loads_every=0] [preview_solids=0]
// diag_every = N > 0: the flow diagnostics of every N-th frame (bq_solver_diagnostics' row: kinetic energy, enstrophy, ...) are
// sampled on the device while the run goes on, printed one line per sampled frame at the end, and the vorticity magnitude of
// those frames is dumped next to the density (vorticity_render_%04u.bqd)
// preview_every = N > 0: a shadowed preview of the density of every N-th frame, drawn on the device (view along +z, lit from
// above), is written next to the density dumps (preview_%04u.pgm); preview_solids = 1 draws the solid obstacles into it
// (opaque, flat-shaded, shadow-casting: with paddle_spin the paddle shows)
// tracers_per_cell = N > 0: N jittered passive tracers in every cell of each emitter's bounding box, moved with every step on the
// device and dumped with every frame (tracers_%04u.bqp: positions and the density sampled at them)
// paddle_spin = S != 0: a box paddle of half extents (0.3 L, 2 h, 0.15 L) at the centre of the domain (scenes.paddle of the Python
// package) turns about the z axis at S rad per time unit in the rising smoke; updateBoundary every frame
// confinement = E > 0: vorticity confinement with the dimensionless coefficient E
// loads_every = N > 0 (with obstacles, i.e. a paddle): the pressure force and torque on every obstacle are
// sampled on the device with every N-th frame and printed, one line per obstacle
// walls: the closed sides (BQ_WALL_* bits of include/bimocq_gpu.h; 55 = the reference CPU solver's container, open at the top)
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bimocq_gpu.h"
#include "fluid_solver.hpp"

int main(int argc, char **argv)
{
    using namespace bqhost;
    const int n = argc > 1 ? std::atoi(argv[1]) : 128;
    const int total_frame = argc > 2 ? std::atoi(argv[2]) : 20;
    const std::string filepath = argc > 3 ? argv[3] : "out";
    const int scheme = argc > 4 ? std::atoi(argv[4]) : 0;            // 0 BIMOCQ, 2 MACCORMACK, 3 MAC_REFLECTION (main.cpp:51 ships 3)
    const int projection = argc > 5 ? std::atoi(argv[5]) : 0;        // 0 Jacobi, 1 multigrid-CG (what the binary ships)
    const bool async_dump = argc > 6 ? std::atoi(argv[6]) != 0 : true;
    const int scene = argc > 7 ? std::atoi(argv[7]) : 0;             // 0 rising smoke, 1 leapfrogging vortex rings, 2 box-shaped plume source
    const int walls = argc > 8 ? std::atoi(argv[8]) : BQ_WALLS_NONE; // closed sides, BQ_WALL_* bits: 55 = the reference's container (open top)
    const int diag_every = argc > 9 ? std::atoi(argv[9]) : 0;        // flow diagnostics and a vorticity dump every N-th frame (0: none)
    const int preview_every = argc > 10 ? std::atoi(argv[10]) : 0;   // a shadowed preview image every N-th frame (0: none)
    const int tracers_per_cell = argc > 11 ? std::atoi(argv[11]) : 0; // passive tracers per cell of the emitters' bounding cells (0: none)
    const float paddle_spin = argc > 12 ? (float)std::atof(argv[12]) : 0.f; // angular velocity of the paddle about z (0: no paddle)
    const float confinement = argc > 13 ? (float)std::atof(argv[13]) : 0.f; // vorticity confinement coefficient (0: none)
    const int loads_every = argc > 14 ? std::atoi(argv[14]) : 0;     // pressure loads on the obstacles every N-th frame (0: none)
    const bool preview_solids = argc > 15 ? std::atoi(argv[15]) != 0 : false; // draw the obstacles into the previews
    if (n < 8 || total_frame < 1 || loads_every < 0 || !(confinement >= 0.f) || !std::isfinite(confinement) || diag_every < 0 || preview_every < 0 || tracers_per_cell < 0 || !std::isfinite(paddle_spin) || (scene == 1 && n % 2) || (scheme != 0 && scheme != 2 && scheme != 3)) {
        std::fprintf(stderr, "usage: %s [N>=8] [frames] [outdir] [scheme: 0 BiMocq, 2 MacCormack, 3 reflection] [projection] [async] [scene] [walls] [diag_every] [preview_every] [tracers_per_cell] [paddle_spin] [confinement] [loads_every] [preview_solids]\n", argv[0]); return 2;
    }

    const int ni = n, nj = n, nk = scene == 1 ? n / 2 : n;
    const float L = 1.f, h = L / (float)n, dt = 2.f * h;
    const float viscosity = 0.f, mapping_blend_coeff = 1.f;          // main.cpp:46-47
    const float smoke_rise = scene == 1 ? 0.f : 1.f, smoke_drop = 0.f;

    if (fl_init(0) != FL_OK) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    auto *myGPUmapper = new gpuMapper(/*device*/0, ni, nj, nk, h);
    BimocqGPUSolver mysolver(ni, nj, nk, L, viscosity, mapping_blend_coeff, scheme == 3 ? MAC_REFLECTION : scheme == 2 ? MACCORMACK : BIMOCQ,
                             myGPUmapper);
    if (!myGPUmapper->ok() || !mysolver.ok()) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }

    // the cells a source of half extents (rx, ry, rz) about (cx, cy, cz) touches get tracers_per_cell tracers each
    long tracers_seeded = 0;
    auto seed_box = [&](float cx, float cy, float cz, float rx, float ry, float rz) {
        if (tracers_per_cell <= 0) return;
        const float c[3] = { cx, cy, cz }, r[3] = { rx, ry, rz };
        int lo[3], hi[3];
        for (int a = 0; a < 3; a++) { lo[a] = (int)std::floor((c[a] - r[a]) / h); hi[a] = (int)std::floor((c[a] + r[a]) / h) + 1; }
        const long added = mysolver.seedTracers(lo, hi, tracers_per_cell, /*seed*/(unsigned)tracers_seeded);
        if (added > 0) tracers_seeded += added;
    };
    if (scene == 1) {
        Emitter a, b;                                                // main.cpp:75-78: 10 frames, density 1, +x velocity ring
        a.emitFrame = b.emitFrame = 10; a.emit_density = b.emit_density = 1.f; a.emit_temperature = b.emit_temperature = 0.f;
        a.emiter = b.emiter = 1.f; a.radius = b.radius = 0.08f;
        // the ring axis passes BETWEEN nodes: a node on it would get 0/0 from the emitter's direction normalisation
        const float yc = 0.5f + 0.37f * h, zc = 0.5f * (float)nk * h + 0.29f * h;
        a.e_pos[0] = 0.15f; a.e_pos[1] = yc; a.e_pos[2] = zc;
        b.e_pos[0] = 0.35f; b.e_pos[1] = yc; b.e_pos[2] = zc;
        mysolver.setSmoke(smoke_drop, smoke_rise, { a, b });
        seed_box(a.e_pos[0], a.e_pos[1], a.e_pos[2], a.radius, a.radius, a.radius);
        seed_box(b.e_pos[0], b.e_pos[1], b.e_pos[2], b.radius, b.radius, b.radius);
    } else if (scene == 2) {
        // the plume of DESIGN.md section 16 with an analytic box in place of the level set: active on every frame,
        // blowing upwards with a slow spin about the vertical axis
        bq_source src{};
        src.shape.shape = BQ_SHAPE_BOX;
        src.shape.cx = 0.5f; src.shape.cy = 0.2f; src.shape.cz = 0.5f;
        src.shape.rx = 0.08f; src.shape.ry = 0.04f; src.shape.rz = 0.08f;
        src.density = src.temperature = 1.f;
        src.ey = 0.5f; src.oy = 0.5f;
        src.emit_frames = total_frame; src.flags = BQ_SOURCE_VELOCITY;
        mysolver.setSmoke(smoke_drop, smoke_rise, {});
        if (!mysolver.setSources(&src, nullptr, 1)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
        seed_box(src.shape.cx, src.shape.cy, src.shape.cz, src.shape.rx, src.shape.ry, src.shape.rz);
    } else {
        Emitter src;                                                 // one warm sphere, applied at frame 0 only
        src.emitFrame = 1; src.emit_density = 1.f; src.emit_temperature = 1.f; src.emiter = 0.f;
        src.e_pos[0] = 0.5f; src.e_pos[1] = 0.2f; src.e_pos[2] = 0.5f; src.radius = 0.1f;
        mysolver.setSmoke(smoke_drop, smoke_rise, { src });
        seed_box(src.e_pos[0], src.e_pos[1], src.e_pos[2], src.radius, src.radius, src.radius);
    }
    if (projection == 1) { mysolver.projection_kind = BQ_PROJECTION_MGCG; mysolver.mg_iters = 50; }
    else                 { mysolver.jacobi_iters = 200; }
    if (!mysolver.setWalls(walls)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }   // (not with projection 1)
    if (paddle_spin != 0.f) {                                        // (not with projection 1: obstacles need Jacobi or PCG)
        bq_boundary box{};
        box.shape = BQ_SHAPE_BOX;
        box.cx = 0.5f * L; box.cy = 0.5f * L; box.cz = 0.5f * (float)nk * h;
        box.rx = 0.3f * L; box.ry = 2.f * h; box.rz = 0.15f * L;
        const bq_pose pose{ 1.f, 0.f, 0.f, 0.f, 0.f, 0.f, paddle_spin };
        if (!mysolver.setBoundary(&box, nullptr, 1, &pose)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    }
    if (!mysolver.setVorticityConfinement(confinement)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    if (diag_every > 0 && !mysolver.setDiagnosticsEvery(diag_every)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    if (loads_every > 0 && !mysolver.setObstacleLoads(loads_every)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    if (fl_last_error() != FL_OK) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    if (tracers_per_cell > 0) std::printf("[ Tracers: %ld ]\n", mysolver.tracer_count);
    mysolver.verbose = true;                                         // "[Bimocq GPU Time: ...ms ]" like the reference

    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < total_frame; i++) {
        std::printf("Frame %d Starts !!!\n", i);
        if (paddle_spin != 0.f && !mysolver.updateBoundary(i, dt)) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
        mysolver.advance(i, dt);
        if (async_dump) mysolver.outputResultAsync((unsigned)i, filepath);      // written while frame i + 1 runs
        else std::printf("[ Valid voxel: %ld ]\n", mysolver.outputResult((unsigned)i, filepath));
        if (diag_every > 0 && (i + 1) % diag_every == 0)
            std::printf("[ Vorticity voxel: %ld ]\n", mysolver.outputVorticity((unsigned)i, filepath, 0.1f));
        if (preview_every > 0 && (i + 1) % preview_every == 0)         // eye looking along +z, light falling along -y
            std::printf("[ Preview bytes: %ld ]\n", preview_solids
                ? mysolver.outputPreviewSolids((unsigned)i, filepath, /*view +z*/4, /*light -y*/3, 12.f, 1.f, 0.1f, 0.6f, 0.15f, 0.f)
                : mysolver.outputPreview((unsigned)i, filepath, /*view +z*/4, /*light -y*/3, 12.f, 1.f, 0.1f, 0.f));
        if (loads_every > 0 && !mysolver.boundaries.empty() && (i + 1) % loads_every == 0) {
            double row[BQ_OLOAD_ROW];
            if (mysolver.obstacleLoads(row) == 1)
                for (int o = 0; o < (int)row[BQ_OLOAD_N]; o++) {
                    const double *q = row + BQ_OLOAD_HEADER + o * BQ_OLOAD_COUNT;
                    std::printf("loads frame %d obstacle %d force %.9e %.9e %.9e torque %.9e %.9e %.9e area %.9e\n", i, o, q[BQ_OLOAD_FX],
                                q[BQ_OLOAD_FY], q[BQ_OLOAD_FZ], q[BQ_OLOAD_TX], q[BQ_OLOAD_TY], q[BQ_OLOAD_TZ], q[BQ_OLOAD_AREA]);
                }
        }
        if (tracers_per_cell > 0)
            std::printf("[ Tracer bytes: %ld ]\n", mysolver.outputTracers((unsigned)i, filepath, BQ_F_RHO));
        if (fl_last_error() != FL_OK) { std::fprintf(stderr, "%s\n", fl_last_error_string()); return 1; }
    }
    if (diag_every > 0) {                                            // the samples waited in device memory: one download for all of them
        std::vector<double> rows((size_t)BimocqGPUSolver::kDiagRing * BQ_DIAG_COUNT);
        const long kept = mysolver.diagnosticsHistory(rows.data(), BimocqGPUSolver::kDiagRing);
        for (long r = 0; r < kept; r++) {
            const double *d = rows.data() + (size_t)r * BQ_DIAG_COUNT;
            std::printf("[diag step %d] kinetic %.9e enstrophy %.9e div_l2 %.3e div_max %.3e rho_sum %.6f centroid %.5f %.5f %.5f vort_max %.5f\n",
                        (int)d[BQ_DIAG_STEP], d[BQ_DIAG_KINETIC], d[BQ_DIAG_ENSTROPHY], d[BQ_DIAG_DIV_L2], d[BQ_DIAG_DIV_MAX], d[BQ_DIAG_RHO_SUM],
                        d[BQ_DIAG_CENTROID_X], d[BQ_DIAG_CENTROID_Y], d[BQ_DIAG_CENTROID_Z], d[BQ_DIAG_VORT_MAX]);
        }
    }
    if (paddle_spin != 0.f) {
        const std::array<double, 4> &q = mysolver.orientations[0];
        std::printf("[ Paddle orientation: %.9f %.9f %.9f %.9f ]\n", q[0], q[1], q[2], q[3]);
    }
    const long last = async_dump ? mysolver.waitOutput() : 0;
    fl_sync();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%d frames of %dx%dx%d in %.3f s (%.1f Mvoxels/s incl. dumps)%s\n", total_frame, ni, nj, nk, sec,
                (double)ni * nj * nk * total_frame / sec / 1e6, async_dump ? (last >= 0 ? ", last dump ok" : ", last dump FAILED") : "");
    return 0;
}
