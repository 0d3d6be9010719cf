// bq_mgcg_slab.hip.inc -- the fp64 multigrid-CG projection DECOMPOSED over z-slab ranks (round 4).  Included by bq_mgcg.hip
// inside namespace bq: it is made of that file's launchers (mg_smooth, mg_residual, mg_dot's two halves, the transfer
// operators), applied to z-ranges of arrays.
//
// Round 3 ran this projection replicated on slab ranks (csrc/host/fluid_solver.cpp: projectionMgcgSlabs): every rank gathers
// the whole velocity and solves the whole grid -- exact, but six global fp64 arrays per rank and no scaling at all, although
// the solve is ~90 % of an MGCG step.  Here a rank holds, of every level it shares, only the planes it owns plus ghost planes:
//
//   level l, global planes [0, nk_l):  rank r owns [own0_l, own1_l), stores [lo_l, hi_l) = own +- G_l planes clipped to the grid.
//   Ownership nests along the reference's pyramid n -> (n - 1) / 2 (GPU_kernel.cu:1636-1707): coarse plane K belongs to the rank
//   that owns fine plane 2 K + 1, the centre of the planes 2 K .. 2 K + 2 the restriction reads (:1553-1608).
//
// Every operator of the cycle is a single-GPU launcher on a z-RANGE of such arrays (a range of planes of an x-fastest array is an
// array): the kernels see a smaller grid whose first / last plane they treat as boundary -- the grid's real boundary where the
// range ends there, a ghost plane otherwise.  Ghost planes are computed redundantly, exactly like the neighbour computes them
// (same operands, same order), and go stale one plane per stencil application from the range's ends inwards; they are refreshed
// by the neighbour exchange of bq_halo.hip (fl_halo_exchange on the double planes as pairs of floats) before that reaches an owned
// plane: 32 smoothing sweeps are 4 chunks of 8 with G = 8.  Levels that are too thin to share (fewer than ~10 planes per rank)
// are gathered -- one point-to-point group -- and run replicated on every rank through the same code as on one GPU.
//
// What keeps it bit-identical to one GPU (and to the oracle's single-domain solve):
//   * the float-narrowed block dot products (M1): a block is 256 consecutive flat indices; with planes of a multiple of 256 cells
//     slab boundaries are block boundaries, so a rank computes exactly the global partials of its planes, the partials are
//     all-gathered, and the final sums run on the whole partial array in the reference's order -- on every rank alike;
//   * maxima are order-free: local maximum, then an all-reduce;
//   * the transfer operators index the coarse array by flat index with the reference's wrap at row and plane ends (M4): a range
//     that starts at an even fine plane f0 pairs with the coarse range that starts at f0 / 2, and whatever a wrap reaches beyond a
//     range's last plane only ever feeds the outermost ghost planes.
// Requirements (else the caller keeps the replicated path): planes of a multiple of 256 cells, equal slabs of a multiple of 8
// planes, at least 17 of them -- the same answer on every rank.  The predicate, the pyramid, every plane range and every count
// or offset derived from them are stated once in bq_mgcg_slab_plan.h (host-only, swept on the CPU by
// tests/test_mgcg_slab_plan_cpu.py); this file allocates and launches by that plan and computes no geometry of its own.
struct SlabLevel : mgslab::Level {          // dims, owned / stored planes, ghost depth, transfer and exchange numbers: the plan's
    double alpha = -1.0, beta = 1.0 / 6.0;
    double *x = nullptr, *b = nullptr, *r = nullptr;
    size_t plane() const { return (size_t)ni * nj; }
    int nkl() const { return hi - lo; }
};

struct SlabMg {
    bool ready = false;
    mgslab::Plan plan;                      // what everything below was allocated by
    int nranks = 1;
    int LS = 0;                             // levels [0, LS) are shared, [LS, levels) replicated
    int nlevels = 0;
    SlabLevel lv[LEVEL_COUNT];
    SCoarseLevelInfo full[LEVEL_COUNT];     // the replicated levels (entries [LS, nlevels) valid), global arrays
    // level-0 conjugate-gradient vectors on [lo, hi)
    double *div = nullptr, *p = nullptr, *dir = nullptr, *residual = nullptr, *temp0 = nullptr, *temp1 = nullptr;
    double *temp_full = nullptr;            // ping-pong buffer of the replicated levels' smoothing
    double *partials = nullptr;             // one per 256-cell block of the GLOBAL level-0 array
    std::vector<void *> owned;              // everything allocated here
};

static void slab_mg_release(SlabMg &m)
{
    for (void *p : m.owned) (void)hipFree(p);
    m = SlabMg();
}

static double *slab_alloc(SlabMg &m, size_t doubles)
{
    void *p = nullptr;
    if (!BQ_HIP(hipMalloc(&p, std::max<size_t>(doubles, 1) * sizeof(double)))) return nullptr;
    if (!BQ_HIP(hipMemsetAsync(p, 0, std::max<size_t>(doubles, 1) * sizeof(double), rt().compute))) { (void)hipFree(p); return nullptr; }
    m.owned.push_back(p);
    return (double *)p;
}

// refresh `depth` ghost planes of a level's array on both sides (blocking for the compute stream)
static void slab_exchange(const SlabLevel &L, double *arr, int depth)
{
    if (comm_ranks() <= 1 || depth <= 0) return;
    if (depth > L.G) depth = L.G;
    // fl_halo_exchange addresses a buffer of own + 2 G planes that starts G planes below the first owned one; a range clipped
    // at the grid's end starts later, so the base is moved back by the planes that do not exist (never touched: the rank
    // there has no neighbour on that side)
    const size_t pd = L.plane();
    float *base = (float *)(arr - (ptrdiff_t)pd * (ptrdiff_t)L.xch_shift);
    float *fields[1] = { base };
    const size_t pe[1] = { pd * 2 };
    const int extra[1] = { 0 };
    fl_halo_exchange(1, fields, pe, extra, L.xch_nk_local, L.G, depth, 1);
}

// `iter` (even) smoothing sweeps of level L on its stored range, ghost planes refreshed every G sweeps.  x_zero: x counts as
// cleared (V_Cycle's way down).  On return x is correct on the owned planes and on G - (sweeps since the last exchange) ghosts.
static void slab_smooth(const SlabLevel &L, const double *rhs, double *temp, double scale, int iter, bool x_zero)
{
    int done = 0;
    const int chunk = std::max(2, L.G - (L.G % 2));
    while (done < iter) {
        const int n = std::min(chunk, iter - done);
        if (done > 0) slab_exchange(L, L.x, L.G);
        const bool zero = x_zero && done == 0;
        if (!mg_smooth_tiled(L.x, rhs, temp, L.alpha * scale, L.beta, L.ni, L.nj, L.nkl(), n, zero))
            mg_smooth(L.x, rhs, temp, L.alpha * scale, L.beta, L.ni, L.nj, L.nkl(), n, zero ? 3 : 1);
        done += n;
    }
}

// all ranks' owned planes of an array of level L -> the global array `full` on every rank (one point-to-point group)
static void slab_gather_planes(const SlabMg &m, int l, const double *local, double *full)
{
    const SlabLevel &L = m.lv[l];
    const size_t pd = L.plane();
    BQ_HIP(hipMemcpyAsync(full + pd * (size_t)L.own0, local + pd * (size_t)(L.own0 - L.lo), pd * (size_t)(L.own1 - L.own0) * sizeof(double),
                          hipMemcpyDeviceToDevice, rt().compute));
    if (m.nranks <= 1) return;
    std::vector<int> peers; std::vector<float *> send, recv; std::vector<size_t> sc, rc;
    for (int r = 0; r < m.nranks; r++) {
        if (r == m.plan.rank) continue;
        const mgslab::Range o = m.plan.own(r, l);
        peers.push_back(r);
        send.push_back((float *)(local + pd * (size_t)(L.own0 - L.lo)));
        sc.push_back(pd * 2 * (size_t)(L.own1 - L.own0));
        recv.push_back((float *)(full + pd * (size_t)o.a));
        rc.push_back(pd * 2 * (size_t)std::max(0, o.b - o.a));
    }
    fl_p2p_exchange((int)peers.size(), peers.data(), send.data(), sc.data(), recv.data(), rc.data());
}

// the reference's dot product (dot_vector + calc_sum) of two level-0 vectors over the whole grid -> result[iter_index]
static void slab_dot(const SlabMg &m, const double *v0, const double *v1, double *result, int iter_index)
{
    const SlabLevel &L = m.lv[0];
    const size_t pd = L.plane(), off = pd * (size_t)(L.own0 - L.lo), own_cells = pd * (size_t)(L.own1 - L.own0);
    const unsigned nb_own = (unsigned)m.plan.dot_nb_own, nb = (unsigned)m.plan.dot_nb;
    const size_t first = (size_t)m.plan.dot_first;                      // (planes are multiples of 256 cells)
    hipStream_t st = rt().compute;
    mg_dot_kernel<<<nb_own, 256, 0, st>>>(v0 + off, v1 + off, m.partials + first, own_cells);
    BQ_LAUNCH_CHECK("mg_dot_kernel");
    if (m.nranks > 1) {
        std::vector<int> peers; std::vector<float *> send, recv; std::vector<size_t> sc, rc;
        for (int r = 0; r < m.nranks; r++) {
            if (r == m.plan.rank) continue;
            const size_t f = (size_t)m.plan.dot_first_of(r), n = (size_t)m.plan.dot_nb_of(r);
            peers.push_back(r);
            send.push_back((float *)(m.partials + first)); sc.push_back((size_t)nb_own * 2);
            recv.push_back((float *)(m.partials + f));     rc.push_back(n * 2);
        }
        fl_p2p_exchange((int)peers.size(), peers.data(), send.data(), sc.data(), recv.data(), rc.data());
    }
    mg_dot_finish(m.partials, result, nb, iter_index);
}

static void slab_max(const SlabMg &m, const double *v, double *result, int iter_index)
{
    const SlabLevel &L = m.lv[0];
    const size_t pd = L.plane();
    mg_max(v + pd * (size_t)(L.own0 - L.lo), result, pd * (size_t)(L.own1 - L.own0), iter_index);
    (void)comm_allreduce(result + iter_index, 1, true, true, rt().compute);
}

// gradient_kernel, double p (GPU_kernel.cu:1009-1023) on a slab rank: p stores the planes [plo, phi), the velocity buffers the
// planes from ulo on; window 2 <= index < p-dims in GLOBAL indices
__global__ __launch_bounds__(256) void mg_gradient_slab_kernel(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w,
                                                               const double *__restrict__ p, int ni, int nj, int nkg, int plo, int phi,
                                                               int ulo, int k_first, double halfrdx)
{
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, kg = blockIdx.z + k_first;
    if (i >= ni + 1 || j >= nj + 1 || kg >= phi) return;
    if (i > 1 && i < ni && j > 1 && j < nj && kg > 1 && kg < nkg && kg - 1 >= plo) {
        const size_t sj = ni, sk = (size_t)ni * nj;
        const size_t id = id3(i, j, kg - plo, ni, nj);
        const int ku = kg - ulo;
        const double p0 = p[id];
        u[id3(i, j, ku, ni + 1, nj)] -= (float)(halfrdx * (p0 - p[id - 1]));
        v[id3(i, j, ku, ni, nj + 1)] -= (float)(halfrdx * (p0 - p[id - sj]));
        w[id3(i, j, ku, ni, nj)]     -= (float)(halfrdx * (p0 - p[id - sk]));
    }
}

static bool same_plan(const mgslab::Plan &a, const mgslab::Plan &b)
{
    return a.ni == b.ni && a.nj == b.nj && a.nkg == b.nkg && a.ghost == b.ghost && a.rank == b.rank && a.nranks == b.nranks;
}

// the arrays of a supported plan (the caller has checked plan.supported: nothing here depends on the geometry any more, what can
// still fail is an allocation)
static bool slab_mg_setup(SlabMg &m, const mgslab::Plan &plan)
{
    if (m.ready && same_plan(m.plan, plan)) return true;
    (void)hipStreamSynchronize(rt().compute);
    slab_mg_release(m);
    m.plan = plan;
    m.nranks = plan.nranks; m.nlevels = plan.nlevels; m.LS = plan.LS;
    const int LS = plan.LS, nl = plan.nlevels;
    for (int l = 0; l < nl; l++) static_cast<mgslab::Level &>(m.lv[l]) = plan.lv[l];
    for (int l = 0; l < LS; l++) {
        SlabLevel &L = m.lv[l];
        const size_t cells = L.plane() * (size_t)L.nkl();
        L.x = slab_alloc(m, cells); L.b = slab_alloc(m, cells); L.r = slab_alloc(m, cells);
        if (!L.x || !L.b || !L.r) return false;
    }
    size_t biggest = 1;
    for (int l = LS; l < nl; l++) {
        SCoarseLevelInfo &F = m.full[l];
        F.ni = m.lv[l].ni; F.nj = m.lv[l].nj; F.nk = m.lv[l].nk; F.number = F.ni * F.nj * F.nk;
        F.alpha = -1.0; F.beta = 1.0 / 6.0;
        F.b = slab_alloc(m, (size_t)F.number); F.x = slab_alloc(m, (size_t)F.number); F.r = slab_alloc(m, (size_t)F.number);
        if (!F.b || !F.x || !F.r) return false;
        biggest = std::max(biggest, (size_t)F.number);
    }
    m.temp_full = slab_alloc(m, biggest);
    if (!m.temp_full) return false;
    // (level LS, the first replicated one, carries this rank's planes of it as the gather sees them, stored in full; that a fine
    // range [lo, hi) finds the coarse range from lo / 2 on stored is part of plan.supported, for every rank alike)
    const SlabLevel &L0 = m.lv[0];
    const size_t c0 = L0.plane() * (size_t)L0.nkl();
    m.div = slab_alloc(m, c0); m.p = slab_alloc(m, c0); m.dir = slab_alloc(m, c0); m.residual = slab_alloc(m, c0);
    m.temp0 = slab_alloc(m, c0); m.temp1 = slab_alloc(m, c0);
    m.partials = slab_alloc(m, (size_t)blocks1d(L0.plane() * (size_t)L0.nk) + 256);
    if (!m.div || !m.p || !m.dir || !m.residual || !m.temp0 || !m.temp1 || !m.partials) return false;
    m.ready = true;
    return true;
}

// V_Cycle (GPU_kernel.cu:1636-1707) with the levels [0, LS) on slabs.  b: level 0's right-hand side of the outer iteration
// (div), x: its solution (p), residual: r = b - A x on entry (correct on every stored plane but the outermost), the new residual
// on return.
static void slab_v_cycle(SlabMg &m, bool last_iteration)
{
    double scale[LEVEL_COUNT] = { 1.0, 1.0, 1.0, 1.0, 1.0, 1.0 };
    scale[1] = 8.0;                                                                          // M3
    hipStream_t st = rt().compute;
    const int LS = m.LS, nl = m.nlevels;
    // the reference copies the residual into L[0].b (:1640); what L[0].b holds afterwards is never read by anyone, so the
    // residual itself serves as level 0's right-hand side (bq_mgcg.hip: v_cycle, copy_b)
    (void)last_iteration;
    auto rhs = [&](int l) -> const double * { return l == 0 ? m.residual : m.lv[l].b; };
    // ---- down: shared levels ----
    for (int l = 0; l < LS; l++) {
        SlabLevel &L = m.lv[l];
        slab_smooth(L, rhs(l), m.temp0, scale[l], 32, true);
        slab_exchange(L, L.x, L.G);
        mg_residual(L.r, rhs(l), L.x, L.ni, L.nj, L.nkl());
        // restriction onto the next level's OWNED planes; the fine range starts at twice the first coarse plane
        const int c0 = L.rest_c0, ck = L.rest_ck, fine_planes = L.rest_fine_planes;
        const int ci = m.lv[l + 1].ni, cj = m.lv[l + 1].nj;
        const double *fine = L.r + L.plane() * (size_t)(L.rest_fine0 - L.lo);
        if (l + 1 < LS) {
            SlabLevel &C = m.lv[l + 1];
            if (ck > 0)
                mg_restrict_kernel<<<grid_for(ci, cj, ck), kBlock, 0, st>>>(fine, C.b + C.plane() * (size_t)(c0 - C.lo), L.ni, L.nj, fine_planes, ci, cj, ck);
            BQ_LAUNCH_CHECK("mg_restrict_kernel");
            slab_exchange(C, C.b, C.G);
        } else {
            // the first replicated level: owned planes into a scratch range of its r array, gathered into its b on every rank
            SCoarseLevelInfo &F = m.full[l + 1];
            const size_t pc = (size_t)ci * cj;
            if (ck > 0)
                mg_restrict_kernel<<<grid_for(ci, cj, ck), kBlock, 0, st>>>(fine, F.r + pc * (size_t)c0, L.ni, L.nj, fine_planes, ci, cj, ck);
            BQ_LAUNCH_CHECK("mg_restrict_kernel");
            // (every rank's planes land at their global position of F.b)
            slab_gather_planes(m, l + 1, F.r, F.b);
        }
    }
    // ---- replicated levels: the single-GPU cycle from level LS down and back up to it ----
    {
        const SCoarseLevelInfo *F = m.full;
        const int lb = nl - 2;
        const bool bottom = rt().opt_mgcg_bottom && rt().opt_mgcg_tile && nl - LS >= 2 && F[lb].number <= kBottomA && F[lb + 1].number <= kBottomB &&
                            F[lb].number > 0 && F[lb + 1].number > 0 && lb >= LS;
        auto smooth_full = [&](int l, int iter, bool clear_x) {
            if (mg_smooth_tiled(F[l].x, F[l].b, m.temp_full, F[l].alpha * scale[l], F[l].beta, F[l].ni, F[l].nj, F[l].nk, iter, clear_x)) return;
            mg_smooth(F[l].x, F[l].b, m.temp_full, F[l].alpha * scale[l], F[l].beta, F[l].ni, F[l].nj, F[l].nk, iter, clear_x ? 3 : 1);
        };
        for (int l = LS; l < (bottom ? lb : nl - 1); l++) {
            smooth_full(l, 32, true);
            mg_residual(F[l].r, F[l].b, F[l].x, F[l].ni, F[l].nj, F[l].nk);
            mg_restrict_kernel<<<grid_for(F[l + 1].ni, F[l + 1].nj, F[l + 1].nk), kBlock, 0, st>>>(F[l].r, F[l + 1].b, F[l].ni, F[l].nj, F[l].nk, F[l + 1].ni, F[l + 1].nj, F[l + 1].nk);
            BQ_LAUNCH_CHECK("mg_restrict_kernel");
        }
        if (bottom) {
            mg_vbottom_kernel<<<1, 1024, 0, st>>>(F[lb].b, F[lb].x, F[lb].r, F[lb + 1].b, F[lb + 1].x, F[lb].ni, F[lb].nj, F[lb].nk,
                                                   F[lb + 1].ni, F[lb + 1].nj, F[lb + 1].nk, F[lb].alpha * scale[lb], F[lb].beta,
                                                   F[lb + 1].alpha * scale[lb + 1], F[lb + 1].beta);
            BQ_LAUNCH_CHECK("mg_vbottom_kernel");
        } else smooth_full(nl - 1, 32, true);
        for (int l = bottom ? lb - 1 : nl - 2; l >= LS; --l) {
            mg_prolong_kernel<<<grid_for(F[l].ni, F[l].nj, F[l].nk), kBlock, 0, st>>>(F[l].x, F[l + 1].x, F[l].ni, F[l].nj, F[l].nk, F[l + 1].ni, F[l + 1].nj, F[l + 1].nk);
            BQ_LAUNCH_CHECK("mg_prolong_kernel");
            smooth_full(l, 4, false);
        }
    }
    // ---- up: shared levels ----
    for (int l = LS - 1; l >= 0; --l) {
        SlabLevel &L = m.lv[l];
        // coarse correction: the fine range [lo, hi) (lo even) samples the coarse range that starts at lo / 2
        const double *coarse; int ck;
        const int ci = m.lv[l + 1].ni, cj = m.lv[l + 1].nj;
        if (l + 1 < LS) {
            SlabLevel &C = m.lv[l + 1];
            slab_exchange(C, C.x, C.G);
            coarse = C.x + C.plane() * (size_t)(L.prol_c0 - C.lo);
        } else {
            coarse = m.full[l + 1].x + (size_t)ci * cj * (size_t)L.prol_c0;
        }
        ck = L.prol_ck;
        mg_prolong_kernel<<<grid_for(L.ni, L.nj, L.nkl()), kBlock, 0, st>>>(L.x, coarse, L.ni, L.nj, L.nkl(), ci, cj, ck);
        BQ_LAUNCH_CHECK("mg_prolong_kernel");
        slab_exchange(L, L.x, L.G);
        slab_smooth(L, rhs(l), m.temp0, scale[l], 4, false);
    }
    // x += L[0].x ; residual = b - A x
    const SlabLevel &L0 = m.lv[0];
    const size_t n0 = L0.plane() * (size_t)L0.nkl();
    slab_exchange(L0, L0.x, L0.G);
    mg_add_kernel<<<blocks1d(n0), 256, 0, st>>>(m.p, L0.x, 1.0, n0);
    BQ_LAUNCH_CHECK("mg_add_kernel");
    mg_residual(m.residual, m.div, m.p, L0.ni, L0.nj, L0.nkl());
}
