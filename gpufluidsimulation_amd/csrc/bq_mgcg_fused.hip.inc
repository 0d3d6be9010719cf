// ---- level-0 vector updates fused into the stencil pass that follows them (FL_OPT_MGCG_FUSE) -------------------------------
// Included by bq_mgcg.hip (namespace bq) after mg_stencil_lean_kernel.  One outer iteration of the multigrid-CG loop
// (GPU_kernel.cu:1764-1815) makes nine separate passes over the level-0 arrays next to the smoothing sweeps:
//     update_x (p += dir a0/a1), residual (r = div - A p)                          -> kFuseXRes
//     add (p += L0.x), residual, calc_max(r), dot(r, r)                            -> kFuseAddRes
//     update_dir (dir = r + dir b2/b0), poisson (t = A dir), dot(dir, t)           -> kFuseDirPoi
// Each group is ONE launch of mg_fused_kernel here: mg_stencil_lean_kernel's z-march in which the vector that the stencil
// reads is made on the fly -- xnew = base + (d * num) / den, or base + d * mul, the reference's expressions (:1275-1338),
// evaluated on every row / plane the thread loads (the halo rows a second time: a division costs less than the second trip
// through memory) -- and stored by the thread that owns the cell, rim rows / planes / columns included (the reference's
// updates run over all `count` elements).  xnew goes to a buffer OTHER than base and d: a neighbour thread may still have to
// read the old values of a cell its owner has already replaced (the caller ping-pongs: p -> temp1 -> p, dir <-> levels[0].b).
// The dot products keep the reference's summation tree (dot_vector_kernel, :1087-1126): 256 consecutive elements per partial
// = one row (half a row at nx = 512), 16 sequential sums of 16 rounded to float, then the 16-term sum with its four raw
// products; a block parks the products of a trip of four planes in LDS and 256 / 16 threads run the two stages.  The max is
// order-free.  Rim elements of `out` -- never written by the stencil -- enter the sums with what memory holds there: rim
// columns are read by their lanes here, partials made of rim rows / planes only come from mg_rim_dot_kernel.
// Shapes: nx = 256 or 512 (a row = 2 or 4 waves of double2 columns), arrays below 2 GB, 16-byte aligned.
enum { kFuseXRes = 0, kFuseAddRes = 1, kFuseDirPoi = 2 };
struct FuseArgs {
    const double *base, *d, *rhs;       // xnew = base (+) d; rhs: the right-hand side of the residual modes
    double *xout, *out;                 // xnew; r = rhs - A xnew or t = A xnew (interior cells)
    const double *coef;                 // tempResult: num = coef[num_idx], den = coef[den_idx] (XRes, DirPoi)
    int num_idx, den_idx;
    double mul;                         // AddRes: xnew = base + d * mul
    double *partials, *maxpart;         // dot partials (one per 256 elements, the reference's index), max per block
    int nx, ny, nz, cw, nby, kchunk;
};

constexpr int kProdStride = 288;        // 16 groups of 16 products, a group every 18 doubles (LDS banks)
__device__ __forceinline__ int prod_at(int e) { return (e >> 4) * 18 + (e & 15); }

// dot_vector_kernel's second and third stage on the products of one partial (`pr`: prod_at layout), by 16 + 1 threads
__device__ __forceinline__ double dot_group_sum(const double *pr, int g)
{
    double s = pr[g * 18];
#pragma unroll
    for (int q = 1; q < 16; q++) s = s + pr[g * 18 + q];
    return (double)(float)s;                                        // `float sum0`
}
__device__ __forceinline__ double dot_final_sum(const double *gs, const double *pr)
{
    const double s = gs[0] + gs[1] + gs[2] + pr[3] + gs[4] + gs[5] + gs[6] + pr[7] +
                     gs[8] + gs[9] + gs[10] + pr[11] + gs[12] + gs[13] + gs[14] + pr[15];
    return (double)(float)s;                                        // `float sum`
}

template <int MODE>
__global__ __launch_bounds__(256) void mg_fused_kernel(const FuseArgs A)
{
    constexpr bool DIV = MODE != kFuseAddRes, POISSON = MODE == kFuseDirPoi, DOT = MODE != kFuseXRes, MAXV = MODE == kFuseAddRes;
    __shared__ __attribute__((aligned(16))) double prod[DOT ? 16 * kProdStride : 2];
    __shared__ double gsum[DOT ? 256 : 1];
    __shared__ double mred[MAXV ? 256 : 1];
    const int nx = A.nx, ny = A.ny, nz = A.nz, cw = A.cw, nby = A.nby, kchunk = A.kchunk;
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);      // XCD-contiguous block order
    const int by = b % nby, bz = b / nby;
    const int rows = 256 / cw;                                      // row pairs per block: 2 (nx = 256) or 1 (nx = 512)
    const int c = threadIdx.x % cw;
    const int r = __builtin_amdgcn_readfirstlane((int)threadIdx.x / cw);
    const int x = 2 * c, j = 2 * (by * rows + r);
    const int kbeg = max(1, bz * kchunk), kend = min(nz - 1, bz * kchunk + kchunk);
    if (kbeg >= kend) {
        if (MAXV && threadIdx.x == 0) A.maxpart[b] = 0.0;
        return;
    }
    const bool xlo = x == 0, xhi = x + 1 == nx - 1;
    const bool rowv[2] = { j < ny, j + 1 < ny };                                    // the row exists (xnew is stored)
    const bool rowi[2] = { j >= 1 && j <= ny - 2, j + 1 >= 1 && j + 1 <= ny - 2 };  // ... and is interior (stencil, sums)
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * 8u;
    const v4i rb = make_rsrc4(A.base, bytes), rdd = make_rsrc4(A.d, bytes), rr = make_rsrc4(POISSON ? A.base : A.rhs, bytes);
    const v4i rx = make_rsrc4(A.xout, bytes), ro = make_rsrc4(A.out, bytes);
    unsigned vo[4];                                                 // rows j-1 .. j+2 (clamped into the array)
#pragma unroll
    for (int a = 0; a < 4; a++) vo[a] = ((unsigned)x + (unsigned)nx * (unsigned)min(max(j - 1 + a, 0), ny - 1)) * 8u;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * 8u;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    // the x neighbour of a wave's first / last lane is the column just outside the wave, rows j, j+1
    const int lane = threadIdx.x & 63;
    const bool edgeL = lane == 0 && x > 0, edgeR = lane == 63 && x + 2 < nx;
    const int xe = edgeL ? x - 1 : (edgeR ? x + 2 : x);
    unsigned ve[2], vb[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        ve[a] = (edgeL || edgeR) ? ((unsigned)xe + (unsigned)nx * (unsigned)min(max(j + a, 0), ny - 1)) * 8u : 0x80000000u;
        // the rim column of rows j, j+1 (lanes at either end of the row): what `out` holds there enters the sums
        vb[a] = (DOT && (xlo || xhi) && rowi[a]) ? vo[a + 1] + (xhi ? 8u : 0u) : 0x80000000u;
    }
    double num = 0.0, den = 1.0;
    if (DIV) { num = A.coef[A.num_idx]; den = A.coef[A.den_idx]; }
    const double mul = A.mul;
    auto comb = [&](double bs, double dv) -> double { return DIV ? bs + (dv * num) / den : bs + dv * mul; };
    auto comb2 = [&](D2 bs, D2 dv) -> D2 { return D2{comb(bs.a, dv.a), comb(bs.b, dv.b)}; };
    // where this lane's two products of row rr go: element index in the block's four partials of a plane
    int pslot[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int flat = (r * 2 + a) * nx + x;
        pslot[a] = (flat >> 8) * kProdStride + prod_at(flat & 255);
    }

    // rings over planes (compile-time slots): X[.][0..3] = xnew on rows j-1 .. j+2 of the planes q-1, q, q+1 and -- still
    // `base`, its d in DD -- the one arriving; R = rhs rows j, j+1; EB / ED = base and d of the outside column
    D2 X[4][4], DD[4], R[2][2];
    double EB[2][2], ED[2][2];
    double mx = 0.0;
    int q = kbeg;
    {
        const unsigned pm = po(q - 1), pc = po(q), pn = po(q + 1);
        D2 d0[4], d1[4];
#pragma unroll
        for (int a = 0; a < 4; a++) {
            X[3][a] = ld_d2(rb, vo[a], pm); d0[a] = ld_d2(rdd, vo[a], pm);
            X[0][a] = ld_d2(rb, vo[a], pc); d1[a] = ld_d2(rdd, vo[a], pc);
            X[1][a] = ld_d2(rb, vo[a], pn); DD[a] = ld_d2(rdd, vo[a], pn);
        }
        if (!POISSON) { R[0][0] = ld_d2(rr, vo[1], pc); R[0][1] = ld_d2(rr, vo[2], pc); }
        EB[0][0] = ld_d(rb, ve[0], pc); EB[0][1] = ld_d(rb, ve[1], pc);
        ED[0][0] = ld_d(rdd, ve[0], pc); ED[0][1] = ld_d(rdd, ve[1], pc);
#pragma unroll
        for (int a = 0; a < 4; a++) { X[3][a] = comb2(X[3][a], d0[a]); X[0][a] = comb2(X[0][a], d1[a]); }
        if (q - 1 == 0) {                                           // the first chunk owns plane 0
            if (rowv[0]) st_d2<0>(X[3][1], rx, vo[1], 0u);
            if (rowv[1]) st_d2<0>(X[3][2], rx, vo[2], 0u);
        }
    }
#define MG_FU_PHASE(T)                                                                                              \
    {                                                                                                               \
        constexpr int im = (T + 3) & 3, ic = T, in_ = (T + 1) & 3, ia = (T + 2) & 3, rc = T & 1, rn = (T + 1) & 1;     \
        const unsigned pa = po(q + 2), pb = po(q + 1), pk = pstride * (unsigned)q;                                  \
        _Pragma("unroll") for (int a = 0; a < 4; a++) X[in_][a] = comb2(X[in_][a], DD[a]);      /* plane q+1 arrived */ \
        _Pragma("unroll") for (int a = 0; a < 4; a++) { X[ia][a] = ld_d2(rb, vo[a], pa); DD[a] = ld_d2(rdd, vo[a], pa); } \
        if (!POISSON) { R[rn][0] = ld_d2(rr, vo[1], pb); R[rn][1] = ld_d2(rr, vo[2], pb); }                         \
        EB[rn][0] = ld_d(rb, ve[0], pb); EB[rn][1] = ld_d(rb, ve[1], pb);                                           \
        ED[rn][0] = ld_d(rdd, ve[0], pb); ED[rn][1] = ld_d(rdd, ve[1], pb);                                         \
        double ob[2] = { 0.0, 0.0 };                                                                                \
        if (DOT) { ob[0] = ld_d(ro, vb[0], pk); ob[1] = ld_d(ro, vb[1], pk); }                                      \
        if (q + 1 == nz - 1) {                                      /* the last chunk owns plane nz-1 */             \
            if (rowv[0]) st_d2<0>(X[in_][1], rx, vo[1], pb);                                                        \
            if (rowv[1]) st_d2<0>(X[in_][2], rx, vo[2], pb);                                                        \
        }                                                                                                           \
        _Pragma("unroll") for (int rw = 0; rw < 2; rw++) {                                                           \
            const D2 ce = X[ic][rw + 1], fr = X[ic][rw], bk = X[ic][rw + 2], dn = X[im][rw + 1], up = X[in_][rw + 1]; \
            if (rowv[rw]) st_d2<0>(ce, rx, vo[rw + 1], pk);                                                         \
            double left = lane_up(ce.b), right = lane_down(ce.a);                                                   \
            const double outside = comb(EB[rc][rw], ED[rc][rw]);                                                    \
            if (edgeL) left = outside;                                                                              \
            if (edgeR) right = outside;                                                                             \
            D2 o;                                                                                                   \
            o.a = (left + ce.b + fr.a + bk.a + dn.a + up.a) - ce.a * 6;                                             \
            o.b = (ce.a + right + fr.b + bk.b + dn.b + up.b) - ce.b * 6;                                            \
            if (!POISSON) { o.a = R[rc][rw].a - o.a; o.b = R[rc][rw].b - o.b; }                                     \
            if (rowi[rw]) {                                                                                         \
                if (!xlo && !xhi) st_d2<0>(o, ro, vo[rw + 1], pk);                                                  \
                else if (xlo && !xhi) bq_buffer_store_x2(__builtin_bit_cast(v2f, o.b), ro, (int)(vo[rw + 1] + 8u), (int)pk, 0); \
                else if (xhi && !xlo) bq_buffer_store_x2(__builtin_bit_cast(v2f, o.a), ro, (int)vo[rw + 1], (int)pk, 0); \
                if (DOT) {                                                                                          \
                    if (xlo) o.a = ob[rw];                                                                          \
                    if (xhi) o.b = ob[rw];                                                                          \
                    if (MAXV) mx = fmax(mx, fmax(o.a, o.b));                                                        \
                    const D2 pv = POISSON ? D2{ce.a * o.a, ce.b * o.b} : D2{o.a * o.a, o.b * o.b};                  \
                    *reinterpret_cast<v2d *>(&prod[T * 4 * kProdStride + pslot[rw]]) = v2d{pv.a, pv.b};             \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        q++;                                                                                                        \
    }
    while (true) {
        const int q0 = q;
        int np = 1;
        MG_FU_PHASE(0)
        if (q < kend) {
            np = 2;
            MG_FU_PHASE(1)
            if (q < kend) {
                np = 3;
                MG_FU_PHASE(2)
                if (q < kend) {
                    np = 4;
                    MG_FU_PHASE(3)
                }
            }
        }
        if (DOT) {      // the partials of this trip's planes: 16 slots = 4 planes x 4 partials (2 rows x 2 halves, or 4 rows)
            __syncthreads();
            const int t = threadIdx.x;
            gsum[t] = dot_group_sum(&prod[(t >> 4) * kProdStride], t & 15);
            __syncthreads();
            if (t < 16) {
                const int ph = t >> 2, sub = t & 3, nbx = nx >> 8;
                const int jrow = 2 * by * rows + sub / nbx;
                if (ph < np && jrow >= 1 && jrow <= ny - 2)
                    A.partials[((size_t)(q0 + ph) * ny + jrow) * nbx + (sub & (nbx - 1))] = dot_final_sum(&gsum[t * 16], &prod[t * kProdStride]);
            }
            __syncthreads();
        }
        if (q >= kend) break;
    }
#undef MG_FU_PHASE
    if (MAXV) {
        mred[threadIdx.x] = mx;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) mred[threadIdx.x] = fmax(mred[threadIdx.x], mred[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) A.maxpart[b] = mred[0];
    }
}

// ---- the same three fusions with a WAVE PER ROW (rows of 256 cells) -------------------------------------------------------
// mg_fused_kernel's threads own two rows and load four, so `base` and `d` cross the L1 path twice and every halo row is divided a
// second time.  Here a block is W = 8 rows + one halo row at either
// end, a wave owns ONE row as in mg_lds3_kernel (lane l: cells 2l, 2l+1 and 128 + 2l, 129 + 2l, x neighbours across the seam by
// wave rotation): it makes xnew of its own row only, puts it into LDS for its two neighbours (double-buffered by plane parity,
// one barrier per plane) and keeps the planes q-1, q, q+1 of its row in registers for the z neighbours -- 10 rows loaded per 8
// produced.  A row is exactly one partial of the dot products: its 256 products go through the wave's own LDS strip and 16 + 1
// lanes run the reference's tree, no block barrier involved.
template <int MODE>
__global__ __launch_bounds__(640) void mg_fused_rows_kernel(const FuseArgs A, int nblk)
{
    constexpr bool DIV = MODE != kFuseAddRes, POISSON = MODE == kFuseDirPoi, DOT = MODE != kFuseXRes, MAXV = MODE == kFuseAddRes;
    constexpr int W = 8, NW = W + 2, SA = 0;        // (blocks of 14 rows and non-temporal stores were measured: nothing, EXPERIMENTS section 9)
    __shared__ v2d rows[2][NW][2][64];                              // xnew of the plane in work: [plane parity][wave][segment][lane]
    __shared__ __attribute__((aligned(16))) double prod[DOT ? W * kProdStride : 2];
    __shared__ double gsum[DOT ? W * 16 : 1];
    __shared__ double mred[MAXV ? NW : 1];
    const int nx = A.nx, ny = A.ny, nz = A.nz, nby = A.nby, kchunk = A.kchunk;
    const int per = (int)gridDim.x >> 3;                            // XCD-contiguous block order (grid padded to 8 k blocks)
    const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
    if (b >= nblk) return;
    const int by = b % nby, bz = b / nby;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int kbeg = max(1, bz * kchunk), kend = min(nz - 1, bz * kchunk + kchunk);
    if (kbeg >= kend) {                                             // (block-uniform)
        if (MAXV && threadIdx.x == 0) A.maxpart[b] = 0.0;
        return;
    }
    const int j = by * W + wv - 1;                                  // this wave's row (the outer two: halo rows)
    const bool halo = wv == 0 || wv == NW - 1;
    const bool rowv = !halo && j < ny, rowi = !halo && j >= 1 && j <= ny - 2;
    const bool first = lane == 0, last = lane == 63;                // (= the x rim: cells 0 and 255)
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * 8u;
    const v4i rb = make_rsrc4(A.base, bytes), rdd = make_rsrc4(A.d, bytes), rr = make_rsrc4(POISSON ? A.base : A.rhs, bytes);
    const v4i rx = make_rsrc4(A.xout, bytes), ro = make_rsrc4(A.out, bytes);
    const unsigned row_own = (unsigned)nx * (unsigned)min(max(j, 0), ny - 1);
    const unsigned voA = ((unsigned)(2 * lane) + row_own) * 8u, voB = ((unsigned)(128 + 2 * lane) + row_own) * 8u;
    // the rim cell of the row (lane 0: cell 0, lane 63: cell 255): what `out` holds there enters the sums
    const unsigned vob = (DOT && rowi && (first || last)) ? (first ? voA : voB + 8u) : 0x80000000u;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * 8u;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    auto ld_row = [&](v4i rs, unsigned pp) -> D4 { return D4{ld_d2(rs, voA, pp), ld_d2(rs, voB, pp)}; };
    auto st_row = [&](D4 v, unsigned pp) { st_d2<SA>(v.a, rx, voA, pp); st_d2<SA>(v.b, rx, voB, pp); };
    auto put = [&](int par, D4 v) { rows[par][wv][0][lane] = v2d{v.a.a, v.a.b}; rows[par][wv][1][lane] = v2d{v.b.a, v.b.b}; };
    auto get = [&](int par, int r) -> D4 { const v2d u = rows[par][r][0][lane], w = rows[par][r][1][lane]; return D4{D2{u.x, u.y}, D2{w.x, w.y}}; };
    double num = 0.0, den = 1.0;
    if (DIV) { num = A.coef[A.num_idx]; den = A.coef[A.den_idx]; }
    const double mul = A.mul;
    auto comb = [&](double bs, double dv) -> double { return DIV ? bs + (dv * num) / den : bs + dv * mul; };
    auto comb4 = [&](D4 bs, D4 dv) -> D4 {
        return D4{D2{comb(bs.a.a, dv.a.a), comb(bs.a.b, dv.a.b)}, D2{comb(bs.b.a, dv.b.a), comb(bs.b.b, dv.b.b)}};
    };
    const D4 zero = D4{D2{0.0, 0.0}, D2{0.0, 0.0}};
    const int rlo = max(wv - 1, 0), rhi = min(wv + 1, NW - 1);
    double *pr = &prod[DOT ? max(wv - 1, 0) % W * kProdStride : 0], *gs = &gsum[DOT ? max(wv - 1, 0) % W * 16 : 0];

    D4 X[4], DD, R[2];
    R[0] = zero; R[1] = zero;
    double mx = 0.0;
    int q = kbeg;
    {
        const unsigned pm = po(q - 1), pc = po(q), pn = po(q + 1);
        X[3] = ld_row(rb, pm); X[0] = ld_row(rb, pc); X[1] = ld_row(rb, pn);
        const D4 d0 = ld_row(rdd, pm), d1 = ld_row(rdd, pc);
        DD = ld_row(rdd, pn);
        if (!POISSON) R[0] = ld_row(rr, pc);
        X[3] = comb4(X[3], d0); X[0] = comb4(X[0], d1);
        if (q - 1 == 0 && rowv) st_row(X[3], 0u);                   // the first chunk owns plane 0
        put(q & 1, X[0]);
        __syncthreads();
    }
#define MG_FR_PHASE(T)                                                                                              \
    {                                                                                                               \
        constexpr int im = (T + 3) & 3, ic = T, in_ = (T + 1) & 3, ia = (T + 2) & 3, rc = T & 1, rn = (T + 1) & 1;     \
        const unsigned pa = po(q + 2), pb = po(q + 1), pk = pstride * (unsigned)q;                                  \
        X[in_] = comb4(X[in_], DD);                                 /* plane q+1 arrived */                          \
        X[ia] = ld_row(rb, pa); DD = ld_row(rdd, pa);                                                               \
        if (!POISSON) R[rn] = ld_row(rr, pb);                                                                       \
        double ob = 0.0;                                                                                            \
        if (DOT) ob = ld_d(ro, vob, pk);                                                                            \
        put((q + 1) & 1, X[in_]);                                   /* the next step's centre plane */               \
        if (!halo) {                                                                                                \
            const D4 fr = get(q & 1, rlo), bk = get(q & 1, rhi);                                                    \
            if (rowv) {                                                                                             \
                st_row(X[ic], pk);                                                                                  \
                if (q + 1 == nz - 1) st_row(X[in_], pb);            /* the last chunk owns plane nz-1 */             \
            }                                                                                                       \
            if (rowi) {                                                                                             \
                D4 o = POISSON ? poi_d4(X[ic], fr, bk, X[im], X[in_], first, last)                                  \
                               : res_d4(X[ic], fr, bk, X[im], X[in_], R[rc], first, last);                          \
                if (!first) st_d2<SA>(o.a, ro, voA, pk);                                                             \
                else bq_buffer_store_x2(__builtin_bit_cast(v2f, o.a.b), ro, (int)(voA + 8u), (int)pk, SA);           \
                if (!last) st_d2<SA>(o.b, ro, voB, pk);                                                              \
                else bq_buffer_store_x2(__builtin_bit_cast(v2f, o.b.a), ro, (int)voB, (int)pk, SA);                  \
                if (DOT) {                                                                                          \
                    if (first) o.a.a = ob;                                                                          \
                    if (last) o.b.b = ob;                                                                           \
                    if (MAXV) mx = fmax(mx, fmax(fmax(o.a.a, o.a.b), fmax(o.b.a, o.b.b)));                          \
                    const D4 ce = X[ic];                                                                            \
                    const D4 pv = POISSON ? D4{D2{ce.a.a * o.a.a, ce.a.b * o.a.b}, D2{ce.b.a * o.b.a, ce.b.b * o.b.b}} \
                                          : D4{D2{o.a.a * o.a.a, o.a.b * o.a.b}, D2{o.b.a * o.b.a, o.b.b * o.b.b}};  \
                    *reinterpret_cast<v2d *>(&pr[prod_at(2 * lane)]) = v2d{pv.a.a, pv.a.b};                         \
                    *reinterpret_cast<v2d *>(&pr[prod_at(128 + 2 * lane)]) = v2d{pv.b.a, pv.b.b};                   \
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                                          \
                    __builtin_amdgcn_wave_barrier();                                                                \
                    if (lane < 16) gs[lane] = dot_group_sum(pr, lane);                                              \
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                                          \
                    __builtin_amdgcn_wave_barrier();                                                                \
                    if (lane == 0) A.partials[(size_t)q * ny + j] = dot_final_sum(gs, pr);                          \
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                                          \
                    __builtin_amdgcn_wave_barrier();                                                                \
                }                                                                                                   \
            }                                                                                                       \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        q++;                                                                                                        \
    }
    while (true) {
        MG_FR_PHASE(0)
        if (q >= kend) break;
        MG_FR_PHASE(1)
        if (q >= kend) break;
        MG_FR_PHASE(2)
        if (q >= kend) break;
        MG_FR_PHASE(3)
        if (q >= kend) break;
    }
#undef MG_FR_PHASE
    if (MAXV) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) mx = fmax(mx, __shfl_xor(mx, s, 64));
        if (lane == 0) mred[wv] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = mred[0];
            for (int w = 1; w < NW; w++) m = fmax(m, mred[w]);
            A.maxpart[b] = m;
        }
    }
}

// The partials that consist of rim elements only -- the rows 0 and ny-1 of every plane, the planes 0 and nz-1 -- as
// dot_vector_kernel makes them (mg_dot_kernel's tree), and their share of the max.  Block rb of the grid:
//   [0, nyb)            plane 0          nyb = ny * (nx / 256)
//   [nyb, 2 nyb)        plane nz-1
//   then per plane 1 .. nz-2: row 0, row ny-1 (nx / 256 blocks each)
template <bool MAXV>
__global__ __launch_bounds__(256) void mg_rim_dot_kernel(const double *__restrict__ v0, const double *__restrict__ v1,
                                                         double *__restrict__ partials, double *__restrict__ maxpart,
                                                         int nx, int ny, int nz)
{
    __shared__ double sh[kProdStride];
    __shared__ double gs[16];
    __shared__ double mred[MAXV ? 256 : 1];
    const int nbx = nx >> 8, nyb = ny * nbx;
    int rb = blockIdx.x;
    size_t gi;                                                      // the partial's index = first element / 256
    if (rb < nyb) gi = (size_t)rb;
    else if (rb < 2 * nyb) gi = (size_t)(nz - 1) * nyb + (size_t)(rb - nyb);
    else {
        rb -= 2 * nyb;
        const int k = 1 + rb / (2 * nbx), w = rb % (2 * nbx);
        gi = ((size_t)k * ny + (w < nbx ? 0 : ny - 1)) * nbx + (size_t)(w % nbx);
    }
    const size_t id = gi * 256 + threadIdx.x;
    const double a = v0[id];
    sh[prod_at(threadIdx.x)] = a * v1[id];
    __syncthreads();
    if (threadIdx.x < 16) gs[threadIdx.x] = dot_group_sum(sh, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) partials[gi] = dot_final_sum(gs, sh);
    if (MAXV) {
        mred[threadIdx.x] = fmax(0.0, a);
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) mred[threadIdx.x] = fmax(mred[threadIdx.x], mred[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) maxpart[blockIdx.x] = mred[0];
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
struct FuseGeom { int cw, nby, kc, nbz, nbx; unsigned nblk, nrim, npart; };
// mg_stencil_lean's decomposition: double2 columns, two rows per thread, z-chunks of ~32 planes sized to whole XCD rounds
static FuseGeom fuse_geom(int ni, int nj, int nk)
{
    FuseGeom g;
    g.cw = ni / 2;
    const int rows2 = 256 / g.cw;
    g.nby = (nj + 2 * rows2 - 1) / (2 * rows2);
    const int nchunks = geom::whole_round_chunks(g.nby, nk, 32, 256);
    g.kc = (nk + nchunks - 1) / nchunks;
    if (g.kc < 4) g.kc = 4;
    g.nbz = (nk + g.kc - 1) / g.kc;
    g.nbx = ni >> 8;
    g.nblk = (unsigned)(g.nby * g.nbz);
    g.nrim = (unsigned)(2 * nj * g.nbx + (nk - 2) * 2 * g.nbx);
    g.npart = (unsigned)(((size_t)ni * nj * nk) >> 8);
    return g;
}
// FL_OPT_MGCG_FUSE: 1 = on for the sizes where the marching stencil is used at all, 2 = whenever the shape allows, 0 = off,
// -1 (the library's default) = nobody has vouched for full-size temp1 / levels[0].b arrays yet: off (the host solver, which
// allocates them, sets 1)
static bool mg_fuse_ok(int ni, int nj, int nk, std::initializer_list<const void *> arrays)
{
    const int f = rt().opt_mgcg_fuse;
    if (f <= 0 || !rt().opt_mgcg_tile || (ni != 256 && ni != 512) || nj < 4 || nk < 4) return false;
    if (f < 2 && (long long)ni * nj * nk < (1ll << 20)) return false;
    if ((double)ni * nj * nk * 8.0 >= 2147483648.0) return false;
    for (const void *a : arrays)
        if (!a || !aligned16(a)) return false;
    return true;
}
// FL_OPT_MGCG_FUSE = 3: the wave-per-row kernel on rows of 256 cells (same time as the two-rows-per-thread one inside one process:
// 109.1 against 108.9 ms per step, tools/mgcg_fuse_ab.py -- both sit at what HBM gives a 40-50 % write share; kept for A/B)
static bool fuse_rows(int ni) { return ni == 256 && rt().opt_mgcg_fuse == 3; }
// mg_lds3_kernel's decomposition: blocks of 8 rows, z-chunks so that every CU has one block
static FuseGeom fuse_geom_rows(int ni, int nj, int nk)
{
    FuseGeom g = fuse_geom(ni, nj, nk);
    g.cw = 0;
    g.nby = (nj + 7) / 8;
    g.kc = std::max(4, geom::once_per_cu_len(nk, g.nby, 1, rt().num_cus));
    if (rt().opt_jacobi_kchunk2 > 0) g.kc = std::max(4, rt().opt_jacobi_kchunk2);      // (A/B timing)
    g.nbz = (nk + g.kc - 1) / g.kc;
    g.nblk = (unsigned)(g.nby * g.nbz);
    return g;
}
static FuseGeom fuse_geom_for(int ni, int nj, int nk) { return fuse_rows(ni) ? fuse_geom_rows(ni, nj, nk) : fuse_geom(ni, nj, nk); }
template <int MODE>
static void mg_fused(FuseArgs A, int ni, int nj, int nk)
{
    if (fuse_rows(ni)) {
        const FuseGeom g = fuse_geom_rows(ni, nj, nk);
        A.nx = ni; A.ny = nj; A.nz = nk; A.cw = 0; A.nby = g.nby; A.kchunk = g.kc;
        hipStream_t st = rt().compute;
        mg_fused_rows_kernel<MODE><<<8 * ((g.nblk + 7) / 8), 640, 0, st>>>(A, (int)g.nblk);
        rt().mg_fused_launches++;
        if (MODE == kFuseAddRes) mg_rim_dot_kernel<true><<<g.nrim, 256, 0, st>>>(A.out, A.out, A.partials, A.maxpart + g.nblk, ni, nj, nk);
        if (MODE == kFuseDirPoi) mg_rim_dot_kernel<false><<<g.nrim, 256, 0, st>>>(A.xout, A.out, A.partials, nullptr, ni, nj, nk);
        BQ_LAUNCH_CHECK("mg_fused_rows_kernel");
        return;
    }
    const FuseGeom g = fuse_geom(ni, nj, nk);
    A.nx = ni; A.ny = nj; A.nz = nk; A.cw = g.cw; A.nby = g.nby; A.kchunk = g.kc;
    hipStream_t st = rt().compute;
    mg_fused_kernel<MODE><<<g.nblk, 256, 0, st>>>(A);
    rt().mg_fused_launches++;
    if (MODE == kFuseAddRes) mg_rim_dot_kernel<true><<<g.nrim, 256, 0, st>>>(A.out, A.out, A.partials, A.maxpart + g.nblk, ni, nj, nk);
    if (MODE == kFuseDirPoi) mg_rim_dot_kernel<false><<<g.nrim, 256, 0, st>>>(A.xout, A.out, A.partials, nullptr, ni, nj, nk);
    BQ_LAUNCH_CHECK("mg_fused_kernel");
}
