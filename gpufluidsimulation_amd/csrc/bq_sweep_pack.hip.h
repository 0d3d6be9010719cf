// bq_sweep_pack.hip.h -- what the marching sweep kernels of the fp32 Jacobi projection (bq_project.hip) and of the fp64
// multigrid smoother (bq_mgcg.hip) share: the packs' loads, stores and stencil expressions, ring_slot, and the lean two-sweep
// kernel, stated once over a cell-pack trait:
//   PackF4   float,  four cells per lane (R4: one float4 column as two v2f halves)
//   PackD2   double, two cells per lane  (D2: one double2 column)
// A pack carries its element type, its 16-byte buffer loads / stores and its stencil expression.  The expressions stay one
// function per type (jac_r4, jac_d2): they are the numerics contract and cite different reference lines.  What else differs
// between the two callers is the plane range of a block, which travels as the kernel's last argument (SlabPairs in
// bq_project.hip, WholeArray here).
#pragma once
#include "bq_device.hip.h"
#include "bq_buffer.hip.h"
#include <climits>
#include <type_traits>

namespace bq {

// slot of the plane at distance d from the centre plane of unrolled step T, in a ring of P planes (d >= -P)
constexpr int ring_slot(int T, int d, int P) { return ((T + d) % P + P) % P; }

// ---- fp32, four cells per lane --------------------------------------------------------------------------------------------
struct R4 { v2f a, b; };                                    // (x, y), (z, w) of one float4 column

__device__ __forceinline__ R4 ld_r4(v4i rs, unsigned voff, unsigned soff)
{
    const v4f v = bq_buffer_load_x4(rs, (int)voff, (int)soff, 0);
    return R4{v2f{v.x, v.y}, v2f{v.z, v.w}};
}
__device__ __forceinline__ float ld_f(v4i rs, unsigned voff, unsigned soff) { return bq_buffer_load_x1(rs, (int)voff, (int)soff, 0); }
// AUX: cache policy bits of the store (2 = nt: a streaming store, for arrays that will not be read again from the caches)
template <int AUX = 0>
__device__ __forceinline__ void st_r4(R4 v, v4i rs, unsigned voff, unsigned soff)
{
    bq_buffer_store_x4(v4f{v.a.x, v.a.y, v.b.x, v.b.y}, rs, (int)voff, (int)soff, AUX);
}

// own + (value of `from` in lane - 1) / (lane + 1), the neighbour taken through the add's own DPP operand: one instruction
// where a DPP move, a move to pair the operands and a packed add stood.  A lane without a source lane (0 / 63) reads 0
// (bound_ctrl): those are x-boundary or out-of-range columns, whose result is replaced or never stored.  The s_nop covers the
// two wait states a DPP read needs after a VALU write of its source, which the compiler cannot see inside the asm.
// `volatile`: the result depends on EXEC and on the neighbouring lanes, which the compiler cannot see either --
// a pure two-operand asm could be sunk into a divergent region or merged across EXEC changes; volatile statements stay where
// the source puts them (every use is in wave-uniform code of the plane loop).  Same ISA at today's -O3, same timings.
__device__ __forceinline__ float add_from_left_lane(float from, float own)
{
    float r;
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0" : "=v"(r) : "v"(from), "v"(own));
    return r;
}
__device__ __forceinline__ float add_from_right_lane(float from, float own)
{
    float r;
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0" : "=v"(r) : "v"(from), "v"(own));
    return r;
}

// jacobi_kernel's expression (GPU_kernel.cu:1833) on a float4 column: ((((((l + r) + f) + b) + d) + u) + alpha div) beta
// WIDE (rows of several waves): the x-neighbour of a wave's first / last lane lives in another wave; `outside` is its
// value, supplied by that lane itself (edgeL / edgeR mark the two lanes)
// PRE: dv already holds alpha * div (the product is formed once per loaded div value and reused by every level that needs
// it -- the same float either way)
// DPPADD (rows of one wave only): the l + r stage as four scalar adds, the two outer ones with a DPP operand
template <bool WIDE = false, bool PRE = false, bool DPPADD = false>
__device__ __forceinline__ R4 jac_r4(R4 ce, R4 fr, R4 bk, R4 dn, R4 up, R4 dv, float alpha, float beta, bool xlo, bool xhi,
                                     float outside = 0.f, bool edgeL = false, bool edgeR = false)
{
    // (l + r) per cell: cell 0 = left + x1, 1 = x0 + x2, 2 = x1 + x3, 3 = x2 + right
    v2f s0, s1;
    if (DPPADD && !WIDE) {
        s0 = v2f{add_from_left_lane(ce.b.y, ce.a.y), ce.a.x + ce.b.x};
        s1 = v2f{ce.a.y + ce.b.y, add_from_right_lane(ce.a.x, ce.b.x)};
    } else {
        float left = lane_up(ce.b.y), right = lane_down(ce.a.x);
        if (WIDE) {
            if (edgeL) left = outside;
            if (edgeR) right = outside;
        }
        // (the compiler forms two v_pk_add_f32 here and assembles their operand pairs {left, x0}, {x1, x2}, {x3, right} with
        // six moves; four scalar adds with the neighbour lanes taken through the adds' own DPP operand (inline asm) are 4
        // instructions instead of 10, but measured no faster: 13.25 vs 13.23 us per sweep in the three-sweep kernel)
        s0 = v2f{left + ce.a.y, ce.a.x + ce.b.x};
        s1 = v2f{ce.a.y + ce.b.y, ce.b.x + right};
    }
    s0 = s0 + fr.a; s1 = s1 + fr.b;
    s0 = s0 + bk.a; s1 = s1 + bk.b;
    s0 = s0 + dn.a; s1 = s1 + dn.b;
    s0 = s0 + up.a; s1 = s1 + up.b;
    if (PRE) { s0 = s0 + dv.a; s1 = s1 + dv.b; }
    else     { s0 = s0 + alpha * dv.a; s1 = s1 + alpha * dv.b; }
    s0 = s0 * beta; s1 = s1 * beta;
    if (xlo) s0.x = ce.a.x;
    if (xhi) s1.y = ce.b.y;
    return R4{s0, s1};
}

struct PackF4 {
    using elem = float;
    using cells = R4;
    static constexpr int N = 4;                             // cells per lane; rows are whole packs
    static constexpr bool ODD_ROWS = false;
    static constexpr bool PRE_ALPHA = true;                 // alpha * div is formed once per loaded value (jac_r4's PRE)
    static constexpr bool HAS_ZIN = false;
    static __device__ __forceinline__ R4 ld(v4i rs, unsigned voff, unsigned soff) { return ld_r4(rs, voff, soff); }
    static __device__ __forceinline__ float ld1(v4i rs, unsigned voff, unsigned soff) { return ld_f(rs, voff, soff); }
    template <int AUX>
    static __device__ __forceinline__ void st(R4 v, v4i rs, unsigned voff, unsigned soff) { st_r4<AUX>(v, rs, voff, soff); }
    static __device__ __forceinline__ float first(R4 v) { return v.a.x; }
    static __device__ __forceinline__ float last(R4 v) { return v.b.y; }
    static __device__ __forceinline__ R4 scaled(float alpha, R4 v) { return R4{alpha * v.a, alpha * v.b}; }
    template <bool WIDE>
    static __device__ __forceinline__ R4 jac(R4 ce, R4 fr, R4 bk, R4 dn, R4 up, R4 dv, float alpha, float beta, bool xlo, bool xhi,
                                             float outside, bool edgeL, bool edgeR)
    {
        return jac_r4<WIDE, true>(ce, fr, bk, dn, up, dv, alpha, beta, xlo, xhi, outside, edgeL, edgeR);
    }
};

// ---- fp64, two cells per lane ---------------------------------------------------------------------------------------------
struct D2 { double a, b; };                                 // two consecutive cells of a row
__device__ __forceinline__ D2 ld_d2(v4i rs, unsigned voff, unsigned soff)
{
    const v2d v = __builtin_bit_cast(v2d, bq_buffer_load_x4(rs, (int)voff, (int)soff, 0));
    return D2{v.x, v.y};
}
__device__ __forceinline__ double ld_d(v4i rs, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(double, bq_buffer_load_x2(rs, (int)voff, (int)soff, 0));
}
template <int AUX = 0>
__device__ __forceinline__ void st_d2(D2 v, v4i rs, unsigned voff, unsigned soff)
{
    bq_buffer_store_x4(__builtin_bit_cast(v4f, v2d{v.a, v.b}), rs, (int)voff, (int)soff, AUX);
}
// smoothing_jacobi_kernel's expression (:1443-1461) on a double2 column; WIDE: `outside` replaces the neighbour lane's
// value at a wave's first / last lane
template <bool WIDE>
__device__ __forceinline__ D2 jac_d2(D2 ce, D2 fr, D2 bk, D2 dn, D2 up, D2 dv, double alpha, double beta, bool xlo, bool xhi,
                                     double outside, bool edgeL, bool edgeR)
{
    double left = lane_up(ce.b), right = lane_down(ce.a);
    if (WIDE) {
        if (edgeL) left = outside;
        if (edgeR) right = outside;
    }
    D2 o;
    o.a = ((left + ce.b + fr.a + bk.a + dn.a + up.a) + alpha * dv.a) * beta;
    o.b = ((ce.a + right + fr.b + bk.b + dn.b + up.b) + alpha * dv.b) * beta;
    if (xlo) o.a = ce.a;
    if (xhi) o.b = ce.b;
    return o;
}

struct PackD2 {
    using elem = double;
    using cells = D2;
    static constexpr int N = 2;
    // odd rows: the last lane of a row holds the single boundary column nx-1 in .a (its .b is the next row's first cell:
    // loaded, never used, never stored -- the lane stores nothing, `out` already holds the boundary column)
    static constexpr bool ODD_ROWS = true;
    static constexpr bool PRE_ALPHA = false;                // jac_d2 multiplies at each use: the same product
    static constexpr bool HAS_ZIN = true;
    static __device__ __forceinline__ D2 ld(v4i rs, unsigned voff, unsigned soff) { return ld_d2(rs, voff, soff); }
    static __device__ __forceinline__ double ld1(v4i rs, unsigned voff, unsigned soff) { return ld_d(rs, voff, soff); }
    template <int AUX>
    static __device__ __forceinline__ void st(D2 v, v4i rs, unsigned voff, unsigned soff) { st_d2<AUX>(v, rs, voff, soff); }
    static __device__ __forceinline__ double first(D2 v) { return v.a; }
    static __device__ __forceinline__ double last(D2 v) { return v.b; }
    template <bool WIDE>
    static __device__ __forceinline__ D2 jac(D2 ce, D2 fr, D2 bk, D2 dn, D2 up, D2 dv, double alpha, double beta, bool xlo, bool xhi,
                                             double outside, bool edgeL, bool edgeR)
    {
        return jac_d2<WIDE>(ce, fr, bk, dn, up, dv, alpha, beta, xlo, xhi, outside, edgeL, edgeR);
    }
};

// The planes of a block when a launch covers the whole array: chunk bz marches [bz * kchunk, (bz + 1) * kchunk) of the interior
// planes 1 .. nz-2.  (An empty kernel argument; the z-slab form with two plane ranges is SlabPairs, bq_project.hip.)
struct WholeArray {
    __device__ __forceinline__ constexpr int kA() const { return 1; }    // (a constant expression in the kernels)
    __device__ __forceinline__ int kB(int nz) const { return nz - 1; }
    __device__ __forceinline__ int r0(int bz, int kchunk) const { return bz * kchunk; }
    __device__ __forceinline__ int r1(int) const { return INT_MAX; }
};

// ---- TWO sweeps per launch, two rows per thread: sweep_lean2r_kernel ------------------------------------------------------
// (host-visible as jacobi_lean2r_kernel in fp32 and mg_lean2r_kernel in fp64)
// The plain two-row march is bound by instruction ISSUE, not by memory: one wave per SIMD issues one VALU instruction per ~4
// cycles, and the compiler's rendering of jacobi_march2r_kernel spends ~680 instructions per plane (64-bit address arithmetic
// for every load, ~120 register moves to rotate planes and to pair operands, selects for boundaries that a wave almost never
// has); mg_smooth2_kernel likewise rotates by moves and owns one row per thread (130 us per launch at 256^3 = 402 MB of
// compulsory traffic at 3.1 TB/s).  Same algorithm, same expression per value, different plumbing:
//   * loads and stores through buffer descriptors: per-thread row offsets computed once (VGPR), the plane offset in an
//     SGPR -- no address arithmetic in the loop;
//   * every plane set lives in a ring of 3 + PF buffers indexed by (plane mod ring); the loop is unrolled as many times so
//     that all ring indices are compile-time: nothing is ever moved to rotate planes;
//   * a thread owns the 16-byte columns of rows j, j+1 and keeps L0 on rows j-1 .. j+2 (+ j-2, j+3 of the centre plane);
//     fp32 columns are two float2 halves (clang ext vectors -> v_pk_add_f32 / v_pk_mul_f32);
//   * boundary rows are a property of the BLOCK (template flag EDGE: only the first and last row blocks pay the
//     selects), boundary planes one wave-uniform branch;
//   * x-boundary columns are stored too: they hold L0's value (a sweep never changes them), which is what `out`
//     already holds there (the fused kernels' precondition: both buffers carry the same boundary layer).
// WIDE: rows of 2-4 waves (fp32 beyond 256 cells, fp64 beyond 128); otherwise rows of one wave.  Every value is the pack's
// own expression (jacobi_kernel's / smoothing_jacobi_kernel's) on the same operands as a single sweep.
// PF: how many planes ahead the loads run (1 or 2; 3 and 4 measured no better anywhere).
// ZIN (fp64 only): the input field is all zeros and is not read (V_Cycle's first sweep of a level starts from a cleared x).
template <class PK, bool WIDE, int PF, bool ZIN, class RANGE>
__global__ __launch_bounds__(256) void sweep_lean2r_kernel(const typename PK::elem *__restrict__ p, const typename PK::elem *__restrict__ div,
                                                           typename PK::elem *__restrict__ out, int nx, int ny, int nz,
                                                           int cw, int nby, int kchunk, typename PK::elem alpha, typename PK::elem beta,
                                                           RANGE range)
{
    static_assert(PK::HAS_ZIN || !ZIN, "only the fp64 smoother starts from a cleared field");
    using elem = typename PK::elem;
    using cells = typename PK::cells;
    constexpr int N = PK::N;
    constexpr unsigned ES = sizeof(elem);
    constexpr int P = 3 + PF;                                       // ring period
    // PF = 2 is the form for arrays that come from HBM (larger than the Infinity Cache): loads two planes ahead and
    // streaming stores (fp32 512^3: 174.6 -> 162.8 us per sweep; in-cache sizes lose with them: 256^3 15.9 -> 20.3).
    constexpr bool HBM = PF >= 2;
    constexpr int ST = HBM ? 2 : 0;
    const int nblk = gridDim.x;
    int b = blockIdx.x;
    if ((nblk & 7) == 0) b = (b & 7) * (nblk >> 3) + (b >> 3);      // XCD-contiguous block order
    const int by = b % nby, bz = b / nby;
    const int rows = 256 / cw;
    // a wave holds one row pair when rows are at least one wave long: the row index is then wave-uniform
    const int c = threadIdx.x % cw;
    const int r = cw >= 64 ? __builtin_amdgcn_readfirstlane((int)threadIdx.x / cw) : (int)threadIdx.x / cw;
    const int xraw = N * c, j = 2 * (by * rows + r);
    const int kA = range.kA(), kB = range.kB(nz);
    const int r0 = range.r0(bz, kchunk), r1 = range.r1(bz);
    const int kbeg = max(kA, r0), kend = min(min(kB, r1), r0 + kchunk);
    if (kbeg >= kend) return;
    const bool xok = xraw < nx;
    const bool xlast = PK::ODD_ROWS && xok && xraw == nx - 1;       // (see PackD2)
    const bool active0 = xok && !xlast && j >= 1 && j <= ny - 2, active1 = xok && !xlast && j + 1 >= 1 && j + 1 <= ny - 2;
    // out-of-range lanes, rows, planes: clamped into the array (odd rows: nx - N is no column start)
    const int x = xok ? xraw : (PK::ODD_ROWS ? 0 : nx - N);
    const bool xlo = x == 0 || xlast, xhi = x + N - 1 == nx - 1;
    const unsigned bytes = (unsigned)nx * (unsigned)ny * (unsigned)nz * ES;
    const v4i rp = make_rsrc4(p, bytes), rd = make_rsrc4(div, bytes), ro = make_rsrc4(out, bytes);
    unsigned vo[6];                                                 // byte offsets of this thread's column in rows j-2 .. j+3
    bool rowb[4];                                                   // rows j-1 .. j+2 are boundary rows (keep L0)
#pragma unroll
    for (int a = 0; a < 6; a++) vo[a] = ((unsigned)x + (unsigned)nx * (unsigned)min(max(j - 2 + a, 0), ny - 1)) * ES;
#pragma unroll
    for (int a = 0; a < 4; a++) rowb[a] = j - 1 + a <= 0 || j - 1 + a >= ny - 1;
    // only the first and the last row block can hold a boundary row: everybody else runs the loop without the selects
    const bool edge_block = 2 * by * rows - 1 <= 0 || 2 * (by * rows + rows - 1) + 2 >= ny - 1;
    const unsigned pstride = (unsigned)nx * (unsigned)ny * ES;
    auto po = [&](int pl) -> unsigned { return pstride * (unsigned)min(max(pl, 0), nz - 1); };
    // WIDE: the first / last lane of a wave looks after the column just outside its wave (xe) -- it needs that column's
    // L0 on rows j-1 .. j+2 (x-neighbour of our own first sweep) and its L1 on rows j, j+1 (x-neighbour of our second
    // sweep), which it evaluates itself from that column's own neighbours (outer x-neighbour xo, rows, planes, div).
    // The other 62 lanes run the same eight scalar loads per plane, but with an offset beyond the descriptor's range: the
    // range check answers 0 and nothing goes to the caches (fp32 512^3: 200 -> 175 us per sweep against loading their own
    // column; an exec-masked branch around the loads does the same at 512^3 but costs 7 % in-cache).
    const int lane = threadIdx.x & 63;
    const bool edgeL = WIDE && lane == 0 && xok && xraw > 0, edgeR = WIDE && lane == 63 && xraw + N < nx;
    const bool edge = edgeL || edgeR;
    const int xe = edgeL ? xraw - 1 : (edgeR ? xraw + N : x), xo = edgeL ? xe - 1 : (edgeR ? xe + 1 : x);
    const bool xe_boundary = xe <= 0 || xe >= nx - 1;
    unsigned ve[4], vx[2];
#pragma unroll
    for (int a = 0; a < 4; a++) ve[a] = ((unsigned)min(max(xe, 0), nx - 1) + (unsigned)nx * (unsigned)min(max(j - 1 + a, 0), ny - 1)) * ES;
#pragma unroll
    for (int a = 0; a < 2; a++) vx[a] = ((unsigned)min(max(xo, 0), nx - 1) + (unsigned)nx * (unsigned)min(max(j + a, 0), ny - 1)) * ES;
    if (WIDE && !edge) {
        // an offset beyond the descriptor's range: the load returns 0 without touching the caches (2 GiB + any plane
        // offset of an array below 2 GiB neither wraps nor lands inside it)
#pragma unroll
        for (int a = 0; a < 4; a++) ve[a] = 0x80000000u;
        vx[0] = vx[1] = 0x80000000u;
    }

    // Rings indexed by the plane's slot (t + d) mod P, t = q - (kbeg - 1) the iteration number, d the plane's distance
    // from q -- all compile-time inside the unrolled loop, so no value is ever moved to rotate planes:
    //   L0[.][0..3]  p on rows j-1 .. j+2            (live: planes q-1 .. q+PF; q+1+PF arriving)
    //   H[.][0..1]   p on rows j-2, j+3              (live: plane q .. q+PF-1; q+PF arriving)
    //   L1[.][0..3]  first sweep on rows j-1 .. j+2  (q being made; q-1; q-2 (rows j, j+1))
    //   D[.][0..3]   div on rows j-1 .. j+2          (q-1 (rows j, j+1) .. q+PF-1; q+PF arriving)
    //   WIDE: E[.][0..3] p(xe) on rows j-1 .. j+2 like L0; Eo / Eb p(xo) / div(xe) on rows j, j+1 like H; X the outside
    //   column's L1 on rows j, j+1 (q being made, q-1 live)
    auto run = [&](auto EDGE_T) {
    constexpr bool EDGE = decltype(EDGE_T)::value;
    cells L0[P][4], H[P][2], L1[P][4], D[P][4];
    elem E[P][4], Eo[P][2], Eb[P][2], X[P][2];
    const cells zero{};
#pragma unroll
    for (int a = 0; a < P; a++) {
#pragma unroll
        for (int bb = 0; bb < 4; bb++) L1[a][bb] = zero;
        X[a][0] = 0; X[a][1] = 0;
    }
    int q = kbeg - 1;
#pragma unroll
    for (int d = -1; d <= PF; d++) {                                // prologue: planes q-1 .. q+PF
        const int sl_ = (d + P) % P;
        const unsigned pp = po(q + d);
#pragma unroll
        for (int a = 0; a < 4; a++) L0[sl_][a] = ZIN ? zero : PK::ld(rp, vo[a + 1], pp);
        if (WIDE) {
#pragma unroll
            for (int a = 0; a < 4; a++) E[sl_][a] = ZIN ? elem(0) : PK::ld1(rp, ve[a], pp);
        }
        if (d >= 0 && d < PF) {
#pragma unroll
            for (int a = 0; a < 4; a++) D[sl_][a] = PK::ld(rd, vo[a + 1], pp);
            H[sl_][0] = ZIN ? zero : PK::ld(rp, vo[0], pp); H[sl_][1] = ZIN ? zero : PK::ld(rp, vo[5], pp);
            if (WIDE) {
#pragma unroll
                for (int a = 0; a < 2; a++) { Eo[sl_][a] = ZIN ? elem(0) : PK::ld1(rp, vx[a], pp); Eb[sl_][a] = PK::ld1(rd, ve[a + 1], pp); }
            }
        }
    }
#define BQ_LEAN_PHASE(T)                                                                                            \
    {                                                                                                               \
        constexpr int im = ring_slot(T, -1, P), ic = ring_slot(T, 0, P), in_ = ring_slot(T, 1, P);                  \
        constexpr int ia = ring_slot(T, 1 + PF, P), ha = ring_slot(T, PF, P);                                       \
        constexpr int mp = ring_slot(T, -1, P), mpp = ring_slot(T, -2, P);                                          \
        const unsigned pa = po(q + 1 + PF), pb = po(q + PF);                                                        \
        _Pragma("unroll") for (int a = 0; a < 4; a++) { L0[ia][a] = ZIN ? zero : PK::ld(rp, vo[a + 1], pa); D[ha][a] = PK::ld(rd, vo[a + 1], pb); } \
        H[ha][0] = ZIN ? zero : PK::ld(rp, vo[0], pb); H[ha][1] = ZIN ? zero : PK::ld(rp, vo[5], pb);               \
        if (WIDE) {                                                                                                 \
            _Pragma("unroll") for (int a = 0; a < 4; a++) E[ia][a] = ZIN ? elem(0) : PK::ld1(rp, ve[a], pa);          \
            _Pragma("unroll") for (int a = 0; a < 2; a++) { Eo[ha][a] = ZIN ? elem(0) : PK::ld1(rp, vx[a], pb); Eb[ha][a] = PK::ld1(rd, ve[a + 1], pb); } \
        }                                                                                                           \
        const bool qb = q < kA || q >= kB;                                                                          \
        if (qb) {                                               /* a boundary plane keeps L0 */                      \
            _Pragma("unroll") for (int a = 0; a < 4; a++) L1[ic][a] = L0[ic][a];                                      \
        } else {                                                                                                    \
            /* PRE_ALPHA: alpha * div once per value: rows j, j+1 reuse the product in the second sweep */           \
            if constexpr (PK::PRE_ALPHA) { _Pragma("unroll") for (int a = 0; a < 4; a++) D[ic][a] = PK::scaled(alpha, D[ic][a]); } \
            L1[ic][0] = PK::template jac<WIDE>(L0[ic][0], H[ic][0], L0[ic][1], L0[im][0], L0[in_][0], D[ic][0], alpha, beta, xlo, xhi, E[ic][0], edgeL, edgeR);   \
            L1[ic][1] = PK::template jac<WIDE>(L0[ic][1], L0[ic][0], L0[ic][2], L0[im][1], L0[in_][1], D[ic][1], alpha, beta, xlo, xhi, E[ic][1], edgeL, edgeR);  \
            L1[ic][2] = PK::template jac<WIDE>(L0[ic][2], L0[ic][1], L0[ic][3], L0[im][2], L0[in_][2], D[ic][2], alpha, beta, xlo, xhi, E[ic][2], edgeL, edgeR);  \
            L1[ic][3] = PK::template jac<WIDE>(L0[ic][3], L0[ic][2], H[ic][1], L0[im][3], L0[in_][3], D[ic][3], alpha, beta, xlo, xhi, E[ic][3], edgeL, edgeR);   \
            if (EDGE) {                                                                                             \
                _Pragma("unroll") for (int a = 0; a < 4; a++)                                                        \
                    if (rowb[a]) L1[ic][a] = L0[ic][a];                                                             \
            }                                                                                                       \
        }                                                                                                           \
        if (WIDE) {                                             /* the outside column's own first sweep, rows j, j+1 */ \
            _Pragma("unroll") for (int rr = 0; rr < 2; rr++) {                                                       \
                const elem own = edgeL ? PK::first(L0[ic][rr + 1]) : PK::last(L0[ic][rr + 1]);                      \
                const elem l = edgeL ? Eo[ic][rr] : own, rg2 = edgeL ? own : Eo[ic][rr];                            \
                const elem v = (l + rg2 + E[ic][rr] + E[ic][rr + 2] + E[im][rr + 1] + E[in_][rr + 1] + alpha * Eb[ic][rr]) * beta; \
                const bool keep = qb || xe_boundary || (j + rr <= 0 || j + rr >= ny - 1);                           \
                X[ic][rr] = keep ? E[ic][rr + 1] : v;                                                               \
            }                                                                                                       \
        }                                                                                                           \
        const int k = q - 1;                                                                                        \
        if (k >= kbeg && k < kend) {                                                                                \
            const cells o0 = PK::template jac<WIDE>(L1[mp][1], L1[mp][0], L1[mp][2], L1[mpp][1], L1[ic][1], D[mp][1], alpha, beta, xlo, xhi, X[mp][0], edgeL, edgeR); \
            const cells o1 = PK::template jac<WIDE>(L1[mp][2], L1[mp][1], L1[mp][3], L1[mpp][2], L1[ic][2], D[mp][2], alpha, beta, xlo, xhi, X[mp][1], edgeL, edgeR); \
            const unsigned pk = pstride * (unsigned)k;                                                              \
            if (active0) PK::template st<ST>(o0, ro, vo[2], pk);                                                    \
            if (active1) PK::template st<ST>(o1, ro, vo[3], pk);                                                    \
        }                                                                                                           \
        q++;                                                                                                        \
    }
    while (true) {
        BQ_LEAN_PHASE(0)
        if (q > kend) break;
        BQ_LEAN_PHASE(1)
        if (q > kend) break;
        BQ_LEAN_PHASE(2)
        if (q > kend) break;
        BQ_LEAN_PHASE(3)
        if (q > kend) break;
        if constexpr (P > 4) {
            BQ_LEAN_PHASE(4)
            if (q > kend) break;
        }
        if constexpr (P > 5) {
            BQ_LEAN_PHASE(5)
            if (q > kend) break;
        }
        if constexpr (P > 6) {
            BQ_LEAN_PHASE(6)
            if (q > kend) break;
        }
    }
    };
    if (edge_block) run(std::true_type{}); else run(std::false_type{});
#undef BQ_LEAN_PHASE
}

} // namespace bq
