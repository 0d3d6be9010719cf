// bq_sparse.hip.h -- FL_OPT_SKIP_EMPTY_BRICKS: the nine-point scalar operators leave out the map look-up and the gathers of
// a block whose taps can only land where the sampled fields hold +0.0f.
//
// Three pieces: brick_flags_kernel marks the 8 x 8 x 8 bricks of the source arrays that hold anything but the word 0;
// tile_range reads the map tile the full kernel would stage, for the value range of the nodes the block's active threads read;
// taps_in_empty_bricks turns that range into a range of cells and tests the bricks it covers.
//
// An operator with the skip is TWO launches of its kernel over the same grid (template parameter SPARSE): 1 classifies --
// it reads the map tile for its range only, runs the stores of the blocks it can skip and appends every other block to a
// list; 2 is the plain kernel on the listed blocks.  Keeping the two apart keeps the heavy path at the registers and the
// occupancy it has without the skip, and lets the light one run at full occupancy (it is bound by the latency of its loads).
//
// The accumulation takes another form (FL_OPT_SKIP_EMPTY_TAPS, at the end of this file): a launch that tests the taps it
// has computed against cell flags, wave by wave (and the SPARSE == 2 launch on an empty list behind it, for the dense case).
// Its map is a backward map whose zeroed border defeats the tile range.
#pragma once
#include "bq_device.hip.h"

namespace bq {
inline namespace BQ_VARIANT {

constexpr int kBrick = 8, kBrickShift = 3;

// What a launch with the skip gets (flags == nullptr: the launch without it).  word[0] == epoch: the flag pass in front of
// this launch found an empty brick -- the launcher counts the passes, so the word never has to be cleared.
// stats (FL_OPT_SKIP_EMPTY_BRICKS = 2 or 4, else null): [0] blocks tested and kept, [1] blocks tested and skipped (the launching
// operator's pair).
struct Sparse {
    const unsigned char *flags;         // nbx * nby * nbz, x fastest: 1 = the brick holds a non-zero word in some field
    const int *word;
    unsigned long long *stats;
    int *list;                          // [0]: how many blocks the classifying launch kept, [1 ...]: their linear block indices
    int epoch, nbx, nby;
};
template <int NF> struct BrickSrc { const float *p[NF]; };

// One block per 64 x 8 x 8 nodes (eight bricks along x); wave w reads rows w, w + 4, ... of the 64, a lane one word per
// row and field -- a wave's load is 256 consecutive bytes.  A brick is empty only if every word of every field in it is
// 0x00000000: -0.0f, denormals, NaN and Inf are occupied.  Bricks at the array's ends are partial; what lies outside
// the array counts as zero.
template <int NF>
__global__ __launch_bounds__(256) void brick_flags_kernel(BrickSrc<NF> s, int nx, int ny, int nz,
                                                          unsigned char *flags, int *word, int epoch, int *list)
{
    __shared__ unsigned part[4][8];
    const int lane = threadIdx.x, wv = threadIdx.y;
    const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * kBrick, z0 = blockIdx.z * kBrick;
    unsigned acc = 0u;
    if (list && (blockIdx.x | blockIdx.y | blockIdx.z | lane | wv) == 0) list[0] = 0;      // the block list of the launch that follows starts empty
    if (x < nx) {
#pragma unroll 4
        for (int r = wv; r < kBrick * kBrick; r += 4) {
            const int y = y0 + (r & 7), z = z0 + (r >> 3);
            if (y < ny && z < nz) {
                const size_t id = (size_t)x + (size_t)nx * y + (size_t)nx * ny * z;
#pragma unroll
                for (int f = 0; f < NF; f++) acc |= __builtin_bit_cast(unsigned, s.p[f][id]);
            }
        }
    }
    // OR over the 8 lanes of a brick, then over the four waves
    acc |= (unsigned)__shfl_xor((int)acc, 1, 64);
    acc |= (unsigned)__shfl_xor((int)acc, 2, 64);
    acc |= (unsigned)__shfl_xor((int)acc, 4, 64);
    if ((lane & 7) == 0) part[wv][lane >> 3] = acc;
    __syncthreads();
    if (wv == 0 && lane < 8) {
        const int bx = blockIdx.x * 8 + lane, nbx = (nx + kBrick - 1) >> kBrickShift, nby = (ny + kBrick - 1) >> kBrickShift;
        if (bx < nbx) {
            const bool occupied = (part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane]) != 0u;
            flags[(size_t)bx + (size_t)nbx * (blockIdx.y + (size_t)nby * blockIdx.z)] = occupied ? 1 : 0;
            // at most one atomic per block, and none once the word carries this pass's number
            if (!occupied && __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) atomicMax(word, epoch);
        }
    }
}

// The value range of each map component over the nodes x in [xlo, xhi], y in [ylo, yhi] of the tile stage_tiles would load for
// block (i0, j0) on plane kl -- the operator's index window widened by one: the nodes its active threads read; the tile's other
// nodes (the wrapped columns beside a row's ends, the map border outside that range) reach no tap.  Every element is loaded by
// the flat index stage_tiles uses.  bad: a NaN or an Inf among those nodes (0 * v is NaN for both).
// part: 32 floats of LDS.  All 256 threads call this; one barrier.
__device__ __forceinline__ void tile_range(const Field (&f)[3], int i0, int j0, int kl, float *part,
                                           int xlo, int xhi, int ylo, int yhi, float (&mn)[3], float (&mx)[3], bool &bad)
{
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int nx = f[0].nx, sk = f[0].nx * f[0].ny;
    const float inf = __builtin_huge_valf();
    float poison = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) { mn[c] = inf; mx[c] = -inf; }
    // (unrolled with every load in front of the first use: the range makes each value a dependence, and a rolled loop
    // would wait for memory once per row instead of once)
    constexpr int kRounds = (kTileY * kTileZ + 3) / 4;
    float v[kRounds][3];
#pragma unroll
    for (int t = 0; t < kRounds; t++) {
        const int r = min(wv + 4 * t, kTileY * kTileZ - 1);         // (the last round of waves 2, 3 repeats row 17: harmless)
        const int z = r / kTileY, y = r - z * kTileY;
        const unsigned off = (unsigned)((i0 + lane) + nx * (j0 - 1 + y) + sk * (kl - 1 + z)) * 4u;
#pragma unroll
        for (int c = 0; c < 3; c++) v[t][c] = ldf(f[c], off);
    }
#pragma unroll
    for (int t = 0; t < kRounds; t++) {
        const int r = min(wv + 4 * t, kTileY * kTileZ - 1);
        const int y = r % kTileY;
        if (xlo <= i0 + lane && i0 + lane <= xhi && ylo <= j0 - 1 + y && j0 - 1 + y <= yhi) {
#pragma unroll
            for (int c = 0; c < 3; c++) { mn[c] = fminf(mn[c], v[t][c]); mx[c] = fmaxf(mx[c], v[t][c]); poison = __builtin_fmaf(0.f, v[t][c], poison); }
        }
    }
    if (wv == 0 && lane < 2 * kTileY * kTileZ) {            // the two edge columns
        const int r = lane >> 1, X = (lane & 1) ? kTileX - 1 : 0;
        const int z = r / kTileY, y = r - z * kTileY;
        const unsigned off = (unsigned)((i0 - 1 + X) + nx * (j0 - 1 + y) + sk * (kl - 1 + z)) * 4u;
        if (xlo <= i0 - 1 + X && i0 - 1 + X <= xhi && ylo <= j0 - 1 + y && j0 - 1 + y <= yhi) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float e = ldf(f[c], off);
                mn[c] = fminf(mn[c], e); mx[c] = fmaxf(mx[c], e); poison = __builtin_fmaf(0.f, e, poison);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64)); }
    const bool wbad = __any(!(poison == 0.f));
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { part[wv * 8 + c] = mn[c]; part[wv * 8 + 3 + c] = mx[c]; }
        part[wv * 8 + 6] = wbad ? 1.f : 0.f;
    }
    __syncthreads();
    bad = false;
#pragma unroll
    for (int w = 0; w < 4; w++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { mn[c] = fminf(mn[c], part[w * 8 + c]); mx[c] = fmaxf(mx[c], part[w * 8 + 3 + c]); }
        bad = bad || part[w * 8 + 6] != 0.f;
    }
}

// The cells the taps of a block can land in, along one axis.
//
// Proof of the bound.  A mapped tap is a three-level lerp of nodes the thread reads, each level with a weight c in [0, 1],
// and every such node lies in [mn, mx] (tile_range; no NaN, no Inf).  One level, by form:
//   * exact build, compile-time weights (lerp_q): c = 0 returns a; c = 1/2 and the Q4 form round the exact convex
//     combination once, and rounding a number between two floats stays between them; c = 1/4 (lerp_const) rounds the exact
//     combination to double, then to float -- the same; c = 3/4 rounds c * b to float first, so the sum can sit half an
//     ulp above the larger operand and round to the next float: one ulp of excess at most;
//   * exact build, tabled weights (lerp_w): c * b is rounded to float as well -- one ulp;
//   * one-fma build: fmaf(c, b - a, a) rounds b - a, an error of at most 2^-24 |b - a| <= 2^-24 (mx - mn), then the sum.
// So a level leaves [mn, mx] by at most 2^-24 (mx - mn) + 2^-23 max(|mn|, |mx|), three levels by 3 * 2^-24 (mx - mn) +
// 3 * 2^-23 max(|mn|, |mx|) to first order, against e = 2^-21 ((mx - mn) + max(|mn|, |mx|)) = 8 * 2^-24 (mx - mn) +
// 4 * 2^-23 max(|mn|, |mx|): a third to spare on the tighter term, which covers the second order (levels two and three start
// from values that carry the excess already) and an underflowing c * b (2^-149 at most).  mx - mn overflowing makes e infinite and the range
// the whole clamp interval, which is still a bound.  The kernel then clamps the tap to [lo, hi] (v_med3_f32) and locates
// it: q = pos / h in locate's own arithmetic (origin 0: an unstaggered field), cell = floor(q).  Clamp, division and floor
// are monotone, so every tap's cell lies in [*c0, *c1] = [floor(q(clamp(mn - e))), floor(q(clamp(mx + e)))], and
// 0 <= *c0 because lo >= 0.  false: no bound (an empty range, or a q that is no index at all).
template <bool P2>
__device__ __forceinline__ bool tap_cells(float mn, float mx, float lo, float hi, const Spacing &sp, int *c0, int *c1)
{
    const float e = 4.76837158203125e-7f * ((mx - mn) + fmaxf(fabsf(mn), fabsf(mx)));
    const float pa = __builtin_amdgcn_fmed3f(mn - e, lo, hi), pb = __builtin_amdgcn_fmed3f(mx + e, lo, hi);
    // (locate's fma form adds -org / h = 0 to the exact product: the same value)
    const float qa = div_h<P2>(pa - 0.f, sp), qb = div_h<P2>(pb - 0.f, sp);
    if (!(mn <= mx && qa >= 0.f && qb < 16777216.f)) return false;      // (dims_ok keeps every dimension below 2^23; a NaN fails)
    *c0 = floor_to_int(qa);
    *c1 = floor_to_int(qb);
    return true;
}

// true when no tap of the block can read a node of an occupied brick.  Block-uniform: every argument is, and every wave
// runs the whole test itself (lanes take one brick each along x, then a ballot), so no barrier is needed.
//
// From cells to nodes.  A tap reads the nodes of its cell and of the next one up on every axis (corners()), so the taps read
// indices [c0, c1 + 1]; the test covers [c0 - 1, c1 + 2], one more on either side than the argument needs, cut off at 0
// (there is nothing below: c0 >= 0).  At the upper end the flat indexing of corners() decides what "one further" is:
//   * x beyond nx - 1 is the start of the NEXT ROW: the test then covers the whole row range and one more row;
//   * y beyond ny - 1 (after that) is the start of the NEXT PLANE: the whole plane range and one more plane;
//   * z beyond nz - 1 is outside the allocation, where every load returns 0 (the buffer's range check): cut off.
// A negative flat index -- the other special case of corners() -- needs a negative cell, and there is none.
// Every brick index used below therefore lies inside the flag array.
template <bool P2>
__device__ __forceinline__ bool taps_in_empty_bricks(const Sparse &s, const float (&mn)[3], const float (&mx)[3], bool bad,
                                                     f3 lo, f3 hi, const Spacing &sp, int nx, int ny, int nz)
{
    if (bad) return false;
    int x0, x1, y0, y1, z0, z1;
    if (!tap_cells<P2>(mn[0], mx[0], lo.x, hi.x, sp, &x0, &x1) || !tap_cells<P2>(mn[1], mx[1], lo.y, hi.y, sp, &y0, &y1) ||
        !tap_cells<P2>(mn[2], mx[2], lo.z, hi.z, sp, &z0, &z1)) return false;
    x0 = max(x0 - 1, 0); y0 = max(y0 - 1, 0); z0 = max(z0 - 1, 0);
    x1 += 2; y1 += 2; z1 += 2;
    if (x1 > nx - 1) { x0 = 0; x1 = nx - 1; y1 += 1; }
    if (y1 > ny - 1) { y0 = 0; y1 = ny - 1; z1 += 1; }
    z1 = min(z1, nz - 1);
    if (x0 > x1 || y0 > y1 || z0 > z1) return false;                     // (a range wholly past the last plane: not worth a case)
    const int bx0 = __builtin_amdgcn_readfirstlane(x0 >> kBrickShift), bx1 = __builtin_amdgcn_readfirstlane(x1 >> kBrickShift);
    const int by0 = __builtin_amdgcn_readfirstlane(y0 >> kBrickShift), by1 = __builtin_amdgcn_readfirstlane(y1 >> kBrickShift);
    const int bz0 = __builtin_amdgcn_readfirstlane(z0 >> kBrickShift), bz1 = __builtin_amdgcn_readfirstlane(z1 >> kBrickShift);
    // a map that jumps inside the block covers many bricks: not worth testing (8 rounds of 64 bricks at most)
    if ((long long)(by1 - by0 + 1) * (bz1 - bz0 + 1) * ((bx1 - bx0 + 64) >> 6) > 8) return false;
    bool occupied = false;
    for (int bz = bz0; bz <= bz1; bz++)
        for (int by = by0; by <= by1; by++) {
            const unsigned char *row = s.flags + (size_t)s.nbx * (by + (size_t)s.nby * bz);
            for (int bx = bx0 + (int)threadIdx.x; bx <= bx1; bx += 64) occupied |= row[bx] != 0;      // (no short circuit: the rounds' loads go out together)
        }
    return !__any(occupied);
}

// SPARSE == 1: a block that is not skipped enters the list (one atomic per block).  b: its linear index in the grid
__device__ __forceinline__ void list_block(const Sparse &s, int b)
{
    if (threadIdx.x == 0 && threadIdx.y == 0) s.list[1 + atomicAdd(s.list, 1)] = b;
}
// SPARSE == 2: which block of the grid this workgroup computes, false: none.  The flag pass found no empty brick: nothing
// was classified and this launch is the plain one, every workgroup its own block.  Otherwise workgroup b takes entry b.
__device__ __forceinline__ bool listed_block(const Sparse &s, int &bX, int &bY, int &bZ)
{
    if (*s.word != s.epoch) return true;
    const int b = bX + gridDim.x * (bY + gridDim.y * bZ);
    if (b >= s.list[0]) return false;
    const int e = s.list[1 + b];
    bX = e % (int)gridDim.x;
    const int t = e / (int)gridDim.x;
    bY = t % (int)gridDim.y; bZ = t / (int)gridDim.y;
    return true;
}

// the counters of FL_OPT_SKIP_EMPTY_BRICKS = 2 and 4: one atomic per tested block
__device__ __forceinline__ void count_block(const Sparse &s, bool skipped)
{
    if (s.stats && threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(s.stats + (skipped ? 1 : 0), 1ull);
}

// ---- FL_OPT_SKIP_EMPTY_TAPS: the test inside the operator's own launch, wave by wave (SPARSE == 3) ----
//
// A block's tile range bounds where its taps COULD land; the kernel computes where they DO land, and that costs it only the
// map look-up.  So there is no classifying launch: after map9_lds and the clamp every lane finds the cell of each of its nine
// taps -- by locate()'s own expressions, so it is the cell corners() will read -- and looks up one byte per tap, the CELL flag
// of the 8 x 8 x 8 brick that holds the cell's base node.  If no lane of the wave finds a set flag, every word the wave's
// gathers could load is 0x00000000 and the wave runs the operator's stores with every gather result taken as +0.0f.
//
// The cell flag of brick C is 0 only if every word corners() can deliver for a cell whose base node lies in C is 0x00000000.
// A cell with base (i, j, k) reads the flat indices base + {0, 1} + nx {0, 1} + nx ny {0, 1}: the nodes of C and of its +1
// neighbours on each axis, and at the array's upper ends what the flat index wraps into (the rule stated at
// taps_in_empty_bricks: x past nx - 1 is the start of the next row, y past ny - 1 the start of the next plane, z past nz - 1 lies
// outside the allocation and reads 0).  Base indices run to n INCLUSIVE on every axis -- the accumulate clamps to [0, h n] --
// so the array has (n >> 3) + 1 bricks per axis, which covers base index n where n is a multiple of 8.
//
// A Sparse for this form carries the CELL flags in `flags`, their dims in nbx / nby, the wave counters in `stats`, no list.
struct CellDims { int ncx, ncy, ncz; };
__host__ __device__ inline CellDims cell_dims(int nx, int ny, int nz)
{
    return CellDims{ (nx >> kBrickShift) + 1, (ny >> kBrickShift) + 1, (nz >> kBrickShift) + 1 };
}

// One wave per cell brick (four to a block): the node range its cells' corners cover, by the rule above, then an OR over the
// brick flags of that range, the lanes taking one brick each.  Every brick index lies inside the flag array: the ranges are
// cut to [0, n - 1] before they are used.
__global__ __launch_bounds__(256) void cell_flags_kernel(const unsigned char *flags, unsigned char *cells, int nx, int ny, int nz)
{
    const CellDims d = cell_dims(nx, ny, nz);
    const int c = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + threadIdx.y));
    if (c >= d.ncx * d.ncy * d.ncz) return;
    const int cx = c % d.ncx, t = c / d.ncx, cy = t % d.ncy, cz = t / d.ncy;
    // base nodes [8 c, min(8 c + 7, n)], their corners one further
    int x0 = cx << kBrickShift, x1 = min(x0 + kBrick - 1, nx) + 1;
    int y0 = cy << kBrickShift, y1 = min(y0 + kBrick - 1, ny) + 1;
    int z0 = cz << kBrickShift, z1 = min(z0 + kBrick - 1, nz) + 1;
    if (x1 > nx - 1) { x0 = 0; x1 = nx - 1; y1 += 1; }
    if (y1 > ny - 1) { y0 = 0; y1 = ny - 1; z1 += 1; }
    z1 = min(z1, nz - 1);
    bool occupied = false;
    if (z0 <= z1) {                                         // (else: every corner lies past the last plane and reads 0)
        const int nbx = (nx + kBrick - 1) >> kBrickShift, nby = (ny + kBrick - 1) >> kBrickShift;
        const int bx0 = x0 >> kBrickShift, by0 = y0 >> kBrickShift, bz0 = z0 >> kBrickShift;
        const int wx = (x1 >> kBrickShift) - bx0 + 1, wy = (y1 >> kBrickShift) - by0 + 1, wz = (z1 >> kBrickShift) - bz0 + 1;
        for (int e = (int)threadIdx.x; e < wx * wy * wz; e += 64) {
            const int ex = e % wx, r = e / wx, ey = r % wy, ez = r / wy;
            occupied |= flags[(size_t)(bx0 + ex) + (size_t)nbx * ((by0 + ey) + (size_t)nby * (bz0 + ez))] != 0;
        }
    }
    const bool any = __any(occupied);
    if (threadIdx.x == 0) cells[c] = any ? 1 : 0;
}

// true when some tap of some lane of this wave may read a word that is not 0x00000000.  mp: the clamped positions; the sampled
// fields are unstaggered, origin 0 on every axis.  The cell is locate<true, true>'s: there q = fma(pos, 1 / h, +0), here
// q = pos * (1 / h) -- both round the same exact product once and can differ in the sign of a zero only, which floor does not
// see.  (Written as a product on purpose: stated as locate's fma the compiler shares the nine cells with the gathers further
// down and keeps 27 more registers alive across the test, which spills.)  The clamp to [0, h n] with h a power of two bounds
// every index by [0, n]: each byte read lies inside the cell-flag array.  The nine loads go out together: one wait.
__device__ __forceinline__ bool wave_taps_may_read(const Sparse &s, const Spacing &sp, const f3 (&mp)[9])
{
    unsigned char fl[9];
#pragma unroll
    for (int a9 = 0; a9 < 9; a9++) {
        const int i = floor_to_int(mp[a9].x * sp.inv_h), j = floor_to_int(mp[a9].y * sp.inv_h), k = floor_to_int(mp[a9].z * sp.inv_h);
        fl[a9] = s.flags[(unsigned)((i >> kBrickShift) + __mul24(s.nbx, (j >> kBrickShift) + __mul24(s.nby, k >> kBrickShift)))];
    }
    unsigned acc = 0u;
#pragma unroll
    for (int a9 = 0; a9 < 9; a9++) acc |= fl[a9];
    return __any(acc != 0u);
}

// the counters of fl_sparse_wave_stats: [0] waves tested and kept, [1] waves tested and skipped -- one atomic per wave, by its
// first active lane
__device__ __forceinline__ void count_wave(const Sparse &s, bool skipped)
{
    if (!s.stats) return;
    const unsigned long long live = __ballot(1);
    if (__lane_id() == (unsigned)(__ffsll((long long)live) - 1)) atomicAdd(s.stats + (skipped ? 1 : 0), 1ull);
}

} // inline namespace BQ_VARIANT
} // namespace bq
