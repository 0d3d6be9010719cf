// bq_jacobi_plan.h -- what the Jacobi tuning options mean and which launch they lead to.  FL_OPT_JACOBI_VARIANT / _ROWS /
// _KCHUNK / _KCHUNK2 / _FUSE are raw integers whose codes mean different things to different kernels (option table in
// include/bimocq_gpu.h); decode_jacobi_tuning turns them into named fields once per entry-point call, and the planners below
// choose kernel, template arguments and geometry of the fp32 launches from those fields, the dims and three facts about the
// runtime (pointer alignment, CU count, z-slab context).  Pure integer arithmetic on the host: no HIP, no runtime state, so that
// tests/test_jacobi_plan_cpu.py can compile it with a plain C++ compiler and check every code and decomposition without a GPU.
// The launchers (bq_project.hip, bq_obstacle.hip, bq_mgcg.hip) switch on the result and launch.
#pragma once
#include "bq_launch_geom.h"

namespace bq {
namespace plan {

enum class Single { kAuto, kGeneric, kTile, kMarch };       // the one-sweep kernel
enum class Pair { kAuto, kNever, kAlways };                 // the two-row rendering of the two-sweep kernel
enum class Quad { kAuto, kForced, kNever };                 // four sweeps per launch
enum class Trust { kNever, kChecked, kVouched };            // may sweeps share a launch: never / after comparing the shells / on the caller's word
enum class SweepsFuse { kNone, kPairsOnly, kAll };          // what gpu_jacobi_sweeps (and its masked twin) may fuse

struct JacobiTuning {
    // ---- one sweep per launch
    Single single;          // VARIANT: 0 auto (march where float4 rows apply, else generic), 1 generic, 3 march; every other value: tile
    int march_waves;        // ROWS 4 / 8 / 16: waves per block of jacobi_march_kernel; anything else 4
    int tile_rows;          // ROWS 1 / 2 / 4: float4 rows per thread of jacobi_tile_kernel; anything else 4
    int single_kchunk;      // KCHUNK > 0: planes per chunk of the march and tile kernels -- the prefetch, shape and fp64 codes included: KCHUNK = 24 is also a 24-plane chunk
    // ---- fused launches, fp32
    bool fused_ok;          // VARIANT 0 or 3: any other variant keeps every fused kernel off
    Pair pair_rows;         // ROWS 1 never, 2 always (short chunks included), else where it pays
    bool keep_march2r;      // ROWS 3: jacobi_march2r_kernel instead of jacobi_lean2r_kernel (A/B timing)
    int prefetch;           // KCHUNK 1 / 2: planes the loads of the lean kernels run ahead, fp64 included; 0 = by cache footprint (jacobi_lean3r_kernel: 1)
    int fused_kchunk;       // KCHUNK2 > 0: planes per chunk of every fused kernel, fp64 included; 0 = by rule
    int lds_min_kc;         // shortest chunk the LDS kernels take on whole arrays: 24, a forced chunk length may go down to 8
    bool lds_triple;        // ROWS 0 / 4 / 6 / 7: jacobi_sweep_triple tries the LDS kernels first
    bool lean_triple;       // ROWS other than 1 / 3: jacobi_lean3r_kernel where the LDS kernels refuse -- live on the default path (256 x 256 x 128)
    bool lean_triple_short; // ROWS 2: ... with chunks below 16 planes too
    Quad quad;              // ROWS 0 auto, 6 forced, else never (7: "auto without quads"); needs fused_ok
    int lds_w[2], lds_r[2]; // output waves and rows per wave of jacobi_lds_kernel for S = 3, 4 sweeps ([S - 3]): KCHUNK 18 / 19 / 24 / 25 / 26 = 10 R + W; four sweeps know 18 (6 x 1) and 24 only
    bool masked_triple;     // the masked triple has the default shape only: KCHUNK 19 / 24 / 25 / 26 refuse it (18 is the default); it ignores ROWS altogether
    bool triple_ranges;     // gpu_jacobi_sweep_triple_ranges: FUSE other than 0 / 4, fused_ok, ROWS other than 5 -- but not ROWS 1 / 2 / 3, which it does not honour
    bool pair_ranges;       // gpu_jacobi_sweep_pair_ranges: FUSE other than 0 (negative values pass)
    // ---- FL_OPT_JACOBI_FUSE
    Trust trust;            // <= 0 never, 1 checked, >= 2 vouched
    bool beyond_pairs;      // FUSE other than 4: three and four sweeps per launch allowed
    SweepsFuse sweeps_fuse; // vouched only: everything, or pairs only (FUSE 4)
    // ---- the fp64 smoothers (mg_smooth)
    bool mg_keep_smooth2;   // ROWS 3 / 8: mg_smooth2_kernel instead of mg_lean2r_kernel (A/B timing)
    int mg_smooth2_threads; // ROWS 8: blocks of 512 threads, else 256
    bool mg_lds3_off;       // ROWS 5: never mg_lds3_kernel
    int mg_lds3_rows;       // KCHUNK 14: blocks of 4 output rows (8 waves) instead of 8 (12 waves)
};

inline JacobiTuning decode_jacobi_tuning(int variant, int rows, int kchunk, int kchunk2, int fuse)
{
    JacobiTuning t{};
    t.single = variant == 0 ? Single::kAuto : variant == 1 ? Single::kGeneric : variant == 3 ? Single::kMarch : Single::kTile;
    t.march_waves = rows == 8 || rows == 16 ? rows : 4;
    t.tile_rows = rows == 1 || rows == 2 ? rows : 4;
    t.single_kchunk = kchunk > 0 ? kchunk : 0;
    t.fused_ok = variant == 0 || variant == 3;
    t.pair_rows = rows == 1 ? Pair::kNever : rows == 2 ? Pair::kAlways : Pair::kAuto;
    t.keep_march2r = rows == 3;
    t.prefetch = kchunk == 1 || kchunk == 2 ? kchunk : 0;
    t.fused_kchunk = kchunk2 > 0 ? kchunk2 : 0;
    t.lds_min_kc = kchunk2 > 0 ? 8 : 24;
    t.lds_triple = rows == 0 || rows == 4 || rows == 6 || rows == 7;
    t.lean_triple = rows != 1 && rows != 3;
    t.lean_triple_short = rows == 2;
    t.quad = !t.fused_ok ? Quad::kNever : rows == 0 ? Quad::kAuto : rows == 6 ? Quad::kForced : Quad::kNever;
    const bool shaped = kchunk == 18 || kchunk == 19 || kchunk == 24 || kchunk == 25 || kchunk == 26;
    const int shape3 = shaped ? kchunk : 18, shape4 = kchunk == 18 ? 18 : 24;       // (four sweeps in row pairs, 6 of them: 10 waves at 168 registers spill)
    t.lds_r[0] = shape3 / 10; t.lds_w[0] = shape3 == 19 ? 12 : shape3 % 10;         // (19: single rows, 12 of them: 16 waves per block)
    t.lds_r[1] = shape4 / 10; t.lds_w[1] = shape4 == 18 ? 6 : 4;                    // (18 with four sweeps: 6 single rows + 6 halo waves)
    t.masked_triple = kchunk != 19 && kchunk != 24 && kchunk != 25 && kchunk != 26;
    t.triple_ranges = fuse != 0 && fuse != 4 && rows != 5 && t.fused_ok;
    t.pair_ranges = fuse != 0;
    t.trust = fuse >= 2 ? Trust::kVouched : fuse == 1 ? Trust::kChecked : Trust::kNever;
    t.beyond_pairs = fuse != 4;
    t.sweeps_fuse = t.trust != Trust::kVouched ? SweepsFuse::kNone : t.beyond_pairs ? SweepsFuse::kAll : SweepsFuse::kPairsOnly;
    t.mg_keep_smooth2 = rows == 3 || rows == 8;
    t.mg_smooth2_threads = rows == 8 ? 512 : 256;
    t.mg_lds3_off = rows == 5;
    t.mg_lds3_rows = kchunk == 14 ? 4 : 8;
    return t;
}

// ---- the fp32 launches --------------------------------------------------------------------------------------------------------
enum class Kernel {
    kNone,          // does not apply: nothing launched, the caller takes the next smaller launch
    kEmpty,         // applies, but there is no plane to produce: nothing launched
    kGeneric, kMarch, kTile,                // one sweep
    kLean2r, kMarch2r, kMarch2,             // two
    kLds, kLds2seg, kLean3r                 // three (kLds: S = 3 or 4)
};

struct LaunchPlan {
    Kernel kernel = Kernel::kNone;
    // template selectors: WIDE (rows of 2 - 4 waves; tile kernel: 256-wide tiles), PF (prefetch distance), W x R (march kernel: W waves; tile
    // kernel: R rows per thread; LDS kernels: W output waves of R rows), S sweeps
    bool wide = false;
    int pf = 0, W = 0, R = 0, S = 0;
    int cw = 0;             // lanes per row
    int col_blocks = 1, row_blocks = 0, nbz = 0;        // blocks along x (one-sweep kernels only), along y, k-chunks
    int kc = 0;             // planes per chunk
    int nblk = 0;           // blocks that have work
    int grid = 0, block = 0;        // the launch: blocks (the LDS kernels round nblk up to a multiple of 8), threads per block
    explicit operator bool() const { return kernel != Kernel::kNone; }
};

// float4 rows: 16-byte aligned buffers, rows that are a multiple of 4 and at least 32 floats
inline bool float4_rows(int ni, bool aligned16) { return ni % 4 == 0 && ni >= 32 && aligned16; }

// One sweep.  The plane range of gpu_jacobi_sweep_range does not enter: the kernels clip, the geometry is that of the whole array.
inline LaunchPlan plan_single(int ni, int nj, int nk, bool aligned16, const JacobiTuning &tun)
{
    LaunchPlan p;
    if (ni < 3 || nj < 3 || nk < 3) { p.kernel = Kernel::kEmpty; return p; }          // no interior
    const bool tile_ok = float4_rows(ni, aligned16);
    Single v = tun.single;
    if (v == Single::kAuto) v = tile_ok ? Single::kMarch : Single::kGeneric;
    if (!tile_ok) v = Single::kGeneric;
    if (v == Single::kGeneric) { p.kernel = Kernel::kGeneric; return p; }              // (64 x 4 blocks, one thread per cell: grid_for)
    if (v == Single::kMarch) {
        p.kernel = Kernel::kMarch;
        p.W = tun.march_waves;
        p.block = p.W * 64;
        p.cw = geom::pow2_lanes(ni, 4, p.block);            // float4 columns per tile row: pow2 >= ni/4
        const int rows = p.block / p.cw;
        p.col_blocks = (ni / 4 + p.cw - 1) / p.cw;
        p.row_blocks = (nj + rows - 1) / rows;
        // k-chunk: measured optimum at 256^3 is 16 planes (tools/jacobi_tune.py: 4/8/16/32 planes ->
        // 34.2/34.5/31.8/34.0 us); shorter chunks re-read more planes, longer ones leave CUs idle.
        // Keep >= ~1024 blocks when the grid is small in x/y.
        p.kc = 16;
        while (p.kc > 4 && (long)p.col_blocks * p.row_blocks * ((nk + p.kc - 1) / p.kc) < 1024) p.kc /= 2;
    } else {
        // tile geometry: 256-wide rows when the row is long enough, else 128-wide; R float4 per thread
        p.kernel = Kernel::kTile;
        p.wide = ni > 128;
        p.R = tun.tile_rows;
        p.block = 256;
        const int TX = p.wide ? 256 : 128, TY = (p.wide ? 4 : 8) * p.R;
        p.col_blocks = (ni + TX - 1) / TX;
        p.row_blocks = (nj + TY - 1) / TY;
        // k-chunks: enough blocks to fill 256 CUs x 2 resident blocks, at least 8 planes per chunk
        const int want = (1024 + p.col_blocks * p.row_blocks - 1) / (p.col_blocks * p.row_blocks);
        p.kc = std::max(8, (nk + want - 1) / want);
    }
    if (tun.single_kchunk > 0) p.kc = tun.single_kchunk;
    p.nbz = (nk + p.kc - 1) / p.kc;
    p.nblk = p.grid = p.col_blocks * p.row_blocks * p.nbz;
    return p;
}

// Two sweeps on the plane ranges `pr` (jacobi_lean2r_kernel / jacobi_march2r_kernel / jacobi_march2_kernel).
inline LaunchPlan plan_pair(int ni, int nj, int nk, bool aligned16, const geom::PlaneRanges &pr, const JacobiTuning &tun, int num_cus)
{
    LaunchPlan p;
    if (ni < 3 || nj < 3 || nk < 3 || !tun.fused_ok || !float4_rows(ni, aligned16) || ni > 1024) return p;
    if (pr.planes == 0) { p.kernel = Kernel::kEmpty; return p; }
    const bool whole = pr.whole;
    const int nkr = pr.planes;                           // planes this launch produces
    p.S = 2;
    p.block = 256;
    p.cw = geom::pow2_lanes(ni, 4);                      // float4 lanes per row: <= 64 one wave, 128/256 = 2/4 waves
    p.wide = p.cw > 64;
    const int rows = 256 / p.cw;
    // Two rows per thread (jacobi_march2r_kernel; rows of one wave only).  It has half as many row blocks, runs one
    // 4-wave block per CU best, and like the one-row kernel only pays when the blocks fill the 256 CUs in whole
    // rounds: 256^3 17.1 us per sweep with 8 chunks of 32 planes (256 blocks) against 19.0-19.7 for the one-row
    // kernel, but 21-23 us with chunks of 24-28 and 28 us with chunks of 64; 272 planes 18.0 (8 chunks of 34) against
    // 20.0; 128^3 is slower with it (5.5 vs 4.6: the chunks get too short).  Pair::kAuto = this rule, kNever = one row,
    // kAlways = two rows whenever the kernel applies.  Short plane ranges (the parts of a split launch next to
    // the ghost planes): one chunk per range.
    if (nj >= 4 && tun.pair_rows != Pair::kNever) {
        const int nby2 = (nj + 2 * rows - 1) / (2 * rows);
        // ~32 planes per chunk for rows of one wave; rows of 2-4 waves (WIDE) like longer marches: 512^3 runs 201 us per
        // sweep with 6 chunks of 86 planes, 203-214 with 8 of 64, 226 with 48, 211 with 128 (one-row kernel: 228-238)
        const int target2 = p.wide ? 80 : 32;
        int nchunks = geom::whole_round_chunks(nby2, nkr, target2, 256);
        if (num_cus != 256) nchunks = geom::chunks_for_cus(nkr, nby2, target2, 2, num_cus, 1);
        int kc = (nkr + nchunks - 1) / nchunks;
        // Grids too small to give every CU a chunk of 16 planes (128^3: 8 row blocks): the two-row kernel still wins with the
        // short chunks that fill the chip exactly once -- 128^3: 32 chunks of 4 planes = 256 blocks, 2.99 us per sweep against
        // 4.41 for the one-row kernel with chunks of 8 (chunks of 2 / 3 / 5 planes: 3.34 / 3.73 / 3.24; the three-sweep kernel
        // with chunks of 4: 3.21; profiles/r03_f_jacobi_tune_128_short_chunks.txt) -- a march this short is bound by the latency of its
        // 6 plane steps at one wave per SIMD, so what counts is that no CU waits for a second round.
        // Smaller still (64^3 2.21 against 4.11 us per sweep, 96^3 3.15 / 4.28, 160^3 7.34 / 9.85, 192^3 8.30 / 12.95,
        // 256 x 256 x 64 5.49 / 6.74; profiles/r03_h_jacobi_small_grids.txt): whole arrays always take the two-row kernel,
        // chunks down to two planes.
        bool pays = kc >= 16 || whole;
        if (!whole && pr.longest <= 48) {
            // short ranges (the ends of a split launch): as many chunks as fill the 256 CUs once -- a block marches its
            // chunk plus two warm-up planes, so 2 ranges x 32 row blocks x 4 chunks of 3 planes beat 2 x 32 x 1 of 10
            kc = std::max(2, geom::once_per_cu_len(pr.longest, nby2, pr.nranges, num_cus));
            pays = true;
        }
        if (tun.fused_kchunk > 0) kc = tun.fused_kchunk;
        if (kc < 2) kc = 2;
        if (pays || tun.pair_rows == Pair::kAlways) {
            p.row_blocks = nby2;
            p.kc = kc;
            p.nbz = pr.chunks(kc).nbz;
            p.nblk = p.grid = nby2 * p.nbz;
            if (tun.keep_march2r) { p.kernel = Kernel::kMarch2r; return p; }     // the older rendering of the same kernel
            // the lean rendering: loads run one plane ahead while p, p', div sit in the 256 MiB Infinity Cache, two planes ahead
            // when they come from HBM (512^3: 199.8 -> 195.6 us per sweep; 256^3 15.75 vs 15.95 the other way round).
            const bool in_cache = 12.0 * (double)ni * (double)nj * (double)nk <= 256.0 * 1048576.0;
            p.kernel = Kernel::kLean2r;
            p.pf = tun.prefetch ? tun.prefetch : (in_cache ? 1 : 2);
            return p;
        }
    }
    // planes per block: ~32 measured best at 256^3 (one wave per row), ~64 at 512^3 (248 vs 254 us per sweep).  What
    // matters more is that the blocks fill the 256 CUs in whole rounds of two blocks per CU: at 256^3, 512 blocks
    // (chunks of 32) run 19.1 us per sweep, 576 or 448 blocks (chunks of 28 or 40) 22.7; a z-slab rank with 272
    // planes runs 25.4 us with chunks of 32 (9 of them) and 20.0 with chunks of 34 (8).  So: the number of chunks is
    // the multiple of 512 / gcd(row blocks, 512) closest to planes / target.
    const int nby = (nj + rows - 1) / rows;
    int kchunk = tun.fused_kchunk;
    if (kchunk <= 0) {
        const int target = p.wide ? 64 : 32;
        int nchunks = geom::whole_round_chunks(nby, nkr, target, 512);
        if (num_cus != 256) nchunks = geom::chunks_for_cus(nkr, nby, target, 2, num_cus, 2);
        kchunk = (nkr + nchunks - 1) / nchunks;
        if (kchunk < 16) kchunk = target;                       // small grids: no whole round to fill anyway
        if (!whole && pr.longest <= 48) kchunk = pr.longest;
    }
    while (whole && kchunk > 8 && (long)nby * ((nk + kchunk - 1) / kchunk) < 512) kchunk /= 2;
    // (loads two planes ahead instead of one measured no better at 256^3: 19.4 vs 19.1 us per sweep)
    p.kernel = Kernel::kMarch2;
    p.row_blocks = nby;
    p.kc = kchunk;
    p.nbz = pr.chunks(kchunk).nbz;
    p.nblk = p.grid = nby * p.nbz;
    return p;
}

// S = 3 or 4 sweeps on the plane ranges `pr` through the kernels that exchange the neighbour rows of the intermediate levels via LDS:
// jacobi_lds_kernel<W, R, S>, or for rows of 260 .. 512 floats jacobi_lds2seg_kernel (three sweeps only, 8 output rows per block).
// masked: the masked rendering, the default three-sweep shape only.  min_kc > 0: refused when the chunks come out shorter than
// that, a forced chunk length included (plan_quad's auto rule).
// Block shapes at 256^3, three sweeps, us per sweep (profiles/r03_l_jacobi_lds_kernel_tuning_256.txt): 8 x 1 with chunks of 32 planes 10.79, 4 x 2 11.06, 5 x 2
// 11.59, 6 x 2 with chunks of 26 11.88, 12 x 1 11.23 -- against 13.1-13.6 for jacobi_lean3r_kernel and 15.6 for the two-sweep kernel.
// A launch then takes 32.4 us for 201 MB of compulsory traffic = 6.2 TB/s: like the two-sweep kernel (31.4 us per launch) it sits on
// the fabric, so what is left is more sweeps per launch, not a better schedule -- hence S = 4.
// Later in round 3 (profiles/r03_r2_jacobi_lds_dppadd_256.txt and the runs after it): the l + r stage through v_add_f32_dpp 10.79 -> 10.71; input rings of 5 / 6
// planes (loads one / two steps further ahead) 11.00 / 11.19; the step's prefetch issued last 11.11, the first level ahead
// of the LDS reads 10.76; blocks of 4 single rows, two per CU 11.83; halo waves that skip the levels nobody needs: S = 3
// 10.69, S = 4 in row pairs 11.40 -> 9.98 (39.9 us per launch).  SQ counters: a wave issues 24-28 % of its cycles, is
// parked on waitcnt / barrier 40 % and stalled at issue 33 % (the L1 path: with the prefetch last the stall moves to the
// barrier) -- VALU, LDS and L1 path are each 25-40 % busy but take turns between the barriers.
inline LaunchPlan plan_lds(int ni, int nj, int nk, bool aligned16, const geom::PlaneRanges &pr, const JacobiTuning &tun, int num_cus,
                           int S, bool masked = false, int min_kc = 0, bool walled = false)
{
    LaunchPlan p;
    if (pr.planes == 0) { p.kernel = Kernel::kEmpty; return p; }
    if (masked && !(S == 3 && ni <= 256 && tun.masked_triple)) return p;
    p.S = S;
    const bool two_seg = S == 3 && ni > 256 && ni <= 512 && ni % 4 == 0 && nj >= 8 && nk >= 12 && aligned16 &&
                         (double)ni * nj * nk * 4.0 < 2147483648.0;
    p.W = two_seg ? 8 : tun.lds_w[S - 3];
    p.R = two_seg ? 1 : tun.lds_r[S - 3];
    const int rows_per_block = p.W * p.R;
    if (!two_seg && !(float4_rows(ni, aligned16) && ni <= 256 && nj >= rows_per_block && nk >= 12)) return p;
    p.row_blocks = (nj + rows_per_block - 1) / rows_per_block;
    // chunk length: whole arrays -- as many chunks as fill the CUs once (one block per CU: LDS, registers), refused below 24
    // planes per chunk (2 (S - 1) warm-up planes: the short-march two-row kernel wins there, 128^3: 4.5 us per sweep with chunks
    // of 8 against 3.1) unless the length is forced (tests, tuning: down to 8); plane ranges (a slab chunk's ends and
    // interiors) -- whatever fills the CUs once, down to 2 planes per chunk
    p.kc = std::max(2, geom::once_per_cu_len(pr.longest, p.row_blocks, pr.nranges, num_cus));
    if (tun.fused_kchunk > 0) p.kc = tun.fused_kchunk;
    // (the walled launch has no shorter-march kernel to lose to: what it refuses runs one masked sweep per launch, so it takes
    // whole arrays at whatever length fills the CUs, down to the 2 planes the kernel marches on plane ranges -- 256 x 128 x 40: 3)
    if ((pr.whole && p.kc < (walled ? 2 : tun.lds_min_kc)) || p.kc < min_kc) return p;
    p.kernel = two_seg ? Kernel::kLds2seg : Kernel::kLds;
    p.nbz = pr.chunks(p.kc).nbz;
    p.nblk = p.row_blocks * p.nbz;
    p.grid = 8 * ((p.nblk + 7) / 8);
    p.block = (p.W + 2 * ((S - 1 + p.R - 1) / p.R)) * 64;        // the output waves + the halo waves on either side
    return p;
}

// Four sweeps in one launch (jacobi_lds_kernel<.., 4>), whole unmasked arrays.  Quad::kForced: wherever the kernel applies.
// kAuto: where the chunk rule gives at least 24 planes per chunk (six of a chunk's planes are warm-up; a forced chunk length below
// that keeps the triples) and the process is not a z-slab rank (nothing measures those) -- 256^3: 49 quads + 1 triple for the
// projection's 199 sweeps instead of 66 triples + 1 single sweep (EXPERIMENTS section 10).  128^3 (chunks of 8), rows of
// 260 .. 512 floats (two-segment kernel), masked sweeps and plane ranges never come here or are refused by plan_lds.
inline LaunchPlan plan_quad(int ni, int nj, int nk, bool aligned16, const JacobiTuning &tun, int num_cus, bool slab_on)
{
    if (tun.quad == Quad::kNever || (tun.quad == Quad::kAuto && slab_on)) return LaunchPlan{};
    return plan_lds(ni, nj, nk, aligned16, geom::PlaneRanges(0, 1 << 30, 0, 0, nk), tun, num_cus, 4, false, tun.quad == Quad::kAuto ? 24 : 0);
}

// Three sweeps through jacobi_lean3r_kernel: whole array, rows of one wave, two rows per thread.
inline LaunchPlan plan_lean_triple(int ni, int nj, int nk, bool aligned16, const JacobiTuning &tun, int num_cus)
{
    LaunchPlan p;
    if (!tun.fused_ok || !tun.lean_triple || !float4_rows(ni, aligned16) || ni > 256) return p;
    p.cw = geom::pow2_lanes(ni, 4);
    const int rows = 256 / p.cw;
    p.row_blocks = (nj + 2 * rows - 1) / (2 * rows);
    const int target = 32;
    int nchunks = geom::whole_round_chunks(p.row_blocks, nk, target, 256);
    if (num_cus != 256) nchunks = geom::chunks_for_cus(nk, p.row_blocks, target, 4, num_cus, 1);
    p.kc = (nk + nchunks - 1) / nchunks;
    if (tun.fused_kchunk > 0) p.kc = tun.fused_kchunk;
    if (p.kc < 16 && !tun.lean_triple_short) return p;           // chunks too short to pay for four warm-up planes
    if (p.kc < 4) p.kc = 4;
    p.kernel = Kernel::kLean3r;
    p.S = 3;
    p.pf = tun.prefetch == 2 ? 2 : 1;
    p.nbz = (nk + p.kc - 1) / p.kc;
    p.nblk = p.grid = p.row_blocks * p.nbz;
    p.block = 256;
    return p;
}

// Three sweeps in one launch, whole array: the LDS kernels where the tuning admits them and they apply, else the lean triple.
inline LaunchPlan plan_triple(int ni, int nj, int nk, bool aligned16, const JacobiTuning &tun, int num_cus)
{
    if (ni < 3 || nj < 4 || nk < 3) return LaunchPlan{};
    if (tun.lds_triple && tun.fused_ok)
        if (const LaunchPlan p = plan_lds(ni, nj, nk, aligned16, geom::PlaneRanges(0, 1 << 30, 0, 0, nk), tun, num_cus, 3)) return p;
    return plan_lean_triple(ni, nj, nk, aligned16, tun, num_cus);
}

// Three MASKED sweeps in one launch (gpu_jacobi_sweeps_masked; walled: gpu_jacobi_sweeps_masked_walls): whole array, never on a
// z-slab rank -- there the walled launch goes through plan_triple_masked_ranges on the plane ranges of the slab schedule, and the
// masked one (obstacles) does not exist yet.  The walled launch takes the shapes of the masked one, and short chunks too.
inline LaunchPlan plan_triple_masked(int ni, int nj, int nk, bool aligned16, const JacobiTuning &tun, int num_cus, bool slab_on, bool walled = false)
{
    if (ni < 3 || nj < 4 || nk < 3 || slab_on) return LaunchPlan{};
    return plan_lds(ni, nj, nk, aligned16, geom::PlaneRanges(0, 1 << 30, 0, 0, nk), tun, num_cus, 3, true, 0, walled);
}

// Three WALLED sweeps on plane ranges (gpu_jacobi_sweep_masked_walls_triple_ranges), z-slab ranks included: the shapes
// plan_triple_masked admits on whole arrays, under the switches of plan_triple_ranges; chunks as short as 2 planes, like every
// launch on plane ranges.
inline LaunchPlan plan_triple_masked_ranges(int ni, int nj, int nk, bool aligned16, const geom::PlaneRanges &pr, const JacobiTuning &tun, int num_cus)
{
    if (!tun.triple_ranges || ni < 3 || nj < 4 || nk < 3) return LaunchPlan{};
    return plan_lds(ni, nj, nk, aligned16, pr, tun, num_cus, 3, true, 0, true);
}

// Three sweeps on plane ranges (gpu_jacobi_sweep_triple_ranges): the LDS kernels only.
inline LaunchPlan plan_triple_ranges(int ni, int nj, int nk, bool aligned16, const geom::PlaneRanges &pr, const JacobiTuning &tun, int num_cus)
{
    if (!tun.triple_ranges || ni < 3 || nj < 4 || nk < 3) return LaunchPlan{};
    return plan_lds(ni, nj, nk, aligned16, pr, tun, num_cus, 3);
}

// ---- fp64: how mg_smooth splits the iter - s sweeps it has left into launches of mg_lds3_kernel --------------------------------
// As many triples as leave an even number of launches in total, so that the newest iterate still ends in x, the rest as pairs
// through the same kernel -- 4 sweeps = 2 pairs.  A call that starts from a cleared x (zin: V_Cycle's way down) is free of the
// parity rule: its first launch does not read its input, so with an odd number of launches it writes straight into x
// (swap_first) -- 32 sweeps = 10 triples + 1 pair.  triples < 0: no split exists (an odd number of sweeps left).
struct MgLds3Split { int triples, pairs; bool swap_first; };
inline MgLds3Split mg_lds3_split(int iter, int s, bool zin)
{
    for (int a = (iter - s) / 3; a >= 0; a--) {
        const int rest = iter - s - 3 * a;
        if (rest % 2 == 0 && (zin || (rest / 2 + a) % 2 == 0)) return MgLds3Split{a, rest / 2, zin && (rest / 2 + a) % 2 == 1};
    }
    return MgLds3Split{-1, 0, false};
}

} // namespace plan
} // namespace bq
