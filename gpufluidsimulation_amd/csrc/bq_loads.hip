// bq_loads.hip -- per-obstacle pressure force and torque on the device: gpu_obstacle_loads walks the
// owner-tagged cell flags once and returns, per obstacle, the sums over its wetted faces (an obstacle cell next to a fluid
// cell) of the signed face pressure, its moment about the obstacle's centre, the face count and the plain pressure sum as
// BQ_MAX_BOUNDARIES x BQ_LOAD_COUNT doubles in device memory.  The definitions are the contract of include/bimocq_gpu.h, every
// line one IEEE double operation (-ffp-contract=off); tests/cpu_abi/obstacle_loads_abi.c restates them in plain C.
//
//   obstacle_loads_kernel  blocks of four waves march a chunk of planes, a wave = 256 cells of one row (j, k) at a time, so the
//                          rows summary is a wave-uniform test and a clean row costs one byte per wave.  A lane reads the flags
//                          of four cells as one word (byte by byte where rows are no multiple of four cells); a wave whose
//                          256 cells hold no obstacle cell moves on after one ballot.  Only an OBSTACLE cell looks at its six
//                          neighbours' flags, and only a fluid neighbour's pressure enters the arithmetic: where a lane has
//                          no such neighbour the load goes to another valid address and its value is dropped by a select.
//                          The loads of eight planes are issued together.  A lane keeps ONE accumulator set, for the
//                          owner it met last; when some lane of the wave meets another owner (a column that
//                          crosses two obstacles), and at the end of the march, the wave loops over the distinct owners its
//                          lanes hold (__ballot), reduces each with wave_sum and lane 0 adds the eight sums to the wave's row
//                          of a [4 waves][16 owners][8] LDS table.  The block stores its n x 8 partials plainly.
//   loads_reduce_kernel    one block adds the partial rows in fixed order (1024 / (8 n) runs of consecutive blocks, then the
//                          run sums left to right) and writes ALL 128 outputs, zeros in the rows o >= n.
// No floating-point atomics: two calls on the same data return the same bits, and so do calls with and without `rows` (a
// skipped row holds no obstacle cell, so its lanes hold nothing either way).  Everything is queued on the compute stream;
// nothing synchronises once the library's scratch holds the partials (scratch() waits for the stream when it has to grow).
#include "bq_device.hip.h"
#include "bq_host.h"
#include "bq_launch_geom.h"
#include <algorithm>

namespace bq {

struct LoadGeom { int ni, nj, nk, n; double h; };
struct LoadCentres { double cx[BQ_MAX_BOUNDARIES], cy[BQ_MAX_BOUNDARIES], cz[BQ_MAX_BOUNDARIES]; };

// the wetted face between the obstacle cell S = (i, j, k) and its fluid neighbour one step d = +-1 along axis A, whose
// pressure is pf: the eight terms of include/bimocq_gpu.h added to acc, centre (cx, cy, cz)
template <int A>
__device__ __forceinline__ void load_face(double (&acc)[BQ_LOAD_COUNT], int d, int i, int j, int k, double pf, double h,
                                          double cx, double cy, double cz)
{
    const double s = d > 0 ? -1.0 : 1.0;                // +1 when S has the higher index
    const double f = s * pf;
    const double x = (A == 0 ? (double)(2 * i + d) * 0.5 : (double)i) * h;
    const double y = (A == 1 ? (double)(2 * j + d) * 0.5 : (double)j) * h;
    const double z = (A == 2 ? (double)(2 * k + d) * 0.5 : (double)k) * h;
    const double rx = x - cx, ry = y - cy, rz = z - cz;
    acc[BQ_LOAD_PX + A] += f;
    if (A == 0) { acc[BQ_LOAD_MY] += rz * f; acc[BQ_LOAD_MZ] -= ry * f; }
    if (A == 1) { acc[BQ_LOAD_MZ] += rx * f; acc[BQ_LOAD_MX] -= rz * f; }
    if (A == 2) { acc[BQ_LOAD_MX] += ry * f; acc[BQ_LOAD_MY] -= rx * f; }
    acc[BQ_LOAD_FACES] += 1.0;
    acc[BQ_LOAD_PSUM] += pf;
}

constexpr int kLoadCells = 4;       // cells of a row per lane: a wave takes 256 cells of a row with one flag word per lane
constexpr int kLoadPlanes = 8;      // planes whose summary bytes, then flag words, are requested before the first is looked at

// the flags of the cells i0 .. i0 + 3 of a row whose first byte is solid[at], lowest cell in the low byte; 0 beyond the row's
// end.  WORD: ni % 4 == 0 and a 4-byte aligned array, so the four bytes are one aligned word inside the row.
template <bool WORD>
__device__ __forceinline__ unsigned load_flags4(const unsigned char *__restrict__ solid, size_t at, int i0, int ni)
{
    if (WORD) return i0 < ni ? *reinterpret_cast<const unsigned *>(solid + at) : 0u;
    unsigned w = 0;
#pragma unroll
    for (int c = 0; c < kLoadCells; c++)
        if (i0 + c < ni) w |= (unsigned)solid[at + c] << (8 * c);
    return w;
}

// Chunk blockIdx.z marches the planes [bz kc, min((bz + 1) kc, nk)); wave w of the block takes row j = 4 by + w, lane l its
// cells 256 bx + 4 l .. + 3.  Every thread of the block takes both barriers and every wave-wide operation; a lane whose cells
// lie outside the grid holds flags of 0.  The march is latency-bound when every plane waits for its summary byte and then for
// its flags, so the loads of kLoadPlanes planes are issued together.  part: n x 8 doubles per block.
template <typename T, bool WORD>
__global__ __launch_bounds__(256) void obstacle_loads_kernel(const T *__restrict__ p, const unsigned char *__restrict__ solid,
                                                             const unsigned char *__restrict__ rows, LoadGeom g, LoadCentres c,
                                                             int kc, double *__restrict__ part)
{
    __shared__ double wacc[4][BQ_MAX_BOUNDARIES][BQ_LOAD_COUNT];
    __shared__ double ctr[3][BQ_MAX_BOUNDARIES];
    const int tx = threadIdx.x, tid = tx + 64 * threadIdx.y;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int ni = g.ni, nj = g.nj, nk = g.nk, n = g.n;
    for (int a = tid; a < 4 * BQ_MAX_BOUNDARIES * BQ_LOAD_COUNT; a += 256) (&wacc[0][0][0])[a] = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int o = 0; o < BQ_MAX_BOUNDARIES; o++) { ctr[0][o] = c.cx[o]; ctr[1][o] = c.cy[o]; ctr[2][o] = c.cz[o]; }
    }
    __syncthreads();
    const int i0 = (blockIdx.x * 64 + tx) * kLoadCells, j = blockIdx.y * 4 + wave;
    const int k0 = blockIdx.z * kc, k1 = min(k0 + kc, nk);
    const size_t sj = (size_t)ni, sk = (size_t)ni * (size_t)nj;
    const unsigned char *__restrict__ rsum = rows ? rows : solid;      // (no summary: a byte that is there, not looked at)
    int held = -1;                                      // the owner this lane's sums belong to
    double acc[BQ_LOAD_COUNT];
#pragma unroll
    for (int t = 0; t < BQ_LOAD_COUNT; t++) acc[t] = 0.0;
    // the lanes' sums into the wave's LDS rows, one distinct owner after the other, lowest holding lane first (wave-uniform call)
    auto flush = [&]() {
        unsigned long long m = __ballot(held >= 0);
        while (m) {
            const int o = __shfl(held, __ffsll((long long)m) - 1, 64);
            const bool mine = held == o;
#pragma unroll
            for (int t = 0; t < BQ_LOAD_COUNT; t++) {
                const double s = wave_sum(mine ? acc[t] : 0.0);
                if (tx == 0) wacc[wave][o][t] += s;
            }
            m &= ~__ballot(mine);
        }
        held = -1;
#pragma unroll
        for (int t = 0; t < BQ_LOAD_COUNT; t++) acc[t] = 0.0;
    };
    for (int kb = k0; kb < k1; kb += kLoadPlanes) {
        bool on[kLoadPlanes];
        unsigned w[kLoadPlanes];
        // (a conditional load is a branch and a wait of its own: the loads below go to an address that is valid either way and
        // the value is dropped where it does not count, so that they leave together)
        // the summary bytes of the batch's rows (j, kb .. kb + 7) in ONE load: lane l asks for plane kb + (l & 7), a ballot hands
        // every lane all eight answers (wave-uniform: a clean row costs the wave this one byte)
        const int ku = kb + (tx & (kLoadPlanes - 1));
        const bool row = ku < k1 && j < nj;
        const unsigned char rbyte = rsum[row ? (size_t)j + (size_t)nj * ku : 0];
        const unsigned long long rmask = __ballot(row && (!rows || rbyte != 0));
#pragma unroll
        for (int u = 0; u < kLoadPlanes; u++) on[u] = (rmask >> u) & 1ull;
#pragma unroll
        for (int u = 0; u < kLoadPlanes; u++)
            w[u] = on[u] ? load_flags4<WORD>(solid, (size_t)i0 + sj * j + sk * (kb + u), i0, ni) : 0u;
#pragma unroll 1
        for (int u = 0; u < kLoadPlanes; u++) {
            unsigned ww = w[0];
#pragma unroll
            for (int v = 1; v < kLoadPlanes; v++) ww = u == v ? w[v] : ww;         // (constant indices: w stays in registers)
            if (__ballot((ww & 0x7f7f7f7fu) != 0u) == 0ull) continue;              // no obstacle cell in the wave's 256 cells
            const int k = kb + u;
            const size_t ic0 = (size_t)i0 + sj * j + sk * k;
            // Requests first, sums after: the neighbour flags of the lane's four cells travel together, then the pressures of
            // the fluid neighbours, so a wave that marches through an obstacle waits two load latencies per plane and not two
            // per cell.  The x neighbours inside the word come from the word itself.
            int own[kLoadCells];
            unsigned wet = 0;                           // bit 6 cc + m: neighbour m (-x, +x, -y, +y, -z, +z) of cell cc is a wetted face's F
#pragma unroll
            for (int cc = 0; cc < kLoadCells; cc++) {
                own[cc] = (int)((ww >> (8 * cc)) & 0x7fu);
                if (own[cc] > n) own[cc] = 0;           // the caller's list is shorter than the flags say: not a cell of anyone
            }
#pragma unroll
            for (int cc = 0; cc < kLoadCells; cc++) {
                const int i = i0 + cc;
                const size_t ic = ic0 + cc;
                const bool obst = own[cc] > 0;
                const size_t safe = obst ? ic : 0;      // (an obstacle cell lies inside the array)
                auto flag = [&](bool there, size_t at) { const unsigned f = solid[there ? at : safe]; return there ? f : 1u; };
                unsigned fl[6];
                fl[0] = cc > 0 ? (ww >> (8 * (cc - 1))) & 0xffu : flag(obst && i > 0, ic - 1);
                fl[1] = cc < kLoadCells - 1 ? (i < ni - 1 ? (ww >> (8 * (cc + 1))) & 0xffu : 1u) : flag(obst && i < ni - 1, ic + 1);
                fl[2] = flag(obst && j > 0, ic - sj);
                fl[3] = flag(obst && j < nj - 1, ic + sj);
                fl[4] = flag(obst && k > 0, ic - sk);
                fl[5] = flag(obst && k < nk - 1, ic + sk);
#pragma unroll
                for (int m = 0; m < 6; m++)
                    if (obst && fl[m] == 0u) wet |= 1u << (6 * cc + m);
            }
            if (__ballot(wet != 0u) == 0ull) continue;  // interior cells only: nothing to add, no pressure to request
            T pv[6 * kLoadCells];
#pragma unroll
            for (int cc = 0; cc < kLoadCells; cc++) {
                const size_t ic = ic0 + cc;
                const size_t nb[6] = { ic - 1, ic + 1, ic - sj, ic + sj, ic - sk, ic + sk };
#pragma unroll
                for (int m = 0; m < 6; m++) {           // (p of a cell that is no F is fetched from the lane's own cell and dropped)
                    const bool f = (wet >> (6 * cc + m)) & 1u;
                    const T v = p[f ? nb[m] : (own[cc] > 0 ? ic : 0)];
                    pv[6 * cc + m] = f ? v : (T)0;
                }
            }
#pragma unroll
            for (int cc = 0; cc < kLoadCells; cc++) {
                if (__ballot(own[cc] > 0 && held >= 0 && held != own[cc] - 1)) flush();
                if (own[cc] == 0) continue;
                held = own[cc] - 1;
                if (((wet >> (6 * cc)) & 63u) == 0u) continue;
                const int i = i0 + cc;
                const double cx = ctr[0][held], cy = ctr[1][held], cz = ctr[2][held];
                if ((wet >> (6 * cc + 0)) & 1u) load_face<0>(acc, -1, i, j, k, (double)pv[6 * cc + 0], g.h, cx, cy, cz);
                if ((wet >> (6 * cc + 1)) & 1u) load_face<0>(acc, +1, i, j, k, (double)pv[6 * cc + 1], g.h, cx, cy, cz);
                if ((wet >> (6 * cc + 2)) & 1u) load_face<1>(acc, -1, i, j, k, (double)pv[6 * cc + 2], g.h, cx, cy, cz);
                if ((wet >> (6 * cc + 3)) & 1u) load_face<1>(acc, +1, i, j, k, (double)pv[6 * cc + 3], g.h, cx, cy, cz);
                if ((wet >> (6 * cc + 4)) & 1u) load_face<2>(acc, -1, i, j, k, (double)pv[6 * cc + 4], g.h, cx, cy, cz);
                if ((wet >> (6 * cc + 5)) & 1u) load_face<2>(acc, +1, i, j, k, (double)pv[6 * cc + 5], g.h, cx, cy, cz);
            }
        }
    }
    flush();
    __syncthreads();
    if (tid < n * BQ_LOAD_COUNT) {
        const int o = tid / BQ_LOAD_COUNT, t = tid % BQ_LOAD_COUNT;
        const size_t b = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
        part[b * (size_t)(n * BQ_LOAD_COUNT) + tid] = ((wacc[0][o][t] + wacc[1][o][t]) + wacc[2][o][t]) + wacc[3][o][t];
    }
}

// d_out[t] for all t < 128.  The 1024 threads form Q = 1024 / n8 runs of n8 columns: thread (q, t) adds column t of the partial
// rows [q per, min(nb, (q + 1) per)), per = ceil(nb / Q), in order; then the threads of run 0 add the Q run sums left to right.
// Columns t >= n8 (rows o >= n) are 0; n8 = 0 or nb = 0 writes 128 zeros.
__global__ __launch_bounds__(1024) void loads_reduce_kernel(const double *__restrict__ part, int nb, int n8, double *__restrict__ out)
{
    __shared__ double run[1024];
    const int tid = threadIdx.x;
    const int Q = n8 > 0 ? 1024 / n8 : 0, q = n8 > 0 ? tid / n8 : 0, t = n8 > 0 ? tid % n8 : 0;
    if (q < Q) {
        const int per = (nb + Q - 1) / Q, b0 = min(nb, q * per), b1 = min(nb, b0 + per);
        double a = 0.0;
#pragma unroll 8
        for (int b = b0; b < b1; b++) a += part[(size_t)b * n8 + t];        // (the loads of eight rows are in flight together)
        run[q * n8 + t] = a;
    }
    __syncthreads();
    if (tid < BQ_MAX_BOUNDARIES * BQ_LOAD_COUNT) {
        double a = 0.0;
        if (tid < n8)
            for (int r = 0; r < Q; r++) a += run[r * n8 + tid];
        out[tid] = a;
    }
}

// [a, a + na) and [b, b + nb) bytes share a byte
static bool ld_overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// chunk length of the march over nk planes: whole rounds of two blocks per CU with about 16 planes per chunk
// (bq_launch_geom.h), and no chunk shorter than 8 planes
static int loads_chunk(int row_blocks, int nk)
{
    const int nchunks = geom::whole_round_chunks(row_blocks, nk, 16, 512);
    return std::min(nk, std::max((nk + nchunks - 1) / nchunks, 8));
}

} // namespace bq

using namespace bq;

extern "C" int gpu_obstacle_loads(const float *p, const double *p64, const unsigned char *solid, const unsigned char *rows,
                                  const bq_boundary *b, int n, float h, int ni, int nj, int nk, double *d_out)
{
    static const char *op = "gpu_obstacle_loads";
    if (!ensure_ready(op)) return fl_last_error();
    const int before = fl_last_error();
    auto refuse = [&](const char *why) { latch(FL_ERR_BAD_ARGUMENT, op, why); return (int)FL_ERR_BAD_ARGUMENT; };
    if ((p != nullptr) == (p64 != nullptr)) return refuse("exactly one of p and p64");
    if (!solid || !d_out) return refuse("null solid or d_out");
    if (n < 0 || n > BQ_MAX_BOUNDARIES) return refuse("0 .. 16 obstacles");
    if (n > 0 && !b) return refuse("obstacles without a list");
    for (int o = 0; o < n; o++)
        if (!std::isfinite(b[o].cx) || !std::isfinite(b[o].cy) || !std::isfinite(b[o].cz)) return refuse("non-finite centre");
    if (!std::isfinite(h) || !(h > 0.f)) return refuse("h not finite or not positive");
    if (ni < 3 || nj < 3 || nk < 3) return refuse("dims below 3");
    if (4.0 * (double)(ni + 1) * (double)(nj + 1) * (double)(nk + 1) >= 2147483648.0) return refuse("field larger than 2 GiB");
    if ((double)(ni + 1) * (double)(nj + 1) >= 8388608.0) return refuse("plane of 2^23 elements or more");
    if (nk + 1 > 65535) return refuse("nk too large for grid.z");
    if ((nj + 4) / 4 > 65535) return refuse("nj too large for grid.y");
    const size_t nc = (size_t)ni * nj * nk, nout = (size_t)BQ_MAX_BOUNDARIES * BQ_LOAD_COUNT * sizeof(double);
    if (ld_overlaps(d_out, nout, p, nc * sizeof(float)) || ld_overlaps(d_out, nout, p64, nc * sizeof(double)) ||
        ld_overlaps(d_out, nout, solid, nc) || ld_overlaps(d_out, nout, rows, (size_t)nj * nk))
        return refuse("d_out overlaps an input");
    const Runtime &r = rt();
    if (r.slab_on) {
        latch(FL_ERR_UNSUPPORTED, op, "not supported under a z-slab context");
        return (int)FL_ERR_UNSUPPORTED;
    }
    const int n8 = n * BQ_LOAD_COUNT;
    const double *part = nullptr;
    size_t nb = 0;
    if (n > 0) {
        LoadGeom g;
        g.ni = ni; g.nj = nj; g.nk = nk; g.n = n; g.h = (double)h;
        LoadCentres c = {};
        for (int o = 0; o < n; o++) { c.cx[o] = (double)b[o].cx; c.cy[o] = (double)b[o].cy; c.cz[o] = (double)b[o].cz; }
        const int gx = (ni + 64 * kLoadCells - 1) / (64 * kLoadCells), gy = (nj + 3) / 4, kc = loads_chunk(gx * gy, nk), gz = (nk + kc - 1) / kc;
        const bool word = ni % 4 == 0 && ((uintptr_t)solid & 3u) == 0;
        nb = (size_t)gx * gy * gz;                      // (below 2^31 / 256 by the size limits)
        double *rowsbuf = (double *)scratch(nb * n8 * sizeof(double));
        if (!rowsbuf) return fl_last_error();
        const dim3 grid(gx, gy, gz);
        if (p) { if (word) obstacle_loads_kernel<float, true><<<grid, kBlock, 0, r.compute>>>(p, solid, rows, g, c, kc, rowsbuf);
                 else      obstacle_loads_kernel<float, false><<<grid, kBlock, 0, r.compute>>>(p, solid, rows, g, c, kc, rowsbuf); }
        else   { if (word) obstacle_loads_kernel<double, true><<<grid, kBlock, 0, r.compute>>>(p64, solid, rows, g, c, kc, rowsbuf);
                 else      obstacle_loads_kernel<double, false><<<grid, kBlock, 0, r.compute>>>(p64, solid, rows, g, c, kc, rowsbuf); }
        BQ_LAUNCH_CHECK("obstacle_loads_kernel");
        part = rowsbuf;
    }
    loads_reduce_kernel<<<1, 1024, 0, r.compute>>>(part, (int)nb, n8, d_out);
    BQ_LAUNCH_CHECK("loads_reduce_kernel");
    return fl_last_error() != before ? fl_last_error() : (int)FL_OK;
}
