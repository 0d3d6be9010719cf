"""CPU tests of csrc/bq_launch_geom.h, the integer rules by which the marching stencil launchers (bq_project.hip, bq_mgcg.hip,
bq_mgcg_fused.hip.inc) choose lanes per row, chunk counts and plane ranges.  The header is compiled with g++ behind
tests/cpu_abi/launch_geom_shim.cpp and called through ctypes.

test_matches_inline_rules compares it, exhaustively over the sizes any launcher can meet, with the expressions the launchers
carried inline before the header existed -- restated here in Python, independently of the header.
test_recorded_configurations pins the decompositions that the launchers' comments quote measurements for."""
import ctypes as C

import numpy as np
import pytest

from build_cpu_host import build_launch_geom

I32P = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def geom():
    lib = C.CDLL(build_launch_geom(), mode=C.RTLD_LOCAL)
    for name, nin in (("geom_pow2_lanes", 3), ("geom_whole_round_chunks", 4), ("geom_chunks_for_cus", 6),
                      ("geom_once_per_cu_len", 4), ("geom_plane_ranges", 1)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = None, [C.c_int] + [I32P] * (nin + 1)

    def call(name, *cols, width=1):
        """one rule of the header on n cases: parallel columns (scalars are broadcast) or one array of n rows; returns int32"""
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in np.broadcast_arrays(*[np.asarray(c) for c in cols])]
        n = arrs[0].shape[0]
        out = np.empty((n, width) if width > 1 else n, dtype=np.int32)
        getattr(lib, name)(n, *arrs, out)
        return out
    return call


def grid(*axes):
    """the cartesian product of the axes as flat int32 columns"""
    return [m.ravel().astype(np.int32) for m in np.meshgrid(*[np.asarray(a) for a in axes], indexing="ij")]


# ---- the launchers' inline expressions, as they stood before the header (int arithmetic; arrays of cases) -------------------
def inline_chunks(nby, nkr, target, rnd):
    """int gcd = nby, rem = 256 | 512; while (rem) { t = gcd % rem; gcd = rem; rem = t; }  quantum = round / gcd;
    nchunks = ((2 nkr + target) / (2 target) + quantum / 2) / quantum * quantum; if (nchunks < quantum) nchunks = quantum;"""
    gcd, rem = nby.astype(np.int64), rnd.astype(np.int64)
    while rem.any():
        nz = rem != 0
        t = gcd[nz] % rem[nz]
        gcd[nz] = rem[nz]
        rem[nz] = t
    quantum = rnd // gcd
    nchunks = ((2 * nkr + target) // (2 * target) + quantum // 2) // quantum * quantum
    return np.where(nchunks < quantum, quantum, nchunks)


def inline_lanes(ni, v, threads=None):
    """int cw = 16; while (cw * V < ni [&& cw < threads]) cw *= 2;"""
    cw = 16
    while cw * v < ni and (threads is None or cw < threads):
        cw *= 2
    return cw


def inline_once_per_cu(longest, nby, nranges, ncus):
    """per_range = max(1, ncus / max(1, nby * nranges)); (max(lenA, lenB) + per_range - 1) / per_range"""
    per_range = np.maximum(1, ncus // np.maximum(1, nby * nranges))
    return (longest + per_range - 1) // per_range


def inline_chunks_for_cus(nkr, nrow, target, warm, ncus, per_cu):
    """chunks_for_cus of bq_project.hip: the loop over n = 1 .. max(1, nkr / 4), run for all cases at once"""
    nkr, nrow, target, warm, ncus, per_cu = [a.astype(np.int64) for a in (nkr, nrow, target, warm, ncus, per_cu)]
    best = np.full(nkr.shape, 1e30)
    best_n = np.ones(nkr.shape, dtype=np.int64)
    best_gap = np.full(nkr.shape, 1 << 30, dtype=np.int64)
    last = np.maximum(1, nkr // 4)
    for n in range(1, int(last.max()) + 1):
        kc = (nkr + n - 1) // n
        blocks = nrow * ((nkr + kc - 1) // kc)
        rounds = (blocks + ncus * per_cu - 1) // (ncus * per_cu)
        cost = rounds.astype(np.float64) * (kc + warm).astype(np.float64)
        gap = np.abs(kc - target)
        take = (n <= last) & ((cost < best * 0.97) | ((cost <= best * 1.03) & (gap < best_gap)))
        best = np.where(take, np.minimum(best, cost), best)
        best_n = np.where(take, n, best_n)
        best_gap = np.where(take, gap, best_gap)
    return best_n


def inline_ranges(k0a, k1a, k0b, k1b, nk, kc):
    """the prelude of jacobi_sweep_pair / jacobi_sweep_lds and the PairRanges / nbz built after it"""
    k0a, k1a, k0b, k1b = max(k0a, 0), min(k1a, nk), max(k0b, 0), min(k1b, nk)
    lenA, lenB = max(k1a - k0a, 0), max(k1b - k0b, 0)
    whole = lenB == 0 and lenA == nk
    chunks_of = lambda ln, c: (ln + c - 1) // c if ln > 0 else 0
    nchA = chunks_of(lenA, kc)
    nbz = nchA + chunks_of(lenB, kc)
    return [k0a, k1a, k0b, k1b, lenA, lenB, lenA + lenB, int(whole), (lenA > 0) + (lenB > 0), max(lenA, lenB), nchA, nbz]


CUS = [256, 248, 240, 128]      # the whole chip, FL_OPT_RESERVE_CUS = 8 and 16 (tests/test_gpu_rccl_path.py), half a chip


def test_matches_inline_rules(geom):
    # whole rounds: every row-block count and plane count a grid of up to 1024 x 1024 x 1100 cells can produce
    nby, nkr, target, rnd = grid(range(1, 513), range(1, 1101), [32, 64, 80], [256, 512])
    got = geom("geom_whole_round_chunks", nby, nkr, target, rnd)
    assert np.array_equal(got, inline_chunks(nby, nkr, target, rnd))

    # lanes per row: float4 and double2 columns, free and capped at the block's threads (jacobi_sweep)
    for v in (2, 4):
        for cap in (None, 256, 512, 1024):
            ni = np.arange(1, 1101)
            got = geom("geom_pow2_lanes", ni, v, cap or 0)
            assert got.tolist() == [inline_lanes(int(n), v, cap) for n in ni], (v, cap)

    # one block per CU
    longest, nby, nranges, ncus = grid(range(1, 601), range(1, 301), [1, 2], CUS)
    got = geom("geom_once_per_cu_len", longest, nby, nranges, ncus)
    assert np.array_equal(got, inline_once_per_cu(longest, nby, nranges, ncus))
    # ... in the form mg_smooth and fuse_geom_rows wrote it for one range: nbz = max(1, ncus / nby); (nk + nbz - 1) / nbz
    one = nranges == 1
    nbz0 = np.maximum(1, ncus[one] // nby[one])
    assert np.array_equal(got[one], (longest[one] + nbz0 - 1) // nbz0)

    # a CU count other than 256
    nkr, nrow, target, warm, ncus, per_cu = grid(range(1, 601), [8, 16, 32, 64, 128], [32, 64, 80], [2, 4], CUS[1:], [1, 2])
    got = geom("geom_chunks_for_cus", nkr, nrow, target, warm, ncus, per_cu)
    assert np.array_equal(got, inline_chunks_for_cus(nkr, nrow, target, warm, ncus, per_cu))

    # plane ranges: whole arrays, proper pairs, empty, reversed and out-of-bounds ones
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(20000):
        nk = int(rng.integers(3, 301))
        kind = rng.integers(0, 4)
        if kind == 0:
            r = [0, 1 << 30, 0, 0]                                   # the launchers' default arguments
        elif kind == 1:
            a, b, c, d = sorted(int(x) for x in rng.integers(0, nk + 1, 4))
            r = [a, b, c, d]                                         # two ordered ranges, either possibly empty
        else:
            r = [int(x) for x in rng.integers(-10, nk + 11, 4)]      # anything: reversed, overlapping, out of bounds
        cases.append(r + [nk, int(rng.integers(1, 65))])
    cases.append([0, 0, 0, 0, 3, 1])
    cases.append([0, 3, 0, 0, 3, 64])
    cases = np.array(cases, dtype=np.int32)
    got = geom("geom_plane_ranges", cases, width=12)
    want = np.array([inline_ranges(*(int(x) for x in row)) for row in cases], dtype=np.int32)
    assert np.array_equal(got, want)
    assert want[:, 7].sum() > 1000 and (want[:, 8] == 2).sum() > 1000 and (want[:, 6] == 0).sum() > 100


RECORDED = [   # dims, two rows per thread, float4 lanes per row, row blocks, target, round -> chunks, planes per chunk
    ((256, 256, 256), True, 64, 32, 32, 256, 8, 32),
    ((256, 256, 272), True, 64, 32, 32, 256, 8, 34),
    ((512, 512, 512), True, 128, 128, 80, 256, 6, 86),
    ((128, 128, 128), True, 32, 8, 32, 256, 32, 4),
    ((256, 256, 256), False, 64, 64, 32, 512, 8, 32),       # 512 blocks: two per CU
    ((512, 512, 512), False, 128, 256, 64, 512, 8, 64),
]


def test_recorded_configurations(geom):
    """the fp32 decompositions whose timings the comments of jacobi_sweep_pair and jacobi_sweep_lds quote"""
    for (ni, nj, nk), two_row, cw, row_blocks, target, rnd, nchunks, kc in RECORDED:
        assert int(geom("geom_pow2_lanes", [ni], 4, 0)[0]) == cw
        rows = 256 // cw * (2 if two_row else 1)
        assert (nj + rows - 1) // rows == row_blocks
        n = int(geom("geom_whole_round_chunks", [row_blocks], nk, target, rnd)[0])
        assert (n, (nk + n - 1) // n) == (nchunks, kc), (ni, nj, nk, two_row)
        assert (row_blocks * n) % rnd == 0

    # one block per CU, blocks of 8 rows, 256 CUs: 256^3 marches chunks of 32 planes, 192 planes land on the four-sweep rule's
    # threshold of 24, and 128^3 comes out at 8 planes, below it: the LDS kernels leave that grid to the two-row kernel
    def once(nj, nk):
        return int(geom("geom_once_per_cu_len", [nk], (nj + 7) // 8, 1, 256)[0])
    assert once(256, 256) == 32
    assert once(256, 192) == 24
    assert once(128, 128) == 8
