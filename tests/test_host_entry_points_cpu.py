"""The cases of tests/test_gpu_host_entry_points.py run against the CPU stand-in of the C-ABI (tests/cpu_abi/oracle_abi.c): they
check the references and the case conditions of tests/host_entry_case.py on a machine without a GPU.  The stand-in has no
fl_nonfinite_seen and stores the kernel-selecting options without acting on them; everything else is asserted as on the GPU.

Also here: the rule by which fl_box_pack / fl_box_unpack / fl_box_copy cut a box list into launches (csrc/bq_box_chunk.h,
compiled behind tests/cpu_abi/box_chunk_shim.cpp)."""
import ctypes as C

import numpy as np
import pytest

import host_entry_case as H
from build_cpu_host import build as build_cpu_host, build_box_chunk


@pytest.fixture(scope="module")
def be():
    lib = H.bind(C.CDLL(build_cpu_host(), mode=C.RTLD_LOCAL))
    lib.orc_set_fast_lerp.restype, lib.orc_set_fast_lerp.argtypes = None, [C.c_int]
    backend = H.Backend(lib, lib.orc_set_fast_lerp, "cpu stand-in")
    yield backend
    backend.check()


# ---- the chunk rule of the box copies -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk():
    lib = C.CDLL(build_box_chunk(), mode=C.RTLD_LOCAL)
    I64P = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    lib.box_chunk_walk.restype = C.c_int
    lib.box_chunk_walk.argtypes = [np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS"), C.c_int, I64P, C.c_int, I64P, C.c_int]
    limit = lib.box_chunk_limit()

    def run(boxes):
        """-> (limit, chunks as rows of (first, next, n, elements), slots as rows of (x0, y0, z0, wx, wy, offset))"""
        a = np.ascontiguousarray(np.array(boxes, np.int32).reshape(-1, 6))
        ranges, slots = np.zeros((len(boxes) + 2, 4), np.int64), np.zeros((len(boxes) + 2, 6), np.int64)
        n = lib.box_chunk_walk(a if a.size else np.zeros((1, 6), np.int32), len(boxes), ranges, len(ranges), slots, len(slots))
        assert n >= 0, "the walk does not advance, or emits more chunks or slots than boxes"
        return limit, ranges[:n], slots
    return run


def chunk_rule_holds(walk, boxes):
    """every box consumed exactly once, in order, at most `limit` non-empty boxes per chunk, packed offsets without gaps"""
    limit, ranges, slots = walk(boxes)
    a = np.array(boxes, np.int64).reshape(-1, 6)
    vol = (a[:, 1] - a[:, 0]) * (a[:, 3] - a[:, 2]) * (a[:, 5] - a[:, 4])
    live = a[vol != 0]
    first, nxt, n, elements = ranges.T
    if not boxes:
        assert len(ranges) == 0
        return
    assert np.array_equal(first, np.concatenate([[0], nxt[:-1]])) and np.all(nxt > first), len(boxes)     # starts where the previous stopped
    assert (nxt[-1] if len(nxt) else 0) == len(boxes)
    assert np.all(n <= limit)
    live_before = np.concatenate([[0], np.cumsum(vol != 0)])
    assert np.array_equal(live_before[nxt] - live_before[first], n), len(boxes)       # the chunk holds the non-empty boxes of its range
    assert n.sum() == len(live), (len(boxes), n.sum(), len(live))                      # none twice, none missing
    want = np.stack([live[:, 0], live[:, 2], live[:, 4], live[:, 1] - live[:, 0], live[:, 3] - live[:, 2]], axis=1)
    assert np.array_equal(slots[:len(live), :5], want), len(boxes)                     # in order
    start = np.concatenate([[0], np.cumsum(vol[vol != 0])])                            # offsets restart with every chunk
    chunk_of = np.repeat(np.arange(len(n)), n)
    chunk_start = start[np.concatenate([[0], np.cumsum(n)])[:-1]] if len(n) else start[:0]
    assert np.array_equal(slots[:len(live), 5], start[:-1] - chunk_start[chunk_of]), len(boxes)
    assert np.array_equal(elements, start[np.cumsum(n)] - chunk_start), len(boxes)


def numbered(n, empty):
    """n boxes that can be told apart (box b starts at x0 = b), those whose index is in `empty` of zero volume"""
    return [(b, b + (0 if b in empty else 1 + b % 3), 0, 2, 5, 6 + b % 2) for b in range(n)]


def test_box_chunks_consume_every_box_once(walk):
    limit = walk([])[0]
    assert limit == 64
    for n in range(0, 201):
        chunk_rule_holds(walk, numbered(n, ()))
        for e in range(n):                                             # one empty box at every position
            chunk_rule_holds(walk, numbered(n, (e,)))
        chunk_rule_holds(walk, numbered(n, range(0, n, 2)))            # every other box
        chunk_rule_holds(walk, numbered(n, range(n)))                  # nothing but empty boxes
        chunk_rule_holds(walk, numbered(n, range(n // 3, 2 * n // 3)))   # a run of them across the chunk boundaries


def test_box_chunks_the_reported_list(walk):
    """more than 64 boxes with one empty box among the first 65: the first chunk takes box 64 as its 64th non-empty box, the
    second starts at box 65 -- not at box 64 again"""
    limit, ranges, slots = walk(numbered(66, (3,)))
    assert [tuple(r) for r in ranges[:, :3]] == [(0, 65, 64), (65, 66, 1)]
    assert slots[63][0] == 64 and slots[64][0] == 65


# ---- 1. reductions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", H.MAX_FIELD_COUNTS)
def test_max_field(be, count):
    H.run_max_field(be, count)


@pytest.mark.parametrize("ni,nj,nk,h", H.RED_GRIDS)
def test_max_abs3(be, ni, nj, nk, h):
    H.run_max_abs3(be, ni, nj, nk, h)


@pytest.mark.parametrize("ni,nj,nk,h", H.RED_GRIDS)
def test_max_field_owned(be, ni, nj, nk, h):
    H.run_max_field_owned(be, ni, nj, nk)


@pytest.mark.parametrize("ranks", [2, 3])
def test_reductions_on_slab_ranks(be, ranks):
    H.run_slab_reductions(be, ranks)


@pytest.mark.parametrize("ni,nj,nk,h", H.RED_GRIDS)
def test_map_travel_z(be, ni, nj, nk, h):
    H.run_map_travel(be, ni, nj, nk, h)


@pytest.mark.parametrize("ranks", [2, 3])
def test_map_travel_z_on_slab_ranks(be, ranks):
    H.run_map_travel_slab(be, ranks)


@pytest.mark.parametrize("ni,nj,nk", H.RESIDUAL_GRIDS)
def test_residual_norms(be, ni, nj, nk):
    H.run_residual_norms(be, ni, nj, nk)


# ---- 2. gpu_gradient_delta ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni,nj,nk", H.GRADIENT_GRIDS)
def test_gradient_delta(be, ni, nj, nk):
    H.run_gradient_delta(be, ni, nj, nk)


def test_gradient_delta_on_slab_ranks(be):
    H.run_gradient_delta_slab(be)


# ---- 3. gpu_accumulate_component, point sampling -----------------------------------------------------------------------------
@pytest.mark.parametrize("ni,nj,nk,h", H.GATHER_GRIDS)
@pytest.mark.parametrize("kind", ["warped", "wild"])
def test_accumulate_component(be, ni, nj, nk, h, kind):
    H.run_accumulate_component(be, ni, nj, nk, h, kind)


@pytest.mark.parametrize("ni,nj,nk,h", H.GATHER_GRIDS[:2])
@pytest.mark.parametrize("kind", ["warped", "wild"])
@pytest.mark.parametrize("fast", [0, 1])
def test_point_sampling_instances(be, ni, nj, nk, h, kind, fast):
    H.run_point_sampling(be, ni, nj, nk, h, kind, fast)


# ---- 4. gpu_clamp_extrema_box_w, gpu_diffuse_sweeps --------------------------------------------------------------------------
@pytest.mark.parametrize("nx", H.CLAMP_ROWS)
@pytest.mark.parametrize("ny,nz", H.CLAMP_PLANES)
def test_clamp_extrema_box_w(be, nx, ny, nz):
    H.run_clamp_box_w(be, nx, ny, nz)


@pytest.mark.parametrize("nx", [33, 260])
def test_clamp_extrema_box_w_thinnest_buffers(be, nx):
    nz = H.thinnest_clamped_buffer(nx, 6)
    H.run_clamp_box_w(be, nx, 6, nz)
    H.run_clamp_box_w(be, nx, 6, nz - 1, writes=False)


@pytest.mark.parametrize("ni,nj,nk", H.DIFFUSE_DIMS)
def test_diffuse_sweeps(be, ni, nj, nk):
    H.run_diffuse_sweeps(be, ni, nj, nk)


# ---- 5. box copies -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("koff", [0, 5])
@pytest.mark.parametrize("name", sorted(H.box_lists(0, H.NKF)))
def test_box_lists(be, koff, name):
    H.run_box_lists(be, koff, name)


@pytest.mark.parametrize("koff", [0, 5])
def test_box_refusals(be, koff):
    H.run_box_refusals(be, koff)


# ---- 6. gpu_accumulate_wall_fixup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,structured,kind", [(1.0 / 32, 1, "wild"), (1.0 / 32, 0, "wild"), (1.0 / 24, 1, "warped")])
def test_wall_fixup(be, h, structured, kind):
    H.run_wall_fixup(be, h, structured, kind)


@pytest.mark.parametrize("h", [1.0 / 32, 1.0 / 24])
def test_wall_fixup_on_slab_ranks(be, h):
    H.run_wall_fixup_slab(be, h)
