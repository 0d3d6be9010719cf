"""GPU parity of the additive entry points that only the host solver (csrc/host) and the z-slab path call, one by one:
gpu_max_abs3 / fl_nonfinite_seen, gpu_max_field, gpu_max_field_owned, gpu_map_travel_z, gpu_residual_norms, gpu_gradient_delta,
gpu_accumulate_component and the is_point instances of the nine-point operators, gpu_clamp_extrema_box_w, gpu_diffuse_sweeps,
fl_box_pack / fl_box_unpack / fl_box_copy and gpu_accumulate_wall_fixup.  The cases, their references (numpy where the
operation is exact, the oracle otherwise) and the checks live in tests/host_entry_case.py; tests/test_host_entry_points_cpu.py
runs the same cases on the CPU stand-in.  Bar: value equality; the summed residual norm alone keeps a relative 1e-6.
The slab cases run in one process without a communicator, where the library's all-reduce is a no-op."""
import pytest

import host_entry_case as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0, lib.fl_last_error_string()
    backend = H.Backend(lib, lambda on: lib.fl_set_option(H.OPT_FAST_LERP, on), "hip")
    yield backend
    backend.check()


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
