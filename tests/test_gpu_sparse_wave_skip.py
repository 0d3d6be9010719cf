"""FL_OPT_SKIP_EMPTY_TAPS on the GPU: the unstaggered accumulation as a launch that tests its own taps wave by wave -- option 1
against 0 with FL_OPT_SKIP_EMPTY_BRICKS = 2, against FL_OPT_SKIP_EMPTY_BRICKS = 0, on the raw bits of every output array, and
against the oracle as tests/test_gpu_ops.py compares; the wave counters against the numpy restatement of the criterion
(sparse_wave_case, pinned to the oracle by tests/test_sparse_wave_skip_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import fields as F
import sparse_case as S
import sparse_wave_case as W
from oracle_lib import fp, lib as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    yield lib
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 1)
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, 1)
    bq.check()


def dev(*arrays):
    from gpufluidsimulation_amd import DeviceBuffer
    return [DeviceBuffer.from_numpy(a) for a in arrays]


def ptrs(bufs):
    return [b.ptr for b in bufs]


def set_opts(hip, bricks, taps):
    import gpufluidsimulation_amd as bq
    hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, bricks)
    hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, taps)


def wave_stats(hip, reset=1):
    out = (C.c_longlong * 2)()
    hip.fl_sparse_wave_stats(out, reset)
    return int(out[0]), int(out[1])


def block_stats(hip):
    out = (C.c_longlong * 2)()
    hip.fl_sparse_stats_kind(2, out, 1)
    return int(out[0]), int(out[1])


def gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, coeffs, dback, dfwd, counts=None):
    """the three operators of the accumulation; counts (a dict): the waves (tested, skipped) of each call"""
    n = ni * nj * nk
    out = {}

    def note(name):
        if counts is not None:
            counts[name] = wave_stats(hip)

    wave_stats(hip)
    da, db = dev(a, b)
    t1, t2 = dev(d1, d2)
    hip.gpu_accumulate_field2(da.ptr, t1.ptr, coeffs[0], db.ptr, t2.ptr, coeffs[1], *ptrs(dback), h, ni, nj, nk, False)
    note("accumulate2")
    out["accumulate2"] = (t1.numpy(), t2.numpy())
    (t,) = dev(d1)                                  # both fields into one buffer: the second starts from what the first stored
    hip.gpu_accumulate_field2(da.ptr, t.ptr, coeffs[0], db.ptr, t.ptr, coeffs[1], *ptrs(dback), h, ni, nj, nk, False)
    note("accumulate2_shared")
    out["accumulate2_shared"] = (t.numpy(),)
    (t3,) = dev(d2)
    hip.gpu_accumulate_field(da.ptr, t3.ptr, *ptrs(dback), h, ni, nj, nk, False, coeffs[0])
    note("accumulate1")
    out["accumulate1"] = (t3.numpy(),)
    # the compensation: error stage through the forward map, then the accumulation of -0.5 err through the backward map
    u, du, us = dev(a, b, np.zeros(n, np.float32))
    hip.gpu_compensate_field(u.ptr, du.ptr, us.ptr, *ptrs(dfwd), *ptrs(dback), h, ni, nj, nk, False)
    note("compensate")
    out["compensate"] = (u.numpy(), du.numpy(), us.numpy())
    return out


def oracle_ops(ni, nj, nk, h, a, b, d1, d2, coeffs, back, fwd):
    n = ni * nj * nk
    o = oracle()
    out = {}
    t1, t2, t3, t4 = d1.copy(), d2.copy(), d2.copy(), d1.copy()
    o.orc_accumulate_field(fp(a), fp(t1), *map(fp, back), h, ni, nj, nk, 0, coeffs[0])
    o.orc_accumulate_field(fp(b), fp(t2), *map(fp, back), h, ni, nj, nk, 0, coeffs[1])
    o.orc_accumulate_field(fp(a), fp(t3), *map(fp, back), h, ni, nj, nk, 0, coeffs[0])
    o.orc_accumulate_field(fp(a), fp(t4), *map(fp, back), h, ni, nj, nk, 0, coeffs[0])
    o.orc_accumulate_field(fp(b), fp(t4), *map(fp, back), h, ni, nj, nk, 0, coeffs[1])
    out["accumulate2"], out["accumulate1"], out["accumulate2_shared"] = (t1, t2), (t3,), (t4,)
    u, du, us = a.copy(), b.copy(), np.zeros(n, np.float32)
    o.orc_compensate_field(fp(u), fp(du), fp(us), *map(fp, fwd), *map(fp, back), h, ni, nj, nk, 0)
    out["compensate"] = (u, du)
    return out


_REFERENCE = {}


def reference(ni, nj, nk, kind):
    """the maps and the tap cells of a (shape, map kind), computed once"""
    key = (ni, nj, nk, kind)
    if key not in _REFERENCE:
        back, fwd = W.maps_of(kind, ni, nj, nk, W.H, 1.1), S.maps_of("smooth", ni, nj, nk, W.H, 0.3)
        _REFERENCE[key] = (back, fwd, W.tap_cells(back, ni, nj, nk, W.H))
    return _REFERENCE[key]


@pytest.mark.parametrize("kind", W.MAP_KINDS)
@pytest.mark.parametrize("ni,nj,nk", W.SHAPES)
def test_wave_skip_changes_no_bit_and_matches_the_oracle(hip, ni, nj, nk, kind):
    h = W.H
    back, fwd, cells = reference(ni, nj, nk, kind)
    dback, dfwd = dev(*back), dev(*fwd)
    try:
        for n_case, case in enumerate(W.cases_for(ni, nj, nk)):
            coeffs = W.COEFFS[n_case % len(W.COEFFS)]
            a, b = W.sources(case, ni, nj, nk)
            d1, d2 = S.targets(ni, nj, nk, a, b)
            set_opts(hip, 0, 1)
            plain = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, coeffs, dback, dfwd)
            set_opts(hip, 2, 0)
            off = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, coeffs, dback, dfwd)
            assert wave_stats(hip) == (0, 0)
            set_opts(hip, 2, 1)
            block_stats(hip)
            counts = {}
            on = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, coeffs, dback, dfwd, counts)
            assert block_stats(hip) == (0, 0)           # the block classification takes no part in the accumulation
            print(case, kind, (ni, nj, nk), counts)
            for name in plain:
                for x, y, z in zip(plain[name], off[name], on[name]):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (case, name, "taps 0")
                    assert np.array_equal(x.view(np.uint32), z.view(np.uint32)), (case, name, "taps 1")
            ref = oracle_ops(ni, nj, nk, h, a, b, d1, d2, coeffs, back, fwd)
            for name in ref:
                for r, g in zip(ref[name], on[name]):
                    assert F.same(r, g), (case, name)
            # the counters: what the numpy restatement of the criterion predicts, wave for wave
            want2 = W.predict(back, [a, b], ni, nj, nk, h, cells)[:2]
            want1 = W.predict(back, [a], ni, nj, nk, h, cells)[:2]
            assert counts["accumulate2"] == want2, (case, counts, want2)
            assert counts["accumulate2_shared"] == want2, (case, counts, want2)
            assert counts["accumulate1"] == want1, (case, counts, want1)
            tested, skipped = counts["accumulate2"]
            if case == "zero":                          # (no flag is set, so not even a tap in a wrap cell keeps a wave)
                assert skipped == tested > 0 and counts["compensate"] == (tested, tested)
            elif case in ("dense", "empty_and_dense"):
                assert tested == 0
            elif kind == "smooth" and case in W.MIXED[(ni, nj, nk)]:
                assert 0 < skipped < tested, (case, counts)
    finally:
        set_opts(hip, 1, 1)


def test_what_takes_no_part(hip):
    """staggered launches, a plane window, point mode, the identity accumulate and FL_OPT_SKIP_EMPTY_BRICKS = 0, 3 and 4 never run
    the wave test; the default options do (and count nothing)"""
    ni, nj, nk = 24, 20, 16
    h = W.H
    back, fwd, _ = reference(ni, nj, nk, "smooth")
    dback = dev(*back)
    n, nu, nv, nw = F.sizes(ni, nj, nk)
    try:
        set_opts(hip, 2, 1)
        wave_stats(hip)
        zero = dev(*[np.zeros(c, np.float32) for c in (nu, nv, nw)])
        out = dev(*[np.zeros(c, np.float32) for c in (nu, nv, nw)])
        hip.gpu_accumulate_velocity(*ptrs(zero), *ptrs(out), *ptrs(dback), h, ni, nj, nk, False, -0.5)
        assert wave_stats(hip) == (0, 0)
        (za, zo) = dev(np.zeros(n, np.float32), np.zeros(n, np.float32))
        assert hip.fl_set_plane_window(2, nk - 3) == 1
        try:
            hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dback), h, ni, nj, nk, False, 2.0)
        finally:
            hip.fl_set_plane_window(-1, 0)
        assert wave_stats(hip) == (0, 0)
        hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dback), h, ni, nj, nk, True, 2.0)       # point mode
        assert wave_stats(hip) == (0, 0)
        for bricks in (0, 3, 4):
            set_opts(hip, bricks, 1)
            hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dback), h, ni, nj, nk, False, 2.0)
            assert wave_stats(hip) == (0, 0), bricks
        set_opts(hip, 2, 1)
        hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dback), h, ni, nj, nk, False, 2.0)
        tested, skipped = wave_stats(hip)
        assert tested == skipped > 0
        set_opts(hip, 1, 1)                             # the default: the same launch, nothing counted
        hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dback), h, ni, nj, nk, False, 2.0)
        assert wave_stats(hip) == (0, 0)
        assert not zo.numpy().any()
    finally:
        set_opts(hip, 1, 1)
