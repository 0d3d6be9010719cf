"""FL_OPT_SKIP_EMPTY_BRICKS on the GPU: the unstaggered nine-point operators with the skip -- option 1, the default (advection
and error stage), and option 4 (the accumulation too, counting) -- against the same build without it (option 0) on the raw bits
of every output array, and against the oracle as tests/test_gpu_ops.py compares; the block counters; the flag pass against
numpy."""
import ctypes as C

import numpy as np
import pytest

import fields as F
import sparse_case as S
from oracle_lib import fp, lib as oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import gpufluidsimulation_amd as bq
    lib = bq.hip_lib()
    assert lib.fl_init(0) == 0
    yield lib
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 1)
    lib.fl_set_option(bq._lib.FL_OPT_FAST_LERP, 0)
    lib.fl_set_option(bq._lib.FL_OPT_FIELD_WINDOW, -1)
    bq.check()


def dev(*arrays):
    from gpufluidsimulation_amd import DeviceBuffer
    return [DeviceBuffer.from_numpy(a) for a in arrays]


def ptrs(bufs):
    return [b.ptr for b in bufs]


def set_skip(hip, v):
    import gpufluidsimulation_amd as bq
    hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, v)


def stats(hip, reset=1):
    out = (C.c_longlong * 2)()
    hip.fl_sparse_stats(out, reset)
    return int(out[0]), int(out[1])


COEFF = (-0.5, 2.0)


def kind_stats(hip, kind):
    out = (C.c_longlong * 2)()
    hip.fl_sparse_stats_kind(kind, out, 0)
    return int(out[0]), int(out[1])


def gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd, counts=None):
    """every operator of the issue, two fields and one; returns the output arrays by name.  counts (a dict): gets the blocks
    (tested, skipped) that the accumulation of two fields into ONE buffer added to the accumulation's counters"""
    n = ni * nj * nk
    out = {}
    da, db = dev(a, b)
    o1, o2 = dev(np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32))
    hip.gpu_advect_field2(o1.ptr, da.ptr, o2.ptr, db.ptr, *ptrs(dback), h, ni, nj, nk, False)
    out["advect2"] = (o1.numpy(), o2.numpy())
    (o3,) = dev(np.full(n, 7.0, np.float32))
    hip.gpu_advect_field(o3.ptr, da.ptr, *ptrs(dback), h, ni, nj, nk, False)
    out["advect1"] = (o3.numpy(),)
    i1, i2, e1, e2 = dev(d1, d2, np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32))
    hip.gpu_compensate_error_field2(da.ptr, i1.ptr, e1.ptr, db.ptr, i2.ptr, e2.ptr, *ptrs(dfwd), h, ni, nj, nk, False)
    out["error2"] = (e1.numpy(), e2.numpy(), i1.numpy(), i2.numpy())
    i3, e3 = dev(d2, np.full(n, 7.0, np.float32))
    hip.gpu_compensate_error_field(db.ptr, i3.ptr, e3.ptr, *ptrs(dfwd), h, ni, nj, nk, False)
    out["error1"] = (e3.numpy(), i3.numpy())
    t1, t2 = dev(d1, d2)
    hip.gpu_accumulate_field2(da.ptr, t1.ptr, COEFF[0], db.ptr, t2.ptr, COEFF[1], *ptrs(dback), h, ni, nj, nk, False)
    out["accumulate2"] = (t1.numpy(), t2.numpy())
    (t3,) = dev(d1)
    hip.gpu_accumulate_field(db.ptr, t3.ptr, *ptrs(dback), h, ni, nj, nk, False, COEFF[1])
    out["accumulate1"] = (t3.numpy(),)
    (t,) = dev(d1)                                  # both fields into one buffer: the second starts from what the first stored
    before = kind_stats(hip, 2)
    hip.gpu_accumulate_field2(da.ptr, t.ptr, COEFF[0], db.ptr, t.ptr, COEFF[1], *ptrs(dback), h, ni, nj, nk, False)
    if counts is not None:
        counts["accumulate2_shared"] = tuple(x - y for x, y in zip(kind_stats(hip, 2), before))
    out["accumulate2_shared"] = (t.numpy(),)
    return out


def oracle_ops(ni, nj, nk, h, a, b, d1, d2, back, fwd):
    n = ni * nj * nk
    o = oracle()
    out = {}
    o1, o2 = np.zeros(n, np.float32), np.zeros(n, np.float32)       # (the operator leaves the nodes outside its window alone)
    o.orc_advect_field(fp(o1), fp(a), *map(fp, back), h, ni, nj, nk, 0)
    o.orc_advect_field(fp(o2), fp(b), *map(fp, back), h, ni, nj, nk, 0)
    out["advect2"], out["advect1"] = (o1, o2), (o1,)
    e1, e2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    o.orc_compensate_error_field(fp(a), fp(d1.copy()), fp(e1), *map(fp, fwd), h, ni, nj, nk, 0)
    o.orc_compensate_error_field(fp(b), fp(d2.copy()), fp(e2), *map(fp, fwd), h, ni, nj, nk, 0)
    out["error2"], out["error1"] = (e1, e2), (e2,)
    t1, t2, t3 = d1.copy(), d2.copy(), d1.copy()
    o.orc_accumulate_field(fp(a), fp(t1), *map(fp, back), h, ni, nj, nk, 0, COEFF[0])
    o.orc_accumulate_field(fp(b), fp(t2), *map(fp, back), h, ni, nj, nk, 0, COEFF[1])
    o.orc_accumulate_field(fp(b), fp(t3), *map(fp, back), h, ni, nj, nk, 0, COEFF[1])
    out["accumulate2"], out["accumulate1"] = (t1, t2), (t3,)
    t4 = d1.copy()
    o.orc_accumulate_field(fp(a), fp(t4), *map(fp, back), h, ni, nj, nk, 0, COEFF[0])
    o.orc_accumulate_field(fp(b), fp(t4), *map(fp, back), h, ni, nj, nk, 0, COEFF[1])
    out["accumulate2_shared"] = (t4,)
    return out


def window_mask(ni, nj, nk, win):
    m = np.zeros((nk, nj, ni), bool)
    m[win + 1:nk - 1 - win, win + 1:nj - 1 - win, win + 1:ni - 1 - win] = True
    return m.ravel()


@pytest.mark.parametrize("kind", ["smooth", "wild", "jump"])
@pytest.mark.parametrize("ni,nj,nk", S.SHAPES)
def test_skip_changes_no_bit_and_matches_the_oracle(hip, ni, nj, nk, kind):
    h = S.H
    back, fwd = S.maps_of(kind, ni, nj, nk, h, 1.1), S.maps_of(kind, ni, nj, nk, h, 0.3)
    dback, dfwd = dev(*back), dev(*fwd)
    skipped_somewhere = 0
    for case in S.CASES:
        a, b = S.sources(case, ni, nj, nk)
        d1, d2 = S.targets(ni, nj, nk, a, b)
        set_skip(hip, 0)
        plain = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
        set_skip(hip, 1)
        default = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
        stats(hip)
        set_skip(hip, 4)
        counts = {}
        skip = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd, counts)
        tested, skipped = stats(hip)
        set_skip(hip, 1)
        if case == "zero" and kind == "smooth":     # every brick empty, every map tile finite: the shared-buffer stores are the skip's
            assert counts["accumulate2_shared"][1] > 0, counts
        for name in plain:
            for x, y, z in zip(plain[name], default[name], skip[name]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (case, name, 1)
                assert np.array_equal(x.view(np.uint32), z.view(np.uint32)), (case, name, 4)
        ref = oracle_ops(ni, nj, nk, h, a, b, d1, d2, back, fwd)
        for name, win in (("advect2", 2), ("advect1", 2), ("error2", 1), ("error1", 1), ("accumulate2", 1), ("accumulate1", 1),
                          ("accumulate2_shared", 1)):
            inside = window_mask(ni, nj, nk, win)
            for r, g in zip(ref[name], skip[name]):
                if name.startswith("accumulate"):
                    assert F.same(r, g), (case, name)
                else:                                   # (outside the window the GPU buffers keep their 7.0f filling)
                    assert F.same(r[inside], g[inside]), (case, name)
        if case == "dense":
            assert skipped == 0, (case, tested, skipped)        # (the flag pass finds no empty brick: nothing is even tested)
        elif case == "zero":
            assert tested > 0 and (skipped > 0 or kind == "wild"), (case, tested, skipped)
        skipped_somewhere += skipped
    assert skipped_somewhere > 0 or kind == "wild"      # (most tiles of the wild maps hold a NaN or an Inf: no bound, no skip)


@pytest.mark.parametrize("ni,nj,nk", S.SHAPES)
def test_counters(hip, ni, nj, nk):
    """option 4: skipped = 0 for a dense field, 0 < skipped < tested for a blob, skipped > 0 for the all-zero case, and nothing
    tested at all by a staggered launch or under a plane window; option 2: the accumulation takes no part"""
    h = S.H
    back, fwd = S.maps_of("smooth", ni, nj, nk, h, 1.1), S.maps_of("smooth", ni, nj, nk, h, 0.3)
    dback, dfwd = dev(*back), dev(*fwd)
    try:
        set_skip(hip, 2)
        a, b = S.sources("zero", ni, nj, nk)
        d1, d2 = S.targets(ni, nj, nk, a, b)
        stats(hip)
        gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
        per_kind = []
        for kind in range(3):
            out = (C.c_longlong * 2)()
            hip.fl_sparse_stats_kind(kind, out, 1)
            per_kind.append((int(out[0]), int(out[1])))
        assert per_kind[0][1] > 0 and per_kind[1][1] > 0 and per_kind[2] == (0, 0), per_kind
        set_skip(hip, 4)
        seen = {}
        for case in ("dense", "blob_inside", "zero"):
            a, b = S.sources(case, ni, nj, nk)
            d1, d2 = S.targets(ni, nj, nk, a, b)
            stats(hip)
            gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
            seen[case] = stats(hip)
        assert seen["dense"][1] == 0, seen
        assert 0 < seen["blob_inside"][1] < seen["blob_inside"][0], seen
        assert seen["zero"][1] > 0, seen
        # staggered: the three velocity components, all zero
        n, nu, nv, nw = F.sizes(ni, nj, nk)
        zero = dev(*[np.zeros(c, np.float32) for c in (nu, nv, nw)])
        out = dev(*[np.zeros(c, np.float32) for c in (nu, nv, nw)])
        hip.gpu_advect_velocity(*ptrs(out), *ptrs(zero), *ptrs(dback), h, ni, nj, nk, False)
        hip.gpu_accumulate_velocity(*ptrs(zero), *ptrs(out), *ptrs(dfwd), h, ni, nj, nk, False, -0.5)
        assert stats(hip) == (0, 0)
        # a plane window
        (za, zo) = dev(np.zeros(n, np.float32), np.zeros(n, np.float32))
        assert hip.fl_set_plane_window(2, nk - 3) == 1
        try:
            hip.gpu_advect_field(zo.ptr, za.ptr, *ptrs(dback), h, ni, nj, nk, False)
            hip.gpu_accumulate_field(za.ptr, zo.ptr, *ptrs(dfwd), h, ni, nj, nk, False, 2.0)
        finally:
            hip.fl_set_plane_window(-1, 0)
        assert stats(hip) == (0, 0)
    finally:
        set_skip(hip, 1)


@pytest.mark.parametrize("ni,nj,nk", S.SHAPES[1:])
def test_fast_lerp_twin_without_the_field_window(hip, ni, nj, nk):
    """FL_OPT_FAST_LERP = 1 with FL_OPT_FIELD_WINDOW = 0: the one-fma build of the same one-plane kernels -- options 1 and 4
    against option 0 on the raw bits, and against the oracle in the same mode"""
    import gpufluidsimulation_amd as bq
    h = S.H
    hip.fl_set_option(bq._lib.FL_OPT_FAST_LERP, 1)
    hip.fl_set_option(bq._lib.FL_OPT_FIELD_WINDOW, 0)
    try:
        for kind in ("smooth", "wild"):
            back, fwd = S.maps_of(kind, ni, nj, nk, h, 1.1), S.maps_of(kind, ni, nj, nk, h, 0.3)
            dback, dfwd = dev(*back), dev(*fwd)
            for case in ("blob_face", "specials", "zero"):
                a, b = S.sources(case, ni, nj, nk)
                d1, d2 = S.targets(ni, nj, nk, a, b)
                set_skip(hip, 0)
                plain = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
                set_skip(hip, 1)
                default = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
                set_skip(hip, 4)
                stats(hip)
                skip = gpu_ops(hip, ni, nj, nk, h, a, b, d1, d2, dback, dfwd)
                tested, skipped = stats(hip)
                assert tested > 0 and (skipped > 0 or kind == "wild"), (kind, case, tested, skipped)
                for name in plain:
                    for x, y, z in zip(plain[name], default[name], skip[name]):
                        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (kind, case, name, 1)
                        assert np.array_equal(x.view(np.uint32), z.view(np.uint32)), (kind, case, name, 4)
                oracle().orc_set_fast_lerp(1)
                try:
                    ref = oracle_ops(ni, nj, nk, h, a, b, d1, d2, back, fwd)
                finally:
                    oracle().orc_set_fast_lerp(0)
                for r, g in zip(ref["accumulate2"], skip["accumulate2"]):
                    assert F.same(r, g), (kind, case)
    finally:
        set_skip(hip, 1)
        hip.fl_set_option(bq._lib.FL_OPT_FAST_LERP, 0)
        hip.fl_set_option(bq._lib.FL_OPT_FIELD_WINDOW, -1)


@pytest.mark.parametrize("ni,nj,nk", S.SHAPES + [(70, 9, 17)])
def test_flag_pass_against_numpy(hip, ni, nj, nk):
    nb = -(-ni // 8) * -(-nj // 8) * -(-nk // 8)
    for case in S.CASES:
        a, b = S.sources(case, ni, nj, nk) if (ni, nj, nk) in S.SHAPES else S.sources("dense" if case == "dense" else "zero", ni, nj, nk)
        if (ni, nj, nk) not in S.SHAPES and case == "node777":
            a[(ni * nj * nk) - 1] = -0.0                      # the very last word, in three partial bricks at once
        da, db = dev(a, b)
        for pair in (True, False):
            want = S.brick_flags([a, b] if pair else [a], ni, nj, nk).ravel()
            got = np.full(nb + 8, 0xAA, np.uint8)
            empty = C.c_int(-1)
            cnt = hip.gpu_brick_flags(da.ptr, db.ptr if pair else None, ni, nj, nk, got.ctypes.data, C.byref(empty))
            assert cnt == nb
            assert np.array_equal(got[:nb], want), (case, pair)
            assert (got[nb:] == 0xAA).all()
            assert empty.value == int((want == 0).any()), (case, pair)
