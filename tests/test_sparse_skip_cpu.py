"""FL_OPT_SKIP_EMPTY_BRICKS, the claim itself, without a GPU: a numpy restatement of the criterion (sparse_case.block_skips:
tile range -> clamp -> cells -> widened brick range) is checked against the ORACLE's operators.  Every node of a block the
criterion would skip must hold, bit for bit, what the operator's stores give with every gather result taken as +0.0f.
This pins the claim, not the HIP code (tests/test_gpu_sparse_scalars.py does that)."""
import numpy as np
import pytest

import sparse_case as S
from oracle_lib import fp, lib as oracle

GRIDS = [(32, 32, 32), (24, 20, 16)]


def bits(a):
    return a.view(np.uint32)


def window_nodes(key, ni, nj, nk, win):
    bx, by, k = key
    return [(k, j, i) for j in range(by * 4, min(by * 4 + 4, nj)) if win < j < nj - 1 - win
            for i in range(bx * 64, min(bx * 64 + 64, ni)) if win < i < ni - 1 - win]


def sources_for(kind, ni, nj, nk):
    """smooth maps: a blob in the middle.  Wild maps throw taps all over the grid (and most tiles hold a NaN), so the only
    blocks that can be skipped are those of a field that is empty wherever their widened range reaches: a blob confined to the
    last brick along y, which the ranges of the blocks on the first rows do not reach."""
    if kind == "smooth":
        return S.sources("blob_inside", ni, nj, nk)
    a = np.zeros((nk, nj, ni), np.float32)
    a[:, 8 * ((nj - 1) // 8):, :] = 1.25
    return np.ascontiguousarray(a.ravel()), np.zeros(ni * nj * nk, np.float32)


@pytest.mark.parametrize("kind", ["smooth", "wild"])
@pytest.mark.parametrize("ni,nj,nk", GRIDS)
def test_skipped_blocks_hold_the_zero_gather_value_in_the_oracle(ni, nj, nk, kind):
    h = S.H
    n = ni * nj * nk
    f32 = np.float32
    back, fwd = S.maps_of(kind, ni, nj, nk, h, 1.1), S.maps_of(kind, ni, nj, nk, h, 0.3)
    a, b = sources_for(kind, ni, nj, nk)
    flags = S.brick_flags([a, b], ni, nj, nk)
    lo_adv, hi_adv = [f32(h)] * 3, [f32(f32(h) * f32(d) - f32(h)) for d in (ni, nj, nk)]
    lo_acc, hi_acc = [f32(0)] * 3, [f32(f32(h) * f32(d)) for d in (ni, nj, nk)]
    d1, d2 = S.targets(ni, nj, nk, a, b)

    def check(name, maps, win, lo, hi, outs, expect):
        skips = S.block_skips(maps, flags, ni, nj, nk, h, win, lo, hi)
        assert any(skips.values()), (name, "no block skipped")
        assert not all(skips.values()), (name, "every block skipped")
        for key, sk in skips.items():
            if not sk:
                continue
            idx = np.array([i + ni * (j + nj * k) for (k, j, i) in window_nodes(key, ni, nj, nk, win)])
            for o, e in zip(outs, expect):
                assert np.array_equal(bits(o)[idx], bits(e)[idx]), (name, key)

    # advection: 0.5f * (+0) + 0.5f * (+0)
    oa, ob = np.full(n, 7.0, f32), np.full(n, 7.0, f32)
    oracle().orc_advect_field(fp(oa), fp(a.copy()), *map(fp, back), h, ni, nj, nk, 0)
    oracle().orc_advect_field(fp(ob), fp(b.copy()), *map(fp, back), h, ni, nj, nk, 0)
    check("advect", back, 2, lo_adv, hi_adv, (oa, ob), (np.zeros(n, f32), np.zeros(n, f32)))
    # error stage: (float)(0.5 * 0 + 0.5 * 0) - init
    ea, eb = np.full(n, 7.0, f32), np.full(n, 7.0, f32)
    oracle().orc_compensate_error_field(fp(a.copy()), fp(d1.copy()), fp(ea), *map(fp, fwd), h, ni, nj, nk, 0)
    oracle().orc_compensate_error_field(fp(b.copy()), fp(d2.copy()), fp(eb), *map(fp, fwd), h, ni, nj, nk, 0)
    with np.errstate(invalid="ignore"):
        check("compensate", fwd, 1, lo_acc, hi_acc, (ea, eb), (f32(0) - d1, f32(0) - d2))
    # accumulation, both signs of the coefficient: dst + (float)(0.5 * (+0) + 0.5 * (coeff * (+0)))
    for coeff in (-0.5, 2.0):
        ra, rb = d1.copy(), d2.copy()
        oracle().orc_accumulate_field(fp(a.copy()), fp(ra), *map(fp, back), h, ni, nj, nk, 0, coeff)
        oracle().orc_accumulate_field(fp(b.copy()), fp(rb), *map(fp, back), h, ni, nj, nk, 0, coeff)
        with np.errstate(invalid="ignore"):
            check("accumulate", back, 1, lo_acc, hi_acc, (ra, rb), (d1 + f32(0), d2 + f32(0)))


def test_brick_flags_count_every_word_that_is_not_zero():
    ni, nj, nk = 24, 20, 16
    a, b = S.sources("specials", ni, nj, nk)
    fl = S.brick_flags([a, b], ni, nj, nk)
    assert fl.shape == (2, 3, 3)
    # -0.0f at (k, j, i) = (3, 4, 5), a denormal at (9, 10, 11), NaN at (4, 12, 14), Inf at (12, 5, 20)
    assert fl[0, 0, 0] and fl[1, 1, 1] and fl[0, 1, 1] and fl[1, 0, 2] and fl.sum() == 4
