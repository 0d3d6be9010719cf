"""FL_OPT_SKIP_EMPTY_TAPS, the claim itself, without a GPU: a numpy restatement of the per-lane criterion (sparse_wave_case:
clamped tap -> cell -> cell flag, with the wrap and upper-end rules) is checked against the ORACLE's accumulation.  Every node
of a wave the criterion skips must hold, on the raw bits, what the operator's stores give with every gather result taken as
+0.0f.  Separately the cell-flag rule is checked against brute force over the eight flat-indexed corner words of every cell.
This pins the claim and the counts the GPU test expects, not the HIP code (tests/test_gpu_sparse_wave_skip.py does that).

The comparison with the oracle is on the raw bits except that a NaN equals any NaN: which NaN an operation returns (sign,
payload) is the processor's choice -- x86 here, the GPU there -- and no part of the arithmetic contract.  The +Inf coefficient and
the NaN nodes of dst are therefore checked for "is a NaN in the same place"; the GPU test compares GPU against GPU on all 32 bits."""
import numpy as np
import pytest

import sparse_case as S
import sparse_wave_case as W
from oracle_lib import fp, lib as oracle

F32 = np.float32
GRIDS = [(24, 20, 16), (64, 8, 8), (32, 32, 32), (80, 24, 16)]      # the last: a row is a full wave and a 16-lane wave


def bits(a):
    return a.view(np.uint32)


def same_bits(a, b):
    """the raw bits, except that a NaN equals a NaN: which NaN an operation returns is the processor's choice, not the contract's"""
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def zero_gather_result(dst, coeff):
    """dst + (float)(0.5 * sum + 0.5 * (coeff * 0)) with sum = eight times (0.125f * coeff) * (+0) added to +0"""
    with np.errstate(invalid="ignore"):
        w = F32(F32(0.125) * F32(coeff))
        s = F32(0)
        for _ in range(8):
            s = F32(s + F32(w * F32(0)))
        r = F32(0.5 * np.float64(s) + 0.5 * np.float64(F32(F32(coeff) * F32(0))))
        return (dst + r).astype(F32)


@pytest.mark.parametrize("kind", W.MAP_KINDS)
@pytest.mark.parametrize("ni,nj,nk", GRIDS)
def test_skipped_waves_hold_the_zero_gather_value_in_the_oracle(ni, nj, nk, kind):
    h = W.H
    maps = W.maps_of(kind, ni, nj, nk, h, 1.1)
    cells = W.tap_cells(maps, ni, nj, nk, h)
    for c, d in zip(cells, (ni, nj, nk)):       # the clamp bounds every base index by [0, n]: the cell-flag array covers it
        assert c.min() >= 0 and c.max() <= d
    seen_skip = seen_keep = 0
    for case in W.cases_for(ni, nj, nk):
        a, b = W.sources(case, ni, nj, nk)
        tested, skipped, skips = W.predict(maps, [a, b], ni, nj, nk, h, cells)
        if case == "dense" or case == "empty_and_dense":
            assert tested == 0, (case, tested)           # the pass word says: no empty brick
            continue
        assert tested > 0
        seen_skip += skipped
        seen_keep += tested - skipped
        d1, d2 = S.targets(ni, nj, nk, a, b)
        for coeff in (-0.5, 1.0, float("inf")):
            ra, rb = d1.copy(), d2.copy()
            oracle().orc_accumulate_field(fp(a.copy()), fp(ra), *map(fp, maps), h, ni, nj, nk, 0, coeff)
            oracle().orc_accumulate_field(fp(b.copy()), fp(rb), *map(fp, maps), h, ni, nj, nk, 0, coeff)
            ea, eb = zero_gather_result(d1, coeff), zero_gather_result(d2, coeff)
            idx = np.array([n for key, sk in skips.items() if sk for n in W.wave_nodes(key, ni, nj, nk)], np.int64)
            if idx.size:
                assert same_bits(ra[idx], ea[idx]), (case, coeff)
                assert same_bits(rb[idx], eb[idx]), (case, coeff)
    assert seen_skip > 0 and seen_keep > 0, (seen_skip, seen_keep)


@pytest.mark.parametrize("ni,nj,nk", W.SHAPES)
def test_what_the_gpu_test_expects_of_its_cases(ni, nj, nk):
    """the inequalities tests/test_gpu_sparse_wave_skip.py asserts from the counters, predicted here from numpy alone: all-zero
    sources under a map that reaches no wrap cell skip every wave; a dense pair tests none; every mixed case (sparse_wave_case.MIXED)
    skips some waves and keeps some"""
    h = W.H
    maps = W.maps_of("smooth", ni, nj, nk, h, 1.1)
    cells = W.tap_cells(maps, ni, nj, nk, h)
    assert cells[0].max() < ni and cells[1].max() < nj and cells[2].max() < nk        # no tap in a wrap cell (base index n)
    for case in W.cases_for(ni, nj, nk):
        tested, skipped, _ = W.predict(maps, list(W.sources(case, ni, nj, nk)), ni, nj, nk, h, cells)
        if case == "zero":
            assert skipped == tested > 0
        elif case in ("dense", "empty_and_dense"):
            assert tested == 0
        elif case in W.MIXED[(ni, nj, nk)]:
            assert 0 < skipped < tested, (case, skipped, tested)


@pytest.mark.parametrize("ni,nj,nk", W.SHAPES + [(70, 9, 17), (8, 8, 8)])
def test_cell_flags_cover_every_corner_word(ni, nj, nk):
    """the rule (brick flags of the brick, its +1 neighbours, the wrapped row / plane at the upper ends) against brute force over
    the eight corner words of every cell with base indices 0 .. n on every axis: a clear flag means every word is zero"""
    for case in W.CASES:
        if (ni, nj, nk) in W.SHAPES[:3]:
            a, b = W.sources(case, ni, nj, nk)
        else:
            a, b = W.sources("high_end" if case != "dense" else "dense", ni, nj, nk)
            if case == "node777":
                a = a.copy(); a[ni * nj * nk - 1] = -0.0
            elif case == "node888":
                a = np.zeros_like(a); b = np.zeros_like(b); a[ni - 1] = 1.0; b[ni * nj - 1] = 1.0     # the ends of the first row and plane
        for fields in ([a, b], [a], [b]):
            rule = W.cell_flags(S.brick_flags(fields, ni, nj, nk), ni, nj, nk)
            exact = W.cell_flags_brute(fields, ni, nj, nk)
            assert rule.shape == exact.shape == ((nk >> 3) + 1, (nj >> 3) + 1, (ni >> 3) + 1)
            assert not (exact & (rule == 0)).any(), (case, np.argwhere(exact & (rule == 0))[:4])
    # ... and it is not vacuous: an all-zero pair clears every flag
    zero = np.zeros(ni * nj * nk, F32)
    assert not W.cell_flags(S.brick_flags([zero], ni, nj, nk), ni, nj, nk).any()
    one = zero.copy()
    one[0] = 1.0
    assert W.cell_flags(S.brick_flags([one], ni, nj, nk), ni, nj, nk)[0, 0, 0] == 1
