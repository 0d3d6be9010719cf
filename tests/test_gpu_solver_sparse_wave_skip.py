"""FL_OPT_SKIP_EMPTY_TAPS through the whole step: 6 steps of 32^3 rising smoke, two solvers advanced side by side -- the
accumulation without the wave test (option 0) and with it (option 1), FL_OPT_SKIP_EMPTY_BRICKS = 2 so that the waves are counted
-- the raw bits of rho, T, u, v, w, p agree after every step, under both re-initialisation policies and with the full per-step
sequence on and off; waves really were skipped, and there is smoke."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BQ_OPT_REINIT_POLICY, BQ_OPT_FULL_STATE = 2, 3


@pytest.mark.parametrize("full_state", [0, 1])
@pytest.mark.parametrize("policy", [0, 1])
def test_six_steps_with_and_without_the_wave_test(policy, full_state):
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    hip = bq.hip_lib()
    n = 32
    em = [(0.5, 0.2, 0.5, 0.1, 1.0, 1.0, 0.0, 1)]
    solvers = []
    for _ in range(2):
        s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0)
        s.setSmoke(0.0, 1.0, em)
        s.setProjection(40, 0.5)
        s.setOption(BQ_OPT_REINIT_POLICY, policy)
        s.setOption(BQ_OPT_FULL_STATE, full_state)
        solvers.append(s)
    out = (C.c_longlong * 2)()
    hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 2)
    hip.fl_sparse_wave_stats(out, 1)
    try:
        for f in range(6):
            for s, opt in zip(solvers, (0, 1)):
                hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, opt)
                s.advance(f, 2.0 / n)
            for name in ("rho", "T", "u", "v", "w", "p"):
                a = np.ascontiguousarray(solvers[0].field(name)).view(np.uint32)
                b = np.ascontiguousarray(solvers[1].field(name)).view(np.uint32)
                assert np.array_equal(a, b), (f, name)
        assert float(np.abs(solvers[1].field("rho")).max()) > 0.5      # (there is smoke)
        hip.fl_sparse_wave_stats(out, 1)
        print("waves tested, skipped:", out[0], out[1])
        assert 0 < out[1] < out[0], (out[0], out[1])
    finally:
        hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 1)
        hip.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, 1)
        for s in solvers:
            s.close()
    bq.check()
