#!/usr/bin/env python3
"""How sparse density and temperature are in the headline scene, and what FL_OPT_SKIP_EMPTY_BRICKS makes of it.

Runs bench.py's workload (rising smoke, 200 Jacobi iterations, the full per-step sequence) on one GPU with the block counters
on (option value 4: all three operators take part; the default leaves the accumulation out) and prints, after steps 0, 20, 100
and 199, one JSON line with
    nonzero_nodes      share of the nodes of rho whose word is not 0x00000000 (T: the same test)
    occupied_bricks    share of the 8 x 8 x 8 bricks the flag pass marks for the pair (gpu_brick_flags)
    skipped / tested   blocks of that step's advection, error-stage and accumulation launch
With --waves the option value is 2: the accumulation runs in its wave-test form (FL_OPT_SKIP_EMPTY_TAPS) and its row holds the
WAVES tested and skipped (fl_sparse_wave_stats) instead of blocks.

    python tools/brick_occupancy.py [--n 256] [--jacobi-iters 200] [--waves]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--jacobi-iters", type=int, default=200)
    ap.add_argument("--report", type=int, nargs="*", default=[0, 20, 100, 199])
    ap.add_argument("--waves", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import DeviceBuffer
    from gpufluidsimulation_amd.scenes import rising_smoke
    from gpufluidsimulation_amd.solver import BimocqGPUSolver
    lib, n = bq.hip_lib(), a.n
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 2 if a.waves else 4)
    s = BimocqGPUSolver(n, n, n, 1.0, 0.0, 1.0)
    s.setSmoke(0.0, 1.0, rising_smoke(n, 1.0 / n))
    s.setProjection(a.jacobi_iters, 0.5)
    s.setOption(3, 1)
    out = (C.c_longlong * 2)()
    nb = (-(-n // 8)) ** 3
    for f in range(max(a.report) + 1):
        for kind in range(3):
            lib.fl_sparse_stats_kind(kind, out, 1)
        lib.fl_sparse_wave_stats(out, 1)
        s.advance(f, 2.0 / n)
        if f not in a.report:
            continue
        row = {"step": f}
        for kind, name in enumerate(("advect", "error", "accumulate")):
            lib.fl_sparse_stats_kind(kind, out, 1)
            row[name] = {"tested": int(out[0]), "skipped": int(out[1]), "ratio": round(out[1] / out[0], 4) if out[0] else None}
        if a.waves:
            lib.fl_sparse_wave_stats(out, 1)
            row["accumulate_waves"] = {"tested": int(out[0]), "skipped": int(out[1]), "ratio": round(out[1] / out[0], 4) if out[0] else None}
        rho, T = s.field("rho"), s.field("T")
        row["nonzero_nodes"] = {"rho": float((np.ascontiguousarray(rho).view(np.uint32) != 0).mean()),
                                "T": float((np.ascontiguousarray(T).view(np.uint32) != 0).mean())}
        d = [DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32).ravel()) for x in (rho, T)]
        flags = np.zeros(nb, np.uint8)
        assert lib.gpu_brick_flags(d[0].ptr, d[1].ptr, n, n, n, flags.ctypes.data, None) == nb
        row["occupied_bricks"] = float(flags.mean())
        print(json.dumps(row), flush=True)
    bq.check()
    s.close()


if __name__ == "__main__":
    main()
