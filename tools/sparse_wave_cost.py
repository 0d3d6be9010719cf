#!/usr/bin/env python3
"""FL_OPT_SKIP_EMPTY_TAPS on its worst and best case, by the method of tools/sparse_dense_cost.py: gpu_accumulate_field2 at n^3 on a
pair with no zero word and on an all-zero pair, option 25 = 1 against 0 in one process (alternating, events on the compute stream,
FL_OPT_SKIP_EMPTY_BRICKS at its default).  On the dense pair the option should cost the flag pass, the cell-flag pass and one
launch that returns at once, and nothing inside the operator's kernel; the rows of those kernels are in
`rocprofv3 --kernel-trace --stats -- python tools/sparse_wave_cost.py`.

    python tools/sparse_wave_cost.py [--n 256] [--reps 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import DeviceBuffer
    import fields as F
    lib, n = bq.hip_lib(), a.n
    h = float(np.float32(1.0 / n))
    dev = lambda x: DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32))
    back = [dev(m) for m in F.warped_maps(n, n, n, h, -0.7, 1.1)]
    pairs = {"dense": [dev(F.scalar(n, n, n, 0.4) + np.float32(2.0)), dev(F.scalar(n, n, n, 1.9) - np.float32(3.0))],
             "all-zero": [dev(np.zeros(n ** 3, np.float32)) for _ in range(2)]}
    o = [dev(np.zeros(n ** 3, np.float32)) for _ in range(2)]
    P = lambda bufs: [b.ptr for b in bufs]
    e0, e1 = lib.fl_event_create(), lib.fl_event_create()

    def timed(fn, reps):
        fn(); lib.fl_sync()
        best, tot = 1e9, 0.0
        for _ in range(reps):
            lib.fl_event_record(e0); fn(); lib.fl_event_record(e1)
            ms = lib.fl_event_elapsed_ms(e0, e1)
            best, tot = min(best, ms), tot + ms
        return {"min_us": round(best * 1e3, 1), "mean_us": round(tot / reps * 1e3, 1)}

    res = {"n": n}
    for name, src in pairs.items():
        fn = lambda: lib.gpu_accumulate_field2(src[0].ptr, o[0].ptr, -0.5, src[1].ptr, o[1].ptr, -0.5, *P(back), h, n, n, n, False)
        row = {}
        for rnd in range(2):                            # alternate the two settings
            for opt in (0, 1):
                lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, opt)
                t = timed(fn, a.reps)
                key = "on" if opt else "off"
                row[key] = t if key not in row or t["min_us"] < row[key]["min_us"] else row[key]
        row["overhead_us"] = round(row["on"]["min_us"] - row["off"]["min_us"], 1)
        res["accumulate2 " + name] = row
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_TAPS, 1)
    print(json.dumps(res), flush=True)
    bq.check()


if __name__ == "__main__":
    main()
