#!/usr/bin/env python3
"""FL_OPT_SKIP_EMPTY_BRICKS on its worst case: the three two-field scalar operators at n^3 on fields with no zero word, option 3
(all three operators take part; the default, 1, leaves the accumulation out) against option 0 in one process (alternating, events
on the compute stream) -- on a dense field the option should cost the flag pass and little else.  The flag pass's own time is the
brick_flags_kernel row of `rocprofv3 --kernel-trace --stats -- python tools/sparse_dense_cost.py`.  With --sparse the same on an
all-zero pair (the best case).

    python tools/sparse_dense_cost.py [--n 256] [--reps 20] [--sparse]
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
    ap.add_argument("--sparse", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import DeviceBuffer
    import fields as F
    lib, n = bq.hip_lib(), a.n
    h = float(np.float32(1.0 / n))
    dev = lambda x: DeviceBuffer.from_numpy(np.ascontiguousarray(x, np.float32))
    back, fwd = [dev(m) for m in F.warped_maps(n, n, n, h, -0.7, 1.1)], [dev(m) for m in F.warped_maps(n, n, n, h, 0.8, 0.3)]
    if a.sparse:
        src = [dev(np.zeros(n ** 3, np.float32)) for _ in range(2)]
    else:
        src = [dev(F.scalar(n, n, n, 0.4) + np.float32(2.0)), dev(F.scalar(n, n, n, 1.9) - np.float32(3.0))]
    o = [dev(np.zeros(n ** 3, np.float32)) for _ in range(4)]
    P = lambda bufs: [b.ptr for b in bufs]
    ops = {
        "advect2": lambda: lib.gpu_advect_field2(o[0].ptr, src[0].ptr, o[1].ptr, src[1].ptr, *P(back), h, n, n, n, False),
        "error2": lambda: lib.gpu_compensate_error_field2(src[0].ptr, o[0].ptr, o[2].ptr, src[1].ptr, o[1].ptr, o[3].ptr, *P(fwd), h, n, n, n, False),
        "accumulate2": lambda: lib.gpu_accumulate_field2(src[0].ptr, o[0].ptr, -0.5, src[1].ptr, o[1].ptr, -0.5, *P(back), h, n, n, n, False),
    }
    e0, e1 = lib.fl_event_create(), lib.fl_event_create()

    def timed(fn, reps):
        fn(); lib.fl_sync()
        best, tot = 1e9, 0.0
        for _ in range(reps):
            lib.fl_event_record(e0); fn(); lib.fl_event_record(e1)
            ms = lib.fl_event_elapsed_ms(e0, e1)
            best, tot = min(best, ms), tot + ms
        return {"min_us": round(best * 1e3, 1), "mean_us": round(tot / reps * 1e3, 1)}

    res = {"n": n, "sparse": bool(a.sparse)}
    for name, fn in ops.items():
        row = {}
        for rnd in range(2):                            # alternate the two settings
            for opt in (0, 3):
                lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, opt)
                t = timed(fn, a.reps)
                key = "on" if opt else "off"
                row[key] = t if key not in row or t["min_us"] < row[key]["min_us"] else row[key]
        row["overhead_us"] = round(row["on"]["min_us"] - row["off"]["min_us"], 1)
        res[name] = row
    lib.fl_set_option(bq._lib.FL_OPT_SKIP_EMPTY_BRICKS, 1)
    flags = np.zeros((-(-n // 8)) ** 3, np.uint8)
    # the flag pass through its own entry point (which adds a read-back of the flags: timed by events around the call, so it is in)
    res["flag_pass_with_readback"] = timed(lambda: lib.gpu_brick_flags(src[0].ptr, src[1].ptr, n, n, n, flags.ctypes.data, None), a.reps)
    print(json.dumps(res), flush=True)
    bq.check()


if __name__ == "__main__":
    main()
