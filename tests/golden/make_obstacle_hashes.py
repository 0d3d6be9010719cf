"""Generates tests/golden/obstacle_hashes.json: per-step SHA-256 of rho, T, u, v, w, p and the cell flags of the 64^3
obstacle scene (tests/obstacle_case.py: a static sphere and a moving box in the rising smoke), 20 steps, 30 Jacobi sweeps,
both schemes, computed by the host solver linked to the CPU stand-in with the obstacle operators
(tests/build_cpu_host_obstacles.py).  tests/test_gpu_obstacles.py checks the GPU run against these.
Usage: python tests/golden/make_obstacle_hashes.py"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import obstacle_case as OC                                  # noqa: E402
from build_cpu_host_obstacles import build                  # noqa: E402
from gpufluidsimulation_amd import solver                   # noqa: E402

N, STEPS, ITERS = 64, 20, 30


def main():
    lib = OC.bind_errors(solver.bind_host(C.CDLL(build(), mode=C.RTLD_LOCAL)))
    out = {"n": N, "steps": STEPS, "jacobi_iters": ITERS}
    for scheme in (0, 3):
        out[f"scheme{scheme}"] = OC.run_scene(lib, lib, N, scheme, STEPS, ITERS)
    with open(os.path.join(HERE, "obstacle_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
