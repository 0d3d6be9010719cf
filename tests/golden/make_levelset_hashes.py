"""Generates tests/golden/levelset_hashes.json: per-step SHA-256 of rho, T, u, v, w, p and the cell flags of the 64^3
level-set scene (tests/levelset_case.py: a static level-set sphere, an analytic box and a moving level-set box in the
rising smoke), 20 steps, 30 Jacobi sweeps, both schemes, computed by the host solver linked to the CPU stand-in with the
level-set operators (tests/build_cpu_host_levelsets.py).  tests/test_gpu_levelsets.py checks the GPU run against these.
Usage: python tests/golden/make_levelset_hashes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import levelset_case as LC                                  # noqa: E402
from build_cpu_host_levelsets import build                  # noqa: E402

N, STEPS, ITERS = 64, 20, 30


def main():
    lib = LC.load(build())
    out = {"n": N, "steps": STEPS, "jacobi_iters": ITERS}
    for scheme in (0, 3):
        out[f"scheme{scheme}"] = LC.run_scene(lib, lib, N, scheme, STEPS, ITERS)
    with open(os.path.join(HERE, "levelset_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
