"""Generates tests/golden/obstacle_hashes.json and tests/golden/levelset_hashes.json: per-step SHA-256 of rho, T, u, v, w,
p and the cell flags of the 64^3 obstacle scene (tests/obstacle_case.py: a static sphere and a moving box in the rising
smoke) and of the 64^3 level-set scene (tests/levelset_case.py: a static level-set sphere, an analytic box and a moving
level-set box), 20 steps, 30 Jacobi sweeps, both schemes, computed by the host solver linked to the CPU stand-ins with the
obstacle and the level-set operators (tests/build_cpu_host.py).  tests/test_gpu_obstacles.py and
tests/test_gpu_levelsets.py check the GPU runs against these.
Usage: python tests/golden/make_obstacle_hashes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import levelset_case as LC                                  # noqa: E402
import obstacle_case as OC                                  # noqa: E402

N, STEPS, ITERS = 64, 20, 30


def main():
    for name, lib, scene in (("obstacle_hashes.json", OC.load_obstacles(), OC.scene),
                             ("levelset_hashes.json", OC.load_levelsets(), LC.scene)):
        out = {"n": N, "steps": STEPS, "jacobi_iters": ITERS}
        for scheme in (0, 3):
            out[f"scheme{scheme}"] = OC.run_scene(lib, lib, N, scheme, STEPS, ITERS, scene)
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
