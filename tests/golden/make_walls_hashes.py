"""Generates tests/golden/walls_hashes.json: per-step SHA-256 of rho, T, u, v, w, p and the obstacle flags of the 64^3
obstacle scene (tests/obstacle_case.py) inside the reference's container (walls closed but +y), 8 steps, schemes 0, 2 and
3, once with 60 Jacobi sweeps (halfrdx 0.5) and once with the PCG projection (halfrdx 1), computed by the host solver
linked to the CPU stand-in with the wall operators (tests/build_cpu_walls.py).  tests/test_gpu_walls.py checks the GPU runs
against these.
Usage: python tests/golden/make_walls_hashes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import walls_case as WC                                     # noqa: E402

N, STEPS = 64, 8
KINDS = {"jacobi": (0, 60, 0.5), "pcg": (2, 1000, 1.0)}     # projection kind, iterations, halfrdx


def main():
    lib = WC.load_walls()
    out = {"n": N, "steps": STEPS, "walls": WC.REFERENCE_BOX, "kinds": KINDS}
    for scheme in (0, 2, 3):
        for name, (kind, iters, halfrdx) in KINDS.items():
            out[f"scheme{scheme}_{name}"] = WC.run_scene(lib, lib, N, scheme, STEPS, iters, kind=kind, halfrdx=halfrdx)
    with open(os.path.join(HERE, "walls_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
