"""Writes tests/golden/source_hashes.json: per-step SHA-256 of rho, T, u, v, w, p of the 64^3 plume scene
(tests/source_case.py scene: scenes.plume drifting sideways, a static sphere source without velocity, the level-set
obstacle scene's sphere), 20 steps, 30 Jacobi sweeps in both schemes and one leg with the kind-2 projection, computed by
the host solver linked to the CPU stand-in that has gpu_emit_sources (tests/build_cpu_sources.py).
tests/test_gpu_sources.py checks the GPU runs against these.  CPU only.
Usage: python tests/golden/make_source_hashes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import source_case as SC  # noqa: E402

N, STEPS, ITERS, PCG_ITERS = 64, 20, 30, 1000


def main():
    lib = SC.load_sources()
    out = {"n": N, "steps": STEPS, "jacobi_iters": ITERS, "pcg_iters": PCG_ITERS}
    for scheme, kind in ((0, 0), (3, 0), (0, 2)):
        out[f"scheme{scheme}_kind{kind}"] = SC.run_scene(lib, lib, N, scheme, STEPS, PCG_ITERS if kind == 2 else ITERS, kind=kind)
    with open(os.path.join(HERE, "source_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
