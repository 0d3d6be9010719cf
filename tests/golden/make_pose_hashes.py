"""Generates tests/golden/pose_hashes.json: per-step SHA-256 of rho, T, u, v, w, p, the obstacle flags and the orientations
of pose_case.scene (a spinning, tilted level-set box and a translating sphere in rising smoke) on 24 x 20 x 16, 6 steps,
schemes 0, 2 and 3, with 40 Jacobi sweeps (halfrdx 0.5) and with the PCG projection (halfrdx 1), with open sides and inside
the reference's container, computed by the host solver linked to the CPU stand-in with the pose operators
(tests/build_cpu_pose.py).  tests/test_pose_cpu.py replays them on the stand-in, tests/test_gpu_pose.py on the GPU.
Usage: python tests/golden/make_pose_hashes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pose_case as P                                       # noqa: E402


def main():
    lib = P.load_pose()
    out = {"dims": P.SCENE_DIMS, "steps": P.SCENE_STEPS, "kinds": P.SCENE_KINDS}
    for scheme, kind, walls in P.scene_cases():
        out[P.case_key(scheme, kind, walls)] = P.run_scene(lib, lib, scheme, kind, walls)
    with open(os.path.join(HERE, "pose_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
