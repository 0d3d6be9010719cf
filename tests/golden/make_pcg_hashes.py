"""Writes tests/golden/pcg_hashes.json: per-step hashes and PCG stats of the 64^3 mixed obstacle + level-set scene with
the kind-2 projection on the CPU stand-in (tests/pcg_case.py run_mixed), for tests/test_gpu_pcg.py.  CPU only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pcg_case as P  # noqa: E402

N, STEPS = 64, 20


def main():
    lib = P.load_pcg()
    out = {"n": N, "steps": STEPS}
    for scheme in (0, 3):
        out[f"scheme{scheme}"] = P.run_mixed(lib, lib, N, scheme, STEPS)
    with open(os.path.join(HERE, "pcg_hashes.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
