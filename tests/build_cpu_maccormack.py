"""Builds the fifth CPU stand-in of the C-ABI (see build_cpu_host.py): the host sources linked against the oracle's
operators, the obstacle, level-set, PCG and source restatements and tests/cpu_abi/maccormack_abi.c (gpu_maccormack,
DESIGN.md section 17).  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_maccormack():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_maccormack.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c"])


if __name__ == "__main__":
    print(build_maccormack())
