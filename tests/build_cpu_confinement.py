"""Builds the CPU stand-in of the C-ABI with the vorticity confinement (see build_cpu_host.py): the diagnostics stand-in's list
plus tests/cpu_abi/confinement_abi.c (gpu_vorticity_confinement) and the wall operators
(tests/cpu_abi/walls_abi.c), which the boxed trajectory of the GPU tests needs.  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_confinement():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_confinement.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c",
                   "walls_abi.c", "confinement_abi.c"])


if __name__ == "__main__":
    print(build_confinement())
