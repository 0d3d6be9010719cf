"""Builds the fourth CPU stand-in of the C-ABI (see build_cpu_host.py): the host sources linked against the oracle's
operators, the obstacle, level-set and PCG restatements and tests/cpu_abi/source_abi.c (gpu_emit_sources, DESIGN.md
section 16).  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_sources():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_sources.so"), ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c"])


if __name__ == "__main__":
    print(build_sources())
