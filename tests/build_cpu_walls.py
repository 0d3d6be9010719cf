"""Builds the CPU stand-in with the wall operators (tests/cpu_abi/walls_abi.c) on top of the
obstacle, level-set and PCG restatements: tests/_build/libbimocq_host_cpu_walls.so.  Test infrastructure."""
import os

import build_cpu_host


def build_walls():
    return build_cpu_host._build(os.path.join(build_cpu_host.OUT, "libbimocq_host_cpu_walls.so"),
                                 ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "walls_abi.c"])


if __name__ == "__main__":
    print(build_walls())
