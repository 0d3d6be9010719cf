"""Builds the CPU stand-in with the PCG projection operators (tests/cpu_abi/pcg_abi.c) on top of the
obstacle and level-set restatements: tests/_build/libbimocq_host_cpu_pcg.so.  Test infrastructure."""
import os

import build_cpu_host


def build_pcg():
    return build_cpu_host._build(os.path.join(build_cpu_host.OUT, "libbimocq_host_cpu_pcg.so"),
                                 ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c"])


if __name__ == "__main__":
    print(build_pcg())
