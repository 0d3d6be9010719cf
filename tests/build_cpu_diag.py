"""Builds the CPU stand-in of the C-ABI with the flow diagnostics (see build_cpu_host.py): the MacCormack stand-in's list
plus tests/cpu_abi/flow_stats_abi.c (gpu_flow_stats).  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_diag():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_diag.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c"])


if __name__ == "__main__":
    print(build_diag())
