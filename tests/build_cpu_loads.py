"""Builds the CPU stand-in of the C-ABI with the per-obstacle pressure loads (see build_cpu_host.py): the diagnostics stand-in's
list plus tests/cpu_abi/obstacle_loads_abi.c (gpu_obstacle_loads), and the wall and pose operators
(walls_abi.c, pose_abi.c), which the spinning box and the boxed case of the load tests need.  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_loads():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_loads.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c",
                   "walls_abi.c", "pose_abi.c", "obstacle_loads_abi.c"])


if __name__ == "__main__":
    print(build_loads())
