"""Builds the CPU stand-in with the pose operators (tests/cpu_abi/pose_abi.c) on top of the
obstacle, level-set, PCG and wall restatements: tests/_build/libbimocq_host_cpu_pose.so.  Test infrastructure."""
import os

import build_cpu_host


def build_pose():
    return build_cpu_host._build(os.path.join(build_cpu_host.OUT, "libbimocq_host_cpu_pose.so"),
                                 ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "walls_abi.c", "pose_abi.c"])


if __name__ == "__main__":
    print(build_pose())
