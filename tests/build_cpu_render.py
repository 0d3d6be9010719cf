"""Builds the CPU stand-in of the C-ABI with the density preview (see build_cpu_host.py): the diagnostics stand-in's list
plus tests/cpu_abi/render_abi.c (gpu_render_density).  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_render():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_render.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c",
                   "render_abi.c"])


if __name__ == "__main__":
    print(build_render())
