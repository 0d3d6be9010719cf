"""Builds the CPU stand-in of the C-ABI with the density preview and its solid-obstacle form (see build_cpu_host.py): the
preview stand-in's list plus tests/cpu_abi/render_solids_abi.c (gpu_render_density_solids).  Test
infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_render_solids():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_render_solids.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c",
                   "render_abi.c", "render_solids_abi.c"])


if __name__ == "__main__":
    print(build_render_solids())
