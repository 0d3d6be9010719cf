"""Builds the CPU stand-in of the C-ABI with the tracer operators (see build_cpu_host.py): the render stand-in's list plus
tests/cpu_abi/tracers_abi.c (gpu_trace_particles, gpu_sample_particles, gpu_seed_particles, gpu_sort_particles; DESIGN.md
section 22).  Test infrastructure."""
import os

from build_cpu_host import OUT, _build


def build_tracers():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_tracers.so"),
                  ["obstacle_abi.c", "levelset_abi.c", "pcg_abi.c", "source_abi.c", "maccormack_abi.c", "flow_stats_abi.c",
                   "render_abi.c", "tracers_abi.c"])


if __name__ == "__main__":
    print(build_tracers())
