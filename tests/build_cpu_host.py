"""Builds the CPU stand-ins of the C-ABI: the product's C++ HOST sources (csrc/host/*.cpp) linked against test-only C
restatements of the operators.  Used by the `-m "not gpu"` tests to check the host step logic without a GPU, and by the
GPU tests as references.  Test infrastructure.
  build()            tests/_build/libbimocq_host_cpu.so: tests/cpu_abi/oracle_abi.c + the oracle
  build_obstacles()  ..._obstacles.so: + the obstacle operators (tests/cpu_abi/obstacle_abi.c)
  build_levelsets()  ..._levelsets.so: + the level-set operators (tests/cpu_abi/levelset_abi.c)
  build_launch_geom() tests/_build/liblaunch_geom.so: csrc/bq_launch_geom.h behind tests/cpu_abi/launch_geom_shim.cpp
  build_jacobi_plan() tests/_build/libjacobi_plan.so: csrc/bq_jacobi_plan.h behind tests/cpu_abi/jacobi_plan_shim.cpp
  build_box_chunk()  tests/_build/libbox_chunk.so: csrc/bq_box_chunk.h behind tests/cpu_abi/box_chunk_shim.cpp
  build_slab_jacobi_plan() tests/_build/libslab_jacobi_plan.so: csrc/host/slab_jacobi_plan.hpp behind tests/cpu_abi/slab_jacobi_plan_shim.cpp
  build_mgcg_slab_plan() tests/_build/libmgcg_slab_plan.so: csrc/bq_mgcg_slab_plan.h behind tests/cpu_abi/mgcg_slab_plan_shim.cpp
A stand-in without some operators leaves the host solver's weak references to them null: set_boundary refuses there."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# BQ_SANITIZE=1 (set by `make sanitize`, which also preloads libasan into the interpreter): the same sources built with
# AddressSanitizer + UndefinedBehaviorSanitizer into a directory of their own (sanitizers on the CPU build)
SANITIZE = os.environ.get("BQ_SANITIZE", "0") not in ("", "0")
OUT = os.path.join(ROOT, "tests", "_build_san" if SANITIZE else "_build")
SO = os.path.join(OUT, "libbimocq_host_cpu.so")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
ABI = os.path.join(ROOT, "tests", "cpu_abi")
CSRC = os.path.join(ROOT, "gpufluidsimulation_amd", "csrc")


def _build(so, extra_abi):
    """the stand-in `so` with the C restatements `extra_abi` (file names under tests/cpu_abi) on top of oracle_abi.c"""
    os.makedirs(OUT, exist_ok=True)
    host = sorted(glob.glob(os.path.join(CSRC, "host", "*.cpp")))
    c_srcs = [(os.path.join(ABI, name), "-std=gnu11") for name in ["oracle_abi.c"] + extra_abi] + [
        (os.path.join(ROOT, "oracle", name), "-std=c11") for name in ("bimocq_oracle.c", "mgcg_oracle.c")]
    deps = host + [src for src, _ in c_srcs] + glob.glob(os.path.join(CSRC, "host", "*.hpp")) + [
        os.path.join(CSRC, "bq_levelset.h"), os.path.join(ROOT, "oracle", "bimocq_oracle.h"),
        os.path.join(ROOT, "include", "bimocq_gpu.h"), os.path.join(ROOT, "include", "bimocq_solver.h")]
    if os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps):
        return so
    cflags = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"]
    if SANITIZE:
        cflags = ["-O1"] + cflags[1:] + SAN_FLAGS
    prefix = os.path.basename(so)[:-len(".so")] + "_"
    objs = []
    for src, cc, std in [(src, "gcc", std) for src, std in c_srcs] + [(h, "g++", "-std=c++17") for h in host]:
        obj = os.path.join(OUT, prefix + os.path.basename(src) + ".o")
        subprocess.check_call([cc, std, *cflags, "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-fopenmp", "-pthread", *(SAN_FLAGS if SANITIZE else []), "-o", so, *objs, "-lm"])
    return so


def build():
    return _build(SO, [])


def build_obstacles():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_obstacles.so"), ["obstacle_abi.c"])


def build_levelsets():
    return _build(os.path.join(OUT, "libbimocq_host_cpu_levelsets.so"), ["obstacle_abi.c", "levelset_abi.c"])


def _build_header_shim(so_name, shim, headers):
    """a host-only header of the product behind its C shim (tests/cpu_abi) as a library for ctypes"""
    os.makedirs(OUT, exist_ok=True)
    so = os.path.join(OUT, so_name)
    deps = [os.path.join(ABI, shim)] + [os.path.join(CSRC, h) for h in headers]
    if os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps):
        return so
    flags = ["-O1", *SAN_FLAGS] if SANITIZE else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-fPIC", "-Wall", "-Wextra", "-shared", "-I" + CSRC, deps[0], "-o", so])
    return so


def build_launch_geom():
    """the launchers' integer geometry rules"""
    return _build_header_shim("liblaunch_geom.so", "launch_geom_shim.cpp", ["bq_launch_geom.h"])


def build_jacobi_plan():
    """the decoder of the Jacobi tuning options and the planners of the sweep launches"""
    return _build_header_shim("libjacobi_plan.so", "jacobi_plan_shim.cpp", ["bq_jacobi_plan.h", "bq_launch_geom.h"])


def build_box_chunk():
    """how the box copies cut a box list into launches"""
    return _build_header_shim("libbox_chunk.so", "box_chunk_shim.cpp", ["bq_box_chunk.h"])


def build_slab_jacobi_plan():
    """a chunk of the z-slab Jacobi projection as a list of passes, and their plane ranges"""
    return _build_header_shim("libslab_jacobi_plan.so", "slab_jacobi_plan_shim.cpp", ["host/slab_jacobi_plan.hpp"])


def build_mgcg_slab_plan():
    """the decomposition of the slab-shared multigrid-CG projection: predicate, pyramid, plane ranges, derived counts"""
    return _build_header_shim("libmgcg_slab_plan.so", "mgcg_slab_plan_shim.cpp", ["bq_mgcg_slab_plan.h"])


if __name__ == "__main__":
    print(build(), build_obstacles(), build_levelsets(), build_launch_geom(), build_jacobi_plan(), build_box_chunk(), build_slab_jacobi_plan(),
          build_mgcg_slab_plan())
