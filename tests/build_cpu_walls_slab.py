"""Builds the CPU stand-in whose wall operators honour the z-slab context and which has the walled sweeps on plane ranges
(tests/cpu_abi/walls_slab_abi.c): tests/_build/libbimocq_host_cpu_walls_slab.so.  The obstacle,
level-set and PCG restatements are linked as in build_cpu_walls; walls_slab_abi.c takes the place of walls_abi.c AND of
oracle_abi.c, which it includes (the slab context and the projection log are file-static there).  Test infrastructure."""
import glob
import os
import subprocess

import build_cpu_host as B


def build_walls_slab():
    os.makedirs(B.OUT, exist_ok=True)
    so = os.path.join(B.OUT, "libbimocq_host_cpu_walls_slab.so")
    host = sorted(glob.glob(os.path.join(B.CSRC, "host", "*.cpp")))
    c_srcs = [(os.path.join(B.ABI, name), "-std=gnu11") for name in ("walls_slab_abi.c", "obstacle_abi.c", "levelset_abi.c", "pcg_abi.c")] + [
        (os.path.join(B.ROOT, "oracle", name), "-std=c11") for name in ("bimocq_oracle.c", "mgcg_oracle.c")]
    deps = host + [src for src, _ in c_srcs] + glob.glob(os.path.join(B.CSRC, "host", "*.hpp")) + [
        os.path.join(B.ABI, "oracle_abi.c"), os.path.join(B.CSRC, "bq_levelset.h"), os.path.join(B.ROOT, "oracle", "bimocq_oracle.h"),
        os.path.join(B.ROOT, "include", "bimocq_gpu.h"), os.path.join(B.ROOT, "include", "bimocq_solver.h")]
    if os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps):
        return so
    cflags = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp"]
    if B.SANITIZE:
        cflags = ["-O1"] + cflags[1:] + B.SAN_FLAGS
    objs = []
    for src, cc, std in [(src, "gcc", std) for src, std in c_srcs] + [(h, "g++", "-std=c++17") for h in host]:
        obj = os.path.join(B.OUT, "libbimocq_host_cpu_walls_slab_" + os.path.basename(src) + ".o")
        subprocess.check_call([cc, std, *cflags, "-I" + os.path.join(B.ROOT, "include"), "-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-fopenmp", "-pthread", *(B.SAN_FLAGS if B.SANITIZE else []), "-o", so, *objs, "-lm"])
    return so


def build_slab_jacobi_plan_walled():
    """csrc/host/slab_jacobi_plan.hpp with its walled mode behind tests/cpu_abi/slab_jacobi_plan_walled_shim.cpp"""
    return B._build_header_shim("libslab_jacobi_plan_walled.so", "slab_jacobi_plan_walled_shim.cpp", ["host/slab_jacobi_plan.hpp"])


if __name__ == "__main__":
    print(build_walls_slab(), build_slab_jacobi_plan_walled())
