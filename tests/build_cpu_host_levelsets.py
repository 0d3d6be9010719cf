"""Builds tests/_build/libbimocq_host_cpu_levelsets.so: the obstacle stand-in of tests/build_cpu_host_obstacles.py plus the
C restatement of the level-set operators (tests/cpu_abi/levelset_abi.c), linked with the same host sources.  The obstacle
stand-in lacks the level-set operators: there the host solver's weak references to them are null and a list with a level
set is refused.  Test infrastructure."""
import glob
import os
import subprocess

from build_cpu_host import ROOT, OUT

SO = os.path.join(OUT, "libbimocq_host_cpu_levelsets.so")


def build():
    os.makedirs(OUT, exist_ok=True)
    host = sorted(glob.glob(os.path.join(ROOT, "gpufluidsimulation_amd", "csrc", "host", "*.cpp")))
    abi = os.path.join(ROOT, "tests", "cpu_abi")
    c_srcs = [os.path.join(abi, "oracle_abi.c"), os.path.join(abi, "obstacle_abi.c"), os.path.join(abi, "levelset_abi.c"),
              os.path.join(ROOT, "oracle", "bimocq_oracle.c"), os.path.join(ROOT, "oracle", "mgcg_oracle.c")]
    deps = host + c_srcs + glob.glob(os.path.join(ROOT, "gpufluidsimulation_amd", "csrc", "host", "*.hpp")) + [
        os.path.join(ROOT, "oracle", "bimocq_oracle.h"),
        os.path.join(ROOT, "include", "bimocq_gpu.h"), os.path.join(ROOT, "include", "bimocq_solver.h")]
    if os.path.exists(SO) and all(os.path.getmtime(d) <= os.path.getmtime(SO) for d in deps):
        return SO
    cflags = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-I" + os.path.join(ROOT, "include")]
    objs = []
    for src in c_srcs + host:
        cc, std = ("g++", "-std=c++17") if src.endswith(".cpp") else ("gcc", "-std=gnu11")
        obj = os.path.join(OUT, "ls_" + os.path.basename(src) + ".o")
        subprocess.check_call([cc, std, *cflags, "-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call(["g++", "-shared", "-fopenmp", "-pthread", "-o", SO, *objs, "-lm"])
    return SO


if __name__ == "__main__":
    print(build())
