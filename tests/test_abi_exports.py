"""The drop-in boundary without a GPU: both shared libraries load, export every function that
include/bimocq_gpu.h and include/bimocq_solver.h declare, the ctypes tables cover the header, and the
product path fails loudly (no CPU fallback) when no GPU is present.  No compute calls."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECL = re.compile(r"^\s*(?:const\s+)?(?:unsigned\s+)?(?:void|int|float|double|long long|size_t|char|bq_solver)\s*\**\s*"
                  r"((?:gpu|fl|bq)_[A-Za-z0-9_]+)\s*\(", re.M)


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"typedef[^;]*;", "", text)          # callback typedefs are not exports
    return sorted(set(DECL.findall(text)))


def test_headers_declare_the_reference_entry_points():
    names = declared("bimocq_gpu.h")
    # the 22 entry points of the reference's GPU_Advection.h that the bimocq3D step uses or exposes
    for ref in ["gpu_solve_forward", "gpu_solve_backwardDMC", "gpu_advect_velocity", "gpu_advect_field",
                "gpu_compensate_velocity", "gpu_compensate_field", "gpu_accumulate_velocity", "gpu_accumulate_field",
                "gpu_estimate_distortion", "gpu_semilag", "gpu_emit_smoke", "gpu_add_buoyancy", "gpu_add",
                "gpu_diffuse_field", "gpu_projection_jacobi", "gpu_clamp_extrema",
                "gpu_conjugate_gradient", "gpu_multi_grid_conjugate_gradient"]:
        assert ref in names, ref
    assert len(names) >= 50


REF_DIGESTS = os.path.join(ROOT, "tests", "golden", "reference_prototypes.json")
REF_NAMES = ["gpu_solve_forward", "gpu_solve_backwardDMC", "gpu_advect_velocity", "gpu_advect_vel_double", "gpu_advect_field",
             "gpu_advect_field_double", "gpu_accumulate_velocity", "gpu_accumulate_field", "gpu_estimate_distortion", "gpu_add",
             "gpu_compensate_velocity", "gpu_compensate_field", "gpu_semilag", "gpu_emit_smoke", "gpu_add_buoyancy",
             "gpu_diffuse_field", "gpu_add_field", "gpu_projection_jacobi", "gpu_clamp_extrema", "gpu_mad",
             "gpu_conjugate_gradient", "gpu_multi_grid_conjugate_gradient"]


def prototypes(text):
    """{name: (return type, [parameter types])} of every `gpu_*(...)` prototype in a header's text, types
    normalised (no parameter names, no `const`, `struct`/`extern "C"` dropped, spaces around `*` removed)"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r'(?:extern\s+"C"\s+)?([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(gpu_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;', text):
        ret, name, params = m.group(1), m.group(2), m.group(3)

        def norm(t):
            t = re.sub(r"\b(const|struct|extern)\b", " ", t)
            t = re.sub(r"\s+", " ", t).strip()
            return t.replace(" *", "*").replace("* ", "*")

        types = []
        for prm in params.split(","):
            prm = prm.strip()
            if not prm or prm == "void":
                continue
            mm = re.match(r"(.*?[\s\*])([A-Za-z_][A-Za-z0-9_]*)$", prm)       # drop the parameter name
            types.append(norm(mm.group(1) if mm else prm))
        out[name] = (norm(ret), types)
    return out


def digest(proto):
    """SHA-256 of one normalised prototype (return type, [parameter types])"""
    return hashlib.sha256(json.dumps([proto[0], proto[1]]).encode()).hexdigest()


def test_prototypes_equal_the_reference_header():
    """all 22 extern "C" prototypes of the reference's operator boundary (GPU_Advection.h:26-108): same return type,
    same parameter types in the same order in include/bimocq_gpu.h -- ours parsed at test time, the reference's pinned as
    digests of its normalised prototypes in tests/golden/reference_prototypes.json (`python tests/test_abi_exports.py
    <reference>/src/bimocq3D/GPU_Advection.h` rewrites that file)"""
    with open(REF_DIGESTS) as f:
        ref = json.load(f)["sha256"]
    ours = prototypes(open(os.path.join(ROOT, "include", "bimocq_gpu.h")).read())
    assert sorted(ref) == sorted(REF_NAMES), sorted(ref)
    for name in REF_NAMES:
        assert name in ours, name
        assert digest(ours[name]) == ref[name], (name, ours[name])


def test_every_reference_entry_point_is_declared_and_exported():
    names = declared("bimocq_gpu.h")
    lib = C.CDLL(os.path.join(ROOT, "gpufluidsimulation_amd", "libbimocq_hip.so"))
    for ref in REF_NAMES:
        assert ref in names and hasattr(lib, ref), ref


@pytest.mark.parametrize("header,so", [("bimocq_gpu.h", "libbimocq_hip.so"), ("bimocq_solver.h", "libbimocq_host.so")])
def test_library_exports_every_declared_symbol(header, so):
    path = os.path.join(ROOT, "gpufluidsimulation_amd", so)
    assert os.path.exists(path), f"{so} missing: run `make`"
    # local scope: the CPU-only host tests load a stand-in that defines the same gpu_* names
    lib = C.CDLL(path)      # libbimocq_host.so finds libbimocq_hip.so through DT_NEEDED + $ORIGIN rpath
    missing = [n for n in declared(header) if not hasattr(lib, n)]
    assert not missing, missing


def test_ctypes_tables_cover_the_headers():
    from gpufluidsimulation_amd import _lib, solver
    for header, table in [("bimocq_gpu.h", _lib.HIP_SIGS), ("bimocq_solver.h", solver.HOST_SIGS)]:
        missing = [n for n in declared(header) if n not in table]
        assert not missing, (header, missing)


def test_no_gpu_means_loud_failure():
    """on a box without a GPU fl_init reports an error and the Python layer raises: nothing computes
    on the CPU behind the caller's back"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import gpufluidsimulation_amd as bq
    from gpufluidsimulation_amd import solver
    lib = bq.hip_lib()
    rc = lib.fl_init(0)
    assert rc != 0
    assert lib.fl_last_error() != 0 and lib.fl_last_error_string()
    lib.fl_clear_error()
    with pytest.raises(bq.BimocqError):
        solver.BimocqGPUSolver(16, 16, 16, 1.0)


if __name__ == "__main__":
    protos = prototypes(open(sys.argv[1]).read())
    with open(REF_DIGESTS, "w") as f:
        json.dump({"source": "src/bimocq3D/GPU_Advection.h of the reference, prototypes() of tests/test_abi_exports.py",
                   "sha256": {n: digest(protos[n]) for n in sorted(protos)}}, f, indent=1)
        f.write("\n")
