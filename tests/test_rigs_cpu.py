"""Several rigs in one call, without a GPU: the plural rig entry points are exported by the built library, declared in include/bpvo_hip/c_api.h with
the argument lists bpvo_amd/capi.py calls them with, refuse a missing context, and bpvo::RigsVisualOdometry (include/bpvo_hip/vo.hpp) compiles as
C++11 and links against the library.  (The feature adds no pure host function to vo_state.h / rig_math.h — RigState is a record — so there is
no new host arithmetic to hold against numpy; tests/test_rig_cpu.py keeps checking the functions the plural path calls per rig.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import bpvo_amd
from bpvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")

# entry point -> the C parameter types after the context, as capi.py passes them (c_void_p for every array, byref for every record)
SIGNATURES = {
    "bpvo_hip_rigs_set": ["int", "const int*", "const int*", "const float*"],
    "bpvo_hip_rigs_get": ["int*", "int*", "int*", "float*"],
    "bpvo_hip_rigs_set_params": ["int", "const bpvo_hip_params*"],
    "bpvo_hip_rigs_get_params": ["int", "bpvo_hip_params*"],
    "bpvo_hip_add_frames_rigs": ["int", "const int*", "const uint8_t*", "const float*", "int", "bpvo_hip_result*"],
    "bpvo_hip_rigs_trajectory_size": ["int", "int*"],
    "bpvo_hip_rigs_get_trajectory": ["int", "float*"],
    "bpvo_hip_rigs_pose_covariance": ["int", "bpvo_hip_pose_covariance*"],
    "bpvo_hip_estimate_pose_rigs": ["int", "const int*", "const int*", "const int*", "const int*", "const float*", "const float*", "float*", "bpvo_hip_stats*"],
}
# the capi.Context method that makes the call, and how many arguments it hands to Context.call / the bound function after the handle
WRAPPERS = {
    "bpvo_hip_rigs_set": "rigs_set", "bpvo_hip_rigs_get": "rigs_get", "bpvo_hip_rigs_set_params": "rigs_set_params",
    "bpvo_hip_rigs_get_params": "rigs_get_params", "bpvo_hip_add_frames_rigs": "add_frames_rigs", "bpvo_hip_rigs_trajectory_size": "rigs_trajectory",
    "bpvo_hip_rigs_get_trajectory": "rigs_trajectory", "bpvo_hip_rigs_pose_covariance": "rigs_pose_covariance",
    "bpvo_hip_estimate_pose_rigs": "estimate_pose_rigs",
}


def declarations(names):
    """name -> parameter types as c_api.h declares them (comments stripped, parameter names dropped, array bounds read as pointers)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(bpvo_hip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        if name not in names:
            continue
        types = []
        for a in args.split(","):
            a = re.sub(r"\[[^\]]*\]", "*", " ".join(a.split()))
            m = re.match(r"^(const\s+)?(\w+)\s*(\**)\s*(\w+)?\s*(\**)$", a)
            assert m, (name, a)
            types.append(f"{m.group(1) or ''}{m.group(2)}{m.group(3)}{m.group(5)}")
        out[name] = types
    return out


def test_plural_rig_entry_points_are_exported_and_declared_as_capi_calls_them():
    lib = bpvo_amd.load()
    decl = declarations(set(SIGNATURES))
    for name, want in SIGNATURES.items():
        assert hasattr(lib.lib, name), f"{name} is not exported by {lib.path}"
        assert name in decl, f"{name} is not declared in c_api.h"
        ctx_type, rest = decl[name][0], decl[name][1:]
        assert ctx_type in ("bpvo_hip_ctx*", "const bpvo_hip_ctx*"), (name, ctx_type)
        assert rest == want, (name, rest, want)
        method = getattr(capi.Context, WRAPPERS[name])
        body = inspect.getsource(method)
        short = name[len("bpvo_hip_"):]
        calls = re.findall(rf'(?:self\.call\("{short}",|self\.b\.fn\("{short}"\)\(self\.h,)(.*?)\)\)?\n', body, flags=re.S)
        assert calls, f"capi.Context.{WRAPPERS[name]} does not call {name}"


def test_plural_rig_entry_points_refuse_a_null_context():
    lib = bpvo_amd.load().lib
    n = C.c_int(7)
    assert lib.bpvo_hip_rigs_get(None, C.byref(n), None, None, None) != 0
    assert lib.bpvo_hip_rigs_get_params(None, 0, C.byref(capi.Params())) != 0
    assert lib.bpvo_hip_rigs_set(None, 1, C.byref(n), None, None) != 0
    assert lib.bpvo_hip_add_frames_rigs(None, 1, None, None, None, 0, None) != 0
    assert lib.bpvo_hip_rigs_trajectory_size(None, 0, C.byref(n)) != 0
    assert lib.bpvo_hip_rigs_pose_covariance(None, 0, C.byref(capi.PoseCovariance())) != 0
    assert lib.bpvo_hip_estimate_pose_rigs(None, 1, C.byref(n), None, None, None, None, None, None, None) != 0


def test_the_header_states_the_rules_of_the_plural_calls():
    """the rig section's matrices are referred to, and every refusal of the plural calls is written down where the calls are declared"""
    src = open(HEADER).read()
    at = src.index("several rigs in one context")
    text = " ".join(src[at:src.index("bpvo_hip_estimate_pose_rigs(", at)].split())
    for phrase in ("DISJOINT", "in two rigs", "parameters of its own", "holds frames", "not rigid", "named twice", "out of range",
                   "BPVO_WARP_DISPARITY_SPACE_F32", "bit for bit", "as if the call had not been made", "name the plural call"):
        assert phrase in text, phrase


def test_rigs_visual_odometry_compiles_as_cpp11_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "rigs_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    csrc = os.path.join(ROOT, "bpvo_amd", "csrc")
    exe = str(tmp_path / "rigs_compile")
    out = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", csrc, "-lbpvo_hip",
                          f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
