"""No-GPU checks of the many-sequence VisualOdometry surface (bpvo_hip_add_frames): the C++ class compiles as C++11 against the C ABI, and the
Python context has the methods.  (test_cabi_cpu.py's export test covers the new C declarations.)"""
import os
import subprocess

from bpvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_visual_odometry_sequences_compiles_as_cpp11():
    src = os.path.join(ROOT, "tests", "cpp", "multi_sequence_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_python_context_has_the_sequence_methods():
    for name in ("add_frames", "add_frames_device", "seq_trajectory", "seq_point_cloud", "seq_num_points_at_level", "seq_reset", "seq_capacity"):
        assert callable(getattr(capi.Context, name, None)), name


def test_header_declares_the_sequence_entry_points():
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    for name in ("bpvo_hip_add_frames", "bpvo_hip_seq_capacity", "bpvo_hip_seq_reset", "bpvo_hip_seq_num_points_at_level", "bpvo_hip_seq_get_point_cloud",
                 "bpvo_hip_seq_trajectory_size", "bpvo_hip_seq_get_trajectory"):
        assert name + "(" in src, name
