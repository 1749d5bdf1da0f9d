"""No-GPU checks of per-sequence algorithm parameters (bpvo_hip_seq_set_params / bpvo_hip_seq_get_params): the header declares them, the Python
and C++ surfaces carry them, and the oracle binding, which has neither, still loads."""
import os
import subprocess

import __graft_entry__ as ge
from bpvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")


def test_header_declares_the_params_entry_points():
    src = open(HEADER).read()
    assert "int bpvo_hip_seq_set_params(bpvo_hip_ctx* ctx, int seq, const bpvo_hip_params* p);" in src
    assert "int bpvo_hip_seq_get_params(const bpvo_hip_ctx* ctx, int seq, bpvo_hip_params* p);" in src


def test_python_surface_has_the_params_methods():
    for name in ("seq_set_params", "seq_get_params"):
        assert callable(getattr(capi.Context, name, None)), name


def test_binding_does_not_require_the_params_symbols():
    """The oracle library shares Binding and has none of these entry points."""
    if not os.path.exists(ge.ORACLE_LIB):
        ge.build_oracle()
    orc = capi.Binding(ge.ORACLE_LIB, "bpvo_orc_")
    assert not orc.has("seq_set_params") and not orc.has("seq_get_params")
    assert isinstance(orc.default_params(), capi.Params)      # the binding works without them


def test_visual_odometry_sequences_with_params_compiles_as_cpp11():
    src = os.path.join(ROOT, "tests", "cpp", "seq_params_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_the_structural_fields_of_the_docs_are_fields_of_the_params():
    """Every field the header's comment block names — as a sequence's own or as fixed by the context — is a field of bpvo_hip_params."""
    fields = {f[0] for f in capi.Params._fields_}
    own = ["lossFunction", "maxIterations", "parameterTolerance", "functionTolerance", "gradientTolerance", "minTranslationMagToKeyFrame",
           "minRotationMagToKeyFrame", "maxFractionOfGoodPointsToKeyFrame", "goodPointThreshold", "minSaliency", "minValidDisparity",
           "maxValidDisparity", "relaxTolerancesForCoarseLevels", "minNumPixelsToWork", "verbosity"]
    fixed = ["numPyramidLevels", "minImageDimensionForPyramid", "descriptor", "gradientEstimation", "interp", "withNormalization", "nonMaxSuppRadius",
             "minNumPixelsForNonMaximaSuppression", "maxTestLevel", "laplacianKernelSize"]
    src = open(HEADER).read()
    block = src[src.index("per-sequence algorithm parameters"):src.index("int bpvo_hip_seq_set_params(")]
    for name in own + fixed:
        assert name in fields and name in block, name
