"""No-GPU checks of the Student-t loss (BPVO_LOSS_STUDENT_T, c_api.h): the serial form of the scale fit, built from bpvo_amd/csrc/tscale_math.h with
a plain C++ compiler, against the numpy evaluation of the definition; the same harness under AddressSanitizer / UBSan; the config-file spelling; the
C ABI's enum and export."""
import os
import re
import subprocess

import numpy as np
import pytest

import bpvo_amd
from bpvo_amd import capi

import student_t_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "tscale_harness.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tscale")
    files = {}
    for name, (r, _) in ref.multisets().items():
        files[name] = str(tmp / (name + ".f32"))
        r.tofile(files[name])
    return dict(tmp=tmp, files=files, plain=_build(tmp, "tscale_harness"),
                san=_build(tmp, "tscale_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


def _run(exe, path, sigma_prev=None):
    out = subprocess.run([exe, path, "0" if sigma_prev is None else "1", repr(float(1.0 if sigma_prev is None else sigma_prev))],
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    ex, fr, passes, sigma, delta = out.stdout.split()
    return dict(exists=bool(int(ex)), frozen=bool(int(fr)), passes=int(passes), sigma=np.float32(sigma), delta=float(delta))


def _agree(h, n, what):
    assert h["exists"] == n["exists"] and h["frozen"] == n["frozen"], (what, h, n)
    # both sides stop within 1e-4 of the same unique fixed point from the same start
    assert abs(float(h["sigma"]) - float(n["sigma"])) <= 2e-4 * float(n["sigma"]), (what, h, n)


@pytest.mark.parametrize("name", sorted(ref.multisets()))
def test_serial_fit_agrees_with_the_definition(work, name):
    r, expect = ref.multisets()[name]
    n = ref.fit(r)
    # the precondition of the comparison: plain iteration ends by its stop rule, not by the guard
    assert n["passes"] < ref.MAX_PASSES, (name, n)
    if expect == "one":
        assert float(n["sigma"]) == 1.0 and (not n["exists"] or name.startswith("zeros")), (name, n)
    else:
        assert n["exists"] and not n["frozen"], (name, n)
        s = float(n["sigma"])
        assert abs(np.sqrt(ref.T(s * s, r)) - s) <= ref.STOP_REL * s, (name, n)      # a fixed point, to the stop rule
    h = _run(work["plain"], work["files"][name])
    _agree(h, n, name)
    assert h["passes"] < ref.MAX_PASSES
    if expect == "one":
        assert float(h["sigma"]) == 1.0


def test_existence_threshold_is_exact():
    r, _ = ref.multisets()["at_threshold"]
    assert (ref.NU + 1) * np.count_nonzero(r) == r.size and not ref.exists(r)
    assert ref.exists(np.concatenate([r, np.float32([0.5])]))      # one more non-zero entry: (nu + 1) (m + 1) > n + 1


@pytest.mark.parametrize("name", ["gaussian_core", "outliers_40", "intensity_30", "half_zeros", "two_valued"])
def test_warm_start_at_the_result_freezes_and_keeps_the_bits(work, name):
    r, _ = ref.multisets()[name]
    first = _run(work["plain"], work["files"][name])
    again = _run(work["plain"], work["files"][name], sigma_prev=first["sigma"])
    n = ref.fit(r, sigma_prev=first["sigma"])
    _agree(again, n, name)
    assert again["frozen"] and again["delta"] == 0.0 and again["passes"] == 1
    assert again["sigma"].tobytes() == first["sigma"].tobytes()
    # ... and from a start far from it the fit moves, to the same fixed point, and says "not frozen"
    far = _run(work["plain"], work["files"][name], sigma_prev=4.0 * float(first["sigma"]))
    nf = ref.fit(r, sigma_prev=4.0 * float(first["sigma"]))
    _agree(far, nf, name)
    assert not far["frozen"] and far["delta"] > 1e-6 and nf["passes"] < ref.MAX_PASSES
    assert abs(float(far["sigma"]) - float(first["sigma"])) <= 2e-4 * float(first["sigma"])


def test_harness_is_clean_under_address_and_undefined_sanitizers(work):
    for name, path in work["files"].items():
        a, b = _run(work["plain"], path), _run(work["san"], path)
        assert a["sigma"].tobytes() == b["sigma"].tobytes() and (a["exists"], a["frozen"], a["passes"]) == (b["exists"], b["frozen"], b["passes"]), name
    first = _run(work["san"], work["files"]["outliers_10"])
    assert _run(work["san"], work["files"]["outliers_10"], sigma_prev=first["sigma"])["frozen"]


def test_weight_and_curvature_of_the_definition():
    x = np.float32([0.0, 1.0, -1.7320508, 2.236068, 10.0])
    w = ref.weights_f32(x, 1.0)
    assert w[0] == np.float32(1.2) and w[1] == np.float32(1.0) and np.all(w > 0) and np.all(w <= np.float32(1.2))
    assert (w > np.float32(0.75)).tolist() == [True, True, False, False, False]      # the default goodPointThreshold: |x| < sqrt(3)
    d = ref.curvature(np.float64([0.0, 1.0, np.sqrt(5.0), 3.0]))
    assert d[0] == 1.2 and d[1] == pytest.approx(24.0 / 36.0) and abs(d[2]) < 1e-15 and d[3] < 0
    # d = psi' for psi(u) = u w(u), by a central difference
    u, h = np.linspace(-6, 6, 49), 1e-6
    psi = lambda v: v * 6.0 / (5.0 + v * v)
    assert np.allclose((psi(u + h) - psi(u - h)) / (2 * h), ref.curvature(u), atol=1e-8)


def test_config_file_reads_prints_and_round_trips_student_t(tmp_path):
    exe = str(tmp_path / "config_file_test")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "config_file_test.cc"),
                        "-o", exe, "-L", CSRC, "-lbpvo_hip", f"-Wl,-rpath,{CSRC}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for spelling in ("StudentT", "studentt", "STUDENTT"):
        cfg = tmp_path / "t.cfg"
        cfg.write_text(f"lossFunction = {spelling}\nnumPyramidLevels = 3\n")
        out = subprocess.run([exe, str(cfg), "print"], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout
        kv = dict(line.split() for line in out.stdout.split("PRINT\n", 1)[0].strip().splitlines())
        assert kv["lossFunction"] == str(capi.LOSS_STUDENT_T) == str(0x13)
        printed = out.stdout.split("PRINT\n", 1)[1].split("\n--\n")[0]
        assert "lossFunction = StudentT" in printed
    # what the facade prints for the loss parses back to the same value
    back = tmp_path / "back.cfg"
    back.write_text("\n".join(l for l in printed.splitlines() if l.startswith("lossFunction")) + "\n")
    out = subprocess.run([exe, str(back)], capture_output=True, text=True)
    assert out.returncode == 0 and dict(line.split() for line in out.stdout.strip().splitlines())["lossFunction"] == str(capi.LOSS_STUDENT_T)
    bad = tmp_path / "bad.cfg"
    bad.write_text("lossFunction = Student\n")
    out = subprocess.run([exe, str(bad)], capture_output=True, text=True)
    assert out.returncode == 1 and "unknown LossFunctionType" in out.stdout


def test_c_abi_declares_the_value_and_exports_the_counter_hook():
    src = open(HEADER).read()
    assert re.search(r"BPVO_LOSS_STUDENT_T\s*=\s*0x13\b", src) and capi.LOSS_STUDENT_T == 0x13
    assert len({capi.LOSS_HUBER, capi.LOSS_TUKEY, capi.LOSS_L2, capi.LOSS_STUDENT_T}) == 4
    assert re.search(r"kStudentT\s*=\s*BPVO_LOSS_STUDENT_T", open(os.path.join(ROOT, "include", "bpvo_hip", "vo.hpp")).read())
    lib = bpvo_amd.load()
    assert lib.has("tscale_counts") and "bpvo_hip_tscale_counts" in src
    # bpvo_hip_params keeps its layout, and the default loss is still Tukey
    assert lib.default_params().lossFunction == capi.LOSS_TUKEY
