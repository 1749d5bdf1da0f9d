"""No-GPU checks of the disparity-fusion rule (c_api.h "disparity fusion"): bpvo_amd/csrc/disparity_fusion_math.h, built into a stand-alone program
around a serial loop (tests/cpp/disparity_fusion_harness.cc) — once plain, once under AddressSanitizer / UBSan, run as a child process —, against the
numpy statement of the same rule (tests/disparity_fusion_ref.py): the fused map, the variance map and the five class counts equal bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_fusion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")
F32 = np.float32


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "disparity_fusion_harness.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("disparity_fusion")
    return dict(tmp=tmp, n=[0], plain=_build(tmp, "df_harness"),
                san=_build(tmp, "df_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


BUILDS = ("plain", "san")


def _harness_step(work, build, cam, prm, M, Dc, Vc, P):
    """One step of the C++ loop: (D, V, counts dict)."""
    tmp = work["tmp"]
    work["n"][0] += 1
    tag = str(tmp / ("c%d_%s" % (work["n"][0], build)))
    rows, cols = cam["rows"], cam["cols"]
    predict = Dc is not None and P is not None
    Pm = np.eye(4, dtype=F32) if P is None else np.asarray(P, F32).reshape(4, 4)
    params = np.concatenate([[rows, cols], [cam[k] for k in ("fx", "fy", "cx", "cy", "b", "lo", "hi")],
                             [prm["measurement_sigma"], prm["process_sigma"], prm["gate"], prm["max_fill_sigma"]], [1.0 if predict else 0.0],
                             Pm.reshape(-1)]).astype(np.float64)
    assert params.size == 30
    params.tofile(tag + ".params")
    np.ascontiguousarray(M, F32).tofile(tag + ".m")
    (np.zeros((rows, cols), F32) if Dc is None else np.ascontiguousarray(Dc, F32)).tofile(tag + ".dc")
    (np.full((rows, cols), -1, F32) if Vc is None else np.ascontiguousarray(Vc, F32)).tofile(tag + ".vc")
    res = subprocess.run([work[build], "step", tag + ".params", tag + ".m", tag + ".dc", tag + ".vc", tag], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout, res.stderr)
    counts = dict(zip(ref.CLASSES, (int(v) for v in res.stdout.split())))
    return np.fromfile(tag + ".d", F32).reshape(rows, cols), np.fromfile(tag + ".v", F32).reshape(rows, cols), counts


def _both(work, build, cam, prm, M, Dc, Vc, P):
    """The numpy statement's step, after the C++ loop has been found equal to it bit for bit."""
    D, V, counts = ref.step(cam, prm, M, Dc, Vc, P)
    hD, hV, hcounts = _harness_step(work, build, cam, prm, M, Dc, Vc, P)
    assert ref.same_bits(hD, D) and ref.same_bits(hV, V), (np.argwhere(ref.bits(hD) != ref.bits(D))[:5], np.argwhere(ref.bits(hV) != ref.bits(V))[:5])
    assert hcounts == counts and sum(counts.values()) == cam["rows"] * cam["cols"]
    return D, V, counts


PRM = ref.rule(0.5, 0.1, 3.0, 2.0)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (33, 65), (120, 160)])
def test_three_chained_steps_equal_numpy(work, build, shape):
    cam, Ms, Ps = ref.chain_case(shape[0], shape[1], seed=shape[1])
    D = V = None
    seen = {k: 0 for k in ref.CLASSES}
    for k, (M, P) in enumerate(zip(Ms, Ps)):
        D, V, counts = _both(work, build, cam, PRM, M, D, V, None if k == 0 else P)      # (the carried variances feed the next step)
        if k == 0:
            assert counts["fused"] == counts["replaced"] == counts["filled"] == 0 and ref.same_bits(D, M)
        for name in ref.CLASSES:
            seen[name] += counts[name]
        with np.errstate(invalid="ignore"):
            assert np.all(ref.valid(D, cam["lo"], cam["hi"])[ref.valid(M, cam["lo"], cam["hi"])])      # a measured-valid pixel stays valid
            assert np.all((V >= 0) == ref.valid(D, cam["lo"], cam["hi"]))
    if shape[0] * shape[1] > 1000:      # (what the case is there for: every class occurs)
        assert all(seen[name] > 0 for name in ref.CLASSES), seen


@pytest.mark.parametrize("build", BUILDS)
def test_identity_motion_with_the_carried_map_as_measurement(work, build):
    cam, Ms, _ = ref.chain_case(33, 65, seed=5)
    prm = ref.rule(0.5, 0.0, 3.0, 2.0)
    M = Ms[0]
    D0, V0, _ = _both(work, build, cam, prm, M, None, None, None)
    D1, V1, counts = _both(work, build, cam, prm, M, D0, V0, ref.motion())
    carried = V0 >= 0
    assert ref.same_bits(D1, M)                                  # pd + k (m - pd) returns m exactly when both agree
    assert np.all(V1[carried] < V0[carried]) and np.all(V1[~carried] == -1)      # and the variance shrinks
    assert counts["fused"] == int(carried.sum()) and counts["replaced"] == counts["filled"] == counts["measured"] == 0


@pytest.mark.parametrize("build", BUILDS)
def test_collision_nearest_wins_then_larger_variance_and_ties_to_even(work, build):
    cam, Dc, Vc, P, M = ref.collision_case()
    prm = ref.rule(0.5, 0.25, 3.0, 2.0)
    z = ref.splat(cam, prm, Dc, Vc, P)
    q2 = prm["q2"]
    want = {2: (F32(2.0), F32(0.5) + q2), 7: (F32(4.0), F32(0.125) + q2)}      # target: (d', v')
    for t in range(8):
        if t in want:
            assert int(z[0, t]) == (int(ref.bits([want[t][0]])[0]) << 32) | int(ref.bits([want[t][1]])[0]), t
        else:
            assert z[0, t] == 0, t
    D, V, counts = _both(work, build, cam, prm, M, Dc, Vc, P)
    assert counts == dict(fused=1, replaced=1, measured=3, filled=0, none=3)
    assert D[0, 2] == 2.0 and V[0, 2] < want[2][1] and D[0, 7] == 8.0 and V[0, 7] == prm["r2"]


@pytest.mark.parametrize("build", BUILDS)
def test_edges_of_the_gate_the_bound_and_the_fill(work, build):
    cam, prm, Dc, Vc, P, M, expect = ref.edge_case()
    D, V, counts = _both(work, build, cam, prm, M, Dc, Vc, P)
    for name in ref.CLASSES:
        assert counts[name] == expect.count(name), (name, counts)
    assert D[0, 0] == F32(4.0) + F32(0.75) * F32(3.0) and V[0, 1] == prm["r2"] and D[0, 3] == 4.0 and V[0, 3] == 0.25
    assert V[0, 4] == -1 and V[0, 6] == prm["r2"] and V[0, 7] == -1 and V[0, 8] == prm["r2"] and V[0, 9] == -1
    assert np.isnan(D[0, 10]) and V[0, 10] == -1 and D[0, 11] == 4.0 and V[0, 11] == 0.0
    # max_fill_sigma = 0: never fill
    never = ref.rule(0.5, 0.0, 3.0, 0.0)
    _, _, counts0 = _both(work, build, cam, never, M, Dc, Vc, P)
    assert counts0["filled"] == 0 and counts0["none"] == counts["none"] + counts["filled"]


@pytest.mark.parametrize("build", BUILDS)
def test_hostile_measurements_keep_their_bits(work, build):
    cam, Ms, Ps = ref.chain_case(33, 65, seed=9)
    D0, V0, _ = _both(work, build, cam, PRM, Ms[0], None, None, None)
    M = ref.hostile_measurement(cam, seed=3)
    D, V, counts = _both(work, build, cam, ref.rule(0.5, 0.1, 3.0, 0.0), M, D0, V0, Ps[1])      # (never fill: an invalid measurement stays as it came)
    untouched = V == -1
    assert untouched.any() and np.array_equal(ref.bits(D)[untouched], ref.bits(M)[untouched])
    assert (ref.bits(D) == 0x7FC12345).sum() == (ref.bits(M) == 0x7FC12345).sum() == 1


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["behind", "outside", "gate", "nan", "inf"])
def test_motions_that_drop_every_candidate(work, build, name):
    cam, Ms, Ps = ref.chain_case(33, 65, seed=11)
    D0, V0, _ = _both(work, build, cam, PRM, Ms[0], None, None, None)
    P = dict(behind=ref.motion(t=(0.0, 0.0, -50.0)),            # Z' <= 0 everywhere (Z = fx b / d < 1)
             outside=ref.motion(t=(40.0, 0.0, 0.0)),            # every target right of the image
             gate=Ps[1],                                        # a small motion, and a gate that ends below every carried disparity (>= 4.7)
             nan=ref.motion(), inf=ref.motion())[name]
    if name == "nan":
        P[1, 2] = np.nan
    if name == "inf":
        P[0, 3] = np.inf
    if name == "gate":      # (the precondition: under the gate the maps were made with, candidates arrive; only the gate drops them)
        assert ref.splat(cam, PRM, D0, V0, P).any()
        cam = dict(cam, hi=F32(4.0))
    z = ref.splat(cam, PRM, D0, V0, P)
    assert not z.any(), name
    D, V, counts = _both(work, build, cam, PRM, Ms[1], D0, V0, P)
    assert counts["fused"] == counts["replaced"] == counts["filled"] == 0 and ref.same_bits(D, Ms[1])


def test_struct_and_entry_points_are_declared_as_the_binding_mirrors_them():
    import ctypes
    from bpvo_amd import capi
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    for struct, mirror in (("bpvo_hip_disparity_fusion", capi.DisparityFusion), ("bpvo_hip_disparity_fusion_info", capi.DisparityFusionInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in re.findall(r"\b(?:float|int|uint32_t)\s+([^;]+);", body) for n in re.findall(r"[A-Za-z_]\w*", re.sub(r"\[\d+\]", "", decl))]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert ctypes.sizeof(capi.DisparityFusion) == 20 and ctypes.sizeof(capi.DisparityFusionInfo) == 8 * 4 + 64
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("set_disparity_fusion", "get_disparity_fusion", "seq_set_disparity_fusion", "seq_get_disparity_fusion", "vo_get_fused_disparity",
                 "seq_get_fused_disparity", "vo_disparity_fusion_info", "seq_disparity_fusion_info", "fuse_disparities", "disparity_fusion_counts"):
        assert re.search(r"\bint bpvo_hip_%s\(" % name, code), name


def test_the_header_includes_no_hip_header_and_the_driver_takes_the_motion_from_one_helper():
    src = open(os.path.join(CSRC, "disparity_fusion_math.h")).read()
    assert "#include <hip" not in src and '#include "' not in src
    state = open(os.path.join(CSRC, "vo_state.h")).read()
    assert state.count("inline M44 vo_frame_motion(") == 1 and "vo_frame_motion(q, T_est" in state.split("inline void vo_finish(")[1]


def test_the_facade_surface_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "disparity_fusion_facade.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
