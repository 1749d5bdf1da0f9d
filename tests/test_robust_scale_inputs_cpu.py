"""The crafted inputs of tests/robust_scale_cases.py really have the properties they are built for — on the CPU oracle alone, so that
tests/test_gpu_robust_scale.py cannot silently test nothing.  Also: the oracle's sigma of every linearisation is the plain numpy rule's.

narrow-bracket (a bracket of fewer than 2^11 keys, where the digit loop of the bracketed path would end after one pass) is absent: the
bracket is never narrower than +-1 % of the median, and for a normal f32 median m x 2^e that is 0.02 m 2^23 >= 167772 keys (18 bits), whatever
e.  Fewer than 2^11 keys would take a subnormal median below 1.4e-40; residuals are differences of interpolated 8-bit or 0/1 values, whose
smallest non-zero magnitudes observed here are ~1e-14.  The narrowest bracket the rule allows, 18 bits, is what every converging level of the
suite's ordinary scenes reaches (rel at its floor); the case is dropped as the issue allows."""
import numpy as np
import pytest

import robust_scale_cases as rsc
from util import bits_equal


@pytest.fixture(scope="module")
def analysed(orc):
    out = {}

    def get(name):
        if name not in out:
            cs = rsc.case(name)
            ctx = cs.create(orc)
            walked = rsc.walk(ctx, cs, want_weights=False)
            ctx.close()
            out[name] = (cs, walked, rsc.analyse(cs, walked))
        return out[name]
    return get


@pytest.mark.parametrize("name", rsc.CASES)
def test_case_has_its_property(analysed, name):
    cs, walked, analysis = analysed(name)
    for k, rows in enumerate(analysis):      # (shown with -s, and when the property does not hold)
        for r in rows:
            print(f"  run {k}:", r["multiset"], "sigma", r["sigma"], r["path"] or "frozen")
    print(rsc.check_property(cs, analysis))


@pytest.mark.parametrize("name", rsc.CASES)
def test_oracle_sigma_is_the_plain_rule(analysed, name):
    """np.partition + the utils.h / mestimator.cc rules in numpy f32, with the freeze rule tracked in numpy: the oracle's sigma bit for bit."""
    cs, walked, analysis = analysed(name)
    for steps, rows in zip(walked, analysis):
        for k, (s, r) in enumerate(zip(steps, rows)):
            assert bits_equal(np.float32(s["sigma"]), np.float32(r["sigma"])), (name, k, s["sigma"], r["sigma"], r["multiset"])
            assert s["num_valid"] * cs.C == r["multiset"]["n"]


def test_tiny_n_starts_reach_their_counts(orc):
    """The estimates tests/test_gpu_robust_scale.py runs through every instantiation: from the start of count n, the coarse level has no valid
    point and leaves the pose alone, and the first linearisation of level 0 sees exactly n keys — n = 6 with sigma = inf."""
    cs = rsc.case("tiny-n")
    ctx = cs.create(orc)
    seen = set()
    for st in cs.starts():
        ctx.frame_set_data(1, st.cur, cs.disp)
        _, _, rec = ctx.estimate_pose_trace(0, 0, 1, st.T0)
        level0 = rec[rec[:, 67] == 0]
        assert int(level0[0, 60]) * cs.C == st.reach_n, (st.label, rec[:, 60], rec[:, 67])
        assert np.isinf(level0[0, 59]) == (st.reach_n == 6), (st.label, level0[0, 59])
        seen.add(st.reach_n)
    assert seen == {1, 2, 3, 5, 6, 7}
    ctx.close()


def test_constants_mirror_the_kernel_header():
    """The shapes this module reasons about are the ones gn_median.h declares."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "bpvo_amd", "csrc", "gn_median.h")).read()
    val = lambda n: int(re.search(r"\b%s = (\d+)" % n, src).group(1))
    assert (val("MED_THREADS"), val("MED_COPIES"), val("MED_CACHE")) == tuple(rsc.SHAPES[1024][k] for k in ("NT", "COPIES", "CACHE"))
    assert (val("MED_THREADS_B"), val("MED_COPIES_B"), val("MED_CACHE_B")) == tuple(rsc.SHAPES[512][k] for k in ("NT", "COPIES", "CACHE"))
    assert val("MED_BINS") == rsc.MED_BINS and rsc.lds_room(1024) == 18432 and rsc.lds_room(512) == 6144
    # the bracket rule at the end of median_block: first use 25 %, then gain x the relative change + floor, at most 50 %
    fl = lambda pat: np.float32(re.search(pat, src).group(1))
    assert fl(r"#define MED_REL_FLOOR ([0-9.]+)f") == rsc.REL_FLOOR and fl(r"#define MED_REL_GAIN ([0-9.]+)f") == rsc.REL_GAIN
    assert fl(r"float rel = ([0-9.]+)f;") == rsc.REL_FIRST and fl(r"rel = fminf\(([0-9.]+)f, fmaxf\(MED_REL_FLOOR") == rsc.REL_MAX
    k6 = open(os.path.join(os.path.dirname(__file__), "..", "bpvo_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"\bkChunkPoints = (\d+)", k6).group(1)) == rsc.CHUNK
