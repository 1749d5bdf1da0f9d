"""irls_reduce's throughput form (C = 8; gn_irls.h), whose fused path takes the point from warp_point instead of requesting it a second time,
against everything that must not notice a change in it: the same batch run with one estimation lane and with the default lanes, with the
fused path for frozen scales on and off, at 1, 3, 130 and 300 pairs — the persistent kernel, the team kernel and the four-kernel chain
(which alone runs the throughput form; the other two keep the latency form of the same arithmetic) — must return the same poses,
statistics and tap-cache counters, bit for bit (the counters: see the comment at their assertion).  At 130 and 300 pairs every run goes
through the throughput form, so there it is compared with itself under other schedules; against independent forms it is pinned by
test_gpu_persistent.py and the reference-order tests.

The inputs mix the plane scene with the layered one (disparity holes, occlusions: invalid points and tap-cache misses), and every pair's
disparity map is cropped to a window of its own, so that the point counts of the levels are not multiples of the 256-point chunk or the
2048-point tile: the last tile of a workspace is ragged.
"""
import numpy as np
import pytest

from bpvo_amd import synth
from util import bits_equal, make_params, set_options

pytestmark = pytest.mark.gpu

PAIRS = (1, 3, 130, 300)
CASES = [pytest.param(376, 1241, 4, "bitplanes", "tukey", id="kitti-1241x376-bitplanes-tukey"),
         pytest.param(480, 640, 4, "intensity", "huber", id="640x480-intensity-huber")]


def cropped_mixed_batch(rows, cols, n):
    """n pairs, even ones from the plane scene and odd ones from the layered scene; the disparities of pair k are valid only inside a window
    whose borders depend on k (0 = no disparity: the selection takes no such pixel)."""
    half = (n + 1) // 2
    plane = synth.make_batch(rows, cols, half, first_index=700, workers=8)
    layered = synth.make_batch(rows, cols, half, first_index=700, workers=8, scene="layered")
    images = np.empty((2 * n, rows, cols), np.uint8)
    disps = np.empty((2 * n, rows, cols), np.float32)
    for k in range(n):
        src = layered if k & 1 else plane
        images[2 * k: 2 * k + 2] = src["images"][2 * (k // 2): 2 * (k // 2) + 2]
        disps[2 * k: 2 * k + 2] = src["disparities"][2 * (k // 2): 2 * (k // 2) + 2]
        top, left, bottom, right = 3 + k % 7, 5 + k % 11, 2 + k % 5, 4 + k % 13
        keep = np.zeros((rows, cols), bool)
        keep[top: rows - bottom, left: cols - right] = True
        disps[2 * k][~keep] = 0.0
    return dict(K=plane["K"], b=plane["b"], images=images, disparities=disps)


@pytest.fixture(scope="module")
def batches():
    cache = {}

    def get(rows, cols):
        if (rows, cols) not in cache:
            cache.clear()      # one size at a time: 300 pairs of 1241x376 are 1.4 GB
            cache[(rows, cols)] = cropped_mixed_batch(rows, cols, max(PAIRS))
        return cache[(rows, cols)]
    return get


def run(hip, b, rows, cols, levels, n, descriptor, loss):
    ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, descriptor=descriptor, loss=loss, levels=levels), n_frames=2 * n, n_pairs=n)
    poses, stats = ctx.batch_run(b["images"][: 2 * n], b["disparities"][: 2 * n])
    rec = dict(poses=poses, stats=stats, taps=np.array(ctx.tap_cache_counts()), fused=ctx.fused_point_counts(),
               points=[ctx.num_points(0, l) for l in range(levels)], team=ctx.team_counts(), pk=ctx.persistent_counts())
    ctx.close()
    return rec


@pytest.mark.parametrize("n", PAIRS)
@pytest.mark.parametrize("rows,cols,levels,descriptor,loss", CASES)
def test_staged_reduction_is_bit_identical_across_lanes_and_fusing(hip, batches, rows, cols, levels, descriptor, loss, n, monkeypatch):
    b = batches(rows, cols)
    recs = {}
    for fuse in (1, 0):
        for lanes in (None, 1):
            monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
            opts = dict(fuse_frozen=fuse)
            if lanes is not None:
                opts["lanes"] = lanes
            set_options(monkeypatch, **opts)
            recs[(fuse, lanes)] = run(hip, b, rows, cols, levels, n, descriptor, loss)
    ref = recs[(1, None)]
    # the tail tile is ragged: some level's point count is no multiple of the chunk, none of the finest levels' of the tile
    assert any(p % 256 for p in ref["points"]) and ref["points"][0] % 2048, ref["points"]
    if n == 1:
        assert ref["pk"][0] > 0 and ref["pk"][1] == 0, ref["pk"]      # the persistent kernel ran (the coarse levels at least)
    elif n == 3:
        assert ref["team"] > 0, ref["team"]                           # the team kernel
    else:
        assert ref["team"] == 0 and ref["pk"] == (0, 0)               # the four-kernel chain
        if descriptor == "bitplanes":
            assert ref["fused"][0] > 0                                # ... through its fused form as well
    for key, rec in recs.items():
        what = f"fuse_frozen={key[0]} lanes={key[1]}"
        assert bits_equal(ref["poses"], rec["poses"]), what
        for field in ("numIterations", "finalError", "firstOrderOptimality", "status"):
            assert np.array_equal(ref["stats"][field], rec["stats"][field]), (what, field)
        print(what, "tap-cache hits, lookups, hits and lookups of the first 8 linearisations:", rec["taps"])
        # The counters of all linearisations, [0] and [1], are kept by the median's finish and by the fused reduction (gn_median.h,
        # gn_step.h): with fuse_frozen=0 nothing counts the lookups of a workspace once its scale is frozen, so the two settings do not
        # define the same quantity (1 pair, persistent kernel, before and after this test's change alike: 2 880 627 lookups with the
        # fused path, 2 050 403 without).  They are compared between the runs of one setting; what both settings count — the first 8
        # linearisations of every level — between all four.
        same_setting = recs[(key[0], None)]
        assert np.array_equal(same_setting["taps"], rec["taps"]), (what, same_setting["taps"], rec["taps"])
        assert np.array_equal(ref["taps"][2:], rec["taps"][2:]), (what, ref["taps"], rec["taps"])
    assert len(np.unique(ref["stats"]["numIterations"][:, 0])) > 1 or n == 1
