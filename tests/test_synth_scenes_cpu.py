"""The synthetic scenes themselves (bpvo_amd/synth.py), no GPU.

* The plane scene is pinned: sha256 digests of what the generators returned before the layered scene was added.  bench.py's inputs are
  make_batch(376, 1241, ...) plane pairs, so this test guards the benchmark's inputs byte for byte.
* The layered scene does what its docstring claims, at both full sizes over indices 0-15: determinism, hole share, visible layers,
  disparity = b * fx / depth at every valid pixel, labels that survive the projection with T_gt, occlusion present.
"""
import hashlib

import numpy as np
import pytest

from bpvo_amd import synth

FULL_SIZES = [pytest.param(480, 640, id="640x480"), pytest.param(376, 1241, id="1241x376")]


def digest(obj):
    """sha256 over a generator's output: arrays by dtype, shape and bytes, dict keys sorted, other values by repr."""
    h = hashlib.sha256()

    def add(x):
        if isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode())
                add(x[k])
        elif isinstance(x, (list, tuple)):
            for v in x:
                add(v)
        elif isinstance(x, np.ndarray):
            h.update(str(x.dtype).encode())
            h.update(str(x.shape).encode())
            h.update(np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())
    add(obj)
    return h.hexdigest()


PLANE_DIGESTS = [
    (lambda: synth.make_pair(480, 640, 0), "007bbd645b7b1fe385a49cf4d1f1ae22f74044467922b8154b585615b74a27d0"),
    (lambda: synth.make_pair(376, 1241, 7), "061e85f8c67b7bc3a4303f5eeb5dec128ed028d6bd8d2f7103b717808edee500"),
    (lambda: synth.make_batch(376, 1241, 3), "2085d91d649ae5cff88788570e1083d01d1665c1f56e6de325c768f01881cbb8"),
    (lambda: synth.make_sequence(120, 160, 3), "c5717715c615cf50af354b2aba979e3975d2d78ae37f910d647d112d97814589"),
    (lambda: synth.make_stereo_pair(376, 1241, 4, z0=8.0), "cabd00d5b30ef54846b5e2e6064c7e49dbd13b6d754a418c4fb269036fca27a7"),
]


@pytest.mark.parametrize("k", range(len(PLANE_DIGESTS)), ids=["make_pair-640x480-0", "make_pair-1241x376-7", "make_batch-1241x376-3",
                                                            "make_sequence-160x120-3", "make_stereo_pair-1241x376-4"])
def test_the_plane_scene_is_pinned(k):
    make, want = PLANE_DIGESTS[k]
    assert digest(make()) == want
    assert digest(make()) == want           # and it does not depend on what ran before


def test_the_scene_argument_defaults_to_the_plane_and_refuses_unknown_names():
    assert digest(synth.make_pair(120, 160, 3, scene="plane")) == digest(synth.make_pair(120, 160, 3))
    assert digest(synth.make_stereo_pair(60, 90, 2, z0=3.0, scene="plane")) == digest(synth.make_stereo_pair(60, 90, 2, z0=3.0))
    for make in (lambda: synth.make_pair(60, 80, 0, scene="planes"), lambda: synth.make_batch(60, 80, 1, scene="x"),
                 lambda: synth.make_sequence(60, 80, 2, scene=""), lambda: synth.make_stereo_pair(60, 80, 0, scene="Layered")):
        with pytest.raises(ValueError):
            make()


def _valid(disp):
    """the template's disparity gate with the default parameters (minValidDisparity 0.001f, maxValidDisparity 512)"""
    return (disp >= np.float32(0.001)) & (disp <= np.float32(512.0))


def _touches(lab, i, j):
    a = ((lab[:, 1:] == i) & (lab[:, :-1] == j)) | ((lab[:, 1:] == j) & (lab[:, :-1] == i))
    b = ((lab[1:, :] == i) & (lab[:-1, :] == j)) | ((lab[1:, :] == j) & (lab[:-1, :] == i))
    return bool(a.any() or b.any())


# Measured over indices 0-15 at both full sizes: occluded share of A's valid pixels 1.0 % - 3.5 % (mean ~2.2 %); the floor is half the minimum.
OCCLUDED_FLOOR = 0.005
OCCLUDED_MEAN_FLOOR = 0.015


@pytest.mark.parametrize("rows,cols", FULL_SIZES)
def test_the_layered_scene_does_what_it_claims(rows, cols):
    lo, hi = synth.default_disp_range(rows, cols)
    occ_shares = []
    for i in range(16):
        d = synth.make_pair(rows, cols, i, scene="layered")
        K, b = d["K"], d["b"]
        # the motion is make_pair's: the scene is the only thing that differs
        assert np.array_equal(d["T_gt"], synth.make_pair(16, 16, i)["T_gt"]) and np.array_equal(d["twist"], synth.make_pair(16, 16, i)["twist"])
        for key in ("imgA", "imgB"):
            assert d[key].dtype == np.uint8 and d[key].shape == (rows, cols)
        for key in ("dispA", "dispB"):
            assert d[key].dtype == np.float32 and d[key].shape == (rows, cols)
            inv = ~_valid(d[key])
            assert 0.05 <= inv.mean() <= 0.15, (i, key, inv.mean())
            assert set(np.unique(d[key][inv]).tolist()) == set(synth.HOLE_VALUES), (i, key)
        lab = d["layerA"]
        assert lab.min() == 0 and len(np.unique(lab)) >= 3, (i, np.unique(lab))
        assert (lab == 0).any() and len(np.unique(d["layerB"])) >= 3
        assert any(_touches(lab, p, q) for p in range(1, lab.max() + 1) for q in range(p + 1, lab.max() + 1)), (i, "no two patches meet in A")
        # disparity = b * fx / depth (the renderer's f32 rounding of the f64 quotient) at every valid pixel
        valid = _valid(d["dispA"])
        want = (b * float(K[0, 0]) / d["depthA"]).astype(np.float32)
        assert np.array_equal(d["dispA"][valid], want[valid]), i
        assert want.min() >= lo * (1 - 1e-6) and want.max() <= hi, (i, want.min(), want.max())
        # every depth edge of A lies inside the hole band
        edge = np.zeros_like(valid)
        dx = lab[:, 1:] != lab[:, :-1]
        edge[:, 1:] |= dx
        edge[:, :-1] |= dx
        assert not (edge & valid).any(), i
        # valid, non-occluded pixels of A projected with T_gt land on their own layer in B (nearest pixel: the misses sit on edges)
        ys, xs = np.nonzero(valid & ~d["occluded"])
        z = d["depthA"][ys, xs]
        X = np.stack([(xs - K[0, 2]) / K[0, 0] * z, (ys - K[1, 2]) / K[1, 1] * z, z], -1)
        XB = X @ d["T_gt"][:3, :3].T + d["T_gt"][:3, 3]
        u = np.rint(K[0, 0] * XB[:, 0] / XB[:, 2] + K[0, 2]).astype(np.int64)
        v = np.rint(K[1, 1] * XB[:, 1] / XB[:, 2] + K[1, 2]).astype(np.int64)
        assert ((u >= 0) & (u < cols) & (v >= 0) & (v < rows)).all()
        same = (d["layerB"][v, u] == lab[ys, xs]).mean()
        assert same >= 0.99, (i, same)
        occ_shares.append(d["occluded"][valid].mean())
        assert occ_shares[-1] >= OCCLUDED_FLOOR, (i, occ_shares[-1])
        # deterministic, every output
        if i < 2:
            again = synth.make_pair(rows, cols, i, scene="layered")
            for key in d:
                assert digest(d[key]) == digest(again[key]), (i, key)
    assert np.mean(occ_shares) >= OCCLUDED_MEAN_FLOOR, occ_shares


def test_layered_batches_sequences_and_stereo_pairs():
    rows, cols = 120, 160
    bt = synth.make_batch(rows, cols, 3, first_index=5, scene="layered", workers=2)
    for p in range(3):
        d = synth.make_pair(rows, cols, 5 + p, scene="layered")
        assert np.array_equal(bt["images"][2 * p], d["imgA"]) and np.array_equal(bt["images"][2 * p + 1], d["imgB"])
        assert bt["disparities"][2 * p].tobytes() == d["dispA"].tobytes() and bt["disparities"][2 * p + 1].tobytes() == d["dispB"].tobytes()
        assert np.array_equal(bt["T_gt"][p], d["T_gt"])
    # a sequence: the plane sequence's trajectory; its first frame is pair A of the same index
    seq = synth.make_sequence(rows, cols, 4, index=2, scene="layered")
    plane = synth.make_sequence(rows, cols, 4, index=2)
    assert all(np.array_equal(a, b) for a, b in zip(seq["poses"], plane["poses"]))
    d = synth.make_pair(rows, cols, 2, scene="layered")
    assert np.array_equal(seq["frames"][0][0], d["imgA"]) and seq["frames"][0][1].tobytes() == d["dispA"].tobytes()
    for img, disp in seq["frames"]:
        assert 0.04 <= (~_valid(disp)).mean() <= 0.2
    # stereo: the true disparity of the left image, the right camera one baseline along +x
    st = synth.make_stereo_pair(rows, cols, 2, scene="layered", disp_range=(2.0, 13.0))
    assert st["left"].dtype == np.uint8 and st["disp"].min() >= 2.0 * (1 - 1e-6) and st["disp"].max() <= 13.0
    assert _valid(st["disp"]).all()
    assert 0.0 < st["occluded"].mean() < 0.3
    lab = st["layer"]
    ys, xs = np.nonzero(~st["occluded"])
    xr = np.rint(xs - st["disp"][ys, xs]).astype(np.int64)     # the matching pixel of the right image
    assert (xr >= 0).all()
    st2 = synth.make_stereo_pair(rows, cols, 2, scene="layered", disp_range=(2.0, 13.0))
    assert digest(st) == digest(st2)


def test_layered_batch_rendering_time():
    """128 pairs at 1241x376 render in well under 30 s with 8 workers (measured ~11 s; ~0.7 s per pair on one CPU).  Checked on 2 pairs
    with one worker, against a generous per-pair bound."""
    import time
    t = time.perf_counter()
    synth.make_batch(376, 1241, 2, first_index=40, scene="layered")
    per_pair = (time.perf_counter() - t) / 2
    assert per_pair < 3.0, per_pair
