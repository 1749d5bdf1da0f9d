"""Option lazy_template_saliency: the template frames (A) of a pair batch keep, at the levels with non-maximum suppression, their census
bytes only.  A census launch writes them, the bit-planes kernel runs over the tile columns that stay dense, the tiled selection forms
channel 0 of its windows from the census bytes and stores no saliency map; bpvo_hip_get_saliency forms the map on demand.  Everything a
caller can read must be what the parent path (option 0) gives, byte for byte.

Shapes: the smallest at which each special case of the 64-pixel tile columns exists (the blur's tiles are 64 x 8, the selection's 64 x 32)."""
import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu

LEVELS = 3
N_PAIRS = 2


def _params(hip, rows, cols):
    # NMS (radius 1) at levels 0 and 1, none at level 2: the two fine levels are the lazy ones
    return make_params(hip, levels=LEVELS, minNumPixelsForNonMaximaSuppression=(rows // 2) * (cols // 2))


def _flat_borders(images):
    """Constant columns and rows at the image border: the census is 0 on the 1-pixel border and 0xff next to it, and the blur reflects both."""
    out = images.copy()
    out[:, :, :3] = 90
    out[:, :, -3:] = 200
    out[:, :2, :] = 17
    out[:, -2:, :] = 17
    return out


def _everything(ctx, slot, poses, stats):
    rec = dict(poses=poses, stats=stats.tobytes(), iters=np.array(stats["numIterations"]))
    for l in range(LEVELS):
        rec["npts", l] = ctx.num_points(slot, l)
        rec["inds", l] = ctx.get_point_indices(slot, l)
        rec["pts", l] = ctx.get_points(slot, l)
        rec["pix", l] = ctx.get_pixels(slot, l)
        rec["jac", l] = ctx.get_jacobians(slot, l)      # the stored gradients, as Jacobian rows
        rec["sal", l] = ctx.get_saliency(slot, l)       # (formed on demand)
        rec["desc", l] = np.stack([ctx.get_descriptor_channel(slot, l, c) for c in range(8)])
    return rec


def _assert_same(a, z):
    assert a.keys() == z.keys()
    for k in a:
        if k == "stats" or (isinstance(k, tuple) and k[0] == "npts"):
            assert a[k] == z[k], k
        else:
            assert bits_equal(a[k], z[k]), k


def _run(hip, rows, cols, n, lazy_saliency, per_level=False, flat=False, first_index=40):
    """One context: a batch of OTHER images with dense records first (so that whatever the lazy forms do not write is stale, not zero), then
    the batch under test."""
    b = synth.make_batch(rows, cols, n, first_index=first_index)
    other = synth.make_batch(rows, cols, n, first_index=first_index + 37)
    images = _flat_borders(b["images"]) if flat else b["images"]
    ctx = hip.create(b["K"], b["b"], rows, cols, _params(hip, rows, cols), n_frames=2 * n, n_pairs=n)
    if per_level:
        ctx.set_option("levels_in_one_launch_max_frames", 0)      # the launches of a large batch: one per level
    ctx.set_option("lazy_template_descriptor", 0)
    ctx.batch_run(other["images"], other["disparities"])
    ctx.set_option("lazy_template_descriptor", 1)
    ctx.set_option("lazy_template_saliency", lazy_saliency)
    assert ctx.get_option("lazy_template_saliency") == float(lazy_saliency)
    return ctx, b, images


SHAPES = [
    pytest.param(60, 200, False, False, id="200x60-width-multiple-of-4-first-column-dense"),
    pytest.param(61, 201, False, False, id="201x61-three-columns-and-an-edge"),
    pytest.param(41, 137, False, False, id="137x41-last-column-narrower-than-the-margin"),
    pytest.param(40, 72, False, False, id="72x40-every-column-dense"),
    pytest.param(35, 131, False, False, id="131x35-ragged-tile-heights"),
    pytest.param(61, 201, False, True, id="201x61-constant-borders"),
    pytest.param(60, 200, True, False, id="200x60-one-launch-per-level"),
    pytest.param(35, 131, True, False, id="131x35-one-launch-per-level"),
    pytest.param(61, 201, True, False, id="201x61-one-launch-per-level"),
]


@pytest.mark.parametrize("rows,cols,per_level,flat", SHAPES)
def test_census_only_template_levels_are_bit_identical(hip, rows, cols, per_level, flat):
    out = {}
    for lazy_saliency in (0, 1):
        ctx, b, images = _run(hip, rows, cols, N_PAIRS, lazy_saliency, per_level=per_level, flat=flat)
        poses, stats = ctx.batch_run(images, b["disparities"])
        out[lazy_saliency] = _everything(ctx, 2, poses, stats)      # slot 2: the template frame of pair 1
        ctx.close()
    assert out[0]["npts", 0] > 0 and out[0]["npts", 1] > 0      # (the lazy levels select something)
    _assert_same(out[0], out[1])


def test_same_batch_twice_then_the_template_as_a_current_frame(hip):
    """The on-demand state of the map is set by every template stage and cleared by the accessor; a template slot of the batch used as the
    CURRENT frame of a later estimate gets its dense records, and the map can still be formed afterwards."""
    rows, cols, n = 61, 201, 3
    out = {}
    for lazy_saliency in (0, 1):
        ctx, b, images = _run(hip, rows, cols, n, lazy_saliency, first_index=11)
        rec = {}
        for _ in range(2):
            poses, stats = ctx.batch_run(images, b["disparities"])
        rec["poses"], rec["stats"] = poses, stats.tobytes()
        for l in range(LEVELS):
            rec["sal-first", l] = ctx.get_saliency(0, l)
            rec["sal-again", l] = ctx.get_saliency(0, l)      # (stored now)
        T, st = ctx.estimate_pose(0, 2, 0)                     # template of pair 1 against the template frame of pair 0
        rec["T"] = T
        rec["iters"] = np.array([s["numIterations"] for s in st])
        for l in range(LEVELS):
            rec["sal-after", l] = ctx.get_saliency(4, l)      # a slot whose records were never made dense
            rec["sal-cur", l] = ctx.get_saliency(0, l)
            rec["desc0", l] = ctx.get_descriptor_channel(0, l, 0)
        out[lazy_saliency] = rec
        ctx.close()
    _assert_same(out[0], out[1])
    for l in range(LEVELS):
        assert bits_equal(out[1]["sal-first", l], out[1]["sal-again", l]) and bits_equal(out[1]["sal-first", l], out[1]["sal-cur", l])


def test_map_of_replaced_data_is_refused_until_the_next_template(hip):
    """The map is formed from the slot's data: once that has been replaced the accessor says so (BPVO_ERR_NO_DATA) instead of handing out the
    map of another image; a new template stores its own map again."""
    rows, cols, n = 60, 200, 2
    ctx, b, images = _run(hip, rows, cols, n, 1)
    ctx.batch_run(images, b["disparities"])
    ctx.frame_set_data(0, b["images"][2], b["disparities"][2])
    with pytest.raises(capi.BpvoError, match="status -3"):
        ctx.get_saliency(0, 0)
    ctx.frame_set_template(0)
    for l in range(LEVELS):
        assert bits_equal(ctx.get_saliency(0, l), ctx.get_saliency(2, l)), l      # the same image, through the frame API and through the batch
    ctx.close()
