"""The compact point stream of the Gauss-Newton kernels: an 8-byte record {Z or d, x | y << 16} per template point, from which
load_point (gn_common.h) rebuilds the (X, Y, Z, 1) the selection kernels stored.  The rebuilt point must BE the stored one, bit for bit, and
everything computed from it must be what the oracle computes: no tolerance here that the suite did not already have.
"""
import numpy as np
import pytest

from bpvo_amd import synth
from util import bits_equal, make_params, normal_equations_f64, perturbed_pose

pytestmark = pytest.mark.gpu

POSES = (np.eye(4, dtype=np.float32), perturbed_pose(1.0), perturbed_pose(8.0))


def _banded(d, cols):
    """a disparity map valid on part of the image only (as test_edge_cases): point counts that are no multiple of 64 or of the 2048-point tile"""
    disp = d["dispA"].copy()
    disp[:, : cols // 3] = 0.0
    disp[::7, :] = 600.0      # above maxValidDisparity
    return disp


def _pair(b, rows, cols, levels, index=0, formulation=0, banded=False, reference=False, **kw):
    d = synth.make_pair(rows, cols, index)
    ctx = b.create(d["K"], d["b"], rows, cols, make_params(b, levels=levels, **kw), n_frames=2, n_pairs=1)
    if formulation:
        ctx.set_warp_formulation(formulation)
    if reference:
        ctx.set_option("reference_reduction", 1)
    ctx.frame_set_data(0, d["imgA"], _banded(d, cols) if banded else d["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    return ctx, d


@pytest.mark.parametrize("formulation", [0, 2], ids=["rigid-body", "disparity-space"])
@pytest.mark.parametrize("rows,cols,levels,kw", [
    pytest.param(240, 320, 4, dict(descriptor="bitplanes", loss="tukey"), id="320x240"),      # x crosses 255: both bytes of the packed coordinate
    pytest.param(96, 128, 2, dict(descriptor="bitplanes", loss="huber"), id="96x128"),        # tests/golden/bp_huber_dspace_96x128.npz's parameters
])
def test_rebuilt_points_are_the_stored_points(hip, orc, rows, cols, levels, kw, formulation):
    ch, _ = _pair(hip, rows, cols, levels, index=3, formulation=formulation, **kw)
    co, _ = _pair(orc, rows, cols, levels, index=3, formulation=formulation, **kw)
    for l in range(levels):
        ch.set_option("points_from_compact_stream", 0)
        stored = ch.get_points(0, l)
        ch.set_option("points_from_compact_stream", 1)
        rebuilt = ch.get_points(0, l)
        assert len(stored) > 0
        assert bits_equal(rebuilt, stored), f"level {l}: {int((rebuilt != stored).any(axis=-1).sum())} of {len(stored)} points differ"
        assert bits_equal(stored, co.get_points(0, l)), f"level {l}: stored points against the oracle's"
    if rows == 240:      # the packed coordinate's high bytes are in use
        assert (ch.get_point_indices(0, 0) % cols).max() > 255


@pytest.mark.parametrize("descriptor,loss", [("bitplanes", "tukey"), ("intensity", "huber"), ("fields2", "huber")], ids=["C8-tukey", "C1-huber", "C3-huber"])
def test_linearisation_is_the_oracles(hip, orc, descriptor, loss):
    """H, G, f at three poses per level on ragged templates: the reference's own sums bit for bit in reference order, and the fast mode at the
    bar of test_linearize_parity (4e-6 of an f64 evaluation of the oracle's bit-identical J, r, w, valid)."""
    rows, cols, levels = 120, 160, 3
    ch, _ = _pair(hip, rows, cols, levels, banded=True, descriptor=descriptor, loss=loss)
    cr, _ = _pair(hip, rows, cols, levels, banded=True, reference=True, descriptor=descriptor, loss=loss)
    co, _ = _pair(orc, rows, cols, levels, banded=True, descriptor=descriptor, loss=loss)
    ns = [ch.num_points(0, l) for l in range(levels)]
    assert ns == [co.num_points(0, l) for l in range(levels)]
    assert any(n % 64 for n in ns) and all(n % 2048 for n in ns), ns
    for l in range(levels):
        for T in POSES:
            a, r, b = ch.linearize(0, 0, 1, l, T), cr.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
            assert r["num_valid"] == b["num_valid"] and r["sigma"] == b["sigma"]
            assert bits_equal(r["H"], b["H"]) and bits_equal(r["G"], b["G"]), f"reference order, level {l}"
            assert np.float32(r["f_norm"]).tobytes() == np.float32(b["f_norm"]).tobytes(), (l, r["f_norm"], b["f_norm"])
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo) and a["num_valid"] == b["num_valid"]
            assert bits_equal(ch.get_residuals(0), co.get_residuals(0)), f"residuals level {l}"
            assert a["sigma"] == b["sigma"]
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, ch.Cn)
            scale = np.abs(H64).max()
            gscale = max(np.abs(G64).max(), 1e-3 * scale)
            assert np.abs(a["H"] - H64).max() <= 4e-6 * scale, f"H level {l}"
            assert np.abs(a["G"] - G64).max() <= 4e-6 * gscale, f"G level {l}"
            assert abs(a["f_norm"] - f64) <= 4e-6 * max(f64, 1e-6)


def _batch(hip, pairs, rows, cols, levels, **opts):
    n = len(pairs)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels)
    ctx = hip.create(pairs[0]["K"], pairs[0]["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    for k, v in opts.items():
        ctx.set_option(k, v)
    images = np.stack([x for d in pairs for x in (d["imgA"], d["imgB"])])
    disps = np.stack([x for d in pairs for x in (d["dispA"], d["dispB"])])
    poses, stats = ctx.batch_run(images, disps)
    teams = ctx.team_counts()
    ctx.close()
    return np.asarray(poses), [[(int(s["numIterations"]), int(s["status"]), np.float32(s["finalError"]).tobytes(),
                                 np.float32(s["firstOrderOptimality"]).tobytes()) for s in st] for st in stats], teams


def test_persistent_team_and_chain_agree(hip):
    """one pair (persistent kernel), 8 pairs (team kernel), the chain forced, and the chain with the plain reduction (fuse_frozen off):
    the same poses and statistics, bit for bit"""
    rows, cols, levels, n = 120, 160, 3, 8
    pairs = [synth.make_pair(rows, cols, 60 + i) for i in range(n)]
    team_T, team_s, teams = _batch(hip, pairs, rows, cols, levels)
    assert teams > 0
    chain_T, chain_s, teams = _batch(hip, pairs, rows, cols, levels, team=0, persistent=0)
    assert teams == 0
    plain_T, plain_s, _ = _batch(hip, pairs, rows, cols, levels, team=0, persistent=0, fuse_frozen=0)
    assert bits_equal(team_T, chain_T) and team_s == chain_s
    assert bits_equal(plain_T, chain_T) and plain_s == chain_s
    for i in (0, n - 1):
        one_T, one_s, _ = _batch(hip, pairs[i:i + 1], rows, cols, levels)      # a single pair: the persistent kernel
        assert bits_equal(one_T[0], chain_T[i]) and one_s[0] == chain_s[i], i
