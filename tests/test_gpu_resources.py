"""What a context takes from the device it gives back: bpvo_hip_debug_live_resources counts the device buffers, pinned buffers, streams and events
the library's owners (bpvo_amd/csrc/device_owned.h) hold, process-wide.  Every case reads the counts, creates its context, drives one family of
lazily acquired resources — and checks that the family's counts rose, so that the path is known to have run —, destroys the context and finds
the four counts where the case started.  Differences only: other contexts of the session may be alive.  The smallest shapes the library takes:
96 x 128 images (the frame-stage ledger's small camera), two pyramid levels, bit-planes."""
import gc

import numpy as np
import pytest

from bpvo_amd import capi, synth
from test_stereo import _sgm_params
from util import make_params, setup_pair

pytestmark = pytest.mark.gpu

ROWS, COLS = 96, 128
SMALL = (80, 112)      # the second camera of the mixed-size calls
DEVICE, PINNED, STREAMS, EVENTS = range(4)
KF = dict(minTranslationMagToKeyFrame=0.02, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)
# bpvo_hip_batch_run hands host buffers to the upload workers from 2 * kUploadChunkPairs = 2 * 16 pairs on (batch.hip: use_pipe)
PIPELINE_PAIRS = 32


def live(hip):
    gc.collect()      # (contexts an earlier test dropped without close() go now, not between two readings)
    return np.array(hip.debug_live_resources())


def rose(after, before, *kinds):
    return all(after[k] > before[k] for k in kinds)


def test_estimate_and_trace(hip):
    c0 = live(hip)
    ctx, _, _ = setup_pair(hip, ROWS, COLS, levels=2)
    c1 = live(hip)
    assert rose(c1, c0, DEVICE, PINNED, STREAMS, EVENTS)      # frame slabs and workspaces, the lane's staging, its stream and events
    ctx.estimate_pose(0, 0, 1)
    c2 = live(hip)
    _, _, rec = ctx.estimate_pose_trace(0, 0, 1)
    c3 = live(hip)
    assert len(rec) > 0 and c3[DEVICE] == c2[DEVICE] + 1      # the trace buffer
    ctx.estimate_pose_trace(0, 0, 1)
    assert (live(hip) == c3).all()                           # ... which the second call finds large enough
    ctx.close()
    assert (live(hip) == c0).all()


def test_add_frame_with_covariance_and_scored_start(hip):
    c0 = live(hip)
    seq = synth.make_sequence(ROWS, COLS, 4, index=5, step_rot=0.01, step_trans=0.06)
    ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, make_params(hip, levels=2, **KF), n_frames=3, n_pairs=1)
    c1 = live(hip)
    ctx.set_option("pose_covariance", 1)
    c2 = live(hip)
    assert c2[DEVICE] == c1[DEVICE] + 1 and c2[PINNED] == c1[PINNED] + 2      # the covariance scratch: one slab, two pinned blocks
    ctx.set_start_policy((capi.START_SCORED, -1, 0.5))
    clouds = 0
    for img, disp in seq["frames"]:
        if ctx.add_frame(img, disp)["hasPointCloud"]:
            clouds += len(ctx.get_point_cloud()[0]) > 0
    assert clouds > 0, "no key frame after the first: the cloud's path did not run"
    c3 = live(hip)
    # the copy stream and its event, the scoring calls' four buffers, the point cloud
    assert c3[STREAMS] > c2[STREAMS] and c3[EVENTS] > c2[EVENTS] and c3[DEVICE] >= c2[DEVICE] + 5
    ctx.close()
    assert (live(hip) == c0).all()


def test_sequences_of_two_sizes_and_their_stereo_form(hip):
    c0 = live(hip)
    cams = []
    for r, c in ((ROWS, COLS), SMALL):
        K, _ = synth.calibration(r, c)
        cams.append((np.asarray(K, np.float32).reshape(3, 3), 0.8, r, c))      # (a wide baseline: disparities of some ten pixels)
    seqs = [synth.make_stereo_sequence(r, c, 2, index=7 + s, step_rot=0.01, step_trans=0.06, camera=(K, b)) for s, (K, b, r, c) in enumerate(cams)]
    ctx = hip.create_sequences(cams, make_params(hip, levels=2, **KF))
    c1 = live(hip)
    ctx.add_frames([q["frames"][0][0] for q in seqs], [q["disps"][0] for q in seqs])
    c2 = live(hip)
    assert c2[DEVICE] >= c1[DEVICE] + 5 and c2[PINNED] >= c1[PINNED] + 4      # the sequences' job tables, counters, offsets and clouds
    ctx.add_frames_stereo([q["frames"][1][0] for q in seqs], [q["frames"][1][1] for q in seqs], ctx.default_stereo_params(16))
    c3 = live(hip)
    # block matching over two sizes: the images' and maps' scratch, the frame table (device and pinned) and its event
    assert c3[DEVICE] >= c2[DEVICE] + 6 and c3[PINNED] >= c2[PINNED] + 1 and c3[EVENTS] >= c2[EVENTS] + 1
    maps = ctx.stereo_frames(cams, [q["frames"][1][0] for q in seqs], [q["frames"][1][1] for q in seqs], _sgm_params(ctx, ndisp=16))
    c4 = live(hip)
    assert len(maps) == 2 and c4[DEVICE] == c3[DEVICE] + 1      # the semi-global matcher's cost volumes
    ctx.close()
    assert (live(hip) == c0).all()


def test_rig_of_two(hip):
    c0 = live(hip)
    X = [np.eye(4), np.eye(4)]
    X[1][0, 3] = -0.1
    seq = synth.make_rig_sequence(ROWS, COLS, 3, X, index=9, step_rot=0.01, step_trans=0.06)
    ctx = hip.create(seq["K"][0], seq["b"][0], ROWS, COLS, make_params(hip, levels=2, **KF), n_frames=6, n_pairs=2)
    ctx.rig_set(np.asarray(X, np.float32))
    c1 = live(hip)
    for frames in seq["frames"]:
        ctx.add_frames_rig([f[0] for f in frames], [f[1] for f in frames])
    c2 = live(hip)
    # estimate_rigs' staging (a device and a pinned block), the bodies' active words (likewise), the sequences' tables
    assert c2[DEVICE] >= c1[DEVICE] + 2 and c2[PINNED] >= c1[PINNED] + 2
    ctx.close()
    assert (live(hip) == c0).all()


def test_batch_from_host_buffers_starts_the_upload_workers(hip):
    c0 = live(hip)
    d = synth.make_pair(ROWS, COLS, 3)
    n = PIPELINE_PAIRS
    images = np.ascontiguousarray(np.tile(np.stack([d["imgA"], d["imgB"]]), (n, 1, 1)))
    disps = np.ascontiguousarray(np.tile(np.stack([d["dispA"], d["dispB"]]), (n, 1, 1)))
    ctx = hip.create(d["K"], d["b"], ROWS, COLS, make_params(hip, levels=2), n_frames=2 * n, n_pairs=n)
    workers = int(ctx.get_option("upload_workers"))
    assert workers > 0
    c1 = live(hip)
    ctx.batch_run(images, disps)
    c2 = live(hip)
    assert ctx.upload_stats()[1] > 0, "the upload pipeline did not run"
    # the workers' copy stream, a pinned block and two events per worker, an event per chunk, the two device staging areas
    assert c2[STREAMS] >= c1[STREAMS] + 1 and c2[PINNED] >= c1[PINNED] + workers and c2[EVENTS] >= c1[EVENTS] + 2 * workers + n // 16
    assert c2[DEVICE] >= c1[DEVICE] + 2
    ctx.batch_run(images, disps)
    assert (live(hip) == c2).all()      # a second batch of the size finds everything in place
    ctx.close()
    assert (live(hip) == c0).all()


def test_accessors_with_temporaries_hold_nothing_afterwards(hip):
    c0 = live(hip)
    ctx, _, _ = setup_pair(hip, ROWS, COLS, levels=2)
    plain = ctx.get_points(0, 0)
    ctx.set_option("points_from_compact_stream", 1)
    c1 = live(hip)
    rebuilt = ctx.get_points(0, 0)
    assert (live(hip) == c1).all()
    assert rebuilt.shape == plain.shape and len(plain) > 0 and not np.array_equal(rebuilt, np.zeros_like(rebuilt))
    J = ctx.get_jacobians(0, 0)
    assert (live(hip) == c1).all()
    assert J.size > 0 and np.isfinite(J).all()
    ctx.close()
    assert (live(hip) == c0).all()


def test_create_that_fails_on_its_options_gives_everything_back(hip, monkeypatch):
    d = synth.make_pair(ROWS, COLS, 0)
    p = make_params(hip, levels=2)
    c0 = live(hip)
    monkeypatch.setenv("BPVO_HIP_OPTIONS", "no_such_option=1")
    with pytest.raises(capi.BpvoError, match="no_such_option"):
        hip.create(d["K"], d["b"], ROWS, COLS, p, n_frames=2, n_pairs=1)
    assert (live(hip) == c0).all()
    monkeypatch.delenv("BPVO_HIP_OPTIONS")
    ctx = hip.create(d["K"], d["b"], ROWS, COLS, p, n_frames=2, n_pairs=1)      # (the same create succeeds without the variable: it did acquire)
    assert rose(live(hip), c0, DEVICE, PINNED, STREAMS, EVENTS)
    ctx.close()
    assert (live(hip) == c0).all()
