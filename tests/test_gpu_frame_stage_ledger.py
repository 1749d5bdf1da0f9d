"""The ledger of the frame stage (scripts/frame_stage_ledger.py): every descriptor form, every selection path with and without a point budget, the
levels in one launch and one by one, lazy and census-only template levels of pair batches, every placement of the normalisation, staggered lanes
and sequences with cameras of their own must come out as tests/golden/frame_stage_ledger.json recorded them: the launches and units of the frame
classes' timers, frame state, point counts and selection records, and the bytes of every array the accessors hand out.  Same kernels on the same
data in the same order on each stream: every value is exact, no tolerance applies.  The recorded file holds the script's folded form (one digest
per slot over the digests of all its arrays); `python scripts/frame_stage_ledger.py --full` prints a digest per slot, level and array, to find which
array of a slot that fails here differs between two builds."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("frame_stage_ledger", os.path.join(ROOT, "scripts", "frame_stage_ledger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_frame_stage_ledger(hip):
    with open(os.path.join(ROOT, "tests", "golden", "frame_stage_ledger.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(load_script().ledger(hip)))      # (through JSON: tuples and lists compare alike)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert sorted(got[case]) == sorted(want[case]), case
        for key in sorted(want[case]):
            assert got[case][key] == want[case][key], (case, key, got[case][key], want[case][key])
