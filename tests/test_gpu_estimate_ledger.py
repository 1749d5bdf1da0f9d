"""The ledger of the estimate driver (scripts/estimate_ledger.py): every path a group of pairs can take through bpvo_amd/csrc/estimate.hip — persistent
kernel, team kernel in one launch and split, the chain in its forms, reference order, channel groups, rigs, add_frames with two losses, the
fall-back reruns — must come out as tests/golden/estimate_ledger.json recorded it: iterations and status per level, the pose bytes, and the
launches it took (persistent levels, team launches, joins and give-ups, median selections by path, fused points, launches per kernel class at
profiling level 2).  The host decides its rounds from device results it has waited for, so the counts are exact: no tolerance applies."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_script():
    spec = importlib.util.spec_from_file_location("estimate_ledger", os.path.join(ROOT, "scripts", "estimate_ledger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_estimate_ledger(hip):
    with open(os.path.join(ROOT, "tests", "golden", "estimate_ledger.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(load_script().ledger(hip)))      # (through JSON: tuples and lists compare alike)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert sorted(got[case]) == sorted(want[case]), case
        for key in sorted(want[case]):
            assert got[case][key] == want[case][key], (case, key, got[case][key], want[case][key])
