#!/usr/bin/env python3
"""Everything two scenarios of the batched addFrame driver leave behind, written by ONE build of the library into one .npz: run it on two builds
(an earlier commit's: scripts/build_exp.sh) on the same GPU and compare the files — a refactor of the driver leaves every array byte-identical.
The scenarios: tests/addframes_scenarios.py (every branch of the sequence driver in one call; two rigs out of step), option "pose_covariance" on.

  python tests/tools/addframes_record.py --lib bpvo_amd/csrc/libbpvo_hip.so --out a.npz
  python tests/tools/addframes_record.py --compare a.npz b.npz
"""
import argparse
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

from bpvo_amd import capi, synth  # noqa: E402


def record(lib, out):
    import addframes_scenarios as sc
    from test_gpu_rigs import INDEX, LARGE, N_FRAMES, SMALL, extrinsics
    hip = capi.Binding(os.path.abspath(lib), "bpvo_hip_")
    arrays = sc.flatten("one_call", *sc.run_one_call(hip))
    scenes = {size: synth.make_rig_sequence(size[0], size[1], N_FRAMES, [x.astype(np.float64) for x in extrinsics()], index=INDEX) for size in (LARGE, SMALL)}
    arrays.update(sc.flatten("rigs_out_of_step", *sc.run_rigs_out_of_step(hip, scenes)))
    np.savez(out, **arrays)
    print(f"{lib}: {len(arrays)} arrays, {sum(a.nbytes for a in map(np.asarray, arrays.values()))} bytes -> {out}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    differ = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        x, y = np.ascontiguousarray(A[k]), np.ascontiguousarray(B[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            differ.append(k)
    print(f"{a} against {b}: {len(A.files)} / {len(B.files)} arrays, {len(differ)} differ" + "".join("\n  " + k for k in differ[:40]))
    return 1 if differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="FILE")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    record(a.lib, a.out)
