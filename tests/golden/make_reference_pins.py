#!/usr/bin/env python3
"""Regenerates tests/golden/reference/pins.npz and tests/golden/reference/conf/ from the reference's own code, where a reference
checkout exists (`BPVO_REFERENCE=<checkout> python tests/golden/make_reference_pins.py`).

  * reference/conf/*.cfg: copies of the reference's conf/*.cfg (data: the inputs of the ConfigFile pin)
  * reference/pins.npz:   what oracle/_ref/libbpvo_ref.so (oracle/Makefile target `ref`: median, v128 census operators, ConfigFile,
    simd::dot / abs, robust_loss.h weights) returns on the seeded inputs of tests/test_reference_pins_cpu.py, and the LATCH
    sampling table of bpvo/latch_descriptor.cc (tests/test_oracle_cpu.py::test_latch_tables_agree)

The suite checks against these stored values, and against the live library too wherever oracle/_ref is built.
"""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

import make_latch_table  # noqa: E402
import test_reference_pins_cpu as pins  # noqa: E402


def main():
    ref = make_latch_table.REF
    if not os.path.isdir(os.path.join(ref, "bpvo")):
        raise SystemExit(f"no reference checkout at {ref} (set BPVO_REFERENCE)")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref", f"REF={ref}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stdout + r.stderr)
    shutil.rmtree(pins.CONF_DIR, ignore_errors=True)
    os.makedirs(pins.CONF_DIR)
    for f in sorted(glob.glob(os.path.join(ref, "conf", "*.cfg"))):
        shutil.copyfile(f, os.path.join(pins.CONF_DIR, os.path.basename(f)))
    lib = pins.bind_reference(C.CDLL(pins.REF_LIB))
    ge, census = pins.ref_census_values(lib)
    dot, absv = pins.ref_simd_values(lib)
    with tempfile.TemporaryDirectory() as tmp:
        rc, val, bad_rc, icmp = pins.ref_config_values(lib, tmp)
    val = np.where(rc == 2, "", val)                   # a throw's message names a temporary path: only its code is pinned
    table, _, _ = make_latch_table.read_reference_table()
    np.savez_compressed(pins.GOLDEN, median=pins.ref_median_values(lib), v128_ge=ge, census=census, config_rc=rc, config_value=val,
                        config_bad_rc=bad_rc, icompare=icmp, simd_dot=dot, simd_abs=absv, weights=pins.ref_weight_values(lib),
                        latch_sampling_points=np.array(table, np.int32))
    print("wrote", pins.GOLDEN, "and", len(os.listdir(pins.CONF_DIR)), "files under", pins.CONF_DIR)


if __name__ == "__main__":
    main()
