#!/usr/bin/env python3
"""Is the reported pose covariance calibrated?  The Monte-Carlo of tests/tools/pose_covariance_calibration.py (150 noisy copies of a 96x128 frame, five
descriptor / loss configurations, on the CPU checker: no GPU needed), which writes profiles/pose_covariance_calibration.json.  The tool lives under
tests/tools/ with the other tools that use the CPU checker; this is its launcher.

  python scripts/pose_covariance_calibration.py [--draws 150] [--out FILE]
"""
import os
import runpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":
    runpy.run_path(os.path.join(ROOT, "tests", "tools", "pose_covariance_calibration.py"), run_name="__main__")
