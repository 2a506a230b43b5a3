#!/usr/bin/env python3
"""Extracts the key -> value content of EVERY mapper configuration file the reference ships (cfg/gaussian_mapper/**/*.yaml)
into tests/golden/mapper_cfg_values.json, keyed by the file's path relative to the reference root.

Runs only where the reference tree exists: python tests/golden/make_cfg_values_golden.py REFERENCE_ROOT.  Like
make_cfg_golden.py the fixture holds hyper-parameter VALUES (data), read with segs_slam_amd.mapper_config.read_opencv_yaml
(first occurrence of a duplicated key, comments dropped), so that tests/test_mapper_config.py covers every shipped
configuration without the reference tree present."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from segs_slam_amd import mapper_config as mc  # noqa: E402

ref = sys.argv[1]
files = sorted(glob.glob(os.path.join(ref, "cfg", "gaussian_mapper", "**", "*.yaml"), recursive=True))
out = {os.path.relpath(f, ref): mc.read_opencv_yaml(f) for f in files}
with open(os.path.join(ROOT, "tests", "golden", "mapper_cfg_values.json"), "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(out), "files")
