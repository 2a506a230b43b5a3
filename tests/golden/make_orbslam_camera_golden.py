#!/usr/bin/env python3
"""Extracts the scalar camera keys of three of the reference's ORB-SLAM3 settings files into
tests/golden/orbslam_camera_values.json.

Runs only where /root/reference exists.  The fixture holds calibration VALUES (data) keyed by the file they come from
(cfg/ORB_SLAM3/**/*.yaml, read with segs_slam_amd.mapper_config.read_opencv_yaml), so that the frame-intake tests can build the
cameras the reference ships where the reference tree is absent.  Only the keys CameraModel.from_settings reads, plus Camera.type,
are kept."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from segs_slam_amd import mapper_config as mc  # noqa: E402

REF = "/root/reference"
FILES = ["cfg/ORB_SLAM3/RGB-D/TUM/tum_freiburg2_xyz.yaml",          # strong five-coefficient distortion
         "cfg/ORB_SLAM3/RGB-D/RealCamera/realsense_d455_rgbd.yaml",
         "cfg/ORB_SLAM3/RGB-D/Replica/room0.yaml"]
KEYS = ("Camera.type", "Camera1.fx", "Camera1.fy", "Camera1.cx", "Camera1.cy", "Camera1.k1", "Camera1.k2", "Camera1.p1", "Camera1.p2",
        "Camera1.k3", "Camera.width", "Camera.height", "RGBD.DepthMapFactor", "Stereo.b")
out = {}
for rel in FILES:
    raw = mc.read_opencv_yaml(os.path.join(REF, rel))
    out[rel] = {k: raw[k] for k in KEYS if k in raw}
with open(os.path.join(ROOT, "tests", "golden", "orbslam_camera_values.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print({k: len(v) for k, v in out.items()})
