"""CPU-side checks of ``hip_plan_capacity`` (one YOLOv8 plan of N images that serves every live-stream count of a tick): the
configuration key, its default and validation, the reference YAMLs, and the four new ABI names.  No GPU is needed."""
import ctypes
import re
from pathlib import Path

import pytest

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import config as C

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW_EXPORTS = ("rva_yolov8_plan_run_n", "rva_yolov8_plan_run_lanes_n", "rva_yolov8_plan_run_range_n", "rva_yolov8_plan_primed_images")


def test_hip_plan_capacity_defaults_to_0_and_validates():
    assert C.DetectorConfig().hip_plan_capacity == 0
    for v in (0, 1, 4, 32):
        C.DetectorConfig(backend="hip", half=True, hip_plan_capacity=v).validate()
        C.DetectorConfig(backend="hip", half=False, hip_engine="plan", hip_plan_capacity=v).validate()
        C.DetectorConfig(backend="hip", half=False, hip_plan_capacity=v).validate()      # PyTorch-ROCm engine: accepted, no effect
    for bad in (-1, -32, "4", 2.5, None, True):
        with pytest.raises(C.ConfigError, match="hip_plan_capacity"):
            C.DetectorConfig(backend="hip", half=True, hip_plan_capacity=bad).validate()


def test_hip_plan_capacity_travels_through_config_from_dict():
    doc = {"streams": [{"name": "a", "url": "synthetic://1920x1080"}],
           "detector": {"backend": "hip", "half": True, "hip_plan_capacity": 32},
           "detectors": {"other": {"backend": "hip", "half": True}}}
    cfg = C.config_from_dict(doc)
    assert cfg.detector.hip_plan_capacity == 32 and cfg.detectors["other"].hip_plan_capacity == 0
    doc["detector"]["hip_plan_capacity"] = -1
    with pytest.raises(C.ConfigError, match="hip_plan_capacity"):
        C.config_from_dict(doc)


def test_reference_yamls_load_with_the_default():
    files = sorted((GOLDEN / "reference_config").glob("*.yaml"))
    assert files
    for f in files:
        cfg = C.load_config(f)
        for d in [cfg.detector] + list(cfg.detectors.values()):
            assert d.hip_plan_capacity == 0, f.name


def test_new_abi_names_are_bound_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rva.h").read_text(), flags=re.S)
    L = ctypes.CDLL(str(N.build()))
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS, name
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in rva.h"
        assert hasattr(L, name), f"{name} is not exported by librva.so"
    assert L.rva_abi_version() == 1                                                    # additive: the version stays
    # the _n forms carry the image count right behind `output`
    for name in NEW_EXPORTS[:3]:
        decl = re.search(rf"\b{name}\s*\(([^;]*)\);", text).group(1)
        assert re.search(r"void \*output,\s*int n,", decl), decl
