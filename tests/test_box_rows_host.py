"""CPU-side checks of the ``hip_box_rows`` option (fp32 box rows beside the fp16 head of the fused plan): the configuration
key and its default, the reference YAMLs, the new ABI names and the plan flag.  No GPU is needed."""
import ctypes
import re
from pathlib import Path

import pytest

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import config as C

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
NEW_EXPORTS = ("rva_conv1x1_head_box32_f16", "rva_yolo_head_box32_f16", "rva_yolo_head3_box32_f16", "rva_postprocess_boxes_batch",
               "rva_yolov8_plan_output_layout")


def test_hip_box_rows_defaults_to_fp16_and_validates():
    assert C.DetectorConfig().hip_box_rows == "fp16"
    for v in ("fp16", "fp32"):
        C.DetectorConfig(backend="hip", half=True, hip_box_rows=v).validate()
        C.DetectorConfig(backend="hip", half=False, hip_box_rows=v).validate()        # fp32 boxes already: accepted, no effect
    for bad in ("FP32", "float32", "", "auto", None, 32):
        with pytest.raises(C.ConfigError, match="hip_box_rows"):
            C.DetectorConfig(backend="hip", half=True, hip_box_rows=bad).validate()


def test_hip_box_rows_travels_through_config_from_dict():
    doc = {"streams": [{"name": "a", "url": "synthetic://1920x1080"}],
           "detector": {"backend": "hip", "half": True, "hip_box_rows": "fp32"},
           "detectors": {"other": {"backend": "hip", "half": True}}}
    cfg = C.config_from_dict(doc)
    assert cfg.detector.hip_box_rows == "fp32" and cfg.detectors["other"].hip_box_rows == "fp16"
    doc["detector"]["hip_box_rows"] = "fp64"
    with pytest.raises(C.ConfigError, match="hip_box_rows"):
        C.config_from_dict(doc)


def test_reference_yamls_load_with_the_default():
    files = sorted((GOLDEN / "reference_config").glob("*.yaml")) + [GOLDEN / "sample-temporal-pipeline.yaml"]
    assert len(files) == 8
    for f in files:
        cfg = C.load_config(f)
        for d in [cfg.detector] + list(cfg.detectors.values()):
            assert d.hip_box_rows == "fp16", f.name


def test_new_abi_names_are_bound_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rva.h").read_text(), flags=re.S)
    L = ctypes.CDLL(str(N.build()))
    for name in NEW_EXPORTS:
        assert name in N.EXPORTS, name
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in rva.h"
        assert hasattr(L, name), f"{name} is not exported by librva.so"
    assert hasattr(N.lib(), "rva_postprocess_boxes_batch")                             # the binding table resolves it too


def test_plan_flag_is_the_next_free_bit():
    others = [N.RVA_PLAN_NO_STEM2, N.RVA_PLAN_NO_CIN_PAD, N.RVA_PLAN_NO_PAIR32, N.RVA_PLAN_F32]
    assert N.RVA_PLAN_BOX_F32 == 16 and all(N.RVA_PLAN_BOX_F32 & o == 0 for o in others)
    assert bin(N.RVA_PLAN_BOX_F32).count("1") == 1
    defines = dict(re.findall(r"#define\s+(RVA_PLAN_[A-Z0-9_]+)\s+(\d+)", (ROOT / "include" / "rva.h").read_text()))
    assert int(defines["RVA_PLAN_BOX_F32"]) == N.RVA_PLAN_BOX_F32
    assert len(set(defines.values())) == len(defines) == 5                             # no two flags share a value
