"""CPU-side checks of the fp32 plan's configuration surface: the ``hip_engine`` detector key and the persisted tuning key."""
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import engine as E
from realtime_video_analytics_32streams_amd.config import ConfigError, DetectorConfig, config_from_dict, load_config
from tests.conftest import GOLDEN


def test_hip_engine_default_values_and_error():
    assert DetectorConfig().hip_engine == "auto"
    for v in ("auto", "plan"):
        DetectorConfig(backend="hip", hip_engine=v).validate()
    with pytest.raises(ConfigError, match="hip_engine"):
        DetectorConfig(backend="hip", hip_engine="fp32").validate()
    cfg = config_from_dict({"streams": [{"name": "a", "url": "x"}],
                            "detector": {"backend": "hip", "half": False, "hip_engine": "plan"}})
    assert cfg.detector.hip_engine == "plan" and cfg.detector.half is False
    with pytest.raises(ConfigError, match="hip_engine"):
        config_from_dict({"streams": [{"name": "a", "url": "x"}], "detector": {"backend": "hip", "hip_engine": "fast"}})


@pytest.mark.parametrize("name", sorted(p.name for p in (GOLDEN / "reference_config").glob("*.yaml")))
def test_reference_yaml_loads_with_hip_engine_auto(name):
    cfg = load_config(GOLDEN / "reference_config" / name)
    dets = [cfg.detector] + list(getattr(cfg, "detectors", {}).values())
    assert dets and all(d.hip_engine == "auto" for d in dets)


# switches of removed experiments: their names keep their (empty) places in the key and no longer fork the cache
RETIRED = ("RVA_TUNE_IN_PLAN", "RVA_TUNE_OVERLAP", "RVA_TUNE_TOP", "RVA_TUNE_WITHIN", "RVA_HEAD_SPLIT")


def _fake_plan(monkeypatch, precision):
    """A FusedYoloV8 with just what _tuning_key reads (no GPU here)."""
    monkeypatch.setattr(torch.cuda, "get_device_name", lambda *a, **k: "AMD Instinct MI355X")
    monkeypatch.setattr(E, "_lib_digest", lambda: "0" * 64)
    for k in ("RVA_SKIP_VARIANTS", "RVA_NO_STEM2", "RVA_NO_CIN_PAD", "RVA_TUNE_LAYER_OVERLAP") + RETIRED:
        monkeypatch.delenv(k, raising=False)
    p = object.__new__(E.FusedYoloV8)
    p.dev, p.B, p.H, p.W, p.tune_overlap = torch.device("cpu"), 32, 640, 640, 4
    p._tunable = [(None, None, "32->64 k3s2 320x320"), (None, None, "64->64 k1s1 160x160")]
    if precision is not None:
        p.precision, p.f32 = precision, precision == "fp32"
    return p


def test_tuning_key_carries_precision_only_for_fp32(monkeypatch):
    legacy = _fake_plan(monkeypatch, None)._tuning_key()                # an object built before the precision argument existed
    k16 = _fake_plan(monkeypatch, "fp16")._tuning_key()
    k32 = _fake_plan(monkeypatch, "fp32")._tuning_key()
    assert k16 == legacy == "1b6d28b490bf74f328c79149"                 # the parent's key for this input: fp16 caches stay valid
    assert k32 != k16


def test_tuning_key_ignores_retired_switches(monkeypatch):
    plan = _fake_plan(monkeypatch, "fp16")
    clean = plan._tuning_key()
    for name in RETIRED:
        with monkeypatch.context() as m:
            m.setenv(name, "1")
            assert plan._tuning_key() == clean, name
    monkeypatch.setenv("RVA_SKIP_VARIANTS", "3")
    assert plan._tuning_key() != clean                                  # a switch the tuner still reads does fork it


def test_plan_flag_and_bindings():
    assert N.RVA_PLAN_F32 == 8 and {N.RVA_PLAN_NO_STEM2, N.RVA_PLAN_NO_CIN_PAD, N.RVA_PLAN_NO_PAIR32, N.RVA_PLAN_F32} == {1, 2, 4, 8}
    for name in ("rva_conv2d_nhwc_f32_v", "rva_conv_f32_num_variants", "rva_stem_conv_f32", "rva_maxpool5_nhwc_f32",
                 "rva_upsample2x_nhwc_f32", "rva_yolo_head_f32"):
        assert name in N.EXPORTS
    assert N.lib().rva_conv_f32_num_variants() >= 2
    with pytest.raises(ValueError, match="precision"):
        E.FusedYoloV8(None, 1, precision="bf16")
