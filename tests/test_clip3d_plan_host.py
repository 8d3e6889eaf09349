"""CPU-side checks of the fp32 3D-CNN clip plan: weight packing (BatchNorm folded in float64, kernel layouts), the engine rule
with ``hip_engine: native``, the configuration key, the FLOP counter of tools/clip3d_plan_report.py and the new ABI names."""
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.clip_plan import ENGINE_3D, clip3d_flops, clip_engine, pack_cnn3d
from realtime_video_analytics_32streams_amd.config import ConfigError, DetectorConfig, load_config
from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet, CnnLstmNet

GOLDEN = Path(__file__).resolve().parent / "golden"


def _module_layout(w):
    """[co, 27, ci] (what the MFMA kernels read) back to the module's [co, ci, 3, 3, 3]."""
    return torch.from_numpy(np.ascontiguousarray(w.transpose(0, 2, 1))).double().reshape(w.shape[0], w.shape[2], 3, 3, 3)


def test_packing_folds_batchnorm_against_the_module_in_float64():
    net = synth.seeded_module(lambda: Cnn3dNet(24), 7)
    p = pack_cnn3d(net)
    assert list(p) == list(N.Cnn3dWeights.NAMES)
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in p.values())
    assert p["conv1_w"].shape == (64, 3, 3, 3, 3) and p["conv2_w"].shape == (128, 27, 64) and p["conv3_w"].shape == (256, 27, 128)
    assert p["conv1_b"].shape == (64,) and p["conv2_b"].shape == (128,) and p["conv3_b"].shape == (256,)
    seq = net.conv3d.double()
    conv = torch.nn.functional.conv3d
    x = torch.randn(2, 3, 5, 10, 14, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with torch.no_grad():
        want1 = seq[1](seq[0](x))
        got1 = conv(x, torch.from_numpy(p["conv1_w"]).double(), torch.from_numpy(p["conv1_b"]).double(), 1, 1)
        assert (got1 - want1).abs().max() < 1e-5
        y = seq[3](seq[2](want1))
        want2 = seq[5](seq[4](y))
        got2 = conv(y, _module_layout(p["conv2_w"]), torch.from_numpy(p["conv2_b"]).double(), 1, 1)
        assert (got2 - want2).abs().max() < 1e-5
        z = seq[7](seq[6](want2))
        want3 = seq[9](seq[8](z))
        got3 = conv(z, _module_layout(p["conv3_w"]), torch.from_numpy(p["conv3_b"]).double(), 1, 1)
        assert (got3 - want3).abs().max() < 1e-5
    # tap index = (kt*3 + ky)*3 + kx, channels innermost
    w2 = _module_layout(p["conv2_w"]).numpy()
    assert p["conv2_w"][5, (1 * 3 + 2) * 3 + 0, 9] == np.float32(w2[5, 9, 1, 2, 0])
    assert np.array_equal(p["head_w"], net.fc.weight.detach().numpy()) and p["head_b"].shape == (24,)


def test_packing_refuses_other_architectures():
    with pytest.raises(ValueError, match="Cnn3dNet"):
        pack_cnn3d(synth.seeded_module(lambda: CnnLstmNet(24, 48), 7))
    net = synth.seeded_module(lambda: Cnn3dNet(24), 7)
    net.conv3d[3] = torch.nn.MaxPool3d(2, 2)
    with pytest.raises(ValueError, match="Cnn3dNet"):
        pack_cnn3d(net)


def test_engine_rule_native_table():
    assert ENGINE_3D == "clip3d-f32"
    # half: false column
    assert clip_engine("cnn_lstm", False, "native") == "clip-f32"
    for m in ("3d_cnn", "slow_fast"):
        assert clip_engine(m, False, "native") == "clip3d-f32"
        with pytest.raises(ValueError, match="fp32 plan only"):
            clip_engine(m, True, "native")
    with pytest.raises(ValueError, match="fp32 plan only"):
        clip_engine("cnn_lstm", True, "native")
    for half in (False, True):
        with pytest.raises(ValueError, match="reference defines no architecture"):
            clip_engine("conv_gru", half, "native")
        with pytest.raises(ValueError, match="no hand-written plan"):
            clip_engine("resnet", half, "native")
    # an infer_fn overrides everything, errors included
    for m in ("cnn_lstm", "3d_cnn", "slow_fast", "conv_gru", "resnet"):
        for half in (False, True):
            assert clip_engine(m, half, "native", has_infer_fn=True) == "infer_fn"


def test_engine_rule_auto_and_plan_unchanged(caplog):
    assert clip_engine("cnn_lstm", False, "plan") == "clip-f32"
    with pytest.raises(ValueError, match="hip_engine: plan runs the CNN-LSTM head as an fp32 plan only"):
        clip_engine("cnn_lstm", True, "plan")
    assert clip_engine("cnn_lstm", True, "plan", has_infer_fn=True) == "infer_fn"
    for m in ("cnn_lstm", "3d_cnn", "slow_fast", "conv_gru"):
        for half in (False, True):
            assert clip_engine(m, half, "auto") == "torch"
    for m in ("3d_cnn", "slow_fast", "conv_gru"):
        for half in (False, True):
            caplog.clear()
            with caplog.at_level(logging.WARNING):
                assert clip_engine(m, half, "plan") == "torch"
            msgs = [r.getMessage() for r in caplog.records]
            assert any(m in s and "hip_engine: plan" in s for s in msgs)
            assert any("native" in s for s in msgs) == (m != "conv_gru")     # the pointer to the strict form, where one exists


def test_config_accepts_native_and_reference_yamls_stay_auto():
    DetectorConfig(hip_engine="native").validate()
    DetectorConfig(hip_engine="plan").validate()
    with pytest.raises(ConfigError, match="hip_engine"):
        DetectorConfig(hip_engine="fp32").validate()
    assert DetectorConfig().hip_engine == "auto"
    yamls = sorted(GOLDEN.glob("*.yaml"))
    assert any(p.name == "sample-temporal-pipeline.yaml" for p in yamls)
    for path in yamls:
        cfg = load_config(path)
        assert cfg.detectors and all(d.hip_engine == "auto" for d in cfg.detectors.values()), path.name


def test_flop_counter():
    f = clip3d_flops(112, 112, 16, 400)
    assert f["conv1"] == 2 * 16 * 112 ** 2 * 64 * 81
    assert f["conv2"] == 2 * 16 * 56 ** 2 * 128 * 1728
    assert f["conv3"] == 2 * 8 * 28 ** 2 * 256 * 3456
    assert 35.3e9 < f["clip"] < 35.5e9
    assert f["pool1"] == (16, 56, 56) and f["pool2"] == (8, 28, 28)
    # floor rule: 25 x 41, T = 7 -> pool 1 keeps 12 x 20 (conv1 computes 24 x 40), pool 2 keeps 3 x 6 x 10 (conv2 computes 6 x 12 x 20)
    g = clip3d_flops(25, 41, 7, 10)
    assert g["pool1"] == (7, 12, 20) and g["pool2"] == (3, 6, 10)
    assert g["conv1"] == 2 * 7 * 24 * 40 * 64 * 81
    assert g["conv2"] == 2 * 6 * 12 * 20 * 128 * 1728
    assert g["conv3"] == 2 * 3 * 6 * 10 * 256 * 3456
    assert g["head"] == 2 * 256 * 10 and g["clip"] == g["conv1"] + g["conv2"] + g["conv3"] + g["head"]


def test_new_names_exported():
    for name in ("rva_cnn3d_plan_create", "rva_cnn3d_plan_destroy", "rva_cnn3d_plan_info", "rva_cnn3d_plan_run",
                 "rva_cnn3d_plan_run_post", "rva_cnn3d_plan_stage"):
        assert name in N.EXPORTS
        assert hasattr(N.lib(), name)
    assert "rva_clip3d.hip" in N.SOURCES
