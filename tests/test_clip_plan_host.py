"""CPU-side checks of the fp32 CNN-LSTM clip plan: weight packing (BatchNorm folded in float64), the engine rule, the FLOP
counter of tools/clip_plan_report.py and the new ABI names."""
import logging

import numpy as np
import pytest
import torch

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.clip_plan import clip_engine, clip_flops, fired_tables, pack_cnn_lstm
from realtime_video_analytics_32streams_amd.temporal import CnnLstmNet


def test_packing_folds_batchnorm_against_the_module_in_float64():
    net = synth.seeded_module(lambda: CnnLstmNet(24, 48), 7)
    p = pack_cnn_lstm(net)
    assert list(p) == list(N.CnnLstmWeights.NAMES)
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in p.values())
    x = torch.randn(2, 3, 20, 28, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    st = net.stem.double()
    with torch.no_grad():
        want1 = st[1](st[0](x))
        got1 = torch.nn.functional.conv2d(x, torch.from_numpy(p["conv1_w"]).double(), torch.from_numpy(p["conv1_b"]).double(), 2, 3)
        assert (got1 - want1).abs().max() < 1e-5
        y = st[3](st[2](want1))
        want2 = st[5](st[4](y))
        got2 = torch.nn.functional.conv2d(y, torch.from_numpy(p["conv2_w"]).double(), torch.from_numpy(p["conv2_b"]).double(), 1, 1)
        assert (got2 - want2).abs().max() < 1e-5
    r = {n: t.detach().double() for n, t in net.rnn.named_parameters()}
    assert p["w_ih1"].shape == (192, 128) and p["w_hh1"].shape == (192, 48) and p["w_ih2"].shape == (192, 48)
    assert np.array_equal(p["w_ih1"], r["weight_ih_l0"].float().numpy()) and np.array_equal(p["w_hh2"], r["weight_hh_l1"].float().numpy())
    assert np.array_equal(p["b1"], (r["bias_ih_l0"] + r["bias_hh_l0"]).float().numpy())
    assert np.array_equal(p["b2"], (r["bias_ih_l1"] + r["bias_hh_l1"]).float().numpy())
    assert np.array_equal(p["head_w"], net.head.weight.detach().numpy()) and p["head_b"].shape == (24,)


def test_engine_rule(caplog):
    assert clip_engine("cnn_lstm", False, "plan") == "clip-f32"
    assert clip_engine("cnn_lstm", False, "auto") == "torch"
    assert clip_engine("cnn_lstm", True, "auto") == "torch"
    assert clip_engine("cnn_lstm", True, "plan", has_infer_fn=True) == "infer_fn"
    with pytest.raises(ValueError, match="fp32"):
        clip_engine("cnn_lstm", True, "plan")
    for m in ("3d_cnn", "slow_fast", "conv_gru"):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert clip_engine(m, False, "plan") == "torch"
        assert any(m in r.getMessage() for r in caplog.records)
        assert clip_engine(m, False, "auto") == "torch"


def test_flop_counter():
    f = clip_flops(224, 224, 16, 512, 400)
    assert round(f["conv1_per_frame"] / 1e6) == 236 and round(f["conv2_per_frame"] / 1e6) == 462
    assert abs(f["frame"] / 1e9 - 0.70) < 0.005 and abs(f["clip"] / 1e9 - 11.2) < 0.1
    assert 0.09e9 < f["lstm"] < 0.11e9
    assert f["lstm_weight_bytes_per_step"] == 3 * 4 * 2048 * 512
    g = clip_flops(40, 56, 5, 48, 24)
    assert g["conv1_per_frame"] == 2 * 20 * 28 * 64 * 147 and g["conv2_per_frame"] == 2 * 10 * 14 * 128 * 576


def test_fired_tables():
    idx, tab = fired_tables([(2, [5, 7], (2160, 3840)), (0, [1, 3], (1080, 1920))], cols=[4, 9, 6], ring_columns=10, rows=3)
    assert idx.tolist() == [56, 76, 14, 34] and idx.dtype == np.int32
    assert tab.tolist() == [[1, 1920, 1080], [-1, 0, 0], [0, 3840, 2160]]


def test_new_names_exported():
    for name in ("rva_cnnlstm_plan_create", "rva_cnnlstm_plan_destroy", "rva_cnnlstm_plan_info", "rva_cnnlstm_plan_run",
                 "rva_cnnlstm_plan_run_post", "rva_cnnlstm_plan_stage"):
        assert name in N.EXPORTS
        assert hasattr(N.lib(), name)
