"""CPU-only checks of the fp16 CNN-LSTM clip plan (engine ``clip-f16``): the engine table, the config key, the packing, the
exports, and -- as tests/test_clip3d_f16_host.py does for the 3D plan -- proof that the bounds of tests/clip_f16_refs.py are met by
the reference alone and see the kernels' bug classes (each mutation must leave its bound by a factor of at least 4)."""
import ctypes
import dataclasses
import functools
import itertools
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.clip_plan import ENGINE_F16, _fold64, clip_engine, clip_flops, pack_cnn_lstm
from realtime_video_analytics_32streams_amd.config import ConfigError, DetectorConfig, load_config
from realtime_video_analytics_32streams_amd.temporal import CLIP_PLANS, CnnLstmNet
from tests import clip_f16_refs as Q
from tests import clip_stage_refs as R

FACTOR = 4.0
L_SMALL, L_RAGGED, L_ODD, L_PASSES, L_BIG = R.LSTM_SHAPES
GOLDEN = Path(__file__).resolve().parent / "golden"
NEW = ["rva_cnnlstm_f16_plan_" + n for n in ("create", "destroy", "info", "run", "run_post", "stage")]
MODELS = ("cnn_lstm", "3d_cnn", "slow_fast", "conv_gru", "resnet")


# ---------------------------------------------------------------------------------------------------------------------
# engine table, config, packing, exports
def _engine(*a, **kw):
    try:
        return clip_engine(*a, **kw)
    except ValueError as e:
        return f"ValueError: {e}"


def test_engine_table_gains_one_cell_and_nothing_else():
    assert ENGINE_F16 == "clip-f16" and ENGINE_F16 in CLIP_PLANS
    for eng in ("plan", "native"):
        assert clip_engine("cnn_lstm", True, eng, lstm_fp16=True) == "clip-f16"
        assert clip_engine("cnn_lstm", True, eng, False, False, True) == "clip-f16"
        with pytest.raises(ValueError, match="fp32 plan only"):
            clip_engine("cnn_lstm", True, eng)
    for m, half, eng, fn, c16 in itertools.product(MODELS, (False, True), ("auto", "plan", "native"), (False, True), (False, True)):
        today = _engine(m, half, eng, fn, c16)
        assert _engine(m, half, eng, fn, c16, lstm_fp16=False) == today and _engine(m, half, eng, fn, c16, False) == today
        with_key = _engine(m, half, eng, fn, c16, lstm_fp16=True)
        if m == "cnn_lstm" and half and eng in ("plan", "native") and not fn:
            assert with_key == "clip-f16" and "fp32 plan only" in today and "hip_lstm_fp16" in today
        else:
            assert with_key == today, (m, half, eng, fn, c16)
    assert _engine("cnn_lstm", True, "auto", lstm_fp16=True) == "torch"
    assert _engine("cnn_lstm", False, "plan", lstm_fp16=True) == "clip-f32"
    assert _engine("cnn_lstm", True, "plan", True, lstm_fp16=True) == "infer_fn"
    assert "fp32 plan only" in _engine("3d_cnn", True, "native", lstm_fp16=True)


def test_config_key_is_a_validated_bool_and_defaults_to_false():
    assert DetectorConfig().hip_lstm_fp16 is False
    DetectorConfig(hip_lstm_fp16=True).validate()
    for bad in ("true", 1, None, "fp16"):
        with pytest.raises(ConfigError, match="hip_lstm_fp16"):
            DetectorConfig(hip_lstm_fp16=bad).validate()
    yamls = sorted(GOLDEN.glob("*.yaml")) + sorted(GOLDEN.glob("*.yml"))
    assert yamls
    for y in yamls:
        cfg = load_config(y)
        for d in [cfg.detector, *cfg.detectors.values()]:
            assert d.hip_lstm_fp16 is False
    cfg = load_config(GOLDEN / "sample-temporal-pipeline.yaml")
    d = dataclasses.replace(cfg.detectors["temporal_cnn_lstm"], backend="hip", hip_engine="plan", half=True, hip_lstm_fp16=True)
    d.validate()
    assert d.model_type == "cnn_lstm"
    assert clip_engine(d.model_type, d.half, d.hip_engine, False, d.hip_clip_fp16, lstm_fp16=d.hip_lstm_fp16) == "clip-f16"


def test_pack_half_is_rounded_once():
    net = synth.seeded_module(lambda: CnnLstmNet(10, 48), 61)
    p16, p32 = pack_cnn_lstm(net, half=True), pack_cnn_lstm(net)
    assert list(p16) == list(p32) == list(N.CnnLstmWeights.NAMES)
    once_differs = 0
    for i, k in zip((0, 4), ("conv1_w", "conv2_w")):
        want = _fold64(net.stem[i], net.stem[i + 1])[0].numpy().astype(np.float16)          # float64 -> fp16: one rounding
        assert np.array_equal(p16[k], want.astype(np.float32))
        once_differs += int((p32[k].astype(np.float16) != want).sum())                      # float64 -> fp32 -> fp16 is NOT the same thing
    print(f"double rounding would move {once_differs} convolution weights")
    params = dict(net.rnn.named_parameters())
    for k, name in (("w_ih1", "weight_ih_l0"), ("w_hh1", "weight_hh_l0"), ("w_ih2", "weight_ih_l1"), ("w_hh2", "weight_hh_l1")):
        assert np.array_equal(p16[k], params[name].detach().numpy().astype(np.float16).astype(np.float32))
        assert not np.array_equal(p16[k], p32[k])
    for k in ("conv1_w", "conv2_w", "w_ih1", "w_hh1", "w_ih2", "w_hh2"):
        assert p16[k].dtype == np.float32 and p16[k].flags.c_contiguous and p16[k].shape == p32[k].shape
        assert np.array_equal(p16[k].astype(np.float16).astype(np.float32), p16[k])         # fp16-representable
    for k in ("conv1_b", "conv2_b", "b1", "b2", "head_w", "head_b"):
        assert np.array_equal(p16[k], p32[k])                                               # biases and the head stay fp32
    again = pack_cnn_lstm(net, half=False)
    assert again.keys() == p32.keys() and all(np.array_equal(again[k], p32[k]) for k in p32)


@pytest.mark.parametrize("name", ["conv1_w", "conv2_w", "w_ih1", "w_hh1", "w_ih2", "w_hh2"])
def test_pack_half_refuses_a_weight_beyond_fp16(name):
    net = synth.seeded_module(lambda: CnnLstmNet(10, 48), 61)
    target = {"conv1_w": net.stem[0].weight, "conv2_w": net.stem[4].weight, "w_ih1": net.rnn.weight_ih_l0, "w_hh1": net.rnn.weight_hh_l0,
              "w_ih2": net.rnn.weight_ih_l1, "w_hh2": net.rnn.weight_hh_l1}[name]
    with torch.no_grad():
        target.view(-1)[17] = 1e6
    with pytest.raises(ValueError, match=name):
        pack_cnn_lstm(net, half=True)
    pack_cnn_lstm(net)                                                       # fp32 holds it


def test_the_six_entries_are_exported():
    assert all(n in N.EXPORTS for n in NEW)
    L = ctypes.CDLL(str(N.build()))
    for n in NEW:
        assert hasattr(L, n), n
    for n in ("create", "destroy", "info", "run", "run_post", "stage"):
        new, old = getattr(N.lib(), f"rva_cnnlstm_f16_plan_{n}"), getattr(N.lib(), f"rva_cnnlstm_plan_{n}")
        assert new.argtypes == old.argtypes and new.restype == old.restype, n


def test_flops_gain_the_fp16_byte_counts():
    f32, f16 = clip_flops(224, 224, 16), clip_flops(224, 224, 16, half=True)
    assert all(f16[k] == f32[k] for k in f32 if "bytes" not in k)
    assert f16["frame_bytes"] * 2 == f32["frame_bytes"] and f16["lstm_weight_bytes_per_step"] * 2 == f32["lstm_weight_bytes_per_step"]
    assert f16["pooled_bytes_per_frame"] == 2.0 * 56 * 56 * 64 and f16["weight_bytes"] < f32["weight_bytes"]


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone meets every condition the GPU tests impose
@functools.lru_cache(maxsize=None)
def _lstm(shape):
    net, p, clips16 = Q.lstm16_case(shape)
    refs = Q.lstm16_refs(None, clips16, p, shape)
    return p, clips16, refs, {k: Q.stored(k, v[0]) for k, v in refs.items() if k != "_lstm"}


def _tiles32(v):
    return torch.stack([v[:, :, k:k + R.TILE].sum(2) for k in range(0, v.shape[2], R.TILE)], 1)


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_float64_chain_rounded_to_the_storage_types_is_inside_every_bound(shape):
    p, clips16, refs, taps = _lstm(shape)
    assert taps["pooled"].dtype == torch.float16 and all(taps[k].dtype == torch.float32 for k in Q.STAGES[1:])
    again = Q.lstm16_refs(taps, clips16, p, shape)
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k], *again[k], out=bad)
    assert not bad, bad


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_torch_fp32_arithmetic_on_the_fp16_values_is_inside_every_bound(shape):
    p, clips16, refs, taps = _lstm(shape)
    H, W, T, hidden, classes, n, _ = shape
    q = {k: v.float() for k, v in p.items()}
    got = {}
    y = F.conv2d(clips16.flatten(0, 1).float(), q["conv1_w"], q["conv1_b"], stride=2, padding=3)
    got["pooled"] = F.max_pool2d(y.relu(), 3, 2, 1).permute(0, 2, 3, 1).half()
    y = F.conv2d(taps["pooled"].float().permute(0, 3, 1, 2), q["conv2_w"], q["conv2_b"], padding=1).relu()
    got["partial"] = _tiles32(y.flatten(2))
    got["feat"] = taps["partial"].sum(1) / torch.tensor(float(y.shape[2] * y.shape[3]), dtype=torch.float32)
    got["gx"] = (taps["feat"] @ q["w_ih1"].T + q["b1"]).view(n, T, -1)
    got["h1"], got["h2"] = R.lstm(taps["gx"], p, dtype=torch.float32)
    got["logits"] = taps["h2"][T - 1] @ q["head_w"].T + q["head_b"]
    bad = []
    for k, v in got.items():
        assert v.dtype == (torch.float16 if k in Q.F16_STAGES else torch.float32)
        R.report(shape, k, v, *refs[k], out=bad)
    assert not bad, bad


@pytest.mark.parametrize("name", Q.E2E_NAMES)
def test_emulation_is_within_a_quarter_of_both_tolerances(name):
    quant, emu, orig, recorded = Q.e2e(name)[2:]
    dq, do = float(np.abs(emu - quant).max()), float(np.abs(emu - orig).max())
    dr = float(np.abs(emu - recorded).max()) if recorded is not None else 0.0
    print(f"{name}: |emulation - quantised| {dq:.3e} (TOL_Q / 4 = {Q.TOL_Q / 4:.2e}), |emulation - original| {do:.3e}, "
          f"|emulation - recorded| {dr:.3e} (TOL_O / 4 = {Q.TOL_O / 4:.2e}), smallest top-(k+1) gap {Q.top_gap(quant):.2e}")
    assert dq <= Q.TOL_Q / 4
    assert do <= Q.TOL_O / 4 and dr <= Q.TOL_O / 4
    assert Q.top_gap(quant) > 30 * max(Q.TOL_Q, Q.TOL_O) / 4
    for e, q in zip(emu, quant):
        assert Q.top(e).tolist() == Q.top(q).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds see the stem's bug classes (k_clip16_stem)
def _seen(mutated, ref, tol):
    return R.ratio(mutated, ref, tol)[0]


def _stem(shape):
    p, clips16, refs, _ = _lstm(shape)
    x = R.f64(clips16).flatten(0, 1)
    y, t = R.stem_conv(x, p)
    return p["conv1_w"], p["conv1_b"], x, y, t, refs["pooled"]


def _cols(x, kw=7):
    """The input value under tap (ci, ky, kx) of conv position (cy, cx): ``[F, 3, 7, kw, Hc, Wc]``; ``kw = 8`` adds the column the
    padded kx = 7 slot of the kernel's K layout reads."""
    F_, _, H, W = x.shape
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return F.unfold(F.pad(x, (3, 3 + kw - 7, 3, 3)), (7, kw), stride=2).view(F_, 3, 7, kw, Hc, Wc)


def _stem_one_position(shape, ym):
    """Largest distance, in bounds, that the mutated conv map ``ym`` leaves in ``pooled`` when taken at ONE conv position of one
    frame (the four positions at which it differs most are tried)."""
    w, b, x, y, t, (ref, tol) = _stem(shape)
    d = (ym.relu() - y.relu()).abs().amax(1)                              # [F, Hc, Wc]
    best = 0.0
    for i in torch.topk(d.flatten(), min(4, d.numel())).indices.tolist():
        f, cy, cx = np.unravel_index(i, tuple(d.shape))
        y2 = y.clone()
        y2[f, :, cy, cx] = ym[f, :, cy, cx]
        assert int((y2 != y).any(1).sum()) <= 1
        best = max(best, _seen(Q.pooled_ref(None, None, conv1=(y2, t))[0], ref, tol))
    return best


STEM_SHAPES = [L_RAGGED, L_ODD, L_BIG]


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=R.shape_id)
def test_stem_lane_half_row_offset_lost_in_one_chunk(shape, c=4):
    """Lane half 1 of chunk c reads the input row of lane half 0 (K row 2c) against its own weights (K row 2c + 1)."""
    w, b, x, y, t, _ = _stem(shape)
    cols = _cols(x)
    (c0, k0), (c1, k1) = divmod(2 * c, 7), divmod(2 * c + 1, 7)
    right = torch.einsum("ok,fkyx->foyx", w[:, c1, k1], cols[:, c1, k1])
    wrong = torch.einsum("ok,fkyx->foyx", w[:, c1, k1], cols[:, c0, k0])
    seen = _stem_one_position(shape, y - right + wrong)
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=R.shape_id)
def test_stem_pad_slot_kx7_given_a_weight(shape, ci=1, ky=3):
    """The padded kx = 7 slot of K row (ci, ky) multiplies input column 2 cx + 4 by the row's kx = 6 weight instead of by zero."""
    w, b, x, y, t, _ = _stem(shape)
    extra = w[:, ci, ky, 6][None, :, None, None] * _cols(x, 8)[:, ci, ky, 7][:, None]
    seen = _stem_one_position(shape, y + extra)
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=R.shape_id)
def test_stem_one_whole_chunk_dropped(shape, c=4):
    w, b, x, y, t, _ = _stem(shape)
    w2 = w.clone().flatten(1, 2)                                          # [co, 21 rows, kx]
    w2[:, 2 * c:2 * c + 2] = 0
    seen = _stem_one_position(shape, F.conv2d(x, w2.view_as(w), b, stride=2, padding=3))
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=R.shape_id)
def test_stem_zero_padding_replaced_by_edge_clamping_on_the_right_and_at_the_bottom(shape):
    w, b, x, y, t, (ref, tol) = _stem(shape)
    clamped = F.conv2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), w, b, stride=2)
    right, bottom = y.clone(), y.clone()
    right[..., -1] = clamped[..., -1]                                     # the last conv column reads input columns >= W
    bottom[..., -1, :] = clamped[..., -1, :]
    s_r = _seen(Q.pooled_ref(None, None, conv1=(right, t))[0], ref, tol)
    s_b = _seen(Q.pooled_ref(None, None, conv1=(bottom, t))[0], ref, tol)
    print(f"{R.shape_id(shape)}: right {s_r:.1f}, bottom {s_b:.1f} x bound")
    assert s_r > FACTOR and s_b > FACTOR


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_stem_pool_padding_zero_instead_of_minus_inf_is_harmless_after_relu(shape):
    """Every pool window holds a real value and every real value is >= 0 after the ReLU, so a padding of 0 gives the same max as
    -inf: this is NOT a bug class the bounds need to see, and the kernel may use either."""
    w, b, x, y, t, (ref, tol) = _stem(shape)
    zero = F.max_pool2d(F.pad(y.relu(), (1, 1, 1, 1), value=0.0), 3, 2, 0).permute(0, 2, 3, 1)
    assert torch.equal(zero, ref)


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=R.shape_id)
def test_stem_pool_window_takes_eight_of_nine(shape):
    """One pooled position (the middle of the map, every frame and channel) loses one of its nine conv values."""
    w, b, x, y, t, (ref, tol) = _stem(shape)
    Hp, Wp = ref.shape[1:3]
    py, px = Hp // 2, Wp // 2
    win = y.relu()[:, :, 2 * py - 1:2 * py + 2, 2 * px - 1:2 * px + 2].flatten(2)          # [F, 64, 9]
    assert win.shape[2] == 9 and torch.equal(win.amax(2), ref[:, py, px])
    worst = []
    for e in range(9):
        mut = ref.clone()
        mut[:, py, px] = win[:, :, [k for k in range(9) if k != e]].amax(2)
        worst.append(_seen(mut, ref, tol))
    print(f"{R.shape_id(shape)}: seen {min(worst):.1f} .. {max(worst):.1f} x bound")
    assert min(worst) > FACTOR


# ---------------------------------------------------------------------------------------------------------------------
# conv2 (k_clip16_conv2): a tile sum hides a change at one position behind the rounding of up to 256, so -- the rule of
# tests/test_clip3d_f16_host.py -- the weights a mutation touches are scaled in that test alone, on inputs for which torch's fp32
# convolution still meets the bound
def _conv2(shape):
    p, _, refs, taps = _lstm(shape)
    x = taps["pooled"].double().permute(0, 3, 1, 2)
    return x, p["conv2_w"], p["conv2_b"], R.conv2_map(taps["pooled"], p), refs["partial"]


def _conv2_one_position(shape, mutate, scale):
    x, w, b, (y, t), (ref, tol) = _conv2(shape)
    ch, tap, k = scale
    w = w.clone().flatten(2)
    w[:, ch, tap] *= k
    w = w.view(-1, 64, 3, 3)
    y, t = R.conv_bound(F.conv2d, x, w, b, 576, padding=1)
    ref, tol = R.partial_from_map(y, t)
    got = _tiles32(F.conv2d(x.float(), w.float(), b.float(), padding=1).relu().flatten(2))
    assert _seen(got, ref, tol) <= 1.0
    ym = mutate(x, w, b)
    d = (ym.relu() - y.relu()).flatten(2).abs()                          # [F, C, P]
    P = d.shape[2]
    r = (d / tol.permute(0, 2, 1)[:, :, torch.arange(P) // R.TILE]).amax(1)
    best = 0.0
    for i in torch.topk(r.flatten(), min(4, r.numel())).indices.tolist():
        f, px = divmod(i, P)
        y2 = y.clone()
        y2.flatten(2)[f, :, px] = ym.flatten(2)[f, :, px]
        assert int((y2 != y).flatten(2).any(1).sum()) == 1                # one position of one frame
        best = max(best, _seen(R.partial_from_map(y2, t)[0], ref, tol))
    return best


def _tap_dropped(x, w, b):
    w2 = w.clone().flatten(2)
    w2[:, 60:64, 8] = 0                                                  # four channels of tap (ky, kx) = (2, 2)
    return F.conv2d(x, w2.view_as(w), b, padding=1)


def _lane_half(x, w, b, c0=16, tap=4):
    """Channels c0 + 8 .. c0 + 15 of one chunk read from c0 .. c0 + 7 (lane half 1 without its offset), at tap 4 (the centre)."""
    ky, kx = divmod(tap, 3)
    xs = F.pad(x, (1, 1, 1, 1))[:, :, ky:ky + x.shape[2], kx:kx + x.shape[3]]
    wt = w.flatten(2)[:, :, tap]                                         # [co, ci]
    right = torch.einsum("oc,ncyx->noyx", wt[:, c0 + 8:c0 + 16], xs[:, c0 + 8:c0 + 16])
    wrong = torch.einsum("oc,ncyx->noyx", wt[:, c0 + 8:c0 + 16], xs[:, c0:c0 + 8])
    return F.conv2d(x, w, b, padding=1) - right + wrong


def _chunk_dropped(x, w, b, c0=32, tap=4):
    w2 = w.clone().flatten(2)
    w2[:, c0:c0 + 16, tap] = 0
    return F.conv2d(x, w2.view_as(w), b, padding=1)


CONV2_SHAPES = [L_RAGGED, L_ODD, L_PASSES, L_BIG]
CONV2_MUTATIONS = {"tap_dropped": (_tap_dropped, (slice(60, 64), 8, 16.0)), "lane_half": (_lane_half, (slice(24, 32), 4, 16.0)),
                   "chunk_dropped": (_chunk_dropped, (slice(32, 48), 4, 8.0))}


@pytest.mark.parametrize("shape", CONV2_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("name", list(CONV2_MUTATIONS))
def test_conv2_mutation_at_one_position(name, shape):
    mutate, scale = CONV2_MUTATIONS[name]
    seen = _conv2_one_position(shape, mutate, scale)
    print(f"{name} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_conv2_last_position_left_out_of_its_tile_sum(shape):
    x, w, b, (y, t), (ref, tol) = _conv2(shape)
    y2 = y.clone().flatten(2)
    y2[:, :, -1] = 0
    seen = _seen(R.partial_from_map(y2.view_as(y), t)[0], ref, tol)
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


# ---------------------------------------------------------------------------------------------------------------------
# LSTM and head
def _lstm_seen(shape, mut):
    p, _, refs, taps = _lstm(shape)
    h1, h2 = R.lstm(taps["gx"], p, mut=mut)
    e_ref, bound = refs["_lstm"]
    d = max(float((h1 - refs["h1"][0]).abs().max()), float((h2 - refs["h2"][0]).abs().max()))
    print(f"{R.shape_id(shape)} {mut}: e_ref {e_ref:.3e}, bound {bound:.3e}, mutation moves h by {d:.3e} = {d / bound:.0f} x bound")
    return d / bound


@pytest.mark.parametrize("shape", [L_PASSES, L_BIG], ids=R.shape_id)                        # more than 8 clips, T >= 2
def test_lstm_cell_state_read_as_zero_from_clip_8(shape):
    assert shape[5] > 8 and shape[2] >= 2
    assert _lstm_seen(shape, "c0_from_8") > FACTOR


@pytest.mark.parametrize("shape", [L_RAGGED, L_ODD, L_PASSES, L_BIG], ids=R.shape_id)
def test_lstm_layer_2_reads_the_wrong_step_of_h1(shape):
    assert _lstm_seen(shape, "l2_next") > FACTOR


@pytest.mark.parametrize("shape", R.LSTM_SHAPES, ids=R.shape_id)
def test_head_drops_the_last_k(shape):
    p, _, refs, taps = _lstm(shape)
    q = dict(p)
    q["head_w"] = p["head_w"].clone()
    q["head_w"][:, -1] = 0
    seen = _seen(R.head(taps["h2"].double()[shape[2] - 1], q)[0], *refs["logits"])
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR
