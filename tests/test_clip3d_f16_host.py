"""CPU-only checks of the fp16 3D-CNN clip plan (engine ``clip3d-f16``): the engine table, the config key, the packing, the
exports, and -- as tests/test_clip_stages_host.py does for the fp32 plans -- proof that the bounds of tests/clip3d_f16_refs.py are
met by the reference alone and see the kernels' bug classes (each mutation must leave its bound by a factor of at least 4)."""
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
from realtime_video_analytics_32streams_amd.clip_plan import ENGINE_3D_F16, _fold64, clip_engine, pack_cnn3d
from realtime_video_analytics_32streams_amd.config import ConfigError, DetectorConfig, load_config
from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet
from tests import clip3d_f16_refs as Q
from tests import clip_stage_refs as R

FACTOR = 4.0
C_ONE, C_ODD, C_RAGGED = R.C3D_SHAPES
GOLDEN = Path(__file__).resolve().parent / "golden"
NEW = ["rva_cnn3d_f16_plan_" + n for n in ("create", "destroy", "info", "run", "run_post", "stage")]


# ---------------------------------------------------------------------------------------------------------------------
# engine table, config, packing, exports
def _engine(*a, **kw):
    try:
        return clip_engine(*a, **kw)
    except ValueError as e:
        return f"ValueError: {e}"


def test_engine_table_gains_one_cell_and_nothing_else():
    assert ENGINE_3D_F16 == "clip3d-f16"
    for m in ("3d_cnn", "slow_fast"):
        assert clip_engine(m, True, "native", clip_fp16=True) == "clip3d-f16"
        assert clip_engine(m, True, "native", False, True) == "clip3d-f16"
        with pytest.raises(ValueError, match="fp32 plan only"):
            clip_engine(m, True, "native")
    for m, half, eng, fn in itertools.product(("cnn_lstm", "3d_cnn", "slow_fast", "conv_gru", "resnet"), (False, True),
                                              ("auto", "plan", "native"), (False, True)):
        without, with_key = _engine(m, half, eng, fn), _engine(m, half, eng, fn, clip_fp16=True)
        assert _engine(m, half, eng, fn, clip_fp16=False) == without
        if m in ("3d_cnn", "slow_fast") and half and eng == "native" and not fn:
            assert with_key == "clip3d-f16" and "fp32 plan only" in without
        else:
            assert with_key == without, (m, half, eng, fn)
    assert "fp32 plan only" in _engine("cnn_lstm", True, "native", clip_fp16=True)
    assert "fp32 plan only" in _engine("cnn_lstm", True, "plan", clip_fp16=True)
    assert _engine("3d_cnn", True, "plan", clip_fp16=True) == "torch" and _engine("3d_cnn", True, "auto", clip_fp16=True) == "torch"
    assert _engine("3d_cnn", False, "native", clip_fp16=True) == "clip3d-f32"
    assert _engine("3d_cnn", True, "native", True, True) == "infer_fn"


def test_config_key_is_a_validated_bool_and_defaults_to_false():
    assert DetectorConfig().hip_clip_fp16 is False
    DetectorConfig(hip_clip_fp16=True).validate()
    for bad in ("true", 1, None, "fp16"):
        with pytest.raises(ConfigError, match="hip_clip_fp16"):
            DetectorConfig(hip_clip_fp16=bad).validate()
    yamls = sorted(GOLDEN.glob("*.yaml")) + sorted(GOLDEN.glob("*.yml"))
    assert yamls
    for y in yamls:
        cfg = load_config(y)
        for d in [cfg.detector, *cfg.detectors.values()]:
            assert d.hip_clip_fp16 is False
    cfg = load_config(GOLDEN / "sample-temporal-pipeline.yaml")
    d = dataclasses.replace(cfg.detectors["temporal_slowfast"], backend="hip", hip_engine="native", hip_clip_fp16=True)
    d.validate()
    assert d.half is True and clip_engine(d.model_type, d.half, d.hip_engine, False, d.hip_clip_fp16) == "clip3d-f16"


def test_pack_half_is_a_float64_fold_rounded_once():
    net = synth.seeded_module(lambda: Cnn3dNet(10), 61)
    p16, p32 = pack_cnn3d(net, half=True), pack_cnn3d(net)
    assert sorted(p16) == sorted(p32) == sorted(N.Cnn3dWeights.NAMES)
    once_differs = 0
    for i, k in zip((0, 4, 8), ("conv1_w", "conv2_w", "conv3_w")):
        w64 = _fold64(net.conv3d[i], net.conv3d[i + 1])[0].numpy()
        if k != "conv1_w":
            w64 = w64.reshape(w64.shape[0], w64.shape[1], 27).transpose(0, 2, 1)
        want = w64.astype(np.float16)                                       # float64 -> fp16: one rounding
        assert p16[k].dtype == np.float32 and p16[k].flags.c_contiguous and p16[k].shape == p32[k].shape
        assert np.array_equal(p16[k].astype(np.float16).astype(np.float32), p16[k])         # fp16-representable
        assert np.array_equal(p16[k], want.astype(np.float32))
        once_differs += int((p32[k].astype(np.float16) != want).sum())      # float64 -> fp32 -> fp16 is NOT the same thing
    print(f"double rounding would move {once_differs} weights")
    for k in ("conv1_b", "conv2_b", "conv3_b", "head_w", "head_b"):
        assert np.array_equal(p16[k], p32[k])                               # biases and the head stay fp32
    assert pack_cnn3d(net, half=False).keys() == p32.keys() and all(np.array_equal(pack_cnn3d(net, half=False)[k], p32[k]) for k in p32)


def test_pack_half_refuses_a_weight_beyond_fp16():
    net = synth.seeded_module(lambda: Cnn3dNet(10), 61)
    with torch.no_grad():
        net.conv3d[4].weight[5, 7, 1, 1, 1] = 1e6
    with pytest.raises(ValueError, match="conv2_w"):
        pack_cnn3d(net, half=True)
    pack_cnn3d(net)                                                          # fp32 holds it


def test_the_six_entries_are_exported():
    assert all(n in N.EXPORTS for n in NEW)
    L = ctypes.CDLL(str(N.build()))
    for n in NEW:
        assert hasattr(L, n), n
    assert N.lib().rva_cnn3d_f16_plan_stage.argtypes == N.lib().rva_cnn3d_plan_stage.argtypes


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone meets every condition the GPU tests impose
@functools.lru_cache(maxsize=None)
def _c3d(shape):
    net, p, frames16 = Q.c3d16_case(shape)
    refs = Q.c3d16_refs(None, frames16, p, shape)
    return p, frames16, refs, {k: Q.stored(k, v[0]) for k, v in refs.items()}


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_float64_chain_rounded_to_the_storage_types_is_inside_every_bound(shape):
    p, frames16, refs, taps = _c3d(shape)
    assert taps["act1"].dtype == taps["act2"].dtype == torch.float16 and taps["partial"].dtype == torch.float32
    again = Q.c3d16_refs(taps, frames16, p, shape)
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k], *again[k], out=bad)
    assert not bad, bad


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_torch_fp32_arithmetic_on_the_fp16_values_is_inside_every_bound(shape):
    p, frames16, refs, taps = _c3d(shape)
    T, H, W, classes, n, _ = shape
    thw = (T // 2, H // 4, W // 4)
    q = {k: v.float() for k, v in p.items()}
    got = {}
    y = F.conv3d(frames16.float().permute(0, 2, 1, 3, 4), q["conv1_w"], q["conv1_b"], padding=1)
    got["act1"] = F.max_pool3d(y.relu(), (1, 2, 2)).permute(0, 2, 3, 4, 1).half()
    y = F.conv3d(taps["act1"].float().permute(0, 4, 1, 2, 3), q["conv2_w"], q["conv2_b"], padding=1)
    got["act2"] = F.max_pool3d(y.relu(), 2).permute(0, 2, 3, 4, 1).flatten(1, 3).half()
    y = F.conv3d(taps["act2"].float().view(n, *thw, 128).permute(0, 4, 1, 2, 3), q["conv3_w"], q["conv3_b"], padding=1).relu()
    got["partial"] = torch.stack([y.flatten(2)[:, :, k:k + R.TILE].sum(2) for k in range(0, y.flatten(2).shape[2], R.TILE)], 1)
    got["feat"] = taps["partial"].sum(1) / torch.tensor(float(thw[0] * thw[1] * thw[2]), dtype=torch.float32)
    got["logits"] = taps["feat"] @ q["head_w"].T + q["head_b"]
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
    gap = min(float(np.min(np.sort(r)[::-1][:min(5, len(r) - 1)] - np.sort(r)[::-1][1:min(5, len(r) - 1) + 1])) for r in quant)
    print(f"{name}: |emulation - quantised| {dq:.2e} (TOL_Q / 4 = {Q.TOL_Q / 4:.2e}), |emulation - original| {do:.2e}, "
          f"|emulation - recorded| {dr:.2e} (TOL_O / 4 = {Q.TOL_O / 4:.2e}), smallest top-(k+1) gap {gap:.2e}")
    assert dq <= Q.TOL_Q / 4
    assert do <= Q.TOL_O / 4 and dr <= Q.TOL_O / 4
    for e, q in zip(emu, quant):
        assert Q.top(e).tolist() == Q.top(q).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds see the kernels' bug classes
def _seen(mutated, ref, tol):
    return R.ratio(mutated, ref, tol)[0]


def _conv2(shape):
    p, _, refs, taps = _c3d(shape)
    x = taps["act1"].double().permute(0, 4, 1, 2, 3)
    return x, p["conv2_w"], p["conv2_b"], R.c3d_conv2(taps["act1"], p), refs["act2"], 1728


def _conv3(shape):
    p, _, refs, taps = _c3d(shape)
    T, H, W, _, n, _ = shape
    thw = (T // 2, H // 4, W // 4)
    x = taps["act2"].double().view(n, *thw, 128).permute(0, 4, 1, 2, 3)
    return x, p["conv3_w"], p["conv3_b"], R.c3d_conv3(taps["act2"], p, thw), refs["partial"], 3456


def _finish(case, y, t):
    return Q.act2_ref(None, None, conv2=(y, t))[0] if case is _conv2 else R.partial_from_map(y, t)[0]


def _bound(case, y, t):
    return Q.act2_ref(None, None, conv2=(y, t)) if case is _conv2 else R.partial_from_map(y, t)


def _tiles32(v):
    return torch.stack([v[:, :, k:k + R.TILE].sum(2) for k in range(0, v.shape[2], R.TILE)], 1)


def _mutate_one_position(case, shape, mutate, scale=None):
    """Largest distance, in bounds, that ``mutate`` applied to the convolution at ONE output position of one clip leaves in the
    stage's output.  ``scale``: (slice of input channels, tap, factor) multiplying those weights first -- the inputs of that test
    only, on which torch's fp32 convolution must still meet the bound."""
    x, w, b, (y, t), (ref, tol), n = case(shape)
    if scale is not None:
        ch, tap, k = scale
        w = w.clone().flatten(2)
        w[:, ch, tap] *= k
        w = w.view(-1, x.shape[1], 3, 3, 3)
        y, t = R.conv_bound(F.conv3d, x, w, b, n, padding=1)
        ref, tol = _bound(case, y, t)
        got = F.conv3d(x.float(), w.float(), b.float(), padding=1).relu()
        got = F.max_pool3d(got, 2).permute(0, 2, 3, 4, 1).flatten(1, 3).half() if case is _conv2 else _tiles32(got.flatten(2))
        assert _seen(got, ref, tol) <= 1.0
    ym = mutate(x, w, b)
    d = (ym.relu() - y.relu()).abs()
    if case is _conv2:                      # a position counts through its pool group: the candidates by |change| / group's bound
        N_, C_, T_, H_, W_ = y.shape
        T2, H2, W2 = T_ // 2, H_ // 2, W_ // 2
        up = tol.view(N_, T2, H2, W2, C_).permute(0, 4, 1, 2, 3)
        for dim in (2, 3, 4):
            up = up.repeat_interleave(2, dim)
        r = torch.zeros_like(d[:, 0])
        r[:, :2 * T2, :2 * H2, :2 * W2] = (d[:, :, :2 * T2, :2 * H2, :2 * W2] / up).amax(1)
    else:                                   # behind a tile sum: |change| / the tile's bound
        P = d.flatten(2).shape[2]
        r = (d.flatten(2) / tol.permute(0, 2, 1)[:, :, torch.arange(P) // R.TILE]).amax(1).view_as(d[:, 0])
    best = 0.0
    for i in torch.topk(r.flatten(), 4).indices.tolist():
        at = np.unravel_index(i, tuple(r.shape))
        at = (at[0], slice(None)) + tuple(at[1:])
        y2 = y.clone()
        y2[at] = ym[at]
        assert int((y2 != y).any(1).sum()) == 1                          # one position of one clip
        best = max(best, _seen(_finish(case, y2, t), ref, tol))
    return best


def _tap_dropped(x, w, b):
    w2 = w.clone().flatten(2)
    w2[:, 60:64, 8] = 0                                                  # four channels of tap (kt, ky, kx) = (0, 2, 2)
    return F.conv3d(x, w2.view_as(w), b, padding=1)


def _lane_half(x, w, b, c0=16, tap=13):
    """Channels c0 + 8 .. c0 + 15 of one chunk read from c0 .. c0 + 7 (lane half 1 without its offset), at tap 13 (the centre)."""
    kt, ky, kx = tap // 9, (tap // 3) % 3, tap % 3
    xs = F.pad(x, (1, 1) * 3)[:, :, kt:kt + x.shape[2], ky:ky + x.shape[3], kx:kx + x.shape[4]]
    wt = w.flatten(2)[:, :, tap]                                         # [co, ci]
    right = torch.einsum("oc,nctyx->notyx", wt[:, c0 + 8:c0 + 16], xs[:, c0 + 8:c0 + 16])
    wrong = torch.einsum("oc,nctyx->notyx", wt[:, c0 + 8:c0 + 16], xs[:, c0:c0 + 8])
    return F.conv3d(x, w, b, padding=1) - right + wrong


def _chunk_dropped(x, w, b, c0=32, tap=4):
    w2 = w.clone().flatten(2)
    w2[:, c0:c0 + 16, tap] = 0
    return F.conv3d(x, w2.view_as(w), b, padding=1)


# The scales follow the rule of test_clip_stages_host.py: conv2 writes its (pooled) map, so a change at one position is seen where
# it happens (60 .. 110 x bound with the seeded weights); behind conv3's tile sum of P positions it competes with the rounding of
# all P and stays at 0.1 .. 1.2 x bound, so the weights the mutation touches are made larger in that test alone
POSITION_CASES = [(_conv2, C_ODD), (_conv2, C_RAGGED), (_conv3, C_ODD), (_conv3, C_RAGGED)]
_ids = lambda v: v.__name__.strip("_") if callable(v) else R.shape_id(v)  # noqa: E731


@pytest.mark.parametrize("case,shape", POSITION_CASES, ids=_ids)
def test_four_input_channels_of_tap_8_dropped_at_one_position(case, shape):
    seen = _mutate_one_position(case, shape, _tap_dropped, scale=None if case is _conv2 else (slice(60, 64), 8, 256.0))
    print(f"{case.__name__} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("case,shape", POSITION_CASES, ids=_ids)
def test_lane_half_offset_lost_in_one_chunk_at_one_position(case, shape):
    seen = _mutate_one_position(case, shape, _lane_half, scale=None if case is _conv2 else (slice(24, 32), 13, 128.0))
    print(f"{case.__name__} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("case,shape", POSITION_CASES, ids=_ids)
def test_one_whole_chunk_of_one_tap_dropped_at_one_position(case, shape):
    seen = _mutate_one_position(case, shape, _chunk_dropped, scale=None if case is _conv2 else (slice(32, 48), 4, 64.0))
    print(f"{case.__name__} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("case,shape", POSITION_CASES, ids=_ids)
def test_zero_padding_replaced_by_edge_clamping_on_the_right(case, shape):
    x, w, b, (y, t), (ref, tol), n = case(shape)
    xp = F.pad(x, (1, 1) * 3)
    xp[..., -1] = xp[..., -2]
    y2 = y.clone()
    y2[..., -1] = F.conv3d(xp, w, b)[..., -1]
    seen = _seen(_finish(case, y2, t), ref, tol)
    print(f"{case.__name__} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_pool_group_takes_seven_of_eight(shape):
    x, w, b, (y, t), (ref, tol), n = _conv2(shape)
    T2, H2, W2 = shape[0] // 2, shape[1] // 4, shape[2] // 4
    worst = []
    for e in range(8):
        y2 = y.clone()
        y2[:, :, 2 * (T2 - 1) + (e >> 2), 2 * (H2 - 1) + ((e >> 1) & 1), 2 * (W2 - 1) + (e & 1)] = -float("inf")
        mut = _finish(_conv2, y2, t)
        assert torch.equal(mut[:, :-1], ref[:, :-1])
        worst.append(_seen(mut, ref, tol))
    print(f"{R.shape_id(shape)}: seen {min(worst):.1f} .. {max(worst):.1f} x bound")
    assert min(worst) > FACTOR


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_last_position_left_out_of_its_tile_sum(shape):
    x, w, b, (y, t), (ref, tol), n = _conv3(shape)
    y2 = y.clone().flatten(2)
    y2[:, :, -1] = 0
    seen = _seen(_finish(_conv3, y2.view_as(y), t), ref, tol)
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", R.C3D_SHAPES, ids=R.shape_id)
def test_head_drops_the_last_k(shape):
    p, _, refs, taps = _c3d(shape)
    w = p["head_w"].clone()
    w[:, -1] = 0
    assert _seen(R.linear(taps["feat"], w, p["head_b"], 256)[0], *refs["logits"]) > FACTOR


@pytest.mark.parametrize("shape", [C_ODD, C_RAGGED], ids=R.shape_id)
def test_conv1_tap_dropped_in_one_column_and_edge_clamping(shape):
    p, frames16, refs, _ = _c3d(shape)
    ref, tol = refs["act1"]
    y, t = R.c3d_conv1(frames16, p)
    x = R.f64(frames16).permute(0, 2, 1, 3, 4)
    w = p["conv1_w"].clone()
    w[:, 2, 2, 2, 2] = 0
    col = y.shape[4] // 2
    y2 = y.clone()
    y2[..., col] = F.conv3d(x, w, p["conv1_b"], padding=1)[..., col]
    seen_tap = _seen(Q.act1_ref(None, None, conv1=(y2, t))[0], ref, tol)
    xp = F.pad(x, (1, 1) * 3)
    xp[..., -1] = xp[..., -2]
    W1 = shape[2] // 2
    y3 = y.clone()
    y3[..., 2 * W1 - 1] = F.conv3d(xp, p["conv1_w"], p["conv1_b"])[..., 2 * W1 - 1]
    seen_edge = _seen(Q.act1_ref(None, None, conv1=(y3, t))[0], ref, tol)
    print(f"{R.shape_id(shape)}: tap {seen_tap:.1f}, edge clamp {seen_edge:.1f} x bound")
    assert seen_tap > FACTOR
    if shape[2] % 2 == 0:                                   # an odd width drops the last column: the pad is never read there
        assert seen_edge > FACTOR


@pytest.mark.parametrize("shape", [C_ODD, C_RAGGED], ids=R.shape_id)
def test_conv1_reads_the_previous_clips_last_frame_in_place_of_the_temporal_zero_pad(shape):
    """Frame t - 1 of clip b + 1 at t = 0 taken from the ring entry before it (clip b's last frame): needs n >= 2."""
    p, frames16, refs, _ = _c3d(shape)
    n, T = shape[4], shape[0]
    assert n >= 2
    ref, tol = refs["act1"]
    x = R.f64(frames16)                                                  # [n, T, 3, H, W]
    flat = x.flatten(0, 1)
    prev = torch.cat([torch.zeros_like(flat[:1]), flat[:-1]])            # entry i - 1 of the frame table
    w = p["conv1_w"]
    # output frame 0 of every clip with its kt = 0 tap reading prev: the other taps are unchanged
    first = torch.arange(n) * T
    extra = F.conv2d(prev[first], w[:, :, 0], padding=1)                 # [n, 64, H, W]
    y, t = R.c3d_conv1(frames16, p)
    y2 = y.clone()
    y2[:, :, 0] += extra
    assert torch.equal(y2[0], y[0])                                      # clip 0 has nothing before it
    seen = _seen(Q.act1_ref(None, None, conv1=(y2, t))[0], ref, tol)
    print(f"{R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR
