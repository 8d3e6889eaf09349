"""CPU-only checks of the fp16 ResNet-18 plan (engine ``resnet-f16``): the packing, the config key, the exports, and -- as
tests/test_clip_f16_host.py does for the CNN-LSTM plan -- proof that the bounds of tests/resnet_f16_refs.py are met by the reference
alone (the float64 chain rounded to the storage types, and torch's fp32 operators on the rounded inputs) and see the bug classes
of k_res16_conv: a stored stage truncated instead of rounded to nearest, the two 8-channel halves of a 16-chunk swapped, a
stride-2 origin off by one, the shortcut taken from the wrong tensor, weights left in fp32.  Truncation errs by at most one fp16
ulp where the bound allows half of one, so it must leave its bound (> 1 x); every other mutation must leave it by a factor of 4.
And the end-to-end constants: TOL_Q / TOL_O are 4 x the measured maxima, and the ``need`` counts hold on the quantised network."""
import ctypes
import dataclasses
import functools
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import resnet_plan as RP
from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.classify import ResNet18
from realtime_video_analytics_32streams_amd.clip_plan import _fold64
from realtime_video_analytics_32streams_amd.config import ConfigError, DetectorConfig, load_config
from tests import resnet_f16_refs as Q
from tests import resnet_stage_refs as R

FACTOR = 4.0
GOLDEN = Path(__file__).resolve().parent / "golden"
NEW = ["rva_resnet_f16_plan_" + n for n in ("create", "destroy", "info", "run", "run_post", "stage")]
S_ONE, S_ODD, S_WIDE, S_MANY = R.SHAPES


# ---------------------------------------------------------------------------------------------------------------------
# packing, config, exports
def test_pack_half_is_rounded_once_and_keeps_names_and_layouts():
    net = synth.seeded_module(lambda: ResNet18(10), 61)
    p16, p32 = RP.pack_resnet18(net, half=True), RP.pack_resnet18(net)
    assert list(p16) == list(p32) == list(N.ResNetWeights.NAMES)
    convs = [(net.stem[0], net.stem[1], "stem_w")]
    i = 0
    for blk in net.layers:
        for conv, bn in [(blk.c1, blk.b1), (blk.c2, blk.b2)] + ([(blk.down[0], blk.down[1])] if blk.down is not None else []):
            convs.append((conv, bn, f"c{i}_w"))
            i += 1
    assert i == 19
    once_differs = 0
    for conv, bn, k in convs:
        want = _fold64(conv, bn)[0].numpy().astype(np.float16)                              # float64 -> fp16: one rounding
        if k != "stem_w":
            want = want.reshape(want.shape[0], want.shape[1], -1).transpose(0, 2, 1)        # [co, k*k, ci]
        assert np.array_equal(p16[k], want.astype(np.float32)), k
        once_differs += int((p32[k].astype(np.float16) != want).sum())                      # float64 -> fp32 -> fp16 is NOT the same thing
        assert p16[k].dtype == np.float32 and p16[k].flags.c_contiguous and p16[k].shape == p32[k].shape
        assert np.array_equal(p16[k].astype(np.float16).astype(np.float32), p16[k])         # fp16-representable
        assert not np.array_equal(p16[k], p32[k])
    print(f"double rounding would move {once_differs} convolution weights")
    for k in p32:
        if not k.endswith("_w") or k == "head_w":
            assert np.array_equal(p16[k], p32[k]), k                                        # biases and the head stay fp32
    again = RP.pack_resnet18(net, half=False)
    assert all(np.array_equal(again[k], p32[k]) for k in p32)


@pytest.mark.parametrize("name", ["stem_w", "c0_w", "c6_w", "c18_w"])
def test_pack_half_refuses_a_weight_beyond_fp16(name):
    net = synth.seeded_module(lambda: ResNet18(10), 61)
    target = {"stem_w": net.stem[0].weight, "c0_w": net.layers[0].c1.weight, "c6_w": net.layers[2].down[0].weight,
              "c18_w": net.layers[7].c2.weight}[name]
    with torch.no_grad():
        target.view(-1)[17] = 1e6
    with pytest.raises(ValueError, match=f"{name} does not stay finite"):
        RP.pack_resnet18(net, half=True)
    RP.pack_resnet18(net)                                                    # fp32 holds it


def test_config_key_is_a_validated_bool_and_defaults_to_false():
    assert DetectorConfig().hip_resnet_fp16 is False
    DetectorConfig(hip_resnet_fp16=True).validate()
    for bad in ("true", 1, None, "fp16"):
        with pytest.raises(ConfigError, match="hip_resnet_fp16"):
            DetectorConfig(hip_resnet_fp16=bad).validate()
    yamls = sorted(GOLDEN.rglob("*.yaml")) + sorted(GOLDEN.rglob("*.yml"))
    assert yamls
    for y in yamls:
        cfg = load_config(y)
        for d in [cfg.detector, *cfg.detectors.values()]:
            assert d.hip_resnet_fp16 is False
    d = dataclasses.replace(DetectorConfig(), backend="hip", model_type="resnet", hip_engine="native", half=True, hip_resnet_fp16=True)
    d.validate()


def test_the_six_entries_are_exported_with_the_fp32_plans_signatures():
    assert RP.ENGINE_F16 == "resnet-f16" and RP.FusedResNet18F16.ABI == "rva_resnet_f16_plan"
    assert RP.FusedResNet18F16.RING_DTYPE == torch.float16 and issubclass(RP.FusedResNet18F16, RP.FusedResNet18)
    assert set(RP.FusedResNet18F16.TAP_DTYPES) == set(Q.F16_STAGES) == set(RP.STAGE_CODES) - {"out7", "feat"}
    assert all(v == torch.float16 for v in RP.FusedResNet18F16.TAP_DTYPES.values())
    assert all(n in N.EXPORTS for n in NEW) and "rva_resnet_f16.hip" in N.SOURCES
    L = ctypes.CDLL(str(N.build()))
    for n in NEW:
        assert hasattr(L, n), n
    for n in ("create", "destroy", "info", "run", "run_post", "stage"):
        new, old = getattr(N.lib(), f"rva_resnet_f16_plan_{n}"), getattr(N.lib(), f"rva_resnet_plan_{n}")
        assert new.argtypes == old.argtypes and new.restype == old.restype, n


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone meets every condition the GPU tests impose
@functools.lru_cache(maxsize=None)
def _chain(shape):
    net, p, frames16 = Q.case16(shape)
    refs = Q.refs16(None, frames16, p, shape)
    return net, p, frames16, refs, {k: Q.stored(k, v[0]) for k, v in refs.items()}


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_float64_chain_rounded_to_the_storage_types_is_inside_every_bound(shape):
    net, p, frames16, refs, taps = _chain(shape)
    assert all(taps[k].dtype == (torch.float16 if k in Q.F16_STAGES else torch.float32) for k in Q.STAGES)
    again = Q.refs16(taps, frames16, p, shape)
    bad = []
    for k in Q.STAGES + ("logits",):
        R.report(shape, k, taps[k], *again[k], out=bad)
    assert not bad, bad
    peak = max(float(taps[k].abs().max()) for k in Q.F16_STAGES)
    print(f"{R.shape_id(shape)}: largest stored fp16 activation {peak:.2f}")
    assert peak < 100.0                                                      # far from fp16's range


def _conv32(name, x, q):
    i = R.CONV_OF[name]
    cin, c, s = R.BLOCKS[int(name[-1])]
    kw = dict(stride=s, padding=1) if name.startswith("mid") else dict(stride=2) if name.startswith("down") else dict(padding=1)
    return F.conv2d(x, q[f"c{i}_w"], q[f"c{i}_b"], **kw)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_torch_fp32_arithmetic_on_the_rounded_inputs_is_inside_every_bound(shape):
    """No fp16 arithmetic anywhere: torch's fp32 operators on the fp16 values widened to fp32, the result rounded once."""
    net, p, frames16, refs, taps = _chain(shape)
    q = {k: v.float() for k, v in p.items()}
    x32 = lambda k: taps[k].float().permute(0, 3, 1, 2)  # noqa: E731
    got = {}
    y = F.conv2d(frames16.float(), q["stem_w"], q["stem_b"], stride=2, padding=3)
    got["pooled"] = R.nhwc(F.max_pool2d(y.relu(), 3, 2, 1)).half()
    prev = "pooled"
    for b in range(8):
        x = x32(prev)
        got[f"mid{b}"] = R.nhwc(_conv32(f"mid{b}", x, q).relu()).half()
        r = x
        if b in R.DOWN:
            got[f"down{b}"] = R.nhwc(_conv32(f"down{b}", x, q)).half()
            r = x32(f"down{b}")
        o = R.nhwc((_conv32(f"out{b}", x32(f"mid{b}"), q) + r).relu())
        got[f"out{b}"] = o if b == 7 else o.half()
        prev = f"out{b}"
    v = taps["out7"].flatten(1, 2)
    got["feat"] = v.sum(1) / torch.tensor(float(v.shape[1]), dtype=torch.float32)
    got["logits"] = taps["feat"] @ q["head_w"].T + q["head_b"]
    bad = []
    for k, v in got.items():
        assert v.dtype == (torch.float16 if k in Q.F16_STAGES else torch.float32), k
        R.report(shape, k, v, *refs[k], out=bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the bounds see k_res16_conv's bug classes
def _seen(mutated, ref, tol):
    return R.ratio(mutated, ref, tol)[0]


def _truncate_f16(v64):
    """float64 -> fp32 -> fp16 by dropping the low 13 mantissa bits (round toward zero; normal fp16 range)."""
    bits = v64.float().contiguous().view(torch.int32) & ~0x1FFF
    h = bits.view(torch.float32).half()
    assert torch.equal(h.float().view(torch.int32), bits) or bool((v64.abs() < 2.0 ** -14).any())
    return h


MUT_SHAPES = [S_ODD, S_WIDE, S_MANY]


@pytest.mark.parametrize("shape", MUT_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("stage", ["pooled", "mid0", "out1", "down2", "out3"])
def test_truncation_instead_of_round_to_nearest_leaves_the_bound(stage, shape):
    """On the stages up to 128 channels.  Deeper, the fp32 term of the bound -- (9 x 512 + 3) u32 times the sum of |products| -- is
    itself as large as half an fp16 ulp of the result, so there the bound cannot tell the two roundings apart (out6: 0.8 x)."""
    net, p, frames16, refs, taps = _chain(shape)
    ref, tol = refs[stage]
    seen = _seen(_truncate_f16(ref), ref, tol)
    print(f"{stage} {R.shape_id(shape)}: seen {seen:.2f} x bound")
    assert seen > 1.0
    assert _seen(Q.stored(stage, ref), ref, tol) <= 1.0


def _stage_inputs(stage, taps):
    b = int(stage[-1])
    src = f"mid{b}" if stage.startswith("out") else ("pooled" if b == 0 else f"out{b - 1}")
    return R.nchw(taps[src])


def _mutated(stage, x, p, taps, relu):
    """The stage's stored value from the (mutated) input / weights: float64 conv, the epilogue, one rounding."""
    b = int(stage[-1])
    y = R.block_conv(stage, x, p)[0]
    if stage.startswith("out"):
        r = R.nchw(taps[f"down{b}"] if b in R.DOWN else taps["pooled" if b == 0 else f"out{b - 1}"])
        y = y + r
    return Q.stored(stage, R.nhwc(y.relu() if relu else y))


@pytest.mark.parametrize("shape", MUT_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("stage,c0", [("mid0", 16), ("down2", 48), ("mid4", 112), ("out5", 240), ("mid7", 496)])
def test_the_two_halves_of_one_chunk_swapped(stage, c0, shape):
    """Lane half 0 supplies channels c0 + 8 .. c0 + 15 and lane half 1 channels c0 .. c0 + 7 of one 16-chunk, at every tap."""
    net, p, frames16, refs, taps = _chain(shape)
    x = _stage_inputs(stage, taps).clone()
    lo, hi = x[:, c0:c0 + 8].clone(), x[:, c0 + 8:c0 + 16].clone()
    x[:, c0:c0 + 8], x[:, c0 + 8:c0 + 16] = hi, lo
    seen = _seen(_mutated(stage, x, p, taps, not stage.startswith("down")), *refs[stage])
    print(f"{stage} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", MUT_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("stage", ["mid2", "down2", "mid4", "down4", "mid6", "down6"])
def test_stride_2_origin_off_by_one(stage, shape):
    """Output pixel (y, x) reads the window of input pixel (2y + 1, 2x + 1): the input shifted by one up and left."""
    net, p, frames16, refs, taps = _chain(shape)
    x = _stage_inputs(stage, taps)
    shifted = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
    assert shifted.shape == x.shape
    seen = _seen(_mutated(stage, shifted, p, taps, stage.startswith("mid")), *refs[stage])
    print(f"{stage} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", MUT_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("b", [1, 2, 5, 7])
def test_shortcut_taken_from_the_wrong_tensor(b, shape):
    """``out<b>`` adds its own ``mid<b>`` (same shape) instead of the block's input or its ``down``."""
    net, p, frames16, refs, taps = _chain(shape)
    a = R.nchw(taps[f"mid{b}"])
    got = Q.stored(f"out{b}", R.nhwc((R.block_conv(f"out{b}", a, p)[0] + a).relu()))
    seen = _seen(got, *refs[f"out{b}"])
    print(f"out{b} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


@pytest.mark.parametrize("shape", MUT_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("stage", ["down2", "down4"])
def test_unrounded_fp32_weights(stage, shape):
    """The float64-folded weights rounded to fp32, not fp16: each differs from the plan's by up to 2**-12 of itself.  The shortcut
    convolutions see it (short sums, no ReLU, outputs that pass near zero, where the storage term of the bound vanishes); behind
    the longer sums the difference sinks into the fp32 term of the bound (down6 3.6 .. 4.4 x, mid0 1.2 x, out4 0.5 x, mid7 0.3 x): there it is the
    end-to-end distance to the quantised network that holds the weights."""
    net, p, frames16, refs, taps = _chain(shape)
    p32 = Q.pack64(net, half=False)
    seen = _seen(_mutated(stage, _stage_inputs(stage, taps), p32, taps, not stage.startswith("down")), *refs[stage])
    print(f"{stage} {R.shape_id(shape)}: seen {seen:.1f} x bound")
    assert seen > FACTOR


# ---------------------------------------------------------------------------------------------------------------------
# end to end
def _up2(v):
    """``v`` rounded up to two significant digits."""
    e = 10.0 ** (math.floor(math.log10(v)) - 1)
    return math.ceil(v / e - 1e-9) * e


def test_tolerances_are_four_times_the_measured_maxima_and_the_need_counts_hold():
    dq, do = [], []
    print("case                          |emu - quantised|  |emu - original|  clear frames (need)  smallest top-6 gaps")
    for case, need in zip(Q.E2E_CASES, Q.NEED):
        net, x, quant, emu, orig = Q.e2e(case)
        dq.append(float(np.abs(emu - quant).max()))
        do.append(float(np.abs(emu - orig).max()))
        gaps = Q.top_gaps(quant)
        clear = [g > 2 * Q.TOL_Q for g in gaps]
        print(f"{str(case):30s}{dq[-1]:.3e}          {do[-1]:.3e}         {sum(clear)} of {len(gaps)} ({need})          "
              f"{' '.join(f'{g:.1e}' for g in gaps)}")
        assert sum(clear) >= need
        for e, q, ok in zip(emu, quant, clear):
            if ok:
                assert Q.top(e).tolist() == Q.top(q).tolist()
    print(f"TOL_Q = 4 x {max(dq):.4e} -> {_up2(4 * max(dq)):.2e} (is {Q.TOL_Q:.2e}); TOL_O = 4 x {max(do):.4e} -> {_up2(4 * max(do)):.2e} "
          f"(is {Q.TOL_O:.2e})")
    # rounding up to two digits adds less than 10 %; the comparison is not on the rounded value itself, which a change in the last
    # digits of a maximum next to a step (4 x 7.0015e-5 = 2.8006e-4 -> 2.9e-4) would move
    assert 4 * max(dq) <= Q.TOL_Q <= 1.1 * 4 * max(dq)
    assert 4 * max(do) <= Q.TOL_O <= 1.1 * 4 * max(do)
    assert Q.NEED == (8, 3, 3, 4)
