"""Float64 references and derived bounds for the fp16 ResNet-18 plan (csrc/rva_resnet_f16.hip, engine ``resnet-f16``), shared by
tests/test_resnet_f16_host.py (CPU) and the GPU tests.  Built on tests/resnet_stage_refs.py as tests/clip_f16_refs.py is on
tests/clip_stage_refs.py: the same per-stage references, each computed from the tap of the stage before it, on the fp16 frames and
the fp16-rounded weights the plan itself holds, with the fp16 storage bound of tests/clip3d_f16_refs.py (``f16_tol``):

  * a stage stored as fp16 (``pooled``, ``mid<b>``, ``down<b>``, ``out0`` .. ``out6``): its fp32 epilogue value obeys the fp32
    plan's bound ``tol32`` of resnet_stage_refs -- a product of two fp16 values is exact in fp32, so only the additions round, and
    the bound holds for any order of them -- and the one rounding to fp16 adds ``f16_tol(ref, tol32)``;
  * ``out<b>``: ``tol32`` includes the residual term ``(9 C + 3) u32 |r|`` with ``r`` the fp16 shortcut tap (widened exactly);
  * ``out7`` (stored fp32), ``feat`` and ``logits`` are fp32 from fp32: exactly the fp32 plan's bounds.

End to end: :func:`network64` is the float64 "quantised network" (fp16 frames, fp16-rounded weights, exact activations) and, with
``round_acts=True``, the float64 "emulation" that additionally rounds every fp16-stored stage as the plan stores it.

TOL_Q / TOL_O are 4 x the largest distance, over the four end-to-end cases, of the float64 emulation to the quantised network /
to the original float64 module, rounded up to two digits.  Measured on the CPU (tests/test_resnet_f16_host.py prints them):

    case (B, H, W, classes, seeds)    |emu - quantised|   |emu - original|   frames whose top-6 gap > 2 TOL_Q (need)
    (8, 224, 224, 1000, 81, 82)       2.30e-5              7.00e-5             8 of 8 (8)
    (3, 34, 34, 10, 85, 86)           3.76e-5              3.98e-5             3 of 3 (3)
    (5, 40, 72, 37, 87, 88)           4.19e-5              5.79e-5             4 of 5 (3)
    (4, 33, 47, 10, 91, 92)           3.30e-5              3.82e-5             4 of 4 (4)

so TOL_Q = 4 x 4.189e-5 = 1.7e-4 and TOL_O = 4 x 7.002e-5 = 2.9e-4.  The smallest top-6 gaps per frame of the quantised network are
7.6e-4 .. 4.9e-3, >= 1.7e-2, (4.6e-4, 5.9e-3, 9.4e-3, 2.1e-3, 4.3e-5) and >= 9.9e-4: the third case has one inherently tied frame and one
near the threshold, which is why its ``need`` leaves two out.  Across all cases and the stage shapes the stored activations stay
far inside fp16's range.  The factor 4 is the margin of the two other fp16 plans: the device's fp32 rounding and the occasional flip of an fp16 rounding
come on top of the emulation's distance.  tools/resnet_f16_report.py records what an MI355X leaves of it.
"""
import copy
import functools

import numpy as np
import torch

from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.classify import ResNet18
from realtime_video_analytics_32streams_amd.resnet_plan import pack_resnet18
from tests import resnet_stage_refs as R
from tests.clip3d_f16_refs import f16_tol, top  # noqa: F401  (top: re-exported for the tests)

TOL_Q = 1.7e-4                              # |plan - quantised float64 network|
TOL_O = 2.9e-4                              # |plan - original float64 module|
STAGES = R.STAGES
F16_STAGES = tuple(n for n in STAGES if n not in ("out7", "feat"))

# (B, H, W, classes, net seed, input seed) and the frames per case whose quantised top-6 gap must exceed 2 TOL_Q
E2E_CASES = ((8, 224, 224, 1000, 81, 82), (3, 34, 34, 10, 85, 86), (5, 40, 72, 37, 87, 88), (4, 33, 47, 10, 91, 92))
NEED = (8, 3, 3, 4)


def pack64(net, half=True):
    """``pack_resnet18(net, half)`` as float64 tensors, the block convolutions back in the module's ``[co, ci, k, k]``."""
    p = {k: R.f64(v) for k, v in pack_resnet18(net, half=half).items()}
    for i in range(19):
        w = p[f"c{i}_w"]
        k = int(round(w.shape[1] ** 0.5))
        p[f"c{i}_w"] = w.permute(0, 2, 1).reshape(w.shape[0], w.shape[2], k, k).contiguous()
    return p


@functools.lru_cache(maxsize=None)
def case16(shape):
    """The seeded case of ``resnet_stage_refs.case`` for the fp16 plan: the module, its fp16-rounded packed weights (float64) and
    the frames ``[B, 3, H, W]`` rounded to fp16 (what the plan reads).  Computed once; callers leave it unchanged."""
    net, _, frames = R.case(shape)
    return net, pack64(net), frames.half()


def stored(name, t):
    """``t`` rounded once to the type the plan stores stage ``name`` in."""
    return R.f64(t).half() if name in F16_STAGES else R.f64(t).float()


def _f16(name, ref, tol32):
    return (ref, f16_tol(ref, tol32)) if name in F16_STAGES else (ref, tol32)


def refs16(taps, frames16, p, shape=None):
    """name -> (float64 reference, bound) for every stage and the logits; each stage from the tap(s) it read, as
    ``resnet_stage_refs.refs``.  ``taps = None`` chains the references themselves, each rounded once to its storage type."""
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: stored(k, out[k][0]))
    out["pooled"] = _f16("pooled", *R.stem_pool(*R.stem_conv(R.f64(frames16), {"conv1_w": p["stem_w"], "conv1_b": p["stem_b"]})))
    prev = "pooled"
    for b in range(8):
        x = R.nchw(tap(prev))
        y, t = R.block_conv(f"mid{b}", x, p)
        out[f"mid{b}"] = _f16(f"mid{b}", R.nhwc(y.relu()), R.nhwc(t))
        r = x
        if b in R.DOWN:
            y, t = R.block_conv(f"down{b}", x, p)
            out[f"down{b}"] = _f16(f"down{b}", R.nhwc(y), R.nhwc(t))
            r = R.nchw(tap(f"down{b}"))
        out[f"out{b}"] = _f16(f"out{b}", *R.out_stage(b, R.nchw(tap(f"mid{b}")), r, p))
        prev = f"out{b}"
    out["feat"] = R.feat_stage(tap("out7"))
    out["logits"] = R.linear(tap("feat"), p["head_w"], p["head_b"], 512)
    return out


def network64(p, frames, round_acts=False):
    """Logits ``[B, classes]`` in float64 of packed weights ``p`` on frames ``[B, 3, H, W]`` (used as they are): exact activations,
    or with ``round_acts`` every fp16-stored stage rounded to fp16 as the plan stores it (``out7`` stays exact: it is fp32)."""
    F = torch.nn.functional
    rnd = (lambda t: t.half().double()) if round_acts else (lambda t: t)
    x = F.conv2d(R.f64(frames), p["stem_w"], p["stem_b"], stride=2, padding=3).relu()
    x = rnd(F.max_pool2d(x, 3, 2, 1))
    for b, (cin, c, s) in enumerate(R.BLOCKS):
        i = R.CONV_OF[f"mid{b}"]
        a = rnd(F.conv2d(x, p[f"c{i}_w"], p[f"c{i}_b"], stride=s, padding=1).relu())
        r = x
        if b in R.DOWN:
            j = R.CONV_OF[f"down{b}"]
            r = rnd(F.conv2d(x, p[f"c{j}_w"], p[f"c{j}_b"], stride=2))
        y = (F.conv2d(a, p[f"c{i + 1}_w"], p[f"c{i + 1}_b"], padding=1) + r).relu()
        x = y if b == 7 else rnd(y)
    return (x.mean((2, 3)) @ p["head_w"].T + p["head_b"]).numpy()


def module64(net, frames):
    """The original module in float64 on frames ``[B, 3, H, W]``."""
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(R.f64(frames)).numpy()


@functools.lru_cache(maxsize=None)
def e2e(case):
    """(net, fp32 frames, quantised, emulation, original): one end-to-end case and its float64 logits, computed once and shared
    (callers leave them unchanged)."""
    B, H, W, classes, seed_net, seed_x = case
    net = synth.seeded_module(lambda: ResNet18(classes), seed_net)
    x = synth.seeded_clip((B, 3, H, W), seed_x)
    p, x16 = pack64(net), x.half()
    return net, x, network64(p, x16), network64(p, x16, round_acts=True), module64(net, x)


def top_gaps(logits):
    """Per row the smallest gap between consecutive values among the top k + 1, k = min(5, classes - 1)."""
    gaps = []
    for r in logits:
        s = np.sort(r)[::-1]
        k = min(5, len(r) - 1)
        gaps.append(float(np.min(s[:k] - s[1:k + 1])))
    return gaps
