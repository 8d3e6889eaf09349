"""Float64 references and derived bounds for the fp16 3D-CNN clip plan (csrc/rva_clip3d.hip, engine ``clip3d-f16``), shared by
tests/test_clip3d_f16_host.py (CPU) and the GPU tests.  Built on tests/clip_stage_refs.py: the same per-stage references, each
computed from the tap of the stage before it, on the fp16 frames and the fp16-rounded convolution weights the plan itself holds.

With u32 = 2**-24 and u16 = 2**-11:

  * a stage stored as fp16 (act1, act2): its fp32 value obeys the fp32 plan's bound ``tol32 = (n + 2) u32 (conv(|x|, |w|) + |b|)``
    pooled with max -- the bound carries over because a product of two fp16 values is exact in fp32, so only the additions
    round -- and the one rounding to fp16 of a value within tol32 of the reference adds at most ``u16 (|ref| + tol32)`` in the
    normal range and ``2**-25`` (half the spacing of fp16 subnormals) below it: ``tol = tol32 + u16 (|ref| + tol32) + 2**-25``;
  * partial, feat, logits are fp32 from fp32: exactly the fp32 plan's bounds.

End to end: :func:`network64` is the float64 "quantised network" (fp16 clips, fp16-rounded weights, exact activations) and, with
``round_acts=True``, the float64 "emulation" that additionally rounds act1 / act2 to fp16 as the plan stores them."""
import copy
import functools

import numpy as np
import torch

from realtime_video_analytics_32streams_amd.clip_plan import pack_cnn3d
from tests import clip_stage_refs as R

U16 = 2.0 ** -11
SUB16 = 2.0 ** -25
TOL_Q = 2.5e-5                            # |plan - quantised float64 network|
TOL_O = 2e-4                              # |plan - original float64 module| and |plan - recorded golden logits|
F16_STAGES = ("act1", "act2")
STAGES = ("act1", "act2", "partial", "feat")

ODD = dict(classes=10, seeds=(61, 62), clips=(2, 3, 7, 25, 41))            # [B, 3, T, H, W]
RAGGED = dict(classes=10, seeds=(81, 82), clips=(6, 3, 4, 36, 68))


def pack64(net, half=True):
    """``pack_cnn3d(net, half)`` as float64 tensors, conv2 / conv3 back in the module's ``[co, ci, 3, 3, 3]``."""
    p = {k: R.f64(v) for k, v in pack_cnn3d(net, half=half).items()}
    for k in ("conv2_w", "conv3_w"):
        w = p[k]
        p[k] = w.permute(0, 2, 1).reshape(w.shape[0], w.shape[2], 3, 3, 3).contiguous()
    return p


def c3d16_case(shape):
    """The seeded case of ``clip_stage_refs.c3d_case`` for the fp16 plan: the module, its fp16-rounded packed weights (float64)
    and the frames ``[n, T, 3, H, W]`` rounded to fp16 (the ring the plan reads)."""
    net, _, frames = R.c3d_case(shape)
    return net, pack64(net), frames.half()


def f16_tol(ref, tol32):
    return tol32 + U16 * (ref.abs() + tol32) + SUB16


def stored(name, t):
    """``t`` rounded once to the type the plan stores stage ``name`` in."""
    return R.f64(t).half() if name in F16_STAGES else R.f64(t).float()


def act1_ref(frames16, p, conv1=None):
    y, t = conv1 if conv1 is not None else R.c3d_conv1(frames16, p)
    a, t = R.c3d_pool(y, t, (1, 2, 2))
    return a, f16_tol(a, t)


def act2_ref(act1, p, conv2=None):
    y, t = conv2 if conv2 is not None else R.c3d_conv2(act1, p)
    a, t = R.c3d_pool(y, t, (2, 2, 2))
    a, t = a.flatten(1, 3), t.flatten(1, 3)
    return a, f16_tol(a, t)


def c3d16_refs(taps, frames16, p, shape):
    """name -> (float64 reference, bound) for act1, act2, partial, feat, logits; each stage from the tap before it.  ``taps =
    None`` chains the references themselves, each rounded once to its storage type (what an exact kernel would leave)."""
    T, H, W = shape[:3]
    thw = (T // 2, H // 4, W // 4)
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: stored(k, out[k][0]))
    out["act1"] = act1_ref(frames16, p)
    out["act2"] = act2_ref(tap("act1"), p)
    out["partial"] = R.partial_from_map(*R.c3d_conv3(tap("act2"), p, thw))
    out["feat"] = R.feat_from_partial(tap("partial"), thw[0] * thw[1] * thw[2])
    out["logits"] = R.linear(tap("feat"), p["head_w"], p["head_b"], 256)
    return out


def network64(p, clips, round_acts=False):
    """Logits ``[B, classes]`` in float64 of packed weights ``p`` on clips ``[B, 3, T, H, W]`` (used as they are): exact
    activations, or with ``round_acts`` act1 / act2 rounded to fp16 as the plan stores them."""
    x = R.f64(clips).permute(0, 2, 1, 3, 4)                       # frames [B, T, 3, H, W]
    B, T, _, H, W = x.shape
    thw = (T // 2, H // 4, W // 4)
    rnd = (lambda t: t.half().double()) if round_acts else (lambda t: t)
    a1 = rnd(R.c3d_pool(*R.c3d_conv1(x, p), (1, 2, 2))[0])
    a2 = rnd(R.c3d_pool(*R.c3d_conv2(a1, p), (2, 2, 2))[0]).flatten(1, 3)
    y = R.c3d_conv3(a2, p, thw)[0].relu()
    return (y.flatten(2).mean(2) @ p["head_w"].T + p["head_b"]).numpy()


def module64(net, clips):
    """The original module in float64 on clips ``[B, 3, T, H, W]``."""
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(R.f64(clips)).numpy()


def seeded(case):
    """(net, fp32 clips ``[B, 3, T, H, W]``) of ODD / RAGGED."""
    from realtime_video_analytics_32streams_amd import synth
    from realtime_video_analytics_32streams_amd.temporal import Cnn3dNet
    return synth.seeded_module(lambda: Cnn3dNet(case["classes"]), case["seeds"][0]), synth.seeded_clip(case["clips"], case["seeds"][1])


def top(v, k=5):
    k = min(k, len(v))
    return np.argsort(v, kind="stable")[-k:][::-1]


E2E_NAMES = ("golden-c400", "golden-c10", "odd", "ragged")          # the end-to-end cases of tests/test_gpu_clip3d_f16_plan.py


@functools.lru_cache(maxsize=None)
def e2e(name):
    """(net, fp32 clips, quantised, emulation, original, recorded or None): one end-to-end case and its float64 logits, computed
    once and shared (callers leave them unchanged)."""
    from tests.conftest import load_golden
    from tests.helpers import temporal_net
    if name.startswith("golden"):
        case = {f"golden-c{c['ctor']['num_classes']}": c for c in load_golden("temporal_nets.json") if c["kind"] == "3d_cnn"}[name]
        net, x = temporal_net(case)
        recorded = np.asarray(case["logits"], np.float64)
    else:
        (net, x), recorded = seeded({"odd": ODD, "ragged": RAGGED}[name]), None
    p, x16 = pack64(net), x.half()
    return net, x, network64(p, x16), network64(p, x16, round_acts=True), module64(net, x), recorded
