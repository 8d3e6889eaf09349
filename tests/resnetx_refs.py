"""Float64 references and derived bounds for the fp16 plan of any ResNet (``rva_resnetx_f16_plan_*`` in csrc/rva_resnet_f16.hip,
resnet_plan.FusedResNetF16, engine ``resnet-f16`` on a :class:`classify.ResNet`), shared by tests/test_resnetx_host.py (CPU) and
the GPU tests.  Built as tests/resnet_f16_refs.py is for the ResNet-18 plan.

Per stage (:func:`refsx`): every stage is computed in float64 from the tap(s) the launch itself read, on the fp16 frames and the
fp16-rounded weights the plan holds, so a bound covers ONE launch.  With u = 2**-24 an fp32 sum of K products plus a bias errs by at
most ``(K + 2) u (conv(|x|, |w|) + |b|)`` in any order (a product of two fp16 values is exact in fp32):

  * ``b<k>.mid1`` / ``b<k>.mid2`` / ``b<k>.down``: K = taps x Cin;
  * ``b<k>.out`` with a residual (identity blocks, and split plans): ``(taps x C + 3) u (conv(|a|, |w|) + |b| + |r|)``;
  * ``b<k>.out`` with the shortcut convolution inside the launch (fused plans): K = taps x C + Cin2 and the absolute-value term of
    both operands, ``(K + 2) u (conv(|a|, |w_close|) + conv(|x|, |w_short|) + |b_close + b_short|)``;
  * a stage stored as fp16 adds the storage term ``f16_tol`` of tests/clip3d_f16_refs.py; the last block's ``out``, ``feat`` and
    the logits are fp32: ``feat`` ``(P + 1) u sum |v| / P``, logits ``(512 e + 2) u (|f| . |W|^T + |b|)``.

End to end (:func:`network64`): the float64 "quantised network" (fp16 frames, fp16-rounded weights, exact activations) and, with
``round_acts``, the float64 "emulation" that rounds every fp16-stored stage as the plan stores it -- for a fused plan the shortcut
convolution is never stored, for a split plan it is rounded like any stage.

TOL_Q / TOL_O per case are 4 x the distance of the fused emulation to the quantised network / to the original float64 module,
rounded up to two digits; the factor 4 is the one the three other fp16 plans use over their emulation (the device's fp32 rounding
and flipped fp16 roundings come on top).  Measured on the CPU (tests/test_resnetx_host.py prints this table):

    case (block, blocks, B, H x W, classes)      |emu - quantised|  |emu - original|  split: |emu - quantised|  clear frames  smallest top-6 gaps
    bottleneck (3,4,6,3)   3 x 64 x 64   c100    7.546e-5           9.141e-5          8.902e-5                  2 of 3        1.2e-3 5.5e-4 1.7e-3
    basic      (3,4,6,3)   3 x 40 x 72   c37     9.303e-5           8.272e-5          5.796e-5                  2 of 3        2.9e-4 2.8e-3 1.8e-3
    bottleneck (3,8,36,3)  2 x 33 x 47   c10     1.963e-4           1.926e-4          2.075e-4                  2 of 2        5.5e-3 8.1e-3
    bottleneck (3,4,23,3)  2 x 64 x 64   c50     1.581e-4           1.792e-4          1.669e-4                  2 of 2        1.2e-2 8.5e-3
    bottleneck (1,2,1,1)   5 x 40 x 72   c37     1.640e-5           3.036e-5          2.459e-5                  5 of 5        1.4e-3 9.4e-4 1.2e-3 3.5e-4 1.7e-3
    basic      (2,2,2,2)   4 x 33 x 47   c10     3.431e-5           5.139e-5          4.655e-5                  4 of 4        1.8e-3 1.6e-2 1.3e-3 1.4e-2

The largest stored activation over all cases is 4.1.  On five cases the fused form is closer to the quantised network than the
split one (one fp16 rounding fewer per stage); on the BasicBlock (3,4,6,3) case it is the other way round, by chance of the
roundings.  The tolerances come from the fused form, the plan's default.

The top-5 is compared on the frames whose quantised top-6 gap exceeds 2 TOL_Q; at most one frame per case may be left out.
"""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.classify import ResNet
from realtime_video_analytics_32streams_amd.resnet_plan import pack_resnet, resnet_blocks
from tests import resnet_stage_refs as R
from tests.clip3d_f16_refs import f16_tol, top  # noqa: F401  (top: re-exported for the tests)
from tests.resnet_f16_refs import top_gaps  # noqa: F401

U = R.U

# (block, blocks, B, H, W, classes, net seed, input seed)
E2E_CASES = (
    ("bottleneck", (3, 4, 6, 3), 3, 64, 64, 100, 501, 502),
    ("basic", (3, 4, 6, 3), 3, 40, 72, 37, 503, 504),
    ("bottleneck", (3, 8, 36, 3), 2, 33, 47, 10, 505, 506),
    ("bottleneck", (3, 4, 23, 3), 2, 64, 64, 50, 507, 508),
    ("bottleneck", (1, 2, 1, 1), 5, 40, 72, 37, 509, 510),
    ("basic", (2, 2, 2, 2), 4, 33, 47, 10, 511, 512),
)
RESNET50, BASIC34, RESNET152, RESNET101, SMALL_BOTT, SMALL_BASIC = E2E_CASES
# per case: |plan - quantised float64 network|, |plan - original float64 module|
TOL_Q = {RESNET50: 3.1e-4, BASIC34: 3.8e-4, RESNET152: 7.9e-4, RESNET101: 6.4e-4, SMALL_BOTT: 6.6e-5, SMALL_BASIC: 1.4e-4}
TOL_O = {RESNET50: 3.7e-4, BASIC34: 3.4e-4, RESNET152: 7.8e-4, RESNET101: 7.2e-4, SMALL_BOTT: 1.3e-4, SMALL_BASIC: 2.1e-4}
LEAVE_OUT = 1                                # frames per case whose top-6 gap may be within 2 TOL_Q


def case_id(c):
    return f"{c[0]}-{'.'.join(str(n) for n in c[1])}-{c[2]}x{c[3]}x{c[4]}-c{c[5]}"


def n_convs(p):
    return (len(p) - 4) // 2


def pack64(net, fused=True, half=True):
    """``pack_resnet(net, half, fused)`` as float64 tensors, the block convolutions back in the module's ``[co, ci, k, k]``."""
    p = {k: R.f64(v) for k, v in pack_resnet(net, half=half, fused=fused).items()}
    for i in range(n_convs(p)):
        w = p[f"c{i}_w"]
        k = int(round(w.shape[1] ** 0.5))
        p[f"c{i}_w"] = w.permute(0, 2, 1).reshape(w.shape[0], w.shape[2], k, k).contiguous()
    return p


def layout(bottleneck, blocks):
    """Per block: the table of ``resnet_plan.resnet_blocks`` plus the indices of its convolutions in the ABI's order: ``convs``
    (conv1, conv2[, conv3]) and ``short`` (or None)."""
    out, i = [], 0
    for t in resnet_blocks(bottleneck, blocks):
        n = 3 if bottleneck else 2
        t = dict(t, convs=tuple(range(i, i + n)), short=(i + n) if t["shortcut"] else None)
        i += n + t["shortcut"]
        out.append(t)
    return out


def stage_names(bottleneck, blocks, fused):
    names = ["pooled"]
    for b, t in enumerate(layout(bottleneck, blocks)):
        names.append(f"b{b}.mid1")
        if bottleneck:
            names.append(f"b{b}.mid2")
        if t["shortcut"] and not fused:
            names.append(f"b{b}.down")
        names.append(f"b{b}.out")
    return tuple(names + ["feat"])


def f16_stages(bottleneck, blocks, fused):
    names = stage_names(bottleneck, blocks, fused)
    return tuple(n for n in names if n not in (f"b{sum(blocks) - 1}.out", "feat"))


def _conv(x, p, i, K, **kw):
    return R.conv_bound(F.conv2d, x, p[f"c{i}_w"], p[f"c{i}_b"], K, **kw)


def refsx(taps, frames16, p, bottleneck, blocks, fused):
    """name -> (float64 reference, bound) for every stage of the plan and the logits, each from the tap(s) its launch read.
    ``taps = None`` chains the references themselves, each rounded once to its storage type."""
    lay = layout(bottleneck, blocks)
    f16 = set(f16_stages(bottleneck, blocks, fused))
    out = {}

    def put(name, ref, tol32):
        out[name] = (ref, f16_tol(ref, tol32)) if name in f16 else (ref, tol32)

    def tap(k):
        if taps is not None:
            return taps[k]
        return R.f64(out[k][0]).half() if k in f16 else R.f64(out[k][0]).float()

    put("pooled", *R.stem_pool(*R.stem_conv(R.f64(frames16), {"conv1_w": p["stem_w"], "conv1_b": p["stem_b"]})))
    prev = "pooled"
    for b, t in enumerate(lay):
        x = R.nchw(tap(prev))
        cin, width, s = t["cin"], t["width"], t["stride"]
        if bottleneck:
            y, tol = _conv(x, p, t["convs"][0], cin)
            put(f"b{b}.mid1", R.nhwc(y.relu()), R.nhwc(tol))
            y, tol = _conv(R.nchw(tap(f"b{b}.mid1")), p, t["convs"][1], 9 * width, stride=s, padding=1)
            put(f"b{b}.mid2", R.nhwc(y.relu()), R.nhwc(tol))
            a, close, taps_c, pad = R.nchw(tap(f"b{b}.mid2")), t["convs"][2], 1, 0
        else:
            y, tol = _conv(x, p, t["convs"][0], 9 * cin, stride=s, padding=1)
            put(f"b{b}.mid1", R.nhwc(y.relu()), R.nhwc(tol))
            a, close, taps_c, pad = R.nchw(tap(f"b{b}.mid1")), t["convs"][1], 9, 1
        K = taps_c * width
        if t["shortcut"] and fused:
            ws = p[f"c{t['short']}_w"]
            y = F.conv2d(a, p[f"c{close}_w"], p[f"c{close}_b"], padding=pad) + F.conv2d(x, ws, None, stride=s)
            mag = F.conv2d(a.abs(), p[f"c{close}_w"].abs(), p[f"c{close}_b"].abs(), padding=pad) + F.conv2d(x.abs(), ws.abs(), None, stride=s)
            put(f"b{b}.out", R.nhwc(y.relu()), R.nhwc((K + cin + 2) * U * mag))
        else:
            r = x
            if t["shortcut"]:
                y, tol = _conv(x, p, t["short"], cin, stride=s)
                put(f"b{b}.down", R.nhwc(y), R.nhwc(tol))
                r = R.nchw(tap(f"b{b}.down"))
            y, tol = _conv(a, p, close, K + 1, padding=pad)               # (K + 3) u (conv(|a|, |w|) + |b|)
            put(f"b{b}.out", R.nhwc((y + r).relu()), R.nhwc(tol + (K + 3) * U * r.abs()))
        prev = f"b{b}.out"
    out["feat"] = R.feat_stage(tap(prev))
    out["logits"] = R.linear(tap("feat"), p["head_w"], p["head_b"], p["head_w"].shape[1])
    return out


def network64(p, frames, round_acts, fused, bottleneck, blocks, peak=None):
    """Logits ``[B, classes]`` in float64 of packed weights ``p`` (of ``pack64(net, fused)``) on frames ``[B, 3, H, W]`` (used as
    they are): exact activations, or with ``round_acts`` every fp16-stored stage rounded to fp16 as the plan stores it (the last
    block's output stays exact: it is fp32).  ``peak``: a list that receives the largest magnitude of every stored stage."""
    lay = layout(bottleneck, blocks)

    def rnd(t):
        if peak is not None:
            peak.append(float(t.abs().max()))
        return t.half().double() if round_acts else t

    x = F.conv2d(R.f64(frames), p["stem_w"], p["stem_b"], stride=2, padding=3).relu()
    x = rnd(F.max_pool2d(x, 3, 2, 1))
    for b, t in enumerate(lay):
        s, c = t["stride"], t["convs"]
        if bottleneck:
            a = rnd(F.conv2d(x, p[f"c{c[0]}_w"], p[f"c{c[0]}_b"]).relu())
            a = rnd(F.conv2d(a, p[f"c{c[1]}_w"], p[f"c{c[1]}_b"], stride=s, padding=1).relu())
            y = F.conv2d(a, p[f"c{c[2]}_w"], p[f"c{c[2]}_b"])
        else:
            a = rnd(F.conv2d(x, p[f"c{c[0]}_w"], p[f"c{c[0]}_b"], stride=s, padding=1).relu())
            y = F.conv2d(a, p[f"c{c[1]}_w"], p[f"c{c[1]}_b"], padding=1)
        if t["shortcut"] and fused:
            y = y + F.conv2d(x, p[f"c{t['short']}_w"], None, stride=s)         # its bias is inside the closing convolution's
        elif t["shortcut"]:
            y = y + rnd(F.conv2d(x, p[f"c{t['short']}_w"], p[f"c{t['short']}_b"], stride=s))
        else:
            y = y + x
        y = y.relu()
        x = y if b == len(lay) - 1 else rnd(y)
    return (x.mean((2, 3)) @ p["head_w"].T + p["head_b"]).numpy()


def module64(net, frames):
    """The original module in float64 on frames ``[B, 3, H, W]``."""
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(R.f64(frames)).numpy()


def make_net(case):
    block, blocks, B, H, W, classes, seed_net, seed_x = case
    return synth.seeded_module(lambda: ResNet(block, blocks, classes), seed_net)


@functools.lru_cache(maxsize=None)
def e2e(case):
    """One end-to-end case, computed once and shared (callers leave it unchanged): a dict with ``net``, fp32 frames ``x``, the
    float64 logits ``quant`` (quantised network), ``emu`` (fused emulation), ``emu_split``, ``orig`` (original module) and ``peak``
    (the largest stored activation of the fused emulation)."""
    block, blocks, B, H, W, classes, seed_net, seed_x = case
    bott = block == "bottleneck"
    net = make_net(case)
    x = synth.seeded_clip((B, 3, H, W), seed_x)
    x16 = x.half()
    pf, ps, peak = pack64(net, fused=True), pack64(net, fused=False), []
    return {"net": net, "x": x, "quant": network64(pf, x16, False, True, bott, blocks),
            "emu": network64(pf, x16, True, True, bott, blocks, peak=peak), "emu_split": network64(ps, x16, True, False, bott, blocks),
            "orig": module64(net, x), "peak": max(peak)}


@functools.lru_cache(maxsize=None)
def stage_case(case, fused):
    """(net, packed float64 weights of that form, fp16 frames) of one case for the per-stage tests."""
    block, blocks, B, H, W, classes, seed_net, seed_x = case
    net = make_net(case)
    return net, pack64(net, fused=fused), synth.seeded_clip((B, 3, H, W), seed_x).half()


def clear_frames(case, quant):
    """Per frame whether its quantised top-6 gap exceeds 2 TOL_Q of the case."""
    return [g > 2 * TOL_Q[case] for g in top_gaps(quant)]
