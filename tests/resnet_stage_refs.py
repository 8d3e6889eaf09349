"""Float64 references and derived rounding bounds for every stage of the fp32 ResNet-18 plan (csrc/rva_resnet.hip), shared by
tests/test_resnet_stages_host.py (CPU: the bounds see the bugs) and tests/test_gpu_resnet_stages.py.

Every stage is computed in float64 from the tensor the kernel under test itself read (the tap of the stage before it), so a
bound covers the rounding of ONE kernel.  The bounds are derived as in tests/clip_stage_refs.py, with u = 2**-24: an fp32 dot
product of n terms plus a bias errs by at most (n + 2) u (sum |w_i x_i| + |b|) in any order, one more u per further addition,
and ReLU / max are 1-Lipschitz:

  * ``pooled``          the stem bound of clip_stage_refs (n = 147) taken through the max pool
  * ``mid<b>``          (9 Cin + 2) u (conv(|x|, |w|) + |b|)
  * ``down<b>``         (Cin + 2) u (conv(|x|, |w|) + |b|)
  * ``out<b>``          (9 C + 3) u (conv(|a|, |w|) + |b| + |r|), r = the shortcut (the block's input or its ``down``)
  * ``feat``            (P + 1) u sum |v| / P over the P pixels of the last map
  * ``logits``          (512 + 2) u (|f| . |W|^T + |b|)

Layouts are those of ``rva_resnet_plan_stage`` (include/rva.h): NHWC."""
import torch
import torch.nn.functional as F

from realtime_video_analytics_32streams_amd import synth
from realtime_video_analytics_32streams_amd.classify import ResNet18
from realtime_video_analytics_32streams_amd.resnet_plan import block_shapes, pack_resnet18
from tests.clip_stage_refs import U, conv_bound, f64, linear, ratio, report, shape_id, stem_conv, stem_pool  # noqa: F401

# (B, H, W, classes, capacity)
SHAPES = [(1, 32, 32, 10, 1), (3, 34, 34, 10, 4), (5, 40, 72, 37, 5), (17, 64, 64, 10, 17)]
BLOCKS = block_shapes()                       # (cin, cout, stride) of the eight blocks
DOWN = (2, 4, 6)                              # blocks with a shortcut convolution
CONV_OF = {}                                  # stage name -> index of its convolution in the ABI's weight order
_i = 0
for _b, (_cin, _c, _s) in enumerate(BLOCKS):
    CONV_OF[f"mid{_b}"], CONV_OF[f"out{_b}"] = _i, _i + 1
    _i += 2
    if _cin != _c:
        CONV_OF[f"down{_b}"] = _i
        _i += 1
STAGES = ("pooled",) + tuple(n for b in range(8) for n in ([f"mid{b}"] + ([f"down{b}"] if b in DOWN else []) + [f"out{b}"])) + ("feat",)


def case(shape):
    """Seeded module, its packed fp32 weights as float64 tensors (block convolutions back in the module's ``[co, ci, k, k]``) and
    frames ``[B, 3, H, W]`` fp32 of one shape."""
    B, H, W, classes, _ = shape
    seed = 300 + SHAPES.index(tuple(shape))
    net = synth.seeded_module(lambda: ResNet18(classes), seed)
    p = {k: f64(v) for k, v in pack_resnet18(net).items()}
    for i in range(19):
        w = p[f"c{i}_w"]
        k = int(round(w.shape[1] ** 0.5))
        p[f"c{i}_w"] = w.permute(0, 2, 1).reshape(w.shape[0], w.shape[2], k, k).contiguous()
    return net, p, synth.seeded_clip((B, 3, H, W), seed + 50)


def nchw(t):
    return f64(t).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def block_conv(name, x, p, **kw):
    """The convolution of stage ``name`` on ``x`` (NCHW float64) -> (conv + bias, bound before the epilogue's extra terms)."""
    i = CONV_OF[name]
    b = int(name[-1])
    cin, c, s = BLOCKS[b]
    if name.startswith("mid"):
        return conv_bound(F.conv2d, x, p[f"c{i}_w"], p[f"c{i}_b"], 9 * cin, **{"stride": s, "padding": 1, **kw})
    if name.startswith("down"):
        return conv_bound(F.conv2d, x, p[f"c{i}_w"], p[f"c{i}_b"], cin, **{"stride": 2, "padding": 0, **kw})
    return conv_bound(F.conv2d, x, p[f"c{i}_w"], p[f"c{i}_b"], 9 * c + 1, **{"padding": 1, **kw})


def out_stage(b, a, r, p):
    """``out<b>`` from the ``mid`` tap ``a`` and the shortcut ``r`` (both NCHW float64) -> (ref, bound), NHWC."""
    y, t = block_conv(f"out{b}", a, p)                     # t = (9 C + 3) u (conv(|a|, |w|) + |b|)
    c = BLOCKS[b][1]
    return nhwc((y + r).relu()), nhwc(t + (9 * c + 3) * U * r.abs())


def feat_stage(v):
    """Last map ``[B, h, w, 512]`` -> (mean ``[B, 512]``, bound)."""
    v = f64(v).flatten(1, 2)
    P = v.shape[1]
    return v.sum(1) / P, (P + 1) * U * v.abs().sum(1) / P


def refs(taps, frames, p, shape):
    """``taps``: name -> fp32 tensor in the tap layout.  Returns name -> (ref, tol) with each stage computed from the tap(s) it
    read.  ``taps = None`` chains the references themselves, each rounded once to fp32 (what an exact kernel would leave)."""
    out = {}
    tap = (lambda k: taps[k]) if taps is not None else (lambda k: out[k][0].float())
    out["pooled"] = stem_pool(*stem_conv(f64(frames), {"conv1_w": p["stem_w"], "conv1_b": p["stem_b"]}))
    prev = "pooled"
    for b in range(8):
        x = nchw(tap(prev))
        y, t = block_conv(f"mid{b}", x, p)
        out[f"mid{b}"] = (nhwc(y.relu()), nhwc(t))
        r = x
        if b in DOWN:
            y, t = block_conv(f"down{b}", x, p)
            out[f"down{b}"] = (nhwc(y), nhwc(t))
            r = nchw(tap(f"down{b}"))
        out[f"out{b}"] = out_stage(b, nchw(tap(f"mid{b}")), r, p)
        prev = f"out{b}"
    out["feat"] = feat_stage(tap("out7"))
    out["logits"] = linear(tap("feat"), p["head_w"], p["head_b"], 512)
    return out


def topk_rule(logits, k):
    """The reference's top-k on host logits ``[n, classes]`` (ascending stable sort, last k reversed) -> (classes, scores)."""
    order = torch.sort(logits, dim=1, stable=True).indices[:, -k:].flip(1)
    return order, torch.gather(logits, 1, order)
