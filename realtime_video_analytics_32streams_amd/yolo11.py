"""YOLO11 n/s/m/l/x detector network, written from the published ``yolo11.yaml`` of Ultralytics 8.3.

YOLO11 is the default family of the library the reference drives (``yolo11n.pt`` ... ``yolo11x.pt``).  Its head tensor is
YOLOv8's ``[B, 4 + nc, A]`` (xywh in input pixels, post-sigmoid class scores), so everything behind the network is unchanged.
What is new against YOLOv8: ``C3k2`` blocks (a C2f whose inner block is a half-width bottleneck or a small C3), the ``C2PSA``
block behind SPPF (multi-head self-attention over the stride-32 map, with a depthwise 3x3 positional encoding), and a class
branch of depthwise + pointwise convolutions in the detect head.  The fused plan is ``engine.FusedYolo11``
(``rva_yolo11_plan_create``).

That library is not a dependency: the layout below is a restatement, and the loader checks every shape of a state dict against
it and names the first key that does not fit.  As for YOLOv8 there are no weights offline: a network is seeded unless
``model_path`` names a local state dict.
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .yolov8 import SPPF, ConvBnAct, DetectHead, _divisible, apply_class_shifts, density_shifts

# depth multiple, width multiple, max channels  (yolo11.yaml scales)
SCALES_11 = {"n": (0.50, 0.25, 1024), "s": (0.50, 0.50, 1024), "m": (0.50, 1.00, 512), "l": (1.00, 1.00, 512),
             "x": (1.00, 1.50, 512)}
KEY_DIM, HEAD_DIM = 32, 64              # per attention head, at every scale (attn_ratio 0.5, heads = c // 64)


class Bottleneck11(nn.Module):
    """``x + cv2_3x3(cv1_3x3(x))`` with ``e * c`` channels in between, without the add when ``shortcut`` is false."""

    def __init__(self, c, shortcut=True, e=0.5):
        super().__init__()
        c_ = int(c * e)
        self.cv1 = ConvBnAct(c, c_, 3)
        self.cv2 = ConvBnAct(c_, c, 3)
        self.add = shortcut

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C3k(nn.Module):
    """C3 at half width with full-width 3x3 bottlenecks: ``cv3(cat(m(cv1(x)), cv2(x)))``."""

    def __init__(self, c, n=2, shortcut=True):
        super().__init__()
        c_ = c // 2
        self.cv1 = ConvBnAct(c, c_, 1)
        self.cv2 = ConvBnAct(c, c_, 1)
        self.cv3 = ConvBnAct(2 * c_, c, 1)
        self.m = nn.ModuleList(Bottleneck11(c_, shortcut, 1.0) for _ in range(n))

    def forward(self, x):
        y = self.cv1(x)
        for m in self.m:
            y = m(y)
        return self.cv3(torch.cat((y, self.cv2(x)), 1))


class C3k2(nn.Module):
    """C2f with ``c = int(c2 * e)`` whose inner blocks are ``Bottleneck11(c, e=0.5)`` or, with ``c3k``, ``C3k(c, 2)``."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, shortcut=True):
        super().__init__()
        self.c = int(c2 * e)
        self.c3k = bool(c3k)
        self.cv1 = ConvBnAct(c1, 2 * self.c, 1)
        self.cv2 = ConvBnAct((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(C3k(self.c, 2, shortcut) if c3k else Bottleneck11(self.c, shortcut, 0.5) for _ in range(n))

    def forward(self, x):
        y = list(self.cv1(x).chunk(2, 1))
        for m in self.m:
            y.append(m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class Attention(nn.Module):
    """Multi-head self-attention over the pixels of a map.  Per head the 128 ``qkv`` channels are ``[q 32 | k 32 | v 64]``;
    ``attn = softmax(q^T k * 32^-0.5)`` over keys, ``out = v attn^T``, then ``proj(out + pe(v))`` with ``pe`` a depthwise 3x3."""

    def __init__(self, c):
        super().__init__()
        assert c % HEAD_DIM == 0, "attention width must be a multiple of 64"
        self.num_heads, self.key_dim, self.head_dim = c // HEAD_DIM, KEY_DIM, HEAD_DIM
        self.scale = KEY_DIM ** -0.5
        self.qkv = ConvBnAct(c, c + 2 * KEY_DIM * self.num_heads, 1, act=False)
        self.proj = ConvBnAct(c, c, 1, act=False)
        self.pe = ConvBnAct(c, c, 3, act=False)
        self.pe.conv = nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False)

    def forward(self, x):
        b, c, h, w = x.shape
        qkv = self.qkv(x).view(b, self.num_heads, 2 * KEY_DIM + HEAD_DIM, h * w)
        q, k, v = qkv.split([KEY_DIM, KEY_DIM, HEAD_DIM], 2)
        attn = ((q.transpose(-2, -1) @ k) * self.scale).softmax(-1)
        out = (v @ attn.transpose(-2, -1)).view(b, c, h, w)
        return self.proj(out + self.pe(v.reshape(b, c, h, w)))


class PSABlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attn = Attention(c)
        self.ffn = nn.Sequential(ConvBnAct(c, 2 * c, 1), ConvBnAct(2 * c, c, 1, act=False))

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.ffn(x)


class C2PSA(nn.Module):
    def __init__(self, c1, n=1):
        super().__init__()
        self.c = c1 // 2
        self.cv1 = ConvBnAct(c1, 2 * self.c, 1)
        self.cv2 = ConvBnAct(2 * self.c, c1, 1)
        self.m = nn.ModuleList(PSABlock(self.c) for _ in range(n))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), 1)
        for m in self.m:
            b = m(b)
        return self.cv2(torch.cat((a, b), 1))


class _DWConv(ConvBnAct):
    """Depthwise 3x3 + BatchNorm + SiLU."""

    def __init__(self, c):
        super().__init__(c, c, 3)
        self.conv = nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False)


def _fuse(m: ConvBnAct) -> None:
    """``ConvBnAct.fuse`` for any group count (it rebuilds the convolution dense)."""
    if m.fused:
        return
    g = m.conv.groups
    if g == 1:
        m.fuse()
        return
    w = m.conv.weight
    scale = m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)
    conv = nn.Conv2d(m.conv.in_channels, m.conv.out_channels, m.conv.kernel_size, m.conv.stride, m.conv.padding, groups=g,
                     bias=True).to(w.device, w.dtype)
    with torch.no_grad():
        conv.weight.copy_(w * scale.view(-1, 1, 1, 1))
        conv.bias.copy_(m.bn.bias - m.bn.running_mean * scale)
    m.conv, m.bn, m.fused = conv, nn.Identity(), True


class Detect11(DetectHead):
    """YOLOv8's head (DFL, decode, ``[B, 4 + nc, A]``) with the class branch of YOLO11:
    ``[DWConv(x) -> Conv(x, c3, 1)] -> [DWConv(c3) -> Conv(c3, c3, 1)] -> Conv2d(c3, nc, 1)``."""

    def __init__(self, nc, ch, strides=(8, 16, 32), reg_max=16):
        super().__init__(nc, ch, strides, reg_max)
        c3 = max(ch[0], min(nc, 100))
        last = [seq[-1] for seq in self.cls]                 # keeps the prior initialisation of the bias
        self.cls = nn.ModuleList(nn.Sequential(nn.Sequential(_DWConv(c), ConvBnAct(c, c3, 1)),
                                               nn.Sequential(_DWConv(c3), ConvBnAct(c3, c3, 1)), conv)
                                 for c, conv in zip(ch, last))


class Yolo11(nn.Module):
    def __init__(self, scale: str = "n", nc: int = 80):
        super().__init__()
        d, w, mc = SCALES_11[scale]
        ch = lambda c: _divisible(min(c, mc) * w)      # noqa: E731
        rep = lambda n: max(round(n * d), 1)           # noqa: E731
        k = scale in "mlx"                              # these scales run C3k inside every C3k2
        c1, c2, c3, c4, c5 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        self.scale, self.nc = scale, nc
        self.l0 = ConvBnAct(3, c1, 3, 2)
        self.l1 = ConvBnAct(c1, c2, 3, 2)
        self.l2 = C3k2(c2, c3, rep(2), k, 0.25)
        self.l3 = ConvBnAct(c3, c3, 3, 2)
        self.l4 = C3k2(c3, c4, rep(2), k, 0.25)
        self.l5 = ConvBnAct(c4, c4, 3, 2)
        self.l6 = C3k2(c4, c4, rep(2), True)
        self.l7 = ConvBnAct(c4, c5, 3, 2)
        self.l8 = C3k2(c5, c5, rep(2), True)
        self.l9 = SPPF(c5, c5, 5)
        self.l10 = C2PSA(c5, rep(2))
        self.l13 = C3k2(c5 + c4, c4, rep(2), k, shortcut=False)
        self.l16 = C3k2(c4 + c4, c3, rep(2), k, shortcut=False)
        self.l17 = ConvBnAct(c3, c3, 3, 2)
        self.l19 = C3k2(c3 + c4, c4, rep(2), k, shortcut=False)
        self.l20 = ConvBnAct(c4, c4, 3, 2)
        self.l22 = C3k2(c4 + c5, c5, rep(2), True, shortcut=False)
        self.detect = Detect11(nc, (c3, c4, c5))

    def features(self, x):
        x = self.l2(self.l1(self.l0(x)))
        p3 = self.l4(self.l3(x))
        p4 = self.l6(self.l5(p3))
        p5 = self.l10(self.l9(self.l8(self.l7(p4))))
        n4 = self.l13(torch.cat((F.interpolate(p5, scale_factor=2.0, mode="nearest"), p4), 1))
        n3 = self.l16(torch.cat((F.interpolate(n4, scale_factor=2.0, mode="nearest"), p3), 1))
        m4 = self.l19(torch.cat((self.l17(n3), n4), 1))
        m5 = self.l22(torch.cat((self.l20(m4), p5), 1))
        return [n3, m4, m5]

    def forward(self, x, raw: bool = False):
        return self.detect(self.features(x), raw=raw)

    @torch.no_grad()
    def fuse(self):
        for m in self.modules():
            if isinstance(m, ConvBnAct):
                _fuse(m)
        return self


_NAME_11 = re.compile(r"^yolov?11([nsmlx])")


def variant_from_path_11(model_path: str) -> Optional[str]:
    """Scale letter of a ``yolo11<n|s|m|l|x>...`` / ``yolov11<...>...`` file name (any directory, suffix and letter case);
    ``None`` for every other name."""
    m = _NAME_11.match(Path(model_path or "").stem.lower())
    return m.group(1) if m else None


# Ultralytics layer index (yolo11.yaml: backbone 0-10, head 11-23; 11/12/14/15/18/21 are Upsample / Concat without parameters)
_ULTRALYTICS_11_LAYERS = {i: f"l{i}" for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 16, 17, 19, 20, 22)}
_DETECT_LAYER = 23


def _strip_model(key: str) -> str:
    while key.startswith("model."):
        key = key[len("model."):]
    return key


def map_ultralytics_11_state_dict(sd, net: "Yolo11") -> dict:
    """Rename an Ultralytics-style YOLO11 state dict (``model.N...`` / ``N...`` keys; ``model.23.cv2`` = box branch, ``.cv3`` =
    class branch, ``.dfl`` = the fixed 0..15 projection) to this module's names, with a shape check against ``net``."""
    own = net.state_dict()
    out = {}
    for key, val in sd.items():
        k = _strip_model(key)
        idx, _, rest = k.partition(".")
        if not idx.isdigit():
            raise KeyError(f"'{key}' is not an Ultralytics YOLO11 parameter name (expected model.<layer>....)")
        i = int(idx)
        if i == _DETECT_LAYER:
            branch, _, tail = rest.partition(".")
            if branch == "dfl":
                if tuple(val.shape) != (1, 16, 1, 1) or not torch.equal(val.flatten().float(), torch.arange(16.0)):
                    raise ValueError("model.23.dfl is not the fixed 0..15 projection this head computes in closed form")
                continue
            if branch not in ("cv2", "cv3"):
                raise KeyError(f"unknown detect-head entry '{key}'")
            new = ("detect.box." if branch == "cv2" else "detect.cls.") + tail
        elif i in _ULTRALYTICS_11_LAYERS:
            new = _ULTRALYTICS_11_LAYERS[i] + "." + rest
        else:
            raise KeyError(f"'{key}': layer {i} has no parameters in YOLO11 (Upsample / Concat)")
        if new.endswith("num_batches_tracked") and new not in own:
            continue
        if new not in own:
            raise KeyError(f"'{key}' -> '{new}' does not exist in YOLO11{net.scale} (wrong model scale?)")
        if tuple(own[new].shape) != tuple(val.shape):
            raise ValueError(f"'{key}': shape {tuple(val.shape)} does not fit YOLO11{net.scale}'s {new} {tuple(own[new].shape)}")
        out[new] = val
    missing = [k for k in own if k not in out and not k.endswith("num_batches_tracked")]
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} parameters of YOLO11{net.scale}, e.g. {missing[:3]}")
    return out


def load_detector_state_dict_11(net: "Yolo11", sd) -> "Yolo11":
    """This module's own naming, or Ultralytics naming (detected by its ``model.N`` / ``N`` layer-index keys)."""
    if _strip_model(next(iter(sd))).split(".", 1)[0].isdigit():
        net.load_state_dict(map_ultralytics_11_state_dict(sd, net), strict=False)      # only num_batches_tracked may be absent
        return net
    own = net.state_dict()
    for key, val in sd.items():
        if key not in own:
            raise KeyError(f"'{key}' does not exist in YOLO11{net.scale} (wrong model scale?)")
        if tuple(own[key].shape) != tuple(val.shape):
            raise ValueError(f"'{key}': shape {tuple(val.shape)} does not fit YOLO11{net.scale}'s {tuple(own[key].shape)}")
    missing = [k for k in own if k not in sd and not k.endswith("num_batches_tracked")]
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} parameters of YOLO11{net.scale}, e.g. {missing[:3]}")
    net.load_state_dict(sd, strict=False)
    return net


# the attention convolution of the first PSA block: bn not folded / folded, under Ultralytics' (outer, inner) and this module's names
_11_QKV_KEYS = tuple(f"{p}10.m.0.attn.qkv.conv.weight" for p in ("model.", "", "l"))
_11_LAST_CLASS_CONV = ("detect.cls.0.2.weight", "model.23.cv3.0.2.weight", "23.cv3.0.2.weight")
_11_STEM_KEYS = ("l0.conv.weight", "model.0.conv.weight", "0.conv.weight")
_11_PSA1_KEYS = tuple(f"{p}10.m.1.attn.qkv.conv.weight" for p in ("model.", "", "l"))


def is_11_state_dict(sd) -> bool:
    """Whether a state dict is a YOLO11 one: it has the attention convolution of C2PSA under this module's or Ultralytics' name."""
    return hasattr(sd, "keys") and any(k in sd for k in _11_QKV_KEYS)


def checkpoint_class_count_11(sd) -> Optional[int]:
    """Classes of a YOLO11 state dict: the output channels of the class branch's last convolution; ``None`` without one."""
    for key in _11_LAST_CLASS_CONV if hasattr(sd, "get") else ():
        w = sd.get(key)
        if w is not None and getattr(w, "dim", lambda: 0)() == 4:
            return int(w.shape[0])
    return None


def scale_of_11(model_path: str, state_dict=None) -> str:
    """Scale letter of a YOLO11 model: from the shapes of its state dict (stem width 16 n, 32 s, 96 x; 64 is m or l, told apart
    by the second PSA block only l has), else from the file name, else ``"n"``."""
    if state_dict is not None:
        for key in _11_STEM_KEYS:
            w = state_dict.get(key)
            if w is not None:
                c = int(w.shape[0])
                if c == 64:
                    return "l" if any(k in state_dict for k in _11_PSA1_KEYS) else "m"
                s = {16: "n", 32: "s", 96: "x"}.get(c)
                if s:
                    return s
    return variant_from_path_11(model_path) or "n"


def build_detector_net_11(scale: str = "n", seed: int = 0, weights: Optional[str] = None, nc: Optional[int] = None) -> Yolo11:
    """Seeded random-init network with the BatchNorm recipe of ``yolov8.build_detector_net``, or a local state dict when
    ``weights`` names an existing file (``weights_only=True``; nothing is ever fetched by name).  ``nc=None``: the class count of
    that file, 80 without one."""
    sd = None
    if weights and Path(weights).is_file():
        sd = torch.load(weights, map_location="cpu", weights_only=True)
    if nc is None:
        nc = (checkpoint_class_count_11(sd) if sd is not None else None) or 80
    g = torch.Generator().manual_seed(seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        net = Yolo11(scale, nc)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    finally:
        torch.random.set_rng_state(state)
    if sd is not None:
        load_detector_state_dict_11(net, sd)
    net.eval()
    return net


@torch.no_grad()
def calibrate_detection_density_11(net: Yolo11, sample: Optional[torch.Tensor], conf_thr: float, target_per_image: int = 120,
                                   iters: int = 24, class_logits: Optional[torch.Tensor] = None) -> Tuple[float, float]:
    """Synthetic-weight helper (tests / tools only): YOLOv8's class-logit shift (``yolov8.density_shifts``) on the last class
    convolution of every level.  Returns the two shifts applied (class 0, classes >= 1)."""
    cls = net(sample, raw=True)[1] if class_logits is None else class_logits
    s0, sr = density_shifts(cls, conf_thr, target_per_image, iters)
    apply_class_shifts(net, s0, sr)
    return s0, sr
