"""YOLOv5 n/s/m/l/x detector network (v6.0 - v7.0 architecture), written from the published ``yolov5{n,s,m,l,x}.yaml``.

``model_type: yolov5`` is a documented value of the reference's configuration, and its post-process
(``scores = pred[:, 5:] * pred[:, 4:5]``, detector.py:294-305) is the YOLOv5 objectness rule.  The reference runs the exported
graph, whose single output is ``[B, A, 5 + nc]`` = (cx, cy, w, h in input pixels, objectness, nc class scores, all post-sigmoid)
with ``A = 3 * (h3 w3 + h4 w4 + h5 w5)`` anchors (25200 at 640 x 640).  This module produces that tensor; the fused plan
(``engine.FusedYoloV5``, ``rva_yolov5_plan_create``) produces its transpose ``[B, 5 + nc, A]``, which K2 reads through strides.

As for YOLOv8 there are no weights offline: a network is seeded unless ``model_path`` names a local state dict.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .yolov8 import SPPF, ConvBnAct, _divisible

# depth multiple, width multiple  (yolov5{n,s,m,l,x}.yaml)
SCALES_V5 = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.00, 1.00), "x": (1.33, 1.25)}

# anchors in input pixels, per level (stride 8 / 16 / 32): three (w, h) pairs each
DEFAULT_ANCHORS = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))
STRIDES = (8, 16, 32)


class Bottleneck5(nn.Module):
    """``x + cv2_3x3(cv1_1x1(x))`` (expansion 1.0 inside C3), without the add when ``shortcut`` is false."""

    def __init__(self, c, shortcut=True):
        super().__init__()
        self.cv1 = ConvBnAct(c, c, 1)
        self.cv2 = ConvBnAct(c, c, 3)
        self.add = shortcut

    def forward(self, x):
        y = self.cv2(self.cv1(x))
        return x + y if self.add else y


class C3(nn.Module):
    """CSP bottleneck with three convolutions: ``cv3(cat(m(cv1(x)), cv2(x)))``."""

    def __init__(self, c1, c2, n=1, shortcut=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = ConvBnAct(c1, c_, 1)
        self.cv2 = ConvBnAct(c1, c_, 1)
        self.cv3 = ConvBnAct(2 * c_, c2, 1)
        self.m = nn.ModuleList(Bottleneck5(c_, shortcut) for _ in range(n))

    def forward(self, x):
        y = self.cv1(x)
        for m in self.m:
            y = m(y)
        return self.cv3(torch.cat((y, self.cv2(x)), 1))


class Detect5(nn.Module):
    """Anchor-based head: per level one ``Conv2d(ch, 3 * (5 + nc), 1)``; channel ``a * (5 + nc) + j`` is anchor ``a``, entry ``j``.

    ``y = sigmoid``; ``xy = (2 y[0:2] - 0.5 + (gx, gy)) * stride``; ``wh = (2 y[2:4])^2 * anchor_px``; entries 4.. are ``y``.
    Inference output ``[B, A, 5 + nc]``, anchor index = level offset + ``a * h * w + y * w + x``."""

    def __init__(self, nc: int, ch: Sequence[int], anchors=None, strides=STRIDES):
        super().__init__()
        self.nc, self.no, self.na, self.strides = nc, nc + 5, 3, tuple(strides)
        a = torch.tensor(DEFAULT_ANCHORS if anchors is None else anchors, dtype=torch.float32).reshape(3, 3, 2)
        self.register_buffer("anchors_px", a)               # [level, anchor, (w, h)] in input pixels
        self.m = nn.ModuleList(nn.Conv2d(c, self.na * self.no, 1) for c in ch)
        for m, s in zip(self.m, self.strides):              # the architecture's prior initialisation
            b = m.bias.data.view(self.na, -1)
            b[:, 4] += math.log(8 / (640 / s) ** 2)
            b[:, 5:] += math.log(0.6 / (nc - 0.99999))

    def forward(self, feats: List[torch.Tensor], raw: bool = False):
        maps = [m(f) for m, f in zip(self.m, feats)]
        if raw:
            return maps
        out = []
        for lv, (z, s) in enumerate(zip(maps, self.strides)):
            b, _, h, w = z.shape
            # a half module decodes in fp32 and rounds once; a float64 module (the references) stays float64 throughout
            cd = z.dtype if z.dtype == torch.float64 else torch.float32
            y = z.view(b, self.na, self.no, h, w).permute(0, 1, 3, 4, 2).to(cd).sigmoid()
            gy, gx = torch.meshgrid(torch.arange(h, device=z.device, dtype=cd), torch.arange(w, device=z.device, dtype=cd), indexing="ij")
            grid = torch.stack((gx, gy), -1).view(1, 1, h, w, 2)
            xy = (y[..., 0:2] * 2 - 0.5 + grid) * float(s)
            t = y[..., 2:4] * 2
            wh = t * t * self.anchors_px[lv].to(cd).view(1, self.na, 1, 1, 2)
            out.append(torch.cat((xy, wh, y[..., 4:]), -1).reshape(b, self.na * h * w, self.no).to(z.dtype))
        return torch.cat(out, 1)


class YoloV5(nn.Module):
    def __init__(self, scale: str = "s", nc: int = 80, anchors=None):
        super().__init__()
        d, w = SCALES_V5[scale]
        ch = lambda c: _divisible(c * w)                # noqa: E731
        rep = lambda n: max(round(n * d), 1)            # noqa: E731
        c1, c2, c3, c4, c5 = ch(64), ch(128), ch(256), ch(512), ch(1024)
        self.scale, self.nc = scale, nc
        self.b0 = ConvBnAct(3, c1, 6, 2)
        self.b0.conv = nn.Conv2d(3, c1, 6, 2, 2, bias=False)       # k6 s2 p2 (ConvBnAct pads k // 2)
        self.b1 = ConvBnAct(c1, c2, 3, 2)
        self.b2 = C3(c2, c2, rep(3))
        self.b3 = ConvBnAct(c2, c3, 3, 2)
        self.b4 = C3(c3, c3, rep(6))
        self.b5 = ConvBnAct(c3, c4, 3, 2)
        self.b6 = C3(c4, c4, rep(9))
        self.b7 = ConvBnAct(c4, c5, 3, 2)
        self.b8 = C3(c5, c5, rep(3))
        self.b9 = SPPF(c5, c5, 5)
        self.h10 = ConvBnAct(c5, c4, 1)
        self.h13 = C3(2 * c4, c4, rep(3), False)
        self.h14 = ConvBnAct(c4, c3, 1)
        self.h17 = C3(2 * c3, c3, rep(3), False)
        self.h18 = ConvBnAct(c3, c3, 3, 2)
        self.h20 = C3(2 * c3, c4, rep(3), False)
        self.h21 = ConvBnAct(c4, c4, 3, 2)
        self.h23 = C3(2 * c4, c5, rep(3), False)
        self.detect = Detect5(nc, (c3, c4, c5), anchors)

    def features(self, x):
        x = self.b2(self.b1(self.b0(x)))
        p3 = self.b4(self.b3(x))
        p4 = self.b6(self.b5(p3))
        p5 = self.b9(self.b8(self.b7(p4)))
        t10 = self.h10(p5)
        n4 = self.h13(torch.cat((F.interpolate(t10, scale_factor=2.0, mode="nearest"), p4), 1))
        t14 = self.h14(n4)
        n3 = self.h17(torch.cat((F.interpolate(t14, scale_factor=2.0, mode="nearest"), p3), 1))
        m4 = self.h20(torch.cat((self.h18(n3), t14), 1))
        m5 = self.h23(torch.cat((self.h21(m4), t10), 1))
        return [n3, m4, m5]

    def forward(self, x, raw: bool = False):
        return self.detect(self.features(x), raw=raw)

    @torch.no_grad()
    def fuse(self):
        for m in self.modules():
            if isinstance(m, ConvBnAct):
                m.fuse()
        return self


def variant_from_path_v5(model_path: str) -> Optional[str]:
    """Scale letter of a ``yolov5<n|s|m|l|x>...`` file name; ``None`` for any other name and for the ``yolov5*u`` names
    (upstream's anchor-free re-exports, which carry the YOLOv8 head)."""
    name = Path(model_path or "").stem.lower()
    if len(name) < 7 or not name.startswith("yolov5") or name[6] not in "nsmlx":
        return None
    if name[7:8] == "u" or name[7:9] == "6u":
        return None
    return name[6]


# Ultralytics layer index (yolov5*.yaml: backbone 0-9, head 10-24; 11/12/15/16/19/22 are Upsample / Concat without parameters)
_ULTRALYTICS_V5_LAYERS = {0: "b0", 1: "b1", 2: "b2", 3: "b3", 4: "b4", 5: "b5", 6: "b6", 7: "b7", 8: "b8", 9: "b9", 10: "h10",
                          13: "h13", 14: "h14", 17: "h17", 18: "h18", 20: "h20", 21: "h21", 23: "h23"}


def _strip_model(key: str) -> str:
    while key.startswith("model."):
        key = key[len("model."):]
    return key


def map_ultralytics_v5_state_dict(sd, net: "YoloV5") -> dict:
    """Rename an Ultralytics-style YOLOv5 state dict (``model.N...`` / ``N...`` keys; ``model.24.m.{0,1,2}`` = the detect
    convolutions, ``model.24.anchors`` ``[3, 3, 2]`` in units of each level's stride) to this module's names, with a shape check
    against ``net``.  The checkpoint's own anchors are honoured: multiplied by the stride they become ``detect.anchors_px``."""
    own = net.state_dict()
    out = {}
    for key, val in sd.items():
        k = _strip_model(key)
        idx, _, rest = k.partition(".")
        if not idx.isdigit():
            raise KeyError(f"'{key}' is not an Ultralytics YOLOv5 parameter name (expected model.<layer>....)")
        i = int(idx)
        if i == 24:
            if rest == "anchors":
                if tuple(val.shape) != (3, 3, 2):
                    raise ValueError(f"'{key}': shape {tuple(val.shape)} is not the [3, 3, 2] anchor table of a three-level head")
                out["detect.anchors_px"] = val.float() * torch.tensor(STRIDES, dtype=torch.float32).view(3, 1, 1)
                continue
            if rest == "anchor_grid" or rest.startswith("anchor_grid."):
                continue                                 # derived from anchors in older exports
            if not rest.startswith("m."):
                raise KeyError(f"unknown detect-head entry '{key}'")
            new = "detect." + rest
        elif i in _ULTRALYTICS_V5_LAYERS:
            new = _ULTRALYTICS_V5_LAYERS[i] + "." + rest
        else:
            raise KeyError(f"'{key}': layer {i} has no parameters in YOLOv5 (Upsample / Concat)")
        if new.endswith("num_batches_tracked"):
            continue
        if new not in own:
            raise KeyError(f"'{key}' -> '{new}' does not exist in YOLOv5{net.scale} (wrong model scale?)")
        if tuple(own[new].shape) != tuple(val.shape):
            raise ValueError(f"'{key}': shape {tuple(val.shape)} does not fit YOLOv5{net.scale}'s {new} {tuple(own[new].shape)}")
        out[new] = val
    missing = [k for k in own if k not in out and not k.endswith("num_batches_tracked") and k != "detect.anchors_px"]
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} parameters of YOLOv5{net.scale}, e.g. {missing[:3]}")
    return out


def load_detector_state_dict_v5(net: "YoloV5", sd) -> "YoloV5":
    """This module's own naming, or Ultralytics naming (detected by its ``model.N`` / ``N`` layer-index keys)."""
    if _strip_model(next(iter(sd))).split(".", 1)[0].isdigit():
        net.load_state_dict(map_ultralytics_v5_state_dict(sd, net), strict=False)      # num_batches_tracked / anchors may be absent
    else:
        net.load_state_dict(sd)
    return net


_V5_DETECT_KEYS = ("detect.m.0.weight", "model.24.m.0.weight", "24.m.0.weight")


def is_v5_state_dict(sd) -> bool:
    """Whether a state dict is a YOLOv5 one: it has the first detect convolution under this module's or Ultralytics' name."""
    return hasattr(sd, "keys") and any(k in sd for k in _V5_DETECT_KEYS)


def checkpoint_class_count_v5(sd) -> Optional[int]:
    """Classes of a YOLOv5 state dict: ``model.24.m.0.weight.shape[0] // 3 - 5``; ``None`` where the dict has no such entry."""
    for key in _V5_DETECT_KEYS if hasattr(sd, "get") else ():
        w = sd.get(key)
        if w is not None and getattr(w, "dim", lambda: 0)() == 4 and w.shape[0] % 3 == 0 and w.shape[0] // 3 > 5:
            return int(w.shape[0]) // 3 - 5
    return None


def build_detector_net_v5(scale: str = "s", seed: int = 0, weights: Optional[str] = None, nc: Optional[int] = None,
                          anchors=None) -> YoloV5:
    """Seeded random-init network with the BatchNorm recipe of ``yolov8.build_detector_net``, or a local state dict when
    ``weights`` names an existing file (``weights_only=True``; nothing is ever fetched by name).  ``nc=None``: the class count of
    that file, 80 without one."""
    sd = None
    if weights and Path(weights).is_file():
        sd = torch.load(weights, map_location="cpu", weights_only=True)
    if nc is None:
        nc = (checkpoint_class_count_v5(sd) if sd is not None else None) or 80
    g = torch.Generator().manual_seed(seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        net = YoloV5(scale, nc, anchors)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    finally:
        torch.random.set_rng_state(state)
    if sd is not None:
        load_detector_state_dict_v5(net, sd)
    net.eval()
    return net


@torch.no_grad()
def density_shifts_v5(maps: Sequence[torch.Tensor], nc: int, conf_thr: float, target_per_image: float, iters: int = 24,
                      objectness_quantile: float = 0.95) -> Tuple[float, float]:
    """The two bias shifts (objectness, class logits) under which about ``target_per_image`` anchors per image clear
    ``conf_thr`` under ``obj * max cls``.  ``maps``: the three raw logit maps ``[B, 3 * (5 + nc), h, w]``.  The anchors above
    ``objectness_quantile`` of the objectness logit are made confident (p = 0.9), the class shift is bisected.  Nothing is
    modified."""
    no = nc + 5
    zo, zc = [], []
    for z in maps:
        b = z.shape[0]
        v = z.float().view(b, 3, no, -1)
        zo.append(v[:, :, 4].reshape(b, -1))
        zc.append(v[:, :, 5:].max(2).values.reshape(b, -1))
    zo, zc = torch.cat(zo, 1), torch.cat(zc, 1)
    want = target_per_image * zo.shape[0]
    q = torch.quantile(zo.flatten()[:2_000_000], objectness_quantile).item()
    s0 = math.log(0.9 / 0.1) - q
    lo, hi = -40.0, 40.0
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if int(((torch.sigmoid(zo + s0) * torch.sigmoid(zc + mid)) >= conf_thr).sum()) > want:
            hi = mid
        else:
            lo = mid
    return s0, 0.5 * (lo + hi)


def apply_shifts_v5(net: "YoloV5", s_obj: float, s_cls: float) -> None:
    for m in net.detect.m:
        b = m.bias.data.view(3, -1)
        b[:, 4] += s_obj
        b[:, 5:] += s_cls


@torch.no_grad()
def calibrate_detection_density_v5(net: YoloV5, sample: torch.Tensor, conf_thr: float, target_per_image: int = 120,
                                   iters: int = 24) -> Tuple[float, float]:
    """Synthetic-weight helper (tests / tools only): shift the objectness and class biases of a seeded head so that about
    ``target_per_image`` anchors per image clear ``conf_thr``; a seeded head otherwise emits nothing.  Returns the shifts."""
    s0, sc = density_shifts_v5(net(sample, raw=True), net.nc, conf_thr, target_per_image, iters)
    apply_shifts_v5(net, s0, sc)
    return s0, sc
