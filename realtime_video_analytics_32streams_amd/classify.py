"""ResNet classification head behind the detector API (reference detector.py:870-1001).

The reference loads a ResNet from an OpenVINO / ONNX file and returns the top-K classes of the RAW output vector as
full-frame ``Detection`` objects (no softmax; ``np.argsort(output)[-k:][::-1]``, kept when ``>= confidence_threshold``).
Pre-process = the float32 ImageNet normalisation of the clip kernel on one frame (``rva_preprocess_frames_*``).  The
network here is a from-scratch torch ResNet-18 with seeded weights (no model files exist offline); any module or
``infer_fn`` mapping ``[B,3,H,W] -> [B,num_classes]`` can replace it.

Which network follows ``model_path``: an existing local state dict of the torchvision family builds a :class:`ResNet` of what the
file says (:func:`build_resnet`: ResNet-18 / 34 / 50 / 101 / 152 or any 1..64 blocks per stage); with no file, a name that starts
with ``resnet34`` / ``resnet50`` / ``resnet101`` / ``resnet152`` builds the seeded :class:`ResNet` of that depth; every other name
keeps the seeded :class:`ResNet18`.  :class:`ResNet` runs as engine ``"resnet-f16"`` (resnet_plan.FusedResNetF16) or through
PyTorch-ROCm; the fp32 plan ``"resnet-f32"`` exists for :class:`ResNet18` only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from . import ops
from .config import DetectorConfig
from .detector import BaseDetector, Detection
from .resnet_plan import ENGINE as RESNET_PLAN, ENGINE_F16 as RESNET_PLAN_F16, FusedResNet18, FusedResNet18F16, FusedResNetF16
from .video_stream import FramePacket


class _BasicBlock(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.c1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False); self.b1 = nn.BatchNorm2d(cout)
        self.c2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False); self.b2 = nn.BatchNorm2d(cout)
        self.down = None
        if stride != 1 or cin != cout:
            self.down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = torch.relu(self.b1(self.c1(x)))
        y = self.b2(self.c2(y))
        return torch.relu(y + (x if self.down is None else self.down(x)))


class ResNet18(nn.Module):
    def __init__(self, num_classes: int = 1000):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
                                  nn.MaxPool2d(3, 2, 1))
        cfg, blocks, cin = [(64, 1), (128, 2), (256, 2), (512, 2)], [], 64
        for cout, stride in cfg:
            blocks += [_BasicBlock(cin, cout, stride), _BasicBlock(cout, cout, 1)]
            cin = cout
        self.layers = nn.Sequential(*blocks)
        self.fc = nn.Linear(512, num_classes)

    def forward(self, x):
        return self.fc(self.layers(self.stem(x)).mean((2, 3)))


class BasicBlock(nn.Module):
    """torchvision's BasicBlock under its parameter names: 3x3 (stride), 3x3, a 1x1 ``downsample`` where the shape changes."""
    expansion = 1

    def __init__(self, cin: int, width: int, stride: int):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 3, stride, 1, bias=False); self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, 1, 1, bias=False); self.bn2 = nn.BatchNorm2d(width)
        self.downsample = None
        if stride != 1 or cin != width:
            self.downsample = nn.Sequential(nn.Conv2d(cin, width, 1, stride, bias=False), nn.BatchNorm2d(width))

    def forward(self, x):
        y = torch.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return torch.relu(y + (x if self.downsample is None else self.downsample(x)))


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride on the 3x3) under its parameter names: 1x1, 3x3 (stride), 1x1 to 4 x width."""
    expansion = 4

    def __init__(self, cin: int, width: int, stride: int):
        super().__init__()
        cout = width * self.expansion
        self.conv1 = nn.Conv2d(cin, width, 1, 1, 0, bias=False); self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False); self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, cout, 1, 1, 0, bias=False); self.bn3 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = torch.relu(self.bn1(self.conv1(x)))
        y = torch.relu(self.bn2(self.conv2(y)))
        y = self.bn3(self.conv3(y))
        return torch.relu(y + (x if self.downsample is None else self.downsample(x)))


RESNET_WIDTHS = (64, 128, 256, 512)
RESNET_DEPTHS = {18: ("basic", (2, 2, 2, 2)), 34: ("basic", (3, 4, 6, 3)), 50: ("bottleneck", (3, 4, 6, 3)),
                 101: ("bottleneck", (3, 4, 23, 3)), 152: ("bottleneck", (3, 8, 36, 3))}
_BLOCK_KINDS = {"basic": BasicBlock, "bottleneck": Bottleneck, BasicBlock: BasicBlock, Bottleneck: Bottleneck}


class ResNet(nn.Module):
    """Any ResNet of the torchvision family: ``block`` = ``"basic"`` or ``"bottleneck"`` (or the block class), ``blocks`` = blocks
    per stage (1..64 each), widths 64 / 128 / 256 / 512.  The parameter names -- and so the ``state_dict()`` keys -- are
    torchvision's: ``conv1``, ``bn1``, ``layer{1..4}.{j}.conv{1,2[,3]}`` / ``bn{1,2[,3]}`` / ``downsample.{0,1}``, ``fc``."""

    def __init__(self, block="bottleneck", blocks: Sequence[int] = (3, 4, 6, 3), num_classes: int = 1000):
        super().__init__()
        if block not in _BLOCK_KINDS:
            raise ValueError(f"ResNet: block must be 'basic' or 'bottleneck', got {block!r}")
        cls = _BLOCK_KINDS[block]
        blocks = tuple(int(n) for n in blocks)
        if len(blocks) != 4 or not all(1 <= n <= 64 for n in blocks):
            raise ValueError(f"ResNet: blocks must be four counts of 1..64, got {blocks}")
        self.block, self.blocks, self.expansion = ("bottleneck" if cls is Bottleneck else "basic"), blocks, cls.expansion
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for s, (width, n) in enumerate(zip(RESNET_WIDTHS, blocks)):
            layer = []
            for j in range(n):
                layer.append(cls(cin, width, 2 if (j == 0 and s > 0) else 1))
                cin = width * cls.expansion
            setattr(self, f"layer{s + 1}", nn.Sequential(*layer))
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(x.mean((2, 3)))


def resnet_depth_of(net) -> Optional[int]:
    """18 / 34 / 50 / 101 / 152 for a :class:`ResNet` of a standard depth, else ``None``."""
    for depth, (block, blocks) in RESNET_DEPTHS.items():
        if (net.block, tuple(net.blocks)) == (block, blocks):
            return depth
    return None


def resnet_depth_from_path(model_path: str) -> Optional[int]:
    """34 / 50 / 101 / 152 when the file name starts with ``resnet<depth>`` (case-insensitive), else ``None``: ``resnet18...`` and
    every other name keep the seeded :class:`ResNet18`."""
    import os
    name = os.path.basename(str(model_path)).lower()
    for depth in (152, 101, 50, 34):
        if name.startswith(f"resnet{depth}"):
            return depth
    return None


def _is_state_dict_file(model_path: str) -> bool:
    import os
    return bool(model_path) and os.path.isfile(str(model_path))


def _resnet_spec_of(sd: Dict[str, torch.Tensor]):
    """(block kind, blocks per stage, classes) of a torchvision-family state dict; every refusal is a ``ValueError`` that names the
    key and the shape found."""
    import re

    def shape(k):
        if k not in sd:
            raise ValueError(f"build_resnet: the state dict has no {k!r}: not a ResNet of the torchvision family")
        return tuple(sd[k].shape)

    if shape("conv1.weight") != (64, 3, 7, 7):
        raise ValueError(f"build_resnet: conv1.weight is {shape('conv1.weight')}: only the 7x7 / 64 stem [64, 3, 7, 7] is supported")
    bott = "layer1.0.conv3.weight" in sd
    exp = 4 if bott else 1
    counts = [0, 0, 0, 0]
    for k in sd:
        m = re.match(r"layer(\d+)\.(\d+)\.", k)
        if m:
            s, j = int(m.group(1)), int(m.group(2))
            if not 1 <= s <= 4:
                raise ValueError(f"build_resnet: {k!r}: a ResNet of this family has layer1 .. layer4")
            counts[s - 1] = max(counts[s - 1], j + 1)
    if not all(1 <= n <= 64 for n in counts):
        raise ValueError(f"build_resnet: blocks per stage {tuple(counts)}: each stage needs 1..64 blocks")
    cin = 64
    for s, n in enumerate(counts):
        width = RESNET_WIDTHS[s]
        for j in range(n):
            pre = f"layer{s + 1}.{j}."
            k1, k2 = pre + "conv1.weight", pre + "conv2.weight"
            want1 = (width, cin, 1, 1) if bott else (width, cin, 3, 3)
            if shape(k2)[1] != shape(k2)[0]:
                raise ValueError(f"build_resnet: {k2} is {shape(k2)}: grouped convolutions (ResNeXt) are not supported")
            if shape(k1) != want1:
                what = "bottleneck widths other than 64 * 2^s (wide ResNets) are not supported" if bott and shape(k1)[1:] == want1[1:] \
                    else f"expected {want1}"
                raise ValueError(f"build_resnet: {k1} is {shape(k1)}: {what}")
            if shape(k2) != (width, width, 3, 3):
                raise ValueError(f"build_resnet: {k2} is {shape(k2)}: expected {(width, width, 3, 3)}")
            cout = width * exp
            if bott and shape(pre + "conv3.weight") != (cout, width, 1, 1):
                raise ValueError(f"build_resnet: {pre}conv3.weight is {shape(pre + 'conv3.weight')}: expected {(cout, width, 1, 1)}")
            stride = 2 if (j == 0 and s > 0) else 1
            kd = pre + "downsample.0.weight"
            if (stride != 1 or cin != cout) and shape(kd) != (cout, cin, 1, 1):
                raise ValueError(f"build_resnet: {kd} is {shape(kd)}: expected {(cout, cin, 1, 1)}")
            cin = cout
    fc = shape("fc.weight")
    if len(fc) != 2 or fc[1] != cin:
        raise ValueError(f"build_resnet: fc.weight is {fc}: expected [classes, {cin}]")
    for k in list(sd):
        if k.endswith(".weight") and sd[k].dim() == 1:                              # a BatchNorm's weight
            for stat in ("running_mean", "running_var"):
                ks = k[:-len("weight")] + stat
                if ks not in sd:
                    raise ValueError(f"build_resnet: {k} of shape {tuple(sd[k].shape)} has no {ks}: the BatchNorm statistics are "
                                     "missing (a plan folds them into the convolution)")
    return ("bottleneck" if bott else "basic"), tuple(counts), int(fc[0])


def load_resnet_state_dict(path: str) -> Dict[str, torch.Tensor]:
    """The state dict of a local file (``weights_only=True``: never unpickles code), a ``module.`` / ``model.`` prefix stripped."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f"build_resnet: {path} does not hold a state dict of tensors")
    for prefix in ("module.", "model."):
        if sd and all(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items()}
    return sd


def build_resnet(depth: Optional[int] = None, seed: int = 2, weights: Optional[str] = None,
                 num_classes: Optional[int] = None) -> ResNet:
    """A :class:`ResNet`: the local state dict ``weights`` when that file exists (block kind from ``layer1.0.conv3.weight``, blocks
    per stage from the ``layer{s}.{j}`` indices, class count from ``fc.weight``; nothing is ever fetched by name), else the seeded
    random-init network of ``depth`` (18 / 34 / 50 / 101 / 152; BatchNorm statistics randomised so that the folded convolutions
    are not trivial).  ``num_classes=None``: the file's class count, 1000 without a file; a count the file contradicts is a
    ``ValueError``, like every architecture outside the family (ResNeXt, wide ResNets, another stem, no BatchNorm statistics)."""
    sd = None
    if weights and _is_state_dict_file(weights):
        sd = load_resnet_state_dict(weights)
        block, blocks, classes = _resnet_spec_of(sd)
        if num_classes is not None and int(num_classes) != classes:
            raise ValueError(f"build_resnet: fc.weight is {tuple(sd['fc.weight'].shape)}: the file has {classes} classes, "
                             f"resnet_num_classes says {int(num_classes)}")
    else:
        if depth not in RESNET_DEPTHS:
            raise ValueError(f"build_resnet: depth must be one of {sorted(RESNET_DEPTHS)}, got {depth!r}")
        block, blocks = RESNET_DEPTHS[depth]
        classes = 1000 if num_classes is None else int(num_classes)
    g = torch.Generator().manual_seed(seed)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        net = ResNet(block, blocks, classes)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.weight.data.copy_(torch.rand(m.num_features, generator=g) * 0.5 + 0.75)
                m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    finally:
        torch.random.set_rng_state(state)
    if sd is not None:
        missing, unexpected = net.load_state_dict(sd, strict=False)
        missing = [k for k in missing if not k.endswith("num_batches_tracked")]
        if missing or unexpected:
            raise ValueError(f"build_resnet: the state dict does not match its own architecture (missing {missing[:3]}, "
                             f"unexpected {list(unexpected)[:3]})")
    return net.eval()


@dataclass
class _ResTick:
    """What ``stage_pre`` hands to ``stage_net`` / ``stage_post`` for one tick of one frame group."""
    rows: int                                   # streams of the group (batch rows of the PostBuffers)
    wh: Tuple[int, int]                         # (width, height) of the group's frames: the full-frame box
    slot: int                                   # pipeline slot (tick parity) whose buffers this tick uses
    x: torch.Tensor                             # [rows, 3, H, W] fp32 (fp16 on "resnet-f16"): a view of the slot's input buffer


class _ResSlot:
    """One tick slot's input buffer (K1 writes it, the network reads it) and, on the plan engine, its plan with two logits
    sets used in turn: the tail of the previous tick that used this slot may still read the other set (temporal._PlanSlot)."""

    def __init__(self, cap: int, hw, device, plan: Optional[FusedResNet18], dtype: torch.dtype = torch.float32):
        self.cap, self.plan, self.turn = cap, plan, 0
        self.input = torch.empty((cap, 3, *hw), dtype=dtype, device=device)
        self.iota = torch.arange(cap, dtype=torch.int32, device=device)
        self.logits = [torch.empty((cap, plan.classes), dtype=torch.float32, device=device) for _ in range(2)] if plan else []


class HipResNetDetector(BaseDetector):
    """``predict(packet)`` / ``predict_batch(packets)`` with the reference's top-K rule (detector.py:945-977), and the batched
    device path of the tick pipeline (``stage_pre`` / ``stage_net`` / ``stage_post``: K1 into the tick slot's input buffer, the
    network, the top-K as device result rows -- no host synchronisation).  ``engine``: ``"infer_fn"`` (a caller's function
    overrides everything), ``"resnet-f32"`` (``hip_engine: plan``: the network and the device path's top-K run as the
    hand-written fp32 plan, resnet_plan.FusedResNet18), ``"resnet-f16"`` (below) or ``"torch"`` (PyTorch-ROCm).  Without the
    detector key ``hip_resnet_fp16`` ``half`` has no effect on this head -- it runs float32 like the reference's pre-process --
    and ``hip_engine: native`` is refused.  ``hip_resnet_fp16: true`` with ``half: true`` and ``hip_engine: plan`` or ``native``
    opts into the fp16 MFMA plan (engine ``"resnet-f16"``, resnet_plan.FusedResNet18F16: K1 writes fp16 frames, fp16 weights and
    stored activations, fp32 sums and logits); the key changes nothing else."""

    def __init__(self, config: DetectorConfig, net: Optional[nn.Module] = None, infer_fn=None, seed: int = 2,
                 device: Optional[int] = None):
        super().__init__(config)
        self.ctx = ops.context(device)
        self.device = torch.device("cuda", self.ctx.device)
        self.input_hw = (int(config.input_size[0]), int(config.input_size[1])) if config.input_size else (224, 224)
        self._infer_fn = infer_fn
        hip_engine = getattr(config, "hip_engine", "auto")
        fp16 = hip_engine in ("plan", "native") and bool(config.half) and bool(getattr(config, "hip_resnet_fp16", False))
        if infer_fn is None and hip_engine == "native" and not fp16:
            raise ValueError("hip_engine: native has no hand-written plan for model_type 'resnet' (the network runs through "
                             "PyTorch-ROCm with hip_engine: auto; half: true with hip_resnet_fp16: true runs the fp16 plan "
                             "resnet-f16)")
        self.engine = "infer_fn" if infer_fn is not None else \
            RESNET_PLAN_F16 if fp16 else (RESNET_PLAN if hip_engine == "plan" else "torch")
        self._planned = self.engine in (RESNET_PLAN, RESNET_PLAN_F16)         # the network and the top-K run as a plan
        self._in_dtype = torch.float16 if self.engine == RESNET_PLAN_F16 else torch.float32     # what K1 writes
        self.net = None
        if infer_fn is None:
            if net is None and _is_state_dict_file(config.model_path):
                net = build_resnet(seed=seed, weights=config.model_path, num_classes=config.resnet_num_classes)   # what the file says
            elif net is None and resnet_depth_from_path(config.model_path) is not None:
                net = build_resnet(resnet_depth_from_path(config.model_path), seed=seed, num_classes=config.resnet_num_classes)
            elif net is None:
                st = torch.random.get_rng_state()
                torch.manual_seed(seed)
                net = ResNet18(config.resnet_num_classes)
                torch.random.set_rng_state(st)
            if isinstance(net, ResNet) and self.engine == RESNET_PLAN:
                raise ValueError("hip_engine: plan runs a classify.ResNet as the fp16 plan resnet-f16 only: the fp32 plan resnet-f32 "
                                 "exists for classify.ResNet18 only; set half: true with hip_resnet_fp16: true, or hip_engine: auto "
                                 "for the PyTorch-ROCm fp32 network")
            self.net = net.eval().float().to(self.device).to(memory_format=torch.channels_last)
        # batched device path
        self.two_chain_ok = True               # every buffer of a tick exists per slot: consecutive ticks may run as two chains
        self._streams = 0                      # streams the pipeline announced (reserve_streams): the slots' capacity
        self._slots: Dict[int, _ResSlot] = {}
        self._post: Dict[tuple, ops.PostBuffers] = {}
        self._tables: Dict[tuple, torch.Tensor] = {}      # (rows, w, h) -> device row table / box rows, uploaded once
        self._host_plan: Optional[FusedResNet18] = None   # plan of predict / predict_batch

    def _preprocess(self, frames: Sequence, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        dev = []
        for f in frames:
            if isinstance(f, ops.Nv12Surface):
                dev.append(f)
            else:
                t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
                dev.append(t.to(self.device).contiguous())
        if out is None:
            out = torch.empty((len(dev), 3, *self.input_hw), dtype=self._in_dtype, device=self.device)
        for b0 in range(0, len(dev), N.RVA_MAX_BATCH):
            ops.preprocess_frames(dev[b0:b0 + N.RVA_MAX_BATCH], self.input_hw, N.NORM_IMAGENET_F32, N.LAYOUT_NCHW, self._in_dtype,
                                  out=out[b0:b0 + N.RVA_MAX_BATCH], ctx=self.ctx)
        return out

    def _make_plan(self, max_frames: int) -> FusedResNet18:
        if isinstance(self.net, ResNet):                  # any depth: the fp16 plan only (refused at construction otherwise)
            return FusedResNetF16(self.net, self.input_hw, max_frames, self.config.resnet_top_k, ctx=self.ctx, device=self.device)
        cls = FusedResNet18F16 if self.engine == RESNET_PLAN_F16 else FusedResNet18
        return cls(self.net, self.input_hw, max_frames, self.config.resnet_top_k, ctx=self.ctx, device=self.device)

    def _network(self, x: torch.Tensor) -> torch.Tensor:
        """``[B, 3, H, W]`` -> raw ``[B, classes]`` on this detector's engine (the host path: a fresh tensor)."""
        if self._planned:
            if self._host_plan is None or self._host_plan.max_clips < x.shape[0]:
                self._host_plan = self._make_plan(int(x.shape[0]))
            return self._host_plan(x)
        return self._infer_fn(x) if self._infer_fn is not None else self.net(x)

    def predict_batch(self, packets: Sequence[FramePacket]) -> List[List[Detection]]:
        groups = {}
        for i, p in enumerate(packets):
            groups.setdefault(self.geometry_key(p.frame), []).append(i)
        out: List[Optional[List[Detection]]] = [None] * len(packets)
        for (w, h, _), idxs in groups.items():
            with torch.inference_mode():
                raw = self._network(self._preprocess([packets[i].frame for i in idxs]))
            scores = raw.float().cpu().numpy()
            for row, i in enumerate(idxs):
                p, o = packets[i], scores[row].flatten()
                order = np.argsort(o, kind="stable")[-self.config.resnet_top_k:][::-1]      # detector.py:956
                out[i] = [Detection(stream_name=p.stream.name, frame_id=p.frame_id, class_id=int(c), confidence=float(o[c]),
                                    bbox_xyxy=(0.0, 0.0, float(w), float(h)))
                          for c in order if o[c] >= self.config.confidence_threshold]
        return out  # type: ignore[return-value]

    def predict(self, packet: FramePacket) -> List[Detection]:
        return self.predict_batch([packet])[0]

    # -- batched device path: a whole tick of this head without a host round trip ----------------------------------------
    geometry_key = staticmethod(ops.geometry_key)

    def reserve_streams(self, names: Sequence[str]) -> None:
        """The most frames a tick can bring (TickPipeline calls this once): the slots are sized for it and never regrown."""
        self._streams = max(self._streams, len(names))

    def _tick_slot(self, slot: int, rows: int) -> _ResSlot:
        """The buffers (and plan) of a tick slot; rebuilt, after a device drain, only for more frames than were announced."""
        rs = self._slots.get(slot)
        if rs is None or rs.cap < rows:
            if rs is not None:
                torch.cuda.synchronize(self.device)          # the old buffers may still be read by a tick in flight
            cap = max(rows, self._streams, 1)
            rs = self._slots[slot] = _ResSlot(cap, self.input_hw, self.device, self._make_plan(cap) if self._planned else None,
                                              self._in_dtype)
        return rs

    def stage_pre(self, packets: Sequence[FramePacket], slot: int = 0) -> _ResTick:
        """K1 of the tick: the group's frames (one geometry) pre-processed into the input buffer of ``slot`` (the tick's parity)."""
        rs = self._tick_slot(slot, len(packets))
        x = self._preprocess([p.frame for p in packets], out=rs.input[:len(packets)])
        w, h, _ = self.geometry_key(packets[0].frame)
        return _ResTick(len(packets), (w, h), slot, x)

    def stage_net(self, pre: _ResTick) -> torch.Tensor:
        """The group's frames as ONE network batch: ``[rows, classes]`` raw outputs (no softmax)."""
        if self._planned:
            rs = self._slots[pre.slot]
            logits = rs.logits[rs.turn]
            rs.turn ^= 1
            return rs.plan.run(rs.input, rs.iota, pre.rows, out=logits)
        with torch.inference_mode():
            return (self._infer_fn(pre.x) if self._infer_fn is not None else self.net(pre.x)).float()

    def stage_post(self, raw: torch.Tensor, pre: _ResTick) -> ops.PostBuffers:
        """Top-K of the raw output per frame in the reference's order (ascending stable sort, last K reversed: detector.py:956),
        full-frame boxes; the ``>= confidence_threshold`` test is the tracker kernel's filter (same float64 comparison)."""
        k = min(int(self.config.resnet_top_k), int(raw.shape[1]))
        key = (pre.rows, pre.slot)
        post = self._post.get(key)
        if post is None:
            post = self._post[key] = ops.PostBuffers.allocate(pre.rows, max(8, k), self.device)
        plan = self._planned
        tkey = (pre.rows, *pre.wh, plan)
        tab = self._tables.get(tkey)
        if tab is None:                        # every row has a frame: the table is constant per (rows, w, h)
            w, h = pre.wh
            tab = self._tables[tkey] = torch.tensor([[r, w, h] for r in range(pre.rows)], dtype=torch.int32, device=self.device) \
                if plan else torch.tensor([0.0, 0.0, float(w), float(h)], device=self.device)
        if plan:
            return self._slots[pre.slot].plan.post(raw, tab, pre.rows, post)
        order = torch.sort(raw, dim=1, stable=True).indices[:, -k:].flip(1)                # [rows, k]
        post.scores[:, :k] = torch.gather(raw, 1, order)
        post.cls[:, :k] = order.to(torch.int32)
        post.boxes[:, :k] = tab
        post.counts.fill_(k)
        return post

    def predict_batch_device(self, packets: Sequence[FramePacket]) -> ops.PostBuffers:
        pre = self.stage_pre(packets)
        return self.stage_post(self.stage_net(pre), pre)
