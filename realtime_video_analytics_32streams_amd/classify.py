"""ResNet classification head behind the detector API (reference detector.py:870-1001).

The reference loads a ResNet from an OpenVINO / ONNX file and returns the top-K classes of the RAW output vector as
full-frame ``Detection`` objects (no softmax; ``np.argsort(output)[-k:][::-1]``, kept when ``>= confidence_threshold``).
Pre-process = the float32 ImageNet normalisation of the clip kernel on one frame (``rva_preprocess_frames_*``).  The
network here is a from-scratch torch ResNet-18 with seeded weights (no model files exist offline); any module or
``infer_fn`` mapping ``[B,3,H,W] -> [B,num_classes]`` can replace it.
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
from .resnet_plan import ENGINE as RESNET_PLAN, ENGINE_F16 as RESNET_PLAN_F16, FusedResNet18, FusedResNet18F16
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
            if net is None:
                st = torch.random.get_rng_state()
                torch.manual_seed(seed)
                net = ResNet18(config.resnet_num_classes)
                torch.random.set_rng_state(st)
            self.net = net.eval().float().to(self.device).to(memory_format=torch.channels_last)
        # batched device path
        self._slot = 0                         # set by PipelinedTicks: tick parity -> which buffers a tick uses
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
    @staticmethod
    def geometry_key(frame) -> tuple:
        if isinstance(frame, ops.Nv12Surface):
            return (int(frame.width), int(frame.height), "nv12")
        return (int(frame.shape[1]), int(frame.shape[0]), "bgr")

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

    def stage_pre(self, packets: Sequence[FramePacket]) -> _ResTick:
        """K1 of the tick: the group's frames (one geometry) pre-processed into the slot's input buffer."""
        rs = self._tick_slot(self._slot, len(packets))
        x = self._preprocess([p.frame for p in packets], out=rs.input[:len(packets)])
        w, h, _ = self.geometry_key(packets[0].frame)
        return _ResTick(len(packets), (w, h), self._slot, x)

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
