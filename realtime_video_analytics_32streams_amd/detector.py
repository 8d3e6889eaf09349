"""Detector plugin API of the reference (detector.py:32-103) with the MI355X backend behind it.

Same names, argument meaning and error behaviour as the reference:
  * ``Detection`` -- slots dataclass of Python scalars + a 4-tuple (detector.py:32-40);
  * ``BaseDetector(config).predict(packet) -> List[Detection]`` (detector.py:43-51);
  * ``create_detector(config)`` -- dispatch on ``model_type`` / ``backend`` (detector.py:54-96), with
    backend ``"hip"`` added; reference-only backends raise the same kind of ``RuntimeError`` the
    reference raises when a runtime is missing (detector.py:496-502);
  * ``filter_detections`` (detector.py:99-103).
``HipYoloDetector`` adds ``predict_batch(packets)``: the cross-stream batching the reference's
docstring promises but never implements.

The score rule is the reference's, including its YOLOv8 class-shift quirk: for
an 84-column head column 4 multiplies columns 5.., so ``class_id = true_class - 1``.
"""
from __future__ import annotations

import abc
import logging
from dataclasses import dataclass
from typing import Iterable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import ops
from .config import HIP_BACKENDS, TEMPORAL_MODELS, DetectorConfig
from .video_stream import FramePacket
from .yolov8 import build_detector_net, variant_from_path

LOGGER = logging.getLogger(__name__)


@dataclass(slots=True)
class Detection:
    """Single detection result from a model inference."""

    stream_name: str
    frame_id: int
    class_id: int
    confidence: float
    bbox_xyxy: tuple[float, float, float, float]


class BaseDetector(abc.ABC):
    """Abstract detector interface."""

    def __init__(self, config: DetectorConfig):
        self.config = config

    @abc.abstractmethod
    def predict(self, packet: FramePacket) -> List[Detection]:
        raise NotImplementedError


def filter_detections(detections: Iterable[Detection], min_confidence: float) -> List[Detection]:
    """Drop low confidence detections (second, float64 comparison: pipeline.py:182)."""
    return [d for d in detections if d.confidence >= min_confidence]


def create_detector(config: DetectorConfig) -> BaseDetector:
    """Instantiate a detector backend based on configuration."""
    backend = config.backend.lower()
    model_type = config.model_type.lower()
    if backend in HIP_BACKENDS:
        if model_type in TEMPORAL_MODELS:
            from .temporal import HipCNN3DDetector, HipCNNLSTMDetector, HipConvGRUDetector
            if model_type == "cnn_lstm":
                return HipCNNLSTMDetector(config)
            if model_type == "conv_gru":
                return HipConvGRUDetector(config)
            return HipCNN3DDetector(config)       # "3d_cnn", and "slow_fast" as in the reference (detector.py:70-74)
        if model_type == "resnet":
            from .classify import HipResNetDetector
            return HipResNetDetector(config)
        if model_type in ("yolov5", "yolov8"):
            return HipYoloDetector(config)
        raise ValueError(f"Model type '{model_type}' not supported with backend '{config.backend}'")
    if backend in ("ultralytics", "tensorrt", "onnx", "onnxruntime", "openvino", "rknn", "rk3588"):
        raise RuntimeError(
            f"Detector backend '{config.backend}' belongs to the reference implementation and its runtime is not "
            "part of this library. Select backend 'hip' to run on MI355X.")
    raise ValueError(f"Unsupported detector backend '{config.backend}'")


def detector_architecture(model_type: str, model_path: str, net=None, state_dict=None) -> str:
    """``"yolo11"``, ``"yolov5"`` or ``"yolov8"``: which network ``HipYoloDetector`` builds.  No configuration key: it follows what
    the user handed over.  YOLO11, checked first and under either ``model_type``, when (1) ``net`` is a ``yolo11.Yolo11``; or (2)
    ``model_path`` is an existing file whose state dict has the attention convolution of C2PSA (``model.10.m.0.attn.qkv.conv.weight`` /
    ``10.m.0...`` / ``l10.m.0...``): the file decides, whatever its name; or (3) no such file exists and the file name starts with
    ``yolo11`` / ``yolov11`` plus a scale letter (seeded weights).  YOLOv5 when (1) ``net`` is a ``yolov5.YoloV5``; or (2) ``model_path`` is an existing file whose state dict
    (``state_dict`` where the caller has loaded it already) has the YOLOv5 detect convolution (``model.24.m.0.weight`` /
    ``24.m.0.weight`` / ``detect.m.0.weight``); or (3) ``model_type`` is ``"yolov5"`` and the file name starts with ``yolov5`` plus
    a scale letter while no such file exists (seeded weights).  Everything else is YOLOv8 as before: ``model_type: yolov5`` with
    the default ``yolov8n.pt``, every ``yolov8*`` name, and the ``yolov5*u`` names (anchor-free re-exports with the v8 head)."""
    from .yolo11 import Yolo11, is_11_state_dict, variant_from_path_11
    from .yolov5 import YoloV5, is_v5_state_dict, variant_from_path_v5
    if net is not None:
        return "yolo11" if isinstance(net, Yolo11) else "yolov5" if isinstance(net, YoloV5) else "yolov8"
    if _is_file(model_path):
        if state_dict is None:
            state_dict = torch.load(model_path, map_location="cpu", weights_only=True)
        return "yolo11" if is_11_state_dict(state_dict) else "yolov5" if is_v5_state_dict(state_dict) else "yolov8"
    if variant_from_path_11(model_path) is not None:
        return "yolo11"
    if str(model_type).lower() == "yolov5" and variant_from_path_v5(model_path) is not None:
        return "yolov5"
    return "yolov8"


def v5_scale_of(model_path: str, state_dict=None) -> str:
    """Scale letter of a YOLOv5 model: from the stem width of its state dict (16 n, 32 s, 48 m, 64 l, 80 x), else from the file
    name, else ``"n"``."""
    from .yolov5 import variant_from_path_v5
    for key in ("b0.conv.weight", "model.0.conv.weight", "0.conv.weight") if state_dict is not None else ():
        w = state_dict.get(key)
        if w is not None:
            s = {16: "n", 32: "s", 48: "m", 64: "l", 80: "x"}.get(int(w.shape[0]))
            if s:
                return s
    return variant_from_path_v5(model_path) or "n"


def select_yolo_engine(arch: str, half: bool, hip_engine: str = "auto") -> str:
    """Engine of a ``HipYoloDetector``: ``"fused"`` (fp16 plan) for ``half: true``; for ``half: false`` the fp32 plan
    (``"fused-f32"``) under ``hip_engine: plan / native`` and the module through PyTorch-ROCm (``"torch-fp32"``) under ``auto``.
    YOLOv5 and YOLO11 have no fp32 plan: ``half: false`` with ``plan`` / ``native`` is a ``ValueError``."""
    if half:
        return "fused"
    if hip_engine in ("plan", "native"):
        if arch in ("yolov5", "yolo11"):
            name = "YOLOv5" if arch == "yolov5" else "YOLO11"
            raise ValueError(f"hip_engine: {hip_engine} with half: false needs an fp32 {name} plan, which does not exist; the "
                             f"hand-written {name} plan is fp16: set `half: true` (or `hip_engine: auto` for fp32 through PyTorch-ROCm)")
        return "fused-f32"
    return "torch-fp32"


class _YoloTick(NamedTuple):
    """What ``HipYoloDetector.stage_pre`` hands to ``stage_net`` / ``stage_post`` for one tick of one frame group."""
    tensor: torch.Tensor                        # [n, 3, H, W]: the slot's input buffer, or its leading n images
    meta: N.Letterbox
    slot: int                                   # pipeline slot (tick parity) whose input buffer and plan this tick uses


@dataclass
class _InputState:
    """What K1 last left in one input buffer of a ``HipYoloDetector``."""
    border: tuple                               # (frame geometry, leading images) whose letterbox border the buffer holds
    rows: tuple                                 # content rows (top, bottom): the plan may skip the others (FusedYoloV8.set_static_rows)
    told: bool                                  # the slot's plan already runs with these rows


class HipYoloDetector(BaseDetector):
    """YOLO detector on MI355X: K1 pre-process -> PyTorch-ROCm network -> K2/K3 post-process.

    One object serves many streams (pipeline.py:472-489).  ``predict`` is the batch-of-one shim of the
    reference API; ``predict_batch`` runs a whole tick in three launches + the network.
    ``infer_fn`` may replace the network (``tensor[B,3,H,W] -> raw[B,d1,d2]``): used by the parity
    tests to feed recorded head tensors, like the reference's ``_infer`` stub point (detector.py:377-379).
    """

    def __init__(self, config: DetectorConfig, infer_fn=None, net: Optional[torch.nn.Module] = None,
                 seed: int = 0, device: Optional[int] = None):
        """``half: true`` (every BASELINE configuration) runs the network as the librva plan: hand-written MFMA kernels, one
        launch per layer, fp16 operands with fp32 accumulation.  ``half: false`` is the reference's fp32 precision
        (detector.py:248-251): by default (``hip_engine: auto``) the module then runs through PyTorch-ROCm (MIOpen) and the
        constructor says so in the log -- a configuration never changes engines silently; ``hip_engine: plan`` runs it as the
        hand-written fp32 plan instead (engine ``"fused-f32"``: exact fp32 MFMA, bit-reproducible, same pipeline integration);
        ``hip_engine: native`` (the strict form, config.py) selects the same engines as ``plan`` here.
        ``hip_box_rows: fp32`` (engine ``"fused"`` only) makes the plan keep the four box rows in fp32 beside its fp16 head
        (``engine.FusedYoloV8(box_rows="fp32")``); the side tensor travels from ``stage_net`` to ``stage_post`` as an
        ``ops.SplitHead`` and K2 reads its boxes from it.
        The architecture (``self.arch``) is YOLOv5 where ``detector_architecture`` says so -- a ``yolov5.YoloV5`` as ``net``, a YOLOv5
        state dict at ``model_path``, or ``model_type: yolov5`` with a ``yolov5<n|s|m|l>`` file name and no file -- and then ``half:
        true`` runs ``engine.FusedYoloV5`` (engine ``"fused"``, head ``[B, 5+nc, A]``), ``half: false`` the module through PyTorch-ROCm
        (``plan`` / ``native``: ``ValueError``, there is no fp32 YOLOv5 plan).  YOLO11 -- a ``yolo11.Yolo11`` as ``net``, a YOLO11 state
        dict at ``model_path``, or a ``yolo11<n|s|m|l>`` file name and no file, under either ``model_type`` -- runs the same way on
        ``engine.FusedYolo11`` (head ``[B, 4+nc, A]``, as YOLOv8's).
        ``hip_plan_capacity: N`` (engines ``"fused"`` and ``"fused-f32"``; default 0 = one plan and input buffer per batch size)
        keeps ONE plan and ONE input buffer of ``N`` images per input size and slot: a call with ``n <= N`` frames writes and
        runs the leading ``n`` images, with the kernels of a full run (config.py)."""
        super().__init__(config)
        self._plans = {}
        self.ctx = ops.context(device)            # raises RuntimeError when no HIP device (no CPU fallback)
        self.device = torch.device("cuda", self.ctx.device)
        if config.input_size:
            self.input_hw = (int(config.input_size[0]), int(config.input_size[1]))
        else:
            self.input_hw = (640, 640)            # detector.py:582-583 default
        self.half = bool(config.half)
        # the architecture follows what the user handed over (detector_architecture); behind an infer_fn there is no network
        sd = None
        if infer_fn is None and net is None and _is_file(config.model_path):
            sd = torch.load(config.model_path, map_location="cpu", weights_only=True)
        self.arch = "yolov8" if infer_fn is not None else detector_architecture(config.model_type, config.model_path, net, sd)
        self.engine = select_yolo_engine(self.arch, self.half, getattr(config, "hip_engine", "auto"))
        self._infer_fn = infer_fn
        # where the fp16 plan keeps its box rows; fp32 elsewhere already (half: false), and no plan behind an infer_fn
        self.box_rows = getattr(config, "hip_box_rows", "fp16") if (self.engine == "fused" and infer_fn is None) else "fp16"
        # one plan of this many images serves every smaller batch (0: a plan per batch size); plans only
        cap = int(getattr(config, "hip_plan_capacity", 0) or 0)
        self.plan_capacity = cap if (infer_fn is None and self.engine in ("fused", "fused-f32")) else 0
        self._over_capacity_warned = False
        self.net = None
        if infer_fn is None:
            if net is None and self.arch == "yolo11":
                from .yolo11 import build_detector_net_11, scale_of_11
                scale = scale_of_11(config.model_path, sd)
                net = build_detector_net_11(scale, seed=seed, weights=config.model_path)
                LOGGER.info("hip detector: YOLO11%s, %s weights", scale,
                            "local state-dict" if sd is not None else "seeded random (no weights offline)")
            elif net is None and self.arch == "yolov5":
                from .yolov5 import build_detector_net_v5
                scale = v5_scale_of(config.model_path, sd)
                net = build_detector_net_v5(scale, seed=seed, weights=config.model_path)
                LOGGER.info("hip detector: YOLOv5%s, %s weights", scale,
                            "local state-dict" if sd is not None else "seeded random (no weights offline)")
            elif net is None:
                scale = variant_from_path(config.model_path)
                net = build_detector_net(scale, seed=seed, weights=config.model_path)
                LOGGER.info("hip detector: YOLOv8%s, %s weights", scale,
                            "local state-dict" if _is_file(config.model_path) else "seeded random (no weights offline)")
            if self.engine == "torch-fp32":
                LOGGER.warning("hip detector: half=false -> fp32 network through PyTorch-ROCm (MIOpen); the hand-written fp16 "
                               "MFMA plan runs with `half: true`")
            net = net.fuse().to(self.device)
            net = net.half() if self.half else net.float()
            self.net = net.to(memory_format=torch.channels_last)
        # buffers are cached per shape and never reallocated: captured hipGraphs (pipeline.PipelinedTicks) keep raw
        # pointers to them, and an interleaved predict() with another batch size must not free what a graph replays on
        self._post_bufs: dict = {}
        self._in_bufs: dict = {}                          # buffer key (_buf_key: images[, slot]) -> the input tensor K1 writes
        self._in_state: dict = {}                         # buffer key -> _InputState, once K1 has written the buffer
        self._post: Optional[ops.PostBuffers] = None      # result buffers of the latest call
        self._in: Optional[torch.Tensor] = None           # input tensor of the latest call
        self.tune_overlap = 1                             # launches the tuner of a new plan times at once (PipelinedTicks: its chains)
        if config.warmup and self.net is not None:  # detector.py:588-593
            with torch.inference_mode():
                self._infer(torch.zeros((1, 3, *self.input_hw), device=self.device,
                                        dtype=torch.float16 if self.half else torch.float32))

    # -- stages ---------------------------------------------------------------------------------
    def _images(self, batch: int) -> int:
        """Images of the input buffer and of the plan that serve a group of ``batch`` frames: the batch itself, or with
        ``hip_plan_capacity: N`` the capacity, for every group it holds (a larger one gets its exact size, and a warning)."""
        cap = self.plan_capacity
        if cap <= 0 or batch == cap:
            return batch
        if batch > cap:
            if not self._over_capacity_warned:
                self._over_capacity_warned = True
                LOGGER.warning("hip detector: a group of %d frames exceeds hip_plan_capacity=%d: it gets a plan of its own size, "
                               "built now", batch, cap)
            return batch
        return cap

    def _buf_key(self, batch: int, slot: int = 0):
        """Key of the input buffer (and of its border / static-rows state): images of the buffer (, slot)."""
        m = self._images(batch)
        return m if slot == 0 else (m, slot)

    def input_tensor(self, batch: int, slot: int = 0) -> torch.Tensor:
        """The input tensor K1 writes for this batch size and slot (cached for the life of the detector); with
        ``hip_plan_capacity`` the leading ``batch`` images of the slot's one buffer."""
        n, m = self._buf_key(batch, slot), self._images(batch)
        t = self._in_bufs.get(n)
        if t is None:
            dt = torch.float16 if self.half else torch.float32
            t = self._in_bufs[n] = torch.empty((m, 3, *self.input_hw), dtype=dt, device=self.device)
        return t if m == batch else t[:batch]

    def _preprocess(self, frames: Sequence, slot: int = 0) -> tuple[torch.Tensor, N.Letterbox]:
        n = self._buf_key(len(frames), slot)
        self._in = self.input_tensor(len(frames), slot)
        f0 = frames[0]
        if isinstance(f0, ops.Nv12Surface):
            # the border (pad value) of the input tensor is constant per geometry: the first launch into a buffer writes it,
            # the following ticks of the same geometry write the content rows only
            key = (f0.width, f0.height) if not any(f.mask is not None for f in frames) else None
            have, bordered = self._in_state[n].border if n in self._in_state else (None, 0)
            # steady: the border of this geometry is in place in every image the tick writes (a capacity buffer serves ticks of
            # several sizes: a tick larger than any before it is not steady)
            steady = key is not None and have == key and len(frames) <= bordered
            res = ops.preprocess_nv12(frames, self.input_hw, self.half, out=self._in, ctx=self.ctx, content_only=steady)
            if not steady:                                # new buffer, new geometry, more images or ROI masks: the border was (re)written
                lb = res[1]
                self._note_written(n, (key, len(frames)),
                                   (int(lb.pad_top), int(lb.pad_top) + int(lb.new_h)) if key is not None else (0, self.input_hw[0]))
            return res
        dev = []
        for f in frames:  # host BGR ndarray (the reference's FramePacket.frame) or device tensor
            t = torch.from_numpy(np.ascontiguousarray(f)) if isinstance(f, np.ndarray) else f
            dev.append(t.to(self.device, non_blocking=True).contiguous())
        self._note_written(n, (None, 0), (0, self.input_hw[0]))        # K1 for host frames writes the whole tensor
        return ops.preprocess_bgr(dev, self.input_hw, self.half, out=self._in, ctx=self.ctx)

    def _note_written(self, n, border, rows) -> None:
        """K1 has just written a whole input buffer whose rows outside ``rows`` will stay as they are on the steady ticks that
        follow: the slot's plan hears of it before its next run (``_infer``), which then covers all rows once."""
        self._in_state[n] = _InputState(border, (max(rows[0], 0), min(rows[1], self.input_hw[0])), told=False)

    def invalidate_engine(self) -> None:
        """Drop cached fused plans (call after editing ``self.net``'s weights)."""
        self._plans.clear()
        for st in self._in_state.values():                # nothing is pending: a new plan is built with the rows (plan_for)
            st.told = True

    def plan_for(self, tensor: torch.Tensor, slot: int = 0):
        """The fused plan of this batch shape and slot (built and autotuned on first use; a later slot's plan takes over the
        first one's kernel selection instead of tuning again).  With ``hip_plan_capacity`` the one plan of that many images,
        told how many of them ``tensor`` holds (``FusedYoloV8.n``: what its ``result()`` hands out)."""
        batch = int(tensor.shape[0])
        shape = (self._images(batch), int(tensor.shape[2]), int(tensor.shape[3]))
        key = shape if slot == 0 else shape + (slot,)
        plan = self._plans.get(key)
        if plan is None:
            from .engine import FusedYolo11, FusedYoloV5, FusedYoloV8
            plan_cls = {"yolov5": FusedYoloV5, "yolo11": FusedYolo11}.get(self.arch, FusedYoloV8)      # the same plan object and surface
            first = self._plans.get(shape) if slot else None
            # the static rows at construction: the tuner times the windowed launches, and a later slot's plan has the first
            # slot's windows, whose kernel selection it takes over
            st = self._in_state.get(self._buf_key(batch, slot))
            rows = first.static_rows if first is not None else (st.rows if st is not None else None)
            plan = self._plans[key] = plan_cls(self.net, shape[0], shape[1:], device=self.device, ctx=self.ctx,
                                               autotune=first is None, tune_overlap=self.tune_overlap,
                                               precision="fp32" if self.engine == "fused-f32" else "fp16", box_rows=self.box_rows,
                                               static_rows=rows if self.engine == "fused" else None)
            if first is not None:
                plan.copy_tuning(first)
        plan.n = batch
        return plan

    def rows_pending(self, batch: int, slot: int = 0) -> bool:
        """K1 has rewritten the border of the slot's input buffer and the slot's plan has not run since."""
        st = self._in_state.get(self._buf_key(batch, slot))
        return st is not None and not st.told

    def _tell_rows(self, plan, tensor: torch.Tensor, slot: int = 0) -> None:
        """Hand the plan the static rows K1 left in the slot's input buffer, once per (re)written border.  The promise is about
        that buffer alone: any other tensor runs over all rows."""
        n = self._buf_key(int(tensor.shape[0]), slot)
        own, st = self._in_bufs.get(n), self._in_state.get(n)
        if own is None or own.data_ptr() != tensor.data_ptr() or st is None:
            if plan.static_rows != (0, plan.H):
                plan.set_static_rows(0, plan.H)
                if st is not None:
                    st.told = False
            return
        if st.told:
            return
        plan.set_static_rows(*st.rows)                    # also where the rows are unchanged: the border bytes may be new
        st.told = True

    def _infer(self, tensor: torch.Tensor, slot: int = 0):
        """The head tensor of the batch; with ``hip_box_rows: fp32`` an ``ops.SplitHead`` (head tensor, fp32 box rows)."""
        if self._infer_fn is not None:
            return self._infer_fn(tensor)
        if self.half:
            if tensor.dtype != torch.float16:
                raise TypeError("half detector: the fused plan takes the fp16 tensor K1 writes")
            plan = self.plan_for(tensor, slot)
            if not torch.cuda.is_current_stream_capturing():
                self._tell_rows(plan, tensor, slot)
            plan(tensor.contiguous())
            return plan.result()
        if self.engine == "fused-f32":
            if tensor.dtype != torch.float32:
                raise TypeError("fp32 plan: takes the fp32 tensor K1 writes for half=false")
            return self.plan_for(tensor, slot)(tensor.contiguous())
        return self.net(tensor.float().contiguous(memory_format=torch.channels_last))

    def _postprocess_device(self, raw, metas: Sequence[N.Letterbox]) -> ops.PostBuffers:
        boxes = None
        if isinstance(raw, ops.SplitHead):
            raw, boxes = raw
        raw = raw.contiguous()
        B = raw.shape[0]
        A = raw.shape[2] if raw.shape[1] < raw.shape[2] else raw.shape[1]
        self._post = self._post_bufs.get((B, A))
        if self._post is None:
            self._post = self._post_bufs[(B, A)] = ops.PostBuffers.allocate(B, A, raw.device)
        return ops.postprocess(raw, self.config.confidence_threshold, self.config.iou_threshold, self.config.classes,
                               metas, max_det=A, out=self._post, ctx=self.ctx, boxes=boxes)

    # -- the three stages of a tick, as the pipelined runner drives them (same protocol as the temporal heads) -------------
    def stage_pre(self, packets: Sequence[FramePacket], slot: int = 0) -> _YoloTick:     # slot: the runner's tick parity; per-frame API: 0
        return _YoloTick(*self._preprocess([p.frame for p in packets], slot), slot)

    def stage_net(self, pre: _YoloTick):
        return self._infer(pre[0], pre.slot)

    def stage_post(self, raw, pre) -> ops.PostBuffers:
        return self._postprocess_device(raw, [pre[1]])

    # -- API ------------------------------------------------------------------------------------
    geometry_key = staticmethod(ops.geometry_key)

    def predict_batch_device(self, packets: Sequence[FramePacket]) -> ops.PostBuffers:
        """Device-resident result (no host sync): feeds the tracker kernel directly.  One frame geometry per call (the
        tick pipeline groups a mixed tick by geometry and issues one call per group)."""
        if len({self.geometry_key(p.frame) for p in packets}) != 1:
            raise ValueError("predict_batch_device needs one frame geometry per call; use predict_batch for mixed sizes")
        with torch.inference_mode():
            tensor, meta = self._preprocess([p.frame for p in packets])
            raw = self._infer(tensor)
            return self._postprocess_device(raw, [meta])

    def predict_batch(self, packets: Sequence[FramePacket]) -> List[List[Detection]]:
        out: List[Optional[List[Detection]]] = [None] * len(packets)
        groups = {}
        for i, p in enumerate(packets):
            groups.setdefault(self.geometry_key(p.frame), []).append(i)
        for idxs in groups.values():
            res = self.predict_batch_device([packets[i] for i in idxs]).to_host()
            for i, r in zip(idxs, res):
                p = packets[i]
                out[i] = [Detection(stream_name=p.stream.name, frame_id=p.frame_id, class_id=int(r["cls"][k]),
                                    confidence=float(r["conf"][k]),
                                    bbox_xyxy=tuple(float(v) for v in r["boxes"][k])) for k in range(r["n"])]
        return out  # type: ignore[return-value]

    def predict(self, packet: FramePacket) -> List[Detection]:
        return self.predict_batch([packet])[0]


def _is_file(p: str) -> bool:
    from pathlib import Path
    return bool(p) and Path(p).is_file()
