"""YAML configuration for the hot path: the same keys the reference reads (config.py:54-351),
restricted to the sections the detect/track path consumes.

Compatibility rules kept from the reference:
  * unknown keys are dropped silently (config.py:304-307);
  * ``streams`` must be a list, ``detectors`` a mapping id -> detector section (config.py:321-336);
  * the validation messages/limits of StreamConfig / DetectorConfig / TrackerConfig / PipelineConfig;
  * fields that the reference declares but never reads (``batch_size``, ``tracker.type``, ...) are
    accepted and carried, so a reference YAML loads unchanged.
Additions: backend ``"hip"`` (this library) is a valid detector backend, and the out-of-scope
sections (kafka / prometheus / ffmpeg_simulator) are kept as opaque dicts.  With backend ``"hip"``, the
detector key ``hip_engine`` picks the network's engine: ``"auto"`` (default; what a reference YAML gets)
= the hand-written fp16 plan for YOLO with ``half: true``, PyTorch-ROCm for YOLO with ``half: false`` and for
every temporal head; ``"plan"`` = the hand-written plan at the configured precision, i.e. the fp32 YOLO plan for
``half: false`` and, for ``model_type: cnn_lstm``, the fp32 clip plan (``half: false`` only: ``half: true`` is
refused at construction) and, for ``model_type: resnet``, the fp32 ResNet-18 plan (engine ``"resnet-f32"``,
resnet_plan.py; this head always runs float32, ``half`` has no effect on it).  The other temporal heads have no plan: with
``"plan"`` they keep PyTorch-ROCm and log a warning.  ``"native"`` is the strict form of ``"plan"``: every network of the detector runs as hand-written HIP at the
configured precision, or construction fails with ``ValueError`` (an ``infer_fn`` still overrides everything):

    head                    half: false                       half: true
    yolov8 architecture     as plan: engine "fused-f32"       as plan: engine "fused"
    yolov5 architecture     ValueError (no fp32 plan; also    as plan: engine "fused" (the fp16 YOLOv5 plan,
                            under plan; auto: PyTorch-ROCm)   engine.FusedYoloV5)
    yolo11 architecture     ValueError (no fp32 plan; also    as plan: engine "fused" (the fp16 YOLO11 plan,
                            under plan; auto: PyTorch-ROCm)   engine.FusedYolo11)
    cnn_lstm                as plan: engine "clip-f32"        ValueError (the plan is fp32 only) unless hip_lstm_fp16: true
    3d_cnn / slow_fast      engine "clip3d-f32"               ValueError (the plan is fp32 only) unless hip_clip_fp16: true
    conv_gru                ValueError (the reference defines no architecture, so there is no plan)
    resnet                  ValueError (no hand-written plan) ValueError (no hand-written plan) unless hip_resnet_fp16: true

Which YOLO architecture a ``yolov5`` / ``yolov8`` detector builds is no key of its own: it follows what the user handed over
(``detector.detector_architecture``).  YOLO11 (the ``yolo11<n|s|m|l>`` files of Ultralytics 8.3; head tensor as YOLOv8's), checked
first and under either ``model_type``, when ``model_path`` is an existing state dict with the attention convolution of C2PSA
(``model.10.m.0.attn.qkv.conv.weight``), or when the file name starts with ``yolo11`` / ``yolov11`` plus a scale letter while no such
file exists (seeded weights, logged as such; scale x has no plan).  YOLOv5 (v6.0 - v7.0, anchor-based head) when ``model_path`` is an existing state dict with
the YOLOv5 detect convolution (``model.24.m.0.weight``), or when ``model_type`` is ``yolov5`` and the file name starts with
``yolov5<n|s|m|l>`` while no such file exists (seeded weights, logged as such); YOLOv8 in every other case, as before -- ``model_type:
yolov5`` with the default ``yolov8n.pt``, every ``yolov8*`` name, and the ``yolov5*u`` names (anchor-free re-exports with the v8 head).

``hip_clip_fp16`` (a bool, default ``false``: what a reference YAML gets) opts the 3D-CNN head into its fp16 plan: with
``hip_engine: native``, ``model_type: 3d_cnn`` / ``slow_fast`` and ``half: true`` the network runs as engine ``"clip3d-f16"``
(clip_plan.Fused3dCnnF16: fp16 frames, weights and stored activations on the fp16 MFMA, fp32 sums and logits) where it is
otherwise refused.  The key changes nothing else: not ``half: false``, not ``cnn_lstm``, not ``plan`` or ``auto``:

    head                    hip_clip_fp16: false              hip_clip_fp16: true
    3d_cnn / slow_fast      half: true -> ValueError          half: true -> engine "clip3d-f16"  (hip_engine: native)

``hip_lstm_fp16`` (a bool, default ``false``: what a reference YAML gets) does the same for the CNN-LSTM head: with ``hip_engine:
plan`` or ``native``, ``model_type: cnn_lstm`` and ``half: true`` the network runs as engine ``"clip-f16"``
(clip_plan.FusedCnnLstmF16: fp16 frames, convolution and LSTM weights and stem output, conv1 and conv2 on the fp16 MFMA, fp32
sums, states and logits) where it is otherwise refused.  The key changes nothing else: not ``half: false``, not the other heads,
not ``auto``:

    head                    hip_lstm_fp16: false              hip_lstm_fp16: true
    cnn_lstm                half: true -> ValueError          half: true -> engine "clip-f16"  (hip_engine: plan / native)

``hip_resnet_fp16`` (a bool, default ``false``: what a reference YAML gets) is the opt-in of the ResNet head: with ``hip_engine:
plan`` or ``native``, ``model_type: resnet`` and ``half: true`` the network runs as engine ``"resnet-f16"``
(resnet_plan.FusedResNet18F16: fp16 frames, convolution weights and stored activations on the fp16 MFMA, fp32 sums, mean and
logits).  The key changes nothing else: without it ``plan`` stays ``"resnet-f32"`` whatever ``half`` says and ``native`` stays
refused, as it does with ``half: false``; ``auto`` is PyTorch-ROCm:

    head                    hip_resnet_fp16: false                        hip_resnet_fp16: true
    resnet, plan            engine "resnet-f32" (half has no effect)      half: true -> engine "resnet-f16"
    resnet, native          ValueError (no hand-written plan)             half: true -> engine "resnet-f16"

Which ResNet the head builds is no key of its own either: it follows ``model_path`` (``classify.HipResNetDetector``).  An existing
state dict of the torchvision family there (ResNet-18 / 34 with BasicBlocks, ResNet-50 / 101 / 152 with Bottlenecks, any 1..64
blocks per stage; ``resnet_num_classes`` must agree with its ``fc.weight``) builds a ``classify.ResNet`` of what the file says;
with no such file, a name that starts with ``resnet34`` / ``resnet50`` / ``resnet101`` / ``resnet152`` builds the seeded network
of that depth; every other name keeps the seeded ``classify.ResNet18``.  Engine ``"resnet-f16"`` runs either module
(``classify.ResNet`` on resnet_plan.FusedResNetF16); the fp32 plan exists for ``classify.ResNet18`` only:

    module                  auto              plan / native, half: true, hip_resnet_fp16: true    plan otherwise
    classify.ResNet18       PyTorch-ROCm      engine "resnet-f16" (FusedResNet18F16)              engine "resnet-f32"
    classify.ResNet         PyTorch-ROCm      engine "resnet-f16" (FusedResNetF16)                ValueError at construction

``hip_box_rows`` picks where the fp16 YOLO plan (engine ``"fused"``: ``half: true``) keeps the four box
rows of its head: ``"fp16"`` (default; what a reference YAML gets) = rows 0-3 of the fp16 head tensor, whose ulp is
0.25 px between 256 and 512; ``"fp32"`` = the head kernels also write them as an fp32 side tensor and the post-process
reads its boxes from there (class rows stay fp16).  With ``half: false`` the boxes are fp32 already and the key is
accepted without effect, as it is for a detector that is given an ``infer_fn`` (no plan).

``hip_plan_capacity`` (an integer >= 0) says how the YOLO plans (engines ``"fused"`` and ``"fused-f32"``) serve the batch of
a tick, which is the number of streams that delivered a frame: ``0`` (default; what a reference YAML gets) = one plan and one
input buffer per batch size, built when that size first occurs; ``N > 0`` = ONE plan and one input buffer of ``N`` images per
input size (and pipeline slot), of which a tick runs its leading ``n <= N`` (``rva_yolov8_plan_run_n``): no plan is built in
the middle of a run when a stream drops a frame, and a stream's head tensor does not depend on how many others delivered one.
A group of more than ``N`` frames gets an exact-size plan as with ``0``, and a warning in the log.  No effect behind an
``infer_fn`` or on the PyTorch-ROCm engine (``half: false`` with ``hip_engine: auto``).
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional

import yaml

HIP_BACKENDS = ("hip", "rocm", "mi355x")
REFERENCE_BACKENDS = ("ultralytics", "tensorrt", "onnx", "onnxruntime", "openvino", "rknn", "rk3588")
HIP_ENGINES = ("auto", "plan", "native")
HIP_BOX_ROWS = ("fp16", "fp32")
TEMPORAL_MODELS = ("cnn_lstm", "3d_cnn", "conv_gru", "slow_fast")
MODEL_TYPES = ("yolov5", "yolov8", "resnet") + TEMPORAL_MODELS


class ConfigError(RuntimeError):
    """Raised when the supplied configuration is invalid."""


def _need(cond: bool, msg: str) -> None:
    if not cond:
        raise ConfigError(msg)


@dataclass(slots=True)
class StreamConfig:
    name: str
    url: str
    enabled: bool = True
    target_fps: Optional[float] = None
    batch_size: int = 1
    warmup_seconds: float = 2.0
    reconnect_backoff: float = 5.0
    max_retries: Optional[int] = None
    detector_id: Optional[str] = None
    roi_polygons: Optional[list] = None
    motion_filter: bool = False
    motion_threshold: float = 0.02
    downsample_ratio: float = 1.0
    adaptive_fps: bool = False
    min_target_fps: float = 5.0
    idle_frame_tolerance: int = 60
    ffmpeg_simulator: Optional[dict] = None   # out of scope: carried, never interpreted

    def validate(self) -> None:
        n = self.name
        _need(bool(n), "Stream name must not be empty")
        _need(bool(self.url), f"Stream '{n}' must define a non-empty url")
        _need(self.batch_size >= 1, f"Stream '{n}' batch_size must be >= 1")
        _need(self.target_fps is None or self.target_fps > 0, f"Stream '{n}' target_fps must be > 0 if provided")
        _need(self.warmup_seconds >= 0, f"Stream '{n}' warmup_seconds must be >= 0")
        _need(self.reconnect_backoff >= 0, f"Stream '{n}' reconnect_backoff must be >= 0")
        _need(self.max_retries is None or self.max_retries >= 0, f"Stream '{n}' max_retries must be >= 0")
        _need(self.motion_threshold >= 0, f"Stream '{n}' motion_threshold must be >= 0")
        _need(0.1 <= self.downsample_ratio <= 1.0, f"Stream '{n}' downsample_ratio must be between 0.1 and 1.0")
        if self.adaptive_fps:
            _need(0 < self.min_target_fps <= (self.target_fps or 30),
                  f"Stream '{n}' min_target_fps must be > 0 and <= target_fps when adaptive_fps is enabled")


@dataclass(slots=True)
class DetectorConfig:
    model_path: str = "yolov8n.pt"
    device: str = "auto"
    backend: str = "ultralytics"
    model_type: str = "yolov8"
    confidence_threshold: float = 0.5
    iou_threshold: float = 0.45
    classes: Optional[List[int]] = None
    half: bool = False
    warmup: bool = True
    input_size: Optional[List[int]] = None  # H, W
    tensorrt_max_workspace_size: int = 1 << 30
    tensorrt_use_fp16: bool = False
    resnet_num_classes: int = 1000
    resnet_top_k: int = 5
    sequence_length: int = 16
    sequence_stride: int = 1
    temporal_overlap: float = 0.5
    temporal_pooling: str = "avg"
    action_classes: Optional[List[str]] = None
    num_action_classes: int = 400
    hip_engine: str = "auto"                # backend "hip": "auto", "plan" or "native" (module docstring)
    hip_box_rows: str = "fp16"              # backend "hip", YOLO with half: true: "fp16" or "fp32" (module docstring)
    hip_clip_fp16: bool = False             # backend "hip", 3d_cnn / slow_fast with half: true and native: the fp16 plan (module docstring)
    hip_lstm_fp16: bool = False             # backend "hip", cnn_lstm with half: true and plan / native: the fp16 plan (module docstring)
    hip_resnet_fp16: bool = False           # backend "hip", resnet with half: true and plan / native: the fp16 plan (module docstring)
    hip_plan_capacity: int = 0              # backend "hip", YOLO plans: 0 = a plan per batch size, N = one plan of N images (module docstring)

    def validate(self) -> None:
        _need(bool(self.model_path), "Detector model_path must not be empty")
        _need(self.hip_engine in HIP_ENGINES, f"hip_engine must be one of {set(HIP_ENGINES)}")
        _need(self.hip_box_rows in HIP_BOX_ROWS, f"hip_box_rows must be one of {set(HIP_BOX_ROWS)}")
        _need(isinstance(self.hip_clip_fp16, bool), "hip_clip_fp16 must be true or false")
        _need(isinstance(self.hip_lstm_fp16, bool), "hip_lstm_fp16 must be true or false")
        _need(isinstance(self.hip_resnet_fp16, bool), "hip_resnet_fp16 must be true or false")
        _need(isinstance(self.hip_plan_capacity, int) and not isinstance(self.hip_plan_capacity, bool) and self.hip_plan_capacity >= 0,
              "hip_plan_capacity must be an integer >= 0")
        _need(self.backend in REFERENCE_BACKENDS + HIP_BACKENDS,
              f"Detector backend must be one of {set(REFERENCE_BACKENDS + HIP_BACKENDS)}")
        _need(self.model_type in MODEL_TYPES, f"Model type must be one of {set(MODEL_TYPES)}")
        _need(0.0 < self.confidence_threshold <= 1.0, "confidence_threshold must be in (0, 1]")
        _need(0.0 < self.iou_threshold <= 1.0, "iou_threshold must be in (0, 1]")
        _need(not self.input_size or len(self.input_size) == 2, "input_size must be [height, width]")
        if self.model_type in TEMPORAL_MODELS:
            _need(self.backend in ("onnx", "onnxruntime", "openvino") + HIP_BACKENDS,
                  "Temporal models currently only supported with ONNX Runtime, OpenVINO or HIP backends")
            _need(self.sequence_length > 0, "sequence_length must be > 0 for temporal models")
            _need(self.sequence_stride > 0, "sequence_stride must be > 0 for temporal models")
            _need(0.0 <= self.temporal_overlap < 1.0, "temporal_overlap must be in [0, 1) for temporal models")
            _need(self.temporal_pooling in ("avg", "max", "last"), "temporal_pooling must be one of: avg, max, last")
            _need(self.num_action_classes > 0, "num_action_classes must be > 0 for temporal models")


@dataclass(slots=True)
class TrackerConfig:
    type: str = "byte_track"      # a label nothing reads: the tracker is always the IoU tracker
    max_age: int = 30
    max_iou_distance: float = 0.7  # despite the name: the MINIMUM IoU for a match (tracker.py:106)
    min_hits: int = 3

    def validate(self) -> None:
        _need(self.max_age >= 1, "Tracker max_age must be >= 1")
        _need(self.max_iou_distance > 0, "Tracker max_iou_distance must be > 0")
        _need(self.min_hits >= 0, "Tracker min_hits must be >= 0")


@dataclass(slots=True)
class PipelineConfig:
    streams: List[StreamConfig] = field(default_factory=list)
    detector: DetectorConfig = field(default_factory=DetectorConfig)
    detectors: Dict[str, DetectorConfig] = field(default_factory=dict)
    tracker: TrackerConfig = field(default_factory=TrackerConfig)
    kafka: Dict[str, Any] = field(default_factory=dict)        # out of scope: opaque
    prometheus: Dict[str, Any] = field(default_factory=dict)   # out of scope: opaque
    max_concurrent_streams: int = 32
    stats_interval_seconds: float = 15.0

    def validate(self) -> None:
        _need(bool(self.streams), "At least one stream must be configured")
        _need(self.max_concurrent_streams >= 1, "max_concurrent_streams must be >= 1")
        _need(len(self.streams) <= self.max_concurrent_streams,
              f"Configured {len(self.streams)} streams but max_concurrent_streams={self.max_concurrent_streams}")
        _need(self.stats_interval_seconds > 0, "stats_interval_seconds must be > 0")
        for s in self.streams:
            _need(not s.detector_id or s.detector_id in self.detectors,
                  f"Stream '{s.name}' references unknown detector_id='{s.detector_id}'")
            s.validate()
        self.detector.validate()
        for d in self.detectors.values():
            d.validate()
        self.tracker.validate()

    def detector_for(self, stream: StreamConfig) -> DetectorConfig:
        return self.detectors[stream.detector_id] if stream.detector_id else self.detector


def _build(cls, data: Optional[dict]):
    names = {f.name for f in dataclasses.fields(cls)}
    return cls(**{k: v for k, v in (data or {}).items() if k in names})


def load_config(path) -> PipelineConfig:
    p = Path(path)
    if not p.exists():
        raise ConfigError(f"Configuration file not found: {p}")
    raw = yaml.safe_load(p.read_text(encoding="utf-8"))
    return config_from_dict(raw)


def config_from_dict(raw) -> PipelineConfig:
    _need(isinstance(raw, dict), "Top level configuration must be a mapping/dictionary")
    _need(isinstance(raw.get("streams"), list), "'streams' must be a list in the configuration")
    dets = raw.get("detectors") or {}
    _need(isinstance(dets, dict), "'detectors' section must be a mapping of id -> config")
    cfg = PipelineConfig(
        streams=[_build(StreamConfig, s) for s in raw["streams"]],
        detector=_build(DetectorConfig, raw.get("detector")),
        detectors={k: _build(DetectorConfig, v) for k, v in dets.items()},
        tracker=_build(TrackerConfig, raw.get("tracker")),
        kafka=dict(raw.get("kafka") or {}),
        prometheus=dict(raw.get("prometheus") or {}),
        max_concurrent_streams=raw.get("max_concurrent_streams", 32),
        stats_interval_seconds=raw.get("stats_interval_seconds", 15.0),
    )
    cfg.validate()
    return cfg
