"""The fused fp16 YOLOv5 plan (``engine.FusedYoloV5`` / ``rva_yolov5_plan_create``), the detector and the pipeline on top of it.

Accuracy: the head tensor against the float64 module fed the same fp16-rounded input and the same folded-then-rounded weights, per
row group (xy, wh, objectness, classes).  The yardstick is the error of the SAME module run by PyTorch-ROCm in fp16 (channels-last)
against that float64 output: both pipelines store fp16 activations and differ only in summation order and rounding points, so the
plan's largest error may be at most twice PyTorch's -- a condition, not a measurement.  Both errors are printed, and recorded where
``RVA_REPORT_DIR`` names a directory.  Every test but one runs variant 0 on every step (``_no_tuner``); that one runs the real tuner
once and holds the tuned plan to the same condition (every row forced on YOLOv5 steps: tests/test_gpu_conv_slices.py).
Bit-identity: ``run_n(1)`` == image 0 of a full run; eager == a hipGraph replay; a primed windowed run == a fresh plan; the gather-64
variants forced on the head steps == variant 0 (each logit is the same fp32 sum over the same 64-channel K-steps in every tile:
tests/test_gpu_yolov5_prims.py shows it for the primitive, so the tolerance is zero).
End to end: ``create_detector`` with ``model_type: yolov5`` against the oracle's post-process of the plan's own head tensor, and
``PipelinedTicks`` against ``TickPipeline.tick``."""
import copy
import functools
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector, create_detector
from realtime_video_analytics_32streams_amd.engine import FusedYoloV5, FusedYoloV8
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from realtime_video_analytics_32streams_amd.yolov5 import YoloV5, build_detector_net_v5, calibrate_detection_density_v5
from tests.helpers import v5_groups_over_twice_torch, v5_head_errors

pytestmark = pytest.mark.gpu

CUSTOM_ANCHORS = [[6, 9, 14, 11, 19, 27], [25, 40, 51, 33, 44, 90], [80, 70, 120, 160, 250, 230]]
CASES = {"n": ("n", 80, None, (2, 64, 96)), "s-nc3-custom-anchors": ("s", 3, CUSTOM_ANCHORS, (1, 64, 64))}


def _with_tuner(test):
    """Marks the one test that runs the real tuner."""
    test.uses_tuner = True
    return test


@pytest.fixture(autouse=True)
def _no_tuner(request, monkeypatch):
    """The detector's plans run every layer with the library's own choice (variant 0): the tuner only picks among kernels."""
    if not getattr(request.function, "uses_tuner", False):
        monkeypatch.setattr(FusedYoloV8, "autotune", lambda self, reps=5: None)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _net(case):
    """Seeded, BatchNorm folded, every parameter rounded to fp16 (kept as fp32): the plan, the fp16 module and the float64 module
    then hold the same numbers, biases included (the plan keeps biases in fp32).  Shared, never modified."""
    scale, nc, anchors, _ = CASES[case]
    net = build_detector_net_v5(scale, seed=7, nc=nc, anchors=anchors).fuse()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.half().float())
    return net


@functools.lru_cache(maxsize=None)
def _input(case):
    b, h, w = CASES[case][3]
    return torch.rand((b, 3, h, w), generator=torch.Generator().manual_seed(11)).half()


@functools.lru_cache(maxsize=None)
def _float64_head(case):
    """``[B, 5 + nc, A]`` float64 from the float64 module on the CPU."""
    with torch.inference_mode():
        return copy.deepcopy(_net(case)).double()(_input(case).double()).transpose(1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _torch_fp16_head(case):
    """``[B, 5 + nc, A]`` float64 on the CPU: the same module run by PyTorch-ROCm in fp16, channels-last."""
    ref16 = copy.deepcopy(_net(case)).half().cuda().to(memory_format=torch.channels_last)
    with torch.inference_mode():
        return ref16(_input(case).cuda().contiguous(memory_format=torch.channels_last)).transpose(1, 2).double().cpu()


def _check_against_float64(case, got, tag):
    """The condition of this file: per row group the plan's error is at most twice PyTorch fp16's.  Returns what was measured."""
    want, tor = _float64_head(case), _torch_fp16_head(case)
    assert bool(torch.isfinite(got).all()) and got.shape == want.shape == tor.shape
    rec = v5_head_errors(got, tor, want)
    for name, e in rec.items():
        print(f"[yolov5 {tag}] {name}: plan max |d| {e['plan_max_err']:.4g}, PyTorch fp16 max |d| {e['torch_fp16_max_err']:.4g}, "
              f"ratio {e['plan_max_err'] / max(e['torch_fp16_max_err'], 1e-30):.2f}")
    bad = v5_groups_over_twice_torch(rec)
    return rec, bad


def _plan(case, **kw):
    b, h, w = CASES[case][3]
    kw.setdefault("autotune", False)
    return FusedYoloV5(copy.deepcopy(_net(case)), b, (h, w), **kw)


def _record(key, value):
    out = os.environ.get("RVA_REPORT_DIR")
    if out and Path(out).is_dir():
        path = Path(out) / "yolov5_accuracy.json"
        data = json.loads(path.read_text()) if path.exists() else {}
        data[key] = value
        path.write_text(json.dumps(data, indent=1, sort_keys=True))


@pytest.mark.parametrize("case", list(CASES))
def test_head_tensor_against_the_float64_module(case):
    scale, nc, _, (b, h, w) = CASES[case]
    A = 3 * sum((h // s) * (w // s) for s in (8, 16, 32))
    plan = _plan(case)
    assert isinstance(plan, FusedYoloV8) and plan.nc == nc and plan.A == A and tuple(plan.out.shape) == (b, 5 + nc, A)
    assert not plan.fused_head_lanes() and plan.n_launches == plan._n_steps
    x = _input(case).cuda()
    got = plan(x).double().cpu()
    torch.cuda.synchronize()
    rec, bad = _check_against_float64(case, got, case)
    _record(case, rec)
    assert not bad, bad


@_with_tuner
def test_autotuned_plan_meets_the_float64_condition(monkeypatch):
    """The real tuner, once: ``autotune(reps=1)`` on the YOLOv5n plan with the selection cache off (nothing read, nothing written)
    moves steps off variant 0 by time alone, and the head tensor still meets the condition of the test above."""
    case = "n"
    monkeypatch.setenv("RVA_TUNE_CACHE", "0")
    for name in ("RVA_SKIP_VARIANTS", "RVA_TUNE_LAYER_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    assert CASES[case][3] == (2, 64, 96)
    plan = _plan(case)
    assert all(st["variant"] == 0 for _, st, _ in plan._tunable)
    plan.autotune(reps=1)
    torch.cuda.synchronize()
    picks = [(desc, st["variant"]) for _, st, desc in plan._tunable]
    print("[yolov5 n tuned] selection:", picks)
    assert plan.tuning_source == "measured" and any(v for _, v in picks), picks
    got = plan(_input(case).cuda()).double().cpu()
    torch.cuda.synchronize()
    rec, bad = _check_against_float64(case, got, "n tuned")
    assert not bad, (bad, picks)


def test_bit_identity_of_partial_runs_graphs_windows_and_head_variants():
    case = "n"
    b, h, w = CASES[case][3]
    x = _input(case).cuda()
    plan = _plan(case)
    full = plan(x).clone()
    torch.cuda.synchronize()
    # one image on the two-image plan
    plan.out.fill_(-3.0)
    one = plan(x[:1].contiguous())
    torch.cuda.synchronize()
    assert _same(one, full[:1]) and bool((plan.out[1] == -3.0).all()), "run_n, n = 1"
    # a hipGraph replay
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan(x)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            plan(x)
    plan.out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same(plan.out, full), "hipGraph replay"
    # the gather-64 tiles forced on the three head steps
    heads = [(st, d) for _, st, d in plan._tunable if d.startswith("head5:")]
    assert len(heads) == 3
    for v in (33, 36, 38):
        for st, _ in heads:
            st["variant"] = v
        plan.out.zero_()
        assert _same(plan(x), full), v
    for st, _ in heads:
        st["variant"] = 0
    del plan
    # static rows: prime on x, then only rows 10..49 of the input change
    x2 = x.clone()
    x2[:, :, 10:50] = torch.rand((b, 3, 40, w), generator=torch.Generator().manual_seed(5)).half().cuda()
    want2 = _plan(case)(x2).clone()
    rows = _plan(case, static_rows=(10, 50))
    assert rows.static_rows == (10, 50) and rows.step_rows(0) == (4, 26)          # stem: output row r reads input rows 2r-2 .. 2r+3
    rows(x)
    assert rows.primed
    got2 = rows(x2).clone()
    torch.cuda.synchronize()
    assert _same(got2, want2), "static rows"
    assert rows.step_rows(1)[0] > 0, "b1 is not windowed"


def test_box_rows_fp32_and_refusals():
    case = "n"
    x = _input(case).cuda()
    want = _plan(case)(x).clone()
    side = _plan(case, box_rows="fp32")
    side.boxes32.fill_(float("nan"))
    got = side(x).clone()
    torch.cuda.synchronize()
    assert _same(got, want) and tuple(side.boxes32.shape) == (2, 4, side.A) and bool(torch.isfinite(side.boxes32).all())
    assert _same(side.boxes32.half(), got[:, :4])
    assert isinstance(side.result(), ops.SplitHead)
    with pytest.raises(ValueError, match="no fp32 YOLOv5 plan"):
        _plan(case, precision="fp32")
    with pytest.raises(RuntimeError, match="stem wider than 64 channels"):
        FusedYoloV5(YoloV5("x", 2).eval(), 1, (64, 64), autotune=False)


# ------------------------------------------------------------------------------------------------ detector and pipeline
def _cfg(**kw):
    base = dict(backend="hip", model_type="yolov5", model_path="yolov5n.pt", half=True, warmup=False, confidence_threshold=0.25,
                iou_threshold=0.5)
    base.update(kw)
    return DetectorConfig(**base)


def _calibrated(sample, target=60, **kw):
    det = create_detector(_cfg(**kw))
    assert isinstance(det, HipYoloDetector) and isinstance(det.net, YoloV5) and det.arch == "yolov5" and det.engine == "fused"
    with torch.inference_mode():
        calibrate_detection_density_v5(det.net, sample.contiguous(memory_format=torch.channels_last), 0.25, target)
    det.invalidate_engine()
    return det


@functools.lru_cache(maxsize=None)
def _frames():
    W, H = 640, 360
    return tuple(ops.Nv12Surface.from_numpy(*synth.make_nv12(40 + i, W, H), W, H) for i in range(2))


def _packets(frames):
    stream = StreamConfig(name="cam", url="x")
    return [FramePacket(stream=stream, frame=f, frame_id=i, timestamp=0.0) for i, f in enumerate(frames)]


def _predict(det, frames):
    raws = []
    infer = det._infer
    det._infer = lambda t: raws.append(infer(t)) or raws[-1]
    dets = det.predict_batch(_packets(frames))
    det._infer = infer
    return dets, raws[0]


def test_create_detector_yolov5_matches_the_oracle_at_640():
    """Two 640 x 360 NV12 frames at 640 x 640: K2 / K3 see 25200 anchors.  The Detection objects == the oracle's post-process of the
    head tensor the plan produced; ``hip_box_rows: fp32`` gives equal scores and boxes from the side tensor; ``hip_plan_capacity: 4``
    gives the exact-size plan's detections."""
    frames = list(_frames())
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12(frames, (640, 640), half=True)
    sample = sample.clone()
    det = _calibrated(sample)
    dets, head = _predict(det, frames)
    plan = det._plans[(2, 640, 640)]
    assert isinstance(plan, FusedYoloV5) and tuple(head.shape) == (2, 85, 25200) and head.dtype == torch.float16
    assert ops.post_status(det.ctx) == 0, "K2 / K3 overflow flag"
    total = 0
    for i in range(2):
        r = orc.postprocess(head[i].float().cpu().numpy(), 0.25, 0.5, None, (640, 360))
        assert [d.class_id for d in dets[i]] == [int(v) for v in r["cls"]], i
        assert [d.confidence for d in dets[i]] == [float(v) for v in r["conf"]], i
        assert [list(d.bbox_xyxy) for d in dets[i]] == [[float(v) for v in b] for b in r["boxes"]], i
        total += len(dets[i])
    assert total > 0, "the calibrated detector produced nothing"
    # the fp32 side tensor: same anchors, classes and scores; boxes from boxes32 (within the fp16 ulp of the head's rows)
    det32 = _calibrated(sample, hip_box_rows="fp32")
    dets32, res = _predict(det32, frames)
    assert isinstance(res, ops.SplitHead) and _same(res[0], head) and _same(res[1].half(), head[:, :4])
    for i in range(2):
        composite = head[i].float().cpu().numpy()                  # the oracle on the same head (equal scores) with its box rows in fp32
        composite[:4] = res[1][i].cpu().numpy()
        r = orc.postprocess(composite, 0.25, 0.5, None, (640, 360))
        assert [(d.class_id, d.confidence) for d in dets32[i]] == [(int(c), float(v)) for c, v in zip(r["cls"], r["conf"])], i
        assert [list(d.bbox_xyxy) for d in dets32[i]] == [[float(v) for v in b] for b in r["boxes"]], i
    # one plan of four images serving two frames
    cap = _calibrated(sample, hip_plan_capacity=4)
    dets4, head4 = _predict(cap, frames)
    assert (4, 640, 640) in cap._plans and tuple(head4.shape) == (2, 85, 25200)
    assert dets4 == dets


def test_half_false_engines():
    det = create_detector(_cfg(half=False))
    assert det.engine == "torch-fp32" and isinstance(det.net, YoloV5)
    for eng in ("plan", "native"):
        with pytest.raises(ValueError, match="half: true"):
            create_detector(_cfg(half=False, hip_engine=eng))
    # what stays YOLOv8
    from realtime_video_analytics_32streams_amd.yolov8 import YoloV8
    assert isinstance(create_detector(_cfg(model_path="yolov8n.pt")).net, YoloV8)
    assert isinstance(create_detector(_cfg(model_path="yolov5nu.pt")).net, YoloV8)


def _tab(tracks):
    return [(t.track_id, t.class_id, t.age, t.hits, t.confidence, t.bbox_xyxy) for t in tracks]


def test_pipelined_ticks_equal_synchronous_ticks():
    """Four synthetic 1080p NV12 streams: ``PipelinedTicks(depth=2)`` gives the tracks of ``TickPipeline.tick(device_gates=True)``."""
    S, T = 4, 4
    streams = [StreamConfig(name=f"cam{i}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]

    def sources():
        out = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
        for s in out:
            s.open_sync()
        return out
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in sources()], (640, 640), half=True)
    det = _calibrated(sample.clone())
    tcfg = TrackerConfig(max_age=3, max_iou_distance=0.5, min_hits=1)

    pipe = TickPipeline(streams, det, IouTracker(tcfg, max_streams=S, capacity=512), sources=sources())
    want = [{n: _tab(v) for n, v in pipe.tick(device_gates=True).tracks.items()} for _ in range(T)]
    assert sum(len(v) for t in want for v in t.values()) > 0
    runner = PipelinedTicks(TickPipeline(streams, det, IouTracker(tcfg, max_streams=S, capacity=512), sources=sources()), depth=2)
    got, inflight = [], 0
    for _ in range(T):
        if inflight == 2:
            got.append({n: _tab(v) for n, v in runner.collect_result().tracks.items()}); inflight -= 1
        runner.submit(); inflight += 1
    while inflight:
        got.append({n: _tab(v) for n, v in runner.collect_result().tracks.items()}); inflight -= 1
    assert got == want
