"""The YOLOv8 plans (fp16 and fp32) for any class count, and the detector and the pipeline on top of them.

Inside the plan the class branch runs with padded channel counts and zero-extended weights (csrc/rva_plan.hip), and the head
kernels store the nc real class rows.  What is pinned, per case and precision:
  (a) the head tensor is ``[B, 4 + nc, A]`` and equals, bit for bit, rows ``0 .. 4+nc-1`` of a SIBLING plan whose module really has
      the padded class count and interior width, with zero-extended weights (for nc = 1, 3, 20 in fp16 that is today's nc = 8 / 24
      path; the fp32 convolutions give the same bits for every tile);
  (b) fp16: the rounding-matched torch reference of tests/helpers.py, tolerances unchanged;
  (c) fp32: the float64 module within the bounds of tests/test_gpu_plan_f32.py (0.01 px, 2e-5, no threshold flips), the net
      calibrated as there;
  (d) ``_run`` == ``_run_lanes`` == a hipGraph replay;  (e) ``run_n`` with n = 1 == image 0 of the full run, image 1 untouched;
  (f) ``box_rows="fp32"``: the fp16 head unchanged, ``half(boxes32)`` == rows 0-3;  (g) a static-row window gives the same bits.
End to end: ``HipYoloDetector(net=...)`` for nc = 1 (the reference's 5-row branch: plain scores) and 3 against the oracle's
post-process of the plan's own head tensor, and a three-tick ``PipelinedTicks`` run against the oracle's tracker."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from realtime_video_analytics_32streams_amd.detector import HipYoloDetector
from realtime_video_analytics_32streams_amd.engine import FusedYoloV8
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from realtime_video_analytics_32streams_amd.yolov8 import ConvBnAct, build_detector_net, calibrate_detection_density
from tests.helpers import assert_matches_rounded_reference, plan_rounded_reference

pytestmark = pytest.mark.gpu

BOX_TOL, PROB_TOL = 0.01, 2e-5          # tests/test_gpu_plan_f32.py
B = 2
CASES = [("n", 1, (64, 96)),            # the C == 5 branch of the post-process
         ("n", 91, (64, 96)),           # interior width 91 -> 96, unfused head (one three-level launch)
         ("s", 3, (96, 160)),
         ("m", 20, (64, 96)),
         ("s", 3, (640, 640))]          # the variant selection depends on the map size
IDS = [f"{s}-nc{nc}-{h}x{w}" for s, nc, (h, w) in CASES]


def _up(n, m):
    return (n + m - 1) // m * m


@functools.lru_cache(maxsize=None)
def _net(scale, nc):
    """Seeded weights, calibrated as tests/test_gpu_plan_f32.py calibrates its nets (four random 640 x 640 images, 60 anchors per
    image above 0.25); fused, fp32, on the device.  Shared, never modified."""
    net = build_detector_net(scale, seed=7, nc=nc).fuse().cuda().float()
    with torch.inference_mode():
        sample = torch.rand((4, 3, 640, 640), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
        calibrate_detection_density(net, sample.contiguous(memory_format=torch.channels_last), 0.25, 60)
    return net


def _input(hw):
    return torch.rand((B, 3, *hw), device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))


def _sibling(net, f32):
    """``net`` with the class branch as the plan runs it: interior width rounded up to 8 (16 for fp32), roundup(nc, 8) classes,
    weights and biases zero-extended."""
    sib = copy.deepcopy(net)
    cc = net.detect.cls[0][1].conv.out_channels
    ccp, ncp = _up(cc, 16 if f32 else 8), _up(net.nc, 8)

    def grown(conv, cin, cout, act):
        if act:
            m = ConvBnAct(conv.in_channels, conv.out_channels, conv.kernel_size[0])
            m.fuse()
            m.conv = torch.nn.Conv2d(cin, cout, conv.kernel_size, conv.stride, conv.padding, bias=True)
            new = m.conv
        else:
            m = new = torch.nn.Conv2d(cin, cout, 1)
        with torch.no_grad():
            new.weight.zero_(); new.bias.zero_()
            new.weight[:conv.out_channels, :conv.in_channels] = conv.weight
            new.bias[:conv.out_channels] = conv.bias
        return m
    sib.detect.cls = torch.nn.ModuleList(
        torch.nn.Sequential(grown(seq[0].conv, seq[0].conv.in_channels, ccp, True), grown(seq[1].conv, ccp, ccp, True), grown(seq[2], ccp, ncp, False))
        for seq in net.detect.cls)
    sib.nc = sib.detect.nc = ncp
    return sib.to(next(net.parameters()).device)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _anchors(hw):
    return sum((hw[0] // s) * (hw[1] // s) for s in (8, 16, 32))


def _graph_replay(plan, x):
    """``plan(x)`` captured into a hipGraph (the plain run, branches in line) and replayed into a zeroed output."""
    plan.concurrent_heads = False
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
    return plan.out.clone()


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_of_any_class_count(case, precision):
    scale, nc, hw = case
    f32 = precision == "fp32"
    net = _net(scale, nc)
    x = _input(hw)
    x = x if f32 else x.half()
    A = _anchors(hw)
    plan = FusedYoloV8(copy.deepcopy(net), B, hw, autotune=False, precision=precision)
    assert plan.nc == nc and plan.A == A and tuple(plan.out.shape) == (B, 4 + nc, A)
    plan.concurrent_heads = False
    run = plan(x).clone()
    torch.cuda.synchronize()
    assert tuple(run.shape) == (B, 4 + nc, A) and bool(torch.isfinite(run).all())
    # (a) the sibling with the padded module
    sib = FusedYoloV8(_sibling(net, f32), B, hw, autotune=False, precision=precision)
    assert sib.nc == _up(nc, 8) and [d for _, _, d in sib._tunable] == [d for _, _, d in plan._tunable]
    sib.concurrent_heads = False
    wide = sib(x).clone()
    torch.cuda.synchronize()
    assert _same(run, wide[:, :4 + nc]), "not the bits of the padded module's plan"
    del sib
    # (b) / (c) the references
    if f32:
        ref = copy.deepcopy(net).cpu().double()
        with torch.inference_mode():
            want = ref(x.detach().cpu().double())
        got = run.detach().cpu().double()
        box, prob = float((got[:, :4] - want[:, :4]).abs().max()), float((got[:, 4:] - want[:, 4:]).abs().max())
        flips = int(((got[:, 4:] >= 0.25) != (want[:, 4:] >= 0.25)).sum())
        print(f"\n[f32 plan {scale} nc {nc} {hw}] max |d box| {box:.3g} px, max |d prob| {prob:.3g}, flips@0.25 {flips}")
        assert box <= BOX_TOL and prob <= PROB_TOL and flips == 0, (box, prob, flips)
    else:
        berr, serr = assert_matches_rounded_reference(run, plan_rounded_reference(net, x))
        print(f"\n[f16 plan {scale} nc {nc} {hw}] max |d box| {berr:.3g} px, max |d score| {serr:.3g} against the rounding-matched reference")
    # (d) lanes and a hipGraph replay
    plan.concurrent_heads = True
    plan.out.zero_()
    lanes = plan(x).clone()
    torch.cuda.synchronize()
    assert _same(run, lanes), "_run_lanes"
    assert _same(run, _graph_replay(plan, x)), "hipGraph replay"
    # (e) one image on the two-image plan
    plan.out.fill_(-3.0)
    one = plan(x[:1].contiguous())
    torch.cuda.synchronize()
    assert tuple(one.shape) == (1, 4 + nc, A) and _same(one, run[:1]) and bool((plan.out[1] == -3.0).all()), "run_n, n = 1"
    del plan
    # (g) a static-row window: the rows outside it keep the priming run's bytes, the rows inside follow the input
    top, bottom = hw[0] // 4, hw[0] - hw[0] // 4
    x2 = x.clone()
    x2[:, :, top:bottom] = torch.rand((B, 3, bottom - top, hw[1]), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).to(x.dtype)
    plain = FusedYoloV8(copy.deepcopy(net), B, hw, autotune=False, precision=precision)
    want2 = plain(x2).clone()
    rows = FusedYoloV8(copy.deepcopy(net), B, hw, autotune=False, precision=precision, static_rows=(top, bottom))
    rows.concurrent_heads = plain.concurrent_heads = False
    rows(x)                                                             # primes: all rows
    got2 = rows(x2).clone()                                             # fp16: windows
    torch.cuda.synchronize()
    assert (rows.primed and rows.static_rows == (top, bottom)) or f32
    assert _same(got2, want2), "static rows"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_box_rows_fp32_of_any_class_count(case):
    """(f): the side tensor sits behind a head of (4 + nc) * A halves per image, whatever its parity."""
    scale, nc, hw = case
    net = _net(scale, nc)
    x = _input(hw).half()
    plain = FusedYoloV8(copy.deepcopy(net), B, hw, autotune=False)
    side = FusedYoloV8(copy.deepcopy(net), B, hw, autotune=False, box_rows="fp32")
    want = plain(x).clone()
    side.boxes32.fill_(float("nan"))
    got = side(x).clone()
    torch.cuda.synchronize()
    assert _same(got, want)
    assert tuple(side.boxes32.shape) == (B, 4, side.A) and bool(torch.isfinite(side.boxes32).all())
    assert _same(side.boxes32.half(), got[:, :4])
    res = side.result()
    assert isinstance(res, ops.SplitHead) and res[0].data_ptr() == side.out.data_ptr()


# ------------------------------------------------------------------------------------------------ detector and pipeline
def _detector(nc, half, classes=None, scale="n"):
    cfg = DetectorConfig(model_path=f"yolov8{scale}.pt", backend="hip", model_type="yolov8", warmup=False, half=half,
                         hip_engine="auto" if half else "plan", confidence_threshold=0.25, iou_threshold=0.5, classes=classes)
    det = HipYoloDetector(cfg, net=build_detector_net(scale, seed=2, nc=nc))
    assert det.engine == ("fused" if half else "fused-f32") and det.net.nc == nc
    return det


def _calibrate(det, sample):
    """Seeded weights give every class >= 1 nearly the same logit, and one of them wins everywhere.  With three classes, shift
    the last one by the median gap at the anchors of high objectness, so that both class ids occur (a ``classes`` filter then has
    something to keep and something to drop); then the usual density calibration."""
    sample = sample.clone().contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        if det.net.nc == 3:
            _, cls = det.net(sample, raw=True)
            cls = cls.float()
            top = cls[:, 0] >= torch.quantile(cls[:, 0].flatten(), 0.95)
            gap = float((cls[:, 1] - cls[:, 2])[top].median())
            for seq in det.net.detect.cls:
                seq[-1].bias.data[2] += gap
        calibrate_detection_density(det.net, sample, 0.25, 60)
    det.invalidate_engine()


@pytest.mark.parametrize("nc,half,classes", [(1, True, None), (1, False, None), (3, True, None), (3, False, None), (3, True, [1])])
def test_detector_with_a_custom_class_count_matches_the_oracle(nc, half, classes):
    """Two 640 x 360 NV12 frames through ``predict_batch``: the Detection objects == the oracle's post-process of the head tensor
    the plan produced (for nc = 1 the reference's 5-row rule: the one class row is the score)."""
    det = _detector(nc, half, classes)
    W, H = 640, 360
    frames = [ops.Nv12Surface.from_numpy(*synth.make_nv12(40 + i, W, H), W, H) for i in range(2)]
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12(frames, (640, 640), half=half)
    _calibrate(det, sample)
    raws = []
    infer = det._infer
    det._infer = lambda t: raws.append(infer(t)) or raws[-1]
    stream = StreamConfig(name="cam", url="x")
    pkts = [FramePacket(stream=stream, frame=f, frame_id=i, timestamp=0.0) for i, f in enumerate(frames)]
    dets = det.predict_batch(pkts)
    plan = det._plans[(2, 640, 640)]
    assert isinstance(plan, FusedYoloV8) and plan.nc == nc and plan.f32 == (not half)
    head = raws[0]
    assert tuple(head.shape) == (2, 4 + nc, 8400) and head.dtype == (torch.float16 if half else torch.float32)
    total = 0
    for i in range(2):
        r = orc.postprocess(head[i].float().cpu().numpy(), 0.25, 0.5, classes, (W, H))
        assert [d.class_id for d in dets[i]] == [int(v) for v in r["cls"]], i
        assert [d.confidence for d in dets[i]] == [float(v) for v in r["conf"]], i
        assert [list(d.bbox_xyxy) for d in dets[i]] == [[float(v) for v in b] for b in r["boxes"]], i
        if classes:
            assert all(d.class_id in classes for d in dets[i])
            every = orc.postprocess(head[i].float().cpu().numpy(), 0.25, 0.5, None, (W, H))
            assert set(int(v) for v in every["cls"]) - set(classes), "the filter had nothing to drop"
        total += len(dets[i])
    assert total > 0, "the calibrated detector produced nothing"


def test_pipelined_ticks_with_a_three_class_detector_match_the_oracle_tracker():
    """Two 1080p NV12 streams, three ticks at depth 2: the track tables == the oracle's post-process + tracker on each tick's head."""
    S, T = 2, 3
    streams = [StreamConfig(name=f"cam{i}", url="synthetic://1920x1080", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    det = _detector(3, True)
    with torch.inference_mode():
        sample, _ = ops.preprocess_nv12([s._ring[0] for s in srcs], (640, 640), half=True)
    _calibrate(det, sample)
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=512)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=2, use_graph=True)
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    checked = 0

    def check(k):
        nonlocal checked
        _, tables = runner.collect()
        par = k % runner.nslots
        assert runner.nslots == runner.depth
        plan = det._plans[(S, 640, 640) if par == 0 else (S, 640, 640, par)]
        assert plan.nc == 3 and tuple(plan._outs[0].shape) == (S, 7, 8400)
        head = plan._outs[0].float().cpu().numpy()
        for s in range(S):
            r = orc.postprocess(head[s], 0.25, 0.5, None, (1920, 1080))
            m = r["conf"].astype(np.float64) >= 0.25
            want = otr.update(s, r["boxes"][m].astype(np.float64), r["conf"][m].astype(np.float64), r["cls"][m].astype(np.int64))
            assert orc.table_of(tables[s]) == orc.table_of(want), (k, s)
            checked += want["n"]
    done = 0
    for k in range(T):
        if k - done == runner.depth:
            check(done); done += 1
        runner.submit()
    while done < T:
        check(done); done += 1
    assert checked > 0
