"""The fp32 CNN-LSTM clip plan (clip_plan.FusedCnnLstm, csrc/rva_clip.hip) on the GPU: golden logits, the default 224x224
T=16 shape and an odd shape against float64, bit-reproducibility, the top-5 rule, the detector and the pipeline with
``hip_engine: plan``.  (tests/test_gpu_clip_stages.py checks every stage of the plan on its own.)

The bound on logits: torch fp32 on the CPU differs from the float64 module by 9.7e-9 / 1.5e-8 on the two goldens, 1.9e-8 on the
default shape and 1.0e-8 on the odd shape, and the logits are |.| <= 0.18.  100 times the reference's own error is 1.9e-6, so the
bound these figures allow is 1e-5; it stays at 1e-4 until the plan's own error (every test prints it, ``pytest -s``) has been
read off an MI355X, which has not happened yet."""
import copy
import logging
from collections import deque

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.clip_plan import FusedCnnLstm
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.temporal import (ClipSchedule, CnnLstmNet, HipCNN3DDetector, HipCNNLSTMDetector,
                                                             TemporalDetection)
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from tests.conftest import load_golden
from tests.helpers import temporal_net

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TOL = 1e-4


def _f64(net, x):
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(x.double().cpu()).numpy()


def _report(what, got, ref):
    err = float(np.abs(got - ref).max())
    print(f"{what}: max |plan - reference| = {err:.3e}")
    return err


def _top(v, k=5):
    return np.argsort(v, kind="stable")[-k:][::-1]


def _dcfg(**kw):
    base = dict(model_path="cnn_lstm.onnx", backend="hip", model_type="cnn_lstm", sequence_length=4, sequence_stride=2,
                temporal_overlap=0.5, confidence_threshold=-1e9, num_action_classes=400, input_size=[224, 224], warmup=False,
                half=False, hip_engine="plan")
    base.update(kw)
    return DetectorConfig(**base)


@pytest.mark.parametrize("case", [c for c in load_golden("temporal_nets.json") if c["kind"] == "cnn_lstm"],
                         ids=lambda c: f"h{c['ctor']['hidden_size']}")
def test_golden_logits_batch_1_and_2(case):
    net, x = temporal_net(case)
    B, T, _, H, W = x.shape
    want = np.asarray(case["logits"], np.float64)
    ref = _f64(net, x)
    plan = FusedCnnLstm(net, (H, W), T, 2)
    xd = x.float().to(DEV)
    one = np.concatenate([plan(xd[b:b + 1]).cpu().numpy() for b in range(B)])
    two = plan(torch.cat([xd, xd])[:2] if B == 1 else xd).cpu().numpy()[:B]
    for got in (one, two):
        assert np.abs(got - want).max() < 1e-3
        assert _report(f"golden {tuple(x.shape)}", got, ref) < TOL
    assert np.array_equal(one, two)


def test_default_shape_224_t16_8_clips_against_float64():
    net = synth.seeded_module(lambda: CnnLstmNet(400), 31)
    x = synth.seeded_clip((8, 16, 3, 224, 224), 32)
    got = FusedCnnLstm(net, (224, 224), 16, 8)(x.to(DEV)).cpu().numpy()
    ref = _f64(net, x)
    assert _report("default shape", got, ref) < TOL
    for g, r in zip(got, ref):
        s = np.sort(r)[::-1]
        if np.min(s[:5] - s[1:6]) > 1e-5:
            assert _top(g).tolist() == _top(r).tolist()


def test_odd_height_width_against_float64():
    net = synth.seeded_module(lambda: CnnLstmNet(10, 48), 61)
    x = synth.seeded_clip((2, 3, 3, 67, 131), 62)
    plan = FusedCnnLstm(net, (67, 131), 3, 2)
    assert plan.pooled_hw == (17, 33) and plan.conv2_tiles == 3
    got = plan(x.to(DEV)).cpu().numpy()
    assert _report("odd shape", got, _f64(net, x)) < TOL
    assert np.array_equal(plan(x[1:2].to(DEV)).cpu().numpy()[0], got[1])


def test_bit_reproducible_across_batch_position_graph_and_index_table():
    net = synth.seeded_module(lambda: CnnLstmNet(400), 41)
    T, H, W = 16, 224, 224
    plan = FusedCnnLstm(net, (H, W), T, 32)
    g = torch.Generator(device=DEV).manual_seed(5)
    clips = torch.randn((32, T, 3, H, W), generator=g, device=DEV)
    alone = plan(clips[5:6])
    in8 = plan(clips[:8])
    moved = plan(torch.cat([clips[5:6], clips[1:5], clips[:1], clips[6:8]]))
    in32 = plan(clips)
    assert torch.equal(alone[0], in8[5]) and torch.equal(alone[0], moved[0]) and torch.equal(alone[0], in32[5])
    for b in (8, 17, 31):                                                      # the LSTM's second and later passes of eight clips
        assert torch.equal(plan(clips[b:b + 1])[0], in32[b]), b
    assert torch.equal(plan(clips), in32)                                      # two runs
    # frames through a permuted index table == contiguous frames
    perm = torch.randperm(32 * T, generator=torch.Generator().manual_seed(9))
    ring = torch.empty_like(clips.view(-1, 3, H, W))
    ring[perm] = clips.view(-1, 3, H, W)
    idx = perm.to(torch.int32).to(DEV)
    assert torch.equal(plan.run(ring, idx, 32).clone(), in32)
    # eager == hipGraph replay
    static_idx = torch.arange(8 * T, dtype=torch.int32, device=DEV)
    src = clips[:8].contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(src, static_idx, 8)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.run(src, static_idx, 8)
    plan.logits.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:8], in8)


def _torch_rule(raw, rows, fired_rows, hw, max_det=8):
    """stage_post's torch rule (temporal.py), on the same logits."""
    post = ops.PostBuffers.allocate(rows, max_det, DEV)
    post.counts.zero_()
    k = min(5, raw.shape[1])
    order = torch.sort(raw, dim=1, stable=True).indices[:, -k:].flip(1)
    r = torch.tensor(fired_rows, device=DEV)
    post.scores[r, :k] = torch.gather(raw, 1, order)
    post.cls[r, :k] = order.to(torch.int32)
    post.boxes[r, :k] = torch.tensor([[0.0, 0.0, float(w), float(h)] for h, w in hw], device=DEV)[:, None, :]
    post.counts[r] = k
    return post


@pytest.mark.parametrize("classes", [10, 3])
def test_top5_rule_ties_k_and_empty_rows(classes):
    net = synth.seeded_module(lambda: CnnLstmNet(classes, 48), 51)
    with torch.no_grad():
        if classes == 10:                  # exact ties: rows 3 and 7 identical, and at the top
            net.head.weight[7] = net.head.weight[3]
            net.head.bias[3] = net.head.bias[7] = 5.0
            net.head.weight[1] = net.head.weight[2]
            net.head.bias[1] = net.head.bias[2]
    T, H, W = 4, 40, 56
    plan = FusedCnnLstm(net, (H, W), T, 2)
    x = synth.seeded_clip((2, T, 3, H, W), 52).to(DEV)
    logits = plan.run(x.contiguous(), torch.arange(2 * T, dtype=torch.int32, device=DEV), 2).clone()
    if classes == 10:
        assert torch.equal(logits[:, 3], logits[:, 7]) and torch.equal(logits[:, 1], logits[:, 2])
    hw = [(1080, 1920), (2160, 3840)]
    table = torch.tensor([[1, 3840, 2160], [-1, 0, 0], [0, 1920, 1080]], dtype=torch.int32, device=DEV)
    post = ops.PostBuffers.allocate(3, 8, DEV)
    post.counts.fill_(7)
    plan.post(logits, table, 3, post)
    want = _torch_rule(logits[[1, 0]], 3, [0, 2], [hw[1], hw[0]])
    k = min(5, classes)
    assert post.counts.tolist() == [k, 0, k]
    for r in (0, 2):
        assert torch.equal(post.cls[r, :k], want.cls[r, :k]) and torch.equal(post.scores[r, :k], want.scores[r, :k])
        assert torch.equal(post.boxes[r, :k], want.boxes[r, :k])
    assert post.boxes[0, 0].tolist() == [0.0, 0.0, 3840.0, 2160.0] and post.boxes[2, 0].tolist() == [0.0, 0.0, 1920.0, 1080.0]
    if classes == 10:
        c = post.cls[0, :2].tolist()
        assert c == [7, 3]                 # the larger class index first on an exact tie


def test_detector_predict_with_the_plan():
    torch.manual_seed(1)
    net = CnnLstmNet(400).eval()
    det = HipCNNLSTMDetector(_dcfg(action_classes=[f"a{i}" for i in range(400)]), net=copy.deepcopy(net))
    assert det.engine == "clip-f32"
    st = StreamConfig(name="cam", url="x")
    frames = [synth.make_nv12(40 + f, 3840, 2160, tick=f) for f in range(12)]
    fired = {}
    for f, (y, uv) in enumerate(frames):
        out = det.predict(FramePacket(st, ops.Nv12Surface.from_numpy(y, uv, 3840, 2160), f, 0.0))
        if out:
            fired[f] = out
    assert sorted(fired) == [7, 9, 11]
    plan = FusedCnnLstm(net, (224, 224), 4, 1)
    for f, ids in ((7, [0, 2, 4, 6]), (9, [2, 4, 6, 8]), (11, [4, 6, 8, 10])):
        x = np.stack([orc.preprocess_clip_frame(nv12=frames[i], wh=(3840, 2160), tw=224, th=224, half=False) for i in ids])
        want = plan(torch.from_numpy(x)[None].to(DEV)).flatten().cpu().numpy()
        top = _top(want)
        dets = fired[f]
        assert all(isinstance(d, TemporalDetection) for d in dets)
        assert [d.class_id for d in dets] == top.tolist()
        assert [d.confidence for d in dets] == [float(v) for v in want[top]]
        assert dets[0].bbox_xyxy == (0.0, 0.0, 3840.0, 2160.0) and dets[0].sequence_start_frame == ids[0]


def _run_pipeline(depth, S=4, T=16):
    streams = [StreamConfig(name=f"uhd{i}", url="synthetic://3840x2160", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=3840, height=2160, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    torch.manual_seed(1)
    net = CnnLstmNet(400).eval()
    det = HipCNNLSTMDetector(_dcfg(action_classes=[f"act{i}" for i in range(400)]), net=copy.deepcopy(net))
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=64)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    assert not runner.use_graph
    plan = FusedCnnLstm(net, (224, 224), 4, 1)
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    sched = ClipSchedule(4, 2, 0.5)
    bufs = [deque() for _ in range(S)]
    cache = {}
    out, fired_ticks = [], []

    def check(k):
        _, tables = runner.collect()
        fired_any = False
        for s in range(S):                                        # canonical order: tick-major, stream-minor
            clip, _ = sched.push(bufs[s], k)
            if clip is None:
                want = otr.update(s, np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int64))
            else:
                fired_any = True
                ring = srcs[s]._ring
                key = (s, tuple(f % len(ring) for f in clip))
                if key not in cache:
                    x = np.stack([orc.preprocess_clip_frame(nv12=(ring[f % len(ring)].y.cpu().numpy(), ring[f % len(ring)].uv.cpu().numpy()),
                                                            wh=(3840, 2160), tw=224, th=224, half=False) for f in clip])
                    cache[key] = plan(torch.from_numpy(x)[None].to(DEV)).flatten().cpu().numpy()
                v = cache[key]
                top = _top(v)
                want = otr.update(s, np.tile([0.0, 0.0, 3840.0, 2160.0], (5, 1)), v[top].astype(np.float64), top.astype(np.int64))
            assert orc.table_of(tables[s]) == orc.table_of(want), (depth, k, s)
            out.append(orc.table_of(tables[s]))
        if fired_any:
            fired_ticks.append(k)

    done = 0
    for k in range(T):
        if k - done == runner.depth:
            check(done); done += 1
        runner.submit()
    while done < T:
        check(done); done += 1
    return fired_ticks, out


def test_pipeline_depth_1_and_4_against_the_oracle():
    f1, t1 = _run_pipeline(1)
    f4, t4 = _run_pipeline(4)
    assert f1 == [7, 9, 11, 13, 15] and f4 == f1
    assert t1 == t4


def test_engine_routing(caplog):
    with pytest.raises(ValueError, match="fp32"):
        HipCNNLSTMDetector(_dcfg(half=True), net=CnnLstmNet(400))
    with caplog.at_level(logging.WARNING):
        d3 = HipCNN3DDetector(_dcfg(model_type="3d_cnn", input_size=None))
    assert d3.engine == "torch" and any("hip_engine: plan" in r.getMessage() for r in caplog.records)
    assert HipCNNLSTMDetector(_dcfg(hip_engine="auto"), net=CnnLstmNet(400)).engine == "torch"
    assert DetectorConfig().hip_engine == "auto"
    assert HipCNNLSTMDetector(_dcfg(), infer_fn=lambda x: x).engine == "infer_fn"
