"""The fp32 3D-CNN clip plan (clip_plan.Fused3dCnn, csrc/rva_clip3d.hip) on the GPU: golden logits, the default 112x112 T=16
shape and an odd shape against float64, bit-reproducibility, the top-5 rule, the detector and the pipeline with
``hip_engine: native``, the routing of the strict engine value, and both detectors of the sample YAML in one pipeline.

The 1e-5 bound on logits: torch fp32 on the CPU differs from the float64 module by 4.8e-8 / 5.9e-8 / 5.3e-8 on the two goldens
and the default shape, and the logits are |.| <= 0.37 -- so 1e-5 is more than 150 times the reference's own error, and 30 times
below the smallest top-6 gap of the default-shape clips used here (3.0e-4 on seeds 31 / 33, all eight clips above 1e-4)."""
import copy
import dataclasses
import logging
from collections import deque
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.classify import HipResNetDetector
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnn
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig, load_config
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.temporal import (ClipSchedule, Cnn3dNet, CnnLstmNet, HipCNN3DDetector, HipCNNLSTMDetector,
                                                             HipConvGRUDetector, TemporalDetection)
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from tests.conftest import load_golden
from tests.helpers import temporal_net

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
TOL = 1e-5


def _f64(net, x):
    with torch.inference_mode():
        return copy.deepcopy(net).double().eval()(x.double().cpu()).numpy()


def _top(v, k=5):
    return np.argsort(v, kind="stable")[-k:][::-1]


def _dcfg(**kw):
    base = dict(model_path="c3d.onnx", backend="hip", model_type="3d_cnn", sequence_length=4, sequence_stride=1,
                temporal_overlap=0.25, confidence_threshold=-1e9, num_action_classes=400, input_size=[112, 112], warmup=False,
                half=False, hip_engine="native")
    base.update(kw)
    return DetectorConfig(**base)


def _report(what, got, ref):
    err = float(np.abs(got - ref).max())
    print(f"{what}: max |plan - reference| = {err:.3e}")
    return err


@pytest.mark.parametrize("case", [c for c in load_golden("temporal_nets.json") if c["kind"] == "3d_cnn"],
                         ids=lambda c: f"c{c['ctor']['num_classes']}")
def test_golden_logits_batch_1_and_2(case):
    net, x = temporal_net(case)
    B, _, T, H, W = x.shape
    want = np.asarray(case["logits"], np.float64)
    plan = Fused3dCnn(net, (H, W), T, 2)
    assert plan.pool1 == (T, H // 2, W // 2) and plan.pool2 == (T // 2, H // 4, W // 4) and plan.n_launches == 5
    xd = x.float().to(DEV)
    one = np.concatenate([plan(xd[b:b + 1]).cpu().numpy() for b in range(B)])
    two = plan(torch.cat([xd, xd])[:2] if B == 1 else xd).cpu().numpy()[:B]
    for got in (one, two):
        assert _report(f"golden {tuple(x.shape)}", got, want) < TOL
    assert np.array_equal(one, two)


def test_default_shape_112_t16_8_clips_against_float64():
    net = synth.seeded_module(lambda: Cnn3dNet(400), 31)
    x = synth.seeded_clip((8, 3, 16, 112, 112), 33)
    got = Fused3dCnn(net, (112, 112), 16, 8)(x.to(DEV)).cpu().numpy()
    ref = _f64(net, x)
    assert _report("default shape", got, ref) < TOL
    clear = [bool(np.min(np.sort(r)[::-1][:5] - np.sort(r)[::-1][1:6]) > 1e-4) for r in ref]
    assert sum(clear) >= 7
    for g, r, ok in zip(got, ref, clear):
        if ok:
            assert _top(g).tolist() == _top(r).tolist()


def test_odd_height_width_and_frames_against_float64():
    net = synth.seeded_module(lambda: Cnn3dNet(10), 61)
    x = synth.seeded_clip((2, 3, 7, 25, 41), 62)
    plan = Fused3dCnn(net, (25, 41), 7, 2)
    assert plan.pool1 == (7, 12, 20) and plan.pool2 == (3, 6, 10)
    got = plan(x.to(DEV)).cpu().numpy()
    assert _report("odd shape", got, _f64(net, x)) < TOL
    assert np.array_equal(plan(x[1:2].to(DEV)).cpu().numpy()[0], got[1])


def test_bit_reproducible_across_batch_position_graph_and_index_table():
    net = synth.seeded_module(lambda: Cnn3dNet(400), 41)
    T, H, W = 16, 112, 112
    plan = Fused3dCnn(net, (H, W), T, 32)
    g = torch.Generator(device=DEV).manual_seed(5)
    frames = torch.randn((32, T, 3, H, W), generator=g, device=DEV)           # the ring's layout: planar frames
    iota = torch.arange(32 * T, dtype=torch.int32, device=DEV)

    def run(fr):
        return plan.run(fr.contiguous(), iota, fr.shape[0]).clone()

    alone = run(frames[5:6])
    in8 = run(frames[:8])
    moved = run(torch.cat([frames[5:6], frames[1:5], frames[:1], frames[6:8]]))
    in32 = run(frames)
    assert torch.equal(alone[0], in8[5]) and torch.equal(alone[0], moved[0]) and torch.equal(alone[0], in32[5])
    assert torch.equal(run(frames), in32)                                      # two runs
    # the module's layout through __call__ == frames through run
    assert torch.equal(plan(frames[:8].permute(0, 2, 1, 3, 4)), in8)
    # frames through a permuted index table == contiguous frames (temporal neighbours come from the table, not the ring)
    perm = torch.randperm(32 * T, generator=torch.Generator().manual_seed(9))
    ring = torch.empty_like(frames.view(-1, 3, H, W))
    ring[perm] = frames.view(-1, 3, H, W)
    idx = perm.to(torch.int32).to(DEV)
    assert torch.equal(plan.run(ring, idx, 32).clone(), in32)
    # eager == hipGraph replay
    static_idx = torch.arange(8 * T, dtype=torch.int32, device=DEV)
    src = frames[:8].contiguous()
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
    net = synth.seeded_module(lambda: Cnn3dNet(classes), 51)
    with torch.no_grad():
        if classes == 10:                  # exact ties: rows 3 and 7 identical, and at the top
            net.fc.weight[7] = net.fc.weight[3]
            net.fc.bias[3] = net.fc.bias[7] = 5.0
            net.fc.weight[1] = net.fc.weight[2]
            net.fc.bias[1] = net.fc.bias[2]
    T, H, W = 4, 20, 28
    plan = Fused3dCnn(net, (H, W), T, 2)
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
        assert post.cls[0, :2].tolist() == [7, 3]                 # the larger class index first on an exact tie


def test_create_refuses_empty_pools_and_oversized_workspaces():
    net = synth.seeded_module(lambda: Cnn3dNet(10), 71)
    for hw, frames in (((3, 40), 4), ((40, 3), 4), ((40, 40), 1)):
        with pytest.raises(RuntimeError, match="bad descriptor"):
            Fused3dCnn(net, hw, frames, 1)
    with pytest.raises(RuntimeError, match="free"):                # 2040 clips of 32 x 256 x 256: 134 MB of first activation each
        Fused3dCnn(net, (256, 256), 32, 2040)


def test_detector_predict_with_the_plan():
    torch.manual_seed(1)
    net = Cnn3dNet(400).eval()
    det = HipCNN3DDetector(_dcfg(action_classes=[f"a{i}" for i in range(400)]), net=copy.deepcopy(net))
    assert det.engine == "clip3d-f32"
    st = StreamConfig(name="cam", url="x")
    frames = [synth.make_nv12(40 + f, 3840, 2160, tick=f) for f in range(10)]
    fired = {}
    for f, (y, uv) in enumerate(frames):
        out = det.predict(FramePacket(st, ops.Nv12Surface.from_numpy(y, uv, 3840, 2160), f, 0.0))
        if out:
            fired[f] = out
    assert sorted(fired) == [3, 6, 9]                                         # need = 4 frames, step = int(4 * 0.75) = 3
    plan = Fused3dCnn(net, (112, 112), 4, 1)
    iota = torch.arange(4, dtype=torch.int32, device=DEV)
    for f, ids in ((3, [0, 1, 2, 3]), (6, [3, 4, 5, 6]), (9, [6, 7, 8, 9])):
        x = orc.preprocess_norm_frames([frames[i] for i in ids], 112, 112, N.NORM_VIDEO_F32, 1, layout=0, nv12_wh=(3840, 2160))
        want = plan.run(torch.from_numpy(x).to(DEV), iota, 1).flatten().cpu().numpy()
        top = _top(want)
        dets = fired[f]
        assert all(isinstance(d, TemporalDetection) for d in dets)
        assert [d.class_id for d in dets] == top.tolist()
        assert [d.action_label for d in dets] == [f"a{c}" for c in top]
        assert [d.confidence for d in dets] == [float(v) for v in want[top]]
        assert all(d.bbox_xyxy == (0.0, 0.0, 3840.0, 2160.0) for d in dets)
        assert all((d.sequence_start_frame, d.sequence_end_frame, d.frame_id) == (ids[0], ids[-1], ids[-1]) for d in dets)


def _run_pipeline(depth, S=4, T=10):
    streams = [StreamConfig(name=f"uhd{i}", url="synthetic://3840x2160", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=3840, height=2160, n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    torch.manual_seed(1)
    net = Cnn3dNet(400).eval()
    det = HipCNN3DDetector(_dcfg(action_classes=[f"act{i}" for i in range(400)]), net=copy.deepcopy(net))
    assert det.engine == "clip3d-f32"
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=64)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    assert not runner.use_graph
    plan = Fused3dCnn(net, (112, 112), 4, 1)
    iota = torch.arange(4, dtype=torch.int32, device=DEV)
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    sched = ClipSchedule(4, 1, 0.25)
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
                    nv12 = [(ring[f % len(ring)].y.cpu().numpy(), ring[f % len(ring)].uv.cpu().numpy()) for f in clip]
                    x = orc.preprocess_norm_frames(nv12, 112, 112, N.NORM_VIDEO_F32, 1, layout=0, nv12_wh=(3840, 2160))
                    cache[key] = plan.run(torch.from_numpy(x).to(DEV), iota, 1).flatten().cpu().numpy()
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
    assert f1 == [3, 6, 9] and f4 == f1
    assert t1 == t4


def test_engine_routing(caplog):
    for m in ("3d_cnn", "slow_fast"):
        assert HipCNN3DDetector(_dcfg(model_type=m, input_size=None)).engine == "clip3d-f32"
        with pytest.raises(ValueError, match="fp32 plan only"):
            HipCNN3DDetector(_dcfg(model_type=m, half=True))
    lstm = dict(model_type="cnn_lstm", input_size=[224, 224])
    assert HipCNNLSTMDetector(_dcfg(**lstm), net=CnnLstmNet(400)).engine == "clip-f32"
    with pytest.raises(ValueError, match="fp32 plan only"):
        HipCNNLSTMDetector(_dcfg(half=True, **lstm), net=CnnLstmNet(400))
    with pytest.raises(ValueError, match="no architecture"):
        HipConvGRUDetector(_dcfg(model_type="conv_gru"), net=torch.nn.Identity())
    with pytest.raises(ValueError, match="no hand-written plan"):
        HipResNetDetector(_dcfg(model_type="resnet", input_size=[224, 224]))
    # an infer_fn wins over every rule
    assert HipCNN3DDetector(_dcfg(half=True), infer_fn=lambda x: x).engine == "infer_fn"
    assert HipConvGRUDetector(_dcfg(model_type="conv_gru"), infer_fn=lambda x: x).engine == "infer_fn"
    HipResNetDetector(_dcfg(model_type="resnet", input_size=[224, 224]), infer_fn=lambda x: x)
    # plan keeps its meaning: best effort, PyTorch-ROCm with a warning
    with caplog.at_level(logging.WARNING):
        d3 = HipCNN3DDetector(_dcfg(hip_engine="plan"))
    assert d3.engine == "torch" and any("hip_engine: plan" in r.getMessage() and "3d_cnn" in r.getMessage() for r in caplog.records)
    assert HipCNN3DDetector(_dcfg(hip_engine="auto")).engine == "torch"


def test_both_detectors_of_the_sample_yaml_on_native_in_one_pipeline():
    cfg = load_config(Path(__file__).resolve().parent / "golden" / "sample-temporal-pipeline.yaml")
    streams = [s for s in cfg.streams if s.enabled]
    assert [s.detector_id for s in streams] == ["temporal_cnn_lstm", "temporal_3d_cnn"]
    dets = []
    for s, cls in zip(streams, (HipCNNLSTMDetector, HipCNN3DDetector)):
        d = dataclasses.replace(cfg.detector_for(s), backend="hip", hip_engine="native", confidence_threshold=-1e9, warmup=False)
        dets.append(cls(d))
    assert [d.engine for d in dets] == ["clip-f32", "clip3d-f32"]
    assert dets[1].input_hw == (112, 112) and (dets[1].sched.need, dets[1].sched.step) == (16, 12)
    srcs = [SyntheticNv12Stream(s, index=i, width=3840, height=2160, n_unique=2) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=2, capacity=64)
    pipe = TickPipeline(streams, dets, trk, sources=srcs)
    first = {}                                # tick at which a stream's first clip left tracks (none exist before it)
    for k in range(32):                       # CNN-LSTM: 16 frames at stride 2 -> tick 31; 3D-CNN: 16 frames -> tick 15
        res = pipe.tick()
        for name, tracks in res.tracks.items():
            if tracks:
                first.setdefault(name, k)
    assert first == {streams[0].name: 31, streams[1].name: 15}
    assert len(res.tracks[streams[0].name]) == 5
    assert all(type(d._plans[0].plan).__name__ == n for d, n in zip(dets, ("FusedCnnLstm", "Fused3dCnn")))
