"""The fp16 3D-CNN clip plan (clip_plan.Fused3dCnnF16, csrc/rva_clip3d.hip, engine ``clip3d-f16``) on the GPU: golden, odd and
ragged logits against the float64 quantised network and the original module, bit-reproducibility, the top-5 rule, the create
refusals, the detector and the pipeline with ``half: true`` + ``hip_engine: native`` + ``hip_clip_fp16: true``, the unchanged
routing of every neighbouring combination, and the sample YAML's ``slow_fast`` section (256 x 256, T = 32).

Tolerances (tests/clip3d_f16_refs.py; measured in float64 on the CPU, tests/test_clip3d_f16_host.py prints them): fp16 storage of
act1 / act2 alone moves these logits by 2.9e-6 .. 6.2e-6 -- TOL_Q = 2.5e-5 is 4 x the largest; weight and input rounding moves
them by up to 4.9e-5 -- TOL_O = 2e-4 is 4 x that; both lie below the smallest top-(k+1) gap of these cases (3.2e-4)."""
import copy
import ctypes as C
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
from realtime_video_analytics_32streams_amd.clip_plan import Fused3dCnn, Fused3dCnnF16, pack_cnn3d
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig, load_config
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.temporal import (ClipSchedule, Cnn3dNet, CnnLstmNet, HipCNN3DDetector, HipCNNLSTMDetector,
                                                             TemporalDetection)
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from tests import clip3d_f16_refs as Q

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _dcfg(**kw):
    base = dict(model_path="c3d.onnx", backend="hip", model_type="3d_cnn", sequence_length=4, sequence_stride=1,
                temporal_overlap=0.25, confidence_threshold=-1e9, num_action_classes=400, input_size=[112, 112], warmup=False,
                half=True, hip_engine="native", hip_clip_fp16=True)
    base.update(kw)
    return DetectorConfig(**base)


def _err(what, got, ref):
    e = float(np.abs(got - ref).max())
    print(f"{what}: {e:.3e}")
    return e


@pytest.mark.parametrize("name", Q.E2E_NAMES)
def test_logits_against_the_quantised_network_and_the_original_module(name):
    net, x, quant, _, orig, recorded = Q.e2e(name)
    B, _, T, H, W = x.shape
    plan = Fused3dCnnF16(net, (H, W), T, 8 if name == "ragged" else B)
    assert plan.pool1 == (T, H // 2, W // 2) and plan.pool2 == (T // 2, H // 4, W // 4) and plan.n_launches == 5
    got = plan(x.to(DEV)).cpu().numpy()
    assert got.dtype == np.float32
    assert np.array_equal(plan(x.half().to(DEV)).cpu().numpy(), got)          # fp32 clips are rounded exactly as .half() does
    eq = _err(f"{name}: |plan - quantised float64 network| (TOL_Q {Q.TOL_Q:.1e})", got, quant)
    eo = _err(f"{name}: |plan - original float64 module| (TOL_O {Q.TOL_O:.1e})", got, orig)
    er = _err(f"{name}: |plan - recorded golden logits|", got, recorded) if recorded is not None else 0.0
    assert eq < Q.TOL_Q
    assert eo < Q.TOL_O and er < Q.TOL_O
    for g, q in zip(got, quant):
        assert Q.top(g).tolist() == Q.top(q).tolist()


def test_bit_reproducible_across_batch_position_graph_and_call():
    net, x, *_ = Q.e2e("ragged")
    B, _, T, H, W = x.shape
    plan = Fused3dCnnF16(net, (H, W), T, 8)
    frames = x.half().to(DEV).permute(0, 2, 1, 3, 4).contiguous()               # the ring's layout: planar frames [6, T, 3, H, W]
    iota = torch.arange(8 * T, dtype=torch.int32, device=DEV)

    def run(fr):
        return plan.run(fr.contiguous(), iota, fr.shape[0]).clone()

    alone = run(frames[4:5])
    full = run(frames)
    moved = run(torch.cat([frames[4:5], frames[1:4], frames[:1], frames[5:6]]))
    eight = run(torch.cat([frames, frames[:2]]))                               # the full capacity
    assert torch.equal(alone[0], full[4]) and torch.equal(alone[0], moved[0]) and torch.equal(eight[:6], full)
    assert torch.equal(eight[6:], full[:2])
    assert torch.equal(run(frames), full)                                      # two runs
    assert torch.equal(plan(x.to(DEV)), full) and torch.equal(plan(x.half().to(DEV)), full)
    src = frames.contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(src, iota, B)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.run(src, iota, B)
    plan.logits.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:B], full)


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
    plan = Fused3dCnnF16(net, (H, W), T, 2)
    x = synth.seeded_clip((2, T, 3, H, W), 52).half().to(DEV)
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
    if classes == 10:
        assert post.cls[0, :2].tolist() == [7, 3]                 # the larger class index first on an exact tie


def test_create_refuses_empty_pools_oversized_workspaces_and_weights_beyond_fp16():
    net = synth.seeded_module(lambda: Cnn3dNet(10), 71)
    for hw, frames in (((3, 40), 4), ((40, 3), 4), ((40, 40), 1)):
        with pytest.raises(RuntimeError, match="bad descriptor"):
            Fused3dCnnF16(net, hw, frames, 1)
    with pytest.raises(RuntimeError, match="free"):                # 2040 clips of 32 x 512 x 512: 268 MB of fp16 first activation each
        Fused3dCnnF16(net, (512, 512), 32, 2040)
    # the C entry's own check (the Python packer refuses earlier): an fp32 weight that fp16 cannot hold names its array
    packed = {k: v.copy() for k, v in pack_cnn3d(net, half=True).items()}
    packed["conv3_w"][7, 3, 5] = 7e4
    ctx = ops.context()
    wt = N.Cnn3dWeights(*[packed[n].ctypes.data_as(C.POINTER(C.c_float)) for n in N.Cnn3dWeights.NAMES])
    h = C.c_void_p()
    rc = N.lib().rva_cnn3d_f16_plan_create(ctx.handle, C.byref(N.Cnn3dDesc(16, 16, 2, 10, 1)), C.byref(wt), C.byref(h))
    assert rc == N.RVA_ERR_ARG and not h and b"conv3_w" in N.lib().rva_last_error(ctx.handle)


def test_detector_predict_rounds_the_weights_once():
    torch.manual_seed(1)
    net = Cnn3dNet(400).eval()
    det = HipCNN3DDetector(_dcfg(action_classes=[f"a{i}" for i in range(400)]), net=copy.deepcopy(net))
    assert det.engine == "clip3d-f16"
    st = StreamConfig(name="cam", url="x")
    frames = [synth.make_nv12(40 + f, 3840, 2160, tick=f) for f in range(10)]
    fired = {}
    for f, (y, uv) in enumerate(frames):
        out = det.predict(FramePacket(st, ops.Nv12Surface.from_numpy(y, uv, 3840, 2160), f, 0.0))
        if out:
            fired[f] = out
    assert sorted(fired) == [3, 6, 9]                                         # need = 4 frames, step = int(4 * 0.75) = 3
    assert type(det._seq_plan).__name__ == "Fused3dCnnF16"
    plan = Fused3dCnnF16(net, (112, 112), 4, 1)                               # an fp32 copy of the net: one rounding of the weights
    iota = torch.arange(4, dtype=torch.int32, device=DEV)
    for f, ids in ((3, [0, 1, 2, 3]), (6, [3, 4, 5, 6]), (9, [6, 7, 8, 9])):
        x = orc.preprocess_norm_frames([frames[i] for i in ids], 112, 112, N.NORM_VIDEO_F32, 0, layout=0, nv12_wh=(3840, 2160))
        assert x.dtype == np.float16
        want = plan.run(torch.from_numpy(x).to(DEV), iota, 1).flatten().cpu().numpy()
        top = Q.top(want)
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
    assert det.engine == "clip3d-f16"
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=64)
    runner = PipelinedTicks(TickPipeline(streams, det, trk, sources=srcs), depth=depth)
    assert not runner.use_graph
    plan = Fused3dCnnF16(net, (112, 112), 4, 1)
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
                    x = orc.preprocess_norm_frames(nv12, 112, 112, N.NORM_VIDEO_F32, 0, layout=0, nv12_wh=(3840, 2160))
                    cache[key] = plan.run(torch.from_numpy(x).to(DEV), iota, 1).flatten().cpu().numpy()
                v = cache[key]
                top = Q.top(v)
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
    assert type(det._plans[0].plan).__name__ == "Fused3dCnnF16"
    return fired_ticks, out


def test_pipeline_depth_1_and_4_against_the_oracle():
    f1, t1 = _run_pipeline(1)
    f4, t4 = _run_pipeline(4)
    assert f1 == [3, 6, 9] and f4 == f1
    assert t1 == t4


def test_routing_of_every_neighbouring_combination_is_unchanged(caplog):
    for m in ("3d_cnn", "slow_fast"):
        assert HipCNN3DDetector(_dcfg(model_type=m, input_size=None)).engine == "clip3d-f16"
        with pytest.raises(ValueError, match="fp32 plan only"):                      # without the key half: true is still refused
            HipCNN3DDetector(_dcfg(model_type=m, hip_clip_fp16=False))
        for key in (False, True):                                                     # half: false: the key has no effect
            d = HipCNN3DDetector(_dcfg(model_type=m, half=False, hip_clip_fp16=key))
            assert d.engine == "clip3d-f32" and type(d._make_plan(1)) is Fused3dCnn
    lstm = dict(model_type="cnn_lstm", input_size=[224, 224])
    with pytest.raises(ValueError, match="fp32 plan only"):
        HipCNNLSTMDetector(_dcfg(**lstm), net=CnnLstmNet(400))
    assert HipCNNLSTMDetector(_dcfg(half=False, **lstm), net=CnnLstmNet(400)).engine == "clip-f32"
    assert HipCNN3DDetector(_dcfg(), infer_fn=lambda x: x).engine == "infer_fn"
    with caplog.at_level(logging.WARNING):
        d3 = HipCNN3DDetector(_dcfg(hip_engine="plan"))
    assert d3.engine == "torch" and any("hip_engine: plan" in r.getMessage() for r in caplog.records)
    auto = HipCNN3DDetector(_dcfg(hip_engine="auto"))
    assert auto.engine == "torch" and next(auto.net.parameters()).dtype == torch.float16 and auto._net_f32 is None


def test_the_sample_yaml_slowfast_section_runs_on_the_fp16_plan():
    cfg = load_config(Path(__file__).resolve().parent / "golden" / "sample-temporal-pipeline.yaml")
    sec = cfg.detectors["temporal_slowfast"]
    assert sec.half is True and sec.model_type == "slow_fast"
    det = HipCNN3DDetector(dataclasses.replace(sec, backend="hip", hip_engine="native", hip_clip_fp16=True, warmup=False))
    assert det.engine == "clip3d-f16" and det.input_hw == (256, 256) and det.sched.need == 64 and det.sched.L == 32
    plan = det._make_plan(2)
    assert type(plan) is Fused3dCnnF16 and (plan.H, plan.W, plan.T) == (256, 256, 32)
    assert plan.pool1 == (32, 128, 128) and plan.pool2 == (16, 64, 64)
    g = torch.Generator(device=DEV).manual_seed(3)
    clip = torch.randn((1, 32, 3, 256, 256), generator=g, device=DEV).half()
    other = torch.randn((1, 32, 3, 256, 256), generator=g, device=DEV).half()
    iota = torch.arange(64, dtype=torch.int32, device=DEV)
    a = plan.run(torch.cat([clip, other]).contiguous(), iota, 2).clone()
    b = plan.run(torch.cat([other, clip]).contiguous(), iota, 2).clone()
    assert a.shape == (2, 400) and bool(torch.isfinite(a).all())
    assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0])
