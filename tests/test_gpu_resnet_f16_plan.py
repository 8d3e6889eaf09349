"""The fp16 ResNet-18 plan (resnet_plan.FusedResNet18F16, csrc/rva_resnet_f16.hip, engine ``resnet-f16``) on the GPU: logits end
to end against the float64 quantised network and the original float64 module, bit-reproducibility, the create refusals, the
detector's routing with ``half: true`` + ``hip_engine: plan`` / ``native`` + ``hip_resnet_fp16: true`` (and every neighbouring
combination unchanged), ``predict_batch`` and both tick runners against the oracle.

TOL_Q / TOL_O and the end-to-end cases are those of tests/resnet_f16_refs.py (4 x the float64 emulation's distance, measured on
the CPU by tests/test_resnet_f16_host.py); the top-5 is compared on every frame whose quantised top-6 gap exceeds 2 TOL_Q, and at
least ``need`` frames per case must be that clear."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from realtime_video_analytics_32streams_amd import _native as N
from realtime_video_analytics_32streams_amd import ops, synth
from realtime_video_analytics_32streams_amd.classify import HipResNetDetector, ResNet18
from realtime_video_analytics_32streams_amd.config import DetectorConfig, StreamConfig, TrackerConfig
from realtime_video_analytics_32streams_amd.pipeline import PipelinedTicks, TickPipeline
from realtime_video_analytics_32streams_amd.resnet_plan import FusedResNet18, FusedResNet18F16, pack_resnet18
from realtime_video_analytics_32streams_amd.tracker import IouTracker
from realtime_video_analytics_32streams_amd.video_stream import FramePacket, SyntheticNv12Stream
from tests import resnet_f16_refs as Q

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _dcfg(**kw):
    base = dict(model_path="resnet.onnx", backend="hip", model_type="resnet", confidence_threshold=-1e9, resnet_num_classes=50,
                resnet_top_k=3, input_size=[64, 64], warmup=False, half=True, hip_engine="plan", hip_resnet_fp16=True)
    base.update(kw)
    return DetectorConfig(**base)


@pytest.mark.parametrize("case,need", list(zip(Q.E2E_CASES, Q.NEED)), ids=lambda c: "x".join(str(v) for v in c[:4]) if isinstance(c, tuple) else str(c))
def test_logits_against_the_quantised_network_and_the_original_module(case, need):
    B, H, W, classes = case[:4]
    net, x, quant, emu, orig = Q.e2e(case)
    got = FusedResNet18F16(net, (H, W), B)(x.to(DEV)).cpu().numpy().astype(np.float64)
    dq, do = float(np.abs(got - quant).max()), float(np.abs(got - orig).max())
    gaps = Q.top_gaps(quant)
    print(f"{case}: |plan - quantised| {dq:.3e} (TOL_Q {Q.TOL_Q:.1e}), |plan - original| {do:.3e} (TOL_O {Q.TOL_O:.1e}), "
          f"|plan - emulation| {float(np.abs(got - emu).max()):.3e}, top-6 gaps {' '.join(f'{g:.1e}' for g in gaps)}")
    assert dq <= Q.TOL_Q
    assert do <= Q.TOL_O
    clear = [g > 2 * Q.TOL_Q for g in gaps]
    assert sum(clear) >= need
    for g, q, ok in zip(got, quant, clear):
        if ok:
            assert Q.top(g).tolist() == Q.top(q).tolist()


def test_bit_reproducible_across_batch_position_and_graph():
    net = synth.seeded_module(lambda: ResNet18(100), 41)
    H = W = 224
    plan = FusedResNet18F16(net, (H, W), 32)
    fp32 = FusedResNet18(net, (H, W), 32)
    print(f"workspace: fp16 plan {plan.workspace_bytes >> 20} MB, fp32 plan {fp32.workspace_bytes >> 20} MB")
    assert 100 << 20 < plan.workspace_bytes < 0.55 * fp32.workspace_bytes
    del fp32
    g = torch.Generator(device=DEV).manual_seed(5)
    frames = torch.randn((32, 3, H, W), generator=g, device=DEV).half()
    iota = torch.arange(32, dtype=torch.int32, device=DEV)

    def run(fr):
        return plan.run(fr.contiguous(), iota, fr.shape[0]).clone()

    alone = run(frames[5:6])
    in8 = run(frames[:8])
    moved = run(torch.cat([frames[5:6], frames[1:5], frames[:1], frames[6:8]]))
    in32 = run(frames)
    assert bool(torch.isfinite(in32).all()) and bool((in32 != 0).any())
    assert torch.equal(alone[0], in8[5]) and torch.equal(alone[0], moved[0]) and torch.equal(alone[0], in32[5])
    assert torch.equal(run(frames), in32)                                      # two runs
    assert torch.equal(plan(frames[:8]), in8)
    assert torch.equal(plan(frames[:8].float()), in8)                          # fp32 frames are rounded to fp16 (exact here)
    # eager == one hipGraph replay on a single stream
    src = frames[:8].contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(src, iota, 8)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.run(src, iota, 8)
    plan.logits.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:8], in8)
    with pytest.raises(ValueError, match="fp16"):                              # the ring's type is checked, not converted
        plan.run(src.float(), iota, 8)


def test_create_refusals():
    net = synth.seeded_module(lambda: ResNet18(10), 71)
    for hw in ((0, 40), (40, 0)):
        with pytest.raises(RuntimeError, match="bad descriptor"):
            FusedResNet18F16(net, hw, 1)
    with pytest.raises(RuntimeError, match="bad descriptor"):
        FusedResNet18F16(net, (40, 40), 1, top_k=0)
    with pytest.raises(RuntimeError, match="free"):                # 65000 frames of 448 x 448: 14 MB of activations each
        FusedResNet18F16(net, (448, 448), 65000)
    bad = ResNet18(10)
    bad.fc = torch.nn.Linear(256, 10)
    with pytest.raises(ValueError, match="not the ResNet18 architecture"):
        FusedResNet18F16(bad, (40, 40), 1)
    big = copy.deepcopy(net)
    with torch.no_grad():
        big.layers[3].c1.weight[3, 5, 1, 1] = 1e6
    with pytest.raises(ValueError, match="c7_w"):                  # the Python packer refuses before the device is touched
        FusedResNet18F16(big, (40, 40), 1)
    # the C entry's own checks: an fp32 weight that fp16 cannot hold names its array; a missing array
    ctx = ops.context()
    fn = N.lib().rva_resnet_f16_plan_create
    desc = N.ResNetDesc(40, 40, 10, 5, 1)
    names = N.ResNetWeights.NAMES
    for name, at, said in (("stem_w", 11, b"stem_w"), ("c0_w", 7, b"conv[0].w"), ("c6_w", 3, b"conv[6].w"), ("c18_w", 5, b"conv[18].w")):
        packed = {k: v.copy() for k, v in pack_resnet18(net, half=True).items()}
        packed[name].reshape(-1)[at] = 7e4
        wt = N.ResNetWeights(*[packed[n].ctypes.data_as(C.POINTER(C.c_float)) for n in names])
        h = C.c_void_p()
        assert fn(ctx.handle, C.byref(desc), C.byref(wt), C.byref(h)) == N.RVA_ERR_ARG and not h
        err = N.lib().rva_last_error(ctx.handle)
        assert said in err and b"fp16" in err, err
    packed = pack_resnet18(net, half=True)
    wt = N.ResNetWeights(*[packed[n].ctypes.data_as(C.POINTER(C.c_float)) for n in names])
    wt.c18_w = None
    h = C.c_void_p()
    assert fn(ctx.handle, C.byref(desc), C.byref(wt), C.byref(h)) == N.RVA_ERR_ARG and not h
    assert b"required" in N.lib().rva_last_error(ctx.handle)


def test_engine_routing():
    for eng in ("plan", "native"):
        d = HipResNetDetector(_dcfg(hip_engine=eng))
        assert d.engine == "resnet-f16" and type(d._make_plan(1)) is FusedResNet18F16
        assert next(d.net.parameters()).dtype == torch.float32                 # the plan rounds the fp32 parameters once
    # every other combination behaves as before the key existed
    for key in (False, True):
        assert HipResNetDetector(_dcfg(hip_engine="auto", hip_resnet_fp16=key)).engine == "torch"
        assert HipResNetDetector(_dcfg(hip_engine="auto", half=False, hip_resnet_fp16=key)).engine == "torch"
        d = HipResNetDetector(_dcfg(hip_engine="plan", half=False, hip_resnet_fp16=key))
        assert d.engine == "resnet-f32" and type(d._make_plan(1)) is FusedResNet18
        with pytest.raises(ValueError, match="no hand-written plan"):
            HipResNetDetector(_dcfg(hip_engine="native", half=False, hip_resnet_fp16=key))
        for e in ("auto", "plan", "native"):
            for half in (False, True):
                assert HipResNetDetector(_dcfg(hip_engine=e, half=half, hip_resnet_fp16=key), infer_fn=lambda x: x).engine == "infer_fn"
    d = HipResNetDetector(_dcfg(hip_engine="plan", hip_resnet_fp16=False))     # half: true without the key: no effect on this head
    assert d.engine == "resnet-f32" and type(d._make_plan(1)) is FusedResNet18
    with pytest.raises(ValueError, match="no hand-written plan"):
        HipResNetDetector(_dcfg(hip_engine="native", hip_resnet_fp16=False))
    for key in ("hip_lstm_fp16", "hip_clip_fp16"):                             # the other heads' keys do nothing here
        assert HipResNetDetector(_dcfg(hip_resnet_fp16=False, **{key: True})).engine == "resnet-f32"


def _net():
    return synth.seeded_module(lambda: ResNet18(50), 61)


def _logits_of(plan, nv12, wh):
    x = orc.preprocess_norm_frames(nv12, 64, 64, N.NORM_IMAGENET_F32, 0, layout=0, nv12_wh=wh)
    assert x.dtype == np.float16
    return plan(torch.from_numpy(x).to(DEV)).cpu().numpy()


def test_predict_batch_is_the_host_rule_on_the_plans_logits():
    net = _net()
    det = HipResNetDetector(_dcfg(), net=copy.deepcopy(net))
    assert det.engine == "resnet-f16"
    st = StreamConfig(name="cam", url="x")
    nv12 = [synth.make_nv12(40 + f, 640, 360, tick=f) for f in range(3)]
    packets = [FramePacket(st, ops.Nv12Surface.from_numpy(y, uv, 640, 360), f, 0.0) for f, (y, uv) in enumerate(nv12)]
    out = det.predict_batch(packets)
    assert type(det._host_plan) is FusedResNet18F16
    want = _logits_of(FusedResNet18F16(net, (64, 64), 3), nv12, (640, 360))
    for f, dets in enumerate(out):
        top = Q.top(want[f], 3)
        assert [d.class_id for d in dets] == top.tolist()
        assert [d.confidence for d in dets] == [float(v) for v in want[f][top]]
        assert all(d.bbox_xyxy == (0.0, 0.0, 640.0, 360.0) and d.frame_id == f for d in dets)
    assert [d.class_id for d in det.predict(packets[1])] == Q.top(want[1], 3).tolist()
    hi = HipResNetDetector(_dcfg(confidence_threshold=1e9), net=copy.deepcopy(net))
    assert hi.predict(packets[0]) == []


def _sources(S, wh=(640, 360)):
    streams = [StreamConfig(name=f"cam{i}", url=f"synthetic://{wh[0]}x{wh[1]}", warmup_seconds=0.0) for i in range(S)]
    srcs = [SyntheticNv12Stream(s, index=i, width=wh[0], height=wh[1], n_unique=3) for i, s in enumerate(streams)]
    for s in srcs:
        s.open_sync()
    return streams, srcs


def _run_ticks(engine, depth, S=4, T=6):
    """Tracker tables of T ticks, each checked against orc.Tracker fed the host rule on the logits of one frame alone (the plan is
    bit-identical for every batch size).  ``depth``: 0 = TickPipeline.tick."""
    streams, srcs = _sources(S)
    net = _net()
    det = HipResNetDetector(_dcfg(hip_engine=engine), net=copy.deepcopy(net))
    assert det.engine == "resnet-f16"
    tcfg = TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1)
    trk = IouTracker(tcfg, max_streams=S, capacity=64)
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    ref_plan = FusedResNet18F16(net, (64, 64), 1)
    otr = orc.Tracker(S, tcfg.max_age, tcfg.max_iou_distance, tcfg.min_hits)
    cache, out = {}, []

    def check(k, tables):
        for s in range(S):                                        # canonical order: tick-major, stream-minor
            key = (s, k % len(srcs[s]._ring))
            if key not in cache:
                f = srcs[s]._ring[k % len(srcs[s]._ring)]
                cache[key] = _logits_of(ref_plan, [(f.y.cpu().numpy(), f.uv.cpu().numpy())], (640, 360))[0]
            v = cache[key]
            top = Q.top(v, 3)
            want = otr.update(s, np.tile([0.0, 0.0, 640.0, 360.0], (3, 1)), v[top].astype(np.float64), top.astype(np.int64))
            assert orc.table_of(tables[s]) == orc.table_of(want), (engine, depth, k, s)
            out.append(orc.table_of(tables[s]))

    if depth == 0:
        for k in range(T):
            pipe.tick()
            check(k, trk.device_tracker.read_all())
    else:
        runner = PipelinedTicks(pipe, depth=depth)
        assert not runner.use_graph and runner.depth == depth
        done = 0
        for k in range(T):
            if k - done == runner.depth:
                check(done, runner.collect()[1]); done += 1
            runner.submit()
        while done < T:
            check(done, runner.collect()[1]); done += 1
    assert all(type(rs.plan) is FusedResNet18F16 and rs.input.dtype == torch.float16 for rs in det._slots.values()) and det._slots
    return out


def test_tick_runners_against_the_oracle():
    t0, t1, t4 = _run_ticks("plan", 0), _run_ticks("plan", 1), _run_ticks("plan", 4)
    assert t0 == t1 == t4 and all(len(t) == 3 for t in t0)
    assert _run_ticks("native", 1) == t0


def test_mixed_geometries_form_two_groups():
    streams_a, srcs_a = _sources(2)
    streams_b = [StreamConfig(name=f"small{i}", url="synthetic://320x240", warmup_seconds=0.0) for i in range(2)]
    srcs_b = [SyntheticNv12Stream(s, index=5 + i, width=320, height=240, n_unique=2) for i, s in enumerate(streams_b)]
    for s in srcs_b:
        s.open_sync()
    net = _net()
    det = HipResNetDetector(_dcfg(), net=copy.deepcopy(net))
    trk = IouTracker(TrackerConfig(max_age=30, max_iou_distance=0.5, min_hits=1), max_streams=4, capacity=64)
    streams, srcs = streams_a + streams_b, srcs_a + srcs_b
    pipe = TickPipeline(streams, det, trk, sources=srcs)
    packets = [FramePacket(st, src._ring[0], 0, 0.0) for st, src in zip(streams, srcs)]
    plan = pipe.plan_tick(packets)
    assert [len(g.idx) for g in plan.groups] == [2, 2] and not plan.host_idx
    pipe.tick()
    tables = trk.device_tracker.read_all()
    want = HipResNetDetector(_dcfg(), net=copy.deepcopy(net)).predict_batch(packets)
    for i, (st, dets) in enumerate(zip(streams, want)):
        t = tables[pipe.slots[i]]
        assert sorted(int(c) for c in t["cls"]) == sorted(d.class_id for d in dets) and t["n"] == 3
        w, h = (640, 360) if i < 2 else (320, 240)
        assert all([float(v) for v in b] == [0.0, 0.0, float(w), float(h)] for b in t["boxes"])
